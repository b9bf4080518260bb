// pem_saltelli_model.h -- what the fused Saltelli launches share (pem_saltelli.hip: first-order and total sums; pem_saltelli2.hip:
// the second-order extension): the launch argument, the two lane-per-sample models and the rows of the design.  Everything sits in
// an anonymous namespace: each translation unit that includes this header compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_model.h"
#include "pem_model_f32.h"
#include "pem_philox.h"
#include "pem_qmc.h"
#include "pem_wave.h"

namespace {

constexpr int NIN = 15;   // P_b V_a T_e V_vac Pstar P_T mdot_a a_1 c0..c5 sigma_cex
constexpr int NQ = 3;     // V_cc, div_angle, T_c

struct SaltelliArg {
    unsigned long long seed, first;
    unsigned int stream;
    int nv;                  // varied inputs
    int varied[NIN];         // their indices (0..14)
    int kind[NIN];
    double a[NIN], b[NIN];
};

struct Eval {                // what the estimator needs from one evaluation
    double f[NQ];
    bool bad_thruster, invalid;
};

// ---- the two models -------------------------------------------------------------------------------------------------
struct Model32 {
    using real = float;
    static constexpr int LDS_BYTES = pem_model32::LDS_FLOATS * 4;
    static constexpr int QMC_WAVES = 4;          // waves per SIMD saltelli_qmc_kernel is compiled for
    pem_model32::Tab32 t;
    float k, rad, inv_r2, inv_2pi_r2;
    __device__ void stage(void* lds, int tid, int nthreads, double torr2pa, double radius) {
        t = pem_model32::stage_tables(static_cast<float*>(lds), tid, nthreads);
        k = (float)torr2pa;
        rad = (float)radius;
        inv_r2 = 1.0f / (rad * rad);
        inv_2pi_r2 = 1.0f / (2.0f * pem_model32::F_PI * (rad * rad));
    }
    __device__ __forceinline__ Eval eval(const float (&x)[NIN]) const {
        const pem_model32::Qoi32 o = pem_model32::coupled_f32(x, k, rad, inv_r2, inv_2pi_r2, t);
        return Eval{{(double)o.V_cc, (double)o.div, (double)o.T_c}, o.T < 0.0f || o.I_B0 < 0.0f, o.invalid};
    }
};

// the reference's literal 91-term sums (plume.py:99-123) for a sample outside the tabulated range.  Out of line: never taken
// under the PEM-v0 priors, and inlined its two exp() bodies cost the rolled evaluation loop registers it does not have
struct LiteralSums {
    double den, num, lo;
};
__device__ __attribute__((noinline)) LiteralSums literal_sums(const double2* simpson, double X1a, double X2a, double j_cex, double a1, double a2) {
#pragma clang fp contract(off)
    using namespace pem_model;
    double dd = 0.0, nn = 0.0, lo = __builtin_inf();
    for (int kk = 0; kk < NANG; ++kk) {
        const double alpha = kk == NANG - 1 ? HALF_PI : (double)kk * GRID_H;
        const double t1 = alpha / a1, t2 = alpha / a2;
        const double f = X1a * exp(-(t1 * t1)) + X2a * exp(-(t2 * t2));
        lo = fmin(lo, f + j_cex);
        dd = __builtin_fma(simpson[kk].x, f, dd);
        nn = __builtin_fma(simpson[kk].y, f, nn);
    }
    return LiteralSums{dd, nn, lo};
}

struct Model64 {
    using real = double;
    static constexpr int QPOLY_DOUBLES = (PEM_NDI + PEM_NQB) * PEM_NDC * 2;
    static constexpr int LDS_BYTES = (PEM_NDI * PEM_NDC + QPOLY_DOUBLES + 2 * 96) * 8;
    static constexpr int QMC_WAVES = 2;
    const double* dpoly;
    const double2* qpoly;
    const double2* simpson;
    double k, rad, inv_r2, inv_2pi_r2;
    __device__ void stage(void* lds, int tid, int nthreads, double torr2pa, double radius) {
        double* d = static_cast<double*>(lds);
        double* q = d + PEM_NDI * PEM_NDC;
        double* s = q + QPOLY_DOUBLES;
        for (int i = tid; i < PEM_NDI * PEM_NDC; i += nthreads) d[i] = PEM_DPOLY[i];
        for (int i = tid; i < QPOLY_DOUBLES; i += nthreads) q[i] = PEM_QPOLY[i];
        for (int i = tid; i < 96; i += nthreads) {
            s[2 * i] = i < PEM_NANGLE ? PEM_SIMPSON_CDEN[i] : 0.0;
            s[2 * i + 1] = i < PEM_NANGLE ? PEM_SIMPSON_CNUM[i] : 0.0;
        }
        dpoly = d;
        qpoly = reinterpret_cast<const double2*>(q);
        simpson = reinterpret_cast<const double2*>(s);
        k = torr2pa;
        rad = radius;
        inv_r2 = 1.0 / (rad * rad);
        inv_2pi_r2 = 1.0 / (2.0 * pem_model::PEM_PI * (rad * rad));
    }
    // cathode.py:24-38 -> tests/sim_hallthruster.jl:35-48 -> plume.py:39-140, reduced QoIs.  The plain branch is, operation
    // for operation, process_tile<..., JMODE 0> of pem_kernels.hip; the other branch is the reference's literal sums.
    __device__ __forceinline__ Eval eval(const double (&x)[NIN]) const {
        using namespace pem_model;
        const double V_cc = cathode_vcc(x[0], x[1], x[2], x[3], x[4], x[5], k);
        const ThrusterQoI th = thruster_stage(x[1], V_cc, x[6], x[7]);
        const PlumeSetup ps = plume_setup(x[0], x[9], x[10], x[11], x[12], x[13], k);
        const double a1 = ps.a1, a2 = ps.a2;
        const double u1 = 1.0 / (a1 * a1), u2 = 1.0 / (a2 * a2);
        const double A1 = (1.0 - x[8]) / normaliser(a1, u1, dpoly);
        const double A2 = x[8] / normaliser(a2, u2, dpoly);
        const double decay = exp(-rad * ps.n_neutral * x[14]);
        const double j_cex = th.I_B0 * (1.0 - decay) * inv_2pi_r2;
        const double base = th.I_B0 * decay * inv_r2;
        const double X1a = base * A1, X2a = base * A2;
        const bool plain = fabs(a1) >= PEM_QA_MIN && fabs(a2) >= PEM_QA_MIN && X1a >= 0.0 && X2a >= 0.0 && j_cex > 0.0 &&
                           (fmax(X1a, X2a) >= 1e-280 || (X1a == 0.0 && X2a == 0.0));
        double d1, n1, d2, n2;
        simpson_functionals(qpoly, fabs(a1), u1, d1, n1);
        simpson_functionals(qpoly, fabs(a2), u2, d2, n2);
        double den = fma(base * A1, d1, (base * A2) * d2), num = fma(base * A1, n1, (base * A2) * n2);
        bool invalid = a1 <= 0.0;
        if (!plain) {
            const LiteralSums ls = literal_sums(simpson, X1a, X2a, j_cex, a1, a2);
            den = ls.den;
            num = ls.num;
            invalid = invalid || ls.lo <= 0.0;
        }
        double cos_div = num / den;
        if (cos_div == __builtin_inf()) cos_div = __builtin_nan("");
        return Eval{{V_cc, acos(cos_div), th.T * cos_div}, th.T < 0.0 || th.I_B0 < 0.0, invalid};
    }
};

// ---- the design -----------------------------------------------------------------------------------------------------
__device__ __attribute__((noinline)) double transform_call_s(int kind, double a, double b, double u) {
    return pem::transform(kind, a, b, u);
}

// one row of the design (stream `st`) for global base sample g: bit-identical to pem_sample_f64_dev (then rounded to the
// model's real type)
template <class real>
__device__ __forceinline__ void design_row(const SaltelliArg& s, const int* lds_kind, const double* lds_ab, unsigned long long g,
                                           unsigned int st, real (&x)[NIN]) {
    const unsigned int k0 = (unsigned int)s.seed, k1 = (unsigned int)(s.seed >> 32);
    double u[16];
#pragma unroll
    for (int pair = 0; pair < 8; ++pair) {
        const pem::Philox4 r = pem::philox4x32_10((unsigned int)g, (unsigned int)(g >> 32), (unsigned int)pair, st, k0, k1);
        u[2 * pair] = pem::u53(r.x, r.y);
        u[2 * pair + 1] = pem::u53(r.z, r.w);
    }
#pragma unroll
    for (int d = 0; d < NIN; ++d) {
        const int kd = __builtin_amdgcn_readfirstlane(lds_kind[d]);      // wave-uniform: a scalar branch inside
        x[d] = (real)transform_call_s(kd, lds_ab[2 * d], lds_ab[2 * d + 1], u[d]);
    }
}

// the same row from the shifted Sobol' sequence (csrc/pem_qmc.h): input c is sequence dimension `dim0` + c (row A: 0, row B: NIN),
// bit-identical to pem_sample_sobol_f64_dev.  `gray_lane`: the Gray code of the lane's index; `wave_part`: lane l < 2 NIN holds the
// fold of the wave's upper Gray-code bits for sequence dimension l, and its shift (pem::qmc_wave_part)
template <class real>
__device__ __forceinline__ void design_row_qmc(const int* lds_kind, const double* lds_ab, unsigned int gray_lane, unsigned int wave_part,
                                               int dim0, real (&x)[NIN]) {
#pragma unroll
    for (int d = 0; d < NIN; ++d) {
        const int kd = __builtin_amdgcn_readfirstlane(lds_kind[d]);
        const unsigned int p = __builtin_amdgcn_readlane(wave_part, dim0 + d) ^ pem::qmc_lane_part(gray_lane, dim0 + d);
        x[d] = (real)transform_call_s(kd, lds_ab[2 * d], lds_ab[2 * d + 1], pem::qmc_uniform(p));
    }
}

struct QmcShifts {           // the digital shift of each of the 2 NIN sequence dimensions (zeros: the unshifted sequence)
    unsigned int s[2 * NIN];
};

}  // namespace
