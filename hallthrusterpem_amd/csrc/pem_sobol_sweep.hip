// pem_sobol_sweep.hip -- the Sobol' study of scripts/pem_v0/sobol.py:46-118 over a sweep of background pressures (gfx950).
//
// The reference varies, per QoI, only the exogenous inputs of the component that produces it (IDX_MAP, sobol.py:24-29) and pins
// the rest at their nominal values (sobol.py:73-80); it repeats the design at five pressures.  One launch here covers one such
// group at EVERY pressure of the sweep: blockIdx.y is the pressure, and each workgroup stages that pressure's prior table.
// Per base sample a lane generates rows A and B of the counter-based design (the numbers of pem_sample_f64_dev), evaluates
// the group's own stage -- never the whole coupled model -- on A, B and, in a rolled loop, on A with column j from B, and adds
// the estimator terms to per-wave fp64 accumulators through the transposing wave reduction of pem_wave.h.  Only one partial
// per workgroup reaches HBM.  The groups are template instantiations, so each carries only its own stage:
//   Cathode   V_cc                      cathode.py:24-38
//   Thruster  T, u_ion at one grid node cathode -> tests/sim_hallthruster.jl:35-48 (the thruster test double)
//   Plume     j_ion at gamma = 0        plume.py:39-106 alone, I_B0 and r given; spike rejection and a clip (sobol.py:50-66, 82-89)
// The fp64 arithmetic is the coupled kernels' (csrc/pem_model.h) and the CPU oracle's, operation for operation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_model.h"
#include "pem_philox.h"
#include "pem_sobol_design.h"
#include "pem_wave.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NFLAG = 4;

struct SweepArg {
    unsigned long long seed, first;
    long long n;
    int n_p, max_attempts;
    double torr2pa, radius, i_b0, uion_den, spike;
};

struct PlumeJ {
    double j0;            // j_ion at gamma = 0 (1e-20 for an invalid sample, plume.py:106)
    bool hit, invalid;    // some j_ion on the 91-angle grid >= the spike threshold; plume.py:105
};

// j_ion on the whole 91-angle grid (plume.py:99-105) for a sample whose maximum need not be at gamma = 0: a beam amplitude
// that is negative or NaN, or a CEX term that is not positive.  Returns bit 0: some j >= thr, bit 1: some j <= 0.  Never taken
// under the PEM-v0 priors, yet inline and rolled: out of line, the call's saved registers put the Plume instantiation into scratch.
__device__ __forceinline__ int literal_j(double X1a, double X2a, double j_cex, double a1, double a2, double thr) {
#pragma clang fp contract(off)
    using namespace pem_model;
    bool hit = false, nonpos = false;
#pragma nounroll
    for (int kk = 0; kk < NANG; ++kk) {
        const double alpha = kk == NANG - 1 ? HALF_PI : (double)kk * GRID_H;
        const double t1 = alpha / a1, t2 = alpha / a2;
        const double j = X1a * exp(-(t1 * t1)) + X2a * exp(-(t2 * t2)) + j_cex;
        hit = hit || j >= thr;
        nonpos = nonpos || j <= 0.0;
    }
    return (int)hit | (int)nonpos << 1;
}

// plume.py:39-106 at one radius with a given I_B0, reduced to j_ion(gamma = 0) and the spike test.  With both beam amplitudes
// non-negative and j_cex > 0 every j_ion(gamma) is X1a g1 + X2a g2 + j_cex with g1, g2 = exp(-(.)^2) <= 1, so (rounding being
// monotone) the profile's maximum is j(0) = X1a + X2a + j_cex; any other sample is tested on the whole grid.
__device__ __forceinline__ PlumeJ plume_j(const double (&x)[NIN], const SweepArg& s, const double* dpoly) {
#pragma clang fp contract(off)
    using namespace pem_model;
    const PlumeSetup ps = plume_setup(x[0], x[9], x[10], x[11], x[12], x[13], s.torr2pa);
    const double a1 = ps.a1, a2 = ps.a2;
    const double A1 = (1.0 - x[8]) / normaliser(a1, 1.0 / (a1 * a1), dpoly);
    const double A2 = x[8] / normaliser(a2, 1.0 / (a2 * a2), dpoly);
    const double rad = s.radius;
    const double decay = exp(-rad * ps.n_neutral * x[14]);
    const double j_cex = s.i_b0 * (1.0 - decay) / (2.0 * PEM_PI * (rad * rad));
    const double base = s.i_b0 * decay / (rad * rad);
    const double X1a = base * A1, X2a = base * A2;
    PlumeJ o;
    o.j0 = X1a + X2a + j_cex;
    o.invalid = a1 <= 0.0;
    if (X1a >= 0.0 && X2a >= 0.0 && j_cex > 0.0) {
        o.hit = o.j0 >= s.spike;
    } else {
        const int l = literal_j(X1a, X2a, j_cex, a1, a2, s.spike);
        o.hit = l & 1;
        o.invalid = o.invalid || (l & 2);
    }
    if (o.invalid) {
        o.j0 = 1e-20;
        o.hit = false;
    }
    return o;
}

// one evaluation of the group's stage: its QoIs, the thruster filter, and for the Plume group the spike test and plume.py:105
struct Eval {
    double f[2];
    bool bad_thruster, invalid, hit;
};
template <int G>
__device__ __forceinline__ Eval eval_stage(const double (&x)[NIN], const SweepArg& s, double uion_den, const double* dpoly) {
    using namespace pem_model;
    if constexpr (G == PEM_SWEEP_PLUME) {
        const PlumeJ o = plume_j(x, s, dpoly);
        return Eval{{o.j0, 0.0}, false, o.invalid, o.hit};
    } else {
        const double V_cc = cathode_vcc(x[0], x[1], x[2], x[3], x[4], x[5], s.torr2pa);
        if constexpr (G == PEM_SWEEP_CATHODE) {
            return Eval{{V_cc, 0.0}, false, false, false};
        } else {
            const ThrusterQoI th = thruster_stage(x[1], V_cc, x[6], x[7]);
            return Eval{{th.T, th.v_exh / uion_den}, th.T < 0.0 || th.I_B0 < 0.0, false, false};
        }
    }
}

__device__ __forceinline__ double clip_to(double j, double thr) { return j > thr ? thr : j; }   // NaN stays NaN, as numpy's mask

// partial: [n_p][gridDim.x][2 + 4 NV][NQ]; flags: [n_p][gridDim.x][4]; j0_out (Plume pre-pass): [n_p][2 n]
// Two waves per SIMD: the Plume instantiation takes 256 registers, the other two about 120.
template <int G>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2)))
void sobol_sweep_kernel(SweepArg s, const int* __restrict__ kind_t, const double* __restrict__ a_t, const double* __restrict__ b_t,
                        const double* __restrict__ clip, double* __restrict__ j0_out, double* __restrict__ partial,
                        uint64_t* __restrict__ flags) {
    constexpr int NV = n_varied(G), NQ = n_qoi(G), ROWS = 2 + 4 * NV;
    constexpr bool PLUME = G == PEM_SWEEP_PLUME;
    __shared__ int lds_kind[NIN];
    __shared__ double lds_a[NIN], lds_b[NIN];
    __shared__ double lds_poly[PLUME ? PEM_NDI * PEM_NDC : 1];
    __shared__ double acc[4][NV + 1][8];      // [wave][0: the A/B statistics, 1 + j: varied input j][value]
    __shared__ double cnt[4][NFLAG];
    const int p = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < NIN) {
        lds_kind[threadIdx.x] = kind_t[p * NIN + threadIdx.x];
        lds_a[threadIdx.x] = a_t[p * NIN + threadIdx.x];
        lds_b[threadIdx.x] = b_t[p * NIN + threadIdx.x];
    }
    if constexpr (PLUME)
        for (int i = threadIdx.x; i < PEM_NDI * PEM_NDC; i += BLOCK) lds_poly[i] = PEM_DPOLY[i];
    for (int i = threadIdx.x; i < 4 * (NV + 1) * 8; i += BLOCK) (&acc[0][0][0])[i] = 0.0;
    __syncthreads();
    const double thr = PLUME && clip ? clip[p] : __builtin_inf();
    const double uion_den = s.uion_den;
    const int my_slot = pem::wave_sum8_slot(lane);
    unsigned int bad_thruster = 0, bad_plume = 0, rejected = 0, unaccepted = 0;
    // every wave runs the same number of iterations (the reductions need all 64 lanes): lanes past n evaluate the last
    // sample and contribute zeros
    const long long n = s.n;
    const long long stride = (long long)gridDim.x * BLOCK;
    const long long iters = (n + stride - 1) / stride;
    for (long long it = 0; it < iters; ++it) {
        const long long i = it * stride + (long long)blockIdx.x * BLOCK + threadIdx.x;
        const bool live = i < n;
        const unsigned long long g = s.first + (unsigned long long)(live ? i : n - 1);
        double xa[NIN], xb[NIN], fa[2], fb[2];
        // ONE model body, a rolled loop over the evaluations of a base sample: 0 = row A, 1 = row B (each redrawn until
        // accepted in the Plume group), 2 + j = A with column varied_input(j) from B
        for (int e = 0; e < NV + 2; ++e) {
            const int d = e >= 2 ? varied_input(G, e - 2) : -1;
            double x[NIN];
            Eval o;
            for (int k = 0;;) {
                if (e < 2) {
                    design_row<G>(s.seed, lds_kind, lds_a, lds_b, g, row_stream(G, s.n_p, p, k, e), x);
                } else {
#pragma unroll
                    for (int c = 0; c < NIN; ++c) x[c] = !is_varied(G, c) ? lds_a[c] : c == d ? xb[c] : xa[c];
                }
                o = eval_stage<G>(x, s, uion_den, lds_poly);
                if (!PLUME || e >= 2 || !o.hit) break;
                if (live) ++rejected;
                if (++k == s.max_attempts) {             // never accepted: reported, the last draw is kept
                    if (live) ++unaccepted;
                    break;
                }
            }
            if (live) {
                bad_thruster += o.bad_thruster;
                bad_plume += o.invalid;
            }
            if (e < 2) {
                if (PLUME && j0_out && live) j0_out[(size_t)p * 2 * n + (size_t)e * n + i] = o.f[0];   // the pre-pass: unclipped
#pragma unroll
                for (int c = 0; c < NIN; ++c) {      // the varied columns only: the pins are read from LDS where they are used
                    if (!is_varied(G, c)) continue;
                    xa[c] = e == 0 ? x[c] : xa[c];
                    xb[c] = e == 1 ? x[c] : xb[c];
                }
            }
            double f[2] = {PLUME ? clip_to(o.f[0], thr) : o.f[0], o.f[1]};
            if (e == 0) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) fa[q] = f[q];
                continue;
            }
            if (PLUME && j0_out) {
                if (e == 1) break;                       // the pre-pass forms no sums
                continue;
            }
            double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (e == 1) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    fb[q] = f[q];
                    v[q] = fa[q] + f[q];
                    v[NQ + q] = fma(fa[q], fa[q], f[q] * f[q]);
                }
            } else {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const double t1 = fb[q] * (f[q] - fa[q]), t2 = (fa[q] - f[q]) * (fa[q] - f[q]);
                    v[q] = t1;
                    v[NQ + q] = t1 * t1;
                    v[2 * NQ + q] = t2;
                    v[3 * NQ + q] = t2 * t2;
                }
            }
            if (!live) {
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = 0.0;
            }
            const double tot = pem::wave_sum8(v, lane);
            if (lane < 8) acc[wave][e - 1][my_slot] += tot;
        }
    }
    {
        double v[8] = {(double)bad_thruster, (double)bad_plume, (double)rejected, (double)unaccepted, 0, 0, 0, 0};
        const double tot = pem::wave_sum8(v, lane);
        if (lane < 8 && my_slot < NFLAG) cnt[wave][my_slot] = tot;
    }
    __syncthreads();
    // one partial per workgroup, in a fixed order (deterministic).  Row 0, 1 <- acc[.][0][{0, 1} NQ + q];
    // row 2 + 4 j + w <- acc[.][1 + j][w NQ + q]
    const size_t blk = (size_t)p * gridDim.x + blockIdx.x;
    if (!j0_out && (int)threadIdx.x < ROWS * NQ) {
        const int row = threadIdx.x / NQ, q = threadIdx.x - row * NQ;
        const int e = row < 2 ? 0 : 1 + (row - 2) / 4, w = row < 2 ? row : (row - 2) % 4;
        partial[blk * ROWS * NQ + threadIdx.x] =
            acc[0][e][w * NQ + q] + acc[1][e][w * NQ + q] + acc[2][e][w * NQ + q] + acc[3][e][w * NQ + q];
    }
    if (threadIdx.x < NFLAG)
        flags[blk * NFLAG + threadIdx.x] =
            (uint64_t)cnt[0][threadIdx.x] + (uint64_t)cnt[1][threadIdx.x] + (uint64_t)cnt[2][threadIdx.x] + (uint64_t)cnt[3][threadIdx.x];
}

template <int G>
void launch(dim3 grid, hipStream_t st, const SweepArg& s, const int32_t* kind, const double* a, const double* b, const double* clip,
            double* j0_out, double* partial, uint64_t* flags) {
    hipLaunchKernelGGL(sobol_sweep_kernel<G>, grid, dim3(BLOCK), 0, st, s, kind, a, b, clip, j0_out, partial, flags);
}

}  // namespace

extern "C" int pem_sobol_sweep_f64_dev(int group, size_t n_base, uint64_t first_index, uint64_t seed, int n_p, const int32_t* kind,
                                       const double* a, const double* b, double torr2pa, double radius, double i_b0, double uion_z,
                                       double spike_threshold, int max_attempts, const double* clip, double* j0_out, double* partial,
                                       uint64_t* flags, int n_blocks, pem_stream_t stream) {
    const char* who = "pem_sobol_sweep_f64";
    if (group < PEM_SWEEP_CATHODE || group > PEM_SWEEP_PLUME) return pem::fail(PEM_ERR_INVALID_ARG, "%s: unknown group %d", who, group);
    if (n_p < 1 || n_p > PEM_SWEEP_MAX_PRESSURES)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 <= n_p <= %d pressures, got %d", who, PEM_SWEEP_MAX_PRESSURES, n_p);
    if (n_blocks < 1) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_blocks must be positive", who);
    if (n_base < 1 || n_base > (size_t)1 << 40) return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 <= n_base <= 2^40", who);
    if (!kind || !a || !b || !flags) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    const bool plume = group == PEM_SWEEP_PLUME;
    if (j0_out && !plume) return pem::fail(PEM_ERR_INVALID_ARG, "%s: the j0 pre-pass exists for the Plume group only", who);
    if (!j0_out && !partial) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL partial", who);
    if (plume && (max_attempts < 1 || (uint64_t)2 * NGROUP * (uint64_t)n_p * (uint64_t)max_attempts > 0xFFFFFFFFull))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: max_attempts must be >= 1 and 6 n_p max_attempts < 2^32", who);
    if (int rc = pem::check_device()) return rc;
    SweepArg s{};
    s.seed = seed;
    s.first = first_index;
    s.n = (long long)n_base;
    s.n_p = n_p;
    s.max_attempts = plume ? max_attempts : 1;
    s.torr2pa = torr2pa;
    s.radius = radius;
    s.i_b0 = i_b0;
    // u_ion at the node z (sim_hallthruster.jl:46-47) is v_exh / (1 + exp(-100 (z - 0.04))): the denominator is formed here, by
    // the host's libm as the reference's numpy does, not by the device exp (one ulp apart at times, which the estimator's
    // differences f(AB) - f(A) of a QoI with little variance turn into 1e-8 of an index)
    s.uion_den = 1.0 + std::exp(-100.0 * (uion_z - 0.04));
    s.spike = spike_threshold;
    const dim3 grid((unsigned)n_blocks, (unsigned)n_p);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (group == PEM_SWEEP_CATHODE) launch<PEM_SWEEP_CATHODE>(grid, st, s, kind, a, b, clip, j0_out, partial, flags);
    else if (group == PEM_SWEEP_THRUSTER) launch<PEM_SWEEP_THRUSTER>(grid, st, s, kind, a, b, clip, j0_out, partial, flags);
    else launch<PEM_SWEEP_PLUME>(grid, st, s, kind, a, b, clip, j0_out, partial, flags);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
