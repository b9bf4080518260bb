// pem_sobol_design.h -- the design of the Sobol' study over a pressure sweep: the QoI groups, the inputs each varies, the stream
// numbering and one row of the counter-based design.  Shared by the launch around the model (pem_sobol_sweep.hip) and the launch
// around the chained surrogate (pem_surrogate_sobol.hip), so that both see the same rows for the same seed.  Everything is local
// to the including unit (each has its own BLOCK and its own kernels).
#pragma once
#include <hip/hip_runtime.h>

#include "pem_hip.h"
#include "pem_philox.h"

namespace {

constexpr int NIN = 15;       // P_b V_a T_e V_vac Pstar P_T mdot_a a_1 c0..c5 sigma_cex
constexpr int NGROUP = 3;     // PEM_SWEEP_CATHODE, PEM_SWEEP_THRUSTER, PEM_SWEEP_PLUME

// the varied inputs of each group, in the order of their partial rows (include/pem_hip.h)
__host__ __device__ constexpr int n_varied(int g) { return g == PEM_SWEEP_CATHODE ? 5 : g == PEM_SWEEP_THRUSTER ? 4 : 8; }
__host__ __device__ constexpr int n_qoi(int g) { return g == PEM_SWEEP_THRUSTER ? 2 : 1; }
__host__ __device__ constexpr int varied_input(int g, int j) {
    return g == PEM_SWEEP_CATHODE    ? (j == 0 ? 0 : j + 1)                                     // P_b T_e V_vac Pstar P_T
           : g == PEM_SWEEP_THRUSTER ? (j == 0 ? 0 : j == 1 ? 6 : j == 2 ? 2 : 7)               // P_b mdot_a T_e a_1
                                     : (j == 0 ? 0 : j + 7);                                   // P_b c0..c5 sigma_cex
}
__host__ __device__ constexpr bool is_varied(int g, int c) {
    for (int j = 0; j < n_varied(g); ++j)
        if (varied_input(g, j) == c) return true;
    return false;
}

__device__ __attribute__((noinline)) double transform_call(int kind, double a, double b, double u) { return pem::transform(kind, a, b, u); }

// stream of attempt k of row r (0: A, 1: B) of group g at pressure p: 2 G P k + 2 (g P + p) + r
__device__ __forceinline__ unsigned int row_stream(int g, int n_p, int p, int k, int r) {
    return 2u * NGROUP * (unsigned)n_p * (unsigned)k + 2u * (unsigned)(g * n_p + p) + (unsigned)r;
}

// one row of the design: the group's varied inputs from stream `st` (bit-identical to pem_sample_f64_dev for the same
// kind/a/b table), every other input at its pin a[c].  Philox blocks whose two inputs are both pinned are not computed.
template <int G>
__device__ __forceinline__ void design_row(unsigned long long seed, const int* kind, const double* a, const double* b,
                                           unsigned long long i, unsigned int st, double (&x)[NIN]) {
    const unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll
    for (int pair = 0; pair < 8; ++pair) {
        const int c0 = 2 * pair, c1 = 2 * pair + 1;
        const bool v0 = is_varied(G, c0), v1 = c1 < NIN && is_varied(G, c1);
        if (v0 || v1) {
            const pem::Philox4 r = pem::philox4x32_10((unsigned int)i, (unsigned int)(i >> 32), (unsigned int)pair, st, k0, k1);
            if (v0) x[c0] = transform_call(__builtin_amdgcn_readfirstlane(kind[c0]), a[c0], b[c0], pem::u53(r.x, r.y));
            if (v1) x[c1] = transform_call(__builtin_amdgcn_readfirstlane(kind[c1]), a[c1], b[c1], pem::u53(r.z, r.w));
        }
        if (!v0) x[c0] = a[c0];
        if (c1 < NIN && !v1) x[c1] = a[c1];
    }
}

}  // namespace
