// pem_surrogate.hip -- batched prediction of a sparse-grid (Smolyak / combination-technique) Lagrange surrogate.
//
// What it stands in for: the surrogate evaluations inside `System.fit(num_refine=1000, ...)` / `System.predict`
// that scripts/fit_surr.py:101-116 and scripts/pem_v0/{monte_carlo,sobol,mcmc}.py drive (BASELINE.json configs[3]:
// "batched tensor-interpolant predict").  The interpolant lives in amisc (third-party, absent): parity UNPINNED.
// Stated formula (hallthrusterpem_amd/surrogate.py builds the tables):
//     f(t) = sum_beta c_beta * sum_{j} Y_beta[j] * prod_{d active in beta} l^{(level_d)}_{j_d}(t_d),   t in [-1, 1]^D
// level 0 has the single node 0 (basis 1); level l >= 1 has m = 2^l + 1 Chebyshev-Lobatto nodes t_j = -cos(pi j/(m-1))
// with barycentric weights (-1)^j (halved at both ends).  Each multi-index beta has at most PEM_SURR_MAX_ACTIVE = 5 active
// dimensions of level <= PEM_SURR_MAX_LEVEL = 4 (round 4; rounds 1-3: 3 and 3).
//
// Shape of the work: per point, sum over the grids of the combination -- K = prod(m) <= 729 products against n_out <= 16
// columns.  It is not a dense GEMM worth MFMA: the "A matrix" (basis products) is generated on the fly per point, n_out
// is skinny (3 pads to 16 columns on the 16x16x4 tile) and the fp64 matrix pipe shares its units with the VALU
// (DESIGN.md section 4.5).  One lane per point; everything about the grid -- its index entry, the node values -- is
// wave-uniform and comes through the scalar cache.
//
// Round 2 rewrite (357 -> see DESIGN.md section 4.7): the first version was latency-bound, not arithmetic-bound -- 22 cycles
// per instruction at two waves per SIMD: one scalar load + one LDS read + a wait per NODE, the point's coordinate re-read
// from global memory per grid and dimension, and m + 1 IEEE divisions per barycentric basis.  Now
//   * the Lagrange bases are taken in product form, l_j(t) = c_j prod_{i != j} (t - t_i) by prefix/suffix products:
//     4 m multiplies, no division, no special case at the nodes;
//   * the point's coordinates are staged in LDS once;
//   * the innermost active dimension of a grid stays in registers and its loop is unrolled (m is 1, 3, 5 or 9): one batch
//     of scalar loads and one wait per ROW of the grid instead of per node, and the row is contracted first
//     (sum-factorisation: n_out FMAs per node, the outer basis product is applied once per row);
//   * only the two outer dimensions' bases go through LDS: 36 KB + coordinates per workgroup instead of 55 KB.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAXA = PEM_SURR_MAX_ACTIVE;    // active dimensions per multi-index
constexpr int MAXO = MAXA - 1;                // of which all but the innermost go through LDS
constexpr int MAXM = 17;                      // nodes at level 4
constexpr int IDX_STRIDE = 2 + 2 * MAXA;      // per beta: n_active, value offset, dims[MAXA], levels[MAXA]
static_assert(MAXA == 5 && PEM_SURR_MAX_LEVEL == 4, "the kernel nests four outer dimensions around the unrolled innermost one; tables up to level 4");

__device__ __forceinline__ int nodes_of(int level) { return level == 0 ? 1 : (1 << level) + 1; }

// Chebyshev-Lobatto nodes of levels 1..4, concatenated (offsets 0, 3, 8, 17): the CORRECTLY ROUNDED doubles of -cos(pi j / (m - 1)),
// the same doubles as surrogate.nodes() that the model is evaluated at (so that the interpolant goes through its training values
// exactly).  Correct rounding makes them nested across levels and antisymmetric.  And the Lagrange denominators
// c_j = 1 / prod_{i != j} (t_j - t_i) OF THESE DOUBLES (exact rational arithmetic, then rounded to nearest).
// tests/test_surrogate_nodes.py parses both tables and checks them.
__device__ const double LOBATTO_NODES[34] = {
    -0x1.0000000000000p+0, 0.0, 0x1.0000000000000p+0,
    -0x1.0000000000000p+0, -0x1.6a09e667f3bcdp-1, 0.0, 0x1.6a09e667f3bcdp-1, 0x1.0000000000000p+0,
    -0x1.0000000000000p+0, -0x1.d906bcf328d46p-1, -0x1.6a09e667f3bcdp-1, -0x1.87de2a6aea963p-2, 0.0,
    0x1.87de2a6aea963p-2, 0x1.6a09e667f3bcdp-1, 0x1.d906bcf328d46p-1, 0x1.0000000000000p+0,
    -0x1.0000000000000p+0, -0x1.f6297cff75cb0p-1, -0x1.d906bcf328d46p-1, -0x1.a9b66290ea1a3p-1, -0x1.6a09e667f3bcdp-1,
    -0x1.1c73b39ae68c8p-1, -0x1.87de2a6aea963p-2, -0x1.8f8b83c69a60bp-3, 0.0, 0x1.8f8b83c69a60bp-3, 0x1.87de2a6aea963p-2,
    0x1.1c73b39ae68c8p-1, 0x1.6a09e667f3bcdp-1, 0x1.a9b66290ea1a3p-1, 0x1.d906bcf328d46p-1, 0x1.f6297cff75cb0p-1,
    0x1.0000000000000p+0};
__device__ const double LOBATTO_INVDEN[34] = {
    0x1.0000000000000p-1, -0x1.0000000000000p+0, 0x1.0000000000000p-1,
    0x1.0000000000001p+0, -0x1.0000000000000p+1, 0x1.fffffffffffffp+0, -0x1.0000000000000p+1, 0x1.0000000000001p+0,
    0x1.fffffffffffffp+2, -0x1.0000000000001p+4, 0x1.0000000000001p+4, -0x1.fffffffffffffp+3, 0x1.fffffffffffffp+3,
    -0x1.fffffffffffffp+3, 0x1.0000000000001p+4, -0x1.0000000000001p+4, 0x1.fffffffffffffp+2,
    0x1.ffffffffffff6p+9, -0x1.ffffffffffffcp+10, 0x1.0000000000002p+11, -0x1.0000000000003p+11, 0x1.fffffffffffffp+10,
    -0x1.fffffffffffffp+10, 0x1.0000000000001p+11, -0x1.0000000000000p+11, 0x1.0000000000000p+11, -0x1.0000000000000p+11,
    0x1.0000000000001p+11, -0x1.fffffffffffffp+10, 0x1.fffffffffffffp+10, -0x1.0000000000003p+11, 0x1.0000000000002p+11,
    -0x1.ffffffffffffcp+10, 0x1.ffffffffffff6p+9};

// Lagrange basis of the M Chebyshev-Lobatto nodes at t, product form
template <int M>
__device__ __forceinline__ void lobatto_basis(double t, double (&b)[M]) {
    if constexpr (M == 1) {
        b[0] = 1.0;
    } else {
        constexpr int off = M == 3 ? 0 : (M == 5 ? 3 : (M == 9 ? 8 : 17));
        double d[M];
#pragma unroll
        for (int j = 0; j < M; ++j) d[j] = t - LOBATTO_NODES[off + j];
        double pre = 1.0;            // prod_{i < j} d_i
#pragma unroll
        for (int j = 0; j < M; ++j) {
            b[j] = pre * LOBATTO_INVDEN[off + j];
            pre *= d[j];
        }
        double suf = 1.0;            // prod_{i > j} d_i
#pragma unroll
        for (int j = M - 1; j >= 0; --j) {
            b[j] *= suf;
            suf *= d[j];
        }
    }
}

// the same into LDS (stride BLOCK), m in {1, 3, 5, 9, 17} wave-uniform
__device__ __forceinline__ void stage_basis(double t, int m, double* dst) {
    if (m == 17) {
        double b[17];
        lobatto_basis<17>(t, b);
#pragma unroll
        for (int j = 0; j < 17; ++j) dst[j * BLOCK] = b[j];
        return;
    }
    if (m == 3) {
        double b[3];
        lobatto_basis<3>(t, b);
#pragma unroll
        for (int j = 0; j < 3; ++j) dst[j * BLOCK] = b[j];
    } else if (m == 5) {
        double b[5];
        lobatto_basis<5>(t, b);
#pragma unroll
        for (int j = 0; j < 5; ++j) dst[j * BLOCK] = b[j];
    } else if (m == 9) {
        double b[9];
        lobatto_basis<9>(t, b);
#pragma unroll
        for (int j = 0; j < 9; ++j) dst[j * BLOCK] = b[j];
    } else {
        dst[0] = 1.0;
    }
}

__device__ __forceinline__ void out_field_store(double* p, double v) { __builtin_nontemporal_store(v, p); }

// One grid: part[o] = sum over the outer dimensions' nodes of (prod_a b_a[j_a]) (sum_{j} bI[j] Y[row M + j][o]); acc += c part.
// Four outer loops, the unused ones (a grid with fewer active dimensions is right-aligned) with one node and weight 1: their
// trip count of one costs a compare per level.  NOUT: columns kept in registers; EXACT: n_out == NOUT (no guards, the row
// loads merge into wide scalar loads).  `outer`: this thread's LDS slots, dimension a at a * ostride, node j at j * BLOCK.
template <int NOUT, bool EXACT, int MI>
__device__ __forceinline__ void contract_grid(const int (&m)[MAXO], const double* outer, int ostride, double ti,
                                              const double* __restrict__ val, int n_out, double c, double (&acc)[NOUT]) {
    double bi[MI];
    lobatto_basis<MI>(ti, bi);
    double part[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) part[o] = 0.0;
    const double* row = val;
    for (int j0 = 0; j0 < m[0]; ++j0) {
        const double w0 = m[0] > 1 ? outer[j0 * BLOCK] : 1.0;
        for (int j1 = 0; j1 < m[1]; ++j1) {
            const double w1 = m[1] > 1 ? w0 * outer[ostride + j1 * BLOCK] : w0;
            for (int j2 = 0; j2 < m[2]; ++j2) {
                const double w2 = m[2] > 1 ? w1 * outer[2 * ostride + j2 * BLOCK] : w1;
                for (int j3 = 0; j3 < m[3]; ++j3) {
                    const double w3 = m[3] > 1 ? w2 * outer[3 * ostride + j3 * BLOCK] : w2;
                    double tmp[NOUT];
#pragma unroll
                    for (int o = 0; o < NOUT; ++o) tmp[o] = 0.0;
#pragma unroll
                    for (int j = 0; j < MI; ++j) {
#pragma unroll
                        for (int o = 0; o < NOUT; ++o)
                            if (EXACT || o < n_out) tmp[o] = fma(bi[j], row[j * n_out + o], tmp[o]);
                    }
                    row += MI * n_out;
#pragma unroll
                    for (int o = 0; o < NOUT; ++o) part[o] = fma(w3, tmp[o], part[o]);
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) acc[o] = fma(c, part[o], acc[o]);
}

// the fused reconstruction (round 4): outputs lat0 .. lat0 + rank - 1 of the prediction are the SVD latent coefficients of a field
// (scripts/pem_v0/pem_v0_SPT-100.yml:273-280: `j_ion`, log10 norm), and the field itself -- denorm(latent @ basis^T), dof values per
// point, row-major -- leaves with the prediction instead of through a second pass (pem_svd_reconstruct_f64_dev)
struct Recon {
    const double* basis;     // [dof][rank]
    double* field;           // [n][dof]
    int dof, rank, lat0, norm;
    double scale;
};

template <int NOUT, bool EXACT>
__global__ __launch_bounds__(BLOCK) void sparse_predict_kernel(long long n, int n_dim, int n_beta, const int32_t* __restrict__ index,
                                                               const double* __restrict__ coef,
                                                               const double* __restrict__ values, int n_out_arg,
                                                               const double* __restrict__ t, size_t ld,
                                                               double* __restrict__ out, size_t ld_out, int per_grid, int max_outer,
                                                               int max_m, int basis_words, Recon rc) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int ostride = max_m * BLOCK;
    double* basis = lds;                                    // [max_outer][max_m][BLOCK]; later: the latents [BLOCK][rank]
    double* coord = lds + (size_t)basis_words * BLOCK;      // [n_dim][BLOCK]  (basis_words = max(max_outer max_m, rank))
    const int n_out = EXACT ? NOUT : n_out_arg;
    const int tid = threadIdx.x;
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i0 = (long long)blockIdx.x * BLOCK; i0 < n; i0 += stride) {
        const long long i = i0 + tid < n ? i0 + tid : n - 1;        // a dead lane recomputes the last point and stores nothing
        for (int d = 0; d < n_dim; ++d) coord[d * BLOCK + tid] = t[(size_t)d * ld + i];
        double acc[NOUT];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) acc[o] = 0.0;
        for (int bi = 0; bi < n_beta; ++bi) {
            // (this grid step has a twin, grid_term below, used by the chain kernel: a change here is made there too)
            const int32_t* e = index + (size_t)bi * IDX_STRIDE;
            const int na = e[0];
            const double* val = values + (size_t)e[1] * n_out;
            // right-align the active dimensions: (1, .., 1, m) / (1, .., m, m') / ... gives the same node order (a dimension with one
            // node contributes no stride), and the innermost -- unrolled -- one is always an active one.  The outer dimensions' LDS
            // slots are right-aligned inside the max_outer slots the launch has room for.
            const int sh = MAXA - na;
            int m[MAXO];
            const double* slots = basis + tid - (MAXO - max_outer) * ostride;     // slot a of this thread (only active ones are touched)
#pragma unroll
            for (int a = 0; a < MAXO; ++a) {
                const bool on = a >= sh;
                m[a] = on ? nodes_of(e[2 + MAXA + (on ? a - sh : 0)]) : 1;
                // (this thread's slots only: no barrier, a wave's LDS traffic is executed in order)
                if (on) stage_basis(coord[e[2 + a - sh] * BLOCK + tid], m[a], const_cast<double*>(slots) + a * ostride);
            }
            const int mi = na > 0 ? nodes_of(e[2 + MAXA + na - 1]) : 1;
            const double ti = na > 0 ? coord[e[2 + na - 1] * BLOCK + tid] : 0.0;
            const double c = coef[bi];
            if (mi == 3) contract_grid<NOUT, EXACT, 3>(m, slots, ostride, ti, val, n_out, c, acc);
            else if (mi == 5) contract_grid<NOUT, EXACT, 5>(m, slots, ostride, ti, val, n_out, c, acc);
            else if (mi == 9) contract_grid<NOUT, EXACT, 9>(m, slots, ostride, ti, val, n_out, c, acc);
            else if (mi == 17) contract_grid<NOUT, EXACT, 17>(m, slots, ostride, ti, val, n_out, c, acc);
            else contract_grid<NOUT, EXACT, 1>(m, slots, ostride, ti, val, n_out, c, acc);     // the constant grid (beta = 0)
            if (per_grid) {      // every grid's own (coefficient-weighted) interpolant: out[bi][o][i]
                if (i0 + tid < n) {
#pragma unroll
                    for (int o = 0; o < NOUT; ++o)
                        if (EXACT || o < n_out) out[((size_t)bi * n_out + o) * ld_out + i] = acc[o];
                }
#pragma unroll
                for (int o = 0; o < NOUT; ++o) acc[o] = 0.0;
            }
        }
        if (per_grid) continue;
        if (i0 + tid < n) {
#pragma unroll
            for (int o = 0; o < NOUT; ++o)
                if (EXACT || o < n_out) out[(size_t)o * ld_out + i] = acc[o];
        }
        if (rc.field) {
            // (twin: rebuild_field below, used by the chain kernel: a change here is made there too)
            // the latents of this workgroup's 256 points through LDS (the basis slots are free again), then every WAVE rebuilds the
            // dof values of its 64 points row by row: lane = field index, 512 contiguous bytes per store
            __syncthreads();                                 // (another wave may still read its basis slots)
            double* lat = lds;                               // [BLOCK][rank]
#pragma unroll
            for (int o = 0; o < NOUT; ++o)
                if (o >= rc.lat0 && o < rc.lat0 + rc.rank) lat[tid * rc.rank + (o - rc.lat0)] = acc[o];
            __syncthreads();
            const int wave = tid >> 6, lane = tid & 63;
            for (int k0 = 0; k0 < rc.dof; k0 += 64) {
                const int k = k0 + lane;
                double bk[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) bk[q] = (k < rc.dof && q < rc.rank) ? rc.basis[(size_t)k * rc.rank + q] : 0.0;
                for (int r = 0; r < 64; ++r) {
                    const long long p = i0 + wave * 64 + r;
                    if (p >= n) break;
                    const double* lr = lat + (wave * 64 + r) * rc.rank;
                    double v = 0.0;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (q < rc.rank) v = fma(lr[q], bk[q], v);
                    if (rc.norm == PEM_NORM_LOG10) v = exp10(v);
                    else if (rc.norm == PEM_NORM_LINEAR) v = v / rc.scale;
                    if (k < rc.dof) out_field_store(rc.field + (size_t)p * rc.dof + k, v);
                }
            }
            __syncthreads();                                 // the next batch of points stages its bases over the latents
        }
    }
}

template <int NOUT, bool EXACT>
void launch_predict(size_t n, int n_dim, int n_beta, const int32_t* index, const double* coef, const double* values, int n_out,
                    const double* t, size_t ld, double* out, size_t ld_out, int per_grid, int max_outer, int max_m, const Recon& rc,
                    hipStream_t st) {
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 256 * 8) blocks = 256 * 8;
    int basis_words = max_outer * max_m;                                           // doubles per thread: bases (or latents) | coordinates
    if (rc.field && rc.rank > basis_words) basis_words = rc.rank;
    const size_t lds = (size_t)(basis_words + n_dim) * BLOCK * sizeof(double);
    if (lds > 64 * 1024) {
        static pem::LdsAttrOnce attr;
        (void)attr.ensure(reinterpret_cast<const void*>(sparse_predict_kernel<NOUT, EXACT>));      // a refusal shows as a launch error below
    }
    hipLaunchKernelGGL((sparse_predict_kernel<NOUT, EXACT>), dim3((unsigned)blocks), dim3(BLOCK), lds, st, (long long)n, n_dim, n_beta,
                       index, coef, values, n_out, t, ld, out, ld_out, per_grid, max_outer, max_m, basis_words, rc);
}

// ---- the component chain (round 5): cathode -> V_cc -> thruster -> I_B0 -> plume, three tables in ONE launch --------------------
// scripts/pem_v0/pem_v0_SPT-100.yml:4-6,55-63,110-178,215-280: the reference trains one surrogate per component and chains them
// through the coupling variables.  The helpers below are the single-table kernel's per-grid and field-rebuild steps, restated for
// the chain's stages: sparse_predict_kernel keeps its own inline copies so that none of its instantiations changes (calling these
// helpers from it, even __forceinline__, reorders its registers and instructions: its assembly is no longer the same), so a fix to
// one copy is made to the other by hand -- both are marked.  Both call
// stage_basis / contract_grid, so a stage sums in the single-table kernel's order and the chain equals three single-table
// launches bit for bit.
// One grid of a table: stage the outer dimensions' bases of this thread's point (coordinates in `coord`, [dims][BLOCK]) in its
// LDS slots under `basis` (max_outer slots of ostride doubles) and add the grid's interpolant, weighted by *cb, to acc.
// twin of the per-grid step inside sparse_predict_kernel's loop over the grids
template <int NOUT, bool EXACT>
__device__ __forceinline__ void grid_term(const int32_t* __restrict__ e, const double* __restrict__ values, int n_out, const double* cb,
                                          const double* coord, double* basis, int tid, int max_outer, int ostride, double (&acc)[NOUT]) {
    const int na = e[0];
    const double* val = values + (size_t)e[1] * n_out;
    // right-align the active dimensions: (1, .., 1, m) / (1, .., m, m') / ... gives the same node order (a dimension with one
    // node contributes no stride), and the innermost -- unrolled -- one is always an active one.  The outer dimensions' LDS
    // slots are right-aligned inside the max_outer slots the launch has room for.
    const int sh = MAXA - na;
    int m[MAXO];
    const double* slots = basis + tid - (MAXO - max_outer) * ostride;     // slot a of this thread (only active ones are touched)
#pragma unroll
    for (int a = 0; a < MAXO; ++a) {
        const bool on = a >= sh;
        m[a] = on ? nodes_of(e[2 + MAXA + (on ? a - sh : 0)]) : 1;
        // (this thread's slots only: no barrier, a wave's LDS traffic is executed in order)
        if (on) stage_basis(coord[e[2 + a - sh] * BLOCK + tid], m[a], const_cast<double*>(slots) + a * ostride);
    }
    const int mi = na > 0 ? nodes_of(e[2 + MAXA + na - 1]) : 1;
    const double ti = na > 0 ? coord[e[2 + na - 1] * BLOCK + tid] : 0.0;
    const double c = *cb;
    if (mi == 3) contract_grid<NOUT, EXACT, 3>(m, slots, ostride, ti, val, n_out, c, acc);
    else if (mi == 5) contract_grid<NOUT, EXACT, 5>(m, slots, ostride, ti, val, n_out, c, acc);
    else if (mi == 9) contract_grid<NOUT, EXACT, 9>(m, slots, ostride, ti, val, n_out, c, acc);
    else if (mi == 17) contract_grid<NOUT, EXACT, 17>(m, slots, ostride, ti, val, n_out, c, acc);
    else contract_grid<NOUT, EXACT, 1>(m, slots, ostride, ti, val, n_out, c, acc);     // the constant grid (beta = 0)
}

// the latents of this workgroup's 256 points through LDS (the basis slots are free again), then every WAVE rebuilds the
// dof values of its 64 points row by row: lane = field index, 512 contiguous bytes per store
// twin of sparse_predict_kernel's `if (rc.field)` epilogue
template <int NOUT>
__device__ __forceinline__ void rebuild_field(const double (&acc)[NOUT], const Recon& rc, double* lds, long long i0, long long n, int tid) {
    __syncthreads();                                 // (another wave may still read its basis slots)
    double* lat = lds;                               // [BLOCK][rank]
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
        if (o >= rc.lat0 && o < rc.lat0 + rc.rank) lat[tid * rc.rank + (o - rc.lat0)] = acc[o];
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int k0 = 0; k0 < rc.dof; k0 += 64) {
        const int k = k0 + lane;
        double bk[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) bk[q] = (k < rc.dof && q < rc.rank) ? rc.basis[(size_t)k * rc.rank + q] : 0.0;
        for (int r = 0; r < 64; ++r) {
            const long long p = i0 + wave * 64 + r;
            if (p >= n) break;
            const double* lr = lat + (wave * 64 + r) * rc.rank;
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q < rc.rank) v = fma(lr[q], bk[q], v);
            if (rc.norm == PEM_NORM_LOG10) v = exp10(v);
            else if (rc.norm == PEM_NORM_LINEAR) v = v / rc.scale;
            if (k < rc.dof) out_field_store(rc.field + (size_t)p * rc.dof + k, v);
        }
    }
    __syncthreads();                                 // the next batch of points stages its bases over the latents
}

struct ChainStage {
    const int32_t* index;
    const double* coef;
    const double* values;
    int n_beta, n_out, max_outer, max_m;
};

// one stage's interpolant at this thread's point: the grids' dims[] are slots of the shared coordinate table `coord`
template <int NOUT, bool EXACT>
__device__ __forceinline__ void stage_predict(const ChainStage& s, const double* coord, double* basis, int tid, double (&acc)[NOUT]) {
    const int n_out = EXACT ? NOUT : s.n_out;
    const int ostride = s.max_m * BLOCK;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) acc[o] = 0.0;
    for (int bi = 0; bi < s.n_beta; ++bi)
        grid_term<NOUT, EXACT>(s.index + (size_t)bi * IDX_STRIDE, s.values, n_out, s.coef + bi, coord, basis, tid, s.max_outer, ostride, acc);
}

// a coupling value y -> its normalised coordinate over [lo, lo + w]: the expression system.py's _predict_surrogate applies to the
// inputs, left to right, no contraction (the torch composition of three single-table launches rounds the same way)
__device__ __forceinline__ double coupling_coord(double y, double lo, double w) {
#pragma clang fp contract(off)
    return 2.0 * (y - lo) / w - 1.0;
}

// out rows: V_cc, I_B0, T, div_angle, T_c = T cos(div_angle) (plume.py:136-140), then plume outputs 1 .. n_out - 1 (the latents)
template <int NOUT, bool EXACT>
__global__ __launch_bounds__(BLOCK) void sparse_chain_kernel(long long n, int n_dim, int vcc_slot, int ib0_slot, ChainStage cat, ChainStage thr,
                                                             ChainStage plu, double vcc_lo, double vcc_w, double ib0_lo, double ib0_w,
                                                             const double* __restrict__ t, size_t ld, double* __restrict__ out,
                                                             size_t ld_out, int basis_words, Recon rc) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* basis = lds;                                    // every stage's outer bases in turn; later: the latents [BLOCK][rank]
    double* coord = lds + (size_t)basis_words * BLOCK;      // [n_dim][BLOCK]: the external coordinates and the two coupling slots
    const int n_out = EXACT ? NOUT : plu.n_out;
    const int tid = threadIdx.x;
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i0 = (long long)blockIdx.x * BLOCK; i0 < n; i0 += stride) {
        const long long i = i0 + tid < n ? i0 + tid : n - 1;        // a dead lane recomputes the last point and stores nothing
        for (int d = 0, r = 0; d < n_dim; ++d)
            if (d != vcc_slot && d != ib0_slot) coord[d * BLOCK + tid] = t[(size_t)(r++) * ld + i];
        // (each stage reads and writes this thread's own slots only: no barrier between the stages)
        double vcc[1], thrust[2], plume[NOUT];
        stage_predict<1, true>(cat, coord, basis, tid, vcc);
        coord[vcc_slot * BLOCK + tid] = coupling_coord(vcc[0], vcc_lo, vcc_w);
        stage_predict<2, true>(thr, coord, basis, tid, thrust);
        coord[ib0_slot * BLOCK + tid] = coupling_coord(thrust[0], ib0_lo, ib0_w);
        stage_predict<NOUT, EXACT>(plu, coord, basis, tid, plume);
        if (i0 + tid < n) {
            out[i] = vcc[0];
            out[ld_out + i] = thrust[0];
            out[2 * ld_out + i] = thrust[1];
            out[3 * ld_out + i] = plume[0];
            out[4 * ld_out + i] = thrust[1] * cos(plume[0]);
#pragma unroll
            for (int o = 1; o < NOUT; ++o)
                if (EXACT || o < n_out) out[(size_t)(4 + o) * ld_out + i] = plume[o];
        }
        if (rc.field) rebuild_field<NOUT>(plume, rc, lds, i0, n, tid);
    }
}

template <int NOUT, bool EXACT>
void launch_chain(size_t n, int n_dim, int vcc_slot, int ib0_slot, const ChainStage (&s)[3], const double (&map)[4], const double* t,
                  size_t ld, double* out, size_t ld_out, int basis_words, const Recon& rc, hipStream_t st) {
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 256 * 8) blocks = 256 * 8;
    const size_t lds = (size_t)(basis_words + n_dim) * BLOCK * sizeof(double);
    if (lds > 64 * 1024) {
        static pem::LdsAttrOnce attr;
        (void)attr.ensure(reinterpret_cast<const void*>(sparse_chain_kernel<NOUT, EXACT>));      // a refusal shows as a launch error below
    }
    hipLaunchKernelGGL((sparse_chain_kernel<NOUT, EXACT>), dim3((unsigned)blocks), dim3(BLOCK), lds, st, (long long)n, n_dim, vcc_slot,
                       ib0_slot, s[0], s[1], s[2], map[0], map[1], map[2], map[3], t, ld, out, ld_out, basis_words, rc);
}

// ---- the chain fused with the multi-QoI likelihood: the surrogate in the model's place inside the calibration --------------------
// scripts/pem_v0/mcmc.py:57-106: `SURR.predict`, `jion_reconstruct`, the Gaussian sums, I_D from the surrogate's own output.  The
// stages are sparse_chain_kernel's (stage_predict, coupling_coord: the same bits); the epilogue is one lane per sample, as
// system_epilogue_sum of the coupled kernel: the j_ion nodes its condition's records touch are rebuilt from the latents (rebuild_field's
// expression) and compared at once, so that the 91-point profile exists nowhere.
struct ChainLik {
    const double* basis;     // [91][rank] or NULL: no j_ion
    const double* rec;       // [n_rec][4] {w, y, 1/std, bits}
    const int32_t* span;     // [n_cond][4 kinds][2] {first record, count}
    const double* a_1;       // NULL or [n]: the discharge-current term
    double* loglik;          // [n]
    double* out;             // NULL or the chain's rows
    double* pred;            // NULL or [ceil(n / n_cond)][ld_pred]
    size_t ld_out, ld_pred;
    int lat0, rank, norm, n_cond, n_rec, staged;
    double scale, discharge, inv_sigma;
};

// profile node k from this thread's latents (`lat`: its LDS slots, latent q at q * BLOCK): rebuild_field's sum and denormalisation
__device__ __forceinline__ double jion_node(const double* lat, const double* jb, int k, int rank, int norm, double scale) {
    double v = 0.0;
    for (int q = 0; q < rank; ++q) v = fma(lat[q * BLOCK], jb[k * rank + q], v);
    if (norm == PEM_NORM_LOG10) v = exp10(v);
    else if (norm == PEM_NORM_LINEAR) v = v / scale;
    return v;
}

// The records of sample i (condition i mod n_cond) against the chain's values: the sum in the order j_ion, V_cc, T, then the
// discharge term; `store`: this lane's sample exists (a dead lane recomputes the last one and writes nothing).  Adjacent lanes belong
// to different conditions: the loops diverge and every lane reads its own records (the odd padding of the blocks spreads them over
// the banks).  Consecutive j_ion records mostly share a node or sit on neighbouring intervals: a node value depends on k alone, so
// the last two are kept.
__device__ __forceinline__ void chain_loglik_epilogue(const ChainLik& lk, const double* rec, const int32_t* span, const double* jb,
                                                      const double* lat, long long i, bool store, double V_cc, double I_B0, double T) {
#pragma clang fp contract(off)
    const long long d = i / lk.n_cond;
    const int c = (int)(i - d * lk.n_cond);
    const double4* r4 = reinterpret_cast<const double4*>(rec);
    const int2* sp = reinterpret_cast<const int2*>(span) + 4 * c;
    const int2 rj = sp[PEM_SYS_JION], rv = sp[PEM_SYS_VCC], rt = sp[PEM_SYS_T], ru = sp[PEM_SYS_UION];
    double* prow = (lk.pred && store) ? lk.pred + (size_t)d * lk.ld_pred : nullptr;
    double ll = 0.0;
    if (jb) {
        int pk = -2;
        double lo = 0.0, hi = 0.0;
        for (int r = max(rj.x, 0); r < min(rj.x + rj.y, lk.n_rec); ++r) {
            const double4 e = r4[r];
            const int k = (int)min((unsigned)__double_as_longlong(e.w), 89u);
            if (k == pk + 1) {
                lo = hi;
                hi = jion_node(lat, jb, k + 1, lk.rank, lk.norm, lk.scale);
            } else if (k != pk) {
                lo = jion_node(lat, jb, k, lk.rank, lk.norm, lk.scale);
                hi = jion_node(lat, jb, k + 1, lk.rank, lk.norm, lk.scale);
            }
            pk = k;
            const double m = fma(e.x, hi - lo, lo);
            if (prow) prow[r] = m;
            const double z = (e.y - m) * e.z;
            ll = fma(-0.5 * z, z, ll);
        }
    }
    for (int r = max(rv.x, 0); r < min(rv.x + rv.y, lk.n_rec); ++r) {   // the cathode stage's coupling voltage
        const double4 e = r4[r];
        if (prow) prow[r] = V_cc;
        const double z = (e.y - V_cc) * e.z;
        ll = fma(-0.5 * z, z, ll);
    }
    for (int r = max(rt.x, 0); r < min(rt.x + rt.y, lk.n_rec); ++r) {   // the thruster stage's thrust T (not T_c)
        const double4 e = r4[r];
        if (prow) prow[r] = T;
        const double z = (e.y - T) * e.z;
        ll = fma(-0.5 * z, z, ll);
    }
    // what the chain cannot give is made visible: no u_ion latents, or j_ion records without a basis
    if (ru.y > 0 || (!jb && rj.y > 0)) ll = __builtin_nan("");
    if (lk.a_1) {                                                       // I_d of the test double from the SURROGATE's I_B0 (mcmc.py:101)
        const double den = 1.0 - 2.0 * lk.a_1[i];
        const double i_d = I_B0 / den;
        const double z = (lk.discharge - i_d) * lk.inv_sigma;
        ll = fma(-0.5 * z, z, ll);
    }
    if (store) lk.loglik[i] = ll;
}

template <int NOUT, bool EXACT>
__global__ __launch_bounds__(BLOCK) void chain_loglik_kernel(long long n, int n_dim, int vcc_slot, int ib0_slot, ChainStage cat, ChainStage thr,
                                                             ChainStage plu, double vcc_lo, double vcc_w, double ib0_lo, double ib0_w,
                                                             const double* __restrict__ t, size_t ld, int basis_words, ChainLik lk) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* basis = lds;                                    // every stage's outer bases in turn; later: this thread's latents [rank][BLOCK]
    double* coord = lds + (size_t)basis_words * BLOCK;      // [n_dim][BLOCK]
    const int n_out = EXACT ? NOUT : plu.n_out;
    const int tid = threadIdx.x;
    // the measurement table, the spans and the j_ion basis: beside the coordinates where the launch found room, else through the cache
    const double* rec = lk.rec;
    const int32_t* span = lk.span;
    const double* jb = lk.basis;
    if (lk.staged) {
        double* srec = coord + (size_t)n_dim * BLOCK;
        int32_t* sspan = reinterpret_cast<int32_t*>(srec + 4 * lk.n_rec);
        double* sjb = srec + 4 * lk.n_rec + 4 * lk.n_cond;
        for (int k = tid; k < 4 * lk.n_rec; k += BLOCK) srec[k] = lk.rec[k];
        for (int k = tid; k < 8 * lk.n_cond; k += BLOCK) sspan[k] = lk.span[k];
        if (lk.basis)
            for (int k = tid; k < PEM_NANGLE * lk.rank; k += BLOCK) sjb[k] = lk.basis[k];
        __syncthreads();
        rec = srec;
        span = sspan;
        if (lk.basis) jb = sjb;
    }
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i0 = (long long)blockIdx.x * BLOCK; i0 < n; i0 += stride) {
        const bool live = i0 + tid < n;
        const long long i = live ? i0 + tid : n - 1;        // a dead lane recomputes the last point and stores nothing
        for (int d = 0, r = 0; d < n_dim; ++d)
            if (d != vcc_slot && d != ib0_slot) coord[d * BLOCK + tid] = t[(size_t)(r++) * ld + i];
        // (each stage and the epilogue read and write this thread's own slots only: no barrier inside the loop)
        double vcc[1], thrust[2], plume[NOUT];
        stage_predict<1, true>(cat, coord, basis, tid, vcc);
        coord[vcc_slot * BLOCK + tid] = coupling_coord(vcc[0], vcc_lo, vcc_w);
        stage_predict<2, true>(thr, coord, basis, tid, thrust);
        coord[ib0_slot * BLOCK + tid] = coupling_coord(thrust[0], ib0_lo, ib0_w);
        stage_predict<NOUT, EXACT>(plu, coord, basis, tid, plume);
        if (lk.out && live) {
            double* out = lk.out;
            const size_t ld_out = lk.ld_out;
            out[i] = vcc[0];
            out[ld_out + i] = thrust[0];
            out[2 * ld_out + i] = thrust[1];
            out[3 * ld_out + i] = plume[0];
            out[4 * ld_out + i] = thrust[1] * cos(plume[0]);
#pragma unroll
            for (int o = 1; o < NOUT; ++o)
                if (EXACT || o < n_out) out[(size_t)(4 + o) * ld_out + i] = plume[o];
        }
        // the latents leave the registers (the basis slots are free again): after this only V_cc, I_B0 and T are live
        if (lk.basis) {
#pragma unroll
            for (int o = 0; o < NOUT; ++o)
                if (o >= lk.lat0 && o < lk.lat0 + lk.rank) basis[(o - lk.lat0) * BLOCK + tid] = plume[o];
        }
        chain_loglik_epilogue(lk, rec, span, jb, basis + tid, i, live, vcc[0], thrust[0], thrust[1]);
    }
}

template <int NOUT, bool EXACT>
void launch_chain_loglik(size_t n, int n_dim, int vcc_slot, int ib0_slot, const ChainStage (&s)[3], const double (&map)[4], const double* t,
                         size_t ld, int basis_words, size_t lds, const ChainLik& lk, hipStream_t st) {
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (lds > 64 * 1024) {
        static pem::LdsAttrOnce attr;
        (void)attr.ensure(reinterpret_cast<const void*>(chain_loglik_kernel<NOUT, EXACT>));      // a refusal shows as a launch error below
    }
    hipLaunchKernelGGL((chain_loglik_kernel<NOUT, EXACT>), dim3((unsigned)blocks), dim3(BLOCK), lds, st, (long long)n, n_dim, vcc_slot,
                       ib0_slot, s[0], s[1], s[2], map[0], map[1], map[2], map[3], t, ld, basis_words, lk);
}

// what both chained entry points ask of the slots, the coupling domains and the three tables; fills the kernels' view of the stages
// and the largest stage's outer-basis words per thread
int check_chain(const char* who, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo, double vcc_w,
                double ib0_lo, double ib0_w, ChainStage (&cs)[3], int& basis_words, int thr_out = 2) {
    if (!stages) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL stage array", who);
    if (n_dim < 2 || n_dim > PEM_SURR_MAX_DIM)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: 2 <= n_dim <= %d (the external coordinates and the two coupling slots)", who, PEM_SURR_MAX_DIM);
    if (vcc_slot < 0 || vcc_slot >= n_dim || ib0_slot < 0 || ib0_slot >= n_dim || vcc_slot == ib0_slot)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the V_cc and I_B0 slots are two different coordinates < n_dim", who);
    if (!std::isfinite(vcc_lo) || !std::isfinite(vcc_w) || !(vcc_w > 0.0) || !std::isfinite(ib0_lo) || !std::isfinite(ib0_w) || !(ib0_w > 0.0))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: a coupling domain needs a finite lo and a finite width w > 0", who);
    const int need_out[3] = {1, thr_out, 0};           // cathode: V_cc; thruster: I_B0, T [, u_ion latents]; plume: div_angle [, latents]
    basis_words = 0;
    for (int k = 0; k < 3; ++k) {
        const pem_surr_stage& g = stages[k];
        if (!g.index || !g.coef || !g.values) return pem::fail(PEM_ERR_INVALID_ARG, "%s: stage %d: NULL table", who, k);
        if (g.n_beta < 1 || g.n_out < 1 || g.n_out > 16 || (need_out[k] && g.n_out != need_out[k]))
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: stage %d: need n_beta >= 1 and n_out %s", who, k,
                             k == 0 ? "== 1" : (k == 1 ? (thr_out == 2 ? "== 2" : "== 2 + u_rank") : "in 1 .. 16"));
        if (g.max_active < 0 || g.max_active > PEM_SURR_MAX_ACTIVE || g.max_level < 0 || g.max_level > PEM_SURR_MAX_LEVEL)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: stage %d: at most %d active dimensions of level <= %d per multi-index", who, k,
                             PEM_SURR_MAX_ACTIVE, PEM_SURR_MAX_LEVEL);
        cs[k] = ChainStage{g.index, g.coef, g.values, g.n_beta, g.n_out, g.max_active > 1 ? g.max_active - 1 : 0,
                           g.max_level == 0 ? 1 : (1 << g.max_level) + 1};
        if (cs[k].max_outer * cs[k].max_m > basis_words) basis_words = cs[k].max_outer * cs[k].max_m;
    }
    return PEM_OK;
}

}  // namespace

// pem_surrogate_fields.hip compiles this file's device code a second time (the node tables above stay in ONE place) and instantiates
// its own kernels only: the entry points below, and with them every kernel instantiation of this file, are left out of that unit
#ifndef PEM_SURROGATE_FIELDS_UNIT
namespace {

int sparse_predict(const char* who, size_t n, int n_dim, int n_beta, const int32_t* index, const double* coef, const double* values,
                   int n_out, const double* t, size_t ld, double* out, size_t ld_out, int per_grid, int max_active, int max_level,
                   const Recon& rc, pem_stream_t stream) {
    if (n_dim < 1 || n_beta < 1 || n_out < 1 || n_out > 16)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: need n_dim, n_beta >= 1 and 1 <= n_out <= 16", who);
    if (max_active < 0 || max_active > PEM_SURR_MAX_ACTIVE || max_level < 0 || max_level > PEM_SURR_MAX_LEVEL)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: at most %d active dimensions of level <= %d per multi-index", who, PEM_SURR_MAX_ACTIVE,
                         PEM_SURR_MAX_LEVEL);
    if (n == 0) return PEM_OK;
    if (!index || !coef || !values || !t || !out) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if (ld < n || ld_out < n) return pem::fail(PEM_ERR_INVALID_ARG, "%s: leading dimension smaller than n", who);
    if (n_dim > PEM_SURR_MAX_DIM) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_dim <= %d", who, PEM_SURR_MAX_DIM);
    if (rc.field && (rc.rank < 1 || rc.rank > 16 || rc.lat0 < 0 || rc.lat0 + rc.rank > n_out || rc.dof < 1 || !rc.basis || per_grid))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the reconstructed field takes 1 <= rank <= 16 latent outputs lat0 .. lat0 + rank - 1 of the n_out", who);
    // the LDS of the outer dimensions' bases is sized by what the table really holds (the caller says): a level-3, three-dimension
    // table keeps rounds 1-3's 36 KB, four outer dimensions of 17 nodes take 139 KB
    const int max_outer = max_active > 1 ? max_active - 1 : 0, max_m = max_level == 0 ? 1 : (1 << max_level) + 1;
    if ((size_t)(max_outer * max_m + n_dim) * BLOCK * sizeof(double) > 160 * 1024)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: %d outer dimensions of %d nodes and %d coordinates do not fit the LDS", who, max_outer, max_m, n_dim);
    if (int rc0 = pem::check_device()) return rc0;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define PEM_PREDICT(NOUT_, EXACT_) \
    launch_predict<NOUT_, EXACT_>(n, n_dim, n_beta, index, coef, values, n_out, t, ld, out, ld_out, per_grid, max_outer, max_m, rc, st)
    switch (n_out) {
        case 1: PEM_PREDICT(1, true); break;
        case 2: PEM_PREDICT(2, true); break;
        case 3: PEM_PREDICT(3, true); break;
        case 4: PEM_PREDICT(4, true); break;
        default:
            if (n_out <= 8) PEM_PREDICT(8, false);
            else PEM_PREDICT(16, false);
    }
#undef PEM_PREDICT
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int sparse_predict_chain(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo, double vcc_w,
                         double ib0_lo, double ib0_w, const double* t, size_t ld, double* out, size_t ld_out, const Recon& rc,
                         pem_stream_t stream) {
    const char* who = "pem_sparse_predict_chain";
    ChainStage cs[3];
    int basis_words = 0;
    if (int rc0 = check_chain(who, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, cs, basis_words)) return rc0;
    const int n_plume = stages[2].n_out;
    if (rc.field && (rc.rank < 1 || rc.rank > 16 || rc.lat0 < 0 || rc.lat0 + rc.rank > n_plume || rc.dof < 1 || !rc.basis))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the reconstructed field takes 1 <= rank <= 16 latent outputs lat0 .. lat0 + rank - 1 of the plume stage", who);
    if (rc.field && rc.rank > basis_words) basis_words = rc.rank;
    // the bases of one stage at a time: the largest stage's (max_active - 1) (2^max_level + 1), plus every coordinate
    if ((size_t)(basis_words + n_dim) * BLOCK * sizeof(double) > 160 * 1024)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the largest stage's outer bases and %d coordinates do not fit the LDS", who, n_dim);
    if (n == 0) return PEM_OK;
    if ((n_dim > 2 && !t) || !out) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if ((n_dim > 2 && ld < n) || ld_out < n) return pem::fail(PEM_ERR_INVALID_ARG, "%s: leading dimension smaller than n", who);
    if (int rc0 = pem::check_device()) return rc0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double map[4] = {vcc_lo, vcc_w, ib0_lo, ib0_w};
#define PEM_CHAIN(NOUT_, EXACT_) launch_chain<NOUT_, EXACT_>(n, n_dim, vcc_slot, ib0_slot, cs, map, t, ld, out, ld_out, basis_words, rc, st)
    switch (n_plume) {
        case 1: PEM_CHAIN(1, true); break;
        case 2: PEM_CHAIN(2, true); break;
        case 3: PEM_CHAIN(3, true); break;
        case 4: PEM_CHAIN(4, true); break;
        default:
            if (n_plume <= 8) PEM_CHAIN(8, false);
            else PEM_CHAIN(16, false);
    }
#undef PEM_CHAIN
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int chain_system_loglik(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo, double vcc_w,
                        double ib0_lo, double ib0_w, const double* t, size_t ld, int dof, double discharge_sigma, ChainLik lk,
                        pem_stream_t stream) {
    const char* who = "pem_chain_system_loglik";
    ChainStage cs[3];
    int basis_words = 0;
    if (int rc0 = check_chain(who, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, cs, basis_words)) return rc0;
    const int n_plume = stages[2].n_out;
    if (lk.basis) {
        if (lk.rank < 1 || lk.rank > 16 || lk.lat0 < 0 || lk.lat0 + lk.rank > n_plume)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: the j_ion map takes 1 <= rank <= 16 latent outputs lat0 .. lat0 + rank - 1 of the plume stage", who);
        if (dof != PEM_NANGLE) return pem::fail(PEM_ERR_INVALID_ARG, "%s: the j_ion records index the %d-point profile: dof must be %d, got %d", who, PEM_NANGLE, PEM_NANGLE, dof);
        if (lk.norm != PEM_NORM_NONE && lk.norm != PEM_NORM_LOG10 && lk.norm != PEM_NORM_LINEAR)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: unknown norm %d", who, lk.norm);
        if (lk.rank > basis_words) basis_words = lk.rank;          // the latents take the basis slots of their thread
    }
    const size_t base = (size_t)(basis_words + n_dim) * BLOCK * sizeof(double);
    if (base > 160 * 1024)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the largest stage's outer bases and %d coordinates do not fit the LDS", who, n_dim);
    if (lk.n_cond < 1 || lk.n_cond > PEM_FUSED_SYSTEM_MAX_RECORDS || lk.n_rec < 1 || lk.n_rec > PEM_FUSED_SYSTEM_MAX_RECORDS)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 .. %d conditions and records (PEM_FUSED_SYSTEM_MAX_RECORDS)", who, PEM_FUSED_SYSTEM_MAX_RECORDS);
    if (lk.a_1 && !(std::isfinite(discharge_sigma) && discharge_sigma > 0.0))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: the discharge term needs a finite discharge_sigma > 0", who);
    if (n == 0) return PEM_OK;
    if ((n_dim > 2 && !t) || !lk.rec || !lk.span || !lk.loglik) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if ((n_dim > 2 && ld < n) || (lk.out && lk.ld_out < n)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: leading dimension smaller than n", who);
    if (lk.pred && lk.ld_pred < (size_t)lk.n_rec) return pem::fail(PEM_ERR_INVALID_ARG, "%s: ld_pred smaller than n_rec", who);
    if (int rc0 = pem::check_device()) return rc0;
    lk.inv_sigma = lk.a_1 ? 1.0 / discharge_sigma : 0.0;
    // the table, the spans and the basis go beside the coordinates where that costs no resident workgroup: the stages hold about
    // 200 VGPRs, two workgroups per CU at most, so up to half of the 160 KB each; a launch that is alone on its CU anyway may fill it
    const size_t extra = (size_t)lk.n_rec * 32 + (size_t)lk.n_cond * 32 + (lk.basis ? (size_t)PEM_NANGLE * lk.rank * sizeof(double) : 0);
    const size_t room = base <= 80 * 1024 ? 80 * 1024 : 160 * 1024;
    lk.staged = base + extra <= room;
    const size_t lds = base + (lk.staged ? extra : 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double map[4] = {vcc_lo, vcc_w, ib0_lo, ib0_w};
#define PEM_CHAIN_LL(NOUT_, EXACT_) launch_chain_loglik<NOUT_, EXACT_>(n, n_dim, vcc_slot, ib0_slot, cs, map, t, ld, basis_words, lds, lk, st)
    switch (n_plume) {
        case 1: PEM_CHAIN_LL(1, true); break;
        case 2: PEM_CHAIN_LL(2, true); break;
        case 3: PEM_CHAIN_LL(3, true); break;
        case 4: PEM_CHAIN_LL(4, true); break;
        default:
            if (n_plume <= 8) PEM_CHAIN_LL(8, false);
            else PEM_CHAIN_LL(16, false);
    }
#undef PEM_CHAIN_LL
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // namespace

extern "C" {

int pem_sparse_predict_f64_dev(size_t n, int n_dim, int n_beta, const int32_t* index, const double* coef, const double* values,
                               int n_out, const double* t, size_t ld, double* out, size_t ld_out, int max_active, int max_level,
                               pem_stream_t stream) {
    return sparse_predict("pem_sparse_predict", n, n_dim, n_beta, index, coef, values, n_out, t, ld, out, ld_out, 0, max_active, max_level,
                          Recon{}, stream);
}

int pem_sparse_grid_values_f64_dev(size_t n, int n_dim, int n_beta, const int32_t* index, const double* coef, const double* values,
                                   int n_out, const double* t, size_t ld, double* out, size_t ld_out, int max_active, int max_level,
                                   pem_stream_t stream) {
    return sparse_predict("pem_sparse_grid_values", n, n_dim, n_beta, index, coef, values, n_out, t, ld, out, ld_out, 1, max_active,
                          max_level, Recon{}, stream);
}

int pem_sparse_predict_field_f64_dev(size_t n, int n_dim, int n_beta, const int32_t* index, const double* coef, const double* values,
                                     int n_out, const double* t, size_t ld, double* out, size_t ld_out, int max_active, int max_level,
                                     int lat0, int rank, int dof, int norm, double norm_scale, const double* basis, double* field,
                                     pem_stream_t stream) {
    if (!field) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sparse_predict_field: NULL field");
    if (norm != PEM_NORM_NONE && norm != PEM_NORM_LOG10 && norm != PEM_NORM_LINEAR) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sparse_predict_field: unknown norm %d", norm);
    Recon rc{};
    rc.basis = basis;
    rc.field = field;
    rc.dof = dof;
    rc.rank = rank;
    rc.lat0 = lat0;
    rc.norm = norm;
    rc.scale = norm_scale;
    return sparse_predict("pem_sparse_predict_field", n, n_dim, n_beta, index, coef, values, n_out, t, ld, out, ld_out, 0, max_active, max_level,
                          rc, stream);
}

int pem_sparse_predict_chain_f64_dev(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                                     double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, double* out, size_t ld_out,
                                     int lat0, int rank, int dof, int norm, double norm_scale, const double* basis, double* field,
                                     pem_stream_t stream) {
    Recon rc{};
    if (field) {
        if (norm != PEM_NORM_NONE && norm != PEM_NORM_LOG10 && norm != PEM_NORM_LINEAR)
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_sparse_predict_chain: unknown norm %d", norm);
        rc.basis = basis;
        rc.field = field;
        rc.dof = dof;
        rc.rank = rank;
        rc.lat0 = lat0;
        rc.norm = norm;
        rc.scale = norm_scale;
    }
    return sparse_predict_chain(n, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, t, ld, out, ld_out, rc, stream);
}

int pem_chain_system_loglik_f64_dev(size_t n, int n_dim, int vcc_slot, int ib0_slot, const pem_surr_stage* stages, double vcc_lo,
                                    double vcc_w, double ib0_lo, double ib0_w, const double* t, size_t ld, int lat0, int rank, int dof,
                                    int norm, double norm_scale, const double* basis, int n_cond, int n_rec, const double* rec,
                                    const int32_t* span, const double* a_1, double discharge_current, double discharge_sigma,
                                    double* loglik, double* out, size_t ld_out, double* pred, size_t ld_pred, pem_stream_t stream) {
    ChainLik lk{};
    lk.basis = basis;
    lk.rec = rec;
    lk.span = span;
    lk.a_1 = a_1;
    lk.loglik = loglik;
    lk.out = out;
    lk.pred = pred;
    lk.ld_out = ld_out;
    lk.ld_pred = ld_pred;
    lk.lat0 = lat0;
    lk.rank = basis ? rank : 0;
    lk.norm = norm;
    lk.n_cond = n_cond;
    lk.n_rec = n_rec;
    lk.scale = norm_scale;
    lk.discharge = discharge_current;
    return chain_system_loglik(n, n_dim, vcc_slot, ib0_slot, stages, vcc_lo, vcc_w, ib0_lo, ib0_w, t, ld, dof, discharge_sigma, lk, stream);
}

}  // extern "C"
#endif  // PEM_SURROGATE_FIELDS_UNIT
