// pem_sampler.hip -- counter-based input samplers for the Monte-Carlo / Latin-hypercube / Saltelli loops.
//
// What it stands in for: `system.sample_inputs(N, normalize=True, use_pdf=[...])` of scripts/gen_data.py:238
// and the `(Ns, Nx)` sampling of scripts/pem_v0/monte_carlo.py:63-300 / sobol.py:46-66.  Those live in amisc /
// uqtils (third-party, absent from the reference tree), so parity is UNPINNED here: the formulas below are this
// library's own and are checked against a numpy restatement (oracle/sampler_np.py), not against the reference.
//
// Every value is a pure function of (seed, stream, global sample index, dimension): Philox4x32-10 with
//   counter = (index_lo, index_hi, dimension pair, stream), key = (seed_lo, seed_hi),
// so a batch can be generated in any sharding over GPUs and any batch size and is always the same batch.
// One Philox call yields 4 x 32 bits = two 53-bit uniforms = dimensions 2b and 2b+1.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_philox.h"
#include "pem_search.h"

namespace {

constexpr int MAXDIM = PEM_SAMPLE_MAX_DIM;

struct DimTable {
    int32_t kind[MAXDIM];
    double a[MAXDIM], b[MAXDIM];
};

using pem::Philox4;
using pem::philox4x32_10;
using pem::u53;
using pem::search::transform_call;   // out of line: inlined, pem::transform costs the kernel 438 registers (one wave per SIMD)

// keyed bijection of [0, n): 4-round Feistel network on 2*h bits with cycle walking (Latin-hypercube strata)
__device__ __forceinline__ uint64_t feistel_permute(uint64_t i, uint64_t n, int half_bits, uint32_t k0, uint32_t k1,
                                                    uint32_t dim) {
    const uint64_t mask = (1ull << half_bits) - 1;
    do {
        uint64_t l = i >> half_bits, r = i & mask;
#pragma unroll
        for (int round = 0; round < 4; ++round) {
            const Philox4 f = philox4x32_10((uint32_t)r, (uint32_t)(r >> 32), dim, 0x4C485300u + round, k0, k1);
            const uint64_t t = l ^ ((((uint64_t)f.y << 32) | f.x) & mask);
            l = r;
            r = t;
        }
        i = (l << half_bits) | r;
    } while (i >= n);
    return i;
}

// mode: 0 Monte-Carlo, 1 Latin hypercube over n_total strata.  swap_dim: Saltelli blocks -- dimension `swap_dim`
// (or every dimension if swap_dim == -2) is drawn from stream+1 instead of stream; -1 = plain.
__global__ __launch_bounds__(256) void sample_kernel(long long n, uint64_t first, uint64_t seed, uint32_t stream,
                                                     int ndim, DimTable tab, int mode, uint64_t n_total, int half_bits,
                                                     int swap_dim, double* __restrict__ out, size_t ld, int tiled) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t g = first + (uint64_t)i;
        // SoA: out[d][i] with leading dimension ld.  Tile-interleaved (pem_sample_tiled_f64_dev): [i / 64][d][i % 64], the
        // layout pem_coupled_tiled_f64_dev reads -- one contiguous ndim x 512-byte block per 64-sample tile.
        double* row = tiled ? out + (size_t)(i >> 6) * ((size_t)ndim * 64) + (size_t)(i & 63) : out + i;
        const size_t dstride = tiled ? 64 : ld;
        for (int d0 = 0; d0 < ndim; d0 += 2) {
            // one Philox call serves both dimensions of the pair unless a Saltelli block draws them from different
            // streams (a wave-uniform choice)
            const uint32_t st0 = stream + ((swap_dim == -2 || swap_dim == d0) ? 1u : 0u);
            const uint32_t st1 = stream + ((swap_dim == -2 || swap_dim == d0 + 1) ? 1u : 0u);
            const Philox4 r0 = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)(d0 >> 1), st0, k0, k1);
            Philox4 r1 = r0;
            if (st1 != st0) r1 = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)(d0 >> 1), st1, k0, k1);
            double u[2] = {u53(r0.x, r0.y), u53(r1.z, r1.w)};
            if (mode == 1) {   // stratum pi_d(g) of n_total, jittered by u
                u[0] = ((double)feistel_permute(g, n_total, half_bits, k0, k1 ^ st0, (uint32_t)d0) + u[0]) / (double)n_total;
                if (d0 + 1 < ndim)
                    u[1] = ((double)feistel_permute(g, n_total, half_bits, k0, k1 ^ st1, (uint32_t)(d0 + 1)) + u[1]) / (double)n_total;
            }
            row[(size_t)d0 * dstride] = transform_call(tab.kind[d0], tab.a[d0], tab.b[d0], u[0]);
            if (d0 + 1 < ndim) row[(size_t)(d0 + 1) * dstride] = transform_call(tab.kind[d0 + 1], tab.a[d0 + 1], tab.b[d0 + 1], u[1]);
        }
    }
}

int launch(size_t n, uint64_t first, uint64_t seed, uint32_t stream, int ndim, const int32_t* kind, const double* a,
           const double* b, int mode, uint64_t n_total, int swap_dim, double* out, size_t ld, hipStream_t st, int tiled = 0) {
    if (ndim < 1 || ndim > MAXDIM) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample: ndim must be in [1, %d]", MAXDIM);
    if (!kind || !a || !b || !out) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample: NULL array");
    if (!tiled && ld < n) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample: leading dimension smaller than n");
    if (swap_dim < -2 || swap_dim >= ndim) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample: swap_dim out of range");
    for (int d = 0; d < ndim; ++d)
        if (kind[d] < 0 || kind[d] > PEM_DIST_NORMAL)
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample: unknown distribution kind %d for dimension %d", kind[d], d);
    if (mode == 1 && (n_total == 0 || first > n_total || n > n_total - first))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample_lhs: indices exceed n_total");
    if (n == 0) return PEM_OK;
    if (int rc = pem::check_device()) return rc;
    DimTable tab;
    for (int d = 0; d < MAXDIM; ++d) {
        tab.kind[d] = d < ndim ? kind[d] : 0;
        tab.a[d] = d < ndim ? a[d] : 0.0;
        tab.b[d] = d < ndim ? b[d] : 0.0;
    }
    int half_bits = 1;
    if (mode == 1)
        while ((1ull << (2 * half_bits)) < n_total) ++half_bits;
    size_t blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (long long)n, first, seed, stream, ndim, tab,
                       mode, n_total, half_bits, swap_dim, out, ld, tiled);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // namespace

extern "C" {

int pem_sample_tiled_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int ndim, const int32_t* kind,
                             const double* a, const double* b, int swap_dim, double* out, pem_stream_t stream) {
    return launch(n, first_index, seed, stream_id, ndim, kind, a, b, 0, 0, swap_dim, out, 0, static_cast<hipStream_t>(stream), 1);
}

int pem_sample_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int ndim, const int32_t* kind,
                       const double* a, const double* b, int swap_dim, double* out, size_t ld, pem_stream_t stream) {
    return launch(n, first_index, seed, stream_id, ndim, kind, a, b, 0, 0, swap_dim, out, ld, static_cast<hipStream_t>(stream));
}

int pem_sample_lhs_f64_dev(size_t n, uint64_t first_index, uint64_t n_total, uint64_t seed, uint32_t stream_id, int ndim,
                           const int32_t* kind, const double* a, const double* b, double* out, size_t ld,
                           pem_stream_t stream) {
    return launch(n, first_index, seed, stream_id, ndim, kind, a, b, 1, n_total, -1, out, ld, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Saltelli accumulation: the per-batch sums behind the Sobol' estimators of hallthrusterpem_amd/drivers.py, one pass.
//   fAB == NULL : out[b][q][0] += sum f_A + f_B,   out[b][q][1] += sum f_A^2 + f_B^2          (mean / variance)
//   fAB != NULL : out[b][q][0] += sum f_B (f_AB - f_A),  out[b][q][1] += sum (f_A - f_AB)^2    (S1_d / ST_d)
// Inputs are [nq][ld] row-major; every workgroup writes its own partial (deterministic), summed by the caller.
// ---------------------------------------------------------------------------------------------------------------
namespace {

constexpr int SOBOL_BLOCK = 256;
constexpr int SOBOL_MAXQ = 8;

__global__ __launch_bounds__(SOBOL_BLOCK) void sobol_partial_kernel(long long m, int nq, size_t ld,
                                                                    const double* __restrict__ fA,
                                                                    const double* __restrict__ fB,
                                                                    const double* __restrict__ fAB,
                                                                    double* __restrict__ partial) {
    __shared__ double red[2 * SOBOL_MAXQ][SOBOL_BLOCK / 64];
    double s0[SOBOL_MAXQ], s1[SOBOL_MAXQ];
#pragma unroll
    for (int q = 0; q < SOBOL_MAXQ; ++q) s0[q] = s1[q] = 0.0;
    const long long stride = (long long)gridDim.x * SOBOL_BLOCK;
    for (long long i = (long long)blockIdx.x * SOBOL_BLOCK + threadIdx.x; i < m; i += stride) {
#pragma unroll
        for (int q = 0; q < SOBOL_MAXQ; ++q) {
            if (q < nq) {
                const double a = fA[(size_t)q * ld + i], b = fB[(size_t)q * ld + i];
                if (fAB) {
                    const double ab = fAB[(size_t)q * ld + i];
                    s0[q] = fma(b, ab - a, s0[q]);
                    s1[q] = fma(a - ab, a - ab, s1[q]);
                } else {
                    s0[q] += a + b;
                    s1[q] = fma(a, a, fma(b, b, s1[q]));
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < SOBOL_MAXQ; ++q) {
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
            s0[q] += __shfl_xor(s0[q], msk);
            s1[q] += __shfl_xor(s1[q], msk);
        }
        if (lane == 0) {
            red[2 * q][wave] = s0[q];
            red[2 * q + 1][wave] = s1[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * nq) {
        double t = 0.0;
        for (int w = 0; w < SOBOL_BLOCK / 64; ++w) t += red[threadIdx.x][w];
        partial[(size_t)blockIdx.x * 2 * nq + threadIdx.x] = t;      // [block][q][2]
    }
}

}  // namespace

extern "C" int pem_sobol_partial_f64_dev(size_t m, int nq, size_t ld, const double* fA, const double* fB, const double* fAB,
                                         double* partial, int n_blocks, pem_stream_t stream) {
    if (nq < 1 || nq > SOBOL_MAXQ) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sobol_partial: 1 <= nq <= %d", SOBOL_MAXQ);
    if (n_blocks < 1 || !fA || !fB || !partial || ld < m) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sobol_partial: bad arguments");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(sobol_partial_kernel, dim3((unsigned)n_blocks), dim3(SOBOL_BLOCK), 0, static_cast<hipStream_t>(stream),
                       (long long)m, nq, ld, fA, fB, fAB, partial);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Predictive checks (hallthrusterpem_amd/predictive.py; scripts/pem_v0/monte_carlo.py:42-60,63-300): the inputs of
// n_draws x n_cond samples -- the design's draws, each condition's operating row, theta drawn from a posterior table or
// kept from the prior -- and a Gaussian-noise copy of the predictions, both counter-based (oracle/sampler_np.py restates them).
// ---------------------------------------------------------------------------------------------------------------
namespace {

constexpr int PRED_DIM = 15;     // the coupled inputs, in COUPLED_INPUTS order
constexpr int PRED_OP_ROWS[3] = {0, 1, 6};   // P_b, V_a, mdot_a: columns 0, 1, 2 of an operating row

struct PredTable {
    int32_t kind[PRED_DIM];
    double a[PRED_DIM], b[PRED_DIM];
    int32_t role[PRED_DIM];      // -1: the design's draw;  0..2: operating column;  3 + j: column j of the theta table
};

__global__ __launch_bounds__(256) void predictive_inputs_kernel(long long n, int n_cond, uint64_t first, uint64_t seed,
                                                                uint32_t stream, PredTable tab, const double* __restrict__ op,
                                                                const double* __restrict__ samples, uint64_t n_samples,
                                                                int n_theta, uint32_t theta_stream, double* __restrict__ out,
                                                                size_t ld) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t g = first + (uint64_t)i;
        const int c = (int)(i % n_cond);
        uint64_t idx = 0;   // PEM_PREDICTIVE_THETA_INDEX: the multiply-high of the first Philox word by S
        if (samples) idx = ((uint64_t)philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, theta_stream, k0, k1).x * n_samples) >> 32;
        for (int d0 = 0; d0 < PRED_DIM; d0 += 2) {
            const bool draw0 = tab.role[d0] < 0 || (tab.role[d0] >= 3 && !samples);
            const bool draw1 = d0 + 1 < PRED_DIM && (tab.role[d0 + 1] < 0 || (tab.role[d0 + 1] >= 3 && !samples));
            Philox4 r{0, 0, 0, 0};
            if (draw0 || draw1) r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)(d0 >> 1), stream, k0, k1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int d = d0 + h;
                if (d >= PRED_DIM) break;
                const int role = tab.role[d];
                double v;
                if (h == 0 ? draw0 : draw1) v = transform_call(tab.kind[d], tab.a[d], tab.b[d], h == 0 ? u53(r.x, r.y) : u53(r.z, r.w));
                else if (role < 3) v = op[3 * c + role];
                else v = samples[idx * (uint64_t)n_theta + (uint64_t)(role - 3)];
                out[(size_t)d * ld + (size_t)i] = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void predictive_noise_kernel(long long n_rows, int m, const double* __restrict__ pred,
                                                               size_t ld_pred, const double* __restrict__ sigma, uint64_t first,
                                                               uint64_t seed, uint32_t stream, double* __restrict__ out,
                                                               size_t ld_out) {
    const long long total = n_rows * (long long)m;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long s = i / m;
        const int j = (int)(i - s * m);
        const uint64_t g = first + (uint64_t)s;
        const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)j, stream, k0, k1);
        out[(size_t)s * ld_out + j] = pred[(size_t)s * ld_pred + j] + transform_call(PEM_DIST_NORMAL, 0.0, sigma[j], u53(r.x, r.y));
    }
}

unsigned grid_for(long long total) {
    long long blocks = (total + 255) / 256;
    return (unsigned)(blocks > 256 * 16 ? 256 * 16 : blocks);
}

}  // namespace

extern "C" int pem_predictive_inputs_f64_dev(size_t n, int n_cond, uint64_t first_index, uint64_t seed, uint32_t stream_id,
                                             const int32_t* kind, const double* a, const double* b, const double* operating,
                                             const double* samples, size_t n_samples, int n_theta, const int32_t* theta_rows,
                                             uint32_t theta_stream, double* out, size_t ld, pem_stream_t stream) {
    if (n_cond < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_inputs: n_cond must be >= 1");
    if (n_theta < 0 || n_theta > PRED_DIM || (n_theta > 0 && !theta_rows))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_inputs: 0 <= n_theta <= %d with its rows", PRED_DIM);
    if (samples && (n_samples < 1 || n_samples > 0xFFFFFFFFull || n_theta < 1))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_inputs: a theta table needs 1 <= S < 2^32 rows and n_theta >= 1");
    if (!kind || !a || !b || !operating || !out) return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_inputs: NULL array");
    if (ld < n) return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_inputs: leading dimension smaller than n");
    PredTable tab;
    for (int d = 0; d < PRED_DIM; ++d) {
        if (kind[d] < 0 || kind[d] > PEM_DIST_NORMAL)
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_inputs: unknown distribution kind %d for dimension %d", kind[d], d);
        tab.kind[d] = kind[d];
        tab.a[d] = a[d];
        tab.b[d] = b[d];
        tab.role[d] = -1;
    }
    for (int k = 0; k < 3; ++k) tab.role[PRED_OP_ROWS[k]] = k;
    for (int j = 0; j < n_theta; ++j) {
        const int d = theta_rows[j];
        if (d < 0 || d >= PRED_DIM || tab.role[d] != -1)
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_inputs: theta row %d is not a free input (or repeated)", d);
        tab.role[d] = 3 + j;
    }
    if (n == 0) return PEM_OK;
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(predictive_inputs_kernel, dim3(grid_for((long long)n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (long long)n, n_cond, first_index, seed, stream_id, tab, operating, samples, (uint64_t)n_samples, n_theta,
                       theta_stream, out, ld);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

extern "C" int pem_predictive_noise_f64_dev(size_t n_rows, int m, const double* pred, size_t ld_pred, const double* sigma,
                                            uint64_t first_row, uint64_t seed, uint32_t stream_id, double* out, size_t ld_out,
                                            pem_stream_t stream) {
    if (m < 0 || ld_pred < (size_t)m || ld_out < (size_t)m)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_noise: m >= 0 and leading dimensions >= m");
    if (n_rows == 0 || m == 0) return PEM_OK;
    if (!pred || !sigma || !out) return pem::fail(PEM_ERR_INVALID_ARG, "pem_predictive_noise: NULL array");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(predictive_noise_kernel, dim3(grid_for((long long)n_rows * m)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), (long long)n_rows, m, pred, ld_pred, sigma, first_row, seed, stream_id,
                       out, ld_out);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
