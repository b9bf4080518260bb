// pem_de.hip -- one generation of differential evolution over the prior's quantile cube (hallthrusterpem_amd/optimize.py).
//
// What it stands in for: `differential_evolution(..., popsize=15, vectorized=True, updating='deferred')` of run_mle
// (scripts/pem_v0/mcmc.py:170-231, optimizer='evolution').  scipy's semantics, restated for a counter-based generator:
// best1bin / rand1bin mutation, a dithered F ~ U(mut_lo, mut_hi) per generation, binomial crossover with one forced
// dimension, deferred updating, out-of-bounds components redrawn uniformly.  The search runs over u in (0, 1)^d; the
// trials are handed to the posterior as theta = pem::transform(kind, a, b, u).
//
// One workgroup holds the whole population (thread i = member i), so selection, the best member, the convergence
// statistic and the next trials are one launch with no grid-wide synchronisation.  The generation counter lives in device
// memory (`state`): a captured graph replays the same kernel arguments and still advances the generator.
//
// Every random number is Philox4x32-10 with counter (member, generation, purpose, pair) and key seed, and every reduction
// has a fixed order (a wave64 xor butterfly, then the waves in order), so tests/de_np.py restates the launch bit for bit.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_philox.h"
#include "pem_search.h"

namespace {

constexpr int MAX_POP = PEM_DE_MAX_POP;
constexpr int MAX_DIM = PEM_DE_MAX_DIM;
constexpr int MAX_WAVES = MAX_POP / 64;

// purposes (word 2 of the Philox counter)
constexpr uint32_t PURPOSE_PICK = 0;     // pair 0: words x, y, z pick r0, r1, r2; word w the forced crossover dimension
constexpr uint32_t PURPOSE_CROSS = 1;    // pair p: the crossover uniforms of dimensions 2p, 2p + 1
constexpr uint32_t PURPOSE_REDRAW = 2;   // pair p: the redraws of dimensions 2p, 2p + 1 that left (0, 1)
constexpr uint32_t PURPOSE_DITHER = 3;   // member 0, pair 0: F of the generation

struct DeTable {
    int32_t kind[MAX_DIM];
    double a[MAX_DIM], b[MAX_DIM];
};

using pem::Philox4;
using pem::philox4x32_10;
using pem::u53;
using pem::u_open;
using pem::search::transform_call;

// an integer in [0, n) from one 32-bit word (multiply-high)
__device__ __forceinline__ int below(uint32_t w, int n) { return (int)(((uint64_t)w * (uint32_t)n) >> 32); }

// NaN and -inf never win a comparison
__device__ __forceinline__ double rank_key(double f) { return f > -INFINITY ? f : -INFINITY; }

__device__ __forceinline__ void sort2(int& x, int& y) {
    const int lo = min(x, y), hi = max(x, y);
    x = lo;
    y = hi;
}

__global__ __launch_bounds__(MAX_POP) void de_step_kernel(int P, int d, int strategy, int finalize, uint32_t k0, uint32_t k1,
                                                          double mut_lo, double mut_hi, double cr, double tol, double atol,
                                                          DeTable tab, double* __restrict__ pop_u, double* __restrict__ pop_f,
                                                          double* __restrict__ trial_u, const double* __restrict__ trial_f,
                                                          double* __restrict__ theta, uint64_t* __restrict__ state,
                                                          double* __restrict__ record, double* __restrict__ history,
                                                          uint64_t history_len) {
#pragma clang fp contract(off)
    __shared__ double s_part[MAX_WAVES], s_best[MAX_WAVES];
    __shared__ int s_idx[MAX_WAVES];
    __shared__ double s_mean;
    __shared__ int s_bi;
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6, nw = blockDim.x >> 6;
    const bool live = i < P;
    const uint64_t g = *state;

    if (g == 0) {   // the initial population: the trials are the design already in trial_u, pulled inside (0, 1)
        if (finalize) return;
        if (live) {
            for (int j = 0; j < d; ++j) {
                const double u = fmin(fmax(trial_u[(size_t)i * d + j], 0x1.0p-53), 1.0 - 0x1.0p-53);
                trial_u[(size_t)i * d + j] = u;
                theta[(size_t)i * d + j] = transform_call(tab.kind[j], tab.a[j], tab.b[j], u);
            }
        }
        if (i == 0) {
            record[0] = -INFINITY;
            record[1] = -1.0;
            record[2] = 0.0;
        }
        __syncthreads();
        if (i == 0) *state = 1;
        return;
    }

    // 1. deferred selection: the trials evaluated since the last launch replace the members they beat (after the first
    //    launch they are the initial population and are taken as they are)
    double f = 0.0;
    if (live) {
        f = pop_f[i];
        const double tf = trial_f[i];
        if (g == 1 || rank_key(tf) > rank_key(f)) {
            for (int j = 0; j < d; ++j) pop_u[(size_t)i * d + j] = trial_u[(size_t)i * d + j];
            pop_f[i] = tf;
            f = tf;
        }
    }

    // 2. the best member (ties to the lowest index) and sum(f), then sum((f - mean)^2): xor butterflies, waves in order
    double bv = live ? rank_key(f) : -INFINITY, s = live ? f : 0.0;
    int bi = live ? i : INT_MAX;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
        s = s + __shfl_xor(s, m);
    }
    if (lane == 0) {
        s_part[wave] = s;
        s_best[wave] = bv;
        s_idx[wave] = bi;
    }
    __syncthreads();
    if (i == 0) {
        double tot = s_part[0], v = s_best[0];
        int k = s_idx[0];
        for (int w = 1; w < nw; ++w) {
            tot = tot + s_part[w];
            if (s_best[w] > v || (s_best[w] == v && s_idx[w] < k)) {
                v = s_best[w];
                k = s_idx[w];
            }
        }
        s_mean = tot / (double)P;
        s_bi = k;
        record[0] = v;
        record[1] = (double)k;
        if (history && g - 1 < history_len) history[g - 1] = v;
    }
    __syncthreads();
    const double mean = s_mean;
    const int best = s_bi;
    double q = 0.0;
    if (live) {
        const double dev = f - mean;
        q = dev * dev;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) q = q + __shfl_xor(q, m);
    __syncthreads();                          // every wave has read s_mean / s_bi before s_part is reused
    if (lane == 0) s_part[wave] = q;
    __syncthreads();
    if (i == 0) {
        double tot = s_part[0];
        for (int w = 1; w < nw; ++w) tot = tot + s_part[w];
        const double sd = sqrt(tot / (double)P);
        record[2] = (sd <= atol + tol * fabs(mean)) ? 1.0 : 0.0;   // NaN (a non-finite member) is never converged
    }

    if (finalize) {   // the population's theta, for the caller to read the best member from
        if (live)
            for (int j = 0; j < d; ++j)
                theta[(size_t)i * d + j] = transform_call(tab.kind[j], tab.a[j], tab.b[j], pop_u[(size_t)i * d + j]);
        return;
    }

    // 3. the next trials
    if (live) {
        const uint32_t gl = (uint32_t)g;
        const Philox4 dz = philox4x32_10(0u, gl, PURPOSE_DITHER, 0u, k0, k1);
        const double F = mut_lo + (mut_hi - mut_lo) * u53(dz.x, dz.y);
        const Philox4 pk = philox4x32_10((uint32_t)i, gl, PURPOSE_PICK, 0u, k0, k1);
        // distinct indices without rejection: a draw from the P - m indices left, shifted past the m excluded ones in order
        int r0 = below(pk.x, P - 1);
        r0 += r0 >= i;
        int e0 = i, e1 = r0;
        sort2(e0, e1);
        int r1 = below(pk.y, P - 2);
        r1 += r1 >= e0;
        r1 += r1 >= e1;
        int base = best, da = r0, db = r1;
        if (strategy == PEM_DE_RAND1BIN) {
            int e2 = r1;
            sort2(e1, e2);
            sort2(e0, e1);
            int r2 = below(pk.z, P - 3);
            r2 += r2 >= e0;
            r2 += r2 >= e1;
            r2 += r2 >= e2;
            base = r0;
            da = r1;
            db = r2;
        }
        const int fill = below(pk.w, d);
        for (int j0 = 0; j0 < d; j0 += 2) {
            const Philox4 cx = philox4x32_10((uint32_t)i, gl, PURPOSE_CROSS, (uint32_t)(j0 >> 1), k0, k1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = j0 + h;
                if (j >= d) break;
                const double uc = h == 0 ? u53(cx.x, cx.y) : u53(cx.z, cx.w);
                double x = pop_u[(size_t)i * d + j];
                if (uc < cr || j == fill) {
                    double t = pop_u[(size_t)da * d + j] - pop_u[(size_t)db * d + j];
                    t = F * t;
                    x = pop_u[(size_t)base * d + j] + t;
                }
                if (!(x > 0.0 && x < 1.0)) {
                    const Philox4 rd = philox4x32_10((uint32_t)i, gl, PURPOSE_REDRAW, (uint32_t)(j0 >> 1), k0, k1);
                    x = h == 0 ? u_open(rd.x, rd.y) : u_open(rd.z, rd.w);
                }
                trial_u[(size_t)i * d + j] = x;
                theta[(size_t)i * d + j] = transform_call(tab.kind[j], tab.a[j], tab.b[j], x);
            }
        }
    }
    __syncthreads();
    if (i == 0) *state = g + 1;
}

}  // namespace

extern "C" int pem_de_step_f64_dev(int pop, int ndim, int strategy, int finalize, uint64_t seed, double mut_lo, double mut_hi,
                                   double cr, double tol, double atol, const int32_t* kind, const double* a, const double* b,
                                   double* pop_u, double* pop_f, double* trial_u, const double* trial_f, double* theta,
                                   uint64_t* state, double* record, double* history, size_t history_len, pem_stream_t stream) {
    if (pop < 4 || pop > MAX_POP) return pem::fail(PEM_ERR_INVALID_ARG, "pem_de_step: population must be in [4, %d]", MAX_POP);
    if (ndim < 1 || ndim > MAX_DIM) return pem::fail(PEM_ERR_INVALID_ARG, "pem_de_step: ndim must be in [1, %d]", MAX_DIM);
    if (strategy != PEM_DE_BEST1BIN && strategy != PEM_DE_RAND1BIN)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_de_step: unknown strategy %d", strategy);
    if (!(cr >= 0.0 && cr <= 1.0) || !(mut_lo <= mut_hi))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_de_step: need 0 <= recombination <= 1 and mut_lo <= mut_hi");
    if (!kind || !a || !b || !pop_u || !pop_f || !trial_u || !trial_f || !theta || !state || !record)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_de_step: NULL array");
    DeTable tab;
    for (int j = 0; j < MAX_DIM; ++j) {
        tab.kind[j] = j < ndim ? kind[j] : 0;
        tab.a[j] = j < ndim ? a[j] : 0.0;
        tab.b[j] = j < ndim ? b[j] : 0.0;
        if (j < ndim && (kind[j] < 0 || kind[j] > PEM_DIST_NORMAL))
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_de_step: unknown distribution kind %d for dimension %d", kind[j], j);
    }
    if (int rc = pem::check_device()) return rc;
    const int threads = (pop + 63) / 64 * 64;
    hipLaunchKernelGGL(de_step_kernel, dim3(1), dim3(threads), 0, static_cast<hipStream_t>(stream), pop, ndim, strategy,
                       finalize ? 1 : 0, (uint32_t)seed, (uint32_t)(seed >> 32), mut_lo, mut_hi, cr, tol, atol, tab, pop_u, pop_f,
                       trial_u, trial_f, theta, state, record, history, (uint64_t)history_len);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
