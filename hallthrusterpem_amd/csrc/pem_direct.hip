// pem_direct.hip -- one launch of DIRECT with its rectangles on the device (hallthrusterpem_amd/optimize.py, `Direct`).
//
// What it stands in for: `direct(obj_fun, bds, eps=1, maxiter=maxfev, locally_biased=False)` of run_mle
// (scripts/pem_v0/mcmc.py:170-231, optimizer='direct').  scipy's DIRECT is compiled code, but wrapping the objective shows every
// point it evaluates, in order; the rules below reproduce that sequence bit for bit (tests/direct_np.py, held to scipy in
// tests/test_direct_host.py).  They are not the paper's: every step of the Pareto staircase of (size, value) is divided, and
// the eps test only eats the staircase from its small end.
//
// DIRECT is the one optimiser of the four whose iterations want many values at once, so its points fill the rows of the
// batched posterior as they are.  A launch takes the values of the rows it emitted last, completes the divisions they belong
// to, runs a selection round when the round's queue of kept anchors is empty, and emits the points of as many queued anchors
// as fit into `rows`; the concatenation of the consumed rows is scipy's evaluation sequence.  The search runs over x in
// [lb, ub]^d of the prior's quantile cube and MAXIMISES f: g = -f is what scipy's comparisons see.
//
// One search, one workgroup of 256 threads.  The launch counter and all state live in device memory, so a captured graph
// replays the same kernel arguments and still advances.  Per-level minima are integer minima in LDS over an order-preserving
// key of g, and the lowest index among the rectangles that equal the minimum is an integer minimum as well: no floating-point
// atomics, the same bits on every run.  Wave 0 walks the level table 64 levels at a time for the staircase (g is decoded from
// the key) and prunes it with a wave-wide minimum of the slopes.  Every loop is bounded by d, rows, the rectangle count or the level count, never by a
// value read from cand_f.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_philox.h"   // pem::transform, the prior transforms (no random numbers are drawn here)
#include "pem_search.h"

namespace {

constexpr int MAX_DIM = PEM_DIRECT_MAX_DIM;
constexpr int MAX_LEVELS = PEM_DIRECT_MAX_LEVELS;
constexpr int MAX_DEPTH = PEM_DIRECT_MAX_DEPTH;
constexpr int MAX_ROWS = PEM_DIRECT_MAX_ROWS;
constexpr int STATE_WORDS = PEM_DIRECT_STATE_WORDS;
constexpr int THREADS = 256;
constexpr int ROW_PAD = -1, ROW_START = -2;   // rowinfo[r][0] of a left-over row and of the start's centre

// state words
enum { W_LAUNCHES, W_NIT, W_NFEV, W_STATUS, W_Q_HEAD, W_Q_LEN, W_BEST, W_PEND, W_TIES, W_END };
static_assert(W_END + 1 == STATE_WORDS, "layout of include/pem_hip.h");

struct DirectTable {
    int32_t kind[MAX_DIM];
    double a[MAX_DIM], b[MAX_DIM], lb[MAX_DIM], ub[MAX_DIM];
};

using pem::search::transform_call;

__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }

// g = -f with -0 folded into +0, so that equal values have equal keys
__device__ __forceinline__ double cost(double f) { return -f + 0.0; }

// unsigned keys ordered as the finite doubles they come from
__device__ __forceinline__ unsigned long long key_of(double g) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(g);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double value_of(unsigned long long key) {
    return __longlong_as_double((long long)((key >> 63) ? (key & 0x7fffffffffffffffull) : ~key));
}

__global__ __launch_bounds__(THREADS) void direct_step_kernel(int d, int rows, uint64_t cap, int n_depth, int finalize, double eps,
                                                              double vol_tol, double len_tol, uint64_t max_iter, uint64_t max_fun,
                                                              DirectTable tab, const double* __restrict__ thirds,
                                                              const double* __restrict__ levels, double* __restrict__ centres,
                                                              double* __restrict__ values, int32_t* __restrict__ expo,
                                                              int32_t* __restrict__ level, int32_t* __restrict__ queue,
                                                              int32_t* __restrict__ rowinfo, const double* __restrict__ cand_f,
                                                              double* __restrict__ theta, uint64_t* __restrict__ state,
                                                              double* __restrict__ history, uint64_t history_len) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_key[MAX_LEVELS];   // per level: the key of its lowest g
    __shared__ int s_idx[MAX_LEVELS];                  // and the lowest index that has it
    __shared__ int s_kept_lv[MAX_LEVELS], s_kept_r[MAX_LEVELS];
    __shared__ double s_kept_g[MAX_LEVELS], s_kept_s[MAX_LEVELS];   // their g and size measures
    __shared__ int s_pop_r[MAX_ROWS / 2], s_pop_base[MAX_ROWS / 2];   // the anchors popped by this launch and their first rows
    __shared__ double s_xs1[MAX_DIM], s_xs2[MAX_DIM];
    __shared__ uint64_t s_w[STATE_WORDS];
    __shared__ unsigned long long s_min;
    __shared__ int s_arg, s_bad, s_ties, s_equal, s_npop, s_used;

    const int tid = threadIdx.x;
    if (tid < STATE_WORDS) s_w[tid] = state[tid];
    if (tid < d) {
        const double xs1 = tab.ub[tid] - tab.lb[tid];
        s_xs1[tid] = xs1;
        s_xs2[tid] = tab.lb[tid] / xs1;
    }
    if (tid == 0) {
        s_bad = 0, s_ties = 0, s_equal = 0, s_arg = INT_MAX, s_npop = 0, s_used = 0;
        s_min = ~0ull;
    }
    __syncthreads();
    const uint64_t launches = s_w[W_LAUNCHES];
    // the point evaluated for a centre is (c + xs2) xs1, rounded twice; the row carries its prior transform
    auto emit = [&](int j, double c) {
        const double t = c + s_xs2[j];
        return transform_call(tab.kind[j], tab.a[j], tab.b[j], t * s_xs1[j]);
    };
    const size_t elems = (size_t)rows * d;

    if (finalize) {   // consumes nothing: row 0 is the best centre's point
        const size_t best = s_w[W_BEST] < cap ? s_w[W_BEST] : cap - 1;
        if (launches >= 1 && s_w[W_NFEV] >= 1 && tid < d) theta[tid] = emit(tid, centres[best * d + tid]);
        return;
    }
    if (launches == 0) {   // the centre of the cube is emitted (every row carries it)
        for (size_t e = tid; e < elems; e += THREADS) theta[e] = emit((int)(e % d), 0.5);
        if (tid < d) centres[tid] = 0.5;
        for (int r = tid; r < rows; r += THREADS) {
            rowinfo[2 * r] = r == 0 ? ROW_START : ROW_PAD;
            rowinfo[2 * r + 1] = 0;
        }
        if (tid < STATE_WORDS) state[tid] = (tid == W_LAUNCHES || tid == W_PEND) ? 1 : 0;
        return;
    }
    if (s_w[W_STATUS] != 0) {   // frozen: every row is the best point already; only the launch counter and the history move
        if (tid == 0) {
            state[W_LAUNCHES] = launches + 1;
            if (history && launches - 1 < history_len) {
                const size_t best = s_w[W_BEST] < cap ? s_w[W_BEST] : cap - 1;
                double* h = history + (launches - 1) * PEM_DIRECT_HISTORY_COLS;
                h[0] = s_w[W_NFEV] >= 1 ? -values[best] : NAN;
                h[1] = (double)s_w[W_NFEV];
                h[2] = (double)s_w[W_NIT];
            }
        }
        return;
    }

    // ---- consume the values of the rows emitted last
    const size_t n0 = s_w[W_NFEV] < cap ? s_w[W_NFEV] : cap;
    int pend = s_w[W_PEND] < (uint64_t)rows ? (int)s_w[W_PEND] : rows;
    if ((uint64_t)pend > cap - n0) pend = (int)(cap - n0);   // (a state the caller has overwritten stays in bounds)
    for (int r = tid; r < pend; r += THREADS)
        if (!finite(cost(cand_f[r]))) atomicOr(&s_bad, 1);
    __syncthreads();
    if (s_bad) {
        if (tid == 0) s_w[W_STATUS] = 7;
    } else {
        // the children: value, exponents and level, from the parents as they still are
        for (int r = tid; r < pend; r += THREADS) {
            const double g = cost(cand_f[r]);
            values[n0 + r] = g;
            atomicMin(&s_min, key_of(g));
            const int par = rowinfo[2 * r], ss = rowinfo[2 * r + 1];
            int32_t* child = expo + (n0 + r) * d;
            if (par < 0 || (size_t)par >= n0) {   // the start's centre
                for (int j = 0; j < d; ++j) child[j] = 0;
                level[n0 + r] = 0;
                continue;
            }
            const int side = ss >> 1, sign = ss & 1;
            const int32_t* ep = expo + (size_t)par * d;
            int k = INT_MAX;
            for (int j = 0; j < d; ++j) k = ep[j] < k ? ep[j] : k;
            int pos = 0;
            for (int j = 0; j < side && j < d; ++j) pos += ep[j] == k;
            int base = r - 2 * pos - sign;
            if (base < 0) base = 0;
            const int own = base + 2 * pos < rows - 1 ? base + 2 * pos : rows - 2;
            const double wi = fmin(cost(cand_f[own]), cost(cand_f[own + 1]));
            int q = 0, kmin = INT_MAX, cnt = 0, ties = 0;
            for (int j = 0; j < d; ++j) {   // side j is divided no later than this row's side when its w sorts no later (stably)
                int e = ep[j];
                if (e == k) {
                    const int at = base + 2 * q < rows - 1 ? base + 2 * q : rows - 2;
                    const double wj = fmin(cost(cand_f[at]), cost(cand_f[at + 1]));
                    ++q;
                    if (wj < wi || (wj == wi && j <= side)) e += 1;
                    if (wj == wi && j < side) ++ties;
                }
                child[j] = e;
                if (e < kmin) kmin = e, cnt = 1;
                else if (e == kmin) ++cnt;
            }
            level[n0 + r] = kmin * d + (d - cnt);
            if (sign == 0 && ties) atomicAdd(&s_ties, ties);
        }
        __syncthreads();
        // then the parents, once each (at the first of their rows), and the lowest new index that has the lowest new value
        for (int r = tid; r < pend; r += THREADS) {
            const int par = rowinfo[2 * r];
            if (par >= 0 && (size_t)par < n0 && (r == 0 || rowinfo[2 * (r - 1)] != par)) {
                int32_t* ep = expo + (size_t)par * d;
                int k = INT_MAX;
                for (int j = 0; j < d; ++j) k = ep[j] < k ? ep[j] : k;
                int kmin = INT_MAX, cnt = 0;
                for (int j = 0; j < d; ++j) {
                    const int e = ep[j] == k ? k + 1 : ep[j];
                    ep[j] = e;
                    if (e < kmin) kmin = e, cnt = 1;
                    else if (e == kmin) ++cnt;
                }
                level[par] = kmin * d + (d - cnt);
            }
            if (key_of(values[n0 + r]) == s_min) atomicMin(&s_arg, r);
        }
        __syncthreads();
        if (tid == 0 && pend > 0) {
            const size_t best = s_w[W_BEST] < cap ? s_w[W_BEST] : cap - 1;
            if (n0 == 0 || values[n0 + s_arg] < values[best]) s_w[W_BEST] = n0 + s_arg;
            s_w[W_NFEV] = n0 + pend;
            s_w[W_TIES] += (uint64_t)s_ties;
        }
    }
    __syncthreads();

    // ---- the round has ended: the stops, then the selection
    const size_t n = s_w[W_NFEV] < cap ? s_w[W_NFEV] : cap;
    const int n_levels = n_depth * d;
    const bool round_over = s_w[W_STATUS] == 0 && s_w[W_Q_HEAD] == s_w[W_Q_LEN];
    __syncthreads();   // (every thread has read the words thread 0 changes next)
    if (round_over) {
        if (n == 1) {   // the start is divided without a selection
            if (tid == 0) {
                queue[0] = 0;
                s_w[W_Q_HEAD] = 0, s_w[W_Q_LEN] = 1;
            }
        } else {
            if (tid == 0) {
                s_w[W_Q_HEAD] = 0;
                s_w[W_NIT] += 1;
                const size_t m = s_w[W_BEST] < cap ? s_w[W_BEST] : cap - 1;
                double vol = 1.0;
                for (int i = 0; i < d; ++i) {
                    const int e = expo[m * d + i];
                    vol = vol * thirds[e < 0 ? 0 : e > n_depth ? n_depth : e];
                }
                const int lm = level[m];
                if (n > max_fun) {
                    s_w[W_STATUS] = 1;
                } else if (vol < vol_tol) {
                    s_w[W_STATUS] = 4;
                } else if (levels[lm < 0 ? 0 : lm >= n_levels ? n_levels - 1 : lm] < len_tol) {
                    s_w[W_STATUS] = 5;
                } else if (s_w[W_NIT] + 1 >= max_iter) {
                    s_w[W_STATUS] = 2;
                    s_w[W_NIT] = max_iter > 2 ? max_iter : 2;   // (scipy reports 2 for maxiter = 1 as well)
                }
            }
            __syncthreads();
            if (s_w[W_STATUS] == 0) {
                for (int l = tid; l < n_levels; l += THREADS) {
                    s_key[l] = ~0ull;
                    s_idx[l] = INT_MAX;
                }
                __syncthreads();
                for (size_t r = tid; r < n; r += THREADS) {
                    const int l = level[r];
                    atomicMin(&s_key[l < 0 ? 0 : l >= n_levels ? n_levels - 1 : l], key_of(values[r]));
                }
                __syncthreads();
                for (size_t r = tid; r < n; r += THREADS) {
                    int l = level[r];
                    l = l < 0 ? 0 : l >= n_levels ? n_levels - 1 : l;
                    if (key_of(values[r]) == s_key[l]) {
                        atomicMin(&s_idx[l], (int)r);
                        atomicAdd(&s_equal, 1);
                    }
                }
                __syncthreads();
                if (tid < 64) {   // wave 0: the staircase, 64 levels at a time, then the pruning
                    const size_t m = s_w[W_BEST] < cap ? s_w[W_BEST] : cap - 1;
                    const double gmin = values[m];
                    const unsigned long long none = ~0ull;   // (no finite g has this key)
                    int K = 0, nonempty = 0;
                    unsigned long long below = none;
                    for (int l0 = 0; l0 < n_levels; l0 += 64) {   // kept: strictly below every anchor before it
                        const int l = l0 + tid;
                        const unsigned long long key = l < n_levels ? s_key[l] : none;
                        unsigned long long upto = key;   // the lowest key of this lane and the ones before it
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const unsigned long long v = __shfl_up(upto, o);
                            if (tid >= o && v < upto) upto = v;
                        }
                        unsigned long long before = __shfl_up(upto, 1);
                        if (tid == 0 || below < before) before = below;
                        const bool keep = key != none && key < before;
                        const unsigned long long mask = __ballot(keep);
                        nonempty += __popcll(__ballot(key != none));
                        if (keep) {
                            const int at = K + __popcll(mask & ((1ull << tid) - 1ull));
                            s_kept_lv[at] = l, s_kept_r[at] = s_idx[l];
                            s_kept_g[at] = value_of(key), s_kept_s[at] = levels[l];
                        }
                        K += __popcll(mask);
                        const unsigned long long all = __shfl(upto, 63);
                        if (all < below) below = all;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const double slack = eps * fabs(gmin);
                    const double bound = gmin - slack;
                    while (K > 1) {   // eps eats the staircase from its small end (the same K in every lane)
                        const double gj = s_kept_g[K - 1], sj = s_kept_s[K - 1];
                        double lo = INFINITY;
                        for (int i = tid; i < K - 1; i += 64) {
                            const double num = s_kept_g[i] - gj;
                            const double den = s_kept_s[i] - sj;
                            lo = fmin(lo, num / den);
                        }
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) lo = fmin(lo, __shfl_xor(lo, o));
                        const double prod = lo * sj;
                        if (gj - prod > bound) --K;
                        else break;
                    }
                    int total = 0, deep = 0;
                    for (int i = tid; i < K; i += 64) {
                        total += 2 * (d - s_kept_lv[i] % d);
                        deep |= s_kept_lv[i] / d + 2 > n_depth;
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        total += __shfl_xor(total, o);
                        deep |= __shfl_xor(deep, o);
                    }
                    const bool fits = !deep && n + (size_t)total <= cap;   // else the level table or the store cannot hold the round
                    if (fits)
                        for (int i = tid; i < K; i += 64) queue[i] = s_kept_r[i];
                    if (tid == 0) {
                        s_w[W_TIES] += (uint64_t)(s_equal - nonempty);
                        if (fits) s_w[W_Q_LEN] = (uint64_t)K;
                        else s_w[W_STATUS] = 6;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- emit: pop the kept anchors whose points still fit
    if (tid == 0 && s_w[W_STATUS] == 0) {
        int used = 0, npop = 0;
        uint64_t head = s_w[W_Q_HEAD];
        const uint64_t len = s_w[W_Q_LEN] < (uint64_t)MAX_LEVELS ? s_w[W_Q_LEN] : MAX_LEVELS;
        while (head < len) {
            const int r = queue[head];
            if (r < 0 || (size_t)r >= n) break;
            const int cnt = 2 * (d - level[r] % d);
            if (cnt < 2 || used + cnt > rows || n + used + cnt > cap) break;
            s_pop_r[npop] = r, s_pop_base[npop] = used;
            ++npop, ++head;
            used += cnt;
        }
        s_w[W_Q_HEAD] = head;
        s_npop = npop, s_used = used;
    }
    __syncthreads();
    const int used = s_used;
    for (int m = tid; m < s_npop; m += THREADS) {   // + and - of every side at the anchor's lowest exponent, ascending
        const int r = s_pop_r[m];
        const int k = level[r] / d;
        int at = s_pop_base[m];
        for (int j = 0; j < d; ++j) {
            if (expo[(size_t)r * d + j] != k || at + 1 >= rows) continue;
            rowinfo[2 * at] = r, rowinfo[2 * at + 1] = 2 * j;
            rowinfo[2 * at + 2] = r, rowinfo[2 * at + 3] = 2 * j + 1;
            at += 2;
        }
    }
    for (int r = used + tid; r < rows; r += THREADS) {
        rowinfo[2 * r] = ROW_PAD;
        rowinfo[2 * r + 1] = 0;
    }
    __syncthreads();
    const size_t best = s_w[W_BEST] < cap ? s_w[W_BEST] : cap - 1;
    for (size_t e = tid; e < elems; e += THREADS) {
        const int t = (int)(e / d), j = (int)(e % d);
        if (t < used) {
            const int par = rowinfo[2 * t], ss = rowinfo[2 * t + 1];
            double c = centres[(size_t)par * d + j];
            if (j == (ss >> 1)) {
                const int k = level[par] / d;
                const double delta = thirds[k < 0 ? 1 : k < n_depth ? k + 1 : n_depth];
                c = (ss & 1) ? c - delta : c + delta;
            }
            centres[(n + t) * d + j] = c;
            theta[e] = emit(j, c);
        } else if (n >= 1) {   // left-over rows: a copy of the best point
            theta[e] = emit(j, centres[best * d + j]);
        }
    }
    if (tid == 0) {
        s_w[W_PEND] = (uint64_t)used;
        s_w[W_LAUNCHES] = launches + 1;
        if (s_w[W_STATUS] != 0) s_w[W_END] = launches + 1;   // the launch that ended the search
        for (int k = 0; k < STATE_WORDS; ++k) state[k] = s_w[k];
        if (history && launches - 1 < history_len) {
            double* h = history + (launches - 1) * PEM_DIRECT_HISTORY_COLS;
            h[0] = n >= 1 ? -values[best] : NAN;
            h[1] = (double)s_w[W_NFEV];
            h[2] = (double)s_w[W_NIT];
        }
    }
}

}  // namespace

extern "C" int pem_direct_step_f64_dev(int ndim, int rows, size_t cap, int n_depth, int finalize, double eps, double vol_tol,
                                       double len_tol, uint64_t max_iter, uint64_t max_fun, const int32_t* kind, const double* a,
                                       const double* b, const double* lb, const double* ub, const double* thirds,
                                       const double* levels, double* centres, double* values, int32_t* expo, int32_t* level,
                                       int32_t* queue, int32_t* rowinfo, const double* cand_f, double* theta, uint64_t* state,
                                       double* history, size_t history_len, pem_stream_t stream) {
    if (ndim < 1 || ndim > MAX_DIM) return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: ndim must be in [1, %d]", MAX_DIM);
    if (rows < 2 * ndim || rows > MAX_ROWS)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: rows must be in [2 ndim, %d]", MAX_ROWS);
    if (cap < (size_t)(2 * ndim + 1) || cap > (size_t)PEM_DIRECT_MAX_STORE)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: cap must be in [2 ndim + 1, %d]", PEM_DIRECT_MAX_STORE);
    if (n_depth < 2 || n_depth > MAX_DEPTH || n_depth * ndim > MAX_LEVELS)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: n_depth must be in [2, %d] with n_depth ndim <= %d", MAX_DEPTH,
                         MAX_LEVELS);
    if (finalize < 0 || finalize > 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: finalize must be 0 or 1");
    if (!(eps >= 0.0) || !(eps < INFINITY)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: eps must be finite and >= 0");
    if (!(vol_tol >= 0.0 && vol_tol <= 1.0) || !(len_tol >= 0.0 && len_tol <= 1.0))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: vol_tol and len_tol must be in [0, 1]");
    if (max_iter < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: max_iter must be >= 1");
    if (!kind || !a || !b || !lb || !ub || !thirds || !levels || !centres || !values || !expo || !level || !queue || !rowinfo ||
        !cand_f || !theta || !state)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: NULL array");
    if (history && history_len == 0)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: a history needs history_len >= 1");
    DirectTable tab;
    for (int j = 0; j < MAX_DIM; ++j) {
        tab.kind[j] = j < ndim ? kind[j] : 0;
        tab.a[j] = j < ndim ? a[j] : 0.0;
        tab.b[j] = j < ndim ? b[j] : 0.0;
        tab.lb[j] = j < ndim ? lb[j] : 0.0;
        tab.ub[j] = j < ndim ? ub[j] : 1.0;
        if (j < ndim && (kind[j] < 0 || kind[j] > PEM_DIST_NORMAL))
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: unknown distribution kind %d for dimension %d", kind[j], j);
        if (j < ndim && !(lb[j] < ub[j] && lb[j] > -INFINITY && ub[j] < INFINITY))
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_direct_step: lb >= ub (or not finite) for dimension %d", j);
    }
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(direct_step_kernel, dim3(1), dim3(THREADS), 0, static_cast<hipStream_t>(stream), ndim, rows, (uint64_t)cap,
                       n_depth, finalize, eps, vol_tol, len_tol, max_iter, max_fun, tab, thirds, levels, centres, values, expo,
                       level, queue, rowinfo, cand_f, theta, state, history, (uint64_t)history_len);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
