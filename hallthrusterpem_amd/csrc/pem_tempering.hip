// pem_tempering.hip -- one half-step of replica exchange (parallel tempering) over the affine-invariant ensemble sampler, for R
// replicas of a ladder of T tempered ensembles of K walkers (hallthrusterpem_amd/calibration.py, DeviceTemperedEnsemble).
//
// Ensemble e = r T + t of replica r samples prior(x) likelihood(x)^beta_t, 1 = beta_0 > beta_1 > ... >= 0.  Its moves are
// pem_ensemble.hip's (pem_ensemble_moves.h: the same draws, the same log q, the same half-step order, the ensemble index e in the
// counter), judged by the tempered ratio: walker w takes y iff its new loglik and logprior are both finite and
//   log(u_acc) < (log q + (pi_new - pi_old)) + beta_t (l_new - l_old)
// so that beta l is never 0 inf (the starts are finite, a value that is not finite never enters).  log q = (d - 1) log z takes
// its log through log_restatable, IEEE operations that tests/tempering_np.py repeats, so that every state word of a launch is
// held bit for bit; the library log that pem_ensemble.hip asks differs from it (and from numpy's) in the last bit now and then.
// With T = 1 and pi = 0 the launch visits pem_ensemble_step_f64_dev's points for finite values: a decision could differ only
// where its two sides tie within that bit.
//
// Swaps, deterministic even-odd: launch s = state[r] resolves half-step s; when s is even, step n = s / 2 (n = 1, 2, ...) has
// ended and the pairs (t, t + 1) with t = n mod 2, n mod 2 + 2, ... are visited -- every ensemble is in at most one pair, the top of
// the ladder idles when its pair is not due.  Walker k of t is paired with walker k of t + 1 (the walkers of an ensemble are
// exchangeable) and the two exchange theta, loglik and logprior iff
//   log(u_swap) < (beta_t - beta_{t+1}) (l_{t+1,k} - l_{t,k})
// u_swap = u53(x, y) of Philox(counter = (r T + t, n mod 2^32, 0x454E0003, k), key = seed): the purpose word keeps it apart from
// the move draws.  beta stays with the ensemble.  Then the trace row, then the proposals of half-step s + 1, which read the
// ladder as the swaps left it.
//
// The swap reads the resolved state of two ensembles and the proposals read what it wrote, so ONE workgroup of 256 owns a whole
// replica's ladder (grid = R) and every phase -- decide, commit, swap, trace, propose -- is separated by __syncthreads() only: no
// atomics, no spinning, nothing crosses workgroups, the same bits on every run.  Each phase loops the flattened (ensemble, walker
// [, dimension]) index over as many ensembles of the ladder as the LDS tables hold at once (MAX_HALF moving walkers: the whole
// ladder when T H <= 512), so a short ladder of small ensembles costs the phases of one ensemble.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_ensemble_moves.h"
#include "pem_hip.h"
#include "pem_philox.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int MAX_HALF = PEM_ENSEMBLE_MAX_WALKERS / 2;

using pem::Philox4;
using pem::philox4x32_10;
using pem::u53;
using pem::ens::DRAW_COLS;
using pem::ens::PURPOSE_ACCEPT;
using pem::ens::PURPOSE_MOVE;
using pem::ens::PURPOSE_SWAP;

__global__ __launch_bounds__(THREADS) void tempered_ensemble_step_kernel(
    int T, int K, int d, uint32_t k0, uint32_t k1, double a, double de_fraction, double g0, double sigma, const double* beta,
    uint64_t trace_first, uint64_t trace_len, uint64_t thin, double* theta, double* loglik, double* logprior, double* prop,
    const double* prop_loglik, const double* prop_logprior, double* log_q, uint64_t* state, uint64_t* accepted,
    uint64_t* swap_attempts, uint64_t* swap_accepted, double* trace, double* loglik_trace, double* logprior_trace, double* draws) {
#pragma clang fp contract(off)
    __shared__ double s_coef[MAX_HALF];          // z (stretch) or g (DE) of the moving walkers of the ensembles in flight
    __shared__ int s_j1[MAX_HALF], s_j2[MAX_HALF];
    __shared__ int s_acc[2 * MAX_HALF];          // accept flags of a half (per moving walker) or of a swap (per walker pair)
    const size_t r = blockIdx.x, E = (size_t)gridDim.x * (size_t)T, e0 = r * (size_t)T;
    const int tid = threadIdx.x;
    const int H = K >> 1;
    const size_t KK = (size_t)K, HH = (size_t)H, dd = (size_t)d;
    const uint64_t s = state[r];
    const int per_pass = MAX_HALF / H;           // ensembles whose moving halves fit the tables together (>= 1)

    if (s >= 1) {                                // uniform over the workgroup, as every condition around a barrier below
        const int base = (int)((s - 1) & 1) * H;
        for (int t0 = 0; t0 < T; t0 += per_pass) {
            const int nt = min(per_pass, T - t0);
            // ---- the decisions of half-step s: thread per moving walker
            for (int i = tid; i < nt * H; i += THREADS) {
                const int c = i / H, m = i - c * H;
                const size_t e = e0 + (size_t)(t0 + c);
                const Philox4 x = philox4x32_10((uint32_t)e, (uint32_t)s, PURPOSE_ACCEPT, (uint32_t)m, k0, k1);
                const double u = u53(x.x, x.y);
                const size_t w = e * KK + (size_t)(base + m), p = e * HH + (size_t)m;
                const double l_new = prop_loglik[p], p_new = prop_logprior[p];
                const bool acc = isfinite(l_new) && isfinite(p_new) &&
                                 log(u) < (log_q[p] + (p_new - logprior[w])) + beta[t0 + c] * (l_new - loglik[w]);
                s_acc[i] = acc ? 1 : 0;
                if (acc) {
                    loglik[w] = l_new;
                    logprior[w] = p_new;
                    accepted[w] += 1;
                }
                if (draws) draws[p * DRAW_COLS + 4] = u;
            }
            __syncthreads();
            // ---- commit: the accepted proposals become the walkers' points
            for (int i = tid; i < nt * H * d; i += THREADS) {
                const int c = i / (H * d), rem = i - c * H * d;
                const size_t e = e0 + (size_t)(t0 + c);
                if (s_acc[c * H + rem / d]) theta[(e * KK + (size_t)base) * dd + (size_t)rem] = prop[e * HH * dd + (size_t)rem];
            }
            __syncthreads();
        }

        if ((s & 1) == 0) {
            const uint64_t n = s / 2;            // the step that has ended
            // ---- the swaps of step n: pairs (t, t + 1), t = n mod 2, n mod 2 + 2, ...
            const int t_first = (int)(n & 1), n_pairs = (T - t_first) / 2;
            const int pairs_per_pass = (2 * MAX_HALF) / K;
            for (int p0 = 0; p0 < n_pairs; p0 += pairs_per_pass) {
                const int np = min(pairs_per_pass, n_pairs - p0);
                for (int i = tid; i < np * K; i += THREADS) {
                    const int c = i / K, k = i - c * K, t = t_first + 2 * (p0 + c);
                    const size_t e = e0 + (size_t)t, lo = e * KK + (size_t)k, hi = lo + KK;
                    const Philox4 x = philox4x32_10((uint32_t)e, (uint32_t)n, PURPOSE_SWAP, (uint32_t)k, k0, k1);
                    const double l_lo = loglik[lo], l_hi = loglik[hi];
                    const bool acc = log(u53(x.x, x.y)) < (beta[t] - beta[t + 1]) * (l_hi - l_lo);
                    s_acc[i] = acc ? 1 : 0;
                    if (acc) {
                        const double p_lo = logprior[lo];
                        loglik[lo] = l_hi;
                        loglik[hi] = l_lo;
                        logprior[lo] = logprior[hi];
                        logprior[hi] = p_lo;
                    }
                }
                __syncthreads();
                for (int i = tid; i < np * K * d; i += THREADS) {
                    const int c = i / (K * d), rem = i - c * K * d;
                    if (s_acc[c * K + rem / d]) {
                        const size_t lo = (e0 + (size_t)(t_first + 2 * (p0 + c))) * KK * dd + (size_t)rem, hi = lo + KK * dd;
                        const double x_lo = theta[lo];
                        theta[lo] = theta[hi];
                        theta[hi] = x_lo;
                    }
                }
                // the counters of (replica, lower temperature): a wave per pair adds up its flags
                for (int c = tid / WAVE; c < np; c += THREADS / WAVE) {
                    int got = 0;
                    for (int k = tid % WAVE; k < K; k += WAVE) got += s_acc[c * K + k];
                    for (int off = WAVE / 2; off > 0; off >>= 1) got += __shfl_xor(got, off);
                    if (tid % WAVE == 0) {
                        const size_t q = r * (size_t)(T - 1) + (size_t)(t_first + 2 * (p0 + c));
                        swap_attempts[q] += (uint64_t)K;
                        swap_accepted[q] += (uint64_t)got;
                    }
                }
                __syncthreads();
            }
            // ---- the trace row of the whole ladder, as the swaps left it, when it is due
            if (n - 1 >= trace_first) {
                const uint64_t q = n - 1 - trace_first;
                if (q % thin == 0 && q / thin < trace_len) {
                    const size_t row = (size_t)(q / thin) * E + e0;
                    if (trace)
                        for (int i = tid; i < T * K * d; i += THREADS) trace[row * KK * dd + (size_t)i] = theta[e0 * KK * dd + (size_t)i];
                    if (loglik_trace)
                        for (int i = tid; i < T * K; i += THREADS) loglik_trace[row * KK + (size_t)i] = loglik[e0 * KK + (size_t)i];
                    if (logprior_trace)
                        for (int i = tid; i < T * K; i += THREADS) logprior_trace[row * KK + (size_t)i] = logprior[e0 * KK + (size_t)i];
                }
            }
        }
    }

    // ---- the proposals of half-step s + 1: the halves that move, against their complements as they now stand
    const int mb = (int)(s & 1) * H, cb = H - mb;
    for (int t0 = 0; t0 < T; t0 += per_pass) {
        const int nt = min(per_pass, T - t0);
        for (int i = tid; i < nt * H; i += THREADS) {
            const int c = i / H, m = i - c * H;
            const size_t e = e0 + (size_t)(t0 + c);
            const Philox4 x = philox4x32_10((uint32_t)e, (uint32_t)(s + 1), PURPOSE_MOVE, 0u, k0, k1);
            const double u_move = u53(x.x, x.y);
            const bool de = u_move < de_fraction;
            const pem::ens::Move w = pem::ens::draw_move<true>((uint32_t)e, (uint32_t)(s + 1), (uint32_t)m, H, d, de, a, g0, sigma, k0, k1);
            s_coef[i] = w.coef;
            s_j1[i] = w.j1;
            s_j2[i] = w.j2;                      // >= 0 marks the DE move
            log_q[e * HH + (size_t)m] = w.log_q;
            if (draws) {
                double* row = draws + (e * HH + (size_t)m) * DRAW_COLS;
                row[0] = de ? 1.0 : 0.0;
                row[1] = w.coef;
                row[2] = (double)w.j1;
                row[3] = (double)w.j2;
                row[5] = u_move;
            }
        }
        __syncthreads();
        for (int i = tid; i < nt * H * d; i += THREADS) {
            const int c = i / (H * d), rem = i - c * H * d, m = rem / d, j = rem - m * d;
            const size_t e = e0 + (size_t)(t0 + c);
            const double* th = theta + e * KK * dd;
            const int li = c * H + m;
            const double cf = s_coef[li];
            const double xw = th[(size_t)mb * dd + (size_t)rem];
            const double x1 = th[(size_t)(cb + s_j1[li]) * dd + (size_t)j];
            double y;
            if (s_j2[li] >= 0) {
                const double x2 = th[(size_t)(cb + s_j2[li]) * dd + (size_t)j];
                y = pem::ens::de_point(cf, xw, x1, x2);
            } else {
                y = pem::ens::stretch_point(cf, xw, x1);
            }
            prop[e * HH * dd + (size_t)rem] = y;
        }
        __syncthreads();
    }
    if (tid == 0) state[r] = s + 1;
}

}  // namespace

extern "C" int pem_tempered_ensemble_step_f64_dev(size_t n_replicas, int n_temperatures, int n_walkers, int ndim, uint64_t seed,
                                                  double a, double de_fraction, double g0, double sigma, const double* beta,
                                                  uint64_t trace_first, size_t trace_len, uint64_t thin, double* theta,
                                                  double* loglik, double* logprior, double* prop, const double* prop_loglik,
                                                  const double* prop_logprior, double* log_q, uint64_t* state, uint64_t* accepted,
                                                  uint64_t* swap_attempts, uint64_t* swap_accepted, double* trace,
                                                  double* loglik_trace, double* logprior_trace, double* draws, pem_stream_t stream) {
    if (n_replicas < 1 || n_replicas > (size_t)INT_MAX)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: n_replicas must be in [1, %d]", INT_MAX);
    if (n_temperatures < 1 || (size_t)n_temperatures > (size_t)INT_MAX / n_replicas)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: need n_temperatures >= 1 and n_replicas n_temperatures <= %d",
                         INT_MAX);
    if (n_walkers < 2 || n_walkers > PEM_ENSEMBLE_MAX_WALKERS || (n_walkers & 1))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: n_walkers must be even and in [2, %d]",
                         PEM_ENSEMBLE_MAX_WALKERS);
    if (ndim < 1 || ndim > PEM_ENSEMBLE_MAX_DIM)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: ndim must be in [1, %d]", PEM_ENSEMBLE_MAX_DIM);
    if ((size_t)n_temperatures * (size_t)n_walkers * (size_t)ndim > (size_t)INT_MAX)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: a ladder of more than %d coordinates", INT_MAX);
    if (!(a > 1.0) || !std::isfinite(a))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: need a finite stretch scale a > 1");
    if (!(de_fraction >= 0.0 && de_fraction <= 1.0))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: de_fraction must be in [0, 1]");
    if (de_fraction > 0.0 && n_walkers < 4)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: the DE move needs two partners: n_walkers >= 4");
    if (!(g0 > 0.0) || !std::isfinite(g0) || !(sigma >= 0.0) || !std::isfinite(sigma))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: need finite g0 > 0 and sigma >= 0");
    if (thin == 0) return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: thin must be at least 1");
    if (!beta || !theta || !loglik || !logprior || !prop || !prop_loglik || !prop_logprior || !log_q || !state || !accepted)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: NULL array");
    if (n_temperatures > 1 && (!swap_attempts || !swap_accepted))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: NULL swap counters with more than one temperature");
    if ((trace || loglik_trace || logprior_trace) && trace_len == 0)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_tempered_ensemble_step: a trace needs trace_len >= 1");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(tempered_ensemble_step_kernel, dim3((unsigned)n_replicas), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       n_temperatures, n_walkers, ndim, (uint32_t)seed, (uint32_t)(seed >> 32), a, de_fraction, g0, sigma, beta,
                       trace_first, (uint64_t)trace_len, thin, theta, loglik, logprior, prop, prop_loglik, prop_logprior, log_q, state,
                       accepted, swap_attempts, swap_accepted, trace, loglik_trace, logprior_trace, draws);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
