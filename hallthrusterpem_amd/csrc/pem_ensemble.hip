// pem_ensemble.hip -- one half-step of the affine-invariant ensemble sampler for E ensembles of K walkers
// (hallthrusterpem_amd/calibration.py, DeviceEnsemble).
//
// The algorithm is Goodman & Weare's (Comm. App. Math. Comp. Sci. 5, 2010), the one behind emcee (third-party and absent:
// parity UNPINNED; tests/ensemble_np.py restates this launch and is held to the algorithm's own exact properties).  An
// ensemble's K walkers are two fixed halves of H = K / 2: half 0 is walkers [0, H), half 1 walkers [H, K).  Half-step s
// (s = 1, 2, ...) moves half (s - 1) mod 2 against the other one, the complement, as it then stands; two half-steps are a step.
// One uniform per (ensemble, half-step) picks the move of the whole half, DE when u_move < de_fraction, otherwise the stretch:
//   stretch  partner j of the complement, z = ((a - 1) u + 1)^2 / a, y = x_j + z (x_w - x_j), log q = (d - 1) log z
//   DE       partners j1 != j2 of the complement, g = g0 (1 + sigma n), y = x_w + g (x_j1 - x_j2), log q = 0
// and walker w takes y iff log(u_acc) < log q + (lp_new - lp_old): a NaN on either side compares false.
//
// Inside-out as pem_dram.hip: launch s = state[e] resolves half-step s (s >= 1) from the H values the caller wrote to
// prop_logp since the last launch, writes the trace row that is due when s is even (a whole step has ended), emits the
// proposals of half-step s + 1 and advances the counter.  The proposals read the complement AFTER half-step s is committed,
// so one workgroup of 256 owns an ensemble and the phases are separated by __syncthreads() only: no atomics, nothing crosses
// workgroups.  Scalar decisions loop thread-per-walker and leave their results in LDS; the vector work loops the flattened
// (walker, dimension) index, so theta / prop / trace are read and written coalesced.
//
// Draws: Philox4x32-10, key = seed, counter = (ensemble, half-step mod 2^32, purpose, m), m the walker's index in its half:
//   0x454E0000, m = 0   u_move = u53(x, y)
//   0x454E0001, m       j1 = (x * H) >> 32;  j2 = (y * (H - 1)) >> 32, + 1 if >= j1 (DE only);  stretch: u = u53(z, w);
//                       DE: n = normcdfinv((2k + 1) 2^-53), k the 52 bits ((z >> 6) << 26) | (w >> 6)
//   0x454E0002, m       u_acc = u53(x, y), drawn by the launch that resolves the half-step
// Every sum and product is rounded separately (no FMA), so the restatement reproduces proposals, points, counters and traces
// bit for bit given the device's z / g, and the decisions up to the last bit of the library log.
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
constexpr int MAX_HALF = PEM_ENSEMBLE_MAX_WALKERS / 2;

using pem::Philox4;
using pem::philox4x32_10;
using pem::u53;
using pem::ens::DRAW_COLS;
using pem::ens::PURPOSE_ACCEPT;
using pem::ens::PURPOSE_MOVE;

__global__ __launch_bounds__(THREADS) void ensemble_step_kernel(int K, int d, uint32_t k0, uint32_t k1, double a, double de_fraction,
                                                                double g0, double sigma, uint64_t trace_first, uint64_t trace_len,
                                                                uint64_t thin, double* theta, double* logp, double* prop,
                                                                const double* prop_logp, double* log_q, uint64_t* state,
                                                                uint64_t* accepted, double* trace, double* logp_trace,
                                                                double* draws) {
#pragma clang fp contract(off)
    __shared__ double s_coef[MAX_HALF];          // z (stretch) or g (DE) of the moving walker
    __shared__ int s_j1[MAX_HALF], s_j2[MAX_HALF];
    __shared__ int s_acc[MAX_HALF];
    const size_t e = blockIdx.x, E = gridDim.x;
    const int tid = threadIdx.x;
    const int H = K >> 1;
    const size_t KK = (size_t)K, HH = (size_t)H, dd = (size_t)d;
    const uint64_t s = state[e];
    double* th = theta + e * KK * dd;            // this ensemble's walkers, proposals and values
    double* lp = logp + e * KK;
    double* pr = prop + e * HH * dd;
    double* lq = log_q + e * HH;
    double* dr = draws ? draws + e * HH * DRAW_COLS : nullptr;

    if (s >= 1) {                                // uniform over the workgroup, as every condition around a barrier below
        // ---- the decisions of half-step s: thread per moving walker
        const int base = (int)((s - 1) & 1) * H;
        for (int m = tid; m < H; m += THREADS) {
            const Philox4 r = philox4x32_10((uint32_t)e, (uint32_t)s, PURPOSE_ACCEPT, (uint32_t)m, k0, k1);
            const double u = u53(r.x, r.y);
            const double lp_old = lp[base + m], lp_new = prop_logp[e * HH + m];
            const bool acc = log(u) < lq[m] + (lp_new - lp_old);
            s_acc[m] = acc ? 1 : 0;
            if (acc) {
                lp[base + m] = lp_new;
                accepted[e * KK + base + m] += 1;
            }
            if (dr) dr[(size_t)m * DRAW_COLS + 4] = u;
        }
        __syncthreads();
        // ---- commit: the accepted proposals become the walkers' points
        for (int idx = tid; idx < H * d; idx += THREADS)
            if (s_acc[idx / d]) th[(size_t)base * dd + idx] = pr[idx];
        __syncthreads();
        // ---- the trace row, when a whole step has ended and its row is due
        if ((s & 1) == 0 && s / 2 - 1 >= trace_first) {
            const uint64_t r = s / 2 - 1 - trace_first;
            if (r % thin == 0 && r / thin < trace_len) {
                const size_t row = (size_t)(r / thin);
                if (trace)
                    for (int idx = tid; idx < K * d; idx += THREADS) trace[(row * E + e) * KK * dd + idx] = th[idx];
                if (logp_trace)
                    for (int w = tid; w < K; w += THREADS) logp_trace[(row * E + e) * KK + w] = lp[w];
            }
        }
    }

    // ---- the proposals of half-step s + 1: the half that moves, against the complement as it now stands
    const int mb = (int)(s & 1) * H, cb = H - mb;
    const Philox4 mv = philox4x32_10((uint32_t)e, (uint32_t)(s + 1), PURPOSE_MOVE, 0u, k0, k1);
    const double u_move = u53(mv.x, mv.y);
    const bool de = u_move < de_fraction;
    for (int m = tid; m < H; m += THREADS) {
        const pem::ens::Move w = pem::ens::draw_move((uint32_t)e, (uint32_t)(s + 1), (uint32_t)m, H, d, de, a, g0, sigma, k0, k1);
        const int j1 = w.j1, j2 = w.j2;
        const double coef = w.coef;
        s_coef[m] = coef;
        s_j1[m] = j1;
        s_j2[m] = j2;
        lq[m] = w.log_q;
        if (dr) {
            double* row = dr + (size_t)m * DRAW_COLS;
            row[0] = de ? 1.0 : 0.0;
            row[1] = coef;
            row[2] = (double)j1;
            row[3] = (double)j2;
            row[5] = u_move;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < H * d; idx += THREADS) {
        const int m = idx / d, j = idx - m * d;
        const double c = s_coef[m];
        const double xw = th[(size_t)mb * dd + idx];
        const double x1 = th[(size_t)(cb + s_j1[m]) * dd + j];
        double y;
        if (de) {
            const double x2 = th[(size_t)(cb + s_j2[m]) * dd + j];
            y = pem::ens::de_point(c, xw, x1, x2);
        } else {
            y = pem::ens::stretch_point(c, xw, x1);
        }
        pr[idx] = y;
    }
    if (tid == 0) state[e] = s + 1;
}

}  // namespace

extern "C" int pem_ensemble_step_f64_dev(size_t n_ensembles, int n_walkers, int ndim, uint64_t seed, double a, double de_fraction,
                                         double g0, double sigma, uint64_t trace_first, size_t trace_len, uint64_t thin,
                                         double* theta, double* logp, double* prop, const double* prop_logp, double* log_q,
                                         uint64_t* state, uint64_t* accepted, double* trace, double* logp_trace, double* draws,
                                         pem_stream_t stream) {
    if (n_ensembles < 1 || n_ensembles > (size_t)INT_MAX)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: n_ensembles must be in [1, %d]", INT_MAX);
    if (n_walkers < 2 || n_walkers > PEM_ENSEMBLE_MAX_WALKERS || (n_walkers & 1))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: n_walkers must be even and in [2, %d]", PEM_ENSEMBLE_MAX_WALKERS);
    if (ndim < 1 || ndim > PEM_ENSEMBLE_MAX_DIM)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: ndim must be in [1, %d]", PEM_ENSEMBLE_MAX_DIM);
    if (!(a > 1.0) || !std::isfinite(a)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: need a finite stretch scale a > 1");
    if (!(de_fraction >= 0.0 && de_fraction <= 1.0))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: de_fraction must be in [0, 1]");
    if (de_fraction > 0.0 && n_walkers < 4)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: the DE move needs two partners: n_walkers >= 4");
    if (!(g0 > 0.0) || !std::isfinite(g0) || !(sigma >= 0.0) || !std::isfinite(sigma))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: need finite g0 > 0 and sigma >= 0");
    if (thin == 0) return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: thin must be at least 1");
    if (!theta || !logp || !prop || !prop_logp || !log_q || !state || !accepted)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: NULL array");
    if ((trace || logp_trace) && trace_len == 0)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_ensemble_step: a trace needs trace_len >= 1");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(ensemble_step_kernel, dim3((unsigned)n_ensembles), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       n_walkers, ndim, (uint32_t)seed, (uint32_t)(seed >> 32), a, de_fraction, g0, sigma, trace_first,
                       (uint64_t)trace_len, thin, theta, logp, prop, prop_logp, log_q, state, accepted, trace, logp_trace, draws);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
