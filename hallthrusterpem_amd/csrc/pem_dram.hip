// pem_dram.hip -- one step of delayed-rejection adaptive Metropolis for K chains (hallthrusterpem_amd/calibration.py, DeviceDRAM).
//
// What it stands in for: `uq.dram(fun, p0, niter, adapt_after=5000, adapt_interval=1000, eps=1e-12, gamma=0.1)` of run_mcmc
// (scripts/pem_v0/mcmc.py:275-300), the algorithm `calibration.DRAM` restates as torch glue: a first-stage proposal
// y1 = x + L z1, a delayed one y2 = x + sqrt(gamma) L z2, the Welford moments of the chain and the adaptation of L.
//
// Both stages are evaluated for every chain on every step and y2 does not depend on the outcome of y1, so ONE launch resolves
// step s from the 2K values the caller wrote since the last launch and draws both proposals of step s + 1.  The step counter
// lives in device memory (`state`, one word per chain): a captured graph [posterior(prop) -> prop_logp ; this kernel] replays
// the same arguments and is one whole DRAM step.
//
// One wave64 workgroup per chain; lane j owns dimension j, row j of L, of the scatter matrix and of the new Cholesky factor.
// Every random number is Philox4x32-10 with counter (chain, step, purpose, pair) and key seed, every sum runs in index order
// with products and sums rounded separately, so tests/dram_np.py restates the launch: bit for bit in everything that is built
// from + - * / sqrt, and up to the last bit of the library exp / log / log1p in the two accept decisions.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_philox.h"

namespace {

constexpr int MAX_DIM = PEM_DRAM_MAX_DIM;
constexpr int LDP = MAX_DIM + 1;   // padded row of the LDS factor: lanes walking their own rows hit distinct banks
static_assert(MAX_DIM <= 64, "one lane per dimension");

// purposes (word 2 of the Philox counter); far above any d / 2 a Design puts there, so a seed shared with one reuses no counter
constexpr uint32_t PURPOSE_Z1 = 0x44520000u;   // pair p: the first-stage normals of dimensions 2p, 2p + 1
constexpr uint32_t PURPOSE_Z2 = 0x44520001u;   // pair p: the delayed-stage normals of dimensions 2p, 2p + 1
constexpr uint32_t PURPOSE_U = 0x44520002u;    // pair 0: words x, y the first-stage uniform, words z, w the delayed-stage one

using pem::Philox4;
using pem::philox4x32_10;
using pem::u53;

// a standard normal from pem::u_open: never +-inf
__device__ __forceinline__ double normal_of(uint32_t hi, uint32_t lo) { return normcdfinv(pem::u_open(hi, lo)); }

struct Normals {
    double z1, z2;
};

// z1_j and z2_j of chain k at step s.  Out of line, a leaf, its result by value: inlined at both call sites the Philox blocks
// and the library normcdfinv bodies cost the kernel more scalar registers than it has; a result handed back through a
// pointer, or a call below this one, would put a stack frame in scratch.
__device__ __attribute__((noinline)) Normals step_normals(uint32_t k, uint32_t s, int j, uint32_t k0, uint32_t k1) {
    const uint32_t pair = (uint32_t)(j >> 1);
    const Philox4 a = philox4x32_10(k, s, PURPOSE_Z1, pair, k0, k1);
    const Philox4 b = philox4x32_10(k, s, PURPOSE_Z2, pair, k0, k1);
    const bool odd = (j & 1) != 0;
    Normals z;
    z.z1 = normal_of(odd ? a.z : a.x, odd ? a.w : a.y);
    z.z2 = normal_of(odd ? b.z : b.x, odd ? b.w : b.y);
    return z;
}

// exp(min(x, 0)) as torch's exp(x.clamp(max=0)): a NaN stays NaN (fmin would drop it)
__device__ __forceinline__ double accept_ratio(double x) { return exp(x > 0.0 ? 0.0 : x); }

__global__ __launch_bounds__(64) void dram_step_kernel(size_t K, int d, uint32_t k0, uint32_t k1, double sqrt_gamma, double eps,
                                                       double cov_scale, uint64_t adapt_after, uint64_t adapt_interval,
                                                       uint64_t trace_first, uint64_t trace_len, uint64_t thin, double* theta,
                                                       double* logp, double* L, double* mean, double* scatter, double* prop,
                                                       const double* prop_logp, uint64_t* state, uint64_t* accepted,
                                                       uint32_t* flags, double* trace, double* logp_trace, double* draws) {
#pragma clang fp contract(off)
    __shared__ double s_a[MAX_DIM], s_b[MAX_DIM];   // z1, z2 of the step in hand; then theta - mean
    __shared__ double s_c[MAX_DIM][LDP];            // the scaled covariance, factorised in place
    const size_t k = blockIdx.x;
    const int j = threadIdx.x;
    const bool live = j < d;
    const size_t dd = (size_t)d;
    const uint64_t s = state[k];
    double* Lk = L + k * dd * dd;
    double x = live ? theta[k * dd + j] : 0.0;

    if (s >= 1) {
        // ---- the decision of step s: both proposals were evaluated since the last launch
        double z1 = 0.0, z2 = 0.0;
        if (live) {
            const Normals z = step_normals((uint32_t)k, (uint32_t)s, j, k0, k1);
            z1 = z.z1;
            z2 = z.z2;
            s_a[j] = z1;
            s_b[j] = z2;
        }
        __syncthreads();
        const Philox4 uu = philox4x32_10((uint32_t)k, (uint32_t)s, PURPOSE_U, 0u, k0, k1);
        const double u1 = u53(uu.x, uu.y), u2 = u53(uu.z, uu.w);
        double ww = 0.0, zz = 0.0;                  // |w|^2 with w = z1 - sqrt(gamma) z2 = L^-1 (y1 - y2), and |z1|^2
        for (int i = 0; i < d; ++i) {
            const double a = s_a[i];
            const double w = a - sqrt_gamma * s_b[i];
            ww = ww + w * w;
            zz = zz + a * a;
        }
        const double lp0 = logp[k], lp1 = prop_logp[k], lp2 = prop_logp[K + k];
        const double a1 = accept_ratio(lp1 - lp0);
        const bool acc1 = u1 < a1;                  // a NaN ratio compares false: rejected
        const double a1_rev = accept_ratio(lp1 - lp2);
        const double log_q = -0.5 * (ww - zz);
        const double log_a2 = (((lp2 - lp0) + log_q) + log1p(-a1_rev)) - log1p(-a1);
        const bool acc2 = !acc1 && log(u2) < log_a2;
        const double lp = acc1 ? lp1 : (acc2 ? lp2 : lp0);
        __syncthreads();                            // every lane has read logp[k] and the normals
        if (live) {
            const double y1 = prop[k * dd + j], y2 = prop[(K + k) * dd + j];
            x = acc1 ? y1 : (acc2 ? y2 : x);
            theta[k * dd + j] = x;
            if (draws) {
                draws[k * (2 * dd + 2) + j] = z1;
                draws[k * (2 * dd + 2) + dd + j] = z2;
            }
        }
        if (j == 0) {
            logp[k] = lp;
            if (acc1) accepted[k] += 1;
            if (acc2) accepted[K + k] += 1;
            if (draws) {
                draws[k * (2 * dd + 2) + 2 * dd] = u1;
                draws[k * (2 * dd + 2) + 2 * dd + 1] = u2;
            }
        }
        if (s - 1 >= trace_first) {                 // row (s - 1 - trace_first) / thin of the trace, when it is due
            const uint64_t r = s - 1 - trace_first;
            if (r % thin == 0 && r / thin < trace_len) {
                const size_t row = (size_t)(r / thin);
                if (trace && live) trace[(row * K + k) * dd + j] = x;
                if (logp_trace && j == 0) logp_trace[row * K + k] = lp;
            }
        }

        // ---- the running moments (Welford); the start point was observation 1, so this is observation s + 1
        const double count = (double)(s + 1);
        double delta = 0.0;
        if (live) {
            const double m = mean[k * dd + j];
            delta = x - m;
            const double m_new = m + delta / count;
            mean[k * dd + j] = m_new;
            s_a[j] = x - m_new;
        }
        __syncthreads();
        const bool adapt = s >= adapt_after && (s - adapt_after) % adapt_interval == 0;   // count >= 2 holds for every s >= 1
        if (live) {
            double* row = scatter + k * dd * dd + (size_t)j * dd;
            for (int i = 0; i < d; ++i) {
                const double v = row[i] + delta * s_a[i];
                row[i] = v;
                if (adapt && i <= j) s_c[j][i] = cov_scale * (v / (count - 1.0) + (i == j ? eps : 0.0));
            }
        }

        // ---- adaptation: L = chol((2.4^2 / d) (scatter / (count - 1) + eps I)), committed only if every pivot is > 0
        if (adapt) {
            __syncthreads();
            bool ok = true;
            for (int c = 0; c < d; ++c) {           // column c of the factor: lane c its pivot, the lanes below it their entry
                double acc = 0.0;
                if (live && j >= c) {
                    acc = s_c[j][c];
                    for (int i = 0; i < c; ++i) acc = acc - s_c[j][i] * s_c[c][i];
                }
                const double pivot = __shfl(acc, c);
                if (!(pivot > 0.0)) {               // uniform: zero, negative or NaN
                    ok = false;
                    break;
                }
                const double r = sqrt(pivot);
                if (live && j >= c) s_c[j][c] = j == c ? r : acc / r;   // column c: no lane read it in this pass
                __syncthreads();
            }
            if (ok) {
                if (live)
                    for (int i = 0; i < d; ++i) Lk[(size_t)j * dd + i] = i <= j ? s_c[j][i] : 0.0;
            } else if (j == 0) {
                flags[k] |= 1u;
            }
        }
        __syncthreads();                            // s_a, s_b are reused below
    }

    // ---- the proposals of step s + 1 from the point and the factor as they now stand
    if (live) {
        const Normals z = step_normals((uint32_t)k, (uint32_t)(s + 1), j, k0, k1);
        s_a[j] = z.z1;
        s_b[j] = z.z2;
    }
    __syncthreads();
    if (live) {
        double t1 = 0.0, t2 = 0.0;
        for (int i = 0; i <= j; ++i) {
            const double l = Lk[(size_t)j * dd + i];
            t1 = t1 + l * s_a[i];
            t2 = t2 + l * s_b[i];
        }
        prop[k * dd + j] = x + t1;
        prop[(K + k) * dd + j] = x + sqrt_gamma * t2;
    }
    if (j == 0) state[k] = s + 1;
}

}  // namespace

extern "C" int pem_dram_step_f64_dev(size_t n_chains, int ndim, uint64_t seed, double gamma, double eps, uint64_t adapt_after,
                                     uint64_t adapt_interval, uint64_t trace_first, size_t trace_len, uint64_t thin, double* theta,
                                     double* logp, double* L, double* mean, double* scatter, double* prop, const double* prop_logp,
                                     uint64_t* state, uint64_t* accepted, uint32_t* flags, double* trace, double* logp_trace,
                                     double* draws, pem_stream_t stream) {
    if (n_chains < 1 || n_chains > (size_t)INT_MAX)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_dram_step: n_chains must be in [1, %d]", INT_MAX);
    if (ndim < 1 || ndim > MAX_DIM) return pem::fail(PEM_ERR_INVALID_ARG, "pem_dram_step: ndim must be in [1, %d]", MAX_DIM);
    if (!(gamma > 0.0) || !(eps >= 0.0)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_dram_step: need gamma > 0 and eps >= 0");
    if (adapt_interval == 0 || thin == 0)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_dram_step: adapt_interval and thin must be at least 1");
    if (!theta || !logp || !L || !mean || !scatter || !prop || !prop_logp || !state || !accepted || !flags)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_dram_step: NULL array");
    if ((trace || logp_trace) && trace_len == 0)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_dram_step: a trace needs trace_len >= 1");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(dram_step_kernel, dim3((unsigned)n_chains), dim3(64), 0, static_cast<hipStream_t>(stream), n_chains, ndim,
                       (uint32_t)seed, (uint32_t)(seed >> 32), sqrt(gamma), eps, (2.4 * 2.4) / (double)ndim, adapt_after,
                       adapt_interval, trace_first, (uint64_t)trace_len, thin, theta, logp, L, mean, scatter, prop, prop_logp, state,
                       accepted, flags, trace, logp_trace, draws);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
