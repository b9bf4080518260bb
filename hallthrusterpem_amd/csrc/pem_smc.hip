// pem_smc.hip -- tempered sequential Monte Carlo for R populations of N particles (hallthrusterpem_amd/calibration.py, DeviceSMC).
//
// The algorithm is TMCMC (Ching & Chen 2007) / the SMC sampler of Del Moral et al. 2006 as PyMC's sample_smc runs it (third-party
// and absent: parity UNPINNED; tests/smc_np.py restates both launches, the rules are in include/pem_hip.h).  A stage is
//   pem_smc_stage_f64_dev   one workgroup of 1024 per population: next temperature by bisection on the ESS, evidence increment,
//                           weighted moments -> Cholesky factor of the proposal, systematic resampling, the first proposals
//   pem_smc_move_f64_dev    a grid over all particles: resolve the pending random-walk Metropolis proposal, draw the next one
// with the caller's log likelihood and log prior evaluated on `prop` between launches.
//
// One LDS array of N doubles carries a population through the stage kernel: l - l_max during the 53 ESS evaluations (thread t
// owns particles t P ... t P + P - 1, P = ceil(N / 1024) <= 16, and reads them back for every evaluation: one exp per particle and
// one block reduction -- wave shuffles, 16 partials in LDS, every thread adds them in the same order, so every decision is
// uniform), then the weights (read by the moment sums), their cumulative sums (searched by the resampler) and, as integers, the
// ancestors (read by the gather).  That array, 128 KiB of the CU's 160, is what limits PEM_SMC_MAX_PARTICLES; held in registers
// instead, 16 values a thread beside the inlined exp left the 128 registers of a 1024-thread workgroup short and spilled.  The
// d (d + 1) / 2 covariance sums are spread over min(64, 1024 / pairs) slices of the particles per pair, one thread per
// (pair, slice), partials reduced in slice order.
//
// No atomics, nothing crosses workgroups, every sum has a fixed order and products and sums are rounded separately, so the same
// bits come out on every run; given the device's beta', weights, factor, normals and decisions the restatement reproduces
// every other word bit for bit.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_philox.h"

namespace {

constexpr int ST = 1024;                             // threads of the stage kernel
constexpr int PER = PEM_SMC_MAX_PARTICLES / ST;      // particles per thread, at most (their ancestors are held in registers)
constexpr int MT = 256;                              // threads of the move kernel
constexpr int PB = 64;                               // particles per proposal batch (a move workgroup's share)
constexpr int MAX_DIM = PEM_SMC_MAX_DIM;
constexpr int LDP = MAX_DIM + 1;                     // padded LDS rows
static_assert(PER * ST == PEM_SMC_MAX_PARTICLES, "a thread owns PER particles");
static_assert(MAX_DIM * (MAX_DIM + 1) / 2 <= ST && PB * LDP >= ST, "one thread per covariance entry; partials fit the work array");

// purposes (word 2 of the Philox counter), apart from DRAM's 0x4452000x and the ensembles' 0x454E000x
constexpr uint32_t PURPOSE_RESAMPLE = 0x534D0000u;   // counter (population, stage, ., 0): u = u53(x, y)
constexpr uint32_t PURPOSE_Z = 0x534D0001u;          // counter (population N + particle, stage n_mcmc + move, ., pair p): z_2p, z_2p+1
constexpr uint32_t PURPOSE_U = 0x534D0002u;          // counter (population N + particle, stage n_mcmc + move, ., 0): u = u53(x, y)

using pem::Philox4;
using pem::philox4x32_10;
using pem::u53;

// a standard normal from pem::u_open, as pem_dram.hip draws them
__device__ __forceinline__ double normal_of(uint32_t hi, uint32_t lo) { return normcdfinv(pem::u_open(hi, lo)); }

// z_j of a particle under counter word `word`.  Out of line, a leaf, its result by value (as pem_dram.hip's step_normals):
// inlined into the batch loops the Philox rounds and the library normcdfinv cost the stage kernel more registers than the 128 a
// workgroup of 1024 leaves a thread.
__device__ __attribute__((noinline)) double particle_normal(uint32_t gp, uint32_t word, int j, uint32_t k0, uint32_t k1) {
    const Philox4 r = philox4x32_10(gp, word, PURPOSE_Z, (uint32_t)(j >> 1), k0, k1);
    const bool odd = (j & 1) != 0;
    return normal_of(odd ? r.z : r.x, odd ? r.w : r.y);
}

// The proposals y = x + L z of particles [p0, p0 + np) of one population, np <= PB, by all THREADS of the workgroup: the normals
// of (particle, dimension) go to LDS, then entry j of a particle sums row j of L with i ascending.  th, pr: the rows of these
// particles; rec_z: NULL or where their normals are reported, rec_ld doubles per particle.
template <int THREADS>
__device__ __forceinline__ void propose_tile(int tid, uint32_t gp0, int np, int d, uint32_t word, uint32_t k0, uint32_t k1,
                                             const double* th, const double* Lr, double* pr, double* rec_z, size_t rec_ld,
                                             double* s_z) {
#pragma clang fp contract(off)
    for (int idx = tid; idx < np * d; idx += THREADS) {
        const int pp = idx / d, j = idx - pp * d;
        const double z = particle_normal(gp0 + (uint32_t)pp, word, j, k0, k1);
        s_z[pp * LDP + j] = z;
        if (rec_z) rec_z[(size_t)pp * rec_ld + j] = z;
    }
    __syncthreads();
    for (int idx = tid; idx < np * d; idx += THREADS) {
        const int pp = idx / d, j = idx - pp * d;
        double t = 0.0;
#pragma unroll 2
        for (int i = 0; i <= j; ++i) t = t + Lr[j * d + i] * s_z[pp * LDP + i];
        pr[idx] = th[idx] + t;
    }
    __syncthreads();                                 // s_z is reused by the next batch
}

struct Pair {
    double a, b;
};

// (sum or max of a, sum of b) over the workgroup, the same bits in every thread: wave shuffles, then the 16 wave partials in
// wave order.  `buf` alternates between two sets of partials so that one barrier per call is enough.
template <bool MAX_A>
__device__ __forceinline__ Pair block_reduce(double a, double b, double (*s_red)[2][ST / 64], int& buf) {
#pragma clang fp contract(off)
    for (int o = 32; o > 0; o >>= 1) {
        const double oa = __shfl_xor(a, o), ob = __shfl_xor(b, o);
        a = MAX_A ? fmax(a, oa) : a + oa;
        b = b + ob;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[buf][0][wave] = a;
        s_red[buf][1][wave] = b;
    }
    __syncthreads();
    Pair out{s_red[buf][0][0], s_red[buf][1][0]};
    for (int w = 1; w < ST / 64; ++w) {
        const double oa = s_red[buf][0][w];
        out.a = MAX_A ? fmax(out.a, oa) : out.a + oa;
        out.b = out.b + s_red[buf][1][w];
    }
    buf ^= 1;
    return out;
}

__global__ __launch_bounds__(ST) __attribute__((amdgpu_waves_per_eu(4, 4))) void smc_stage_kernel(int N, int d, uint32_t k0, uint32_t k1, double tau, double scale2, double eps,
                                                       uint32_t n_mcmc, double* theta, double* loglik, double* logprior,
                                                       double* beta, double* log_evidence, uint64_t* stage, double* L, double* prop,
                                                       uint32_t* accept_count, uint64_t* accepted, uint32_t* flags,
                                                       uint32_t* moves_active, double* scratch, double* hist_beta, double* hist_ess,
                                                       double* hist_accept, double* hist_dlogz, uint64_t history_len,
                                                       double* record) {
#pragma clang fp contract(off)
    __shared__ double s_v[PEM_SMC_MAX_PARTICLES];    // l - l_max, then weights, then cumulative weights, then (as int) ancestors
    __shared__ double s_work[PB * LDP];              // partial moments, then the normals of a proposal batch
    __shared__ double s_c[MAX_DIM][LDP];             // scale^2 cov + eps I, factorised in place
    __shared__ double s_red[2][2][ST / 64];
    __shared__ double s_mean[MAX_DIM];
    __shared__ double s_wave[ST / 64];
    __shared__ double s_piv;
    const size_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t NN = (size_t)N, dd = (size_t)d;
    double* th = theta + r * NN * dd;
    double* ll = loglik + r * NN;
    double* lp = logprior + r * NN;
    uint32_t* ac = accept_count + r * NN;
    int buf = 0;
    const double b0 = beta[r];
    const uint64_t s0 = stage[r];
    const uint32_t active = moves_active[r];         // (thread 0 writes these words only after a barrier every thread has passed)

    // ---- the moves of stage s0 have ended: their acceptances, counted per particle by the move launches
    if (active) {
        double c = 0.0;
        for (int i = tid; i < N; i += ST) c += (double)ac[i];
        const Pair t = block_reduce<false>(c, 0.0, s_red, buf);          // whole numbers below 2^53: exact in any order
        if (tid == 0) {
            accepted[r] = (uint64_t)t.a;
            if (s0 >= 1 && s0 - 1 < history_len) hist_accept[r * history_len + (s0 - 1)] = t.a / ((double)N * (double)n_mcmc);
        }
    }
    if (!(b0 < 1.0)) {                               // finished
        if (tid == 0) moves_active[r] = 0u;
        return;
    }

    // ---- this thread's particles tid P ... tid P + P - 1: l - l_max in s_v, -inf for a value that is not finite (weight 0 at
    // every b).  A thread reads and writes its own entries only until the barrier that follows the weights.
    const int P = (N + ST - 1) / ST;
    const int i0 = min(tid * P, N), i1 = min(i0 + P, N);
    double mx = -INFINITY, nfin = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double x = ll[i];
        const bool fin = isfinite(x);
        s_v[i] = fin ? x : -INFINITY;
        if (fin) {
            mx = fmax(mx, x);
            nfin += 1.0;
        }
    }
    const Pair top = block_reduce<true>(mx, nfin, s_red, buf);
    const double lmax = top.a;
    if (top.b == 0.0) {
        if (tid == 0) {
            flags[r] |= 2u;
            moves_active[r] = 0u;
        }
        return;
    }
    for (int i = i0; i < i1; ++i) s_v[i] = s_v[i] - lmax;

    // ---- 1. the next temperature
    auto sums_at = [&](double b) {
        const double db = b - b0;
        double a = 0.0, q = 0.0;
#pragma unroll 2
        for (int i = i0; i < i1; ++i) {
            const double x = s_v[i];
            const double w = x == -INFINITY ? 0.0 : exp(db * x);
            a = a + w;
            q = q + w * w;
        }
        return block_reduce<false>(a, q, s_red, buf);
    };
    const double tauN = tau * (double)N;
    double b1 = 1.0;
    {
        const Pair s1 = sums_at(1.0);
        if (!((s1.a * s1.a) / s1.b >= tauN)) {
            double lo = b0, hi = 1.0;
            for (int it = 0; it < PEM_SMC_BISECTIONS; ++it) {
                const double mid = 0.5 * (lo + hi);
                const Pair sm = sums_at(mid);
                if ((sm.a * sm.a) / sm.b >= tauN) lo = mid;
                else hi = mid;
            }
            b1 = lo > b0 ? lo : hi;
        }
    }

    // ---- 2. the weights at beta' (s_v from here on), the evidence increment
    double* rec = record ? record + r * (3 * NN + NN * dd + 1 + dd + dd * dd) : nullptr;
    const double db = b1 - b0;
    double wa = 0.0, wq = 0.0, lastp = -1.0;
    for (int i = i0; i < i1; ++i) {
        const double x = s_v[i];
        const double w = x == -INFINITY ? 0.0 : exp(db * x);
        s_v[i] = w;
        wa = wa + w;
        wq = wq + w * w;
        if (w > 0.0) lastp = (double)i;
    }
    const Pair sw = block_reduce<false>(wa, wq, s_red, buf);
    const Pair lastr = block_reduce<true>(lastp, 0.0, s_red, buf);
    const int last = max((int)lastr.a, 0);           // the last particle of positive weight (the one at l_max has weight 1)
    const double ess = (sw.a * sw.a) / sw.b;
    const double inc = log(sw.a / (double)N) + db * lmax;
    if (rec)
        for (int i = i0; i < i1; ++i) {
            rec[i] = s_v[i];
            rec[NN + i] = s_v[i] / sw.a;
        }
    __syncthreads();

    // ---- 3. weighted mean and covariance: one thread per (entry, slice of the particles), slices added in order
    {
        const int G = min(64, ST / d);
        if (tid < G * d) {
            const int j = tid % d, g = tid / d;
            double acc = 0.0;
            for (int i = g; i < N; i += G) acc = acc + s_v[i] * th[(size_t)i * dd + j];
            s_work[g * d + j] = acc;
        }
        __syncthreads();
        if (tid < d) {
            double m = 0.0;
            for (int g = 0; g < G; ++g) m = m + s_work[g * d + tid];
            m = m / sw.a;
            s_mean[tid] = m;
            if (rec) rec[3 * NN + NN * dd + 1 + tid] = m;
        }
        __syncthreads();
    }
    {
        // NOT a tuned layout: one thread per (entry, slice) reads theta from global memory with stride d.  It serves the small d of
        // the calibrations (d = 6: 21 entries x 48 slices); at d = 32 the 528 entries leave G = 1, 528 threads walk all N particles
        // one after the other while 496 idle, and the sums are most of the launch (DESIGN.md 4.6.9 has the figures).  Tiles of
        // particles staged through LDS and a register block of entries per thread are what that case wants.
        const int pairs = d * (d + 1) / 2;
        const int G = min(64, ST / pairs);
        int j = 0, k = 0;
        if (tid < G * pairs) {
            const int p = tid % pairs, g = tid / pairs;
            while ((j + 1) * (j + 2) / 2 <= p) ++j;
            k = p - j * (j + 1) / 2;
            const double mj = s_mean[j], mk = s_mean[k];
            double acc = 0.0;
            for (int i = g; i < N; i += G) {
                const double yj = th[(size_t)i * dd + j] - mj, yk = th[(size_t)i * dd + k] - mk;
                acc = acc + (s_v[i] * yj) * yk;
            }
            s_work[g * pairs + p] = acc;
        }
        __syncthreads();
        if (tid < pairs) {                           // (slice 0 of entry tid: j, k are this entry's)
            double c = 0.0;
            for (int g = 0; g < G; ++g) c = c + s_work[g * pairs + tid];
            c = c / sw.a;
            s_c[j][k] = scale2 * c + (j == k ? eps : 0.0);
            if (rec) {
                double* rc = rec + 3 * NN + NN * dd + 1 + dd;
                rc[(size_t)j * dd + k] = c;
                rc[(size_t)k * dd + j] = c;
            }
        }
        __syncthreads();
    }
    // L = chol(scale^2 cov + eps I) column by column, committed only if every pivot is > 0 (pem_dram.hip's rule)
    {
        bool ok = true;
        for (int c = 0; c < d; ++c) {
            double acc = 0.0;
            if (tid < d && tid >= c) {
                acc = s_c[tid][c];
                for (int i = 0; i < c; ++i) acc = acc - s_c[tid][i] * s_c[c][i];
                if (tid == c) s_piv = acc;
            }
            __syncthreads();
            const double pivot = s_piv;
            if (!(pivot > 0.0)) {                    // uniform: zero, negative or NaN
                ok = false;
                break;
            }
            const double rt = sqrt(pivot);
            if (tid < d && tid >= c) s_c[tid][c] = tid == c ? rt : acc / rt;
            __syncthreads();
        }
        if (ok) {
            for (int idx = tid; idx < d * d; idx += ST) {
                const int j = idx / d, i = idx - j * d;
                L[r * dd * dd + idx] = i <= j ? s_c[j][i] : 0.0;
            }
        } else if (tid == 0) {
            flags[r] |= 1u;
        }
    }
    __syncthreads();

    // ---- 4. systematic resampling.  C_i = W_w + (O_t + c_k): c_k the running sum of the thread's own weights in particle order,
    // O_t the running sum (from 0) of the totals of the threads before it in its wave, W_w the running sum (from 0) of the totals
    // of the waves before it, each total the end of the chain below it -- every level is a chain of rounded additions of
    // non-negative terms and an upper level starts where the lower one ends, so C is non-decreasing in i.
    double T = 0.0;
    for (int i = i0; i < i1; ++i) T = T + s_v[i];
    double O = 0.0, run = 0.0;
    for (int l = 0; l < 64; ++l) {
        const double tl = __shfl(T, l);
        if (lane == l) O = run;
        run = run + tl;
    }
    if (lane == 0) s_wave[wave] = run;
    __syncthreads();
    double Woff = 0.0;
    for (int w = 0; w < wave; ++w) Woff = Woff + s_wave[w];
    T = 0.0;
    for (int i = i0; i < i1; ++i) {                  // the same chain again, now with its offsets known
        T = T + s_v[i];
        s_v[i] = Woff + (O + T);
    }
    __syncthreads();
    const uint32_t s1 = (uint32_t)(s0 + 1);
    const Philox4 ru = philox4x32_10((uint32_t)r, s1, PURPOSE_RESAMPLE, 0u, k0, k1);
    const double u = u53(ru.x, ru.y);
    const double CN = s_v[N - 1];
    int anc[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int j = tid + k * ST;
        anc[k] = 0;
        if (j < N) {
            const double t = (((double)j + u) / (double)N) * CN;
            int lo = 0, hi = N;                      // the smallest i with C_i > t, N if there is none
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_v[mid] > t) hi = mid;
                else lo = mid + 1;
            }
            anc[k] = min(lo, last);
        }
    }
    __syncthreads();
    int* s_anc = reinterpret_cast<int*>(s_v);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int j = tid + k * ST;
        if (j < N) {
            s_anc[j] = anc[k];
            if (rec) rec[2 * NN + j] = (double)anc[k];
        }
    }
    if (rec && tid == 0) rec[3 * NN + NN * dd] = u;
    __syncthreads();
    double* sc = scratch + r * NN * (dd + 2);
    for (int idx = tid; idx < N * d; idx += ST) {
        const int j = idx / d, c = idx - j * d;
        sc[idx] = th[(size_t)s_anc[j] * dd + c];
    }
    for (int j = tid; j < N; j += ST) {
        sc[NN * dd + j] = ll[s_anc[j]];
        sc[NN * dd + NN + j] = lp[s_anc[j]];
    }
    __syncthreads();
    for (int idx = tid; idx < N * d; idx += ST) th[idx] = sc[idx];
    for (int j = tid; j < N; j += ST) {
        ll[j] = sc[NN * dd + j];
        lp[j] = sc[NN * dd + NN + j];
        ac[j] = 0u;
    }

    // ---- 5. the history row and the state words
    if (tid == 0) {
        if (s0 < history_len) {
            hist_beta[r * history_len + s0] = b1;
            hist_ess[r * history_len + s0] = ess;
            hist_dlogz[r * history_len + s0] = inc;
        }
        beta[r] = b1;
        log_evidence[r] = log_evidence[r] + inc;
        stage[r] = s0 + 1;
        moves_active[r] = 1u;
    }
    __syncthreads();

    // ---- 6. the proposals of move 1 of the new stage
    const uint32_t word = (uint32_t)((s0 + 1) * (uint64_t)n_mcmc + 1);
    for (int p0 = 0; p0 < N; p0 += PB) {
        const int np = min(PB, N - p0);
        propose_tile<ST>(tid, (uint32_t)(r * NN) + (uint32_t)p0, np, d, word, k0, k1, th + (size_t)p0 * dd, L + r * dd * dd,
                         prop + (r * NN + (size_t)p0) * dd, rec ? rec + 3 * NN + (size_t)p0 * dd : nullptr, dd, s_work);
    }
}

__global__ __launch_bounds__(MT) __attribute__((amdgpu_waves_per_eu(8, 8))) void smc_move_kernel(int N, int d, int blocks_per_pop, uint32_t k0, uint32_t k1, uint32_t n_mcmc,
                                                      uint32_t move, int propose, double* theta, double* loglik, double* logprior,
                                                      const double* beta, const uint64_t* stage, const double* L, double* prop,
                                                      const double* prop_loglik, const double* prop_logprior,
                                                      uint32_t* accept_count, const uint32_t* moves_active, double* record) {
#pragma clang fp contract(off)
    __shared__ double s_z[PB * LDP];
    __shared__ int s_acc[PB];
    const size_t r = blockIdx.x / (unsigned)blocks_per_pop;
    const int p0 = (int)(blockIdx.x % (unsigned)blocks_per_pop) * PB;
    const int tid = threadIdx.x;
    if (!moves_active[r]) return;                    // uniform over the workgroup
    const size_t NN = (size_t)N, dd = (size_t)d;
    const int np = min(PB, N - p0);
    const size_t g0 = r * NN + (size_t)p0;           // the first particle of this workgroup among all R N
    const double b = beta[r];
    const uint32_t word = (uint32_t)(stage[r] * (uint64_t)n_mcmc + move);
    double* rec = record ? record + g0 * (dd + 2) : nullptr;

    // ---- resolve proposal `move` of the stage: thread per particle
    if (tid < np) {
        const size_t gp = g0 + (size_t)tid;
        const Philox4 ru = philox4x32_10((uint32_t)gp, word, PURPOSE_U, 0u, k0, k1);
        const double u = u53(ru.x, ru.y);
        const double l0 = loglik[gp], q0 = logprior[gp], l1 = prop_loglik[gp], q1 = prop_logprior[gp];
        const bool acc = isfinite(l1) && isfinite(q1) && log(u) < (q1 - q0) + b * (l1 - l0);
        s_acc[tid] = acc ? 1 : 0;
        if (acc) {
            loglik[gp] = l1;
            logprior[gp] = q1;
            accept_count[gp] += 1u;
        }
        if (rec) {
            rec[(size_t)tid * (dd + 2) + dd] = u;
            rec[(size_t)tid * (dd + 2) + dd + 1] = acc ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < np * d; idx += MT)
        if (s_acc[idx / d]) theta[g0 * dd + idx] = prop[g0 * dd + idx];
    __syncthreads();

    // ---- the proposals of move + 1 from the points as they now stand
    if (propose)
        propose_tile<MT>(tid, (uint32_t)g0, np, d, word + 1u, k0, k1, theta + g0 * dd, L + r * dd * dd, prop + g0 * dd, rec, dd + 2,
                         s_z);
}

// what both entry points refuse; `who` names the caller in the message
int check_common(const char* who, size_t R, int N, int d, double tau, double scale, double eps, uint32_t n_mcmc) {
    if (R < 1 || R > (size_t)INT_MAX) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_populations must be in [1, %d]", who, INT_MAX);
    if (N < 2 || N > PEM_SMC_MAX_PARTICLES)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_particles must be in [2, %d]", who, PEM_SMC_MAX_PARTICLES);
    if (d < 1 || d > MAX_DIM) return pem::fail(PEM_ERR_INVALID_ARG, "%s: ndim must be in [1, %d]", who, MAX_DIM);
    if (R * (size_t)N > (size_t)UINT32_MAX)
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_populations n_particles must fit a 32-bit counter word", who);
    if (!(tau > 0.0 && tau < 1.0)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: tau must be in (0, 1)", who);
    if (!(scale > 0.0) || !std::isfinite(scale)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: need a finite scale > 0", who);
    if (!(eps >= 0.0)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: need eps >= 0", who);
    if (n_mcmc == 0) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_mcmc must be at least 1", who);
    return PEM_OK;
}

}  // namespace

extern "C" int pem_smc_stage_f64_dev(size_t n_populations, int n_particles, int ndim, uint64_t seed, double tau, double scale,
                                     double eps, uint32_t n_mcmc, double* theta, double* loglik, double* logprior, double* beta,
                                     double* log_evidence, uint64_t* stage, double* L, double* prop, uint32_t* accept_count,
                                     uint64_t* accepted, uint32_t* flags, uint32_t* moves_active, double* scratch,
                                     double* hist_beta, double* hist_ess, double* hist_accept, double* hist_dlogz,
                                     size_t history_len, double* record, pem_stream_t stream) {
    if (int rc = check_common("pem_smc_stage", n_populations, n_particles, ndim, tau, scale, eps, n_mcmc)) return rc;
    if (!theta || !loglik || !logprior || !beta || !log_evidence || !stage || !L || !prop || !accept_count || !accepted || !flags ||
        !moves_active || !scratch || !hist_beta || !hist_ess || !hist_accept || !hist_dlogz)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_smc_stage: NULL array");
    if (history_len == 0) return pem::fail(PEM_ERR_INVALID_ARG, "pem_smc_stage: the history needs history_len >= 1");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(smc_stage_kernel, dim3((unsigned)n_populations), dim3(ST), 0, static_cast<hipStream_t>(stream), n_particles,
                       ndim, (uint32_t)seed, (uint32_t)(seed >> 32), tau, scale * scale, eps, n_mcmc, theta, loglik, logprior, beta,
                       log_evidence, stage, L, prop, accept_count, accepted, flags, moves_active, scratch, hist_beta, hist_ess,
                       hist_accept, hist_dlogz, (uint64_t)history_len, record);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

extern "C" int pem_smc_move_f64_dev(size_t n_populations, int n_particles, int ndim, uint64_t seed, double tau, double scale,
                                    double eps, uint32_t n_mcmc, uint32_t move, int propose, double* theta, double* loglik,
                                    double* logprior, const double* beta, const uint64_t* stage, const double* L, double* prop,
                                    const double* prop_loglik, const double* prop_logprior, uint32_t* accept_count,
                                    const uint32_t* moves_active, double* record, pem_stream_t stream) {
    if (int rc = check_common("pem_smc_move", n_populations, n_particles, ndim, tau, scale, eps, n_mcmc)) return rc;
    if (move < 1 || move > n_mcmc) return pem::fail(PEM_ERR_INVALID_ARG, "pem_smc_move: move must be in [1, n_mcmc]");
    if (move == n_mcmc && propose)   // its normals would be drawn under the counter word of the next stage's first proposals
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_smc_move: the last move of a stage proposes nothing: propose must be 0");
    if (!theta || !loglik || !logprior || !beta || !stage || !L || !prop || !prop_loglik || !prop_logprior || !accept_count ||
        !moves_active)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_smc_move: NULL array");
    const size_t blocks_per_pop = ((size_t)n_particles + PB - 1) / PB;
    if (n_populations * blocks_per_pop > (size_t)INT_MAX)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_smc_move: n_populations ceil(n_particles / %d) must be at most %d", PB, INT_MAX);
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(smc_move_kernel, dim3((unsigned)(n_populations * blocks_per_pop)), dim3(MT), 0,
                       static_cast<hipStream_t>(stream), n_particles, ndim, (int)blocks_per_pop, (uint32_t)seed,
                       (uint32_t)(seed >> 32), n_mcmc, move, propose, theta, loglik, logprior, beta, stage, L, prop, prop_loglik,
                       prop_logprior, accept_count, moves_active, record);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
