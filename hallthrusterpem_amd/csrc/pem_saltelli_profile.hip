// pem_saltelli_profile.hip -- first-order and total Sobol' sums of the whole 91-angle j_ion profile as ONE launch per shard (gfx950).
//
// What it stands in for: the Saltelli design of pem_saltelli.hip with the ion current density profile (plume.py:99-107) as the
// output instead of three scalars -- d + 2 design blocks, d + 2 stored profiles of 728 B per base sample and 4 d 91 reductions when
// composed from `Design.fill`, `CoupledBatch(profile=True)` and torch.  Here the rows A and B of a base sample are generated once
// (pem_saltelli_model.h: the numbers of the other Saltelli launches), the model runs on A, B and AB_j (A with column varied[j] from
// B) up to the beam amplitudes, the 91 values of every evaluation are formed in registers, and only the sums below reach HBM.
//
// One evaluation at angle k, alpha_k = k (pi/2) / 90 and alpha_90 = pi/2 exactly, without contraction (plume.py:99-102):
//     t1 = alpha_k / a1,  t2 = alpha_k / a2,  j_k = X1a exp(-(t1 t1)) + X2a exp(-(t2 t2)) + j_cex
// a1, a2, X1a, X2a, j_cex from the stage code of Model64::eval (cathode_vcc, thruster_stage, plume_setup, normaliser); exp is
// pem_model::exp_nonpos (the argument is never positive).  a1 <= 0, or any j_k <= 0, makes the whole row 1e-20 (plume.py:105-107).
// f_k = j_k (norm 0) or log10 j_k by pem_log10_tab (norm 1).
//
// partial: [n_blocks][2 + 4 nv][91] doubles, c_k the centre of angle k:
//   row 0        sum (fA - c) + (fB - c)
//   row 1        sum (fA - c)^2 + (fB - c)^2
//   row 2 + 4 j  sum t1,    t1 = (fB - c) (fAB_j - fA)
//   row 3 + 4 j  sum t1^2
//   row 4 + 4 j  sum t2,    t2 = (fA - fAB_j)^2
//   row 5 + 4 j  sum t2^2
// flags: [n_blocks][2] = non-physical thruster results and invalid plume rows among all n_base (nv + 2) evaluations.
//
// A workgroup of four waves takes tiles of 64 consecutive base samples (64-aligned in the global index on the Sobol' design, as the
// other launches walk it).  The waves do two different jobs, and never the other's: a lane that carried the 62 running sums (124
// registers) through the model's scalar stages spilled 40 to 110 of them.
//   wave 3, lane per sample: generates rows A and B (B waits in LDS, read back by its own lane), runs the stage code on the nv + 2
//       evaluations in a rolled loop and leaves the five scalars of each, and its invalid bit, in LDS (42.5 KB + 1 KB).  The bit is
//       decided here: a1 <= 0, or -- only when X1a >= 0, X2a >= 0, j_cex > 0 does not already make every j_k positive -- the 91
//       values themselves, by the expression the other waves use (row_has_nonpositive, out of line)
//   waves 0..2, lane per angle: lanes 0..90 take the even samples of the tile, lanes 96..186 the odd ones (10 of 192 idle), each with
//       its 2 + 4 nv sums in registers.  The scalars arrive as LDS broadcasts.  An AB_j whose a1 (a2) has the bits of A's reuses A's
//       exponential: the same bits, and under a fixed P_b only c1, c2, c3 change a width
// Two barriers per tile hand the scalars over and back.  A term passes through one addition per sample its lane sees, one for the two
// halves of the workgroup, and the sum over the workgroups.  One deterministic partial per workgroup, no floating-point atomics.
// LDS: 72 KB with the log10 table (16 KB) and the normaliser's polynomials (3 KB): two workgroups per CU, two waves per SIMD.
#include "pem_math.h"
#include "pem_saltelli_model.h"

namespace {

constexpr int NA = pem_model::NANG;          // 91
constexpr int TILE = 64;                     // base samples per tile: the lanes of the wave that evaluates the stages
constexpr int WG = 256;                      // lanes per workgroup
constexpr int CONSUMERS = 192;               // lanes of waves 0..2
constexpr int HALF = 96;                     // lanes per half of them (91 hold an angle)
constexpr int NE = NIN + 2;                  // evaluations per base sample at most
constexpr int NSC = 5;                       // a1, a2, X1a, X2a, j_cex
constexpr int MAXROWS = 2 + 4 * NIN;
constexpr int SCAL_DOUBLES = NE * TILE * NSC;
constexpr int XB_DOUBLES = NIN * TILE;
constexpr int POOL_DOUBLES = SCAL_DOUBLES + XB_DOUBLES;
static_assert(MAXROWS * HALF <= POOL_DOUBLES, "the final reduction reuses the pool");
constexpr double FILL = 1e-20;

struct ProfileArg {
    const double* centre;                    // 91 device doubles, or nullptr: zeros
    double torr2pa, radius;
};

__device__ __forceinline__ double beam_exp(double alpha, double a) {
#pragma clang fp contract(off)
    const double t = alpha / a;
    return pem_model::exp_nonpos(-(t * t));
}

__device__ __forceinline__ double profile_j(double X1a, double X2a, double j_cex, double e1, double e2) {
#pragma clang fp contract(off)
    return X1a * e1 + X2a * e2 + j_cex;
}

__device__ __forceinline__ double angle_of(int k) { return k == NA - 1 ? pem_model::HALF_PI : (double)k * pem_model::GRID_H; }

// does any of the 91 values of a row come out <= 0?  Never called under the PEM-v0 priors (X1a, X2a >= 0 and j_cex > 0 there)
__device__ __attribute__((noinline)) bool row_has_nonpositive(double a1, double a2, double X1a, double X2a, double j_cex) {
    bool bad = false;
    for (int k = 0; k < NA; ++k) {
        const double alpha = angle_of(k);
        bad = bad || profile_j(X1a, X2a, j_cex, beam_exp(alpha, a1), beam_exp(alpha, a2)) <= 0.0;
    }
    return bad;
}

template <bool QMC, int NORM>
__device__ __forceinline__ void profile_body(long long n, const SaltelliArg& s, const ProfileArg& pa, const unsigned int* shift,
                                             double* __restrict__ partial, uint64_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) double pool[POOL_DOUBLES];     // scalars [NE][TILE][NSC] | row B [NIN][TILE]
    __shared__ __attribute__((aligned(16))) double logtab[NORM ? pem::LOG_TABLE_DOUBLES : 2];
    __shared__ double dpoly[PEM_NDI * PEM_NDC];
    __shared__ unsigned char inv[NE][TILE];
    __shared__ int lds_kind[NIN + 1], lds_varied[NIN + 1];
    __shared__ double lds_ab[2 * NIN];
    __shared__ unsigned int bad[2];
    double* const scal = pool;
    double* const xb_lds = pool + SCAL_DOUBLES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (NORM) pem::load_log_table(logtab, tid, WG);
    for (int i = tid; i < PEM_NDI * PEM_NDC; i += WG) dpoly[i] = PEM_DPOLY[i];
    if (tid < NIN) {
        lds_kind[tid] = s.kind[tid];
        lds_varied[tid] = s.varied[tid];
        lds_ab[2 * tid] = s.a[tid];
        lds_ab[2 * tid + 1] = s.b[tid];
    }
    __syncthreads();
    const int nv = s.nv, nrows = 2 + 4 * nv;
    const long long lead = QMC ? (long long)(s.first & 63ull) : 0;
    const long long ntiles = (n + lead + TILE - 1) / TILE;

    if (wave == 3) {
        // ---- the stages, lane per sample
        using namespace pem_model;
        const double k_pa = pa.torr2pa, rad = pa.radius;
        const double inv_r2 = 1.0 / (rad * rad), inv_2pi_r2 = 1.0 / (2.0 * PEM_PI * (rad * rad));
        unsigned int bad_thruster = 0, bad_plume = 0;
        for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            const long long i = tile * TILE - lead + lane;            // the lane's base sample (local index)
            const bool live = i >= 0 && i < n;
            // (QMC: a lane that is not live forms the point of its own index: every point is a valid input)
            const unsigned long long g = s.first + (unsigned long long)(QMC || live ? i : n - 1);
            unsigned int gray_lane = 0, wave_part = 0;
            if (QMC) {
                const unsigned int gw = (unsigned int)g & ~63u;
                gray_lane = (unsigned int)g ^ ((unsigned int)g >> 1);
                if (lane < 2 * NIN) wave_part = pem::qmc_wave_part(gw ^ (gw >> 1), lane) ^ shift[lane];
            }
            double xa[NIN];
            {
                double xb[NIN];
                if (QMC) design_row_qmc(lds_kind, lds_ab, gray_lane, wave_part, NIN, xb);
                else design_row(s, lds_kind, lds_ab, g, s.stream + 1u, xb);
#pragma unroll
                for (int col = 0; col < NIN; ++col) xb_lds[col * TILE + lane] = xb[col];     // read back by this lane only: no barrier
                asm volatile("" ::: "memory");                        // (keeps row B out of the registers, as in pem_saltelli.hip)
            }
            if (QMC) design_row_qmc(lds_kind, lds_ab, gray_lane, wave_part, 0, xa);
            else design_row(s, lds_kind, lds_ab, g, s.stream, xa);
            for (int e = 0; e < nv + 2; ++e) {                        // 0: A, 1: B, 2 + j: A with column varied[j] from B
                const int d = e >= 2 ? __builtin_amdgcn_readfirstlane(lds_varied[e - 2]) : -1;
                double x[NIN];
#pragma unroll
                for (int col = 0; col < NIN; ++col) x[col] = (e == 1 || col == d) ? xb_lds[col * TILE + lane] : xa[col];
                // (the lines of Model64::eval up to the beam amplitudes)
                const double V_cc = cathode_vcc(x[0], x[1], x[2], x[3], x[4], x[5], k_pa);
                const ThrusterQoI th = thruster_stage(x[1], V_cc, x[6], x[7]);
                const PlumeSetup ps = plume_setup(x[0], x[9], x[10], x[11], x[12], x[13], k_pa);
                const double a1 = ps.a1, a2 = ps.a2;
                const double u1 = 1.0 / (a1 * a1), u2 = 1.0 / (a2 * a2);
                const double A1 = (1.0 - x[8]) / normaliser(a1, u1, dpoly);
                const double A2 = x[8] / normaliser(a2, u2, dpoly);
                const double decay = exp(-rad * ps.n_neutral * x[14]);
                const double j_cex = th.I_B0 * (1.0 - decay) * inv_2pi_r2;
                const double base = th.I_B0 * decay * inv_r2;
                const double X1a = base * A1, X2a = base * A2;
                bool invalid = a1 <= 0.0;
                if (!invalid && !(X1a >= 0.0 && X2a >= 0.0 && j_cex > 0.0)) invalid = row_has_nonpositive(a1, a2, X1a, X2a, j_cex);
                double* sc = scal + (e * TILE + lane) * NSC;
                sc[0] = a1;
                sc[1] = a2;
                sc[2] = X1a;
                sc[3] = X2a;
                sc[4] = j_cex;
                inv[e][lane] = invalid ? 1 : 0;
                if (live) {
                    bad_thruster += (th.T < 0.0 || th.I_B0 < 0.0) ? 1u : 0u;
                    bad_plume += invalid ? 1u : 0u;
                }
            }
            __syncthreads();                                          // the scalars are there
            __syncthreads();                                          // ... and have been read
        }
        // the counts of the wave, by the butterfly of the other launches
        double v[8] = {(double)bad_thruster, (double)bad_plume, 0, 0, 0, 0, 0, 0};
        const double tot = pem::wave_sum8(v, lane);
        if (lane < 8 && pem::wave_sum8_slot(lane) < 2) bad[pem::wave_sum8_slot(lane)] = (unsigned int)tot;
        __syncthreads();
        __syncthreads();
        if (lane < 2) flags[(size_t)blockIdx.x * 2 + lane] = (uint64_t)bad[lane];
    } else {
        // ---- the profile and the sums, lane per angle
        const int half = tid >= HALF ? 1 : 0, k = tid - half * HALF;
        const bool has_angle = k < NA;
        const double alpha = angle_of(has_angle ? k : 0);
        const double c = (has_angle && pa.centre) ? pa.centre[k] : 0.0;
        double acc[MAXROWS];
#pragma unroll
        for (int r = 0; r < MAXROWS; ++r) acc[r] = 0.0;
        for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            const long long i0 = tile * TILE - lead;
            __syncthreads();
            if (has_angle) {
                for (int p = 0; p < TILE / 2; ++p) {
                    const int sidx = 2 * p + half;
                    const long long i = i0 + sidx;
                    if (i < 0 || i >= n) continue;
                    const double* sa = scal + sidx * NSC;
                    const double a1A = sa[0], a2A = sa[1];
                    const double e1A = beam_exp(alpha, a1A), e2A = beam_exp(alpha, a2A);
                    double jA = profile_j(sa[2], sa[3], sa[4], e1A, e2A);
                    if (inv[0][sidx]) jA = FILL;
                    const double* sb = scal + (TILE + sidx) * NSC;
                    double jB = profile_j(sb[2], sb[3], sb[4], beam_exp(alpha, sb[0]), beam_exp(alpha, sb[1]));
                    if (inv[1][sidx]) jB = FILL;
                    const double fA = NORM ? pem::pem_log10_tab(jA, logtab) : jA;
                    const double fB = NORM ? pem::pem_log10_tab(jB, logtab) : jB;
                    const double vA = fA - c, vB = fB - c;
                    acc[0] += vA + vB;
                    acc[1] += fma(vA, vA, vB * vB);
#pragma unroll
                    for (int j = 0; j < NIN; ++j) {
                        if (j < nv) {
                            const double* sj = scal + ((2 + j) * TILE + sidx) * NSC;
                            const double a1 = sj[0], a2 = sj[1];
                            double e1 = e1A, e2 = e2A;
                            if (__double_as_longlong(a1) != __double_as_longlong(a1A)) e1 = beam_exp(alpha, a1);
                            if (__double_as_longlong(a2) != __double_as_longlong(a2A)) e2 = beam_exp(alpha, a2);
                            double jj = profile_j(sj[2], sj[3], sj[4], e1, e2);
                            if (inv[2 + j][sidx]) jj = FILL;
                            const double fAB = NORM ? pem::pem_log10_tab(jj, logtab) : jj;
                            const double dd = fAB - fA;
                            const double t1 = vB * dd, t2 = dd * dd;
                            acc[2 + 4 * j] += t1;
                            acc[3 + 4 * j] += t1 * t1;
                            acc[4 + 4 * j] += t2;
                            acc[5 + 4 * j] += t2 * t2;
                        }
                    }
                }
            }
            __syncthreads();
        }
        // one partial per workgroup: the odd half through LDS (the pool is free now), added to the even half
        __syncthreads();
        if (half == 1 && has_angle) {
#pragma unroll
            for (int r = 0; r < MAXROWS; ++r)
                if (r < nrows) pool[r * HALF + k] = acc[r];
        }
        __syncthreads();
        if (half == 0 && has_angle) {
            double* out = partial + (size_t)blockIdx.x * nrows * NA + k;
#pragma unroll
            for (int r = 0; r < MAXROWS; ++r)
                if (r < nrows) out[(size_t)r * NA] = acc[r] + pool[r * HALF + k];
        }
    }
}

// 62 sums per lane are 124 registers; two waves per SIMD leave each 256
template <int NORM>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
void saltelli_profile_kernel(long long n, SaltelliArg s, ProfileArg pa, double* __restrict__ partial, uint64_t* __restrict__ flags) {
    profile_body<false, NORM>(n, s, pa, nullptr, partial, flags);
}

template <int NORM>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
void saltelli_profile_qmc_kernel(long long n, SaltelliArg s, ProfileArg pa, QmcShifts shifts, double* __restrict__ partial,
                                 uint64_t* __restrict__ flags) {
    profile_body<true, NORM>(n, s, pa, shifts.s, partial, flags);
}

template <bool QMC>
int launch(const char* who, size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind, const double* a,
           const double* b, int n_varied, const int32_t* varied, int norm, const double* centre, double torr2pa, double radius,
           double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream, int scramble = 0) {
    if (!kind || !a || !b || !partial || !flags) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if (n_varied < 0 || n_varied > NIN) return pem::fail(PEM_ERR_INVALID_ARG, "%s: 0 <= n_varied <= %d", who, NIN);
    if (n_varied > 0 && !varied) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL varied", who);
    if (norm != 0 && norm != 1) return pem::fail(PEM_ERR_INVALID_ARG, "%s: norm must be 0 (none) or 1 (log10)", who);
    if (n_blocks < 1) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_blocks must be positive", who);
    if (!(radius > 0.0)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: radius must be positive", who);
    if (QMC && (first_index > pem::QMC_MAX_POINTS || n_base > pem::QMC_MAX_POINTS - first_index))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: indices exceed the 2^%d points of the sequence", who, PEM_SOBOL_BITS);
    if (int rc = pem::check_device()) return rc;
    const size_t nrows = 2 + 4 * (size_t)n_varied;
    if (n_base == 0) {   // an empty shard contributes zero to every sum
        HIP_TRY(hipMemsetAsync(partial, 0, (size_t)n_blocks * nrows * NA * sizeof(double), static_cast<hipStream_t>(stream)));
        HIP_TRY(hipMemsetAsync(flags, 0, (size_t)n_blocks * 2 * sizeof(uint64_t), static_cast<hipStream_t>(stream)));
        return PEM_OK;
    }
    SaltelliArg s{};
    s.seed = seed;
    s.first = first_index;
    s.stream = stream_id;
    s.nv = n_varied;
    for (int d = 0; d < NIN; ++d) {
        if (kind[d] < PEM_DIST_UNIFORM || kind[d] > PEM_DIST_NORMAL)
            return pem::fail(PEM_ERR_INVALID_ARG, "%s: unknown distribution kind %d for input %d", who, kind[d], d);
        s.kind[d] = kind[d];
        s.a[d] = a[d];
        s.b[d] = b[d];
        s.varied[d] = 0;
    }
    for (int j = 0; j < n_varied; ++j) {
        if (varied[j] < 0 || varied[j] >= NIN) return pem::fail(PEM_ERR_INVALID_ARG, "%s: varied[%d] = %d out of range", who, j, varied[j]);
        s.varied[j] = varied[j];
    }
    const ProfileArg pa{centre, torr2pa, radius};
    const dim3 grid((unsigned)n_blocks), block(WG);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (QMC) {
        QmcShifts shifts;
        for (int d = 0; d < 2 * NIN; ++d) shifts.s[d] = pem::qmc_shift(seed, stream_id, scramble, d);
        if (norm) hipLaunchKernelGGL(saltelli_profile_qmc_kernel<1>, grid, block, 0, st, (long long)n_base, s, pa, shifts, partial, flags);
        else hipLaunchKernelGGL(saltelli_profile_qmc_kernel<0>, grid, block, 0, st, (long long)n_base, s, pa, shifts, partial, flags);
    } else {
        if (norm) hipLaunchKernelGGL(saltelli_profile_kernel<1>, grid, block, 0, st, (long long)n_base, s, pa, partial, flags);
        else hipLaunchKernelGGL(saltelli_profile_kernel<0>, grid, block, 0, st, (long long)n_base, s, pa, partial, flags);
    }
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // namespace

extern "C" {

int pem_saltelli_profile_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                                 const double* a, const double* b, int n_varied, const int32_t* varied, int norm, const double* centre,
                                 double torr2pa, double radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<false>("pem_saltelli_profile_f64", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, norm, centre,
                         torr2pa, radius, partial, flags, n_blocks, stream);
}

// the same launch with rows A and B taken from the shifted Sobol' sequence, as pem_saltelli_qmc_f64_dev takes them
int pem_saltelli_profile_qmc_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble,
                                     const int32_t* kind, const double* a, const double* b, int n_varied, const int32_t* varied, int norm,
                                     const double* centre, double torr2pa, double radius, double* partial, uint64_t* flags, int n_blocks,
                                     pem_stream_t stream) {
    return launch<true>("pem_saltelli_profile_qmc_f64", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, norm, centre,
                        torr2pa, radius, partial, flags, n_blocks, stream, scramble);
}

}  // extern "C"
