// pem_jacobian.hip -- the Jacobian of the coupled fp64 model written out, and the sums of a derivative-based sensitivity study as
// ONE launch per shard (gfx950).
//
// pem_coupled_jacobian_f64_dev: a lane per sample runs pem_jacobian.h's jacobian() on inputs read from HBM and writes the three
// QoIs, the columns of d f / d x that were asked for, and the two flag bits of the evaluation.
//
// pem_gradient_sums_f64_dev / pem_gradient_sums_qmc_f64_dev: what they stand in for is `Design.sample` (a [15][n] block in HBM),
// the launch above (3 + 3 d more rows) and 3 (2 + 2 d + d (d + 1) / 2) reductions over them.  Here row A of the design is generated
// on chip (pem_saltelli_model.h: the numbers of the Saltelli launches, bit-identical to `Design.sample`), jacobian() runs on it, the
// gradient is taken in the prior's own coordinate z_i -- x_i, or log10 x_i for PEM_DIST_LOGUNIFORM: g_i = (x_i ln 10) df/dx_i -- and
// only the sums reach HBM.  partial[n_blocks][rows][3], per QoI q with centre c_q and d = n_varied:
//   row 0                 sum (f - c)
//   row 1                 sum (f - c)^2
//   rows 2 .. 1 + d       sum g_i
//   rows 2 + d .. 1 + 2d  sum g_i^4
//   rows 2 + 2d ..        sum g_i g_j, i <= j, the upper triangle row by row
// flags[n_blocks][3]: non-physical thruster results, invalid plume rows, skipped samples.  A sample with an f or a g that is not
// finite is skipped: it adds an exact zero to every sum of every QoI.
//
// 3 x 152 sums at d = 15 do not fit a lane that also evaluates the model (pem_saltelli2.hip met the same with its pairs), so a
// wave works in two roles on its tile of 64 samples.  Lane per sample: the design row, jacobian(), and for one QoI at a time the
// 2 + d numbers 1, f - c, g_0 .. g_{d-1} of the sample into the wave's [64][17] block of LDS (zeros for a skipped or absent
// sample; stride 17: the lanes of either role hit different banks).  Lane per row: lane l owns rows l, l + 64 and l + 128 of each
// QoI -- nine running sums in registers -- and adds, sample after sample in the tile's order, the product of two of those numbers
// (squared for g^4).  A term passes through one addition per sample of the tiles its wave sees, three for the four waves of the
// workgroup, and the sum over the workgroups: a fixed order, one deterministic partial per workgroup, no floating-point atomics.
// The workgroup walks groups of four tiles (64-aligned in the global index on the Sobol' design, as the other launches walk it)
// with two barriers per QoI.  LDS: 22.5 KB of tables (Model64::stage) + 34 KB of blocks: two workgroups per CU, two waves per SIMD.
#include "pem_jacobian.h"

namespace {

constexpr int WG = 256;                      // lanes per workgroup
constexpr int WAVES = WG / 64;
constexpr int TILE = 64;                     // samples per wave and tile
constexpr int NS = 2 + NIN;                  // numbers per sample and QoI: 1, f - c, g_0 .. g_14
constexpr int OWN = 3;                       // rows per lane
constexpr int MAXROWS = 2 + 2 * NIN + NIN * (NIN + 1) / 2;     // 152
constexpr int POOL_DOUBLES = WAVES * TILE * NS;
constexpr double LN10 = 2.302585092994045684;
static_assert(MAXROWS <= OWN * 64, "a wave owns every row");
static_assert(WAVES * NQ * OWN * 64 <= POOL_DOUBLES, "the final reduction reuses the blocks");

struct JacArg {
    int nv;
    int varied[NIN];
};

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < __builtin_inf(); }

// ---- the Jacobian written out ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
void coupled_jacobian_kernel(long long n, const double* __restrict__ x, JacArg a, double torr2pa, double radius,
                             double* __restrict__ qoi, double* __restrict__ jac, unsigned char* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) unsigned char tables[Model64::LDS_BYTES];
    __shared__ int lds_varied[NIN + 1];
    const int tid = threadIdx.x;
    Model64 m;
    m.stage(tables, tid, WG, torr2pa, radius);
    if (tid < NIN) lds_varied[tid] = a.varied[tid];
    __syncthreads();
    const int nv = a.nv;
    for (long long i = (long long)blockIdx.x * WG + tid; i < n; i += (long long)gridDim.x * WG) {
        double xv[NIN];
#pragma unroll
        for (int c = 0; c < NIN; ++c) xv[c] = x[(size_t)c * n + i];
        const Jac o = jacobian(m, xv);
#pragma unroll
        for (int q = 0; q < NQ; ++q) qoi[(size_t)q * n + i] = o.f[q];
        flags[i] = (unsigned char)((o.bad_thruster ? 1 : 0) | (o.invalid ? 2 : 0));
        for (int j = 0; j < nv; ++j) {
            const int iv = __builtin_amdgcn_readfirstlane(lds_varied[j]);
            double e[NQ], xi;
            o.entries(iv, xv, e, xi);
#pragma unroll
            for (int q = 0; q < NQ; ++q) jac[((size_t)q * nv + j) * n + i] = e[q];
        }
    }
}

// ---- the fused launch -----------------------------------------------------------------------------------------------------------
// row r of the partial is the sum of s[ia] s[ib] (squared where sq) over the samples, s = (1, f - c, g_0 .. g_{d-1})
__device__ __forceinline__ void row_factors(int r, int d, int& ia, int& ib, bool& sq) {
    ia = ib = 0;
    sq = false;
    if (r == 0) {
        ia = 1;
    } else if (r == 1) {
        ia = ib = 1;
    } else if (r < 2 + d) {
        ia = r;
    } else if (r < 2 + 2 * d) {
        ia = ib = r - d;
        sq = true;
    } else {
        int t = r - (2 + 2 * d), i = 0;
        while (i < d && t >= d - i) {
            t -= d - i;
            ++i;
        }
        if (i < d) {
            ia = 2 + i;
            ib = 2 + i + t;
        }
    }
}

template <bool QMC>
__device__ __forceinline__ void gradient_body(long long n, const SaltelliArg& s, const double* centre, double torr2pa, double radius,
                                              const unsigned int* shift, double* __restrict__ partial, uint64_t* __restrict__ flags) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) unsigned char tables[Model64::LDS_BYTES];
    __shared__ __attribute__((aligned(16))) double pool[POOL_DOUBLES];
    __shared__ int lds_kind[NIN + 1], lds_varied[NIN + 1];
    __shared__ double lds_ab[2 * NIN];
    __shared__ unsigned int counts[WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Model64 m;
    m.stage(tables, tid, WG, torr2pa, radius);
    if (tid < NIN) {
        lds_kind[tid] = s.kind[tid];
        lds_varied[tid] = s.varied[tid];
        lds_ab[2 * tid] = s.a[tid];
        lds_ab[2 * tid + 1] = s.b[tid];
    }
    __syncthreads();
    const int nv = s.nv, nrows = 2 + 2 * nv + nv * (nv + 1) / 2;
    const long long lead = QMC ? (long long)(s.first & 63ull) : 0;
    const long long ntiles = (n + lead + TILE - 1) / TILE;
    const long long ngroups = (ntiles + WAVES - 1) / WAVES;
    double* const blk = pool + wave * (TILE * NS);

    int ia[OWN], ib[OWN];
    bool sq[OWN];
#pragma unroll
    for (int o = 0; o < OWN; ++o) row_factors(lane + 64 * o, nv, ia[o], ib[o], sq[o]);
    double c[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) c[q] = centre ? centre[q] : 0.0;
    double acc[NQ][OWN];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int o = 0; o < OWN; ++o) acc[q][o] = 0.0;
    unsigned int bad_thruster = 0, bad_plume = 0, skipped = 0;

    for (long long group = blockIdx.x; group < ngroups; group += gridDim.x) {
        const long long tile = group * WAVES + wave;
        const long long i = tile * TILE - lead + lane;            // the lane's sample (local index)
        const bool live = i >= 0 && i < n;
        double xa[NIN];
#pragma unroll
        for (int col = 0; col < NIN; ++col) xa[col] = 0.0;
        Jac jc{};
        bool ok = false;
        if (tile < ntiles) {                                      // (wave-uniform; a tile past the end holds no sample)
            // (QMC: a lane that is not live forms the point of its own index: every point is a valid input)
            const unsigned long long g = s.first + (unsigned long long)(QMC || live ? i : n - 1);
            if (QMC) {
                const unsigned int gw = (unsigned int)g & ~63u;
                const unsigned int gray_lane = (unsigned int)g ^ ((unsigned int)g >> 1);
                unsigned int wave_part = 0;
                if (lane < 2 * NIN) wave_part = pem::qmc_wave_part(gw ^ (gw >> 1), lane) ^ shift[lane];
                design_row_qmc(lds_kind, lds_ab, gray_lane, wave_part, 0, xa);
            } else {
                design_row(s, lds_kind, lds_ab, g, s.stream, xa);
            }
            jc = jacobian(m, xa);
            ok = live && finite_d(jc.f[0]) && finite_d(jc.f[1]) && finite_d(jc.f[2]);
            for (int j = 0; j < nv; ++j) {
                const int iv = __builtin_amdgcn_readfirstlane(lds_varied[j]);
                const int kd = __builtin_amdgcn_readfirstlane(lds_kind[iv]);
                double e[NQ], xi;
                jc.entries(iv, xa, e, xi);
                if (kd == PEM_DIST_LOGUNIFORM) {
                    const double sc = xi * LN10;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) e[q] = sc * e[q];
                }
                ok = ok && finite_d(e[0]) && finite_d(e[1]) && finite_d(e[2]);
            }
            if (live) {
                bad_thruster += jc.bad_thruster ? 1u : 0u;
                bad_plume += jc.invalid ? 1u : 0u;
                skipped += ok ? 0u : 1u;
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double* sv = blk + lane * NS;
            sv[0] = ok ? 1.0 : 0.0;
            sv[1] = ok ? jc.f[q] - c[q] : 0.0;
            for (int j = 0; j < nv; ++j) {
                const int iv = __builtin_amdgcn_readfirstlane(lds_varied[j]);
                const int kd = __builtin_amdgcn_readfirstlane(lds_kind[iv]);
                double e[NQ], xi;
                jc.entries(iv, xa, e, xi);
                double gq = e[q];
                if (kd == PEM_DIST_LOGUNIFORM) gq = (xi * LN10) * gq;
                sv[2 + j] = ok ? gq : 0.0;
            }
            __syncthreads();                                      // the numbers of this QoI are there
            for (int smp = 0; smp < TILE; ++smp) {
                const double* sr = blk + smp * NS;
#pragma unroll
                for (int o = 0; o < OWN; ++o) {
                    double p = sr[ia[o]] * sr[ib[o]];
                    if (sq[o]) p = p * p;
                    acc[q][o] += p;
                }
            }
            __syncthreads();                                      // ... and have been read
        }
    }

    // one partial per workgroup: the four waves' sums added in the order of the waves
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int o = 0; o < OWN; ++o) pool[((wave * NQ + q) * OWN + o) * 64 + lane] = acc[q][o];
    {
        double v[8] = {(double)bad_thruster, (double)bad_plume, (double)skipped, 0, 0, 0, 0, 0};
        const double tot = pem::wave_sum8(v, lane);
        if (lane < 8 && pem::wave_sum8_slot(lane) < 3) counts[wave][pem::wave_sum8_slot(lane)] = (unsigned int)tot;
    }
    __syncthreads();
    for (int idx = tid; idx < nrows * NQ; idx += WG) {
        const int r = idx / NQ, q = idx - r * NQ;
        double t = pool[((0 * NQ + q) * OWN) * 64 + r];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += pool[((w * NQ + q) * OWN) * 64 + r];
        partial[((size_t)blockIdx.x * nrows + r) * NQ + q] = t;
    }
    if (tid < 3) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += counts[w][tid];
        flags[(size_t)blockIdx.x * 3 + tid] = t;
    }
}

template <bool QMC>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
void gradient_sums_kernel(long long n, SaltelliArg s, const double* centre, double torr2pa, double radius, QmcShifts shifts,
                          double* __restrict__ partial, uint64_t* __restrict__ flags) {
    gradient_body<QMC>(n, s, centre, torr2pa, radius, shifts.s, partial, flags);
}

int check_varied(const char* who, int n_varied, const int32_t* varied) {
    if (n_varied < 0 || n_varied > NIN) return pem::fail(PEM_ERR_INVALID_ARG, "%s: 0 <= n_varied <= %d", who, NIN);
    if (n_varied > 0 && !varied) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL varied", who);
    for (int j = 0; j < n_varied; ++j)
        if (varied[j] < 0 || varied[j] >= NIN) return pem::fail(PEM_ERR_INVALID_ARG, "%s: varied[%d] = %d out of range", who, j, varied[j]);
    return PEM_OK;
}

template <bool QMC>
int launch(const char* who, size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind, const double* a,
           const double* b, int n_varied, const int32_t* varied, const double* centre, double torr2pa, double radius, double* partial,
           uint64_t* flags, int n_blocks, pem_stream_t stream, int scramble = 0) {
    if (!kind || !a || !b || !partial || !flags) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if (int rc = check_varied(who, n_varied, varied)) return rc;
    if (n_blocks < 1) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_blocks must be positive", who);
    if (!(radius > 0.0)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: radius must be positive", who);
    if (QMC && (first_index > pem::QMC_MAX_POINTS || n > pem::QMC_MAX_POINTS - first_index))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: indices exceed the 2^%d points of the sequence", who, PEM_SOBOL_BITS);
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
        s.varied[d] = d < n_varied ? varied[d] : 0;
    }
    if (int rc = pem::check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nrows = 2 + 2 * (size_t)n_varied + (size_t)n_varied * (n_varied + 1) / 2;
    if (n == 0) {   // an empty shard contributes zero to every sum
        HIP_TRY(hipMemsetAsync(partial, 0, (size_t)n_blocks * nrows * NQ * sizeof(double), st));
        HIP_TRY(hipMemsetAsync(flags, 0, (size_t)n_blocks * 3 * sizeof(uint64_t), st));
        return PEM_OK;
    }
    QmcShifts shifts{};
    if (QMC)
        for (int d = 0; d < 2 * NIN; ++d) shifts.s[d] = pem::qmc_shift(seed, stream_id, scramble, d);
    hipLaunchKernelGGL(gradient_sums_kernel<QMC>, dim3((unsigned)n_blocks), dim3(WG), 0, st, (long long)n, s, centre, torr2pa, radius, shifts,
                       partial, flags);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // namespace

extern "C" {

int pem_coupled_jacobian_f64_dev(size_t n, const double* x, int n_varied, const int32_t* varied, double torr2pa, double radius,
                                 double* qoi, double* jac, uint8_t* flags, pem_stream_t stream) {
    const char* who = "pem_coupled_jacobian_f64";
    if (int rc = check_varied(who, n_varied, varied)) return rc;
    if (!(radius > 0.0)) return pem::fail(PEM_ERR_INVALID_ARG, "%s: radius must be positive", who);
    if (n > 0 && (!x || !qoi || !flags || (n_varied > 0 && !jac))) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if (n == 0) return PEM_OK;
    if (int rc = pem::check_device()) return rc;
    JacArg a{};
    a.nv = n_varied;
    for (int j = 0; j < n_varied; ++j) a.varied[j] = varied[j];
    const size_t blocks = (n + WG - 1) / WG;
    hipLaunchKernelGGL(coupled_jacobian_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(WG), 0, static_cast<hipStream_t>(stream),
                       (long long)n, x, a, torr2pa, radius, qoi, jac, flags);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int pem_gradient_sums_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind, const double* a,
                              const double* b, int n_varied, const int32_t* varied, const double* centre, double torr2pa, double radius,
                              double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<false>("pem_gradient_sums_f64", n, first_index, seed, stream_id, kind, a, b, n_varied, varied, centre, torr2pa, radius,
                         partial, flags, n_blocks, stream);
}

// the same launch with row A taken from the shifted Sobol' sequence, as pem_saltelli_qmc_f64_dev takes it
int pem_gradient_sums_qmc_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble, const int32_t* kind,
                                  const double* a, const double* b, int n_varied, const int32_t* varied, const double* centre,
                                  double torr2pa, double radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<true>("pem_gradient_sums_qmc_f64", n, first_index, seed, stream_id, kind, a, b, n_varied, varied, centre, torr2pa, radius,
                        partial, flags, n_blocks, stream, scramble);
}

}  // extern "C"
