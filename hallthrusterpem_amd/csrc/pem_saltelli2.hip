// pem_saltelli2.hip -- the Saltelli (2002) design with second-order indices as ONE launch per shard (gfx950).
//
// What it stands in for: `uq.sobol_sa(..., compute_s2=True)` (uqtils, third-party and absent: parity UNPINNED; the estimator is
// stated in hallthrusterpem_amd/drivers.py and DESIGN.md section 4.4).  Per base sample the model runs 2 nv + 2 times:
//   A, B, AB_0 .. AB_{nv-1} (A with column varied[j] from B), BA_0 .. BA_{nv-1} (B with column varied[j] from A)
// in a rolled loop around ONE model body, one base sample per lane, rows A and B generated once (pem_saltelli_model.h: the models
// and the design rows of the first-order launch, pem_saltelli.hip, whose plan this kernel follows).
//
// partial: [n_blocks][rows][3] doubles (columns V_cc, div_angle, T_c), rows = 3 + 4 nv + nv (nv - 1) / 2, c = the centre:
//   0, 1                          sum fA + fB,  sum fA^2 + fB^2
//   2 + 2 j, 3 + 2 j              sum fB (fAB_j - fA),  sum (fA - fAB_j)^2         j < nv: the rows of pem_saltelli_*_dev
//   2 + 2 nv + 2 j, 3 + 2 nv + 2 j    sum fA (fBA_j - fB),  sum (fB - fBA_j)^2     the mirrored first-order and total sums
//   2 + 4 nv                      D = sum (fA - c) (fB - c)
//   3 + 4 nv + p                  C_ij = sum (fBA_i - c) (fAB_j - c),  i < j < nv in the order of `varied`, p counting the pairs
//                                 (i, j) lexicographically: p = i nv - i (i + 1) / 2 + j - i - 1
// flags: [n_blocks][2] = non-physical thruster results and invalid plume samples among all n_base (2 nv + 2) evaluations.
//
// The f(AB_j) of a base sample wait in LDS for the BA evaluations, [nv * 3][256] values of the model's real type (the fp32 model's
// QoIs are floats): lane-consecutive, written and read back by their own lane, no barrier.  After the BA_i evaluation a lane forms
// the 3 (nv - 1 - i) products with f(AB_j), j > i; they are consecutive in that array, and are summed over the wave eight at a time
// by pem::wave_sum8 into per-wave fp64 accumulators in LDS (every input i starts a new group of eight: 46 groups at nv = 15).  The
// array is sized for nv = 15: 90 KB for the fp64 model, beside 19.5 KB of accumulators and 22.5 KB of tables -- ONE workgroup per
// CU, one wave per SIMD, so row B stays in registers (the cap is 512) instead of the 30 KB of LDS the first-order kernel spends on
// it to fit two waves.  The fp32 model: 45 KB, 73 KB in all, two workgroups per CU.
#include "pem_saltelli_model.h"

namespace {

constexpr int PAIR_GROUPS = 46;                       // sum over i < 14 of ceil(3 (14 - i) / 8): the groups of eight at nv = 15
constexpr int SLOTS = 2 + 2 * NIN + PAIR_GROUPS;      // accumulator slots: A/B statistics | first-order | mirror | D | pair groups

struct Centre {
    double c[NQ];
};

template <class Model, bool QMC>
__device__ __forceinline__ void saltelli2_body(long long n, const SaltelliArg& s, const Centre& centre, const unsigned int* shift,
                                               double torr2pa, double radius, double* __restrict__ partial, uint64_t* __restrict__ flags) {
    using real = typename Model::real;
    __shared__ __attribute__((aligned(16))) unsigned char lds_model[Model::LDS_BYTES];
    __shared__ int lds_kind[NIN + 1], lds_varied[NIN + 1];
    __shared__ double lds_ab[2 * NIN];
    __shared__ double acc[4][SLOTS][8];               // [wave][slot][value]
    __shared__ real fab_lds[NIN * NQ][256];           // [3 j + q][thread]: f_q(AB_j) of the thread's base sample (Model32: a float, exactly)
    __shared__ unsigned int bad[4][2];
    Model model;
    model.stage(lds_model, threadIdx.x, 256, torr2pa, radius);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < NIN) {
        lds_kind[threadIdx.x] = s.kind[threadIdx.x];
        lds_varied[threadIdx.x] = s.varied[threadIdx.x];
        lds_ab[2 * threadIdx.x] = s.a[threadIdx.x];
        lds_ab[2 * threadIdx.x + 1] = s.b[threadIdx.x];
    }
    for (int i = threadIdx.x; i < 4 * SLOTS * 8; i += 256) (&acc[0][0][0])[i] = 0.0;
    __syncthreads();
    const int nv = s.nv;
    const int my_slot = pem::wave_sum8_slot(lane);
    const double c[NQ] = {centre.c[0], centre.c[1], centre.c[2]};
    unsigned int bad_thruster = 0, bad_plume = 0;
    // every wave runs the same number of iterations (the reductions inside need all 64 lanes): lanes past n evaluate
    // the last sample and contribute zeros
    const long long stride = (long long)gridDim.x * 256;
    const long long lead = QMC ? (long long)(s.first & 63ull) : 0;
    const long long iters = (n + lead + stride - 1) / stride;
    for (long long it = 0; it < iters; ++it) {
        const long long i = it * stride + (long long)blockIdx.x * 256 + threadIdx.x - lead;
        const bool live = QMC ? (i >= 0 && i < n) : i < n;
        // (QMC: a lane that is not live evaluates the point of its own index, whatever that is: every point is a valid input)
        const unsigned long long g = s.first + (unsigned long long)(QMC || live ? i : n - 1);
        unsigned int gray_lane = 0, wave_part = 0;
        if (QMC) {               // (every lane of the wave is here, live or not)
            const unsigned int gw = (unsigned int)g & ~63u;
            gray_lane = (unsigned int)g ^ ((unsigned int)g >> 1);
            if (lane < 2 * NIN) wave_part = pem::qmc_wave_part(gw ^ (gw >> 1), lane) ^ shift[lane];
        }
        real xa[NIN], xb[NIN];
        if (QMC) {
            design_row_qmc(lds_kind, lds_ab, gray_lane, wave_part, NIN, xb);
            design_row_qmc(lds_kind, lds_ab, gray_lane, wave_part, 0, xa);
        } else {
            design_row(s, lds_kind, lds_ab, g, s.stream + 1u, xb);
            design_row(s, lds_kind, lds_ab, g, s.stream, xa);
        }
        double fa[NQ] = {0.0, 0.0, 0.0}, fb[NQ] = {0.0, 0.0, 0.0};
        int pair_slot = 2 + 2 * nv;                           // the first group of eight of the pairs (i, .) of the BA_i at hand
        for (int e = 0; e < 2 * nv + 2; ++e) {                // 0: A, 1: B, 2 + j: AB_j, 2 + nv + j: BA_j
            const bool ba = e >= nv + 2;
            const int j = ba ? e - nv - 2 : e - 2;
            const int d = e >= 2 ? __builtin_amdgcn_readfirstlane(lds_varied[j]) : -1;
            const bool from_b = e == 1 || ba;
            real x[NIN];
#pragma unroll
            for (int col = 0; col < NIN; ++col) x[col] = (from_b != (col == d)) ? xb[col] : xa[col];
            const Eval o = model.eval(x);
            if (live) {
                bad_thruster += o.bad_thruster;
                bad_plume += o.invalid;
            }
            if (e == 0) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) fa[q] = o.f[q];
                continue;
            }
            double v[8];
            int slot;
            if (e == 1) {
                slot = 0;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    fb[q] = o.f[q];
                    const double a = fa[q], b = o.f[q];
                    v[q] = a + b;
                    v[NQ + q] = fma(a, a, b * b);
                }
            } else if (!ba) {
                slot = 1 + j;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const double a = fa[q], b = fb[q], ab = o.f[q];
                    v[q] = b * (ab - a);
                    v[NQ + q] = (a - ab) * (a - ab);
                    fab_lds[j * NQ + q][threadIdx.x] = (real)ab;
                }
            } else {
                slot = 1 + nv + j;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const double a = fa[q], b = fb[q], bq = o.f[q];
                    v[q] = a * (bq - b);
                    v[NQ + q] = (b - bq) * (b - bq);
                }
            }
            v[6] = v[7] = 0.0;
            if (!live) {
#pragma unroll
                for (int q = 0; q < 6; ++q) v[q] = 0.0;
            }
            {
                const double tot = pem::wave_sum8(v, lane);
                if (lane < 8) acc[wave][slot][my_slot] += tot;   // lanes 0..7 carry the eight sums, one each
            }
            if (e == 1) {                                     // D
#pragma unroll
                for (int q = 0; q < NQ; ++q) v[q] = live ? (fa[q] - c[q]) * (fb[q] - c[q]) : 0.0;
#pragma unroll
                for (int q = NQ; q < 8; ++q) v[q] = 0.0;
                const double tot = pem::wave_sum8(v, lane);
                if (lane < 8) acc[wave][1 + 2 * nv][my_slot] += tot;
            } else if (ba) {
                // the pairs (j, j') with j' > j: value t = 3 (j' - j - 1) + q of them is (f_q(BA_j) - c_q) * (fab_lds[3 (j + 1) + t] - c_q),
                // and q = t % 3.  Within group gr of eight, value k has q = (2 gr + k) % 3: the three factors and centres are rotated
                // once per group (gr is wave-uniform), then picked by a compile-time k % 3.
                const double dba[NQ] = {o.f[0] - c[0], o.f[1] - c[1], o.f[2] - c[2]};
                const int m3 = 3 * (nv - 1 - j), groups = (m3 + 7) >> 3, last = nv * NQ - 1;
                for (int gr = 0; gr < groups; ++gr) {
                    const int r = (2 * gr) % 3;
                    const double rot[NQ] = {r == 0 ? dba[0] : r == 1 ? dba[1] : dba[2], r == 0 ? dba[1] : r == 1 ? dba[2] : dba[0],
                                            r == 0 ? dba[2] : r == 1 ? dba[0] : dba[1]};
                    const double crot[NQ] = {r == 0 ? c[0] : r == 1 ? c[1] : c[2], r == 0 ? c[1] : r == 1 ? c[2] : c[0],
                                             r == 0 ? c[2] : r == 1 ? c[0] : c[1]};
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int t = 8 * gr + k;
                        const int row = min(3 * (j + 1) + t, last);          // (past the last pair: any row in range, the value is dropped)
                        const double w = rot[k % 3] * ((double)fab_lds[row][threadIdx.x] - crot[k % 3]);
                        v[k] = (live && t < m3) ? w : 0.0;
                    }
                    const double tot = pem::wave_sum8(v, lane);
                    if (lane < 8) acc[wave][pair_slot + gr][my_slot] += tot;
                }
                pair_slot += groups;
            }
        }
    }
    {
        double v[8] = {(double)bad_thruster, (double)bad_plume, 0, 0, 0, 0, 0, 0};
        const double tot = pem::wave_sum8(v, lane);
        if (lane < 8 && my_slot < 2) bad[wave][my_slot] = (unsigned int)tot;
    }
    __syncthreads();
    // one partial per workgroup, in a fixed order (deterministic)
    const int npairs = nv * (nv - 1) / 2;
    const int values = (3 + 4 * nv + npairs) * NQ;
    for (int t = threadIdx.x; t < values; t += 256) {
        const int row = t / NQ, q = t - row * NQ;
        int slot, val;
        if (row < 2 + 4 * nv) {                       // statistics, first-order and mirror rows: slot (row / 2), value (row & 1) NQ + q
            slot = row >> 1;
            val = (row & 1) * NQ + q;
        } else if (row == 2 + 4 * nv) {
            slot = 1 + 2 * nv;
            val = q;
        } else {
            int p = row - 3 - 4 * nv, i = 0;
            slot = 2 + 2 * nv;
            while (p >= nv - 1 - i) {
                p -= nv - 1 - i;
                slot += (3 * (nv - 1 - i) + 7) >> 3;
                ++i;
            }
            const int tt = 3 * p + q;
            slot += tt >> 3;
            val = tt & 7;
        }
        partial[(size_t)blockIdx.x * values + t] = acc[0][slot][val] + acc[1][slot][val] + acc[2][slot][val] + acc[3][slot][val];
    }
    if (threadIdx.x < 2)
        flags[(size_t)blockIdx.x * 2 + threadIdx.x] = (uint64_t)bad[0][threadIdx.x] + bad[1][threadIdx.x] + bad[2][threadIdx.x] + bad[3][threadIdx.x];
}

// Model64: one workgroup of 256 per CU (the LDS above: 132 KB), one wave per SIMD, up to 512 registers.  Model32: its f(AB) are floats
// and its tables a third as large, 73 KB: two workgroups per CU, two waves per SIMD, up to 256 registers.
template <class Model>
constexpr int S2_WAVES = sizeof(typename Model::real) == 4 ? 2 : 1;

template <class Model>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(S2_WAVES<Model>, S2_WAVES<Model>)))
void saltelli2_kernel(long long n, SaltelliArg s, Centre centre, double torr2pa, double radius, double* __restrict__ partial,
                      uint64_t* __restrict__ flags) {
    saltelli2_body<Model, false>(n, s, centre, nullptr, torr2pa, radius, partial, flags);
}

template <class Model>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(S2_WAVES<Model>, S2_WAVES<Model>)))
void saltelli2_qmc_kernel(long long n, SaltelliArg s, Centre centre, QmcShifts shifts, double torr2pa, double radius,
                          double* __restrict__ partial, uint64_t* __restrict__ flags) {
    saltelli2_body<Model, true>(n, s, centre, shifts.s, torr2pa, radius, partial, flags);
}

template <class Model, bool QMC = false>
int launch(const char* who, size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
           const double* a, const double* b, int n_varied, const int32_t* varied, const double* centre, double torr2pa, double radius,
           double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream, int scramble = 0) {
    if (!kind || !a || !b || !varied || !centre || !partial || !flags) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if (n_varied < 1 || n_varied > NIN) return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 <= n_varied <= %d", who, NIN);
    if (n_blocks < 1) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_blocks must be positive", who);
    if (QMC && (first_index > pem::QMC_MAX_POINTS || n_base > pem::QMC_MAX_POINTS - first_index))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: indices exceed the 2^%d points of the sequence", who, PEM_SOBOL_BITS);
    if (int rc = pem::check_device()) return rc;
    const size_t rows = 3 + 4 * (size_t)n_varied + (size_t)n_varied * (n_varied - 1) / 2;
    if (n_base == 0) {   // an empty shard contributes zero to every sum: the caller adds the partials up whatever n_base was
        HIP_TRY(hipMemsetAsync(partial, 0, (size_t)n_blocks * rows * NQ * sizeof(double), static_cast<hipStream_t>(stream)));
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
    const Centre c{{centre[0], centre[1], centre[2]}};
    if (QMC) {
        QmcShifts shifts;
        for (int d = 0; d < 2 * NIN; ++d) shifts.s[d] = pem::qmc_shift(seed, stream_id, scramble, d);
        hipLaunchKernelGGL(saltelli2_qmc_kernel<Model>, dim3((unsigned)n_blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                           (long long)n_base, s, c, shifts, torr2pa, radius, partial, flags);
    } else {
        hipLaunchKernelGGL(saltelli2_kernel<Model>, dim3((unsigned)n_blocks), dim3(256), 0, static_cast<hipStream_t>(stream), (long long)n_base, s,
                           c, torr2pa, radius, partial, flags);
    }
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // namespace

extern "C" {

int pem_saltelli2_f32_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                          const double* a, const double* b, int n_varied, const int32_t* varied, const double* centre, float torr2pa,
                          float radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<Model32>("pem_saltelli2_f32", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, centre, torr2pa, radius,
                           partial, flags, n_blocks, stream);
}

int pem_saltelli2_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                          const double* a, const double* b, int n_varied, const int32_t* varied, const double* centre, double torr2pa,
                          double radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<Model64>("pem_saltelli2_f64", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, centre, torr2pa, radius,
                           partial, flags, n_blocks, stream);
}

// the same two launches with rows A and B taken from the shifted Sobol' sequence, as pem_saltelli_qmc_*_dev take them
int pem_saltelli2_qmc_f32_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble, const int32_t* kind,
                              const double* a, const double* b, int n_varied, const int32_t* varied, const double* centre, float torr2pa,
                              float radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<Model32, true>("pem_saltelli2_qmc_f32", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, centre,
                                 torr2pa, radius, partial, flags, n_blocks, stream, scramble);
}

int pem_saltelli2_qmc_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble, const int32_t* kind,
                              const double* a, const double* b, int n_varied, const int32_t* varied, const double* centre, double torr2pa,
                              double radius, double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<Model64, true>("pem_saltelli2_qmc_f64", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, centre,
                                 torr2pa, radius, partial, flags, n_blocks, stream, scramble);
}

}  // extern "C"
