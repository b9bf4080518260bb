// pem_saltelli.hip -- the Saltelli design of BASELINE configs[4] as ONE launch per shard (gfx950).
//
// What it stands in for: scripts/pem_v0/sobol.py:46-118 -- sample the A and B matrices, run the model on A, B and on A
// with column d from B for every varied input d, and form the sums inside `uq.sobol_sa(..., compute_s2=False)` (uqtils,
// third-party and absent: parity UNPINNED; the estimators are stated in hallthrusterpem_amd/drivers.py).
//
// The block-by-block driver (drivers.sobol_indices, fused=False) launches d + 2 coupled evaluations per batch, each
// regenerating all 15 inputs (8 Philox blocks per evaluation), writes QoIs to HBM and reduces them with a second kernel.
// Here, per base sample, the rows A and B of the counter-based design are generated once (16 Philox blocks; the numbers of
// pem_sample_f64_dev), the model runs in a rolled loop around ONE model body -- one sample per lane -- and the six
// estimator terms of an evaluation are summed over the wave at once (a transposing butterfly: 10 additions instead of
// 48) and added to per-wave fp64 accumulators in LDS; only [workgroups][2 + 2 d][3] partial sums reach HBM.
// Two models share the kernel:
//   Model32  csrc/pem_model_f32.h: single-precision arithmetic on the design rounded to float (pem_saltelli_f32_dev)
//   Model64  the fp64 model, lane per sample: the scalar stages and tables of csrc/pem_model.h with the expression of the
//            reduced-QoI table path of plume_r1_kernel (pem_kernels.hip) -- bit-identical to it for "plain" samples --
//            and the literal 91-term sums for the others (pem_saltelli_f64_dev)
#include "pem_saltelli_model.h"

namespace {

// partial: [gridDim.x][2 + 2 nv][NQ]: rows 0,1 = sum fA + fB, sum fA^2 + fB^2; rows 2+2j, 3+2j = sum fB (fAB_j - fA),
// sum (fA - fAB_j)^2 for varied input j.  flags: [gridDim.x][2] = non-physical thruster results (T < 0 or I_B0 < 0,
// thruster.py:490-493) and invalid plume samples among all evaluations.
// One model body, a rolled loop over the nv + 2 evaluations of a base sample (A, B, then A with one column of B); a lane
// carries two design rows and one evaluation, not 2 (nv + 1) x 3 running sums.
// `shift` != nullptr (a compile-time choice, QMC): the rows come from the Sobol' sequence.  The grid then walks 64-aligned groups of
// the global index (the first s.first % 64 lanes of the first group are not live), which makes the upper Gray-code bits wave-uniform.
template <class Model, bool QMC>
__device__ __forceinline__ void saltelli_body(long long n, const SaltelliArg& s, const unsigned int* shift, double torr2pa, double radius,
                                              double* __restrict__ partial, uint64_t* __restrict__ flags) {
    using real = typename Model::real;
    __shared__ __attribute__((aligned(16))) unsigned char lds_model[Model::LDS_BYTES];
    __shared__ int lds_kind[NIN + 1], lds_varied[NIN + 1];
    __shared__ double lds_ab[2 * NIN];
    __shared__ double acc[4][NIN + 1][8];           // [wave][evaluation slot: 0 = the A/B statistics, 1 + j = varied input j][value]
    // row B of the design lives in LDS, one column per input (lane-consecutive: conflict-free): an evaluation needs one value of
    // it (all fifteen only for the B evaluation itself), and held in registers beside row A and the model's own temporaries it
    // pushed the fp64 instantiation past 256 VGPRs (20 spilled, 96 bytes of scratch per lane)
    __shared__ real xb_lds[NIN][256];
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
    for (int i = threadIdx.x; i < 4 * (NIN + 1) * 8; i += 256) (&acc[0][0][0])[i] = 0.0;
    __syncthreads();
    const int nv = s.nv;
    const int my_slot = pem::wave_sum8_slot(lane);
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
        real xa[NIN];
        {
            real xb[NIN];
            if (QMC) design_row_qmc(lds_kind, lds_ab, gray_lane, wave_part, NIN, xb);
            else design_row(s, lds_kind, lds_ab, g, s.stream + 1u, xb);
#pragma unroll
            for (int c = 0; c < NIN; ++c) xb_lds[c][threadIdx.x] = xb[c];     // read back by this lane only: no barrier
            // (a compiler barrier: without it the stores are forwarded to the loads below and row B is back in registers)
            asm volatile("" ::: "memory");
        }
        if (QMC) design_row_qmc(lds_kind, lds_ab, gray_lane, wave_part, 0, xa);
        else design_row(s, lds_kind, lds_ab, g, s.stream, xa);
        double fa[NQ] = {0.0, 0.0, 0.0}, fb[NQ] = {0.0, 0.0, 0.0};
        for (int e = 0; e < nv + 2; ++e) {                    // 0: A, 1: B, 2 + j: A with column varied[j] from B
            const int d = e >= 2 ? __builtin_amdgcn_readfirstlane(lds_varied[e - 2]) : -1;
            real x[NIN];
#pragma unroll
            for (int c = 0; c < NIN; ++c) x[c] = (e == 1 || c == d) ? xb_lds[c][threadIdx.x] : xa[c];
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
            if (e == 1) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    fb[q] = o.f[q];
                    const double a = fa[q], b = o.f[q];
                    v[q] = a + b;
                    v[NQ + q] = fma(a, a, b * b);
                }
            } else {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const double a = fa[q], b = fb[q], ab = o.f[q];
                    v[q] = b * (ab - a);
                    v[NQ + q] = (a - ab) * (a - ab);
                }
            }
            v[6] = v[7] = 0.0;
            if (!live) {
#pragma unroll
                for (int q = 0; q < 6; ++q) v[q] = 0.0;
            }
            const double tot = pem::wave_sum8(v, lane);
            if (lane < 8) acc[wave][e - 1][my_slot] += tot;   // lanes 0..7 carry the eight sums, one each
        }
    }
    {
        double v[8] = {(double)bad_thruster, (double)bad_plume, 0, 0, 0, 0, 0, 0};
        const double tot = pem::wave_sum8(v, lane);
        if (lane < 8 && my_slot < 2) bad[wave][my_slot] = (unsigned int)tot;
    }
    __syncthreads();
    // one partial per workgroup, in a fixed order (deterministic): row 2 j' + {0, 1} x NQ + q  <-  acc[.][j'][{0, 1} NQ + q]
    const int rows = (2 + 2 * nv) * NQ;
    if ((int)threadIdx.x < rows) {
        const int row = threadIdx.x / NQ, q = threadIdx.x - row * NQ, e = row >> 1, which = row & 1;
        partial[(size_t)blockIdx.x * rows + threadIdx.x] =
            acc[0][e][which * NQ + q] + acc[1][e][which * NQ + q] + acc[2][e][which * NQ + q] + acc[3][e][which * NQ + q];
    }
    if (threadIdx.x < 2)
        flags[(size_t)blockIdx.x * 2 + threadIdx.x] = (uint64_t)bad[0][threadIdx.x] + bad[1][threadIdx.x] + bad[2][threadIdx.x] + bad[3][threadIdx.x];
}

template <class Model>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))   // two waves per SIMD: <= 256 registers (the fp64 model takes 277 unconstrained)
void saltelli_kernel(long long n, SaltelliArg s, double torr2pa, double radius,
                                                       double* __restrict__ partial, uint64_t* __restrict__ flags) {
    saltelli_body<Model, false>(n, s, nullptr, torr2pa, radius, partial, flags);
}

template <class Model>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Model::QMC_WAVES)))   // fp32: held to the four waves of the Monte-Carlo launch (130 registers unconstrained)
void saltelli_qmc_kernel(long long n, SaltelliArg s, QmcShifts shifts, double torr2pa, double radius,
                         double* __restrict__ partial, uint64_t* __restrict__ flags) {
    saltelli_body<Model, true>(n, s, shifts.s, torr2pa, radius, partial, flags);
}

template <class Model, bool QMC = false>
int launch(const char* who, size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
           const double* a, const double* b, int n_varied, const int32_t* varied, double torr2pa, double radius, double* partial,
           uint64_t* flags, int n_blocks, pem_stream_t stream, int scramble = 0) {
    if (!kind || !a || !b || !varied || !partial || !flags) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL array", who);
    if (n_varied < 1 || n_varied > NIN) return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 <= n_varied <= %d", who, NIN);
    if (n_blocks < 1) return pem::fail(PEM_ERR_INVALID_ARG, "%s: n_blocks must be positive", who);
    if (QMC && (first_index > pem::QMC_MAX_POINTS || n_base > pem::QMC_MAX_POINTS - first_index))
        return pem::fail(PEM_ERR_INVALID_ARG, "%s: indices exceed the 2^%d points of the sequence", who, PEM_SOBOL_BITS);
    if (int rc = pem::check_device()) return rc;
    if (n_base == 0) {   // an empty shard contributes zero to every sum: the caller adds the partials up whatever n_base was
        HIP_TRY(hipMemsetAsync(partial, 0, (size_t)n_blocks * (2 + 2 * n_varied) * NQ * sizeof(double), static_cast<hipStream_t>(stream)));
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
    if (QMC) {
        QmcShifts shifts;
        for (int d = 0; d < 2 * NIN; ++d) shifts.s[d] = pem::qmc_shift(seed, stream_id, scramble, d);
        hipLaunchKernelGGL(saltelli_qmc_kernel<Model>, dim3((unsigned)n_blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                           (long long)n_base, s, shifts, torr2pa, radius, partial, flags);
    } else {
        hipLaunchKernelGGL(saltelli_kernel<Model>, dim3((unsigned)n_blocks), dim3(256), 0, static_cast<hipStream_t>(stream), (long long)n_base, s,
                           torr2pa, radius, partial, flags);
    }
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // namespace

extern "C" {

int pem_saltelli_f32_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                         const double* a, const double* b, int n_varied, const int32_t* varied, float torr2pa, float radius,
                         double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<Model32>("pem_saltelli_f32", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, torr2pa, radius,
                           partial, flags, n_blocks, stream);
}

int pem_saltelli_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, const int32_t* kind,
                         const double* a, const double* b, int n_varied, const int32_t* varied, double torr2pa, double radius,
                         double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<Model64>("pem_saltelli_f64", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, torr2pa, radius,
                           partial, flags, n_blocks, stream);
}

// the same two launches with rows A and B taken from the shifted Sobol' sequence (sequence dimensions 0..14 and 15..29 of the
// base sample's point; the numbers of pem_sample_sobol_f64_dev) instead of two Philox streams
int pem_saltelli_qmc_f32_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble, const int32_t* kind,
                             const double* a, const double* b, int n_varied, const int32_t* varied, float torr2pa, float radius,
                             double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<Model32, true>("pem_saltelli_qmc_f32", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, torr2pa,
                                 radius, partial, flags, n_blocks, stream, scramble);
}

int pem_saltelli_qmc_f64_dev(size_t n_base, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble, const int32_t* kind,
                             const double* a, const double* b, int n_varied, const int32_t* varied, double torr2pa, double radius,
                             double* partial, uint64_t* flags, int n_blocks, pem_stream_t stream) {
    return launch<Model64, true>("pem_saltelli_qmc_f64", n_base, first_index, seed, stream_id, kind, a, b, n_varied, varied, torr2pa,
                                 radius, partial, flags, n_blocks, stream, scramble);
}

}  // extern "C"
