// pem_qmc.hip -- the low-discrepancy design of the sampling loops: a Sobol' sequence with a random digital shift.
//
// What it stands in for: the `sampler='sobol'` designs users of a Saltelli / forward-UQ code expect (SALib,
// scipy.stats.sobol_indices); the reference delegates sampling to amisc / uqtils (absent), so parity is UNPINNED: the formulas are
// this library's own, restated in numpy by tests/qmc_np.py and pinned there against torch.quasirandom.SobolEngine and
// scipy.stats.qmc.Sobol(bits=30).
//
// Value (i, d) of a design = transform_d( (x + 0.5) 2^-30 ),  x = XOR_{j in gray(i)} v[d][j]  ^  s_d,
// with v the 30-bit Joe-Kuo direction numbers (csrc/pem_sobol_seq.h) and s_d the shift of dimension d (csrc/pem_qmc.h): a pure
// function of (seed, stream, index, dimension) like the Philox designs of pem_sampler.hip, so any sharding is the same design.
// Saltelli blocks: matrix B is sequence dimensions ndim .. 2 ndim - 1 of the same points.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_qmc.h"

namespace {

constexpr int MAXDIM = PEM_SAMPLE_MAX_DIM;
static_assert(MAXDIM == PEM_SOBOL_DIMS, "one direction-number row per sampler dimension");

struct QmcTable {
    int32_t kind[MAXDIM];
    double a[MAXDIM], b[MAXDIM];
    uint32_t shift[MAXDIM];      // by SEQUENCE dimension (matrix B of a Saltelli block uses ndim .. 2 ndim - 1)
};

// out of line, as in sample_kernel: inlined, the library exp / normcdfinv bodies take the kernel to one wave per SIMD
__device__ __attribute__((noinline)) double transform_call_q(int kind, double a, double b, double u) { return pem::transform(kind, a, b, u); }

// One lane per sample.  The grid walks 64-ALIGNED groups of the global index: group base `gbase` (a multiple of 64) + k, so that
// the upper 24 Gray-code bits are wave-uniform: lane d folds them for dimension d (pem::qmc_wave_part) together with the dimension's
// shift, every lane of the wave taking part.  The first `lead` = first_index % 64 lanes of the first group and the lanes past the
// end then write nothing.  Column of sample k: k - lead.
__global__ __launch_bounds__(256) void sobol_sample_kernel(long long n_lanes, uint32_t gbase, int lead, int ndim, QmcTable tab, int swap_dim,
                                                           double* __restrict__ out, size_t ld) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    // the sequence dimension behind column `lane` of this block (matrix B of a Saltelli block: ndim .. 2 ndim - 1) and its shift
    const int my_sd = lane < ndim ? ((swap_dim == -2 || swap_dim == lane) ? lane + ndim : lane) : 0;
    const uint32_t my_shift = lane < ndim ? tab.shift[my_sd] : 0u;
    for (long long kw = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); kw < n_lanes; kw += stride) {    // wave-uniform
        const long long k = kw + lane;
        const uint32_t g = gbase + (uint32_t)k;                 // < 2^30 for every lane that writes (checked by the host)
        const uint32_t gw = gbase + (uint32_t)kw;
        const uint32_t gray_lane = g ^ (g >> 1), gray_wave = gw ^ (gw >> 1);
        const uint32_t wave_part = lane < ndim ? pem::qmc_wave_part(gray_wave, my_sd) ^ my_shift : 0u;
        if (k < lead || k >= n_lanes) continue;
        double* col = out + (k - lead);
        for (int d = 0; d < ndim; ++d) {
            const int sd = (swap_dim == -2 || swap_dim == d) ? d + ndim : d;       // wave-uniform
            const uint32_t x = __builtin_amdgcn_readlane(wave_part, d) ^ pem::qmc_lane_part(gray_lane, sd);
            col[(size_t)d * ld] = transform_call_q(tab.kind[d], tab.a[d], tab.b[d], pem::qmc_uniform(x));
        }
    }
}

}  // namespace

extern "C" {

int pem_sobol_directions(int dim, uint32_t* out30) {
    if (dim < 0 || dim >= PEM_SOBOL_DIMS) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sobol_directions: dim must be in [0, %d)", PEM_SOBOL_DIMS);
    if (!out30) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sobol_directions: NULL array");
    for (int j = 0; j < PEM_SOBOL_BITS; ++j) out30[j] = PEM_SOBOL_V[dim][j];
    return PEM_OK;
}

int pem_sample_sobol_f64_dev(size_t n, uint64_t first_index, uint64_t seed, uint32_t stream_id, int scramble, int ndim,
                             const int32_t* kind, const double* a, const double* b, int swap_dim, double* out, size_t ld,
                             pem_stream_t stream) {
    if (ndim < 1 || ndim > MAXDIM) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample_sobol: ndim must be in [1, %d]", MAXDIM);
    if (!kind || !a || !b || !out) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample_sobol: NULL array");
    if (ld < n) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample_sobol: leading dimension smaller than n");
    if (swap_dim < -2 || swap_dim >= ndim) return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample_sobol: swap_dim out of range");
    if (swap_dim != -1 && 2 * ndim > MAXDIM)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample_sobol: a Saltelli block takes 2 ndim <= %d sequence dimensions", MAXDIM);
    if (first_index > pem::QMC_MAX_POINTS || n > pem::QMC_MAX_POINTS - first_index)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample_sobol: indices exceed the 2^%d points of the sequence", PEM_SOBOL_BITS);
    for (int d = 0; d < ndim; ++d)
        if (kind[d] < 0 || kind[d] > PEM_DIST_NORMAL)
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_sample_sobol: unknown distribution kind %d for dimension %d", kind[d], d);
    if (n == 0) return PEM_OK;
    if (int rc = pem::check_device()) return rc;
    QmcTable tab;
    for (int d = 0; d < MAXDIM; ++d) {
        tab.kind[d] = d < ndim ? kind[d] : 0;
        tab.a[d] = d < ndim ? a[d] : 0.0;
        tab.b[d] = d < ndim ? b[d] : 0.0;
        tab.shift[d] = pem::qmc_shift(seed, stream_id, scramble, d);
    }
    const int lead = (int)(first_index & 63u);
    const size_t n_lanes = n + (size_t)lead;
    size_t blocks = (n_lanes + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(sobol_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), (long long)n_lanes,
                       (uint32_t)(first_index - (uint64_t)lead), lead, ndim, tab, swap_dim, out, ld);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // extern "C"
