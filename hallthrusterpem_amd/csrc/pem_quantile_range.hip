// pem_quantile_range.hip -- the multi-rank form of the percentile selection: histograms over caller-given key ranges, one level
// per call (pem_range_hist_f64_dev, pem_range_narrow_dev; gfx950).  Keys, lanes and the streaming loop: csrc/pem_quantile_core.h.
// Samples sharded over ranks cannot be copied out and sorted in one place cheaply, but histograms add: every rank counts its
// own values inside the current range of every wanted rank, the counts are all-reduced (<= 144 KB), all ranks pick the same
// bin and narrow the range to it -- until a range is one key (hallthrusterpem_amd/percentiles.py drives the levels).
// Range r of column c: keys klo[c][r] .. khi[c][r]; d = (k - klo) >> shift with shift such that the span fits 31 bits;
// bin = d when the shifted span is smaller than `bins` (every key its own bin: the next range is a single key), else
// floor(d mult / 2^32), mult = min(2^32 - 1, floor(2^32 bins / (span' + 1))).  percentiles.py inverts exactly this map.
#include "pem_quantile_core.h"

namespace {

struct RangeScale {
    u64 lo, hi;
    unsigned mult;
    int shift, identity;
};
__device__ __forceinline__ RangeScale range_scale(u64 lo, u64 hi, int bins) {
    RangeScale r;
    r.lo = lo;
    r.hi = hi;
    const u64 span = hi >= lo ? hi - lo : 0;
    int shift = 0;
    while ((span >> shift) >> 31) ++shift;
    const u64 d = span >> shift;
    r.shift = shift;
    r.identity = d < (u64)bins;
    const u64 mult = (((u64)bins) << 32) / (d + 1);
    r.mult = mult > 0xffffffffull ? 0xffffffffu : (unsigned)mult;
    return r;
}

template <int NC, int NR>
__global__ __launch_bounds__(QBLOCK) void range_hist_kernel(long long n, int m, size_t ld, const double* __restrict__ data,
                                                             const u64* __restrict__ klo, const u64* __restrict__ khi, int bins,
                                                             unsigned* __restrict__ hist) {
    extern __shared__ unsigned lds_hist[];
    for (int i = threadIdx.x; i < m * NR * bins; i += QBLOCK) lds_hist[i] = 0;
    __syncthreads();
    const Lanes L(m, threadIdx.x & 63);
    RangeScale rs[NC][NR];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
#pragma unroll
        for (int r = 0; r < NR; ++r) rs[j][r] = on ? range_scale(klo[c * NR + r], khi[c * NR + r], bins) : range_scale(1, 0, bins);
    }
    stream_values<NC, (NC >= 4 && NR >= 4) ? 2 : UNROLL>(n, m, ld, data, L, [&](int j, int c, double x) {
        if (x == x) {
            const u64 k = key_of(x);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const RangeScale& q = rs[j][r];
                if (k >= q.lo && k <= q.hi) {
                    const unsigned d = (unsigned)((k - q.lo) >> q.shift);
                    const int b = q.identity ? (int)d : (int)(((u64)d * q.mult) >> 32);
                    atomicAdd(&lds_hist[(c * NR + r) * bins + b], 1u);
                }
            }
        }
    });
    __syncthreads();
    for (int i = threadIdx.x; i < m * NR * bins; i += QBLOCK) {
        const unsigned v = lds_hist[i];
        if (v) atomicAdd(&hist[i], v);
    }
}

// One level's decision on the device (one wave per range): the bin of the all-reduced histogram that holds the wanted rank,
// and the keys of that bin -- the inverse of range_scale's map, as percentiles.bin_interval states it -- become the next range.
__global__ __launch_bounds__(64) void range_narrow_kernel(int bins, const unsigned* __restrict__ hist, u64* __restrict__ klo,
                                                           u64* __restrict__ khi, long long* __restrict__ resid) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const u64 lo = klo[i], hi = khi[i];
    if (lo >= hi) return;                                     // already one key (or an empty column)
    const Found f = find_bin(hist + (size_t)i * bins, bins, (u64)resid[i], lane);
    if (lane != 0) return;
    const RangeScale q = range_scale(lo, hi, bins);
    const u64 b = (u64)f.bin, two32 = 1ull << 32;
    const u64 d_lo = q.identity ? b : (b * two32 + q.mult - 1) / q.mult;
    const u64 d_hi = q.identity ? b : ((b + 1) * two32 + q.mult - 1) / q.mult - 1;
    const bool last = d_hi >= ((hi - lo) >> q.shift);
    u64 nlo = lo + (d_lo << q.shift);
    u64 nhi = last ? hi : lo + (((d_hi + 1) << q.shift) - 1);
    if (nlo < lo) nlo = lo;
    if (nhi > hi) nhi = hi;
    klo[i] = nlo;
    khi[i] = nhi;
    resid[i] -= (long long)f.before;
}

}  // namespace

extern "C" int pem_range_hist_f64_dev(size_t n, int m, const double* data, size_t ld, int nr, const uint64_t* klo, const uint64_t* khi,
                                      int bins, uint32_t* hist, pem_stream_t stream) {
    if (m < 1 || m > 64 * MAX_NC) return pem::fail(PEM_ERR_INVALID_ARG, "pem_range_hist: 1 <= m <= %d columns", 64 * MAX_NC);
    if (nr != 1 && nr != 2 && nr != 4 && nr != 6) return pem::fail(PEM_ERR_INVALID_ARG, "pem_range_hist: 1, 2, 4 or 6 ranges per column");
    if (bins < 1 || (long long)m * nr * bins > LDS_WORDS)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_range_hist: m * nr * bins must not exceed %d", LDS_WORDS);
    if (ld < (size_t)m) return pem::fail(PEM_ERR_INVALID_ARG, "pem_range_hist: leading dimension smaller than m");
    if (!klo || !khi || !hist || (n && !data)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_range_hist: NULL array");
    if (int rc = pem::check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(hist, 0, sizeof(uint32_t) * (size_t)m * nr * bins, st));
    if (n == 0) return PEM_OK;
    const dim3 grid = stream_grid(n, m), blk(QBLOCK);
    const size_t lds = (size_t)m * nr * bins * 4;
    HIP_TRY(with_columns_and(columns_per_lane(m), nr, RangeCounts{}, RangeCounts{}, [&](auto NC, auto NR) {
        return launch_lds<range_hist_kernel<NC(), NR()>>(grid, blk, lds, st, (long long)n, m, ld, data, (const u64*)klo, (const u64*)khi, bins,
                                                          (unsigned*)hist);
    }));
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

extern "C" int pem_range_narrow_dev(int n_ranges, int bins, const uint32_t* hist, uint64_t* klo, uint64_t* khi, int64_t* resid,
                                    pem_stream_t stream) {
    if (n_ranges < 1 || bins < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_range_narrow: need ranges and bins");
    if (!hist || !klo || !khi || !resid) return pem::fail(PEM_ERR_INVALID_ARG, "pem_range_narrow: NULL array");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(range_narrow_kernel, dim3((unsigned)n_ranges), dim3(64), 0, static_cast<hipStream_t>(stream), bins,
                       (const unsigned*)hist, (u64*)klo, (u64*)khi, (long long*)resid);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
