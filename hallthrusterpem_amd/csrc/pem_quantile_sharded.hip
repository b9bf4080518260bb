// pem_quantile_sharded.hip -- the percentile selection over samples sharded over ranks, on the single-GPU selection's passes
// (pem_qsel_*; gfx950; round 3).  Keys, binning, lanes, the streaming loop and the selection from a list: csrc/pem_quantile_core.h.
// The level loop (csrc/pem_quantile_range.hip) narrows a key range by 64 bins per streaming pass: eleven passes for 1e7 x 91 values.  The single-GPU
// selection needs four, and its two histograms ADD across ranks just as well: every rank runs the same passes over its own
// rows, the per-column min / max and the two histograms are all-reduced between them (91 x 256 and 91 x 6 x 64 counters:
// nothing on xGMI), every rank takes the same decisions, and what is left per wanted rank -- 1 / (bins1 bins2) of a column --
// is copied out into fixed-length padded lists that are all-gathered and selected from by one workgroup per list.
// hallthrusterpem_amd/percentiles.py drives the stages and restates them in numpy for the gloo rehearsal on the CPU.
// State lives in plain caller-owned device arrays (so that the collectives can run on them):
//   kmin / kmax [m] u64, has_nan [m] i32; hist1 [m][bins1] u32; hist2 [m][nt][bins2] u32;
//   resid [m nt] u64 (in: the wanted 0-based ranks, rewritten to the rank inside the chosen bin, then sub-bin);
//   bin1 / bin2 [m nt] i32; done [m nt] i32 + answer [m nt] u64 (constant columns are decided at once);
//   cand [m nt][L] u64 padded with ~0, cursor [m nt] u32 (values a list was offered: > L means it overflowed).
#include "pem_quantile_core.h"

namespace {

__global__ void qsel_init_kernel(int m, u64* kmin, u64* kmax, int* has_nan) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m) {
        kmin[c] = ~0ull;
        kmax[c] = 0ull;
        has_nan[c] = 0;
    }
}

template <int NC>
__global__ __launch_bounds__(QBLOCK) void qsel_minmax_kernel(long long n, int m, size_t ld, const double* __restrict__ data, u64* __restrict__ kmin,
                                                              u64* __restrict__ kmax, int* __restrict__ has_nan) {
    const Lanes L(m, threadIdx.x & 63);
    u64 lo[NC], hi[NC];
    int nan[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        lo[j] = ~0ull;
        hi[j] = 0ull;
        nan[j] = 0;
    }
    stream_values<NC>(n, m, ld, data, L, [&](int j, int, double x) {
        if (x != x) nan[j] = 1;
        else {
            const u64 k = key_of(x);
            lo[j] = k < lo[j] ? k : lo[j];
            hi[j] = k > hi[j] ? k : hi[j];
        }
    });
    __shared__ u64 s_lo[64 * MAX_NC], s_hi[64 * MAX_NC];
    __shared__ int s_nan[64 * MAX_NC];
    for (int c = threadIdx.x; c < m; c += QBLOCK) {
        s_lo[c] = ~0ull;
        s_hi[c] = 0ull;
        s_nan[c] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        if (L.active && c < m) {
            if (lo[j] <= hi[j]) {
                atomicMin(&s_lo[c], lo[j]);
                atomicMax(&s_hi[c], hi[j]);
            }
            if (nan[j]) atomicOr(&s_nan[c], 1);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < m; c += QBLOCK) {
        if (s_lo[c] <= s_hi[c]) {
            atomicMin(&kmin[c], s_lo[c]);
            atomicMax(&kmax[c], s_hi[c]);
        }
        if (s_nan[c]) atomicOr(&has_nan[c], 1);
    }
}

template <int NC>
__global__ __launch_bounds__(QBLOCK) void qsel_hist1_kernel(long long n, int m, size_t ld, const double* __restrict__ data, const u64* __restrict__ kmin,
                                                             const u64* __restrict__ kmax, int bins1, unsigned* __restrict__ hist1) {
    extern __shared__ unsigned lds_hist[];
    for (int i = threadIdx.x; i < m * bins1; i += QBLOCK) lds_hist[i] = 0;
    __syncthreads();
    const Lanes L(m, threadIdx.x & 63);
    Scale sc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
        sc[j] = on ? column_scale(kmin[c], kmax[c], bins1) : column_scale(1, 0, bins1);
    }
    stream_values<NC>(n, m, ld, data, L, [&](int j, int c, double x) {
        if (x == x) {
            unsigned frac;
            atomicAdd(&lds_hist[c * bins1 + bin_of(key_of(x), sc[j], frac)], 1u);
        }
    });
    __syncthreads();
    for (int i = threadIdx.x; i < m * bins1; i += QBLOCK) {
        const unsigned v = lds_hist[i];
        if (v) atomicAdd(&hist1[i], v);
    }
}

// one wave per (column, target): the bin of the (all-reduced) histogram that holds the wanted rank
__global__ __launch_bounds__(64) void qsel_decide1_kernel(int nt, const u64* __restrict__ kmin, const u64* __restrict__ kmax,
                                                           const unsigned* __restrict__ hist1, int bins1, u64* __restrict__ resid,
                                                           int* __restrict__ bin1, int* __restrict__ done, u64* __restrict__ answer) {
    const int i = blockIdx.x, lane = threadIdx.x, c = i / nt;
    if (kmin[c] >= kmax[c]) {                 // a constant column, or one without a value (its result is NaN anyway)
        if (lane == 0) {
            done[i] = 1;
            answer[i] = kmin[c];
            bin1[i] = -1;
        }
        return;
    }
    const Found f = find_bin(hist1 + (size_t)c * bins1, bins1, resid[i], lane);
    if (lane == 0) {
        done[i] = 0;
        bin1[i] = f.bin;
        resid[i] -= f.before;
    }
}

template <int NC, int NT>
__global__ __launch_bounds__(QBLOCK) void qsel_hist2_kernel(long long n, int m, size_t ld, const double* __restrict__ data, const u64* __restrict__ kmin,
                                                             const u64* __restrict__ kmax, const int* __restrict__ bin1, int bins1, int bins2,
                                                             unsigned* __restrict__ hist2) {
    extern __shared__ unsigned lds_hist[];
    for (int i = threadIdx.x; i < m * NT * bins2; i += QBLOCK) lds_hist[i] = 0;
    __syncthreads();
    const Lanes L(m, threadIdx.x & 63);
    Scale sc[NC];
    int tb[NC][NT];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
        sc[j] = on ? column_scale(kmin[c], kmax[c], bins1) : column_scale(1, 0, bins1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            // targets of a column often share a bin: each DISTINCT bin is counted once, under the first target that has it
            int b = on ? bin1[c * NT + t] : -1;
#pragma unroll
            for (int u = 0; u < t; ++u)
                if (on && bin1[c * NT + u] == b) b = -1;
            tb[j][t] = b;
        }
    }
    // (no high-word test in front of the binning here, as the copy pass has: a first-level bin around the median holds 5-10 % of a
    // column, so nearly every wave instruction has a lane inside one and the test only adds to the work: 1972 -> 2255 us for 1e7 x 91)
    stream_values<NC>(n, m, ld, data, L, [&](int j, int c, double x) {
        if (x == x) {
            unsigned frac;
            const int b = bin_of(key_of(x), sc[j], frac);
            int hit = -1;                                   // at most one target holds a given bin (deduplicated above): one branch, not NT
#pragma unroll
            for (int t = 0; t < NT; ++t) hit = tb[j][t] == b ? t : hit;
            if (hit >= 0) atomicAdd(&lds_hist[(c * NT + hit) * bins2 + subbin_of(frac, bins2)], 1u);
        }
    });
    __syncthreads();
    for (int i = threadIdx.x; i < m * NT * bins2; i += QBLOCK) {
        const unsigned v = lds_hist[i];
        if (v) atomicAdd(&hist2[i], v);
    }
}

// one wave per (column, target): the sub-bin that holds the rank, from the all-reduced counts; how many of THIS rank's values
// sit in it, from the local ones (the histogram of a bin is kept under the column's first target that has it)
__global__ __launch_bounds__(64) void qsel_decide2_kernel(int nt, const unsigned* __restrict__ hist2, const unsigned* __restrict__ hist2_local,
                                                           int bins2, const int* __restrict__ bin1, const int* __restrict__ done,
                                                           u64* __restrict__ resid, int* __restrict__ bin2, u64* __restrict__ count,
                                                           unsigned* __restrict__ count_local) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int c = i / nt, t = i - c * nt;
    if (done[i]) {
        if (lane == 0) {
            bin2[i] = -1;
            count[i] = 0;
            count_local[i] = 0;
        }
        return;
    }
    int first = t;
    for (int u = t - 1; u >= 0; --u)
        if (!done[c * nt + u] && bin1[c * nt + u] == bin1[i]) first = u;
    const Found f = find_bin(hist2 + (size_t)(c * nt + first) * bins2, bins2, resid[i], lane);
    if (lane == 0) {
        bin2[i] = f.bin;
        resid[i] -= f.before;
        count[i] = f.count;
        count_local[i] = hist2_local[(size_t)(c * nt + first) * bins2 + f.bin];
    }
}

// this rank's values of every wanted (bin, sub-bin), one padded list per (column, target) -- only the first target of a column
// with a given pair collects (the others read its list)
template <int NC, int NT>
__global__ __launch_bounds__(QBLOCK) void qsel_compact_kernel(long long n, int m, size_t ld, const double* __restrict__ data, const u64* __restrict__ kmin,
                                                               const u64* __restrict__ kmax, const int* __restrict__ bin1, const int* __restrict__ bin2,
                                                               const int* __restrict__ done, int bins1, int bins2, unsigned list_len,
                                                               u64* __restrict__ cand, unsigned* __restrict__ cursor) {
    // the key range of every collected (bin, sub-bin), found once per workgroup -- thread i bisects for list i -- and shared
    // through LDS: done by every lane for its own columns, the bisections were a quarter of a 1.25e6-row shard's pass
    __shared__ unsigned s_rloh[64 * MAX_NC * 2 * PEM_QUANTILE_MAX_Q], s_rwords[64 * MAX_NC * 2 * PEM_QUANTILE_MAX_Q];
    for (int i = threadIdx.x; i < m * NT; i += QBLOCK) {
        const int c = i / NT, t = i - c * NT;
        bool own = !done[i];
        for (int u = 0; u < t; ++u)
            if (own && !done[c * NT + u] && bin1[c * NT + u] == bin1[i] && bin2[c * NT + u] == bin2[i]) own = false;
        u64 klo = ~0ull, khi = 0ull;
        if (own) keys_of_bin(column_scale(kmin[c], kmax[c], bins1), kmax[c], bins2, (long long)bin1[i] * bins2 + bin2[i], klo, khi);
        if (klo > khi) klo = khi = ~0ull;                       // nothing to collect: a range no value's key lies in
        s_rloh[i] = (unsigned)(klo >> 32);
        s_rwords[i] = (unsigned)(khi >> 32) - (unsigned)(klo >> 32);
    }
    __syncthreads();
    const Lanes L(m, threadIdx.x & 63);
    Scale sc[NC];
    int tb1[NC][NT], tb2[NC][NT];
    unsigned rloh[NC][NT], rwords[NC][NT];                  // high words of the collected sub-bins' key ranges
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
        sc[j] = on ? column_scale(kmin[c], kmax[c], bins1) : column_scale(1, 0, bins1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            bool own = on && !done[c * NT + t];
#pragma unroll
            for (int u = 0; u < t; ++u)
                if (own && !done[c * NT + u] && bin1[c * NT + u] == bin1[c * NT + t] && bin2[c * NT + u] == bin2[c * NT + t]) own = false;
            tb1[j][t] = own ? bin1[c * NT + t] : -1;
            tb2[j][t] = own ? bin2[c * NT + t] : -1;
            rloh[j][t] = on ? s_rloh[c * NT + t] : 0xffffffffu;
            rwords[j][t] = on ? s_rwords[c * NT + t] : 0u;
        }
    }
    stream_values<NC>(n, m, ld, data, L, [&](int j, int c, double x) {
        const unsigned kh = key_high(x);
        bool near = false;
#pragma unroll
        for (int t = 0; t < NT; ++t) near |= kh - rloh[j][t] <= rwords[j][t];
        if (near && x == x) {
            const u64 k = key_of(x);
            unsigned frac;
            const int b = bin_of(k, sc[j], frac);
            const int sb = subbin_of(frac, bins2);
            int hit = -1;                                   // list owners have distinct (bin, sub-bin) pairs: at most one matches
#pragma unroll
            for (int t = 0; t < NT; ++t) hit = (tb1[j][t] == b && tb2[j][t] == sb) ? t : hit;
            if (hit >= 0) {
                const unsigned at = atomicAdd(&cursor[c * NT + hit], 1u);
                if (at < list_len) cand[(size_t)(c * NT + hit) * list_len + at] = k;
            }
        }
    });
}

// one workgroup per (column, target): x_(resid) of the union of every rank's list of its (bin, sub-bin)
__global__ __launch_bounds__(QBLOCK) void qsel_select_kernel(int nt, int world, unsigned list_len, size_t rank_stride, const u64* __restrict__ gathered,
                                                              const int* __restrict__ bin1, const int* __restrict__ bin2, const int* __restrict__ done,
                                                              const u64* __restrict__ resid, u64* __restrict__ answer) {
    const int i = blockIdx.x;
    if (done[i]) return;
    const int c = i / nt, t = i - c * nt;
    int owner = t;
    for (int u = t - 1; u >= 0; --u)
        if (!done[c * nt + u] && bin1[c * nt + u] == bin1[i] && bin2[c * nt + u] == bin2[i]) owner = u;
    const u64* base = gathered + (size_t)(c * nt + owner) * list_len;
    const u64 r = select_from([=](u64 k) { return base[(size_t)(k / list_len) * rank_stride + (size_t)(k % list_len)]; },
                              (u64)world * list_len, resid[i], 0xfff0000000000000ull /* key of +inf: the padding lies above it */);
    if (threadIdx.x == 0) answer[i] = r;
}

int qsel_check(const char* who, size_t n, int m, size_t ld, const void* data) {
    if (m < 1 || m > 64 * MAX_NC) return pem::fail(PEM_ERR_INVALID_ARG, "%s: 1 <= m <= %d columns", who, 64 * MAX_NC);
    if (ld < (size_t)m) return pem::fail(PEM_ERR_INVALID_ARG, "%s: leading dimension smaller than m", who);
    if (n && !data) return pem::fail(PEM_ERR_INVALID_ARG, "%s: NULL data", who);
    return pem::check_device();
}

}  // namespace

extern "C" {

int pem_qsel_bins(int m, int nt, int* bins1, int* bins2) {
    if (m < 1 || m > 64 * MAX_NC || nt < 1 || nt > 2 * PEM_QUANTILE_MAX_Q || !bins1 || !bins2)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_bins: 1 <= m <= %d, 1 <= nt <= %d", 64 * MAX_NC, 2 * PEM_QUANTILE_MAX_Q);
    *bins1 = pow2_at_most(LDS_WORDS / m, 4096);
    *bins2 = pow2_at_most(LDS_WORDS / (m * nt), 4096);
    return PEM_OK;
}

int pem_qsel_minmax_f64_dev(size_t n, int m, const double* data, size_t ld, uint64_t* kmin, uint64_t* kmax, int32_t* has_nan,
                            pem_stream_t stream) {
    if (int rc = qsel_check("pem_qsel_minmax", n, m, ld, data)) return rc;
    if (!kmin || !kmax || !has_nan) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_minmax: NULL array");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(qsel_init_kernel, dim3((m + 63) / 64), dim3(64), 0, st, m, (u64*)kmin, (u64*)kmax, (int*)has_nan);
    if (n) {
        with_value(columns_per_lane(m), ColumnCounts{}, [&](auto NC) {
            hipLaunchKernelGGL(qsel_minmax_kernel<NC()>, stream_grid(n, m), dim3(QBLOCK), 0, st, (long long)n, m, ld, data, (u64*)kmin,
                               (u64*)kmax, (int*)has_nan);
        });
    }
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int pem_qsel_hist1_f64_dev(size_t n, int m, const double* data, size_t ld, const uint64_t* kmin, const uint64_t* kmax, int bins1,
                           uint32_t* hist1, pem_stream_t stream) {
    if (int rc = qsel_check("pem_qsel_hist1", n, m, ld, data)) return rc;
    if (!kmin || !kmax || !hist1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_hist1: NULL array");
    if (bins1 < 1 || (long long)m * bins1 > LDS_WORDS) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_hist1: m * bins1 must not exceed %d", LDS_WORDS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(hist1, 0, sizeof(uint32_t) * (size_t)m * bins1, st));
    if (n == 0) return PEM_OK;
    HIP_TRY(with_value(columns_per_lane(m), ColumnCounts{}, [&](auto NC) {
        return launch_lds<qsel_hist1_kernel<NC()>>(stream_grid(n, m), dim3(QBLOCK), (size_t)m * bins1 * 4, st, (long long)n, m, ld, data,
                                                    (const u64*)kmin, (const u64*)kmax, bins1, (unsigned*)hist1);
    }));
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int pem_qsel_decide1_dev(int m, int nt, const uint64_t* kmin, const uint64_t* kmax, const uint32_t* hist1, int bins1, uint64_t* resid,
                         int32_t* bin1, int32_t* done, uint64_t* answer, pem_stream_t stream) {
    if (m < 1 || nt < 1 || bins1 < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_decide1: need columns, targets and bins");
    if (!kmin || !kmax || !hist1 || !resid || !bin1 || !done || !answer) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_decide1: NULL array");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(qsel_decide1_kernel, dim3((unsigned)(m * nt)), dim3(64), 0, static_cast<hipStream_t>(stream), nt, (const u64*)kmin,
                       (const u64*)kmax, (const unsigned*)hist1, bins1, (u64*)resid, (int*)bin1, (int*)done, (u64*)answer);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int pem_qsel_hist2_f64_dev(size_t n, int m, const double* data, size_t ld, const uint64_t* kmin, const uint64_t* kmax, int nt,
                           const int32_t* bin1, int bins1, int bins2, uint32_t* hist2, pem_stream_t stream) {
    if (int rc = qsel_check("pem_qsel_hist2", n, m, ld, data)) return rc;
    if (nt < 2 || nt > 2 * PEM_QUANTILE_MAX_Q || (nt & 1)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_hist2: 2, 4, ... %d targets per column", 2 * PEM_QUANTILE_MAX_Q);
    if (!kmin || !kmax || !bin1 || !hist2) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_hist2: NULL array");
    if (bins1 < 1 || bins2 < 1 || (long long)m * nt * bins2 > LDS_WORDS)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_hist2: m * nt * bins2 must not exceed %d", LDS_WORDS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(hist2, 0, sizeof(uint32_t) * (size_t)m * nt * bins2, st));
    if (n == 0) return PEM_OK;
    const int nc = columns_per_lane(m);
    if (nc == 4 && nt > 2 * PEM_QUANTILE_MAX_Q_WIDE) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_hist2: at most %d targets for more than 128 columns", 2 * PEM_QUANTILE_MAX_Q_WIDE);
    HIP_TRY(with_columns_and(nc, nt, TargetCounts{}, TargetCountsWide{}, [&](auto NC, auto NT) {
        return launch_lds<qsel_hist2_kernel<NC(), NT()>>(stream_grid(n, m), dim3(QBLOCK), (size_t)m * nt * bins2 * 4, st, (long long)n, m, ld, data,
                                                          (const u64*)kmin, (const u64*)kmax, (const int*)bin1, bins1, bins2, (unsigned*)hist2);
    }));
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int pem_qsel_decide2_dev(int m, int nt, const uint32_t* hist2, const uint32_t* hist2_local, int bins2, const int32_t* bin1, const int32_t* done,
                         uint64_t* resid, int32_t* bin2, uint64_t* count, uint32_t* count_local, pem_stream_t stream) {
    if (m < 1 || nt < 1 || bins2 < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_decide2: need columns, targets and bins");
    if (!hist2 || !hist2_local || !bin1 || !done || !resid || !bin2 || !count || !count_local)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_decide2: NULL array");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(qsel_decide2_kernel, dim3((unsigned)(m * nt)), dim3(64), 0, static_cast<hipStream_t>(stream), nt, (const unsigned*)hist2,
                       (const unsigned*)hist2_local, bins2, (const int*)bin1, (const int*)done, (u64*)resid, (int*)bin2, (u64*)count,
                       (unsigned*)count_local);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int pem_qsel_compact_f64_dev(size_t n, int m, const double* data, size_t ld, const uint64_t* kmin, const uint64_t* kmax, int nt,
                             const int32_t* bin1, const int32_t* bin2, const int32_t* done, int bins1, int bins2, uint32_t list_len,
                             uint64_t* cand, uint32_t* cursor, pem_stream_t stream) {
    if (int rc = qsel_check("pem_qsel_compact", n, m, ld, data)) return rc;
    if (nt < 2 || nt > 2 * PEM_QUANTILE_MAX_Q || (nt & 1)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_compact: 2, 4, ... %d targets per column", 2 * PEM_QUANTILE_MAX_Q);
    if (!kmin || !kmax || !bin1 || !bin2 || !done || !cand || !cursor || list_len < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_compact: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(cand, 0xff, sizeof(uint64_t) * (size_t)m * nt * list_len, st));       // padding: ~0, above every key
    HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(uint32_t) * (size_t)m * nt, st));
    if (n == 0) return PEM_OK;
    const int nc = columns_per_lane(m);
    if (nc == 4 && nt > 2 * PEM_QUANTILE_MAX_Q_WIDE) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_compact: at most %d targets for more than 128 columns", 2 * PEM_QUANTILE_MAX_Q_WIDE);
    with_columns_and(nc, nt, TargetCounts{}, TargetCountsWide{}, [&](auto NC, auto NT) {
        hipLaunchKernelGGL((qsel_compact_kernel<NC(), NT()>), stream_grid(n, m), dim3(QBLOCK), 0, st, (long long)n, m, ld,
                           data, (const u64*)kmin, (const u64*)kmax, (const int*)bin1, (const int*)bin2, (const int*)done, bins1, bins2,
                           (unsigned)list_len, (u64*)cand, (unsigned*)cursor);
    });
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

int pem_qsel_select_dev(int m, int nt, int world, uint32_t list_len, const uint64_t* gathered, const int32_t* bin1, const int32_t* bin2,
                        const int32_t* done, const uint64_t* resid, uint64_t* answer, pem_stream_t stream) {
    if (m < 1 || nt < 1 || world < 1 || list_len < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_select: need columns, targets, ranks and a list length");
    if (!gathered || !bin1 || !bin2 || !done || !resid || !answer) return pem::fail(PEM_ERR_INVALID_ARG, "pem_qsel_select: NULL array");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(qsel_select_kernel, dim3((unsigned)(m * nt)), dim3(QBLOCK), 0, static_cast<hipStream_t>(stream), nt, world,
                       (unsigned)list_len, (size_t)m * nt * list_len, (const u64*)gathered, (const int*)bin1, (const int*)bin2, (const int*)done,
                       (const u64*)resid, (u64*)answer);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

}  // extern "C"
