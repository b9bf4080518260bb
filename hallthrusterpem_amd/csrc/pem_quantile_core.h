// pem_quantile_core.h -- what the forms of the percentile selection share: the exact selection over an array, a subsample's
// brackets or a producer's records (csrc/pem_quantile.hip), the level loop over caller-given key ranges
// (csrc/pem_quantile_range.hip) and the selection over samples sharded over ranks (csrc/pem_quantile_sharded.hip).  The
// order-preserving keys and their binning, a lane's columns and the streaming loop, the search in a histogram, the selection
// from a list, and the host's way from a runtime (columns per lane, ranks per column) to a kernel instantiation.
// Everything sits in an unnamed namespace: each unit compiles, and inlines, its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "pem_common.h"
#include "pem_hip.h"

namespace {

typedef unsigned long long u64;
constexpr int QBLOCK = 512;               // two waves per SIMD share one workgroup's LDS histogram
constexpr int QWAVES = QBLOCK / 64;
constexpr int LDS_WORDS = 36864;          // 144 KB of 32-bit counters per workgroup
constexpr int SORT_CAP = 4096;            // keys a workgroup's LDS sort buffer holds (32 KB)
constexpr int SORT_DIRECT = 512;          // ... and sorts without narrowing the list first: a bitonic sort of 4096 keys is 78 passes with a
                                          // barrier each (80 us for the 910 lists of a campaign), one 1024-bin narrowing round three
constexpr int MAX_NC = 4;                 // columns per lane: m <= 256
constexpr int UNROLL = 8;                 // row groups a wave requests before it consumes any (loads in flight per lane: UNROLL x NC)
static_assert(PEM_QUANTILE_MAX_Q == 6, "hist2_kernel / compact_kernel are instantiated for 2, 4, ... 12 ranks per column");

// order-preserving image of a double (NaN excluded by the callers): negative values reversed, sign bit flipped
__device__ __forceinline__ u64 key_of(double x) {
    const u64 b = (u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(u64 k) {
    const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
// the high word of key_of(x) from the high word of x alone (three instructions; the passes below decide nearly every value on it)
__device__ __forceinline__ unsigned key_high(double x) {
    const int bh = __double2hiint(x);
    return (unsigned)bh ^ ((unsigned)(bh >> 31) | 0x80000000u);
}
// Binning of the streaming passes, in integer arithmetic (a u64 -> f64 conversion is six instructions on this chip, and the
// passes over 7 GB were bound by them): d = (k - lo) >> shift fits 31 bits, bin = floor(d * mult / 2^32) with
// mult = floor(2^32 BINS / (D + 1)), D = (hi - lo) >> shift -- never decreases with the key and stays below BINS; the low
// 32 bits of the product are the position inside the bin, scaled to BINS2 sub-bins the same way.
struct Scale {
    u64 lo;
    unsigned mult;
    int shift;
};
__device__ __forceinline__ int bin_of(u64 k, const Scale& s, unsigned& frac) {
    const unsigned d = (unsigned)((k - s.lo) >> s.shift);
    const u64 p = (u64)d * s.mult;
    frac = (unsigned)p;
    return (int)(p >> 32);
}
__device__ __forceinline__ int subbin_of(unsigned frac, int bins2) { return (int)__umulhi(frac, (unsigned)bins2); }
// The keys of bin b (bins2 = 1, g = b) or of sub-bin (b, sb) (g = b bins2 + sb) of a column's binning, [klo, khi], by bisection on
// the monotone map d -> bin(d) bins2 + sub-bin(d).  The streaming passes test a value's HIGH word against these ranges (two 32-bit
// instructions per wanted bin) before they bin it in full: a value outside every wanted bin -- all but a few per cent -- costs
// neither the 64-bit subtraction nor the quarter-rate multiply of bin_of.  An empty bin comes out as klo > khi.
__device__ __forceinline__ void keys_of_bin(const Scale& sc, u64 kmax, int bins2, long long g, u64& klo, u64& khi) {
    const u64 D = kmax >= sc.lo ? (kmax - sc.lo) >> sc.shift : 0;
    auto first = [&](long long G) {
        u64 lo = 0, hi = D + 1;
        while (lo < hi) {
            const u64 mid = (lo + hi) >> 1, prod = mid * sc.mult;
            const long long gd = (long long)(prod >> 32) * bins2 + (bins2 > 1 ? (long long)__umulhi((unsigned)prod, (unsigned)bins2) : 0);
            if (gd >= G) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    };
    const u64 d0 = first(g), d1 = first(g + 1);
    klo = sc.lo + (d0 << sc.shift);
    khi = d1 > D ? kmax : sc.lo + (d1 << sc.shift) - 1;
    if (d0 > D || d0 >= d1) {
        klo = ~0ull;
        khi = 0ull;
    }
}
// the select kernel's own refinement (rare, over short lists): bins in double arithmetic over any key range
__device__ __forceinline__ int bin_of_d(u64 k, u64 lo, double inv, int bins) {
    const int b = (int)((double)(k - lo) * inv);
    return b < bins - 1 ? b : bins - 1;
}
__device__ __forceinline__ Scale column_scale(u64 kmin, u64 kmax, int bins1) {      // scale_columns_kernel, per lane
    Scale sc;
    const u64 span = kmax >= kmin ? kmax - kmin : 0;
    int shift = 0;
    while ((span >> shift) >> 31) ++shift;
    const u64 mult = (((u64)bins1) << 32) / ((span >> shift) + 1);
    sc.lo = kmin;
    sc.shift = shift;
    sc.mult = mult > 0xffffffffull ? 0xffffffffu : (unsigned)mult;
    return sc;
}

struct Column {          // per column
    u64 kmin, kmax;
    int has_nan, pad;    // has_nan: the number of NaNs the min / max pass met (the pilot form's counting pass only flags: 1)
    unsigned mult;       // floor(2^32 BINS1 / (((kmax - kmin) >> shift) + 1))
    int shift;           // so that (kmax - kmin) >> shift < 2^31
};
struct Target {          // per (column, wanted rank)
    u64 rank;            // in: 0-based rank in the column; then the rank inside the current bin / list
    u64 count;           // values in the target's sub-bin (= length of its list)
    u64 offset;          // start of its list in the candidate buffer
    u64 cursor;          // append position during pass 4
    u64 answer;          // the key x_(rank)
    int bin1, bin2;
    int owner;           // index of the target (of this column) whose list this one shares, or its own index
    int done;            // answer already known (constant column)
};

// lane -> the columns it owns.  m <= 64: a wave instruction covers rpw = 64 / m whole rows (lane = row-in-group * m + column);
// m > 64: one row per wave instruction and chunk, column = lane + 64 chunk.
struct Lanes {
    int rpw, active, col0, rsub;
    size_t cs = 1;       // elements between consecutive columns of a row (1: row-major [n][ld]; n with ld = 1: the transposed [m][n])
    __device__ Lanes(int m, int lane, size_t col_stride = 1) : cs(col_stride) {
        if (m <= 64) {
            rpw = 64 / m;
            active = lane < rpw * m;
            col0 = lane % m;
            rsub = lane / m;
        } else {
            rpw = 1;
            active = 1;
            col0 = lane;
            rsub = 0;
        }
    }
};

// Every value of the array once: f(j, column, x) for the lane's j-th column.  A wave takes UNROLL consecutive row groups at a
// time and requests all their values before it consumes the first (with one workgroup of 144 KB of LDS per CU the memory
// latency has to be covered inside the wave).
template <int NC, int U = UNROLL, class F>
__device__ __forceinline__ void stream_values(long long n, int m, size_t ld, const double* __restrict__ data, const Lanes& L, F f) {
    const long long wave = (long long)blockIdx.x * QWAVES + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * QWAVES;
    const long long groups = (n + L.rpw - 1) / L.rpw;
    for (long long g0 = wave * U; g0 < groups; g0 += nwaves * U) {
        double x[U][NC];
        bool ok[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long row = (g0 + u) * L.rpw + L.rsub;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int c = L.col0 + 64 * j;
                ok[u][j] = L.active && c < m && row < n;
                x[u][j] = ok[u][j] ? data[(size_t)row * ld + (size_t)c * L.cs] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (ok[u][j]) f(j, L.col0 + 64 * j, x[u][j]);
        }
    }
}

struct Wanted {          // the call's quantiles travel in the kernel arguments (nq <= 3): no host-to-device copy to wait for
    u64 prev[PEM_QUANTILE_MAX_Q], next[PEM_QUANTILE_MAX_Q];
    double gamma[PEM_QUANTILE_MAX_Q];
};

// The bin of a histogram that holds `rank` (0-based among the counted values), searched by one WAVE: every lane sums a
// chunk of the bins, the lanes' sums are scanned with shuffles, the lane whose chunk holds the rank walks it.  (One thread
// walking 4096 bins in global memory took 0.4-0.9 ms per launch -- more than the four passes over a scalar QoI's data.)
struct Found {
    int bin;
    u64 before;      // values in the bins below
    unsigned count;  // values in the bin
};
__device__ __forceinline__ Found find_bin(const unsigned* __restrict__ h, int bins, u64 rank, int lane) {
    const int per = (bins + 63) / 64, b0 = lane * per;
    u64 mine = 0;
    for (int b = b0; b < b0 + per && b < bins; ++b) mine += h[b];
    u64 incl = mine;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const u64 up = __shfl_up(incl, sh);
        if (lane >= sh) incl += up;
    }
    const unsigned long long holds = __ballot(incl > rank);
    const int src = holds ? __builtin_ctzll(holds) : 63;
    u64 cum = __shfl(incl - mine, src);
    const int s0 = src * per;
    int bin = s0;
    unsigned cnt = 0;
    if (lane == src) {
        int last = s0 + per < bins ? s0 + per : bins;
        for (; bin < last - 1; ++bin) {
            if (cum + h[bin] > rank) break;
            cum += h[bin];
        }
        if (bin > bins - 1) bin = bins - 1;
        cnt = h[bin];
    }
    Found f;
    f.bin = __shfl(bin, src);
    f.before = __shfl(cum, src);
    f.count = (unsigned)__shfl((int)cnt, src);
    return f;
}

// ---- the lists: one workgroup per (column, target) ----------------------------------------------------------------------------
__device__ void block_sort(u64* s, int np2) {      // bitonic, np2 a power of two <= SORT_CAP, all QBLOCK threads
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < np2; i += QBLOCK) {
                const int p = i ^ j;
                if (p > i) {
                    const u64 a = s[i], b = s[p];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        s[i] = b;
                        s[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// x_(rank) of the keys list(0) .. list(len - 1) that lie in [0, top], by one workgroup: sorted in LDS when they fit, narrowed
// by 1024-bin histograms over the list itself until they do (heavy ties) or one key is left.  `list` is any accessor: the
// contiguous candidate list of the single-GPU path, or the padded per-rank pieces of the sharded one (padding = ~0 > top).
// (`short_list`, when given: set if the keys gathered for the sort are not as many as were counted a moment earlier -- a
// slot allocation lost, as the copy pass of the pilot form once did; the caller refuses the result.)
template <class List>
__device__ u64 select_from(const List& list, u64 len, u64 rank, u64 top, int* short_list = nullptr) {
    __shared__ u64 keys[SORT_CAP];
    __shared__ unsigned hist[1024];
    __shared__ u64 s_lo, s_hi, s_cnt, s_rank;
    __shared__ int s_bin;
    u64 lo = 0, hi = top;
    for (;;) {
        // the keys of the list inside [lo, hi]: how many, their smallest and largest
        if (threadIdx.x == 0) {
            s_lo = ~0ull;
            s_hi = 0;
            s_cnt = 0;
        }
        __syncthreads();
        u64 mn = ~0ull, mx = 0, cnt = 0;
        for (u64 i = threadIdx.x; i < len; i += QBLOCK) {
            const u64 k = list(i);
            if (k >= lo && k <= hi) {
                mn = k < mn ? k : mn;
                mx = k > mx ? k : mx;
                ++cnt;
            }
        }
        if (cnt) {
            atomicMin(&s_lo, mn);
            atomicMax(&s_hi, mx);
            atomicAdd(&s_cnt, cnt);
        }
        __syncthreads();
        lo = s_lo;
        hi = s_hi;
        const u64 inside = s_cnt;
        __syncthreads();
        if (lo >= hi) return lo;               // one value left (or, defensively, nothing)
        if (inside <= SORT_DIRECT) {
            int np2 = 1;
            while (np2 < (int)inside) np2 <<= 1;
            if (threadIdx.x == 0) s_cnt = 0;
            for (int i = threadIdx.x; i < np2; i += QBLOCK) keys[i] = ~0ull;
            __syncthreads();
            for (u64 i = threadIdx.x; i < len; i += QBLOCK) {
                const u64 k = list(i);
                if (k >= lo && k <= hi) keys[atomicAdd(&s_cnt, 1ull)] = k;
            }
            __syncthreads();
            if (short_list && threadIdx.x == 0 && s_cnt != inside) atomicExch(short_list, 1);
            block_sort(keys, np2);
            const u64 r = keys[rank < inside ? rank : inside - 1];
            __syncthreads();
            return r;
        }
        // more keys than a short sort takes (or than LDS holds): 1024-bin histogram over [lo, hi], keep the bin that holds the rank
        for (int i = threadIdx.x; i < 1024; i += QBLOCK) hist[i] = 0;
        __syncthreads();
        const double inv = 1024.0 / ((double)(hi - lo) + 1.0);
        for (u64 i = threadIdx.x; i < len; i += QBLOCK) {
            const u64 k = list(i);
            if (k >= lo && k <= hi) atomicAdd(&hist[bin_of_d(k, lo, inv, 1024)], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {                // the bin that holds the rank: one wave, 16 bins per lane, a scan over the lanes' sums
            const int lane = threadIdx.x;
            u64 mine = 0;
#pragma unroll
            for (int b = 0; b < 16; ++b) mine += hist[16 * lane + b];
            u64 incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const u64 up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            const u64 before = incl - mine;
            // the first lane whose running total exceeds the rank owns it (the last lane, defensively, if none does)
            const bool owns = incl > rank && before <= rank;
            const u64 any = __ballot(owns);
            if (any ? owns : lane == 63) {
                u64 cum = before;
                int b = 16 * lane;
                for (; b < 16 * lane + 15; ++b) {
                    if (cum + hist[b] > rank) break;
                    cum += hist[b];
                }
                s_bin = b;
                s_rank = rank - cum;
            }
        }
        __syncthreads();
        const int keep = s_bin;
        rank = s_rank;
        // the keys of that bin form an interval of keys (monotone binning): its ends are found by the next round's min / max
        if (threadIdx.x == 0) {
            s_lo = ~0ull;
            s_hi = 0;
        }
        __syncthreads();
        mn = ~0ull;
        mx = 0;
        for (u64 i = threadIdx.x; i < len; i += QBLOCK) {
            const u64 k = list(i);
            if (k >= lo && k <= hi && bin_of_d(k, lo, inv, 1024) == keep) {
                mn = k < mn ? k : mn;
                mx = k > mx ? k : mx;
            }
        }
        if (mn <= mx) {
            atomicMin(&s_lo, mn);
            atomicMax(&s_hi, mx);
        }
        __syncthreads();
        lo = s_lo;
        hi = s_hi;
        __syncthreads();
    }
}

// ---- the host's side ---------------------------------------------------------------------------------------------------------
inline int pow2_at_most(long long x, int cap) {
    int p = 1;
    while (2LL * p <= x && 2 * p <= cap) p <<= 1;
    return p;
}

// columns a lane owns (Lanes: column = lane + 64 chunk): the NC of the streaming kernels
inline int columns_per_lane(int m) { return m <= 64 ? 1 : (m <= 128 ? 2 : 4); }

// the grid of a streaming pass over n rows (stream_values: a wave takes UNROLL row groups at a time): two workgroups per CU at most
inline dim3 stream_grid(size_t n, int m) {
    const long long rpw = m <= 64 ? 64 / m : 1, groups = ((long long)n + rpw - 1) / rpw;
    long long blocks = (groups + (long long)QWAVES * UNROLL - 1) / ((long long)QWAVES * UNROLL);
    if (blocks > 256 * 2) blocks = 256 * 2;
    if (blocks < 1) blocks = 1;
    return dim3((unsigned)blocks);
}

// From the runtime (nc, nt), (nc, nq) or (nc, nr) to a kernel instantiation: f(Int<NC>{}, Int<N>{}) for the N of the list that
// equals the runtime value -- the last of the list when none does (the callers have refused what is not in it) -- and returns
// what f returns.  Only the listed pairs are instantiated.  More than three quantiles per call for up to 128 columns only: four
// columns per lane with more run out of registers (PEM_QUANTILE_MAX_Q_WIDE) and are not compiled.
template <int V>
using Int = std::integral_constant<int, V>;
template <int... V>
using Ints = std::integer_sequence<int, V...>;
using TargetCounts = Ints<2, 4, 6, 8, 10, 12>;      // NT = 2 NQ targets per column ...
using TargetCountsWide = Ints<2, 4, 6>;             // ... and with four columns per lane
using QuantileCounts = Ints<1, 2, 3, 4, 5, 6>;      // NQ quantiles per call
using QuantileCountsWide = Ints<1, 2, 3>;
using RangeCounts = Ints<1, 2, 4, 6>;               // NR ranges per column of the level loop
using ColumnCounts = Ints<1, 2, 4>;                 // NC

template <class F, int V, int... Rest>
auto with_value(int v, Ints<V, Rest...>, F&& f) {
    if constexpr (sizeof...(Rest) == 0) {
        return f(Int<V>{});
    } else {
        if (v == V) return f(Int<V>{});
        return with_value(v, Ints<Rest...>{}, f);
    }
}
template <class Narrow, class Wide, class F>
auto with_columns_and(int nc, int v, Narrow, Wide, F&& f) {
    if (nc == 1) return with_value(v, Narrow{}, [&](auto N) { return f(Int<1>{}, N); });
    if (nc == 2) return with_value(v, Narrow{}, [&](auto N) { return f(Int<2>{}, N); });
    return with_value(v, Wide{}, [&](auto N) { return f(Int<4>{}, N); });
}

// A launch with more than 64 KB of dynamic LDS: the kernel instantiation's limit is raised first, once per device
// (pem::LdsAttrOnce: one per instantiation), and a failure to raise it is returned instead of a launch that cannot succeed.
template <auto Kernel, int LIMIT = 160 * 1024, class... Args>
hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    static pem::LdsAttrOnce attr;
    const hipError_t e = attr.ensure(reinterpret_cast<const void*>(Kernel), LIMIT);
    if (e == hipSuccess) hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return e;
}

}  // namespace
