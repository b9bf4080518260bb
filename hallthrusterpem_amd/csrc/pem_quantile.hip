// pem_quantile.hip -- per-column order statistics over the SAMPLE axis of a row-major [n][m] array (gfx950): the percentiles
// behind the NaN / interquartile-range masks of scripts/gen_data.py:125-174 (`np.percentile(arr, 25 | 75, axis=0)`) and the
// 5 / 50 / 95 % bands of scripts/pem_v0/monte_carlo.py:363-658, at forward-UQ sizes: 1e7 samples x 91 angles is 7.3 GB, and
// a sort-based quantile (torch.quantile) refuses more than 2^24 values per column and sorts everything to pick two of them.
//
// Exact selection, not an estimate: the caller (drivers.column_percentiles) hands over the RANKS numpy's method 'linear' reads
// -- floor((n - 1) q) and the one above -- with its interpolation weight, this file returns x_(rank) for every column and
// applies numpy's _lerp, so the result equals np.percentile bit for bit (NaN in a column -> NaN, as there).
//
// Four streaming passes over the data, each coalesced (a lane owns fixed columns: consecutive lanes read consecutive
// addresses of a row, or of several short rows) and each bound by HBM:
//   1. min / max per column of the order-preserving integer image of the values (and whether a NaN is present);
//   2. a histogram per column over [min, max] (BINS1 bins, counted in LDS, merged with one atomic per bin and workgroup);
//      -> for every wanted rank: the bin that holds it and its rank inside the bin;
//   3. a second histogram per wanted rank inside its bin (BINS2 sub-bins);
//      -> the sub-bin and the rank inside it: by now 1 / (BINS1 BINS2) of a column's values are left per rank;
//   4. those values are copied out (exact sizes are known from pass 3; ranks that share a sub-bin share a list).
// Then one workgroup per list sorts it in LDS and reads the ranks off; a list too long for LDS -- heavy ties, e.g. the
// 1e-20 profile of invalid samples -- is narrowed by further histograms over the list itself until it fits or is one value.
// Monotone binning is all the method needs: a bin index that never decreases with the key, so that everything in a lower
// bin is <= everything in a higher one and equal keys share a bin.
// The keys, their binning, a lane's columns, the streaming loop and the selection from a list are in csrc/pem_quantile_core.h,
// the record passes of the fused form in csrc/pem_quantile_records.h; the selection over samples sharded over ranks has units of
// its own (csrc/pem_quantile_sharded.hip, and the level loop it falls back to: csrc/pem_quantile_range.hip).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <mutex>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_qfused.h"
#include "pem_quantile_core.h"

namespace {

__global__ void init_columns_kernel(Column* col, Target* tg, int m, int nq, Wanted w) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m) {
        col[c].kmin = ~0ull;
        col[c].kmax = 0ull;
        col[c].has_nan = 0;
        for (int q = 0; q < nq; ++q) {
            Target t = {};
            t.rank = w.prev[q];
            tg[c * 2 * nq + 2 * q] = t;
            t.rank = w.next[q];
            tg[c * 2 * nq + 2 * q + 1] = t;
        }
    }
}

// ---- pass 1: min / max / NaN per column ------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(QBLOCK) void minmax_kernel(long long n, int m, size_t ld, size_t cs, const double* __restrict__ data, Column* __restrict__ col) {
    const Lanes L(m, threadIdx.x & 63, cs);
    u64 lo[NC], hi[NC];
    int nan[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        lo[j] = ~0ull;
        hi[j] = 0ull;
        nan[j] = 0;
    }
    stream_values<NC>(n, m, ld, data, L, [&](int j, int, double x) {
        if (x != x) nan[j] += 1;                   // (counted: the histogram's total is checked against n - NaNs, decide1_kernel)
        else {
            const u64 k = key_of(x);
            lo[j] = k < lo[j] ? k : lo[j];
            hi[j] = k > hi[j] ? k : hi[j];
        }
    });
    // workgroup first (LDS), then one global atomic per column and workgroup: with few columns every lane of the grid owns
    // the same ones, and 2.6e5 lanes queueing on one address cost 7 ms
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
            if (nan[j]) atomicAdd(&s_nan[c], nan[j]);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < m; c += QBLOCK) {
        if (s_lo[c] <= s_hi[c]) {
            atomicMin(&col[c].kmin, s_lo[c]);
            atomicMax(&col[c].kmax, s_hi[c]);
        }
        if (s_nan[c]) atomicAdd(&col[c].has_nan, s_nan[c]);
    }
}

__global__ void scale_columns_kernel(Column* col, int m, int bins1) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m) {
        const Column k = col[c];
        const u64 span = k.kmax >= k.kmin ? k.kmax - k.kmin : 0;
        int shift = 0;
        while ((span >> shift) >> 31) ++shift;
        col[c].shift = shift;
        const u64 mult = (((u64)bins1) << 32) / ((span >> shift) + 1);        // >= 2^32 when there are fewer keys than bins:
        col[c].mult = mult > 0xffffffffull ? 0xffffffffu : (unsigned)mult;      // capped (two keys may then share a bin: still monotone)
    }
}

// ---- pass 2: histogram per column ------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(QBLOCK) void hist1_kernel(long long n, int m, size_t ld, size_t cs, const double* __restrict__ data, const Column* __restrict__ col,
                                                        int bins1, unsigned* __restrict__ hist1) {
    extern __shared__ unsigned lds_hist[];
    for (int i = threadIdx.x; i < m * bins1; i += QBLOCK) lds_hist[i] = 0;
    __syncthreads();
    const Lanes L(m, threadIdx.x & 63, cs);
    Scale sc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
        sc[j].lo = on ? col[c].kmin : 0;
        sc[j].mult = on ? col[c].mult : 0;
        sc[j].shift = on ? col[c].shift : 0;
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

// one wave per (column, target): the bin that holds the rank
// (and an invariant while the histogram is at hand -- ADVICE r3: an LDS atomic lost in the counting pass would shift a rank silently,
// both later passes agreeing on the wrong count: the column's bins must add up to its rows minus its NaNs, or the call fails)
__global__ __launch_bounds__(64) void decide1_kernel(int m, int nt, const Column* __restrict__ col, const unsigned* __restrict__ hist1, int bins1,
                                                      Target* __restrict__ tg, long long rows, int* __restrict__ inconsistent) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int c = i / nt;
    if (i == c * nt) {
        u64 sum = 0;
        for (int b = lane; b < bins1; b += 64) sum += hist1[(size_t)c * bins1 + b];
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) sum += __shfl_xor(sum, sh);
        if (lane == 0 && sum != (u64)(rows - col[c].has_nan)) atomicExch(inconsistent, 1 + c);
    }
    Target t = tg[i];
    t.owner = i - c * nt;
    if (col[c].kmin >= col[c].kmax) {          // a constant column (or one without a finite value: its result is NaN anyway)
        t.done = 1;
        t.answer = col[c].kmin;
        t.bin1 = -1;
    } else {
        const Found f = find_bin(hist1 + (size_t)c * bins1, bins1, t.rank, lane);
        t.bin1 = f.bin;
        t.rank -= f.before;
    }
    if (lane == 0) tg[i] = t;
}

// ---- pass 3: histogram of every target's bin -----------------------------------------------------------------------------
template <int NC, int NT>
__global__ __launch_bounds__(QBLOCK) void hist2_kernel(long long n, int m, size_t ld, size_t cs, const double* __restrict__ data, const Column* __restrict__ col,
                                                        const Target* __restrict__ tg, int bins1, int bins2,
                                                        unsigned* __restrict__ hist2) {
    extern __shared__ unsigned lds_hist[];
    for (int i = threadIdx.x; i < m * NT * bins2; i += QBLOCK) lds_hist[i] = 0;
    __syncthreads();
    const Lanes L(m, threadIdx.x & 63, cs);
    Scale sc[NC];
    int tb[NC][NT];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
        sc[j].lo = on ? col[c].kmin : 0;
        sc[j].mult = on ? col[c].mult : 0;
        sc[j].shift = on ? col[c].shift : 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            // targets of a column often share a bin: each DISTINCT bin is counted once, under the first target that has it
            int b = on ? tg[c * NT + t].bin1 : -1;
#pragma unroll
            for (int u = 0; u < t; ++u)
                if (tb[j][u] == b || (on && tg[c * NT + u].bin1 == b)) b = -1;
            tb[j][t] = b;
        }
    }
    stream_values<NC>(n, m, ld, data, L, [&](int j, int c, double x) {
        if (x == x) {
            const u64 k = key_of(x);
            unsigned frac;
            const int b = bin_of(k, sc[j], frac);
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

// one wave per (column, target): the sub-bin that holds the rank (the histogram sits under the column's first target with
// the same bin)
__global__ __launch_bounds__(64) void decide2_kernel(int nt, const unsigned* __restrict__ hist2, int bins2, Target* __restrict__ tg) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int c = i / nt, t = i - c * nt;
    Target T = tg[i];
    if (T.done) return;
    int first = t;
    for (int u = t - 1; u >= 0; --u)
        if (!tg[c * nt + u].done && tg[c * nt + u].bin1 == T.bin1) first = u;
    const Found f = find_bin(hist2 + (size_t)(c * nt + first) * bins2, bins2, T.rank, lane);
    T.bin2 = f.bin;
    T.rank -= f.before;
    T.count = f.count;
    if (lane == 0) tg[i] = T;
}

// ONE workgroup, one thread per column: which targets of a column share a list (same bin and sub-bin), and where the lists
// start in the candidate buffer (a scan over the columns in LDS)
__global__ __launch_bounds__(64 * MAX_NC) void layout_kernel(int m, int nt, Target* __restrict__ tg, u64* __restrict__ total) {
    __shared__ u64 start[64 * MAX_NC + 1];
    constexpr int NTMAX = 2 * PEM_QUANTILE_MAX_Q;
    const int c = threadIdx.x;
    // (the column's targets are read ONCE, side by side, into registers: walked through global memory -- a dependent load per
    // comparison, ~50 per column -- this one workgroup took 50 us of a campaign's critical path)
    int bin1[NTMAX], bin2[NTMAX], owner[NTMAX];
    bool done[NTMAX];
    u64 count[NTMAX];
    u64 mine = 0;
    if (c < m) {
#pragma unroll
        for (int t = 0; t < NTMAX; ++t) {
            const Target& T = tg[c * nt + (t < nt ? t : 0)];
            done[t] = t >= nt || T.done != 0;
            bin1[t] = T.bin1;
            bin2[t] = T.bin2;
            count[t] = T.count;
            owner[t] = t;
        }
#pragma unroll
        for (int t = 0; t < NTMAX; ++t) {
            if (done[t]) continue;
            bool found = false;
#pragma unroll
            for (int u = 0; u < NTMAX; ++u) {
                if (u < t && !found && !done[u] && bin1[u] == bin1[t] && bin2[u] == bin2[t]) {
                    owner[t] = owner[u];
                    found = true;
                }
            }
            if (owner[t] == t) mine += count[t];
        }
    }
    start[c + 1] = mine;
    if (c == 0) start[0] = 0;
    __syncthreads();
    if (c == 0) {
        for (int k = 1; k <= 64 * MAX_NC; ++k) start[k] += start[k - 1];          // 256 additions in LDS
        total[0] = start[m];
    }
    __syncthreads();
    if (c < m) {
        u64 off = start[c];
        u64 offs[NTMAX];
#pragma unroll
        for (int t = 0; t < NTMAX; ++t) {
            offs[t] = 0;
            if (done[t]) continue;
            if (owner[t] == t) {
                offs[t] = off;
                off += count[t];
            } else {
#pragma unroll
                for (int u = 0; u < NTMAX; ++u)
                    if (u < t && u == owner[t]) offs[t] = offs[u];
            }
            tg[c * nt + t].owner = owner[t];
            tg[c * nt + t].offset = offs[t];
        }
    }
}

// ---- pass 4: copy the candidates out ----------------------------------------------------------------------------------------
template <int NC, int NT>
__global__ __launch_bounds__(QBLOCK) void compact_kernel(long long n, int m, size_t ld, size_t cs, const double* __restrict__ data, const Column* __restrict__ col,
                                                          Target* __restrict__ tg, int bins1, int bins2, u64* __restrict__ cand) {
    const Lanes L(m, threadIdx.x & 63, cs);
    Scale sc[NC];
    int tb1[NC][NT], tb2[NC][NT];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
        sc[j].lo = on ? col[c].kmin : 0;
        sc[j].mult = on ? col[c].mult : 0;
        sc[j].shift = on ? col[c].shift : 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool own = on && !tg[c * NT + t].done && tg[c * NT + t].owner == t;       // only list owners collect
            tb1[j][t] = own ? tg[c * NT + t].bin1 : -1;
            tb2[j][t] = own ? tg[c * NT + t].bin2 : -1;
        }
    }
    stream_values<NC>(n, m, ld, data, L, [&](int j, int c, double x) {
        if (x == x) {
            const u64 k = key_of(x);
            unsigned frac;
            const int b = bin_of(k, sc[j], frac);
            const int sb = subbin_of(frac, bins2);
            int hit = -1;                                   // list owners have distinct (bin, sub-bin) pairs: at most one matches
#pragma unroll
            for (int t = 0; t < NT; ++t) hit = (tb1[j][t] == b && tb2[j][t] == sb) ? t : hit;
            if (hit >= 0) {
                Target& T = tg[c * NT + hit];
                cand[T.offset + atomicAdd(&T.cursor, 1ull)] = k;
            }
        }
    });
}

// (`incomplete`: a list whose copy pass delivered another number of values than the histogram counted -- the two passes bin
// the same way, so this says the code is wrong, not the data; the host refuses the result.  It has happened: a version of
// compact_bracket_kernel that parked its hits in LDS lost one value in a few thousand -- percentiles one rank off, in some runs;
// the cause was not found (the parking pattern alone does not lose anything: tools/microbench/lds_slot_alloc.hip) and the
// parking, no faster than appending on the spot, was dropped.)
__global__ __launch_bounds__(QBLOCK) void select_kernel(int nt, Target* __restrict__ tg, const u64* __restrict__ cand, int* __restrict__ incomplete) {
    Target& T = tg[blockIdx.x];
    if (T.done) return;
    if (threadIdx.x == 0 && T.owner == (int)(blockIdx.x % nt) && T.cursor != T.count && atomicExch(incomplete, 1) == 0) {
        u64* note = reinterpret_cast<u64*>(incomplete) + 1;               // which list, for the error message
        note[0] = blockIdx.x;
        note[1] = T.cursor;
        note[2] = T.count;
    }
    const u64* list = cand + T.offset;
    const u64 answer = select_from([list](u64 i) { return list[i]; }, T.count, T.rank, ~0ull, incomplete);
    if (threadIdx.x == 0) {
        T.answer = answer;
        T.done = 1;
    }
}

// out[q][c] = numpy's _lerp(x_(prev), x_(next), gamma); NaN where the column holds one
__global__ void finish_kernel(int m, int nq, const Column* __restrict__ col, const Target* __restrict__ tg, Wanted w,
                              double* __restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nq) return;
    const int q = i / m, c = i - q * m;
    const double a = value_of(tg[c * 2 * nq + 2 * q].answer), b = value_of(tg[c * 2 * nq + 2 * q + 1].answer), t = w.gamma[q];
    const double diff = b - a;
    double r = a + diff * t;
    if (t >= 0.5) r = b - diff * (1.0 - t);
    if (col[c].has_nan || col[c].kmin > col[c].kmax) r = __builtin_nan("");
    out[(size_t)q * m + c] = r;
}

// ---- the pilot form (round 3): two passes over the data instead of four ------------------------------------------------------
// The selection above spends its first two passes finding, per wanted rank, a key interval that holds 1/BINS1 of the column.
// A strided subsample -- every PILOT-th row, 3 % of the data -- gives such an interval for the price of the four passes over
// the subsample alone: the order statistics of the subsample a few standard deviations either side of the wanted quantile
// bracket it ("the bracket" [lo, hi] per column and quantile; both ranks numpy reads for a quantile lie in one bracket).
// Then ONE pass counts, per bracket, the values below it and a histogram inside it (a value outside every bracket costs two
// compares per bracket and no LDS atomic -- pass 2 above pays one per value), the wanted ranks become (sub-bin, rank inside)
// exactly as in decide2_kernel, and ONE pass copies the few values of those sub-bins out; lists, sort and interpolation are the
// ones above.  Exactness does not rest on the subsample: the counts say whether a wanted rank really lies inside its bracket
// (below <= rank < below + inside), and if any does not -- data ordered so that the strided rows misrepresent it -- the call
// falls back to the four passes.  The subsample only decides how often that happens: with brackets 7 sigma wide, for
// exchangeable rows (Monte-Carlo, Latin hypercube and Saltelli designs), about once in 1e9 calls.
using pem::Bracket;     // per (column, quantile): the keys lo .. hi, binned on their HIGH WORDS (round 4; csrc/pem_qfused.h)
// Binning inside a bracket (round 4).  The counting pass met a value of SOME bracket in nearly every wave instruction (64 lanes
// x nq brackets x 1.3 %), so whatever a value inside a bracket costs, every value paid: with the sub-bin taken from the 64-bit
// offset k - lo (subtract, shift, quarter-rate multiply, per bracket) three quantiles ran at 1.35 ms per 1e7 x 91 and five at
// 3.0 ms -- instruction issue, not memory.  The sub-bin is now a function of the key's high word alone: t = kh - loh,
// bin = floor(t mult / 2^32) -- never decreasing with the key, so still a valid binning -- which a lane gets from the
// subtraction that also tells it whether the value lies below the bracket (the borrow) or inside (t <= words).  Only a key whose
// high word EQUALS that of lo or hi (one value in 1e5) is compared in full.  A bracket narrower than `bins` high words -- a
// column with a relative spread below 1e-5 -- puts several sub-bins' worth of values into one list; select_from narrows such a
// list by histograms of its own, as it does for ties.
// The fused form's pilot does not need the subsample's order statistics themselves: any key at or below x_(r_lo) will do as a
// bracket's lower end, any key at or above x_(r_hi) as its upper end (the counts of the full run prove the bracket, whatever it
// is).  So its run stops after the second histogram: a lower end becomes the FIRST key of the sub-bin that holds its rank, an
// upper end the LAST key of its sub-bin -- no candidate lists, no copy pass over the subsample, no sort (a sub-bin holds a few
// dozen of the subsample's ~4000 values between the ends).  Targets 2q / 2q + 1 are a bracket's lower / upper end.
__global__ __launch_bounds__(64) void pilot_edges_kernel(int total, int nt, int bins2, const Column* __restrict__ col, Target* __restrict__ tg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    Target T = tg[i];
    if (T.done) return;
    const Column C = col[i / nt];
    Scale sc;
    sc.lo = C.kmin;
    sc.mult = C.mult;
    sc.shift = C.shift;
    u64 klo, khi;
    keys_of_bin(sc, C.kmax, bins2, (long long)T.bin1 * bins2 + T.bin2, klo, khi);
    tg[i].answer = ((i % nt) & 1) ? khi : klo;
}

struct PilotEnds {       // a bracket end that would lie outside the subsample is open: the smallest / largest key
    int open_lo[PEM_QUANTILE_MAX_Q], open_hi[PEM_QUANTILE_MAX_Q];
};

// brackets from the order statistics of the subsample (targets 2q, 2q + 1 of the pilot run: the lower and the upper end).
// The ends are moved outwards to whole high words -- lo to the first key of its word, hi to the last key of its -- so that
// "below", "inside" and the sub-bin are all functions of a key's high word: any interval that holds the wanted ranks will do,
// and this one is at most two parts in a million wider.  The exception is a bracket whose ends are ONE key (the subsample's
// order statistics coincide: a constant column, or heavy ties such as the 1e-20 profile of invalid samples): it stays that key,
// is counted by comparing whole keys (mult = 0 marks it; `any_single` tells the counting pass to take its general loop) and
// answers its ranks without a list.
__global__ void brackets_kernel(int m, int nq, const Target* __restrict__ ptg, PilotEnds e, int bins, Bracket* __restrict__ br,
                                int* __restrict__ any_single) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nq) return;
    const int c = i / nq, q = i - c * nq;
    u64 lo = e.open_lo[q] ? 0ull : ptg[c * 2 * nq + 2 * q].answer;
    u64 hi = e.open_hi[q] ? ~0ull : ptg[c * 2 * nq + 2 * q + 1].answer;
    if (hi < lo) hi = lo;                  // (a subsample column without a finite value: the column's result is NaN anyway)
    Bracket b;
    const bool single = lo == hi;
    if (!single) {
        lo &= 0xffffffff00000000ull;
        hi |= 0x00000000ffffffffull;
    }
    b.lo = lo;
    b.hi = hi;
    b.loh = (unsigned)(lo >> 32);
    b.words = (unsigned)(hi >> 32) - b.loh;
    const u64 mult = (((u64)bins) << 32) / ((u64)b.words + 1);
    b.mult = single ? 0u : (mult > 0xffffffffull ? 0xffffffffu : (unsigned)mult);
    b.pad = 0;
    br[i] = b;
    if (single) atomicExch(any_single, 1);
}

// the smallest t in [0, words + 1] whose bin is >= b (words + 1: none) -- the binning is monotone, so this is where sub-bin b begins
__device__ __forceinline__ u64 first_t_of_bin(unsigned mult, int b, unsigned words) {
    u64 lo = 0, hi = (u64)words + 1;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if ((int)((mid * mult) >> 32) >= b) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// pass A: per (column, quantile) the number of values below the bracket and a histogram of those inside it; NaN per column
// Up to 128 columns and three quantiles two workgroups share a CU (16 waves): the bracket histogram gets half the LDS (LDS_WORDS_A)
// and the registers have to fit twice; four columns per lane, or more quantiles, take a CU each.
constexpr int LDS_WORDS_A = 20224;        // 79 KB of 32-bit counters per workgroup
template <int NC, int NQ>
constexpr int bracket_waves_per_simd() { return NC <= 2 ? 4 : 2; }
template <int NC, int NQ>
__global__ __launch_bounds__(QBLOCK) __attribute__((amdgpu_waves_per_eu(bracket_waves_per_simd<NC, NQ>()))) void bracket_hist_kernel(long long n, int m, size_t ld, size_t cs, const double* __restrict__ data,
                                                               const Bracket* __restrict__ br, const int* __restrict__ any_single, int bins,
                                                               Column* __restrict__ col, u64* __restrict__ below, unsigned* __restrict__ hist) {
    extern __shared__ unsigned lds_hist[];                      // [m][NQ][bins] | below [m][NQ]
    unsigned* lds_below = lds_hist + m * NQ * bins;
    for (int i = threadIdx.x; i < m * NQ * (bins + 1); i += QBLOCK) lds_hist[i] = 0;
    __syncthreads();
    const Lanes L(m, threadIdx.x & 63, cs);
    unsigned bloh[NC][NQ], bwords[NC][NQ], bmult[NC][NQ], nbelow[NC][NQ];
    int nan[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
        nan[j] = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            bloh[j][q] = on ? br[c * NQ + q].loh : 0;
            bwords[j][q] = on ? br[c * NQ + q].words : 0;
            bmult[j][q] = on ? br[c * NQ + q].mult : 0;
            nbelow[j][q] = 0;
        }
    }
    // Per value and bracket: one subtraction of high words -- its borrow says "below", its result t <= words says "inside" and is
    // the sub-bin's argument; nothing else.  A NaN is flagged and otherwise counted as whatever its bits say: the column's result
    // is NaN whatever the counts are.  The general loop (taken by every wave when some bracket is a single key) compares whole
    // keys for those brackets.
    // (four brackets or more per column: four row groups in flight per wave instead of eight -- the brackets' registers and sixteen
    // values did not fit the 128 registers of four waves per SIMD: 9-41 spilled)
    constexpr int U = NC >= 4 ? 4 : ((NC >= 2 && NQ >= 6) ? 2 : ((NC >= 2 && NQ >= 4) ? 4 : UNROLL));
    if (*any_single == 0) {
        stream_values<NC, U>(n, m, ld, data, L, [&](int j, int c, double x) {
            const bool num = x == x;
            nan[j] |= num ? 0 : 1;
            const unsigned kh = key_high(x);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                unsigned t;
                nbelow[j][q] += __builtin_sub_overflow(kh, bloh[j][q], &t) ? 1u : 0u;
                // (a borrow leaves t above every `words`: 2^32 - loh + kh > hih - loh)
                if (t <= bwords[j][q] && num) atomicAdd(&lds_hist[(c * NQ + q) * bins + (int)__umulhi(t, bmult[j][q])], 1u);
            }
        });
    } else {
        stream_values<NC, U>(n, m, ld, data, L, [&](int j, int c, double x) {
            const bool num = x == x;
            nan[j] |= num ? 0 : 1;
            const unsigned kh = key_high(x);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                unsigned t;
                nbelow[j][q] += __builtin_sub_overflow(kh, bloh[j][q], &t) ? 1u : 0u;
                if (t <= bwords[j][q] && num) {
                    if (bmult[j][q] != 0) {
                        atomicAdd(&lds_hist[(c * NQ + q) * bins + (int)__umulhi(t, bmult[j][q])], 1u);
                    } else {                                    // a bracket of one key: its word holds keys below, equal and above
                        const u64 k = key_of(x), only = br[c * NQ + q].lo;
                        if (k < only) nbelow[j][q] += 1u;
                        else if (k == only) atomicAdd(&lds_hist[(c * NQ + q) * bins], 1u);
                    }
                }
            }
        });
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        if (L.active && c < m) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (nbelow[j][q]) atomicAdd(&lds_below[c * NQ + q], nbelow[j][q]);
            if (nan[j]) atomicOr(&col[c].has_nan, 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < m * NQ * bins; i += QBLOCK) {
        const unsigned v = lds_hist[i];
        if (v) atomicAdd(&hist[i], v);
    }
    for (int i = threadIdx.x; i < m * NQ; i += QBLOCK) {
        const unsigned v = lds_below[i];
        if (v) atomicAdd(&below[i], (u64)v);
    }
}

// one wave per (column, target): is the rank inside its bracket, and if so in which sub-bin (decide2_kernel's role; bin1 = the
// quantile, so that layout_kernel's "same bin and sub-bin" is "same bracket and sub-bin")
__global__ __launch_bounds__(64) void decide_bracket_kernel(int nt, Column* __restrict__ col, const Bracket* __restrict__ br,
                                                             const u64* __restrict__ below, const unsigned* __restrict__ hist, int bins,
                                                             Target* __restrict__ tg, int* __restrict__ outside) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int c = i / nt, t = i - c * nt, q = t >> 1, nq = nt >> 1;
    Target T = tg[i];
    if (t == 0 && lane == 0) {             // finish_kernel reads kmin > kmax as "no finite value": every such column holds a NaN here
        col[c].kmin = 0ull;
        col[c].kmax = ~0ull;
    }
    T.owner = t;
    if (col[c].has_nan) {                   // the column's result is NaN whatever the ranks are
        T.done = 1;
        T.answer = 0;
    } else {
        const Bracket b = br[c * nq + q];
        const u64 lowc = below[c * nq + q];
        const u64 r = T.rank - lowc;
        const Found f = find_bin(hist + (size_t)(c * nq + q) * bins, bins, r, lane);
        if (T.rank < lowc || f.before + f.count <= r) {      // not in the bracket: the call falls back to the four passes
            T.done = 1;
            T.answer = 0;
            if (lane == 0) atomicExch(outside, 1);
        } else if (b.lo == b.hi) {         // a bracket of one key (a constant column): the answer is that key
            T.done = 1;
            T.answer = b.lo;
        } else {
            T.bin1 = q;
            T.bin2 = f.bin;
            T.rank = r - f.before;
            T.count = f.count;
        }
    }
    if (lane == 0) tg[i] = T;
}

// pass B: copy out the values of the chosen sub-bins.  (Parking the hits in LDS and appending them after the last row, so that no
// wave waits for a global atomic in mid-stream, measured the same 1.67 ms as appending on the spot: not kept.)
template <int NC, int NQ>
__global__ __launch_bounds__(QBLOCK) void compact_bracket_kernel(long long n, int m, size_t ld, size_t cs, const double* __restrict__ data,
                                                                  const Bracket* __restrict__ br, Target* __restrict__ tg,
                                                                  u64* __restrict__ cand) {
    constexpr int NT = 2 * NQ;
    const Lanes L(m, threadIdx.x & 63, cs);
    // per (column, quantile): the range of high words (as offsets t from the bracket's first) of the sub-bins its list owners
    // collect (two adjacent ranks: one sub-bin, or two neighbours), found from the binning itself; a value is tested against it
    // with one subtraction and one comparison
    unsigned rloh[NC][NQ], rwords[NC][NQ];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = L.col0 + 64 * j;
        const bool on = L.active && c < m;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            u64 lo = ~0ull, hi = 0ull;                          // as high words (64-bit so that "none" fits)
#pragma unroll
            for (int t = 2 * q; t < 2 * q + 2; ++t) {
                const bool own = on && !tg[c * NT + t].done && tg[c * NT + t].owner == t;   // only list owners collect
                if (own) {
                    const Bracket B = br[c * NQ + q];
                    const int b2 = tg[c * NT + t].bin2;
                    const u64 t0 = first_t_of_bin(B.mult, b2, B.words), t1 = first_t_of_bin(B.mult, b2 + 1, B.words);
                    const u64 h0 = (u64)B.loh + t0, h1 = (u64)B.loh + (t1 > (u64)B.words ? (u64)B.words : t1 - 1);
                    lo = h0 < lo ? h0 : lo;
                    hi = h1 > hi ? h1 : hi;
                }
            }
            if (lo > hi) {                                      // no owner: a range no high word lies in
                rloh[j][q] = 0xffffffffu;
                rwords[j][q] = 0u;
            } else {
                rloh[j][q] = (unsigned)lo;
                rwords[j][q] = (unsigned)(hi - lo);
            }
        }
    }
    stream_values<NC>(n, m, ld, data, L, [&](int j, int c, double x) {
        const unsigned kh = key_high(x);
        bool near = false;
#pragma unroll
        for (int q = 0; q < NQ; ++q) near |= kh - rloh[j][q] <= rwords[j][q];
        if (near && x == x) {                                   // (about one wave instruction in ten)
            const u64 k = key_of(x);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (kh - rloh[j][q] <= rwords[j][q]) {
                    const Bracket B = br[c * NQ + q];
                    {                                           // (list owners' brackets end on whole words: the high word has decided)
                        const int b = (int)__umulhi(kh - B.loh, B.mult);
                        // (the two targets of a quantile share a list when they share the sub-bin: at most one of them owns it)
                        const Target& T0 = tg[c * NT + 2 * q];
                        const Target& T1 = tg[c * NT + 2 * q + 1];
                        const int hit = (!T0.done && T0.owner == 2 * q && T0.bin2 == b) ? 2 * q
                                        : ((!T1.done && T1.owner == 2 * q + 1 && T1.bin2 == b) ? 2 * q + 1 : -1);
                        if (hit >= 0) {
                            Target& T = tg[c * NT + hit];
                            cand[T.offset + atomicAdd(&T.cursor, 1ull)] = k;
                        }
                    }
                }
            }
        }
    });
}

// ---- the fused form (round 4): counts and records come from the kernel that PRODUCES the array (csrc/pem_qfused.h) ------------
// pass A's below-counts are already there; its histogram inside the brackets, and pass B's copy, run over the records -- the few
// per cent of the values that lie inside a bracket -- instead of over the array.

// a producer's counting launch assumes brackets that end on whole words (not a single key) and do not overlap within a column
__global__ void bracket_check_kernel(int m, int nq, const Bracket* __restrict__ br, int* __restrict__ unfit) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nq) return;
    const int c = i / nq, q = i - c * nq;
    const Bracket b = br[i];
    bool bad = b.mult == 0;
    for (int u = 0; u < nq; ++u) {
        if (u == q) continue;
        const Bracket o = br[c * nq + u];
        if ((u64)b.loh <= (u64)o.loh + o.words && (u64)o.loh <= (u64)b.loh + b.words) bad = true;
    }
    if (bad) atomicExch(unfit, 1);
}

// The premask's thresholds (csrc/pem_kernels.hip count_round): p25 and p75 lie in their brackets [A, B] and [C, D], so numpy's
// lo = p25 - f (p75 - p25) and hi = p75 + f (p75 - p25) (gen_data.py:163-168; every operation rounded on its own, every one of
// them monotone in p25 and p75 for f >= 0) lie in [lo_min, lo_max] and [hi_min, hi_max].  Per column the high words of the
// four ends' keys; `bad` when an end is zero (the key order splits -0 from +0, numpy's comparison does not), not finite, or f < 0.
__global__ void premask_bounds_kernel(int m, int nq, const Bracket* __restrict__ br, int q25, int q75, double f, uint4* __restrict__ thr,
                                      int* __restrict__ bad) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m) return;
    const double A = value_of(br[c * nq + q25].lo), B = value_of(br[c * nq + q25].hi);
    const double C = value_of(br[c * nq + q75].lo), D = value_of(br[c * nq + q75].hi);
    const double iqr_max = D - A, iqr_min = C - B;
    const double lo_min = A - f * iqr_max, lo_max = B - f * iqr_min, hi_min = C + f * iqr_min, hi_max = D + f * iqr_max;
    const double v[4] = {lo_min, lo_max, hi_min, hi_max};
    bool ok = f >= 0.0;
    for (int i = 0; i < 4; ++i) ok = ok && __builtin_isfinite(v[i]) && v[i] != 0.0;
    if (!ok) atomicExch(bad, 1);
    thr[c] = make_uint4(key_high(lo_min), key_high(lo_max), key_high(hi_min), key_high(hi_max));
}

}  // namespace

#include "pem_quantile_records.h"

// which way the last call of pem_quantiles_f64_dev went: 0 four passes, 1 pilot + two passes, 2 pilot, then four passes (a
// wanted rank outside its bracket)
static std::atomic<int> g_last_path{0};
extern "C" int pem_quantiles_last_path(void) { return g_last_path.load(); }

// ---- the host's side: one call is validate -> plan -> workspace -> (pilot brackets -> counting pass -> copy pass | four passes) -> finish
namespace {

// A device buffer kept between calls.  It only grows: a hipFree + hipMalloc in the middle of a call costs a device synchronisation
// and a millisecond.
template <class T>
struct DeviceBuffer {
    T* ptr = nullptr;
    size_t cap = 0;                            // elements
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
    hipError_t reserve(size_t need, size_t room) {      // at least `need` elements; `room` of them when it has to grow
        if (cap >= need) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&ptr, room * sizeof(T));
        if (e == hipSuccess) cap = room;
        return e;
    }
};

// The buffers a selection keeps between calls (grow-only).  Two sets: calls are serialised on a set, and the second one lets the
// scalar QoIs of a campaign be selected on another host thread and stream while the fused form is busy with the profile's records.
struct QWork {
    std::mutex mu;
    int dev = -1;                              // the device the buffers live on: all of them are freed when it changes
    DeviceBuffer<char> ws;                     // the workspace (Selection::lay_out)
    DeviceBuffer<u64> cand;                    // the candidate lists
    DeviceBuffer<pem::Record> rec;             // fused form: the producer's records
    DeviceBuffer<unsigned> part;               // fused form: the record histograms of every workgroup | their offsets into the lists
};
QWork g_qwork[2];

// The words the kernels report through: 256 bytes of the workspace behind hist2, zeroed with the histograms (four passes) or on
// their own (pilot form).  The kernels get the addresses of single members; the host reads the groups back whole.
struct Flags {
    struct Counted {
        u64 candidates;                        // layout_kernel: the length of all candidate lists
        int outside, pad;                      // decide_bracket_kernel: a wanted rank lies outside its bracket
    } counted;
    u64 incomplete[4];                         // select_kernel: [0] (as int) a list shorter or longer than counted, or sorted with fewer keys;
                                               // then which list, the values it was given, the values counted
    u64 unused[2];
    int any_single, pad;                       // brackets_kernel: a bracket of one key exists
    struct Fused {                             // fused form
        int unfit;                             // bracket_check_kernel: brackets a producer cannot count against
        int prod_flags[2];                     // the producer's: a wave's record region overflowed | a non-finite sample
        int pm_bad;                            // premask_bounds_kernel: the premask's bounds are unfit
    } fused;
    int inconsistent;                          // a histogram's total is not the number of values counted: 1 + column (decide1_kernel),
                                               // -1 the record histogram (record_total_check_kernel)
    int pad2[9];
    u64 rec_sums[2];                           // record_reduce_kernel: the record histogram's total | the producer's record count
};
static_assert(offsetof(Flags, incomplete) == 16 && offsetof(Flags, any_single) == 64 && offsetof(Flags, fused) == 72 &&
                  offsetof(Flags, inconsistent) == 88 && offsetof(Flags, rec_sums) == 128 && sizeof(Flags) <= 256,
              "the kernels' flag words keep their places in the workspace");

// One call.  `fused` (with `fused_ok`): the array does not exist (yet) -- `data` are its first ceil(n / pilot) rows, written by the
// producer, and pass A / pass B are the producer's counting launch and two passes over its records (csrc/pem_qfused.h).
// *fused_ok = 0: the brackets were unfit for the producer, a rank fell outside its bracket, or the producer reported an overflow or
// a non-finite sample -- `out` is then not written and the caller takes the passes over the array itself.
struct Selection {
    // the data and what is wanted of it
    size_t n;
    int m;
    const double* data;
    size_t ld, cs;
    int nq;
    double* out;
    hipStream_t st;
    pem::FusedProducer* fused;
    int* fused_ok;
    int slot;
    const pem::SidePlan* plan;
    Wanted w{};
    int nt = 0, nc = 0;                        // targets per column, columns per lane
    // the plan
    int bins1 = 0, bins2 = 0, binsA = 0;       // bins of the two histograms; of the pilot form's histogram inside a bracket
    long long pilot = 0;                       // the subsample's stride
    bool use_pilot = false;
    unsigned fused_waves = 0;                  // waves of the producer's counting launch
    // the workspace: columns | targets | hist1 | hist2 | flags | brackets | below | histA | record counts | premask bounds
    QWork* work = nullptr;
    Column* col = nullptr;
    Target* tg = nullptr;
    unsigned *hist1 = nullptr, *hist2 = nullptr;
    Flags* flags = nullptr;
    Bracket* br = nullptr;
    u64* below = nullptr;
    unsigned* histA = nullptr;
    unsigned* rec_count = nullptr;
    uint4* pm_thr = nullptr;
    size_t hists_and_flags = 0, counts = 0;    // bytes from hist1 to the end of the flags, and from `below` to the end
    int path = 0;                              // pem_quantiles_last_path

    // every error return waits for the stream: the workspace belongs to the next call as soon as this one gives up the lock
    int cleanup(int code) const {
        (void)hipStreamSynchronize(st);
        return code;
    }
    size_t lay_out(char* ws);
};

// HIP_TRY for the steps of a Selection `q` (after the workspace is in use: with cleanup)
#define Q_TRY(expr)                                                                                            \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return q.cleanup(pem::fail(PEM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_))); \
    } while (0)

int validate(Selection& q, const uint64_t* rank_prev, const uint64_t* rank_next, const double* gamma) {
    const size_t n = q.n, ld = q.ld, cs = q.cs;
    const int m = q.m, nq = q.nq;
    if (m < 1 || m > 64 * MAX_NC) return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: 1 <= m <= %d columns", 64 * MAX_NC);
    if (q.fused && (m > 128 || !q.fused_ok)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: the fused form takes up to 128 columns");
    if (cs < 1 || (cs == 1 ? ld < (size_t)m : (ld != 1 || cs < n)))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: rows of m columns (column stride 1, ld >= m) or columns of n rows (ld 1, column stride >= n)");
    if (nq < 1 || nq > (m <= 128 ? PEM_QUANTILE_MAX_Q : PEM_QUANTILE_MAX_Q_WIDE))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: 1 <= nq <= %d per call (%d for more than 128 columns)", PEM_QUANTILE_MAX_Q, PEM_QUANTILE_MAX_Q_WIDE);
    if (n == 0) return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: no samples");
    if (!q.data || !rank_prev || !rank_next || !gamma || !q.out) return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: NULL array");
    for (int i = 0; i < nq; ++i) {
        if (rank_prev[i] >= n || rank_next[i] >= n || rank_prev[i] > rank_next[i])
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: ranks must satisfy prev <= next < n");
        q.w.prev[i] = rank_prev[i];
        q.w.next[i] = rank_next[i];
        q.w.gamma[i] = gamma[i];
    }
    q.nt = 2 * nq;
    q.nc = columns_per_lane(m);
    return pem::check_device();
}

// bins, the pilot choice and the environment's overrides (read on every call)
int plan_selection(Selection& q) {
    const int m = q.m, nq = q.nq;
    const long long n = (long long)q.n;
    q.bins1 = pow2_at_most(LDS_WORDS / m, 4096);
    q.bins2 = pow2_at_most(LDS_WORDS / (m * q.nt), 4096);
    // (four quantiles or more: the brackets' registers leave room for one workgroup per CU anyway -- it gets all of the LDS)
    q.binsA = pow2_at_most((m <= 128 ? LDS_WORDS_A : LDS_WORDS) / (m * nq) - 1, 4096);   // the pilot form's histogram inside a bracket (+ 1 counter)
    if (q.fused) q.binsA = pow2_at_most(LDS_WORDS / (m * nq), 4096);        // (the record passes: one workgroup per CU with all of its LDS)
    if (const char* e = getenv("PEM_QUANTILE_BINSA")) q.binsA = pow2_at_most(atoll(e) < q.binsA ? atoll(e) : q.binsA, 4096);

    // the pilot form: every `pilot`-th row brackets the wanted ranks (PEM_QUANTILE_PILOT: the stride, 0 = never;
    // PEM_QUANTILE_PILOT_MIN: the smallest n * m it is used for -- 1e7 x 1 takes 0.24 ms with the four passes and 0.32 with the
    // pilot's dozen launches in front of two, 1e7 x 3 the same either way, 6e5 x 91 0.60 against 0.56: profiles/quantile_pilot_r03.txt)
    long long pilot = 32, pilot_min = 1 << 25;
    if (const char* e = getenv("PEM_QUANTILE_PILOT")) pilot = atoll(e);
    if (const char* e = getenv("PEM_QUANTILE_PILOT_MIN")) pilot_min = atoll(e);
    if (q.fused) {                                                          // (the producer writes rows 0 .. ceil(n / 32) - 1 at most)
        pilot = 32;
        if (const char* e = getenv("PEM_FUSED_PILOT")) pilot = atoll(e) >= 32 ? atoll(e) : 32;
    }
    if (q.plan) pilot = 32;                                                 // (the rows the plan's caller has written: 0 .. ceil(n / 32) - 1)
    q.pilot = pilot;
    q.use_pilot = q.fused ? true : q.plan ? n >= 4 * pilot : (pilot >= 2 && n * m >= pilot_min && n >= 4 * pilot);
    if (q.fused && n < 4 * pilot) return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: the fused form needs at least %lld rows", 4 * pilot);
    if (q.fused) return q.fused->waves(nq, &q.fused_waves);
    return PEM_OK;
}

// the workspace's parts at `ws` (nullptr: only their total size is wanted)
size_t Selection::lay_out(char* ws) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_tg = up(sizeof(Column) * m), o_h1 = o_tg + up(sizeof(Target) * m * nt);
    const size_t o_h2 = o_h1 + up(sizeof(unsigned) * (size_t)m * bins1), o_fl = o_h2 + up(sizeof(unsigned) * (size_t)m * nt * bins2);
    const size_t o_br = o_fl + 256, o_bl = o_br + up(sizeof(Bracket) * m * nq), o_hA = o_bl + up(sizeof(u64) * m * nq);
    const size_t o_rc = o_hA + up(sizeof(unsigned) * (size_t)m * nq * binsA), o_pm = o_rc + up(sizeof(unsigned) * fused_waves);
    const size_t o_end = o_pm + up(sizeof(uint4) * (size_t)m);
    auto at = [ws](size_t o) { return ws ? ws + o : nullptr; };
    col = reinterpret_cast<Column*>(at(0));
    tg = reinterpret_cast<Target*>(at(o_tg));
    hist1 = reinterpret_cast<unsigned*>(at(o_h1));
    hist2 = reinterpret_cast<unsigned*>(at(o_h2));
    flags = reinterpret_cast<Flags*>(at(o_fl));
    br = reinterpret_cast<Bracket*>(at(o_br));
    below = reinterpret_cast<u64*>(at(o_bl));
    histA = reinterpret_cast<unsigned*>(at(o_hA));
    rec_count = reinterpret_cast<unsigned*>(at(o_rc));
    pm_thr = reinterpret_cast<uint4*>(at(o_pm));
    hists_and_flags = o_br - o_h1;
    counts = o_end - o_bl;
    return o_end;
}

// the slot's buffers on the current device, the workspace large enough for this call (the caller holds the slot's lock: calls are
// serialised on it, and each one ends with a stream synchronisation before the next may touch the buffers)
int size_workspace(Selection& q) {
    QWork& work = g_qwork[q.slot];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != work.dev) {
        work.ws.release();
        work.cand.release();
        work.rec.release();
        work.part.release();
        work.dev = dev;
    }
    const size_t bytes = q.lay_out(nullptr);
    HIP_TRY(work.ws.reserve(bytes, bytes));
    q.lay_out(work.ws.ptr);
    q.work = &work;
    return PEM_OK;
}

hipError_t grow_candidates(Selection& q, u64 need) {
    // (a quarter more than asked for: the lists of two campaigns differ by a few values, and a hipFree + hipMalloc in the middle of
    // a call costs a device synchronisation and a millisecond)
    return q.work->cand.reserve((size_t)need + 1, (size_t)(need + need / 4 + 1024));
}

// the four passes over rows 0, step, 2 step, ... (`rows` of them, leading dimension ldd): x_(rank) of every target ends in tg[].answer
// (edges: stop after the second histogram and take the sub-bins' first / last keys as the answers -- pilot_edges_kernel)
int four_passes(Selection& q, size_t rows, size_t ldd, const Wanted& ww, bool edges = false) {
    const int m = q.m, nq = q.nq, nt = q.nt, bins1 = q.bins1, bins2 = q.bins2;
    hipStream_t st = q.st;
    const dim3 grid = stream_grid(rows, m), blk(QBLOCK), columns((m + 63) / 64), targets((unsigned)(m * nt));
    Q_TRY(hipMemsetAsync(q.hist1, 0, q.hists_and_flags, st));              // hist1, hist2, flags
    hipLaunchKernelGGL(init_columns_kernel, columns, dim3(64), 0, st, q.col, q.tg, m, nq, ww);
    with_value(q.nc, ColumnCounts{}, [&](auto NC) {
        hipLaunchKernelGGL(minmax_kernel<NC()>, grid, blk, 0, st, (long long)rows, m, ldd, q.cs, q.data, q.col);
    });
    hipLaunchKernelGGL(scale_columns_kernel, columns, dim3(64), 0, st, q.col, m, bins1);
    Q_TRY(with_value(q.nc, ColumnCounts{}, [&](auto NC) {
        return launch_lds<hist1_kernel<NC()>>(grid, blk, (size_t)m * bins1 * 4, st, (long long)rows, m, ldd, q.cs, q.data, q.col, bins1, q.hist1);
    }));
    hipLaunchKernelGGL(decide1_kernel, targets, dim3(64), 0, st, m, nt, q.col, q.hist1, bins1, q.tg, (long long)rows, &q.flags->inconsistent);
    Q_TRY(with_columns_and(q.nc, nt, TargetCounts{}, TargetCountsWide{}, [&](auto NC, auto NT) {
        return launch_lds<hist2_kernel<NC(), NT()>>(grid, blk, (size_t)m * nt * bins2 * 4, st, (long long)rows, m, ldd, q.cs, q.data, q.col, q.tg, bins1,
                                                     bins2, q.hist2);
    }));
    hipLaunchKernelGGL(decide2_kernel, targets, dim3(64), 0, st, nt, q.hist2, bins2, q.tg);
    if (edges) {
        hipLaunchKernelGGL(pilot_edges_kernel, dim3((unsigned)((m * nt + 63) / 64)), dim3(64), 0, st, m * nt, nt, bins2, q.col, q.tg);
        Q_TRY(hipGetLastError());
        return PEM_OK;
    }
    hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(64 * MAX_NC), 0, st, m, nt, q.tg, &q.flags->counted.candidates);
    Q_TRY(hipGetLastError());
    u64 h_total = 0;
    Q_TRY(hipMemcpyAsync(&h_total, &q.flags->counted.candidates, sizeof(u64), hipMemcpyDeviceToHost, st));
    Q_TRY(hipStreamSynchronize(st));
    Q_TRY(grow_candidates(q, h_total));
    u64* cand = q.work->cand.ptr;
    with_columns_and(q.nc, nt, TargetCounts{}, TargetCountsWide{}, [&](auto NC, auto NT) {
        hipLaunchKernelGGL((compact_kernel<NC(), NT()>), grid, blk, 0, st, (long long)rows, m, ldd, q.cs, q.data, q.col, q.tg, bins1, bins2, cand);
    });
    hipLaunchKernelGGL(select_kernel, targets, blk, 0, st, nt, q.tg, cand, reinterpret_cast<int*>(q.flags->incomplete));
    Q_TRY(hipGetLastError());
    return PEM_OK;
}

struct PilotRun {
    size_t rows = 0;                           // of the subsample
    Wanted pw{};                               // the subsample's ranks that bracket the wanted ones
    PilotEnds ends{};
    unsigned rcap = 0;                         // fused form: record room per wave
    bool pm_launched = false;                  // fused form: the counting launch carried the premask
    u64 candidates = 0;                        // what the counting pass found: the length of all lists ...
    bool outside = false;                      // ... a wanted rank outside its bracket: the four passes answer
    bool declined = false;                     // ... fused form: the run cannot be used (*fused_ok = 0)
};

// 1. the subsample's order statistics around every wanted quantile: 7 standard deviations of the subsample's rank, + 8 -- and the
// brackets made of them
int pilot_brackets(Selection& q, PilotRun& p) {
    const size_t n = q.n;
    const int m = q.m, nq = q.nq;
    hipStream_t st = q.st;
    p.rows = (n + (size_t)q.pilot - 1) / (size_t)q.pilot;
    const double n1 = n > 1 ? (double)(n - 1) : 1.0, np1 = (double)(p.rows - 1);
    for (int i = 0; i < nq; ++i) {
        const double p_lo = (double)q.w.prev[i] / n1, p_hi = (double)q.w.next[i] / n1;
        // (the fused form: 5 -- every value inside a bracket costs a record, in the counting launch and in both passes over the
        // records: 3.7-3.85 ms per 1e7-sample campaign with 6, 3.6 with 5, 3.5 with 4.5 on one box.  A rank outside its bracket
        // -- 2.9e-7 per bracket end, 910 ends: one campaign in four thousand -- is noticed by the counts and costs that call the
        // stored-profile route; PEM_FUSED_SIGMA moves it)
        double sig = q.fused ? 5.0 : 7.0;
        if (q.fused)
            if (const char* e = getenv("PEM_FUSED_SIGMA")) sig = atof(e) >= 3.0 ? atof(e) : 3.0;
        const double d_lo = sig * sqrt((double)p.rows * p_lo * (1.0 - p_lo)) + 8.0, d_hi = sig * sqrt((double)p.rows * p_hi * (1.0 - p_hi)) + 8.0;
        const double r_lo = floor(p_lo * np1 - d_lo) - 1.0, r_hi = ceil(p_hi * np1 + d_hi) + 1.0;
        p.ends.open_lo[i] = r_lo < 0.0;
        p.ends.open_hi[i] = r_hi > np1;
        p.pw.prev[i] = p.ends.open_lo[i] ? 0 : (u64)r_lo;
        p.pw.next[i] = p.ends.open_hi[i] ? (u64)(p.rows - 1) : (u64)r_hi;
    }
    if (q.fused) {                                                          // the producer writes the pilot rows (contiguous) first
        if (int rc = q.fused->pilot(p.rows, const_cast<double*>(q.data), st)) return q.cleanup(rc);
        const bool edges = !(getenv("PEM_FUSED_PILOT_EXACT") && atoi(getenv("PEM_FUSED_PILOT_EXACT")));
        PEM_TRY(four_passes(q, p.rows, q.ld, p.pw, edges));
    } else if (q.plan) {                                                    // the FIRST rows are the subsample; the rest is awaited
        PEM_TRY(four_passes(q, p.rows, q.ld, p.pw));
        if (q.plan->before_full)
            if (int rc = q.plan->before_full(q.plan->ctx, st)) return q.cleanup(rc);
    } else {
        PEM_TRY(four_passes(q, p.rows, q.ld * (size_t)q.pilot, p.pw));
    }
    Q_TRY(hipMemsetAsync(q.flags, 0, 256, st));                             // the flags
    Q_TRY(hipMemsetAsync(q.below, 0, q.counts, st));                        // below, histA (and the fused form's record counts)
    hipLaunchKernelGGL(brackets_kernel, dim3((unsigned)((m * nq + 63) / 64)), dim3(64), 0, st, m, nq, q.tg, p.ends, q.binsA, q.br, &q.flags->any_single);
    hipLaunchKernelGGL(init_columns_kernel, dim3((m + 63) / 64), dim3(64), 0, st, q.col, q.tg, m, nq, q.w);
    return PEM_OK;
}

// fused form, pass A: the producer counts below the brackets while it makes the array and writes the values inside them out as
// records; their histogram inside the brackets is taken over the records
int count_records(Selection& q, PilotRun& p) {
    const int m = q.m, nq = q.nq, nt = q.nt, binsA = q.binsA;
    hipStream_t st = q.st;
    pem::FusedProducer* fused = q.fused;
    // brackets the producer can count against?  (one small read: nothing else has to wait for the host here)
    hipLaunchKernelGGL(bracket_check_kernel, dim3((unsigned)((m * nq + 63) / 64)), dim3(64), 0, st, m, nq, q.br, &q.flags->fused.unfit);
    const bool want_pm = fused->pm_q25 >= 0 && fused->pm_q25 < nq && fused->pm_q75 >= 0 && fused->pm_q75 < nq && nq <= 5 && fused->pm_certain &&
                         fused->pm_uncertain;
    fused->pm_done = 0;
    if (want_pm)
        hipLaunchKernelGGL(premask_bounds_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, m, nq, q.br, fused->pm_q25, fused->pm_q75,
                           fused->pm_factor, q.pm_thr, &q.flags->fused.pm_bad);
    // (No host round trip here -- it cost every campaign 40 us of an idle GPU: whether the brackets are fit for the producer and
    // the premask's bounds usable is read back WITH the counts, after the counting launch.  Unfit brackets -- heavy ties,
    // overlapping percentiles -- are counted against all the same, harmlessly, and the run is then declined: the producer's
    // launch has written every output but the percentiles by then.)
    p.pm_launched = want_pm;
    // record room per wave: the brackets hold `expected` values of the array (their ranks in the subsample say so) -- half as
    // much again, and a few thousand for the waves that get more than their share
    double expected = 0.0;
    for (int i = 0; i < nq; ++i) expected += (double)(p.pw.next[i] - p.pw.prev[i] + 1) * (double)q.pilot * (double)m;
    p.rcap = (unsigned)(1.5 * expected / (double)q.fused_waves) + 4096u;
    if (const char* e = getenv("PEM_QUANTILE_RECORD_CAP")) p.rcap = (unsigned)atoll(e);      // (tests: force the overflow path)
    const size_t records = (size_t)q.fused_waves * p.rcap;
    Q_TRY(q.work->rec.reserve(records, records));
    pem::CountIO cio;
    cio.br = q.br;
    cio.nq = nq;
    cio.below = reinterpret_cast<unsigned long long*>(q.below);
    cio.rec = q.work->rec.ptr;
    cio.rec_count = q.rec_count;
    cio.cap = p.rcap;
    cio.flags = q.flags->fused.prod_flags;
    if (want_pm) {
        cio.premask = q.pm_thr;
        cio.row_certain = fused->pm_certain;
        cio.row_uncertain = fused->pm_uncertain;
    }
    if (int rc = fused->count(cio, st)) return q.cleanup(rc);
    int cus = 256;
    Q_TRY(pem::device_cus(&cus));
    const int cells = m * nq * binsA;
    const size_t parts = (size_t)cus * cells + (size_t)cus * m * nt;
    Q_TRY(q.work->part.reserve(parts, parts));
    unsigned* part = q.work->part.ptr;
    Q_TRY(with_value(nq, QuantileCounts{}, [&](auto NQ) {
        // (148 KB at most: + 12 KB of static tables)
        return launch_lds<record_hist_kernel<NQ()>, 148 * 1024>(dim3((unsigned)cus), dim3(RBLOCK), (size_t)m * nq * binsA * 4, st, q.work->rec.ptr,
                                                                 q.rec_count, p.rcap, q.fused_waves, q.br, m * nq, binsA, part);
    }));
    hipLaunchKernelGGL(record_reduce_kernel, dim3((unsigned)((cells + 63) / 64)), dim3(256), 0, st, part, cus, cells, q.histA, q.rec_count, p.rcap,
                       q.fused_waves, q.flags->rec_sums);
    hipLaunchKernelGGL(record_total_check_kernel, dim3(1), dim3(64), 0, st, q.flags->rec_sums, &q.flags->inconsistent, q.flags->fused.prod_flags);
    return PEM_OK;
}

// 2. pass A over everything: below / inside counts; the ranks inside their brackets become sub-bins
int counting_pass(Selection& q, PilotRun& p) {
    const int m = q.m, nq = q.nq, nt = q.nt, binsA = q.binsA;
    hipStream_t st = q.st;
    if (q.fused) {
        PEM_TRY(count_records(q, p));
    } else {
        Q_TRY(with_columns_and(q.nc, nq, QuantileCounts{}, QuantileCountsWide{}, [&](auto NC, auto NQ) {
            return launch_lds<bracket_hist_kernel<NC(), NQ()>>(stream_grid(q.n, m), dim3(QBLOCK), (size_t)m * nq * (binsA + 1) * 4, st, (long long)q.n, m,
                                                                q.ld, q.cs, q.data, q.br, &q.flags->any_single, binsA, q.col, q.below, q.histA);
        }));
    }
    hipLaunchKernelGGL(decide_bracket_kernel, dim3((unsigned)(m * nt)), dim3(64), 0, st, nt, q.col, q.br, q.below, q.histA, binsA, q.tg, &q.flags->counted.outside);
    hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(64 * MAX_NC), 0, st, m, nt, q.tg, &q.flags->counted.candidates);
    Q_TRY(hipGetLastError());
    Flags::Counted counted = {};
    Flags::Fused fused = {};
    Q_TRY(hipMemcpyAsync(&counted, &q.flags->counted, sizeof counted, hipMemcpyDeviceToHost, st));
    if (q.fused) Q_TRY(hipMemcpyAsync(&fused, &q.flags->fused, sizeof fused, hipMemcpyDeviceToHost, st));
    Q_TRY(hipStreamSynchronize(st));
    if (q.fused) q.fused->pm_done = (p.pm_launched && fused.pm_bad == 0) ? 1 : 0;
    // fused form: unfit brackets, a rank outside its bracket, record overflow, a non-finite sample
    p.declined = q.fused && (fused.unfit || counted.outside != 0 || fused.prod_flags[0] || fused.prod_flags[1]);
    p.outside = counted.outside != 0;
    p.candidates = counted.candidates;
    return PEM_OK;
}

// 3. pass B: the values of those sub-bins, then the lists as in the four-pass form
int copy_pass(Selection& q, PilotRun& p) {
    const int m = q.m, nq = q.nq, nt = q.nt;
    hipStream_t st = q.st;
    Q_TRY(grow_candidates(q, p.candidates));
    u64* cand = q.work->cand.ptr;
    if (!q.fused) {
        with_columns_and(q.nc, nq, QuantileCounts{}, QuantileCountsWide{}, [&](auto NC, auto NQ) {
            hipLaunchKernelGGL((compact_bracket_kernel<NC(), NQ()>), stream_grid(q.n, m), dim3(QBLOCK), 0, st, (long long)q.n, m, q.ld, q.cs, q.data, q.br,
                               q.tg, cand);
        });
    } else {
        int cus = 256;
        Q_TRY(pem::device_cus(&cus));
        unsigned* part = q.work->part.ptr;
        unsigned* woff = part + (size_t)cus * m * nq * q.binsA;
        hipLaunchKernelGGL(record_offsets_kernel, dim3((unsigned)(m * nt)), dim3(64), 0, st, nt, q.binsA, q.tg, part, cus, m * nq * q.binsA, woff);
        with_value(nq, QuantileCounts{}, [&](auto NQ) {
            hipLaunchKernelGGL(record_compact_kernel<NQ()>, dim3((unsigned)cus), dim3(RBLOCK), 0, st, q.work->rec.ptr, q.rec_count, p.rcap, q.fused_waves,
                               q.br, m * nq, q.tg, woff, cand);
        });
    }
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)(m * nt)), dim3(QBLOCK), 0, st, nt, q.tg, cand, reinterpret_cast<int*>(q.flags->incomplete));
    Q_TRY(hipGetLastError());
    return PEM_OK;
}

// the interpolation, and what the kernels reported about their own counts
int finish(Selection& q) {
    const int m = q.m, nq = q.nq, nt = q.nt, path = q.path;
    hipStream_t st = q.st;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((m * nq + 63) / 64)), dim3(64), 0, st, m, nq, q.col, q.tg, q.w, q.out);
    Q_TRY(hipGetLastError());
    u64 h_incomplete[4] = {0, 0, 0, 0};
    int h_inconsistent = 0;
    Q_TRY(hipMemcpyAsync(h_incomplete, q.flags->incomplete, sizeof h_incomplete, hipMemcpyDeviceToHost, st));
    Q_TRY(hipMemcpyAsync(&h_inconsistent, &q.flags->inconsistent, sizeof(int), hipMemcpyDeviceToHost, st));
    Q_TRY(hipStreamSynchronize(st));
    if (h_inconsistent > 0)
        return pem::fail(PEM_ERR_HIP, "pem_quantiles: the histogram of column %d does not add up to its number of values (internal error; result discarded; path %d)",
                         h_inconsistent - 1, path);
    if (h_inconsistent < 0)
        return pem::fail(PEM_ERR_HIP, "pem_quantiles: the record histogram does not add up to the number of records (internal error; result discarded)");
    if ((h_incomplete[0] & 0xffffffffull) && h_incomplete[2] == h_incomplete[3])
        return pem::fail(PEM_ERR_HIP, "pem_quantiles: a candidate list was sorted with fewer keys than it holds (internal error; result discarded; path %d)", path);
    if (h_incomplete[0] & 0xffffffffull)
        return pem::fail(PEM_ERR_HIP,
                         "pem_quantiles: the list of column %llu, rank %llu holds %llu values where %llu were counted (internal error; result "
                         "discarded; path %d)",
                         h_incomplete[1] / nt, h_incomplete[1] % nt, h_incomplete[2], h_incomplete[3], path);
    if (q.slot == 0) g_last_path.store(path);
    if (q.fused_ok) *q.fused_ok = 1;
    return q.cleanup(PEM_OK);
}

int quantiles_impl(size_t n, int m, const double* data, size_t ld, size_t cs, int nq, const uint64_t* rank_prev, const uint64_t* rank_next,
                   const double* gamma, double* out, pem_stream_t stream, pem::FusedProducer* fused, int* fused_ok, int slot = 0,
                   const pem::SidePlan* plan = nullptr) {
    Selection q{n, m, data, ld, cs, nq, out, static_cast<hipStream_t>(stream), fused, fused_ok, slot, plan};
    PEM_TRY(validate(q, rank_prev, rank_next, gamma));
    PEM_TRY(plan_selection(q));
    std::lock_guard<std::mutex> lock(g_qwork[slot].mu);
    PEM_TRY(size_workspace(q));
    bool answered = false;
    if (plan && !q.use_pilot && plan->before_full)                          // (too few rows for a subsample: everything is awaited)
        if (int rc = plan->before_full(plan->ctx, q.st)) return q.cleanup(rc);
    if (q.use_pilot) {
        PilotRun p;
        PEM_TRY(pilot_brackets(q, p));
        PEM_TRY(counting_pass(q, p));
        if (p.declined) {
            *fused_ok = 0;
            return q.cleanup(PEM_OK);
        }
        if (!p.outside) PEM_TRY(copy_pass(q, p));
        answered = !p.outside;
        q.path = answered ? 1 : 2;
    }
    if (!answered) PEM_TRY(four_passes(q, n, ld, q.w));
    return finish(q);
}

}  // namespace

extern "C" int pem_quantiles_strided_f64_dev(size_t n, int m, const double* data, size_t ld, size_t cs, int nq, const uint64_t* rank_prev,
                                             const uint64_t* rank_next, const double* gamma, double* out, pem_stream_t stream) {
    return quantiles_impl(n, m, data, ld, cs, nq, rank_prev, rank_next, gamma, out, stream, nullptr, nullptr);
}

int pem::quantiles_fused(size_t n, int m, int nq, const uint64_t* rank_prev, const uint64_t* rank_next, const double* gamma, double* pilot_rows,
                         pem::FusedProducer& prod, double* out, int* fused_ok, hipStream_t st) {
    return quantiles_impl(n, m, pilot_rows, (size_t)m, 1, nq, rank_prev, rank_next, gamma, out, static_cast<pem_stream_t>(st), &prod, fused_ok);
}

int pem::quantiles_side(size_t n, int m, const double* data, size_t ld, size_t cs, int nq, const uint64_t* rank_prev, const uint64_t* rank_next,
                        const double* gamma, double* out, hipStream_t st, const pem::SidePlan* plan) {
    return quantiles_impl(n, m, data, ld, cs, nq, rank_prev, rank_next, gamma, out, static_cast<pem_stream_t>(st), nullptr, nullptr, 1, plan);
}

extern "C" int pem_quantiles_f64_dev(size_t n, int m, const double* data, size_t ld, int nq, const uint64_t* rank_prev, const uint64_t* rank_next,
                                     const double* gamma, double* out, pem_stream_t stream) {
    if (ld < (size_t)(m > 0 ? m : 0)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_quantiles: leading dimension smaller than m");
    return pem_quantiles_strided_f64_dev(n, m, data, ld, 1, nq, rank_prev, rank_next, gamma, out, stream);
}
