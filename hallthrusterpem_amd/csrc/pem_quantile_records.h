// pem_quantile_records.h -- the record passes of the selection's fused form (csrc/pem_quantile.hip, which alone includes this;
// csrc/pem_qfused.h): the histogram inside the brackets and the copy of the chosen sub-bins run over the records the producing
// kernel wrote -- the few per cent of the values that lie inside a bracket -- instead of over the array.
#pragma once
#include "pem_qfused.h"
#include "pem_quantile_core.h"

namespace {

using pem::Bracket;

// the records the producer wrote are the values the record histogram counted (sums: record_reduce_kernel's)
__global__ void record_total_check_kernel(const u64* __restrict__ sums, int* __restrict__ inconsistent, const int* __restrict__ prod_flags) {
    // (a run the producer flagged -- overflow, a non-finite value -- is discarded anyway, and its records need not add up)
    if (threadIdx.x == 0 && sums[0] != sums[1] && !prod_flags[0] && !prod_flags[1]) atomicExch(inconsistent, -1);
}

constexpr int REC_LISTS_MAX = 64 * 2 * PEM_QUANTILE_MAX_Q;     // (column, quantile) pairs the record kernels keep a table of (m <= 128)

// the list (column * nq + quantile) of a record: the bracket of its column whose high words hold the key's (they do not overlap)
template <int NQ>
__device__ __forceinline__ int record_list(const uint4* __restrict__ s_br, const pem::Record& e, unsigned& t, unsigned& mult, bool& none) {
    const unsigned kh = (unsigned)(e.key >> 32);
    const int c0 = (int)e.col * NQ;
    int cq = c0;
    uint4 b[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) b[q] = s_br[c0 + q];
    t = kh - b[0].x;
    mult = b[0].z;
    none = t > b[0].y;
#pragma unroll
    for (int q = 1; q < NQ; ++q) {
        const unsigned tq = kh - b[q].x;
        if (tq <= b[q].y) {
            cq = c0 + q;
            t = tq;
            mult = b[q].z;
            none = false;
        }
    }
    return cq;
}

constexpr int REC_UNROLL = 4;   // records a thread has in flight

// (the record passes run one workgroup per CU -- its histogram takes the CU's LDS -- so the workgroup is 1024 threads: with 256 the
// passes were latency-bound at 2.5 TB/s over the records)
constexpr int RBLOCK = 1024;
template <int NQ>
__global__ __launch_bounds__(RBLOCK) void record_hist_kernel(const pem::Record* __restrict__ rec, const unsigned* __restrict__ rec_count, unsigned cap,
                                                              unsigned waves, const Bracket* __restrict__ br, int lists, int bins,
                                                              unsigned* __restrict__ hist) {
    extern __shared__ unsigned lds_hist[];                      // [lists][bins]
    __shared__ uint4 s_br[REC_LISTS_MAX];                       // {loh, words, mult, -}
    for (int i = threadIdx.x; i < lists * bins; i += RBLOCK) lds_hist[i] = 0;
    for (int i = threadIdx.x; i < lists; i += RBLOCK) s_br[i] = make_uint4(br[i].loh, br[i].words, br[i].mult, 0u);
    __syncthreads();
    for (unsigned w = blockIdx.x; w < waves; w += gridDim.x) {
        const unsigned cnt = rec_count[w] < cap ? rec_count[w] : cap;
        const pem::Record* r = rec + (size_t)w * cap;
        for (unsigned i0 = threadIdx.x; i0 < cnt; i0 += RBLOCK * REC_UNROLL) {
            pem::Record e[REC_UNROLL];
#pragma unroll
            for (int u = 0; u < REC_UNROLL; ++u) e[u] = r[i0 + u * RBLOCK < cnt ? i0 + u * RBLOCK : i0];
#pragma unroll
            for (int u = 0; u < REC_UNROLL; ++u) {
                unsigned t, mult;
                bool none;
                const int cq = record_list<NQ>(s_br, e[u], t, mult, none);
                // (none: not a value of any bracket -- a NaN's bits; the producer has flagged the run)
                if (!none && i0 + u * RBLOCK < cnt) atomicAdd(&lds_hist[cq * bins + (int)__umulhi(t, mult)], 1u);
            }
        }
    }
    __syncthreads();
    // the workgroup's own counts, whole (no atomics): summed over the workgroups by record_reduce_kernel, and read again -- per chosen
    // sub-bin -- by record_offsets_kernel, which gives every workgroup its own place in every list
    unsigned* mine = hist + (size_t)blockIdx.x * lists * bins;
    for (int i = threadIdx.x; i < lists * bins; i += RBLOCK) mine[i] = lds_hist[i];
}

// 64 cells x 4 slices of the workgroups per block, eight loads in flight per thread (one thread per cell walking the 256 partial
// histograms took 60-120 us of the critical path for 30 MB); the histogram's total and the producer's record count ride along
// (sums[0], sums[1]: record_total_check_kernel compares them)
__global__ __launch_bounds__(256) void record_reduce_kernel(const unsigned* __restrict__ part, int groups, int cells, unsigned* __restrict__ hist,
                                                            const unsigned* __restrict__ rec_count, unsigned cap, unsigned waves,
                                                            u64* __restrict__ sums) {
    __shared__ unsigned s_part[4][64];
    __shared__ u64 s_tot;
    const int cx = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + cx;
    if (threadIdx.x == 0) s_tot = 0;
    unsigned sum = 0;
    if (i < cells) {
        int g = slice;
        for (; g + 28 < groups; g += 32) {
            unsigned v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(g + 4 * u) * cells + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += v[u];
        }
        for (; g < groups; g += 4) sum += part[(size_t)g * cells + i];
    }
    s_part[slice][cx] = sum;
    __syncthreads();
    if (slice == 0) {
        const unsigned all = s_part[0][cx] + s_part[1][cx] + s_part[2][cx] + s_part[3][cx];
        if (i < cells) {
            hist[i] = all;
            atomicAdd(&s_tot, (u64)all);
        }
    }
    if (blockIdx.x == 0) {
        u64 r = 0;
        for (unsigned w = threadIdx.x; w < waves; w += 256) r += rec_count[w] < cap ? rec_count[w] : cap;
        if (r) atomicAdd(&sums[1], r);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_tot) atomicAdd(&sums[0], s_tot);
}

// One wave per target that owns a list: where each workgroup of the copy pass appends its hits -- the exclusive prefix, over the
// workgroups, of their counts in the list's sub-bin (record_hist_kernel's own histograms).  The copy pass then needs no global
// atomic (it drew one per hit: 5.6e5 returning atomics on 910 addresses, 0.36 ms for 580 MB of records).
__global__ __launch_bounds__(64) void record_offsets_kernel(int nt, int bins, const Target* __restrict__ tg, const unsigned* __restrict__ part,
                                                             int groups, int cells, unsigned* __restrict__ woff) {
    const int i = blockIdx.x, lane = threadIdx.x, targets = gridDim.x;
    const Target T = tg[i];
    const int t = i % nt;
    const bool own = !T.done && T.owner == t;
    const int cell = (i / 2) * bins + (own ? T.bin2 : 0);      // targets 2q, 2q + 1 of column c belong to list c nq + q = i / 2
    unsigned base = 0;
    for (int g0 = 0; g0 < groups; g0 += 64) {
        const int g = g0 + lane;
        const unsigned v = (own && g < groups) ? part[(size_t)g * cells + cell] : 0u;
        unsigned incl = v;
#pragma unroll
        for (int sh = 1; sh < 64; sh <<= 1) {
            const unsigned up = __shfl_up(incl, sh);
            if (lane >= sh) incl += up;
        }
        if (g < groups) woff[(size_t)g * targets + i] = base + incl - v;
        base += __shfl(incl, 63);
    }
}

template <int NQ>
__global__ __launch_bounds__(RBLOCK) void record_compact_kernel(const pem::Record* __restrict__ rec, const unsigned* __restrict__ rec_count, unsigned cap,
                                                                 unsigned waves, const Bracket* __restrict__ br, int lists, Target* __restrict__ tg,
                                                                 const unsigned* __restrict__ woff, u64* __restrict__ cand) {
    __shared__ uint4 s_br[REC_LISTS_MAX];                       // {loh, words, mult, -}
    __shared__ int2 s_bin[REC_LISTS_MAX];                       // the sub-bins the quantile's two targets collect (-1: not a list owner)
    __shared__ unsigned s_cur[2 * REC_LISTS_MAX];               // this workgroup's cursor in every target's list (from record_offsets_kernel)
    __shared__ u64 s_base[2 * REC_LISTS_MAX];                   // the lists' starts in `cand`
    const unsigned* my_off = woff + (size_t)blockIdx.x * 2 * lists;
    for (int i = threadIdx.x; i < lists; i += RBLOCK) {
        s_br[i] = make_uint4(br[i].loh, br[i].words, br[i].mult, 0u);
        const Target &T0 = tg[2 * i], &T1 = tg[2 * i + 1];     // targets 2q, 2q + 1 of column c sit at (c nq + q) 2
        s_bin[i] = make_int2((!T0.done && (T0.owner & 1) == 0) ? T0.bin2 : -1, (!T1.done && (T1.owner & 1) == 1) ? T1.bin2 : -1);
        s_cur[2 * i] = my_off[2 * i];
        s_cur[2 * i + 1] = my_off[2 * i + 1];
        s_base[2 * i] = T0.offset;
        s_base[2 * i + 1] = T1.offset;
    }
    __syncthreads();
    // (the same records as this workgroup counted in record_hist_kernel: same grid, same walk)
    for (unsigned w = blockIdx.x; w < waves; w += gridDim.x) {
        const unsigned cnt = rec_count[w] < cap ? rec_count[w] : cap;
        const pem::Record* r = rec + (size_t)w * cap;
        for (unsigned i0 = threadIdx.x; i0 < cnt; i0 += RBLOCK * REC_UNROLL) {
            pem::Record e[REC_UNROLL];
#pragma unroll
            for (int u = 0; u < REC_UNROLL; ++u) e[u] = r[i0 + u * RBLOCK < cnt ? i0 + u * RBLOCK : i0];
#pragma unroll
            for (int u = 0; u < REC_UNROLL; ++u) {
                unsigned t, mult;
                bool none;
                const int cq = record_list<NQ>(s_br, e[u], t, mult, none);
                if (none || i0 + u * RBLOCK >= cnt) continue;
                const int bin = (int)__umulhi(t, mult);
                const int2 want = s_bin[cq];
                const int hit = want.x == bin ? 0 : (want.y == bin ? 1 : -1);
                if (hit >= 0) cand[s_base[2 * cq + hit] + atomicAdd(&s_cur[2 * cq + hit], 1u)] = e[u].key;
            }
        }
    }
    __syncthreads();
    // what this workgroup appended, onto the lists' counters: select_kernel compares them with the counts (the "incomplete" check)
    for (int i = threadIdx.x; i < 2 * lists; i += RBLOCK) {
        const unsigned wrote = s_cur[i] - my_off[i];
        if (wrote) atomicAdd(&tg[i].cursor, (u64)wrote);
    }
}

}  // namespace
