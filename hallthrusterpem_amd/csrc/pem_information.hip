// pem_information.hip -- all-pairs Gaussian log-density with a log-sum-exp over the inner draws, per group of columns: the hot
// path of hallthrusterpem_amd/information.py (the nested Monte Carlo estimator of the expected information gain, Ryan 2003,
// Huan & Marzouk 2013).  The reference has no such analysis: there is nothing to pin, the arithmetic is held to a long double
// restatement (tests/information_np.py).
//
// z_out [n_out][ld_out] standardised observations, z_in [n_in][ld_in] standardised predictions, n_col columns partitioned into
// n_groups contiguous groups by group_end; group index n_groups is the union of all columns.  For every outer row i and group c
//   d2_c(i, j) = sum_{k in c} (z_out[i][k] - z_in[j][k])^2      one fma chain over the group's columns in increasing k;
//                                                               the union's is the sum of the groups' d2 in group order
//   l = -d2 / 2,  m = max_j l,  s1 = sum_j exp(l - m),  s2 = sum_j exp(l - m)^2
//   lse[i][c] = m + log s1 - log n_in,   ess[i][c] = s1^2 / s2
// The n_out x n_in matrix is never written.  Two launches:
//   1. information_partial_kernel: workgroup (32 outer rows, block of 512 inner rows).  The block is walked in tiles of 128
//      inner rows; lane (ti, tj) owns the 4 x 4 pairs (rows ti + 8 r, inner rows tj + 32 q) of a tile and keeps their d2 of
//      the current group and of the union in registers.  Both operands are staged in LDS 16 columns at a time, the next
//      chunk's loads in flight during the FMAs.  At a group's last column the 16 values of a lane are folded into the running
//      (m, s1, s2) of (row, group), which lives in LDS: the tile's maximum by a butterfly over the 32 lanes of a row, the
//      terms against max(running m, tile maximum), their sums by the same butterfly (an addition's two lanes add the same
//      two numbers, so every lane of a row holds the same bits), and one lane per row rescales the running sums.  After the
//      block's last tile the state goes to work[block][row][group][3].
//   2. information_merge_kernel: one lane per (row, group) merges the blocks' states in block order.
// The tiling of the inner rows depends on n_in alone and a pair's chain on its two rows alone: row i's bits depend on that
// row, z_in and the groups, not on n_out, the grid or the other rows of the call.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"

namespace {

constexpr int THREADS = 256;                       // threads of the partial kernel
constexpr int WAVES = 3;                           // its waves per SIMD: three workgroups' LDS fit a CU
constexpr int MERGE_THREADS = 256;                 // threads of the merge kernel
constexpr int MERGE_WAVES = 8;                     // its waves per SIMD
constexpr int MICRO = 4;                           // a lane's pairs: MICRO outer rows x MICRO inner rows
constexpr int LANES_J = 32;                        // lanes along the inner rows: one half of a wave, one butterfly
constexpr int LANES_I = THREADS / LANES_J;         // 8
constexpr int TILE_I = LANES_I * MICRO;            // 32 outer rows per workgroup
constexpr int TILE_J = LANES_J * MICRO;            // 128 inner rows per tile
constexpr int BLOCK_J = PEM_INFORMATION_INNER_BLOCK;   // inner rows per workgroup: one partial state per block
constexpr int CHUNK = PEM_INFORMATION_CHUNK;       // columns staged per step
constexpr int LDC = CHUNK + 1;                     // odd row stride: lanes tj = 0 .. 31 read 32 different bank pairs
constexpr int STAGE_ROWS = THREADS / CHUNK;        // rows one staging pass covers
constexpr int PASSES_I = TILE_I / STAGE_ROWS;      // 2
constexpr int PASSES_J = TILE_J / STAGE_ROWS;      // 8
constexpr int MAX_SETS = PEM_INFORMATION_MAX_GROUPS + 1;   // the groups and their union
static_assert(BLOCK_J % TILE_J == 0 && TILE_I % STAGE_ROWS == 0 && TILE_J % STAGE_ROWS == 0 && THREADS % CHUNK == 0 &&
              LANES_J == 32, "tile constants");

struct GroupEnds {
    int end[PEM_INFORMATION_MAX_GROUPS];
};

// the same value in all 32 lanes of a row: lanes l and l ^ w exchange and combine the same two numbers
__device__ __forceinline__ double row_max(double v) {
#pragma unroll
    for (int w = LANES_J / 2; w >= 1; w >>= 1) v = fmax(v, __shfl_xor(v, w));
    return v;
}
__device__ __forceinline__ double row_sum(double v) {
#pragma unroll
    for (int w = LANES_J / 2; w >= 1; w >>= 1) v += __shfl_xor(v, w);
    return v;
}

__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void information_partial_kernel(
    size_t n_out, size_t n_in, int n_col, const double* __restrict__ z_out, size_t ld_out, const double* __restrict__ z_in,
    size_t ld_in, int n_groups, GroupEnds ends, double* __restrict__ work) {
    __shared__ double sa[TILE_I][LDC];
    __shared__ double sb[TILE_J][LDC];
    __shared__ double st_m[MAX_SETS][TILE_I], st_s1[MAX_SETS][TILE_I], st_s2[MAX_SETS][TILE_I];
    __shared__ int ge[PEM_INFORMATION_MAX_GROUPS];

    const int t = threadIdx.x;
    const int tj = t % LANES_J, ti = t / LANES_J;
    const size_t i0 = (size_t)blockIdx.x * TILE_I;
    const size_t j0 = (size_t)blockIdx.y * BLOCK_J;
    const size_t j1 = j0 + BLOCK_J < n_in ? j0 + BLOCK_J : n_in;
    const int n_tiles = (int)((j1 - j0 + TILE_J - 1) / TILE_J);
    const int n_chunks = (n_col + CHUNK - 1) / CHUNK;
    const int n_sets = n_groups + 1;

    for (int e = t; e < n_sets * TILE_I; e += THREADS) {
        st_m[e / TILE_I][e % TILE_I] = -INFINITY;
        st_s1[e / TILE_I][e % TILE_I] = 0.0;
        st_s2[e / TILE_I][e % TILE_I] = 0.0;
    }
    if (t < PEM_INFORMATION_MAX_GROUPS) ge[t] = ends.end[t];

    // staging role: column sc of rows sr, sr + STAGE_ROWS, ...; what lies past a row or column count is staged as zero
    const int sc = t % CHUNK, sr = t / CHUNK;
    double pre_a[PASSES_I], pre_b[PASSES_J];
    auto fetch = [&](int step) {
        const int tile = step / n_chunks, k = (step % n_chunks) * CHUNK + sc;
        const size_t jb = j0 + (size_t)tile * TILE_J;
#pragma unroll
        for (int p = 0; p < PASSES_I; ++p) {
            const size_t i = i0 + sr + p * STAGE_ROWS;
            pre_a[p] = (k < n_col && i < n_out) ? z_out[i * ld_out + k] : 0.0;
        }
#pragma unroll
        for (int p = 0; p < PASSES_J; ++p) {
            const size_t j = jb + sr + p * STAGE_ROWS;
            pre_b[p] = (k < n_col && j < j1) ? z_in[j * ld_in + k] : 0.0;
        }
    };

    // fold the lane's 16 values of one set (a group, or the union) into the running state of its 4 rows
    auto fold = [&](const double (&d2)[MICRO][MICRO], int set, unsigned valid) {
#pragma unroll
        for (int r = 0; r < MICRO; ++r) {
            double l[MICRO], lm = -INFINITY;
#pragma unroll
            for (int q = 0; q < MICRO; ++q) {
                l[q] = (valid >> q & 1u) ? -0.5 * d2[r][q] : -INFINITY;
                lm = fmax(lm, l[q]);
            }
            lm = row_max(lm);
            const int row = ti + LANES_I * r;
            const double m_old = st_m[set][row];
            const double m_new = fmax(m_old, lm);
            double p1 = 0.0, p2 = 0.0;
#pragma unroll
            for (int q = 0; q < MICRO; ++q) {
                const double e = exp(l[q] - m_new);
                p1 += e;
                p2 = fma(e, e, p2);
            }
            p1 = row_sum(p1);
            p2 = row_sum(p2);
            if (tj == 0) {
                const double sc1 = exp(m_old - m_new);       // 0 for the first tile (m_old = -inf), 1 while the maximum stands
                st_m[set][row] = m_new;
                st_s1[set][row] = fma(st_s1[set][row], sc1, p1);
                st_s2[set][row] = fma(st_s2[set][row], sc1 * sc1, p2);
            }
        }
    };

    fetch(0);
    const int n_steps = n_tiles * n_chunks;
    double acc[MICRO][MICRO], uni[MICRO][MICRO];
    int set = 0;
    unsigned valid = 0;
    for (int step = 0; step < n_steps; ++step) {
        const int tile = step / n_chunks, chunk = step % n_chunks;
        __syncthreads();                                     // every lane is done with the previous chunk (and the state is set)
#pragma unroll
        for (int p = 0; p < PASSES_I; ++p) sa[sr + p * STAGE_ROWS][sc] = pre_a[p];
#pragma unroll
        for (int p = 0; p < PASSES_J; ++p) sb[sr + p * STAGE_ROWS][sc] = pre_b[p];
        __syncthreads();
        if (step + 1 < n_steps) fetch(step + 1);             // in flight during the FMAs below
        if (chunk == 0) {
            set = 0;
            valid = 0;
#pragma unroll
            for (int q = 0; q < MICRO; ++q) valid |= (j0 + (size_t)tile * TILE_J + tj + LANES_J * q < j1 ? 1u : 0u) << q;
#pragma unroll
            for (int r = 0; r < MICRO; ++r)
#pragma unroll
                for (int q = 0; q < MICRO; ++q) acc[r][q] = uni[r][q] = 0.0;
        }
        const int k0 = chunk * CHUNK;
        const int k_end = n_col - k0 < CHUNK ? n_col - k0 : CHUNK;
        int kk = 0;
        while (kk < k_end) {
            const int g_end = ge[set] - k0;                  // > kk: the groups are not empty
            const int seg = g_end < k_end ? g_end : k_end;
#pragma unroll 4
            for (; kk < seg; ++kk) {
                double a[MICRO], b[MICRO];
#pragma unroll
                for (int r = 0; r < MICRO; ++r) a[r] = sa[ti + LANES_I * r][kk];
#pragma unroll
                for (int q = 0; q < MICRO; ++q) b[q] = sb[tj + LANES_J * q][kk];
#pragma unroll
                for (int r = 0; r < MICRO; ++r)
#pragma unroll
                    for (int q = 0; q < MICRO; ++q) {
                        const double d = a[r] - b[q];
                        acc[r][q] = fma(d, d, acc[r][q]);
                    }
            }
            if (kk == g_end) {                               // the group's last column: uniform over the workgroup
                fold(acc, set, valid);
#pragma unroll
                for (int r = 0; r < MICRO; ++r)
#pragma unroll
                    for (int q = 0; q < MICRO; ++q) {
                        uni[r][q] += acc[r][q];
                        acc[r][q] = 0.0;
                    }
                ++set;
                if (set == n_groups) fold(uni, n_groups, valid);
            }
        }
    }
    __syncthreads();
    for (int e = t; e < n_sets * TILE_I; e += THREADS) {
        const int c = e / TILE_I, row = e % TILE_I;
        if (i0 + row < n_out) {
            double* w = work + (((size_t)blockIdx.y * n_out + i0 + row) * n_sets + c) * 3;
            w[0] = st_m[c][row];
            w[1] = st_s1[c][row];
            w[2] = st_s2[c][row];
        }
    }
}

__global__ __launch_bounds__(MERGE_THREADS) __attribute__((amdgpu_waves_per_eu(MERGE_WAVES, MERGE_WAVES))) void information_merge_kernel(
    size_t per_block, size_t n_blocks, double log_n_in, const double* __restrict__ work, double* __restrict__ lse,
    double* __restrict__ ess) {
    const size_t e = (size_t)blockIdx.x * MERGE_THREADS + threadIdx.x;      // (row, set)
    if (e >= per_block) return;
    double m = -INFINITY;
    for (size_t b = 0; b < n_blocks; ++b) m = fmax(m, work[(b * per_block + e) * 3]);
    double s1 = 0.0, s2 = 0.0;
    for (size_t b = 0; b < n_blocks; ++b) {
        const double* w = work + (b * per_block + e) * 3;
        const double sc1 = exp(w[0] - m);
        s1 = fma(w[1], sc1, s1);
        s2 = fma(w[2], sc1 * sc1, s2);
    }
    lse[e] = m + log(s1) - log_n_in;
    ess[e] = s1 * s1 / s2;
}

size_t blocks_of(size_t n_in) { return (n_in + BLOCK_J - 1) / BLOCK_J; }

}  // namespace

extern "C" size_t pem_pairwise_lse_work_len(size_t n_out, size_t n_in, int n_groups) {
    if (!n_out || !n_in || n_groups < 1 || n_groups > PEM_INFORMATION_MAX_GROUPS) return 0;
    const size_t per_row = 3 * (size_t)(n_groups + 1), nb = blocks_of(n_in);
    if (n_out > SIZE_MAX / per_row || n_out * per_row > SIZE_MAX / sizeof(double) / nb) return 0;
    return n_out * per_row * nb;
}

extern "C" int pem_pairwise_lse_f64_dev(size_t n_out, size_t n_in, int n_col, const double* z_out, size_t ld_out,
                                        const double* z_in, size_t ld_in, int n_groups, const int* group_end, double* lse,
                                        double* ess, double* work, size_t work_len, pem_stream_t stream) {
    if (!n_out || !n_in || n_col < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: zero size");
    if (n_groups < 1 || n_groups > PEM_INFORMATION_MAX_GROUPS)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: n_groups %d outside [1, PEM_INFORMATION_MAX_GROUPS = %d]", n_groups,
                         PEM_INFORMATION_MAX_GROUPS);
    if (!z_out || !z_in || !group_end || !lse || !ess || !work) return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: null pointer");
    if (ld_out < (size_t)n_col || ld_in < (size_t)n_col)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: ld_out %zu or ld_in %zu < n_col %d", ld_out, ld_in, n_col);
    GroupEnds ends;
    for (int c = 0; c < PEM_INFORMATION_MAX_GROUPS; ++c) ends.end[c] = n_col;
    for (int c = 0, prev = 0; c < n_groups; prev = group_end[c++]) {
        if (group_end[c] <= prev || group_end[c] > n_col)
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: group_end[%d] = %d: the ends must ascend strictly within (0, n_col = %d]",
                             c, group_end[c], n_col);
        ends.end[c] = group_end[c];
    }
    if (group_end[n_groups - 1] != n_col)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: the last group ends at %d, not at n_col = %d", group_end[n_groups - 1], n_col);
    const size_t n_ti = (n_out + TILE_I - 1) / TILE_I, nb = blocks_of(n_in);
    // (a workgroup counts ceil(n_col / CHUNK) * BLOCK_J / TILE_J steps in an int: below 2^29 once n_col + CHUNK does not overflow)
    if (n_ti > 0x7fffffffu || nb > 65535 || n_col > 0x7fffffff - CHUNK)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: problem too large for one launch");
    const size_t need = pem_pairwise_lse_work_len(n_out, n_in, n_groups);
    if (!need || work_len < need)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: work_len %zu < %zu = ceil(n_in / %d) * n_out * (n_groups + 1) * 3", work_len,
                         need, BLOCK_J);
    if (int rc = pem::check_device()) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(information_partial_kernel, dim3((unsigned)n_ti, (unsigned)nb), dim3(THREADS), 0, s, n_out, n_in, n_col, z_out,
                       ld_out, z_in, ld_in, n_groups, ends, work);
    HIP_TRY(hipGetLastError());
    const size_t per_block = n_out * (size_t)(n_groups + 1);
    const size_t merge_blocks = (per_block + MERGE_THREADS - 1) / MERGE_THREADS;
    if (merge_blocks > 0x7fffffffu) return pem::fail(PEM_ERR_INVALID_ARG, "pem_pairwise_lse: problem too large for one launch");
    hipLaunchKernelGGL(information_merge_kernel, dim3((unsigned)merge_blocks), dim3(MERGE_THREADS), 0, s, per_block, nb,
                       log((double)n_in), work, lse, ess);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
