// pem_marginals.hip -- binned counts and kernel density estimates of a pooled MCMC trace, the hot path of
// hallthrusterpem_amd/marginals.py.
//
// What it stands in for: the arrays behind `uq.ndscatter(samples, plot1d='kde', plot2d='hist' / 'hex', bins, cmin)`
// (scripts/pem_v0/mcmc.py:339-385; uqtils is third-party: parity UNPINNED).  The definitions are numpy's and scipy's public
// behaviour: the counts are np.histogram / np.histogram2d with `range=` given, the density is scipy.stats.gaussian_kde's
// formula in one dimension.  The trace stays where the sampler wrote it: n_rows pooled draws of n_par parameters, unit
// column stride, row stride ld.
//
// chain_hist_kernel (pem_chain_hist_f64_dev).  A task is one table: task t < d is the 1-D histogram of parameter t
// (`bins` counters), task d + p is pair p = (i, j), i < j, in the order (0,1), (0,2) ... (d-2,d-1) (bins^2 counters).  A
// workgroup (task block, row block) keeps the tables of its task block in LDS as u32 and walks 128-row tiles:
//   1. bin stage: every value of the tile is binned ONCE, by a multiply-and-truncate guess that is then corrected against the
//      edge table in LDS in both directions until edges[k] <= v < edges[k+1] holds (the last bin also takes v == edges[bins]);
//      the decision is the comparison, never the guess.  The bin, or 255 for "no bin", is one byte in LDS.  The workgroups of
//      task block 0 also count `dropped` and `nonfinite` here.  The values of the NEXT tile are loaded into registers before
//      this tile is counted.
//   2. count stage: lane (task, row slice) reads the two bin bytes of its rows and increments its task's table with an LDS
//      integer add.  Lane tid owns task tid % tasks and row slice tid / tasks, so neighbouring lanes own different tables;
//      with fewer than 64 tasks in the block a wave also holds lanes tid and tid + tasks of ONE task (two at 39 tasks, ten at
//      6), and those meet on a word when their rows fall into one cell.  The add is atomic, so nothing is lost (every row
//      identical: a word sees at most min(row slices, ceil(64 / tasks)) adders per wave-instruction).
//   At the end one 64-bit integer atomicAdd per non-zero counter into the global tables, which the entry point zeroed.
// Integer adds only: the counts do not depend on any order.  A workgroup counts fewer than 2^32 rows (checked on the host).
//
// chain_kde_partial_kernel + chain_kde_reduce_kernel (pem_chain_kde_f64_dev).  Workgroup (256 grid points, parameter,
// 4096-row block); a lane keeps 4 grid points (q = lane, lane + 64, ...) and their sums in registers, the 4 waves take the
// four 64-row quarters of each staged 256-row tile, so one LDS read of a draw feeds 4 exp.  Per grid point: one chain per
// wave over its rows in increasing t (at most 1024 terms), the 4 wave sums added in wave order, one partial per row block
// in the workspace, the partials added in block order and multiplied by scale.  The order depends on n_rows alone, a grid
// point's value not on which other grid points are asked for; no floating-point atomics.
//   a = ((g - x) inv_h)^2 / 2 is formed as written (subtract, multiply, square, halve); exp is the device library's
//   (OCML exp f64, documented to 1 ulp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_PAR = PEM_MARGINALS_MAX_PAR;
constexpr int MAX_BINS = PEM_MARGINALS_MAX_BINS;
constexpr int HIST_ROWS = PEM_HIST_ROW_TILE;           // rows binned per stage
constexpr int CNT_WORDS = 9216;                        // u32 counters per workgroup: 2 tables at 64 bins, 40 at 15
constexpr int HIST_VALS = HIST_ROWS * MAX_PAR / THREADS;   // values of a tile per lane, at most
constexpr int HIST_WGS = 1024;                         // workgroups a launch aims at: two rounds of the two resident per CU
constexpr unsigned char NO_BIN = 255;
constexpr int KDE_POINTS = 4;                          // grid points per lane
constexpr int KDE_GRID_BLOCK = 64 * KDE_POINTS;        // grid points per workgroup
constexpr int KDE_TILE = THREADS;                      // rows staged per step
constexpr int KDE_ROW_BLOCK = PEM_KDE_ROW_BLOCK;
constexpr int REDUCE_THREADS = 256;
static_assert(MAX_BINS < NO_BIN && MAX_BINS * MAX_BINS <= CNT_WORDS && KDE_ROW_BLOCK % KDE_TILE == 0, "tile constants");

__global__ __launch_bounds__(THREADS) void chain_hist_kernel(const double* __restrict__ x, size_t ld, size_t n_rows, int d, int bins,
                                                             const double* __restrict__ edges, int n_tasks, int tpw, size_t n_tiles,
                                                             unsigned long long* __restrict__ hist1d,
                                                             unsigned long long* __restrict__ hist2d,
                                                             unsigned long long* __restrict__ dropped,
                                                             unsigned long long* __restrict__ nonfinite) {
    // dynamic LDS, sized by the host for this launch: edges [d][bins + 1] f64, counters [tpw][bins^2] u32, dropped and
    // nonfinite [2][MAX_PAR] u32, bins of the tile [HIST_ROWS][d] u8
    extern __shared__ double hist_lds[];
    double* edge_s = hist_lds;
    unsigned* cnt = reinterpret_cast<unsigned*>(edge_s + d * (bins + 1));
    unsigned* drop_s = cnt + tpw * bins * bins;
    unsigned char* bin_s = reinterpret_cast<unsigned char*>(drop_s + 2 * MAX_PAR);
    const int tid = threadIdx.x;
    const int slot = bins * bins;
    const int task0 = (int)blockIdx.x * tpw;
    const int ntask = n_tasks - task0 < tpw ? n_tasks - task0 : tpw;
    const bool first = blockIdx.x == 0;
    if (ntask <= 0) return;                                     // uniform; the host's task blocks are never empty

    for (int k = tid; k < ntask * slot; k += THREADS) cnt[k] = 0;
    for (int k = tid; k < d * (bins + 1); k += THREADS) edge_s[k] = edges[k];
    if (tid < 2 * MAX_PAR) drop_s[tid] = 0;

    // count role: task task0 + tid % ntask, rows slice, slice + n_slices, ... of a tile
    const int n_slices = THREADS / ntask;
    const int slice = tid / ntask, tl = tid % ntask;
    const bool counts = slice < n_slices;
    int ci = 0, cj = 0, stride_i = 0;
    unsigned* table = cnt + tl * slot;
    {
        const int task = task0 + tl;
        if (task < d) {
            ci = cj = task;                                     // 1-D: cell = bin of ci
        } else {
            int p = task - d;
            while (p >= d - 1 - ci) {
                p -= d - 1 - ci;
                ++ci;
            }
            cj = ci + 1 + p;
            stride_i = bins;                                    // pair: cell = bin_i * bins + bin_j
        }
    }
    __syncthreads();

    // bin role: elements tid, tid + 256, ... of the tile; their (row, column) do not depend on the tile.  The values of
    // the next tile are loaded into registers while this one is counted, so a tile never waits for memory.
    int er[HIST_VALS], ec[HIST_VALS];
    double val[HIST_VALS];
#pragma unroll
    for (int k = 0; k < HIST_VALS; ++k) {
        const int idx = tid + k * THREADS;
        er[k] = idx < HIST_ROWS * d ? idx / d : -1;
        ec[k] = idx < HIST_ROWS * d ? idx - er[k] * d : 0;
    }
    auto fetch = [&](size_t tile) {
        const size_t row0 = tile * HIST_ROWS;
#pragma unroll
        for (int k = 0; k < HIST_VALS; ++k)
            if (er[k] >= 0 && row0 + er[k] < n_rows) val[k] = x[(row0 + er[k]) * ld + ec[k]];
    };
    if (blockIdx.y < n_tiles) fetch(blockIdx.y);

    for (size_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const size_t row0 = tile * HIST_ROWS;
#pragma unroll
        for (int k = 0; k < HIST_VALS; ++k) {
            if (er[k] < 0) continue;
            const int c = ec[k];
            unsigned char b = NO_BIN;
            if (row0 + er[k] < n_rows) {
                const double v = val[k];
                const double* e = edge_s + c * (bins + 1);
                if (v >= e[0] && v <= e[bins]) {                // false for NaN
                    const double guess = (v - e[0]) * ((double)bins / (e[bins] - e[0]));
                    int q = (int)fmin(fmax(guess, 0.0), (double)(bins - 1));   // fmax(NaN, 0) = 0
                    while (q > 0 && v < e[q]) --q;
                    while (q < bins - 1 && v >= e[q + 1]) ++q;
                    b = (unsigned char)q;                       // edges[q] <= v < edges[q+1], or q = bins-1 and v <= edges[bins]
                }
                if (first) {
                    if (b == NO_BIN) atomicAdd(&drop_s[c], 1u);
                    if (!isfinite(v)) atomicAdd(&drop_s[MAX_PAR + c], 1u);
                }
            }
            bin_s[tid + k * THREADS] = b;
        }
        if (tile + gridDim.y < n_tiles) fetch(tile + gridDim.y);
        __syncthreads();
        if (counts) {
#pragma unroll 4
            for (int r = slice; r < HIST_ROWS; r += n_slices) {
                const unsigned bi = bin_s[r * d + ci], bj = bin_s[r * d + cj];
                if (bi != NO_BIN && bj != NO_BIN) atomicAdd(&table[stride_i ? bi * stride_i + bj : bi], 1u);
            }
        }
        __syncthreads();
    }

    for (int k = tid; k < ntask * slot; k += THREADS) {
        const unsigned v = cnt[k];
        if (!v) continue;
        const int task = task0 + k / slot, cell = k % slot;
        if (task < d)
            atomicAdd(&hist1d[(size_t)task * bins + cell], (unsigned long long)v);
        else
            atomicAdd(&hist2d[(size_t)(task - d) * slot + cell], (unsigned long long)v);
    }
    if (first && tid < d) {
        if (drop_s[tid]) atomicAdd(&dropped[tid], (unsigned long long)drop_s[tid]);
        if (drop_s[MAX_PAR + tid]) atomicAdd(&nonfinite[tid], (unsigned long long)drop_s[MAX_PAR + tid]);
    }
}

// the draws ys[0 .. n) of one wave against NK of the lane's grid points, in increasing t: one chain per grid point
template <int NK>
__device__ __forceinline__ void kde_rows(const double* ys, int n, const double (&g)[KDE_POINTS], double ih, double (&acc)[KDE_POINTS]) {
    for (int t = 0; t < n; ++t) {
        const double y = ys[t];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const double z = (g[k] - y) * ih;
            acc[k] += exp(-(z * z * 0.5));
        }
    }
}

__global__ __launch_bounds__(THREADS) void chain_kde_partial_kernel(const double* __restrict__ x, size_t ld, size_t n_rows,
                                                                    size_t n_grid, const double* __restrict__ grid,
                                                                    const double* __restrict__ inv_h, double* __restrict__ work) {
    __shared__ double ys[KDE_TILE];
    __shared__ double part[THREADS / 64][KDE_GRID_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t par = blockIdx.y, n_par = gridDim.y, rb = blockIdx.z;
    const size_t q0 = (size_t)blockIdx.x * KDE_GRID_BLOCK;
    const int nk = (int)((n_grid - q0 + 63) / 64 < KDE_POINTS ? (n_grid - q0 + 63) / 64 : KDE_POINTS);   // uniform
    double g[KDE_POINTS], acc[KDE_POINTS];
#pragma unroll
    for (int k = 0; k < KDE_POINTS; ++k) {
        const size_t q = q0 + k * 64 + lane;
        g[k] = q < n_grid ? grid[par * n_grid + q] : 0.0;
        acc[k] = 0.0;
    }
    const double ih = inv_h[par];
    const size_t r0 = rb * KDE_ROW_BLOCK;
    const size_t r1 = r0 + KDE_ROW_BLOCK < n_rows ? r0 + KDE_ROW_BLOCK : n_rows;
    for (size_t t0 = r0; t0 < r1; t0 += KDE_TILE) {
        __syncthreads();
        ys[tid] = t0 + tid < r1 ? x[(t0 + tid) * ld + par] : 0.0;
        __syncthreads();
        const size_t first = t0 + (size_t)w * 64;
        const int n = first >= r1 ? 0 : (r1 - first < 64 ? (int)(r1 - first) : 64);
        if (nk == KDE_POINTS)                                   // uniform: the four exp of a draw interleave
            kde_rows<KDE_POINTS>(ys + w * 64, n, g, ih, acc);
        else if (nk == 3)
            kde_rows<3>(ys + w * 64, n, g, ih, acc);
        else if (nk == 2)
            kde_rows<2>(ys + w * 64, n, g, ih, acc);
        else
            kde_rows<1>(ys + w * 64, n, g, ih, acc);
    }
#pragma unroll
    for (int k = 0; k < KDE_POINTS; ++k) part[w][k * 64 + lane] = acc[k];
    __syncthreads();
    const size_t q = q0 + tid;
    if (q < n_grid) work[(rb * n_par + par) * n_grid + q] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

__global__ __launch_bounds__(REDUCE_THREADS) void chain_kde_reduce_kernel(size_t n_grid, size_t total, size_t n_rb,
                                                                          const double* __restrict__ work,
                                                                          const double* __restrict__ scale,
                                                                          double* __restrict__ kde) {
    const size_t i = (size_t)blockIdx.x * REDUCE_THREADS + threadIdx.x;
    if (i >= total) return;
    double s = 0.0;
    for (size_t b = 0; b < n_rb; ++b) s += work[b * total + i];
    kde[i] = scale[i / n_grid] * s;
}

}  // namespace

extern "C" int pem_chain_hist_f64_dev(size_t n_rows, int n_par, size_t ld, const double* x, int bins, const double* edges,
                                      uint64_t* hist1d, uint64_t* hist2d, uint64_t* dropped, uint64_t* nonfinite,
                                      pem_stream_t stream) {
    if (!n_rows) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hist: zero size");
    if (n_par < 1 || n_par > MAX_PAR) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hist: need 1 <= n_par <= %d, got %d", MAX_PAR, n_par);
    if (bins < 1 || bins > MAX_BINS) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hist: need 1 <= bins <= %d, got %d", MAX_BINS, bins);
    if (ld < (size_t)n_par) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hist: ld %zu < n_par %d", ld, n_par);
    if (!x || !edges || !hist1d || !dropped || !nonfinite) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hist: null pointer");
    const int n_pairs = n_par * (n_par - 1) / 2;
    const int n_tasks = n_par + (hist2d ? n_pairs : 0);
    const int slot = bins * bins;
    int tpw = CNT_WORDS / slot < THREADS ? CNT_WORDS / slot : THREADS;
    const int n_tb = (n_tasks + tpw - 1) / tpw;
    tpw = (n_tasks + n_tb - 1) / n_tb;                                   // even task blocks
    const size_t n_tiles = (n_rows + HIST_ROWS - 1) / HIST_ROWS;
    size_t n_rb = HIST_WGS / n_tb ? HIST_WGS / n_tb : 1;
    if (n_rb > n_tiles) n_rb = n_tiles;
    // a workgroup's u32 counters: (tiles per row block) * HIST_ROWS rows must stay below 2^32
    if ((n_tiles + n_rb - 1) / n_rb >= ((size_t)1 << 32) / HIST_ROWS)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hist: n_rows %zu too large for one launch", n_rows);
    if (int rc = pem::check_device()) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(hist1d, 0, sizeof(uint64_t) * n_par * bins, s));
    if (hist2d && n_pairs) HIP_TRY(hipMemsetAsync(hist2d, 0, sizeof(uint64_t) * n_pairs * slot, s));
    HIP_TRY(hipMemsetAsync(dropped, 0, sizeof(uint64_t) * n_par, s));
    HIP_TRY(hipMemsetAsync(nonfinite, 0, sizeof(uint64_t) * n_par, s));
    const size_t lds = sizeof(double) * n_par * (bins + 1) + sizeof(unsigned) * ((size_t)tpw * slot + 2 * MAX_PAR) + (size_t)HIST_ROWS * n_par;
    hipLaunchKernelGGL(chain_hist_kernel, dim3((unsigned)n_tb, (unsigned)n_rb), dim3(THREADS), lds, s, x, ld, n_rows, n_par, bins, edges,
                       n_tasks, tpw, n_tiles, reinterpret_cast<unsigned long long*>(hist1d),
                       reinterpret_cast<unsigned long long*>(hist2d), reinterpret_cast<unsigned long long*>(dropped),
                       reinterpret_cast<unsigned long long*>(nonfinite));
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}

extern "C" int pem_chain_kde_f64_dev(size_t n_rows, int n_par, size_t ld, const double* x, size_t n_grid, const double* grid,
                                     const double* inv_h, const double* scale, double* kde, double* work, size_t work_len,
                                     pem_stream_t stream) {
    if (!n_rows || !n_grid) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_kde: zero size");
    if (n_par < 1 || n_par > MAX_PAR) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_kde: need 1 <= n_par <= %d, got %d", MAX_PAR, n_par);
    if (n_grid > PEM_KDE_MAX_GRID) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_kde: n_grid %zu > %d", n_grid, PEM_KDE_MAX_GRID);
    if (ld < (size_t)n_par) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_kde: ld %zu < n_par %d", ld, n_par);
    if (!x || !grid || !inv_h || !scale || !kde || !work) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_kde: null pointer");
    const size_t n_rb = (n_rows + KDE_ROW_BLOCK - 1) / KDE_ROW_BLOCK;
    if (n_rb > 65535) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_kde: n_rows %zu too large for one launch", n_rows);
    const size_t total = (size_t)n_par * n_grid;
    if (work_len / total < n_rb)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_kde: work_len %zu < ceil(n_rows / %d) * n_par * n_grid", work_len, KDE_ROW_BLOCK);
    if (int rc = pem::check_device()) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(chain_kde_partial_kernel, dim3((unsigned)((n_grid + KDE_GRID_BLOCK - 1) / KDE_GRID_BLOCK), (unsigned)n_par, (unsigned)n_rb),
                       dim3(THREADS), 0, s, x, ld, n_rows, n_grid, grid, inv_h, work);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(chain_kde_reduce_kernel, dim3((unsigned)((total + REDUCE_THREADS - 1) / REDUCE_THREADS)), dim3(REDUCE_THREADS), 0, s,
                       n_grid, total, n_rb, work, scale, kde);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
