// pem_hexbin.hip -- hexagonal pair bins of a pooled MCMC trace, the `plot2d='hex'` panels of hallthrusterpem_amd/marginals.py.
//
// What it stands in for: one matplotlib `Axes.hexbin(x_i, x_j, gridsize=(nx, ny), extent=..., C=None)` call per pair on the
// host, which is what `uq.ndscatter(..., plot2d='hex', bins=15, cmin=...)` of journal_plots draws (scripts/pem_v0/mcmc.py:344-385;
// uqtils is third-party: parity UNPINNED).  The binning rule is matplotlib's, bit for bit (matplotlib/axes/_axes.py, hexbin):
// two rectangular lattices, the second shifted by half a cell; a draw goes to the nearer lattice point under the metric
// dx^2 + 3 dy^2 in lattice coordinates.  With the per-parameter table {x0, sx, y0, sy} (x0 = lo - pad, sx = (hi + pad - x0) / nx,
// y0 = lo, sy = (hi - lo) / ny, pad = 1e-9 (hi - lo): the host's numpy) a draw (x, y) of pair (i, j), i < j, is
//     ix = (x - x0_i) / sx_i               iy = (y - y0_j) / sy_j
//     r1 = rint(ix)  r2 = floor(ix)        s1 = rint(iy)  s2 = floor(iy)
//     d1 = (ix - r1)^2 + 3.0 (iy - s1)^2   d2 = (ix - r2 - 0.5)^2 + 3.0 (iy - s2 - 0.5)^2
//     d1 <  d2: cell r1 (ny + 1) + s1                     iff 0 <= r1 <= nx and 0 <= s1 <= ny
//     else    : cell (nx + 1)(ny + 1) + r2 ny + s2        iff 0 <= r2 <  nx and 0 <= s2 <  ny
// Every operation is rounded once, left to right (contraction is off for this file; the divisions are divisions), so the
// comparison d1 < d2 sees the bits numpy sees; ties go to the second lattice.  The range tests are made on the floating-point
// r and s, so a NaN, an infinity or an |ix| beyond the integers is in no cell and nothing undefined is cast.
//
// chain_hex_kernel (pem_chain_hex_f64_dev) follows chain_hist_kernel (pem_marginals.hip).  A task is one pair's table of
// n_cells = (nx + 1)(ny + 1) + nx ny counters, the pairs in the order (0,1), (0,2) ... (d-2,d-1).  A workgroup (task block, row
// block) keeps the tables of its task block in LDS as u32 and walks 128-row tiles:
//   1. index stage: every value of the tile is turned ONCE into its two lattice coordinates, ix (its role as the x of a pair)
//      and iy (its role as the y), two fp64 divisions per value, kept in LDS as fp64; a row past the end gets NaN.  The values of
//      the NEXT tile are loaded into registers before this tile is counted.
//   2. count stage: lane (task, row slice) reads ix of its pair's i and iy of its j for each of its rows, forms r, s, d1, d2
//      in registers and increments the chosen cell with an LDS integer add.  Lane tid owns task tid % tasks and row slice
//      tid / tasks, as in chain_hist_kernel; the add is atomic, so lanes of one task that meet on a word lose nothing.
//   At the end one 64-bit integer atomicAdd per non-zero counter into the global tables, which the entry point zeroed.
// Integer adds only: the counts do not depend on any order.  A workgroup counts fewer than 2^32 rows (checked on the host).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_PAR = PEM_MARGINALS_MAX_PAR;
constexpr int MAX_GRID = PEM_HEX_MAX_GRID;
constexpr int HEX_ROWS = PEM_HEX_ROW_TILE;             // rows indexed per stage
constexpr int CNT_WORDS = 9216;                        // u32 counters per workgroup, as chain_hist_kernel: 1 table at 64 x 64, 34 at 15 x 8
constexpr int HEX_VALS = HEX_ROWS * MAX_PAR / THREADS; // values of a tile per lane, at most
constexpr int HEX_WGS = 1024;                          // workgroups a launch aims at
static_assert((MAX_GRID + 1) * (MAX_GRID + 1) + MAX_GRID * MAX_GRID <= CNT_WORDS, "the largest table fits a workgroup");

struct HexLattice {
    double v[MAX_PAR][4];                              // {x0, sx, y0, sy} per parameter
};

__global__ __launch_bounds__(THREADS) void chain_hex_kernel(const double* __restrict__ x, size_t ld, size_t n_rows, int d, int nx, int ny,
                                                            HexLattice lat, int n_tasks, int tpw, size_t n_tiles,
                                                            unsigned long long* __restrict__ counts) {
    // dynamic LDS, sized by the host for this launch: lattice [d][4] f64, ix and iy of the tile [HEX_ROWS][d] f64 each,
    // counters [tpw][n_cells] u32
    extern __shared__ double hex_lds[];
    double* lat_s = hex_lds;
    double* ix_s = lat_s + 4 * d;
    double* iy_s = ix_s + HEX_ROWS * d;
    unsigned* cnt = reinterpret_cast<unsigned*>(iy_s + HEX_ROWS * d);
    const int tid = threadIdx.x;
    const int ny1 = ny + 1, n1 = (nx + 1) * ny1;
    const int slot = n1 + nx * ny;
    const int task0 = (int)blockIdx.x * tpw;
    const int ntask = n_tasks - task0 < tpw ? n_tasks - task0 : tpw;
    if (ntask <= 0) return;                                     // uniform; the host's task blocks are never empty

    for (int k = tid; k < ntask * slot; k += THREADS) cnt[k] = 0;
    for (int k = tid; k < 4 * d; k += THREADS) lat_s[k] = lat.v[k >> 2][k & 3];

    // count role: pair task0 + tid % ntask, rows slice, slice + n_slices, ... of a tile
    const int n_slices = THREADS / ntask;
    const int slice = tid / ntask, tl = tid % ntask;
    const bool counting = slice < n_slices;
    int ci = 0, cj = 0;
    unsigned* table = cnt + tl * slot;
    {
        int p = task0 + tl;
        while (p >= d - 1 - ci) {
            p -= d - 1 - ci;
            ++ci;
        }
        cj = ci + 1 + p;
    }
    __syncthreads();

    // index role: elements tid, tid + 256, ... of the tile; their (row, column) do not depend on the tile.  The values of
    // the next tile are loaded into registers while this one is counted.
    int er[HEX_VALS], ec[HEX_VALS];
    double val[HEX_VALS];
#pragma unroll
    for (int k = 0; k < HEX_VALS; ++k) {
        const int idx = tid + k * THREADS;
        er[k] = idx < HEX_ROWS * d ? idx / d : -1;
        ec[k] = idx < HEX_ROWS * d ? idx - er[k] * d : 0;
    }
    auto fetch = [&](size_t tile) {
        const size_t row0 = tile * HEX_ROWS;
#pragma unroll
        for (int k = 0; k < HEX_VALS; ++k)
            if (er[k] >= 0 && row0 + er[k] < n_rows) val[k] = x[(row0 + er[k]) * ld + ec[k]];
    };
    if (blockIdx.y < n_tiles) fetch(blockIdx.y);

    const double fnx = (double)nx, fny = (double)ny;
    for (size_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const size_t row0 = tile * HEX_ROWS;
#pragma unroll
        for (int k = 0; k < HEX_VALS; ++k) {
            if (er[k] < 0) continue;
            double ix = NAN, iy = NAN;                          // a row past the end is in no cell
            if (row0 + er[k] < n_rows) {
                const double v = val[k];
                const double* l = lat_s + 4 * ec[k];
                ix = (v - l[0]) / l[1];
                iy = (v - l[2]) / l[3];
            }
            ix_s[tid + k * THREADS] = ix;
            iy_s[tid + k * THREADS] = iy;
        }
        if (tile + gridDim.y < n_tiles) fetch(tile + gridDim.y);
        __syncthreads();
        if (counting) {
#pragma unroll 2
            for (int r = slice; r < HEX_ROWS; r += n_slices) {
                const double ix = ix_s[r * d + ci], iy = iy_s[r * d + cj];
                const double r1 = rint(ix), s1 = rint(iy);      // half to even, as np.round
                const double r2 = floor(ix), s2 = floor(iy);
                const double ax = ix - r1, ay = iy - s1;
                const double bx = ix - r2 - 0.5, by = iy - s2 - 0.5;
                const double d1 = ax * ax + 3.0 * (ay * ay);
                const double d2 = bx * bx + 3.0 * (by * by);
                int cell = -1;                                  // every comparison below is false for NaN
                if (d1 < d2) {
                    if (r1 >= 0.0 && r1 <= fnx && s1 >= 0.0 && s1 <= fny) cell = (int)r1 * ny1 + (int)s1;
                } else {
                    if (r2 >= 0.0 && r2 < fnx && s2 >= 0.0 && s2 < fny) cell = n1 + (int)r2 * ny + (int)s2;
                }
                if (cell >= 0) atomicAdd(&table[cell], 1u);
            }
        }
        __syncthreads();
    }

    for (int k = tid; k < ntask * slot; k += THREADS) {
        const unsigned v = cnt[k];
        if (v) atomicAdd(&counts[(size_t)task0 * slot + k], (unsigned long long)v);
    }
}

}  // namespace

extern "C" int pem_chain_hex_f64_dev(size_t n_rows, int n_par, size_t ld, const double* x, int nx, int ny, const double* lattice,
                                     uint64_t* counts, pem_stream_t stream) {
    if (!n_rows) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hex: zero size");
    if (n_par < 2 || n_par > MAX_PAR) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hex: need 2 <= n_par <= %d, got %d", MAX_PAR, n_par);
    if (nx < 1 || nx > MAX_GRID || ny < 1 || ny > MAX_GRID)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hex: need 1 <= nx, ny <= %d, got %d, %d", MAX_GRID, nx, ny);
    if (ld < (size_t)n_par) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hex: ld %zu < n_par %d", ld, n_par);
    if (!x || !lattice || !counts) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hex: null pointer");
    HexLattice lat = {};
    for (int i = 0; i < n_par; ++i) {
        const double* l = lattice + 4 * i;
        if (!std::isfinite(l[0]) || !std::isfinite(l[1]) || !std::isfinite(l[2]) || !std::isfinite(l[3]) || !(l[1] > 0.0) || !(l[3] > 0.0))
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hex: lattice of parameter %d must be finite with sx, sy > 0", i);
        for (int k = 0; k < 4; ++k) lat.v[i][k] = l[k];
    }
    const int n_tasks = n_par * (n_par - 1) / 2;
    const int slot = (nx + 1) * (ny + 1) + nx * ny;
    int tpw = CNT_WORDS / slot < THREADS ? CNT_WORDS / slot : THREADS;
    const int n_tb = (n_tasks + tpw - 1) / tpw;
    tpw = (n_tasks + n_tb - 1) / n_tb;                                   // even task blocks
    const size_t n_tiles = (n_rows + HEX_ROWS - 1) / HEX_ROWS;
    size_t n_rb = HEX_WGS / n_tb ? HEX_WGS / n_tb : 1;
    if (n_rb > n_tiles) n_rb = n_tiles;
    // a workgroup's u32 counters: (tiles per row block) * HEX_ROWS rows must stay below 2^32
    if ((n_tiles + n_rb - 1) / n_rb >= ((size_t)1 << 32) / HEX_ROWS)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_hex: n_rows %zu too large for one launch", n_rows);
    if (int rc = pem::check_device()) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(uint64_t) * n_tasks * slot, s));
    const size_t lds = sizeof(double) * n_par * (4 + 2 * (size_t)HEX_ROWS) + sizeof(unsigned) * (size_t)tpw * slot;
    static pem::LdsAttrOnce attr;                                        // up to 101 KB at n_par = 32
    HIP_TRY(attr.ensure(reinterpret_cast<const void*>(chain_hex_kernel)));
    hipLaunchKernelGGL(chain_hex_kernel, dim3((unsigned)n_tb, (unsigned)n_rb), dim3(THREADS), lds, s, x, ld, n_rows, n_par, nx, ny, lat,
                       n_tasks, tpw, n_tiles, reinterpret_cast<unsigned long long*>(counts));
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
