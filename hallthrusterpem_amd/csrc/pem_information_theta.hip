// pem_information_theta.hip -- the conditional term of the information gain about a subset of the inputs: for every outer draw
// the log-mean-exp of the Gaussian log-density of its observation over that draw's OWN set of predictions (the inputs asked
// about held at the draw's values, the other inputs drawn anew), per group of columns.  The hot path of
// hallthrusterpem_amd/information.py's `about=`; the reference has no such analysis, the arithmetic is held to a long double
// restatement (tests/information_theta_np.py).
//
// z_out [n_out][ld_out] standardised observations; pred [n_out n_per][ld_pred] the raw output of the system-predict launch (padding
// records included), outer row i owning rows i n_per ... (i + 1) n_per - 1; column k of the estimator is record col[k] of a row
// times scale[k].  For outer row i, its row l and group c
//   v_k    = fl64(pred[i n_per + l][col[k]] * scale[k])      rounded before the subtraction
//   d2_c   = sum_{k in c} (z_out[i][k] - v_k)^2              one fma chain in increasing k; the union's is the sum of the groups'
//   a row is used iff its union d2 is finite;  l = -d2 / 2,  m = max l,  s1 = sum exp(l - m),  s2 = sum exp(l - m)^2 over the used rows
//   lse[i][c] = m + log s1 - log used[i],   ess[i][c] = s1^2 / s2;   used[i] = 0 gives NaN for both
// Neither the gathered columns nor the scaled (n_out n_per, n_col) tensor is written.  One launch: a workgroup of one wave owns an
// outer row and walks its rows in tiles of 64, lane = row.  A tile is staged in LDS 32 columns at a time -- the gather and the
// scaling happen on the way in, a wave load covering 2 rows x 32 columns, the next chunk's 32 loads per lane in flight during the
// FMAs and its record indices looked up a chunk earlier -- and
// every lane runs its row's chain, leaving d2 of each group in LDS.  After a tile's last column the lanes know which rows are
// used (the others get d2 = inf) and the tile is folded into the running (m, s1, s2) of every set, which lane c keeps for set c
// in registers, with the lanes changing roles: as sets they take the tile's smallest d2 against the running maximum, as rows
// they replace d2 by exp(-d2 / 2 - m) for every set, as sets they sum the 64 terms (4 interleaved chains in row order) and
// rescale the running sums.  No cross-lane reduction, one exponential per (row, set).
// The tiling depends on n_per alone and a chain on its two rows alone: row i's bits depend on that row, its n_per rows, col,
// scale and the groups, not on n_out or the grid.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"

namespace {

constexpr int THREADS = 64;                        // one wave: lane = a row of the tile
constexpr int WAVES = 1;                           // declared waves per SIMD: four workgroups' LDS fit a CU
constexpr int TILE = THREADS;                      // rows per tile
constexpr int CHUNK = PEM_CONDITIONAL_CHUNK;       // columns staged per step: 256 contiguous bytes of a row where col ascends
constexpr int LDC = CHUNK + 1;                     // odd row stride: the lanes read different banks
constexpr int STAGE_ROWS = THREADS / CHUNK;        // rows one staging pass covers
constexpr int PASSES = TILE / STAGE_ROWS;          // 32 loads per lane and chunk
constexpr int MAX_SETS = PEM_INFORMATION_MAX_GROUPS + 1;   // the groups and their union
constexpr int LDT = TILE + 1;                      // odd stride of a set's rows: the lanes as sets read different banks
constexpr int LANES = 4;                           // interleaved chains of a set's sum over the rows of a tile
static_assert(THREADS % CHUNK == 0 && TILE % STAGE_ROWS == 0 && MAX_SETS <= THREADS && TILE % LANES == 0 && LANES == 4,
              "tile constants");

struct GroupEnds {
    int end[PEM_INFORMATION_MAX_GROUPS];
};

__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void conditional_lse_kernel(
    size_t n_per, int n_col, const double* __restrict__ z_out, size_t ld_out, const double* __restrict__ pred, size_t ld_pred,
    const int* __restrict__ col, const double* __restrict__ scale, int n_groups, GroupEnds ends, double* __restrict__ lse,
    double* __restrict__ ess, int* __restrict__ used) {
    __shared__ double sa[CHUNK];
    __shared__ double sb[TILE][LDC];
    __shared__ double sd[MAX_SETS][LDT];                           // d2, then the term, of (set, row of the tile)
    __shared__ double sm[MAX_SETS];                                // the sets' running maxima, for the lanes as rows
    __shared__ int ge[PEM_INFORMATION_MAX_GROUPS];

    const int t = threadIdx.x;
    const size_t i = blockIdx.x;
    const double* __restrict__ zo = z_out + i * ld_out;
    const double* __restrict__ rows = pred + i * n_per * ld_pred;
    const size_t n_tiles = (n_per + TILE - 1) / TILE;
    const int n_chunks = (n_col + CHUNK - 1) / CHUNK;
    const int n_sets = n_groups + 1;

    double m = -INFINITY, s1 = 0.0, s2 = 0.0;                      // lane c < n_sets: the running state of set c
    if (t < PEM_INFORMATION_MAX_GROUPS) ge[t] = ends.end[t];

    // staging role: column sc of rows sr, sr + STAGE_ROWS, ...; what lies past a row or column count is staged as zero, a record
    // index outside the row as NaN (its rows are then not used)
    const int sc = t % CHUNK, sr = t / CHUNK;
    double pre_a, pre_b[PASSES];
    // the lane's column of a chunk: its record index, factor and observation, looked up one chunk before the chunk is fetched, so
    // that a fetch does not wait for its own addresses
    long long nx_c = 0;
    double nx_s = 1.0, nx_a = 0.0;
    auto lookup = [&](int chunk) {
        const int k = chunk * CHUNK + sc;
        const bool in = k < n_col;
        nx_c = in ? (col ? (long long)col[k] : (long long)k) : -1;
        nx_s = (in && scale) ? scale[k] : 1.0;
        nx_a = (in && sr == 0) ? zo[k] : 0.0;
    };
    // A fetch only loads: every pass from a valid address (the set's first record where the pass has no row or column), with
    // nothing that waits for a load between the loads; `staged` makes the value of a pass once the loads have landed.
    bool pre_ok = false;
    size_t pre_left = 0;
    double pre_s = 1.0;
    auto fetch = [&](size_t tile, int chunk) {
        const bool in = chunk * CHUNK + sc < n_col;
        pre_ok = nx_c >= 0 && (unsigned long long)nx_c < ld_pred;
        pre_s = nx_s;
        pre_a = nx_a;
        const size_t l0 = tile * TILE + sr;                  // the lane's first row of the tile; its rows left in the set:
        pre_left = in && l0 < n_per ? n_per - l0 : 0;
        const double* src = rows + l0 * ld_pred + (pre_ok ? (size_t)nx_c : 0);
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            pre_b[p] = *((size_t)(p * STAGE_ROWS) < pre_left ? src : rows);
            src += STAGE_ROWS * ld_pred;
        }
        lookup(chunk + 1 < n_chunks ? chunk + 1 : 0);        // the chunk that is fetched next, in this tile or the next
    };
    auto staged = [&](int p) {
        return (size_t)(p * STAGE_ROWS) < pre_left ? (pre_ok ? __dmul_rn(pre_b[p], pre_s) : (double)NAN) : 0.0;
    };

    lookup(0);
    fetch(0, 0);
    int n_used = 0;
    for (size_t tile = 0; tile < n_tiles; ++tile) {
        const bool valid = tile * TILE + t < n_per;
        double acc = 0.0;
        int set = 0;
        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            __syncthreads();                                 // every lane is done with the previous chunk (and the state is set)
            if (sr == 0) sa[sc] = pre_a;
#pragma unroll
            for (int p = 0; p < PASSES; ++p) sb[sr + p * STAGE_ROWS][sc] = staged(p);
            __syncthreads();
            if (chunk + 1 < n_chunks) fetch(tile, chunk + 1);    // in flight during the FMAs below
            else if (tile + 1 < n_tiles) fetch(tile + 1, 0);
            const int k0 = chunk * CHUNK;
            const int k_end = n_col - k0 < CHUNK ? n_col - k0 : CHUNK;
            int kk = 0;
            while (kk < k_end) {
                const int g_end = ge[set] - k0;              // > kk: the groups are not empty
                const int seg = g_end < k_end ? g_end : k_end;
#pragma unroll 4
                for (; kk < seg; ++kk) {
                    const double d = sa[kk] - sb[t][kk];
                    acc = fma(d, d, acc);
                }
                if (kk == g_end) {                           // the group's last column: uniform over the wave
                    sd[set][t] = acc;
                    acc = 0.0;
                    ++set;
                }
            }
        }
        // the tile's rows are complete.  Lane = row: which rows are used; a row that is not gets d2 = inf in every set
        double uni = 0.0;
        for (int c = 0; c < n_groups; ++c) uni += sd[c][t];
        const bool use = valid && isfinite(uni);
        n_used += __popcll(__ballot(use));
        if (use) {
            sd[n_groups][t] = uni;
        } else {
            for (int c = 0; c < n_sets; ++c) sd[c][t] = INFINITY;
        }
        __syncthreads();
        // lane = set: the tile's smallest d2 against the running maximum
        const double m_old = m;
        if (t < n_sets) {
            double lo[LANES];
#pragma unroll
            for (int j = 0; j < LANES; ++j) lo[j] = INFINITY;
            for (int r = 0; r < TILE; r += LANES)
#pragma unroll
                for (int j = 0; j < LANES; ++j) lo[j] = fmin(lo[j], sd[t][r + j]);
            m = fmax(m_old, -0.5 * fmin(fmin(lo[0], lo[1]), fmin(lo[2], lo[3])));
            sm[t] = m;
        }
        __syncthreads();
        // lane = row: every set's term against the new maximum (0 for a row that is not used, and before the first used row)
        for (int c = 0; c < n_sets; ++c) {
            const double mc = sm[c];
            sd[c][t] = mc == -INFINITY ? 0.0 : exp(-0.5 * sd[c][t] - mc);
        }
        __syncthreads();
        // lane = set: the tile's sums, LANES interleaved chains in row order, and the rescaled running sums
        if (t < n_sets && m != -INFINITY) {
            double p1[LANES], p2[LANES];
#pragma unroll
            for (int j = 0; j < LANES; ++j) p1[j] = p2[j] = 0.0;
            for (int r = 0; r < TILE; r += LANES)
#pragma unroll
                for (int j = 0; j < LANES; ++j) {
                    const double e = sd[t][r + j];
                    p1[j] += e;
                    p2[j] = fma(e, e, p2[j]);
                }
            const double sc1 = exp(m_old - m);               // 0 before the first used row (m_old = -inf), 1 while the maximum stands
            s1 = fma(s1, sc1, (p1[0] + p1[1]) + (p1[2] + p1[3]));
            s2 = fma(s2, sc1 * sc1, (p2[0] + p2[1]) + (p2[2] + p2[3]));
        }
    }
    if (t < n_sets) {
        lse[i * n_sets + t] = n_used ? m + log(s1) - log((double)n_used) : (double)NAN;
        ess[i * n_sets + t] = n_used ? s1 * s1 / s2 : (double)NAN;
    }
    if (t == 0) used[i] = n_used;
}

bool mul_overflows(size_t a, size_t b) { return b && a > SIZE_MAX / b; }

}  // namespace

extern "C" int pem_conditional_lse_f64_dev(size_t n_out, size_t n_per, int n_col, const double* z_out, size_t ld_out,
                                           const double* pred, size_t ld_pred, const int* col, const double* scale, int n_groups,
                                           const int* group_end, double* lse, double* ess, int* used, pem_stream_t stream) {
    if (!n_out || !n_per || n_col < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: zero size");
    if (n_groups < 1 || n_groups > PEM_INFORMATION_MAX_GROUPS)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: n_groups %d outside [1, PEM_INFORMATION_MAX_GROUPS = %d]", n_groups,
                         PEM_INFORMATION_MAX_GROUPS);
    if (!z_out || !pred || !group_end || !lse || !ess || !used)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: null pointer");
    if (ld_out < (size_t)n_col) return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: ld_out %zu < n_col %d", ld_out, n_col);
    if (ld_pred < 1) return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: ld_pred %zu < 1", ld_pred);
    if (!col && ld_pred < (size_t)n_col)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: ld_pred %zu < n_col %d without col (column k is record k)", ld_pred, n_col);
    GroupEnds ends;
    for (int c = 0; c < PEM_INFORMATION_MAX_GROUPS; ++c) ends.end[c] = n_col;
    for (int c = 0, prev = 0; c < n_groups; prev = group_end[c++]) {
        if (group_end[c] <= prev || group_end[c] > n_col)
            return pem::fail(PEM_ERR_INVALID_ARG,
                             "pem_conditional_lse: group_end[%d] = %d: the ends must ascend strictly within (0, n_col = %d]", c,
                             group_end[c], n_col);
        ends.end[c] = group_end[c];
    }
    if (group_end[n_groups - 1] != n_col)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: the last group ends at %d, not at n_col = %d", group_end[n_groups - 1],
                         n_col);
    // the byte offsets of the last elements of pred, z_out and lse must fit size_t
    if (mul_overflows(n_out, n_per) || mul_overflows(n_out * n_per, ld_pred) || mul_overflows(n_out * n_per * ld_pred, sizeof(double)) ||
        mul_overflows(n_out, ld_out) || mul_overflows(n_out * ld_out, sizeof(double)) ||
        mul_overflows(n_out, (size_t)(n_groups + 1) * sizeof(double)))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: n_out %zu x n_per %zu x ld_pred %zu (or n_out x ld_out %zu) is past size_t",
                         n_out, n_per, ld_pred, ld_out);
    // (a workgroup counts its used rows in an int and its chunks in an int)
    if (n_out > 0x7fffffffu || n_per > 0x7fffffffu || n_col > 0x7fffffff - CHUNK)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_conditional_lse: problem too large for one launch");
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(conditional_lse_kernel, dim3((unsigned)n_out), dim3(THREADS), 0, static_cast<hipStream_t>(stream), n_per, n_col,
                       z_out, ld_out, pred, ld_pred, col, scale, n_groups, ends, lse, ess, used);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
