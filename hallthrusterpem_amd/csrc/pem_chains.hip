// pem_chains.hip -- autocovariance of MCMC chains, the hot path of hallthrusterpem_amd/diagnostics.py.
//
// What it stands in for: the lag sums behind `uq.autocorrelation(samples, step=20, maxlag=500)` (scripts/pem_v0/mcmc.py:310;
// uqtils is third-party: parity UNPINNED) and behind split R-hat and the cross-chain ESS.  The trace stays where the
// sampler wrote it: an (n, K, d) device tensor seen as n rows of K*d series, unit column stride, row stride ld.
//
// For every segment s (rows s*seg_stride ... + seg_len) and series c, with N = seg_len and y_t = x_t - mean:
//   mean[s][c]    = (1/N) sum_t x_t
//   acov[s][i][c] = (1/N) sum_{t < N - l} y_t y_{t+l},    l = lag0 + i*lag_step
//
// Three launches, every sum in an order that depends only on N and the series:
//   1. chain_mean_kernel: row group g of 32 sums rows g, g + 32, ... in order; the 32 group sums are added in order.
//      A non-finite mean is stored as NaN, so every value staged from that series is NaN.
//   2. chain_acov_partial_kernel: workgroup (128-lag block, 32-series block, segment x 4096-row time block).  The values
//      are centred as they are staged in LDS, 64 rows at a time.  Lane (series, window) owns 16 consecutive lags and
//      keeps y_{t+l0} ... y_{t+l0+15} in registers; the time loop is unrolled by 16, so the window rotates by register
//      index and each time step costs two LDS reads (y_t and the window's next value) for 16 FMAs.  The shifted operand
//      lives in a ring of 192 rows that receives 64 new rows per stage.  One fma chain per lag runs over the time block
//      in increasing t; products past the end of the segment or of the time block are products with a staged zero and
//      leave the sum unchanged, so a lag's partial does not depend on the lag block or on which other lags are asked for.
//      One deterministic partial per (segment, time block, lag, series) goes to the caller's workspace.
//   3. chain_acov_reduce_kernel: the time-block partials summed in block order, divided by N.
// No floating-point atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"

namespace {

constexpr int COLS = 32;                       // series per workgroup: one 256-byte LDS row, conflict-free ds_read_b64
constexpr int R = 16;                          // lags per lane: the register window
constexpr int WINDOWS = 8;                     // lag windows per workgroup
constexpr int THREADS = COLS * WINDOWS;        // 256
constexpr int LAG_BLOCK = R * WINDOWS;         // 128 lags per workgroup
constexpr int CHUNK = 64;                      // rows staged per step
constexpr int RING = CHUNK + LAG_BLOCK;        // rows of the shifted operand held in LDS
constexpr int STAGE_ROWS = THREADS / COLS;     // rows one staging instruction covers
constexpr int TIME_BLOCK = PEM_CHAIN_TIME_BLOCK;
constexpr int MEAN_GROUPS = 32;
constexpr int REDUCE_THREADS = 256;
static_assert(TIME_BLOCK % CHUNK == 0 && CHUNK % R == 0 && RING % R == 0 && CHUNK % STAGE_ROWS == 0 &&
              LAG_BLOCK % STAGE_ROWS == 0, "tile constants");

__device__ double chain_zero = 0.0;            // never written: what an out-of-range staging load reads

__global__ __launch_bounds__(COLS * MEAN_GROUPS) void chain_mean_kernel(const double* __restrict__ x, size_t ld, size_t n_series,
                                                                        size_t seg_len, size_t seg_stride,
                                                                        double* __restrict__ mean) {
    __shared__ double part[MEAN_GROUPS][COLS];
    const int c = threadIdx.x % COLS, g = threadIdx.x / COLS;
    const size_t col = (size_t)blockIdx.x * COLS + c, seg = blockIdx.y;
    double s = 0.0;
    if (col < n_series) {
        const double* p = x + seg * seg_stride * ld + col;
        for (size_t t = g; t < seg_len; t += MEAN_GROUPS) s += p[t * ld];
    }
    part[g][c] = s;
    __syncthreads();
    if (g == 0 && col < n_series) {
        double t = 0.0;
        for (int k = 0; k < MEAN_GROUPS; ++k) t += part[k][c];
        const double m = t / (double)seg_len;
        mean[seg * n_series + col] = isfinite(m) ? m : NAN;
    }
}

__global__ __launch_bounds__(THREADS, 2) void chain_acov_partial_kernel(const double* __restrict__ x, size_t ld, size_t n_series,
                                                                        size_t seg_len, size_t seg_stride, size_t lag0,
                                                                        size_t lag_step, size_t n_lags, unsigned n_lb,
                                                                        unsigned n_tb, const double* __restrict__ mean,
                                                                        double* __restrict__ work) {
    __shared__ double left[CHUNK][COLS];
    __shared__ double ring[RING][COLS];
    const unsigned lb = blockIdx.x % n_lb, cb = blockIdx.x / n_lb;
    const unsigned seg = blockIdx.y / n_tb, tb = blockIdx.y % n_tb;
    const size_t span = (n_lags - 1) * lag_step + 1;       // offsets 0 .. span-1 from lag0; requested: multiples of lag_step
    const size_t off_b = (size_t)lb * LAG_BLOCK;
    const size_t first_req = (off_b + lag_step - 1) / lag_step * lag_step;
    if (first_req >= off_b + LAG_BLOCK || first_req >= span) return;   // no requested lag in this block (uniform)

    const size_t N = seg_len;
    const size_t lag_b = lag0 + off_b;                      // <= a requested lag < N
    const size_t T0 = (size_t)tb * TIME_BLOCK;
    const size_t T1 = T0 + TIME_BLOCK < N ? T0 + TIME_BLOCK : N;
    const size_t t_end = T1 < N - lag_b ? T1 : N - lag_b;  // from here on every lag of the block pairs y_t with a zero
    const size_t n_chunks = t_end > T0 ? (t_end - T0 + CHUNK - 1) / CHUNK : 0;

    // staging role: series sc, rows sr, sr + 8, ...
    const int sc = threadIdx.x % COLS, sr = threadIdx.x / COLS;
    const size_t scol = (size_t)cb * COLS + sc;
    const bool live = scol < n_series;
    const double mu = live ? mean[(size_t)seg * n_series + scol] : 0.0;
    const double* xs = x + (size_t)seg * seg_stride * ld + (live ? scol : 0);
    // left operand: y_t for T0 <= t < t_end, zero past it (later times belong to the next time block or add nothing);
    // shifted operand: y_a for a < N, zero past the segment.  An out-of-range element is a load of chain_zero less a zero
    // mean: every load is issued unconditionally, so no branch holds one back and a stage's loads are in flight together.
    auto centred = [&](size_t a, size_t end) -> double {
        const bool in = live && a < end;
        return *(in ? xs + a * ld : &chain_zero) - (in ? mu : 0.0);
    };

    // ring slot of shifted row a = T0 + lag_b + i is i mod RING; slots 0 .. LAG_BLOCK-1 first (all loads, then the stores)
    {
        double v[LAG_BLOCK / STAGE_ROWS];
#pragma unroll
        for (int k = 0; k < LAG_BLOCK / STAGE_ROWS; ++k) v[k] = centred(T0 + lag_b + sr + k * STAGE_ROWS, N);
#pragma unroll
        for (int k = 0; k < LAG_BLOCK / STAGE_ROWS; ++k) ring[sr + k * STAGE_ROWS][sc] = v[k];
    }
    double pre_l[CHUNK / STAGE_ROWS], pre_r[CHUNK / STAGE_ROWS];
    auto fetch = [&](size_t ch) {
#pragma unroll
        for (int k = 0; k < CHUNK / STAGE_ROWS; ++k) {
            const size_t i = ch * CHUNK + sr + k * STAGE_ROWS;
            pre_l[k] = centred(T0 + i, t_end);
            pre_r[k] = centred(T0 + lag_b + LAG_BLOCK + i, N);
        }
    };
    if (n_chunks) fetch(0);
    __syncthreads();

    const int c = threadIdx.x % COLS, w = threadIdx.x / COLS;   // compute role: series c, lags lag_b + w*R + j
    double win[R], acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        win[j] = ring[w * R + j][c];
        acc[j] = 0.0;
    }
    for (size_t ch = 0; ch < n_chunks; ++ch) {
        __syncthreads();                                     // every lane is done with the previous stage
#pragma unroll
        for (int k = 0; k < CHUNK / STAGE_ROWS; ++k) {
            const int i = sr + k * STAGE_ROWS;
            left[i][sc] = pre_l[k];
            ring[(ch * CHUNK + LAG_BLOCK + i) % RING][sc] = pre_r[k];
        }
        __syncthreads();
        if (ch + 1 < n_chunks) fetch(ch + 1);                // in flight during the FMAs below
        for (int tt = 0; tt < CHUNK; tt += R) {
            // shifted rows t + l0 + R, t = T0 + ch*CHUNK + tt + k: ring slots base + k, never wrapping inside the group
            const int base = (int)((ch * CHUNK + tt + (size_t)(w + 1) * R) % RING);
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const double yt = left[tt + k][c];
#pragma unroll
                for (int j = 0; j < R; ++j) acc[j] = fma(yt, win[(k + j) % R], acc[j]);
                win[k] = ring[base + k][c];
            }
        }
    }

    const size_t col = (size_t)cb * COLS + c;
    if (col >= n_series) return;
    const size_t row0 = ((size_t)seg * n_tb + tb) * n_lags;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const size_t off = off_b + (size_t)w * R + j;
        if (off < span && off % lag_step == 0) work[(row0 + off / lag_step) * n_series + col] = acc[j];
    }
}

__global__ __launch_bounds__(REDUCE_THREADS) void chain_acov_reduce_kernel(size_t per_seg, size_t total, unsigned n_tb,
                                                                           size_t seg_len, const double* __restrict__ work,
                                                                           double* __restrict__ acov) {
    for (size_t i = (size_t)blockIdx.x * REDUCE_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * REDUCE_THREADS) {
        const size_t seg = i / per_seg, rem = i % per_seg;
        const double* p = work + seg * n_tb * per_seg + rem;
        double s = 0.0;
        for (unsigned b = 0; b < n_tb; ++b) s += p[(size_t)b * per_seg];
        acov[i] = s / (double)seg_len;
    }
}

}  // namespace

extern "C" int pem_chain_autocov_f64_dev(size_t n_rows, size_t n_series, size_t ld, const double* x, size_t n_seg, size_t seg_len,
                                         size_t seg_stride, size_t lag0, size_t lag_step, size_t n_lags, double* mean, double* acov,
                                         double* work, size_t work_len, pem_stream_t stream) {
    if (!n_rows || !n_series || !n_seg || !n_lags) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: zero size");
    if (ld < n_series) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: ld %zu < n_series %zu", ld, n_series);
    if (seg_len < 2 || seg_len > n_rows) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: need 2 <= seg_len <= n_rows");
    if (n_seg > 1 && seg_stride > (n_rows - seg_len) / (n_seg - 1))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: segment %zu runs past n_rows %zu", n_seg - 1, n_rows);
    if (!lag_step) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: lag_step 0");
    if (lag0 >= seg_len || n_lags - 1 > (seg_len - 1 - lag0) / lag_step)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: every lag must be < seg_len %zu", seg_len);
    if (!x || !mean || !acov || !work) return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: null pointer");
    const size_t n_tb = (seg_len + TIME_BLOCK - 1) / TIME_BLOCK;
    const size_t n_cb = (n_series + COLS - 1) / COLS;
    const size_t span = (n_lags - 1) * lag_step + 1;
    const size_t n_lb = (span + LAG_BLOCK - 1) / LAG_BLOCK;
    if (n_seg > 65535 || n_seg * n_tb > 65535 || n_cb > 0x7fffffffu / n_lb)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: problem too large for one launch");
    const size_t per_seg = n_lags * n_series;
    if (per_seg / n_series != n_lags || work_len / per_seg < n_seg * n_tb)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_chain_autocov: work_len %zu < n_seg * ceil(seg_len / %d) * n_lags * n_series",
                         work_len, TIME_BLOCK);
    if (int rc = pem::check_device()) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(chain_mean_kernel, dim3((unsigned)n_cb, (unsigned)n_seg), dim3(COLS * MEAN_GROUPS), 0, s, x, ld, n_series,
                       seg_len, seg_stride, mean);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(chain_acov_partial_kernel, dim3((unsigned)(n_lb * n_cb), (unsigned)(n_seg * n_tb)), dim3(THREADS), 0, s, x,
                       ld, n_series, seg_len, seg_stride, lag0, lag_step, n_lags, (unsigned)n_lb, (unsigned)n_tb, mean, work);
    HIP_TRY(hipGetLastError());
    const size_t total = n_seg * per_seg;
    const size_t blocks = (total + REDUCE_THREADS - 1) / REDUCE_THREADS;
    hipLaunchKernelGGL(chain_acov_reduce_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(REDUCE_THREADS), 0, s,
                       per_seg, total, (unsigned)n_tb, seg_len, work, acov);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
