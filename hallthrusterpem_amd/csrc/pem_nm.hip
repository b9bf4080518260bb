// pem_nm.hip -- one iteration of bounded Nelder-Mead for many independent simplices (hallthrusterpem_amd/optimize.py).
//
// What it stands in for: `minimize(obj_fun, x0, method='Nelder-Mead', bounds=bds, tol=1e-4, options={'adaptive': True})` of
// run_mle (scripts/pem_v0/mcmc.py:170-231, the default optimizer).  scipy's `_minimize_neldermead`, restated so that no
// function value is waited for: every point an iteration can ask for -- the reflection, the expansion, the outside and the
// inside contraction and the d shrunk vertices -- is emitted before the iteration starts, the caller evaluates all d + 4 rows
// in one posterior launch, and the next launch of this kernel takes scipy's decisions from those values.  The search runs
// over x in [lb, ub]^d of the prior's quantile cube and MAXIMISES f: g = -f is what scipy's comparisons see, a NaN f is
// g = +inf.  The rows are handed to the posterior as theta = pem::transform(kind, a, b, x).
//
// One wave64 workgroup per simplex, lane j owns dimension j, the (d + 1) x d simplex sits in LDS.  The launch counter lives
// in device memory (`state`), so a captured graph replays the same kernel arguments and still advances.  Products and sums
// are rounded separately and every sum has a fixed order, so tests/nm_np.py restates the launch bit for bit.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_philox.h"   // pem::transform, the prior transforms (no random numbers are drawn here)
#include "pem_search.h"

namespace {

constexpr int MAX_DIM = PEM_NM_MAX_DIM;
constexpr int MAX_VERT = MAX_DIM + 1;
constexpr int STATE_WORDS = PEM_NM_STATE_WORDS;

// the code of an iteration's operation (state word 9); its count is state word 3 + code
constexpr int OP_NONE = 0, OP_REFLECT = 1, OP_EXPAND = 2, OP_OUTSIDE = 3, OP_INSIDE = 4, OP_SHRINK = 5;

struct NmTable {
    int32_t kind[MAX_DIM];
    double a[MAX_DIM], b[MAX_DIM], lb[MAX_DIM], ub[MAX_DIM];
};

using pem::search::clip;
using pem::search::cost;
using pem::search::transform_call;

// |diff| <= tol as scipy's `np.max(np.abs(...)) <= tol` decides it for one entry: NaN and inf are "not converged"
__device__ __forceinline__ bool within(double diff, double tol) {
    const double v = fabs(diff);
    return v < INFINITY && v <= tol;
}

__global__ __launch_bounds__(64) void nm_step_kernel(int d, int finalize, double rho, double chi, double psi, double sigma,
                                                     double xatol, double fatol, NmTable tab, double* __restrict__ sim,
                                                     double* __restrict__ fsim, double* __restrict__ cand_x,
                                                     const double* __restrict__ cand_f, double* __restrict__ theta,
                                                     uint64_t* __restrict__ state, double* __restrict__ history,
                                                     uint64_t history_len) {
#pragma clang fp contract(off)
    __shared__ double s_sim[MAX_VERT][MAX_DIM], s_new[MAX_VERT][MAX_DIM];
    __shared__ double s_g[MAX_VERT], s_gn[MAX_VERT];
    __shared__ int s_rank[MAX_VERT], s_ok[MAX_VERT];
    const int lane = threadIdx.x, nv = d + 1, nc = d + 4;
    const size_t s = blockIdx.x, S = gridDim.x;
    const bool dim = lane < d, vert = lane < nv;
    double* sim_s = sim + s * nv * d;
    double* fsim_s = fsim + s * nv;
    double* cx = cand_x + s * nc * d;
    const double* cf = cand_f + s * nc;
    double* th = theta + s * nc * d;
    uint64_t* st = state + s * STATE_WORDS;
    const uint64_t launches = st[0];
    const int kind = dim ? tab.kind[lane] : 0;
    const double pa = dim ? tab.a[lane] : 0.0, pb = dim ? tab.b[lane] : 0.0;
    const double lb = dim ? tab.lb[lane] : 0.0, ub = dim ? tab.ub[lane] : 0.0;

    if (launches == 0) {   // the uploaded simplex: rows 0 ... d are its vertices, rows d + 1 ... d + 3 repeat vertex 0
        if (finalize) return;
        if (dim) {
            for (int r = 0; r < nc; ++r) {
                const double x = sim_s[(size_t)(r < nv ? r : 0) * d + lane];
                cx[(size_t)r * d + lane] = x;
                th[(size_t)r * d + lane] = transform_call(kind, pa, pb, x);
            }
        }
        if (lane == 0) {
            st[0] = 1;
            for (int w = 1; w < STATE_WORDS; ++w) st[w] = 0;
        }
        return;
    }

    uint64_t nit = st[1], nfev = st[2], status = st[3];
    int op = OP_NONE;
    double best_g, x0 = 0.0;
    if (status != 0) {   // frozen: nothing but the launch counter and the history moves
        best_g = -fsim_s[0];
        if (dim) x0 = sim_s[lane];
    } else {
        if (dim)
            for (int i = 0; i < nv; ++i) s_sim[i][lane] = sim_s[(size_t)i * d + lane];
        if (vert) s_g[lane] = launches == 1 ? cost(cf[lane]) : -fsim_s[lane];
        __syncthreads();
        if (launches == 1) {   // the values of the uploaded vertices
            nit = 1;
            nfev = (uint64_t)nv;
        } else {               // scipy's decision tree, from the row values instead of from calls
            const double gr = cost(cf[0]), ge = cost(cf[1]), gc = cost(cf[2]), gcc = cost(cf[3]);
            const double g_best = s_g[0], g_second = s_g[d - 1], g_worst = s_g[d];
            int take = -1;
            if (gr < g_best) {
                nfev += 2;
                take = ge < gr ? 1 : 0;
                op = ge < gr ? OP_EXPAND : OP_REFLECT;
            } else if (gr < g_second) {
                nfev += 1;
                take = 0;
                op = OP_REFLECT;
            } else if (gr < g_worst) {
                nfev += 2;
                if (gc <= gr) {
                    take = 2;
                    op = OP_OUTSIDE;
                }
            } else {
                nfev += 2;
                if (gcc < g_worst) {
                    take = 3;
                    op = OP_INSIDE;
                }
            }
            __syncthreads();   // every lane has read s_g before it changes
            if (take >= 0) {
                if (dim) s_sim[d][lane] = cx[(size_t)take * d + lane];
                if (lane == 0) s_g[d] = cost(cf[take]);
            } else {
                op = OP_SHRINK;
                nfev += (uint64_t)d;
                if (dim)
                    for (int i = 1; i < nv; ++i) s_sim[i][lane] = cx[(size_t)(3 + i) * d + lane];
                if (vert && lane >= 1) s_g[lane] = cost(cf[3 + lane]);
            }
            nit += 1;
            __syncthreads();
        }

        // stable sort, best (smallest g) first: rank of vertex i = #{j : g_j < g_i or (g_j == g_i and j < i)}
        if (vert) {
            const double gi = s_g[lane];
            int rank = 0;
            for (int j = 0; j < nv; ++j) {
                const double gj = s_g[j];
                rank += (gj < gi || (gj == gi && j < lane)) ? 1 : 0;
            }
            s_rank[lane] = rank;
            s_gn[rank] = gi;
        }
        __syncthreads();
        if (dim)
            for (int i = 0; i < nv; ++i) s_new[s_rank[i]][lane] = s_sim[i][lane];
        __syncthreads();
        if (dim)
            for (int i = 0; i < nv; ++i) sim_s[(size_t)i * d + lane] = s_new[i][lane];
        if (vert) fsim_s[lane] = -s_gn[lane];

        // scipy's convergence test, before any candidate is emitted
        if (vert) {
            bool ok = true;
            if (dim)
                for (int i = 1; i < nv; ++i) ok = ok && within(s_new[i][lane] - s_new[0][lane], xatol);
            if (lane >= 1) ok = ok && within(s_gn[0] - s_gn[lane], fatol);
            s_ok[lane] = ok ? 1 : 0;
        }
        __syncthreads();
        int all_ok = 1;
        for (int i = 0; i < nv; ++i) all_ok &= s_ok[i];
        status = all_ok ? 1 : 0;
        best_g = s_gn[0];
        if (dim) x0 = s_new[0][lane];

        if (status == 0 && !finalize && dim) {   // the d + 4 points the next iteration can ask for
            double xbar = s_new[0][lane];
            for (int i = 1; i < d; ++i) xbar = xbar + s_new[i][lane];
            xbar = xbar / (double)d;
            const double worst = s_new[d][lane];
            const double rc = rho * chi, pr = psi * rho;
            double pts[4];
            pts[0] = (1.0 + rho) * xbar - rho * worst;
            pts[1] = (1.0 + rc) * xbar - rc * worst;
            pts[2] = (1.0 + pr) * xbar - pr * worst;
            pts[3] = (1.0 - psi) * xbar + psi * worst;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double x = clip(pts[r], lb, ub);
                cx[(size_t)r * d + lane] = x;
                th[(size_t)r * d + lane] = transform_call(kind, pa, pb, x);
            }
            for (int i = 1; i < nv; ++i) {
                const double x = clip(x0 + sigma * (s_new[i][lane] - x0), lb, ub);
                cx[(size_t)(3 + i) * d + lane] = x;
                th[(size_t)(3 + i) * d + lane] = transform_call(kind, pa, pb, x);
            }
        }
    }

    if (finalize && dim) {   // every row of the simplex's block of theta is its best vertex
        const double t = transform_call(kind, pa, pb, x0);
        for (int r = 0; r < nc; ++r) th[(size_t)r * d + lane] = t;
    }
    if (lane == 0) {
        if (!finalize) st[0] = launches + 1;
        st[1] = nit;
        st[2] = nfev;
        st[3] = status;
        if (op != OP_NONE) {
            st[3 + op] += 1;
            st[9] = (uint64_t)op;
        }
        if (history && launches - 1 < history_len) history[(launches - 1) * S + s] = -best_g;
    }
}

}  // namespace

extern "C" int pem_nm_step_f64_dev(size_t n_simplex, int ndim, int finalize, double rho, double chi, double psi, double sigma,
                                   double xatol, double fatol, const int32_t* kind, const double* a, const double* b,
                                   const double* lb, const double* ub, double* sim, double* fsim, double* cand_x,
                                   const double* cand_f, double* theta, uint64_t* state, double* history, size_t history_len,
                                   pem_stream_t stream) {
    if (n_simplex == 0 || n_simplex > (size_t)INT_MAX)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_nm_step: n_simplex must be in [1, %d]", INT_MAX);
    if (ndim < 1 || ndim > MAX_DIM) return pem::fail(PEM_ERR_INVALID_ARG, "pem_nm_step: ndim must be in [1, %d]", MAX_DIM);
    if (!(xatol >= 0.0) || !(fatol >= 0.0))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_nm_step: xatol and fatol must be >= 0");
    if (!kind || !a || !b || !lb || !ub || !sim || !fsim || !cand_x || !cand_f || !theta || !state)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_nm_step: NULL array");
    if (history && history_len == 0) return pem::fail(PEM_ERR_INVALID_ARG, "pem_nm_step: a history needs history_len >= 1");
    NmTable tab;
    for (int j = 0; j < MAX_DIM; ++j) {
        tab.kind[j] = j < ndim ? kind[j] : 0;
        tab.a[j] = j < ndim ? a[j] : 0.0;
        tab.b[j] = j < ndim ? b[j] : 0.0;
        tab.lb[j] = j < ndim ? lb[j] : 0.0;
        tab.ub[j] = j < ndim ? ub[j] : 0.0;
        if (j < ndim && (kind[j] < 0 || kind[j] > PEM_DIST_NORMAL))
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_nm_step: unknown distribution kind %d for dimension %d", kind[j], j);
        if (j < ndim && !(lb[j] <= ub[j]))
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_nm_step: lb > ub (or NaN) for dimension %d", j);
    }
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(nm_step_kernel, dim3((unsigned)n_simplex), dim3(64), 0, static_cast<hipStream_t>(stream), ndim,
                       finalize ? 1 : 0, rho, chi, psi, sigma, xatol, fatol, tab, sim, fsim, cand_x, cand_f, theta, state,
                       history, (uint64_t)history_len);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
