// pem_powell.hip -- one function value of bounded Powell for many independent searches (hallthrusterpem_amd/optimize.py).
//
// What it stands in for: `minimize(obj_fun, x0, method='Powell', bounds=bds, options={'maxiter': maxfev, 'ftol': tol})` of
// run_mle (scripts/pem_v0/mcmc.py:170-231, optimizer='powell').  scipy's `_minimize_powell` with its bounded line search
// (`_linesearch_powell`, `_line_for_search`, `_minimize_scalar_bounded`) turned inside out: a launch takes the value of the
// point it emitted last, advances the algorithm until the next value is needed, and emits that point.  Powell's line searches
// are sequential, so one launch is one value per search; S searches share the posterior launch as its S rows.  The search
// runs over x in [lb, ub]^d of the prior's quantile cube and MAXIMISES f: g = -f is what scipy's comparisons see, a NaN f is
// g = +inf.  The row is handed to the posterior as theta = pem::transform(kind, a, b, x).
//
// One wave64 workgroup per search, lane j owns dimension j; every scalar of the algorithm is computed by all lanes alike, the
// only traffic between lanes is the max / min / any of `_line_for_search`.  The launch counter and all state live in device
// memory, so a captured graph replays the same kernel arguments and still advances.  Products and sums are rounded
// separately and there is no sum across dimensions, so tests/powell_np.py restates the launch bit for bit.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_philox.h"   // pem::transform, the prior transforms (no random numbers are drawn here)
#include "pem_search.h"

namespace {

constexpr int MAX_DIM = PEM_POWELL_MAX_DIM;
constexpr int STATE_WORDS = PEM_POWELL_STATE_WORDS;
constexpr int SCALARS = PEM_POWELL_SCALARS;
constexpr int VEC_ROWS = PEM_POWELL_VEC_ROWS;
constexpr uint64_t LINE_CAP = 500;   // maxiter of _minimize_scalar_bounded

// state words
enum { W_LAUNCHES, W_NIT, W_NFEV, W_STATUS, W_PHASE, W_I, W_BIGIND, W_NUM, W_LINES, W_GOLDEN, W_PARABOLIC, W_REJECTED, W_OFF_END,
       W_TOL1, W_CLIPPED, W_EXTRA, W_REPLACED, W_WORSE, W_ZERO_DIR, W_ZERO_DISP, W_DEGENERATE, W_ONE_EVAL, W_CAP, W_SPARE };
// rows of vec
enum { V_X, V_X1, V_P, V_XI, V_BEST_X, V_CAND };
// entries of scal
enum { C_A, C_B, C_FULC, C_NFC, C_XF, C_RAT, C_E, C_LFX, C_FFULC, C_FNFC, C_FU, C_XM, C_TOL1, C_TOL2, C_ALPHA, C_FX, C_FVAL, C_FX2,
       C_DELTA, C_BEST_F };
enum { PH_X0, PH_LINE, PH_EXTRAP, PH_EXTRA };
enum { BEGIN_ITER, START_LINE, LINE_DONE, END_ITER, EMIT };

static_assert(W_SPARE + 1 == STATE_WORDS && C_BEST_F + 1 == SCALARS && V_CAND + 1 == VEC_ROWS, "layout of include/pem_hip.h");

struct PowellTable {
    int32_t kind[MAX_DIM];
    double a[MAX_DIM], b[MAX_DIM], lb[MAX_DIM], ub[MAX_DIM];
};

using pem::search::clip;
using pem::search::cost;
using pem::search::transform_call;

__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// scipy's _line_for_search: the l with lb <= x0 + l alpha <= ub, over the non-zero components of alpha only.  false for an
// all-zero alpha.  Bounds that cross (or are not finite) become (0, 0).
__device__ __forceinline__ bool line_for_search(bool dim, double x0, double alpha, double lb, double ub, double& lmin,
                                                double& lmax) {
#pragma clang fp contract(off)
    const bool nz = dim && alpha != 0.0;
    if (__ballot(nz) == 0) return false;
    const double low = (lb - x0) / alpha, high = (ub - x0) / alpha;
    const bool pos = alpha > 0.0;
    const double lo = wave_max(nz ? (pos ? low + 0.0 : 0.0 + high) : -INFINITY);
    const double hi = wave_min(nz ? (pos ? high + 0.0 : 0.0 + low) : INFINITY);
    const bool ok = hi >= lo && finite(lo) && finite(hi);
    lmin = ok ? lo : 0.0;
    lmax = ok ? hi : 0.0;
    return true;
}

__global__ __launch_bounds__(64) void powell_step_kernel(int d, int finalize, double xtol, double ftol, uint64_t max_iter,
                                                         double sqrt_eps, double golden_mean, PowellTable tab,
                                                         double* __restrict__ vec, double* __restrict__ direc,
                                                         double* __restrict__ scal, const double* __restrict__ cand_f,
                                                         double* __restrict__ theta, uint64_t* __restrict__ state,
                                                         double* __restrict__ history, uint64_t history_len) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x, S = gridDim.x;
    const bool dim = lane < d;
    const int col = dim ? lane : 0;                  // lanes past d read column 0 and write nothing
    double* v = vec + s * VEC_ROWS * d;
    double* D = direc + s * (size_t)d * d;
    double* sc = scal + s * SCALARS;
    double* th = theta + s * d;
    uint64_t* st = state + s * STATE_WORDS;
    const uint64_t launches = st[W_LAUNCHES];
    const int kind = dim ? tab.kind[lane] : 0;
    const double pa = dim ? tab.a[lane] : 0.0, pb = dim ? tab.b[lane] : 0.0;
    const double lb = dim ? tab.lb[lane] : 0.0, ub = dim ? tab.ub[lane] : 0.0;

    if (finalize) {   // consumes nothing: the row is x, the point after the last completed line search (2: best_x)
        if (launches >= 1 && dim) th[lane] = transform_call(kind, pa, pb, v[(finalize == 2 ? V_BEST_X : V_X) * d + lane]);
        return;
    }
    if (launches == 0) {   // the uploaded start (already inside the bounds) is emitted
        if (dim) {
            const double x0 = v[V_X * d + lane];
#pragma unroll
            for (int r = 1; r < VEC_ROWS; ++r) v[r * d + lane] = x0;
            th[lane] = transform_call(kind, pa, pb, x0);
        }
        if (lane == 0) {
            for (int k = 0; k < SCALARS; ++k) sc[k] = k == C_BEST_F ? -INFINITY : 0.0;
            for (int w = 0; w < STATE_WORDS; ++w) st[w] = w == W_LAUNCHES ? 1 : 0;   // phase PH_X0
        }
        return;
    }
    if (st[W_STATUS] != 0) {   // frozen: its row of theta is x already; only the launch counter and the history move
        if (lane == 0) {
            st[W_LAUNCHES] = launches + 1;
            if (history && launches - 1 < history_len) history[(launches - 1) * S + s] = sc[C_BEST_F];
        }
        return;
    }

    uint64_t w[STATE_WORDS];
    double c[SCALARS];
#pragma unroll
    for (int k = 0; k < STATE_WORDS; ++k) w[k] = st[k];
#pragma unroll
    for (int k = 0; k < SCALARS; ++k) c[k] = sc[k];
    double x = v[V_X * d + col], x1 = v[V_X1 * d + col], p = v[V_P * d + col], xi = v[V_XI * d + col];
    double best_x = v[V_BEST_X * d + col], cand = v[V_CAND * d + col];
    const double xatol = (xtol * 100.0) / 100.0;     // _minimize_powell passes xtol * 100, _linesearch_powell tol / 100
    const double g = cost(cand_f[s]);
    int phase = (int)w[W_PHASE], todo;
    const uint64_t last = (uint64_t)(d - 1);         // i and bigind index direc: a state the caller has overwritten stays in bounds

    w[W_NFEV] += 1;
    if (launches == 1 || g < -c[C_BEST_F]) {
        c[C_BEST_F] = -g;
        best_x = cand;
    }

    if (phase == PH_X0) {
        c[C_FVAL] = g;
        todo = BEGIN_ITER;
    } else if (phase == PH_EXTRAP) {
        c[C_FX2] = g;
        const double fx = c[C_FX], fx2 = g, fval = c[C_FVAL], delta = c[C_DELTA];
        todo = BEGIN_ITER;
        if (fx > fx2) {
            double t = 2.0 * (fx + fx2 - 2.0 * fval);
            double temp = fx - fval - delta;
            t = t * (temp * temp);
            temp = fx - fx2;
            t = t - delta * temp * temp;
            if (t < 0.0) {
                phase = PH_EXTRA;
                w[W_EXTRA] += 1;
                todo = START_LINE;
            }
        }
    } else {   // a value of the line search in progress: scipy's _minimize_scalar_bounded from where it waited
        double a = c[C_A], b = c[C_B], fulc = c[C_FULC], nfc = c[C_NFC], xf = c[C_XF], lfx = c[C_LFX], ffulc = c[C_FFULC],
               fnfc = c[C_FNFC], al = c[C_ALPHA];
        bool capped = false;
        if (w[W_NUM] == 0) {
            lfx = g;
            w[W_NUM] = 1;
            c[C_FU] = INFINITY;
            ffulc = fnfc = lfx;
        } else {
            const double fu = g;
            c[C_FU] = fu;
            w[W_NUM] += 1;
            if (fu <= lfx) {
                if (al >= xf) a = xf; else b = xf;
                fulc = nfc, ffulc = fnfc;
                nfc = xf, fnfc = lfx;
                xf = al, lfx = fu;
            } else {
                if (al < xf) a = al; else b = al;
                if (fu <= fnfc || nfc == xf) {
                    fulc = nfc, ffulc = fnfc;
                    nfc = al, fnfc = fu;
                } else if (fu <= ffulc || fulc == xf || fulc == nfc) {
                    fulc = al, ffulc = fu;
                }
            }
            capped = w[W_NUM] >= LINE_CAP;
        }
        const double xm = 0.5 * (a + b);
        const double tol1 = sqrt_eps * fabs(xf) + xatol / 3.0;
        const double tol2 = 2.0 * tol1;
        c[C_A] = a, c[C_B] = b, c[C_FULC] = fulc, c[C_NFC] = nfc, c[C_XF] = xf, c[C_LFX] = lfx, c[C_FFULC] = ffulc, c[C_FNFC] = fnfc;
        c[C_XM] = xm, c[C_TOL1] = tol1, c[C_TOL2] = tol2;
        if (capped) {
            w[W_CAP] += 1;
            todo = LINE_DONE;
        } else if (fabs(xf - xm) > (tol2 - 0.5 * (b - a))) {
            bool golden = true;
            double e = c[C_E], rat = c[C_RAT];
            if (fabs(e) > tol1) {   // a parabolic fit
                golden = false;
                double r = (xf - nfc) * (lfx - ffulc);
                double q = (xf - fulc) * (lfx - fnfc);
                double pp = (xf - fulc) * q - (xf - nfc) * r;
                q = 2.0 * (q - r);
                if (q > 0.0) pp = -pp;
                q = fabs(q);
                r = e;
                e = rat;
                const double stepv = pp / q;
                if (fabs(pp) < fabs(0.5 * q * r) && pp > q * (a - xf) && pp < q * (b - xf) && finite(pp) && finite(q) &&
                    finite(stepv)) {
                    rat = (pp + 0.0) / q;
                    const double xn = xf + rat;
                    w[W_PARABOLIC] += 1;
                    if ((xn - a) < tol2 || (b - xn) < tol2) {   // moved off an interval end
                        const double dm = xm - xf;
                        rat = tol1 * (dm < 0.0 ? -1.0 : 1.0);
                        w[W_OFF_END] += 1;
                    }
                } else {
                    golden = true;
                    w[W_REJECTED] += 1;
                }
            }
            if (golden) {
                e = xf >= xm ? a - xf : b - xf;
                rat = golden_mean * e;
                w[W_GOLDEN] += 1;
            }
            const double si = rat < 0.0 ? -1.0 : 1.0;   // sign(rat) + (rat == 0)
            if (fabs(rat) < tol1) w[W_TOL1] += 1;
            al = xf + si * fmax(fabs(rat), tol1);
            c[C_E] = e, c[C_RAT] = rat, c[C_ALPHA] = al;
            cand = clip(p + al * xi, lb, ub);
            todo = EMIT;
        } else {
            todo = LINE_DONE;
        }
    }

    // transitions that need no value: at most d + 2 of them before a point is emitted or the search ends
    while (todo != EMIT && w[W_STATUS] == 0) {
        if (todo == BEGIN_ITER) {
            c[C_FX] = c[C_FVAL];
            w[W_BIGIND] = 0;
            c[C_DELTA] = 0.0;
            w[W_I] = 0;
            phase = PH_LINE;
            todo = START_LINE;
        } else if (todo == START_LINE) {
            if (phase == PH_LINE) {
                xi = D[(w[W_I] < last ? w[W_I] : last) * d + col];
                c[C_FX2] = c[C_FVAL];
            }
            p = x;
            double lmin, lmax;
            if (!line_for_search(dim, p, xi, lb, ub, lmin, lmax)) {   // a zero direction is not searched
                w[W_ZERO_DIR] += 1;
                if (phase == PH_LINE) {
                    w[W_I] += 1;
                    todo = w[W_I] < (uint64_t)d ? START_LINE : END_ITER;
                } else {
                    todo = BEGIN_ITER;
                }
                continue;
            }
            w[W_LINES] += 1;
            if (!(lmax > lmin)) w[W_DEGENERATE] += 1;
            const double fulc = lmin + golden_mean * (lmax - lmin);
            c[C_A] = lmin, c[C_B] = lmax, c[C_FULC] = fulc, c[C_NFC] = fulc, c[C_XF] = fulc, c[C_RAT] = 0.0, c[C_E] = 0.0;
            c[C_ALPHA] = fulc;
            w[W_NUM] = 0;
            cand = clip(p + fulc * xi, lb, ub);
            todo = EMIT;
        } else if (todo == LINE_DONE) {
            if (w[W_NUM] == 1) w[W_ONE_EVAL] += 1;
            const double stepv = c[C_XF] * xi;
            x = clip(p + stepv, lb, ub);
            if (c[C_LFX] > c[C_FVAL]) w[W_WORSE] += 1;
            c[C_FVAL] = c[C_LFX];
            if (phase == PH_LINE) {
                if ((c[C_FX2] - c[C_FVAL]) > c[C_DELTA]) {
                    c[C_DELTA] = c[C_FX2] - c[C_FVAL];
                    w[W_BIGIND] = w[W_I];
                }
                w[W_I] += 1;
                todo = w[W_I] < (uint64_t)d ? START_LINE : END_ITER;
            } else {
                if (__ballot(dim && stepv != 0.0) != 0) {   // the displacement replaces the direction of the largest decrease
                    if (dim) {
                        D[(w[W_BIGIND] < last ? w[W_BIGIND] : last) * d + lane] = D[(size_t)(d - 1) * d + lane];
                        D[(size_t)(d - 1) * d + lane] = stepv;
                    }
                    w[W_REPLACED] += 1;
                }
                todo = BEGIN_ITER;
            }
        } else {   // END_ITER
            w[W_NIT] += 1;
            const double fx = c[C_FX], fval = c[C_FVAL];
            const double bnd = ftol * (fabs(fx) + fabs(fval)) + 1e-20;
            if (2.0 * (fx - fval) <= bnd) {
                w[W_STATUS] = 1;
            } else if (max_iter != 0 && w[W_NIT] >= max_iter) {
                w[W_STATUS] = 2;
            } else {   // the extrapolated point, kept inside the bounds
                const double direc1 = x - x1;
                x1 = x;
                double lmin, lmax;
                if (!line_for_search(dim, x, direc1, lb, ub, lmin, lmax)) {
                    w[W_ZERO_DISP] += 1;
                    lmax = 1.0;
                }
                if (lmax < 1.0) w[W_CLIPPED] += 1;
                xi = direc1;
                cand = clip(x + (lmax < 1.0 ? lmax : 1.0) * direc1, lb, ub);
                phase = PH_EXTRAP;
                todo = EMIT;
            }
        }
    }
    w[W_PHASE] = (uint64_t)phase;
    if (w[W_STATUS] != 0) cand = x;
    w[W_LAUNCHES] = launches + 1;

    if (dim) {
        v[V_X * d + lane] = x;
        v[V_X1 * d + lane] = x1;
        v[V_P * d + lane] = p;
        v[V_XI * d + lane] = xi;
        v[V_BEST_X * d + lane] = best_x;
        v[V_CAND * d + lane] = cand;
        th[lane] = transform_call(kind, pa, pb, cand);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < STATE_WORDS; ++k) st[k] = w[k];
#pragma unroll
        for (int k = 0; k < SCALARS; ++k) sc[k] = c[k];
        if (history && launches - 1 < history_len) history[(launches - 1) * S + s] = c[C_BEST_F];
    }
}

}  // namespace

extern "C" int pem_powell_step_f64_dev(size_t n_search, int ndim, int finalize, double xtol, double ftol, uint64_t max_iter,
                                       double sqrt_eps, double golden_mean, const int32_t* kind, const double* a, const double* b,
                                       const double* lb, const double* ub, double* vec, double* direc, double* scal,
                                       const double* cand_f, double* theta, uint64_t* state, double* history, size_t history_len,
                                       pem_stream_t stream) {
    if (n_search == 0 || n_search > (size_t)INT_MAX)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: n_search must be in [1, %d]", INT_MAX);
    if (ndim < 1 || ndim > MAX_DIM) return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: ndim must be in [1, %d]", MAX_DIM);
    if (finalize < 0 || finalize > 2) return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: finalize must be 0, 1 or 2");
    if (!(xtol >= 0.0) || !(ftol >= 0.0)) return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: xtol and ftol must be >= 0");
    if (!(sqrt_eps > 0.0 && sqrt_eps < 1.0) || !(golden_mean > 0.0 && golden_mean < 1.0))
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: sqrt_eps and golden_mean must be in (0, 1)");
    if (!kind || !a || !b || !lb || !ub || !vec || !direc || !scal || !cand_f || !theta || !state)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: NULL array");
    if (history && history_len == 0)
        return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: a history needs history_len >= 1");
    PowellTable tab;
    for (int j = 0; j < MAX_DIM; ++j) {
        tab.kind[j] = j < ndim ? kind[j] : 0;
        tab.a[j] = j < ndim ? a[j] : 0.0;
        tab.b[j] = j < ndim ? b[j] : 0.0;
        tab.lb[j] = j < ndim ? lb[j] : 0.0;
        tab.ub[j] = j < ndim ? ub[j] : 0.0;
        if (j < ndim && (kind[j] < 0 || kind[j] > PEM_DIST_NORMAL))
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: unknown distribution kind %d for dimension %d", kind[j], j);
        if (j < ndim && !(lb[j] <= ub[j]))
            return pem::fail(PEM_ERR_INVALID_ARG, "pem_powell_step: lb > ub (or NaN) for dimension %d", j);
    }
    if (int rc = pem::check_device()) return rc;
    hipLaunchKernelGGL(powell_step_kernel, dim3((unsigned)n_search), dim3(64), 0, static_cast<hipStream_t>(stream), ndim,
                       finalize, xtol, ftol, max_iter, sqrt_eps, golden_mean, tab, vec, direc, scal, cand_f, theta, state,
                       history, (uint64_t)history_len);
    HIP_TRY(hipGetLastError());
    return PEM_OK;
}
