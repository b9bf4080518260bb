"""numpy restatement of one `pem_powell_step_f64_dev` launch (csrc/pem_powell.hip): scipy's `_minimize_powell` with bounds
(`_linesearch_powell`, `_line_for_search`, `_minimize_scalar_bounded`) turned inside out, one function value in and one point
out per launch, the same IEEE operations in the same order, so that the state words, the vectors, the direction set, the
scalars and the history compare bit for bit.  `minimize` drives ONE search to completion with a Python f.  It is the
definition the kernel is held to.  TEST INFRASTRUCTURE ONLY.

Where it is scipy and where it is not.  Against scipy 1.15.3 every evaluated point, x, fun, nit, nfev and direc are equal bit
for bit (tests/test_powell_host.py).  scipy's behaviour is left in three places, none of which a finite function on a box
with a start inside it reaches unless rounding carries a point one ulp past a bound:
  * an all-zero displacement x - x1: scipy raises on an empty max; here lmax = 1, so the extrapolated point is x;
  * a parabola whose p, q or step p / q is not finite (values of +-inf): the golden step is taken;
  * every emitted point, and x after a line search, is min(max(., lb), ub); a line whose bounds are not finite (a direction
    with a denormal component) is searched over (0, 0), like one whose bounds cross.
"""
import math

import numpy as np

from oracle import sampler_np as snp

# state words
(LAUNCHES, NIT, NFEV, STATUS, PHASE, I, BIGIND, NUM, N_LINES, N_GOLDEN, N_PARABOLIC, N_REJECTED, N_OFF_END, N_TOL1, N_CLIPPED,
 N_EXTRA, N_REPLACED, N_WORSE, N_ZERO_DIR, N_ZERO_DISP, N_DEGENERATE, N_ONE_EVAL, N_CAP, _SPARE) = range(24)
STATE_WORDS = 24
COUNTERS = ('lines', 'golden', 'parabolic', 'rejected', 'off_end', 'tol1', 'clipped', 'extra', 'replaced', 'worse', 'zero_dir',
            'zero_disp', 'degenerate', 'one_eval', 'cap')
TABLE = ('golden', 'parabolic', 'rejected', 'off_end', 'tol1', 'clipped', 'extra', 'replaced', 'worse')   # met by real functions
# rows of vec (S, 6, d)
X, X1, P, XI, BEST_X, CAND = range(6)
VEC_ROWS = 6
# entries of scal (S, 20)
A, B, FULC, NFC, XF, RAT, E, LFX, FFULC, FNFC, FU, XM, TOL1, TOL2, ALPHA, FX, FVAL, FX2, DELTA, BEST_F = range(20)
SCALARS = 20
# phases
PH_X0, PH_LINE, PH_EXTRAP, PH_EXTRA = range(4)
RUNNING, FTOL, MAX_ITER = 0, 1, 2
LINE_CAP = 500                                      # _minimize_scalar_bounded's maxiter

SQRT_EPS = math.sqrt(2.2e-16)
GOLDEN_MEAN = 0.5 * (3.0 - math.sqrt(5.0))
UNBOUNDED = 0                                       # max_iter: no limit


def cost(f):
    """g = -f, a NaN f is +inf"""
    f = float(f)
    return math.inf if f != f else -f


def transform(kind, a, b, x):
    """theta of rows x (..., d)"""
    return np.stack([snp.transform(kind[j], a[j], b[j], x[..., j]) for j in range(x.shape[-1])], axis=-1)


def line_for_search(x0, alpha, lb, ub):
    """scipy's `_line_for_search`; None for an all-zero alpha (scipy is never asked)"""
    nz = alpha != 0
    if not nz.any():
        return None
    with np.errstate(over='ignore'):
        low = (lb[nz] - x0[nz]) / alpha[nz]
        high = (ub[nz] - x0[nz]) / alpha[nz]
    pos = alpha[nz] > 0
    lmin = np.max(np.where(pos, low, 0) + np.where(pos, 0, high))
    lmax = np.min(np.where(pos, high, 0) + np.where(pos, 0, low))
    if lmax >= lmin and np.isfinite(lmin) and np.isfinite(lmax):
        return float(lmin), float(lmax)
    return 0.0, 0.0


def _clip(x, lb, ub):
    return np.minimum(np.maximum(x, lb), ub)


def _advance(g, xtol, ftol, max_iter, lb, ub, v, D, c, st):
    """one search, one value: v (6, d), D (d, d), c (20,), st (24,) are changed in place; leaves the next point in v[CAND]"""
    d = v.shape[1]
    xatol = (xtol * 100) / 100
    BEGIN_ITER, START_LINE, LINE_DONE, END_ITER, EMIT = range(5)
    phase = int(st[PHASE])

    st[NFEV] += 1
    if int(st[LAUNCHES]) == 1 or g < -c[BEST_F]:
        c[BEST_F] = -g
        v[BEST_X] = v[CAND]

    if phase == PH_X0:
        c[FVAL] = g
        todo = BEGIN_ITER
    elif phase == PH_EXTRAP:
        c[FX2] = g
        fx, fx2, fval, delta = c[FX], c[FX2], c[FVAL], c[DELTA]
        todo = BEGIN_ITER
        if fx > fx2:
            t = 2.0 * (fx + fx2 - 2.0 * fval)
            temp = fx - fval - delta
            t = t * (temp * temp)
            temp = fx - fx2
            t = t - delta * temp * temp
            if t < 0.0:
                phase = PH_EXTRA
                st[N_EXTRA] += 1
                todo = START_LINE
    else:                                            # a value of the line search in progress
        a, b, fulc, nfc, xf, lfx, ffulc, fnfc, x = c[A], c[B], c[FULC], c[NFC], c[XF], c[LFX], c[FFULC], c[FNFC], c[ALPHA]
        capped = False
        if st[NUM] == 0:
            lfx = g
            st[NUM] = 1
            c[FU] = math.inf
            ffulc = fnfc = lfx
        else:
            fu = g
            c[FU] = fu
            st[NUM] += 1
            if fu <= lfx:
                if x >= xf:
                    a = xf
                else:
                    b = xf
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = xf, lfx
                xf, lfx = x, fu
            else:
                if x < xf:
                    a = x
                else:
                    b = x
                if fu <= fnfc or nfc == xf:
                    fulc, ffulc = nfc, fnfc
                    nfc, fnfc = x, fu
                elif fu <= ffulc or fulc == xf or fulc == nfc:
                    fulc, ffulc = x, fu
            capped = st[NUM] >= LINE_CAP
        xm = 0.5 * (a + b)
        tol1 = SQRT_EPS * abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        c[A], c[B], c[FULC], c[NFC], c[XF], c[LFX], c[FFULC], c[FNFC] = a, b, fulc, nfc, xf, lfx, ffulc, fnfc
        c[XM], c[TOL1], c[TOL2] = xm, tol1, tol2
        if capped:
            st[N_CAP] += 1
            todo = LINE_DONE
        elif abs(xf - xm) > (tol2 - 0.5 * (b - a)):
            golden = True
            e, rat = c[E], c[RAT]
            if abs(e) > tol1:
                golden = False
                r = (xf - nfc) * (lfx - ffulc)
                q = (xf - fulc) * (lfx - fnfc)
                p = (xf - fulc) * q - (xf - nfc) * r
                q = 2.0 * (q - r)
                if q > 0.0:
                    p = -p
                q = abs(q)
                r = e
                e = rat
                step = p / q if q != 0.0 else math.nan
                if (abs(p) < abs(0.5 * q * r) and p > q * (a - xf) and p < q * (b - xf)
                        and math.isfinite(p) and math.isfinite(q) and math.isfinite(step)):
                    rat = (p + 0.0) / q
                    x = xf + rat
                    st[N_PARABOLIC] += 1
                    if (x - a) < tol2 or (b - x) < tol2:
                        si = (1.0 if xm - xf > 0 else -1.0 if xm - xf < 0 else 0.0) + (1.0 if xm - xf == 0 else 0.0)
                        rat = tol1 * si
                        st[N_OFF_END] += 1
                else:
                    golden = True
                    st[N_REJECTED] += 1
            if golden:
                e = a - xf if xf >= xm else b - xf
                rat = GOLDEN_MEAN * e
                st[N_GOLDEN] += 1
            si = (1.0 if rat > 0 else -1.0 if rat < 0 else 0.0) + (1.0 if rat == 0 else 0.0)
            if abs(rat) < tol1:
                st[N_TOL1] += 1
            x = xf + si * max(abs(rat), tol1)
            c[E], c[RAT], c[ALPHA] = e, rat, x
            v[CAND] = _clip(v[P] + x * v[XI], lb, ub)
            todo = EMIT
        else:
            todo = LINE_DONE

    while todo != EMIT and st[STATUS] == RUNNING:
        if todo == BEGIN_ITER:
            c[FX] = c[FVAL]
            st[BIGIND] = 0
            c[DELTA] = 0.0
            st[I] = 0
            phase = PH_LINE
            todo = START_LINE
        elif todo == START_LINE:
            if phase == PH_LINE:
                v[XI] = D[int(st[I])]
                c[FX2] = c[FVAL]
            v[P] = v[X]
            bound = line_for_search(v[P], v[XI], lb, ub)
            if bound is None:                        # a zero direction is not searched
                st[N_ZERO_DIR] += 1
                if phase == PH_LINE:
                    st[I] += 1
                    todo = START_LINE if st[I] < d else END_ITER
                else:
                    todo = BEGIN_ITER
                continue
            st[N_LINES] += 1
            a, b = bound
            if not b > a:
                st[N_DEGENERATE] += 1
            fulc = a + GOLDEN_MEAN * (b - a)
            c[A], c[B], c[FULC], c[NFC], c[XF], c[RAT], c[E], c[ALPHA] = a, b, fulc, fulc, fulc, 0.0, 0.0, fulc
            st[NUM] = 0
            v[CAND] = _clip(v[P] + fulc * v[XI], lb, ub)
            todo = EMIT
        elif todo == LINE_DONE:
            if st[NUM] == 1:
                st[N_ONE_EVAL] += 1
            step = c[XF] * v[XI]
            v[X] = _clip(v[P] + step, lb, ub)
            if c[LFX] > c[FVAL]:
                st[N_WORSE] += 1
            c[FVAL] = c[LFX]
            if phase == PH_LINE:
                if (c[FX2] - c[FVAL]) > c[DELTA]:
                    c[DELTA] = c[FX2] - c[FVAL]
                    st[BIGIND] = st[I]
                st[I] += 1
                todo = START_LINE if st[I] < d else END_ITER
            else:
                if step.any():
                    D[int(st[BIGIND])] = D[d - 1]
                    D[d - 1] = step
                    st[N_REPLACED] += 1
                todo = BEGIN_ITER
        else:                                        # END_ITER
            st[NIT] += 1
            fx, fval = c[FX], c[FVAL]
            bnd = ftol * (abs(fx) + abs(fval)) + 1e-20
            if 2.0 * (fx - fval) <= bnd:
                st[STATUS] = FTOL
            elif max_iter != UNBOUNDED and st[NIT] >= max_iter:
                st[STATUS] = MAX_ITER
            else:
                direc1 = v[X] - v[X1]
                v[X1] = v[X]
                bound = line_for_search(v[X], direc1, lb, ub)
                if bound is None:
                    st[N_ZERO_DISP] += 1
                    lmax = 1.0
                else:
                    lmax = bound[1]
                if lmax < 1:
                    st[N_CLIPPED] += 1
                v[XI] = direc1
                v[CAND] = _clip(v[X] + min(lmax, 1) * direc1, lb, ub)
                phase = PH_EXTRAP
                todo = EMIT
    st[PHASE] = phase
    if st[STATUS] != RUNNING:
        v[CAND] = v[X]


def step(finalize, xtol, ftol, max_iter, kind, a, b, lb, ub, vec, direc, scal, cand_f, theta, state, history=None):
    """One launch.  vec (S, 6, d), direc (S, d, d), scal (S, 20), cand_f (S,), theta (S, d), state (S, 24) uint64, history (L, S)
    or None.  Before launch 0 the caller has put x0 (inside the bounds) into vec[:, X] and the directions into direc and
    zeroed state word 0.  Returns a dict of the arrays it leaves behind; the arguments are not changed."""
    vec, direc, scal, theta, state = vec.copy(), direc.copy(), scal.copy(), theta.copy(), state.copy()
    history = None if history is None else history.copy()
    out = dict(vec=vec, direc=direc, scal=scal, theta=theta, state=state, history=history)
    S = vec.shape[0]
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    emit = np.zeros(S, dtype=bool)                   # the searches whose row of theta this launch writes
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for s in range(S):
            L = int(state[s, LAUNCHES])
            if finalize:
                emit[s] = L >= 1
                continue
            if L == 0:
                x0 = vec[s, X].copy()
                vec[s] = x0
                scal[s] = 0.0
                scal[s, BEST_F] = -np.inf
                state[s] = 0
                state[s, LAUNCHES] = 1
                state[s, PHASE] = PH_X0
                emit[s] = True
                continue
            if state[s, STATUS] == RUNNING:          # (a frozen search's row is its x already)
                _advance(cost(cand_f[s]), xtol, ftol, max_iter, lb, ub, vec[s], direc[s], scal[s], state[s])
                emit[s] = True
            state[s, LAUNCHES] = L + 1
            if history is not None and L - 1 < history.shape[0]:
                history[L - 1, s] = scal[s, BEST_F]
        if emit.any():
            theta[emit] = transform(kind, a, b, vec[emit, (BEST_X if finalize == 2 else X) if finalize else CAND])
    return out


def counters(state):
    """the branch counters of one search's state words, by name"""
    return {k: int(state[N_LINES + j]) for j, k in enumerate(COUNTERS)}


def minimize(f, x0, lb, ub, xtol=1e-4, ftol=1e-4, max_iterations=None, max_evaluations=None, direc=None, record=None):
    """Drive ONE search with f: (d,) point -> value (f is maximised) as `optimize.Powell.run` does: scipy's rule for the two
    limits, a stop after `max_evaluations` values, then a finalize.  `record`: a list that receives every evaluated point.
    Returns the final dict with 'x', 'fun' (scipy's, of g = -f), 'nit', 'nfev', 'status' (3: stopped by max_evaluations)."""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    d = lb.size
    if max_iterations is None and max_evaluations is None:
        max_iterations = max_evaluations = 1000 * d
    max_iter = UNBOUNDED if max_iterations is None else int(max_iterations)
    kind, a, b = np.zeros(d, np.int32), np.zeros(d), np.ones(d)              # theta = x
    vec = np.zeros((1, VEC_ROWS, d))
    vec[0, X] = np.clip(np.asarray(x0, dtype=np.float64), lb, ub)
    D = np.eye(d) if direc is None else np.array(direc, dtype=np.float64)
    t = dict(vec=vec, direc=D[None].copy(), scal=np.zeros((1, SCALARS)), theta=np.zeros((1, d)),
             state=np.zeros((1, STATE_WORDS), dtype=np.uint64))
    cand_f = np.zeros(1)
    args = (xtol, ftol, max_iter, kind, a, b, lb, ub)
    while True:
        t = step(False, *args, t['vec'], t['direc'], t['scal'], cand_f, t['theta'], t['state'])
        st = t['state'][0]
        if st[STATUS] != RUNNING or (max_evaluations is not None and st[NFEV] >= max_evaluations):
            break
        pt = t['vec'][0, CAND].copy()
        if record is not None:
            record.append(pt)
        cand_f = np.array([f(pt)], dtype=np.float64)
    t = step(True, *args, t['vec'], t['direc'], t['scal'], cand_f, t['theta'], t['state'])
    st = t['state'][0]
    t.update(x=t['vec'][0, X].copy(), fun=float(t['scal'][0, FVAL]), nit=int(st[NIT]), nfev=int(st[NFEV]),
             status=int(st[STATUS]) if st[STATUS] != RUNNING else 3, counters=counters(st))
    return t
