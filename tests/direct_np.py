"""numpy restatement of pem_direct_step_f64_dev (csrc/pem_direct.hip), launch by launch, and of scipy's
`direct(f, bounds, locally_biased=False)` driven through it.

One launch consumes the values of the rows it emitted last, completes the divisions those rows belong to, runs a selection round
when the round's queue of kept anchors is empty, and emits the points of as many queued anchors as fit into `rows`.  The rules
are the ones include/pem_hip.h lists for the entry point; tests/test_direct_host.py holds `minimize` to scipy bit for bit --
every evaluated point in order, x, fun, nit, nfev and status -- and tests/test_direct.py holds the kernel to `step`.

The arithmetic that decides anything is written so that numpy and the kernel round alike: one operation per statement, no sum
across dimensions, the volume as a product in ascending dimension.
"""
import math

import numpy as np

from oracle import sampler_np as snp

# state words
LAUNCHES, NIT, NFEV, STATUS, Q_HEAD, Q_LEN, BEST, PEND, TIES, END = range(10)
STATE_WORDS = 10
MAX_DIM, MAX_LEVELS, MAX_DEPTH, MAX_ROWS = 32, 1024, 64, 1024
HISTORY_COLS = 3
PAD, START = -1, -2                                  # rowinfo[:, 0] of a padding row and of the start's centre
STATUS_NAMES = {0: 'running', 1: 'max_evaluations exceeded', 2: 'max_iterations reached', 4: 'vol_tol met', 5: 'len_tol met',
                6: 'store or level table full', 7: 'non-finite value'}


def depth(d):
    """exponents the level table of PEM_DIRECT_MAX_LEVELS entries holds for d dimensions"""
    return min(MAX_LEVELS // d, MAX_DEPTH)


def tables(d, n_depth=None):
    """(thirds (n_depth + 1,), levels (n_depth d,)) as the host builds them"""
    n = depth(d) if n_depth is None else n_depth
    thirds = np.empty(n + 1)
    thirds[0] = 1.0
    h = 3.0
    for i in range(1, n + 1):
        thirds[i] = 1.0 / h
        h *= 3.0
    w = [math.sqrt(d - j + j / 9.) * 0.5 for j in range(d)]
    levels = np.empty(n * d)
    h = 1.0
    for i in range(n):
        for j in range(d):
            levels[i * d + j] = w[j] / h
        h *= 3.0
    return thirds, levels


def transform(kind, a, b, x):
    """theta of rows x (..., d)"""
    return np.stack([snp.transform(kind[j], a[j], b[j], x[..., j]) for j in range(x.shape[-1])], axis=-1)


def point(c, lb, ub):
    """the point evaluated for a centre: two operations, rounded separately"""
    xs1 = ub - lb
    xs2 = lb / xs1
    t = c + xs2
    return t * xs1


def reported_x(c, lb, ub):
    """scipy's `x` for the centre it ends with: c xs1 + xs1 xs2 (not the point it evaluated; they differ by an ulp)"""
    xs1 = ub - lb
    xs2 = lb / xs1
    return c * xs1 + xs1 * xs2


def cost(f):
    """g = -f, with -0 folded into +0 (the integer key of the scan tells them apart)"""
    return -np.asarray(f, dtype=np.float64) + 0.0


def level_of(L, d):
    k = int(L.min())
    return k * d + (d - int((L == k).sum()))


def store_size(d, max_fun):
    """rectangles the driver makes room for: a round is never cut short, so the last one may overshoot max_fun"""
    return max_fun + 1 + 2 * d * MAX_DEPTH


def new_state(d, rows, cap):
    """the caller-owned arrays, zeroed (launch 0 needs state word 0 to be 0 and nothing else)"""
    return dict(centres=np.zeros((cap, d)), values=np.zeros(cap), expo=np.zeros((cap, d), np.int32), level=np.zeros(cap, np.int32),
                queue=np.zeros(MAX_LEVELS, np.int32), rowinfo=np.zeros((rows, 2), np.int32), theta=np.zeros((rows, d)),
                state=np.zeros(STATE_WORDS, np.uint64))


def _select(d, eps, cap, n_depth, levels, values, level, n, gmin):
    """one selection round over the n rectangles: (kept anchors in ascending level, ties met, whether the store and the level
    table hold their divisions)"""
    lv, g = level[:n], values[:n]
    kept, ties, best = [], 0, math.inf
    for l in np.unique(lv):                                          # ascending
        members = np.flatnonzero(lv == l)
        low = g[members].min()
        at = members[g[members] == low]
        ties += at.size - 1
        if low < best:                                               # the Pareto staircase
            kept.append((int(l), int(at[0])))
            best = low
    while len(kept) > 1:                                              # eps eats the staircase from its small end
        lj, j = kept[-1]
        lo = math.inf
        for li, i in kept[:-1]:
            num = g[i] - g[j]
            den = levels[li] - levels[lj]
            lo = min(lo, num / den)
        prod = lo * levels[lj]
        slack = eps * abs(gmin)
        if g[j] - prod > gmin - slack:
            kept.pop()
        else:
            break
    total = sum(2 * (d - l % d) for l, _ in kept)
    fits = n + total <= cap and all(l // d + 2 <= n_depth for l, _ in kept)
    return kept, ties, fits


def step(finalize, eps, vol_tol, len_tol, max_iter, max_fun, kind, a, b, lb, ub, thirds, levels, t, cand_f, history=None):
    """One launch on t = dict(centres (cap, d), values (cap,), expo (cap, d) int32, level (cap,) int32, queue (1024,) int32,
    rowinfo (rows, 2) int32, theta (rows, d), state (10,) uint64).  Returns the dict (and history) it leaves behind; the
    arguments are not changed."""
    t = {k: v.copy() for k, v in t.items()}
    history = None if history is None else history.copy()
    t['history'] = history
    C_, G, E, LV, Q, RI, TH, st = (t[k] for k in ('centres', 'values', 'expo', 'level', 'queue', 'rowinfo', 'theta', 'state'))
    cap, d = C_.shape
    rows = TH.shape[0]
    n_depth = thirds.size - 1
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    L = int(st[LAUNCHES])
    n = int(st[NFEV])
    T = lambda c: transform(kind, a, b, point(c, lb, ub)[None])[0]                     # noqa: E731

    def record():
        if history is not None and L - 1 < history.shape[0]:
            history[L - 1] = (-G[int(st[BEST])] if int(st[NFEV]) >= 1 else math.nan, float(st[NFEV]), float(st[NIT]))

    if finalize:
        if L >= 1 and n >= 1:
            TH[0] = T(C_[int(st[BEST])])
        return t
    if L == 0:                                                       # the centre of the cube is emitted
        st[:] = 0
        st[LAUNCHES], st[PEND] = 1, 1
        C_[0] = 0.5
        RI[:] = (PAD, 0)
        RI[0] = (START, 0)
        TH[:] = T(C_[0])
        return t
    if st[STATUS] != 0:                                              # frozen
        st[LAUNCHES] = L + 1
        record()
        return t

    # ---- consume
    pend = int(st[PEND])
    g = cost(cand_f[:pend])
    if not np.isfinite(g).all():
        st[STATUS] = 7
    else:
        G[n:n + pend] = g
        for r in range(pend):                                        # the children, from the parents as they still are
            par, ss = int(RI[r, 0]), int(RI[r, 1])
            if par == START:
                E[n + r] = 0
                LV[n + r] = 0
                continue
            side, sign = ss >> 1, ss & 1
            k = int(E[par].min())
            I = np.flatnonzero(E[par] == k)
            pos = int(np.searchsorted(I, side))
            base = r - 2 * pos - sign
            w = np.minimum(g[base + 2 * np.arange(I.size)], g[base + 2 * np.arange(I.size) + 1])
            first = (w < w[pos]) | ((w == w[pos]) & (I <= side))     # the sides divided no later than this one (stable sort)
            if sign == 0:
                st[TIES] += int(((w == w[pos]) & (I < side)).sum())
            child = E[par].copy()
            child[I[first]] += 1
            E[n + r] = child
            LV[n + r] = level_of(child, d)
        for r in range(pend):                                        # then the parents, once each: at the first of their rows
            par = int(RI[r, 0])
            if par >= 0 and (r == 0 or int(RI[r - 1, 0]) != par):
                E[par][E[par] == E[par].min()] += 1
                LV[par] = level_of(E[par], d)
        low = g.min()
        if n == 0 or low < G[int(st[BEST])]:
            st[BEST] = n + int(np.flatnonzero(g == low)[0])
        n += pend
        st[NFEV] = n
    st[PEND] = 0

    # ---- the round has ended
    if st[STATUS] == 0 and st[Q_HEAD] == st[Q_LEN]:
        st[Q_HEAD] = 0
        if n == 1:                                                   # the start is divided without a selection
            Q[0] = 0
            st[Q_LEN] = 1
        else:
            st[NIT] += 1
            m = int(st[BEST])
            vol = 1.0
            for i in range(d):
                vol = vol * thirds[E[m, i]]
            if n > max_fun:
                st[STATUS] = 1
            elif vol < vol_tol:
                st[STATUS] = 4
            elif levels[LV[m]] < len_tol:
                st[STATUS] = 5
            elif int(st[NIT]) + 1 >= max_iter:
                st[STATUS] = 2
                st[NIT] = max(max_iter, 2)                           # (scipy reports 2 for maxiter = 1 as well)
            else:
                kept, ties, fits = _select(d, eps, cap, n_depth, levels, G, LV, n, G[m])
                st[TIES] += ties
                if not fits:
                    st[STATUS] = 6
                else:
                    Q[:len(kept)] = [r for _, r in kept]
                    st[Q_LEN] = len(kept)

    # ---- emit
    used = 0
    RI[:] = (PAD, 0)
    if st[STATUS] == 0:
        while st[Q_HEAD] < st[Q_LEN]:
            r = int(Q[int(st[Q_HEAD])])
            k, cnt = int(LV[r]) // d, 2 * (d - int(LV[r]) % d)
            if used + cnt > rows:
                break
            st[Q_HEAD] += 1
            delta = thirds[k + 1]
            for i in np.flatnonzero(E[r] == k):
                for sign in (0, 1):
                    c = C_[r].copy()
                    c[i] = c[i] - delta if sign else c[i] + delta
                    C_[n + used] = c
                    TH[used] = T(c)
                    RI[used] = (r, 2 * i + sign)
                    used += 1
    if n >= 1:
        TH[used:] = T(C_[int(st[BEST])])                             # left-over rows: a copy of the best point
    st[PEND] = used
    st[LAUNCHES] = L + 1
    if st[STATUS] != 0:
        st[END] = L + 1
    record()
    return t


def minimize(f, lb, ub, eps=1e-4, maxfun=None, maxiter=1000, vol_tol=1e-16, len_tol=1e-6, rows=None, cap=None, record=None,
             hostile=None, max_launches=10 ** 6):
    """scipy.optimize.direct(f, bounds, locally_biased=False) through `step`: f is MINIMISED here, as scipy's, over the box
    itself (identity priors).  hostile: launch -> values to consume instead of f's, or None."""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    d = lb.size
    rows = 2 * d if rows is None else rows
    maxfun = 1000 * d if maxfun is None else maxfun
    cap = store_size(d, maxfun) if cap is None else cap
    kind, a, b = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    thirds, levels = tables(d)
    t = new_state(d, rows, cap)
    cand_f = np.zeros(rows)
    launches = 0
    while launches < max_launches:
        t = step(0, eps, vol_tol, len_tol, maxiter, maxfun, kind, a, b, lb, ub, thirds, levels, t, cand_f)
        t.pop('history')
        launches += 1
        if t['state'][STATUS] != 0:
            break
        pend = int(t['state'][PEND])
        vals = np.array([f(x) for x in t['theta'][:pend]])
        if record is not None:
            record.extend(x.copy() for x in t['theta'][:pend])
        if hostile is not None and hostile(launches) is not None:
            vals = hostile(launches)[:pend]
        cand_f = np.zeros(rows)
        cand_f[:pend] = -vals                                        # the kernel MAXIMISES
    st = t['state']
    m = int(st[BEST])
    return dict(x=reported_x(t['centres'][m], lb, ub), fun=float(t['values'][m]), nit=int(st[NIT]), nfev=int(st[NFEV]),
                status=int(st[STATUS]), ties=int(st[TIES]), launches=launches, state=t)
