"""numpy restatement of one `pem_nm_step_f64_dev` launch (csrc/pem_nm.hip): scipy's `_minimize_neldermead` with every point an
iteration can ask for emitted before the iteration starts, the same IEEE operations in the same order, a stable sort, so that
the simplex, its values, the candidate rows, the counters and the history compare bit for bit.  `minimize` drives launches to
completion with a Python f.  It is the definition the kernel is held to.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import sampler_np as snp

LAUNCHES, NIT, NFEV, STATUS, N_REFLECT, N_EXPAND, N_OUTSIDE, N_INSIDE, N_SHRINK, LAST_OP = range(10)
REFLECT, EXPAND, OUTSIDE, INSIDE, SHRINK = 1, 2, 3, 4, 5
STATE_WORDS = 10


def coefficients(d, adaptive=True):
    """(rho, chi, psi, sigma) exactly as scipy writes them"""
    if adaptive:
        dim = float(d)
        return 1, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim
    return 1, 2, 0.5, 0.5


def initial_simplex(x0, lb, ub, sim=None):
    """scipy's construction: x0 clipped, vertex k + 1 = x0 with component k times 1.05 (0.00025 where it is zero); then -- for a
    caller's simplex too -- entries above ub reflected into the interior, and clipped"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    if sim is None:
        x0 = np.clip(np.asarray(x0, dtype=np.float64), lb, ub)
        n = x0.size
        sim = np.empty((n + 1, n))
        sim[0] = x0
        for k in range(n):
            y = x0.copy()
            y[k] = (1 + 0.05) * y[k] if y[k] != 0 else 0.00025
            sim[k + 1] = y
    sim = np.asarray(sim, dtype=np.float64)
    sim = np.where(sim > ub, 2 * ub - sim, sim)
    return np.clip(sim, lb, ub)


def cost(f):
    """g = -f, a NaN f is +inf"""
    f = np.asarray(f, dtype=np.float64)
    return np.where(np.isnan(f), np.inf, -f)


def _within(diff, tol):
    v = np.abs(diff)
    return (v < np.inf) & (v <= tol)


def transform(kind, a, b, x):
    """theta of rows x (..., d)"""
    return np.stack([snp.transform(kind[j], a[j], b[j], x[..., j]) for j in range(x.shape[-1])], axis=-1)


def step(finalize, coef, xatol, fatol, kind, a, b, lb, ub, sim, fsim, cand_x, cand_f, theta, state, history=None):
    """One launch.  sim (S, d+1, d), fsim (S, d+1), cand_x (S, d+4, d), cand_f (S, d+4), theta (S (d+4), d), state (S, 10)
    uint64, history (L, S) or None.  Returns a dict of the arrays it leaves behind; the arguments are not changed."""
    sim, fsim, cand_x, theta, state = sim.copy(), fsim.copy(), cand_x.copy(), theta.copy(), state.copy()
    history = None if history is None else history.copy()
    out = dict(sim=sim, fsim=fsim, cand_x=cand_x, theta=theta, state=state, history=history)
    S, nv, d = sim.shape
    nc = d + 4
    rho, chi, psi, sigma = coef
    th = theta.reshape(S, nc, d)
    tie = False
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(S):
            L = int(state[s, LAUNCHES])
            if L == 0:
                if finalize:
                    continue
                cand_x[s, :nv] = sim[s]
                cand_x[s, nv:] = sim[s, 0]
                th[s] = transform(kind, a, b, cand_x[s])
                state[s] = 0
                state[s, LAUNCHES] = 1
                continue
            x, g = sim[s].copy(), -fsim[s]
            if state[s, STATUS] == 0:
                cg = cost(cand_f[s])
                op = 0
                if L == 1:
                    g = cg[:nv].copy()
                    state[s, NIT], state[s, NFEV] = 1, nv
                else:
                    gr, ge, gc, gcc = cg[:4]
                    take = -1
                    if gr < g[0]:
                        state[s, NFEV] += 2
                        take, op = (1, EXPAND) if ge < gr else (0, REFLECT)
                    elif gr < g[d - 1]:
                        state[s, NFEV] += 1
                        take, op = 0, REFLECT
                    elif gr < g[d]:
                        state[s, NFEV] += 2
                        if gc <= gr:
                            take, op = 2, OUTSIDE
                    else:
                        state[s, NFEV] += 2
                        if gcc < g[d]:
                            take, op = 3, INSIDE
                    g = g.copy()
                    if take >= 0:
                        x[d], g[d] = cand_x[s, take], cg[take]
                    else:
                        op = SHRINK
                        state[s, NFEV] += d
                        x[1:], g[1:] = cand_x[s, 4:], cg[4:]
                    state[s, NIT] += 1
                    state[s, 3 + op] += 1
                    state[s, LAST_OP] = op
                tie = tie or len(set(g.tolist())) < nv
                order = np.argsort(g, kind='stable')
                x, g = x[order], g[order]
                sim[s], fsim[s] = x, -g
                conv = bool(np.all(_within(x[1:] - x[0], xatol)) and np.all(_within(g[0] - g[1:], fatol)))
                state[s, STATUS] = 1 if conv else 0
                if not conv and not finalize:
                    xbar = x[0].copy()
                    for i in range(1, d):
                        xbar = xbar + x[i]
                    xbar = xbar / float(d)
                    w = x[d]
                    rows = np.empty((nc, d))
                    rows[0] = (1 + rho) * xbar - rho * w
                    rows[1] = (1 + rho * chi) * xbar - rho * chi * w
                    rows[2] = (1 + psi * rho) * xbar - psi * rho * w
                    rows[3] = (1 - psi) * xbar + psi * w
                    rows[4:] = x[0] + sigma * (x[1:] - x[0])
                    cand_x[s] = np.minimum(np.maximum(rows, lb), ub)
                    th[s] = transform(kind, a, b, cand_x[s])
            if finalize:
                th[s] = transform(kind, a, b, x[0])[None]
            else:
                state[s, LAUNCHES] = L + 1
            if history is not None and L - 1 < history.shape[0]:
                history[L - 1, s] = -g[0]
    out['tie'] = tie
    return out


def minimize(f, x0, lb, ub, adaptive=True, xatol=1e-4, fatol=1e-4, max_iterations=None, sim0=None):
    """Drive ONE simplex with f: (n, d) rows -> (n,) values (f is maximised) until it freezes or nit == max_iterations, as
    `optimize.NelderMead.run` does.  Returns the final state dict with 'operations', 'ties' (a sort ever saw two equal values)."""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    d = lb.size
    m = 200 * d if max_iterations is None else int(max_iterations)
    kind, a, b = np.zeros(d, np.int32), np.zeros(d), np.ones(d)              # theta = x
    t = dict(sim=initial_simplex(x0, lb, ub, sim0)[None], fsim=np.zeros((1, d + 1)), cand_x=np.zeros((1, d + 4, d)),
             theta=np.zeros((d + 4, d)), state=np.zeros((1, STATE_WORDS), dtype=np.uint64))
    coef = coefficients(d, adaptive)
    cand_f = np.zeros((1, d + 4))
    ties = False
    for _ in range(m):
        t = step(False, coef, xatol, fatol, kind, a, b, lb, ub, t['sim'], t['fsim'], t['cand_x'], cand_f, t['theta'], t['state'])
        ties = ties or t['tie']
        if t['state'][0, STATUS] == 1:
            break
        cand_f = np.asarray(f(t['cand_x'][0]), dtype=np.float64)[None]
    t = step(True, coef, xatol, fatol, kind, a, b, lb, ub, t['sim'], t['fsim'], t['cand_x'], cand_f, t['theta'], t['state'])
    t['ties'] = ties or t['tie']
    t['operations'] = t['state'][0, N_REFLECT:N_SHRINK + 1].astype(np.int64)
    return t
