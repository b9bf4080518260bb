"""numpy restatement of one `pem_de_step_f64_dev` launch (csrc/pem_de.hip): the same Philox counters, the same integer
maps, the same IEEE operations in the same order (wave64 xor butterflies, then the waves in order), so that the trial u,
the selected population, the best index and the convergence record compare bit for bit.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import sampler_np as snp

PICK, CROSS, REDRAW, DITHER = 0, 1, 2, 3
BEST1BIN, RAND1BIN = 0, 1
_U = np.uint64


def u_open(hi, lo):
    k = ((np.asarray(hi, dtype=_U) >> _U(6)) << _U(26)) | (np.asarray(lo, dtype=_U) >> _U(6))
    return (_U(2) * k + _U(1)).astype(np.float64) * 2.0 ** -53


def below(w, n):
    return ((np.asarray(w, dtype=_U) * _U(n)) >> _U(32)).astype(np.int64)


def rank_key(f):
    return np.where(f > -np.inf, f, -np.inf)


def block_sum(x, P):
    """sum of x[:P] as the kernel forms it: zeros up to whole waves, a xor butterfly per wave, the waves in order"""
    n = (P + 63) // 64 * 64
    v = np.zeros(n)
    v[:P] = x[:P]
    v = v.reshape(-1, 64)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ m]
    tot = v[0, 0]
    for w in range(1, v.shape[0]):
        tot = tot + v[w, 0]
    return tot


def _sort2(x, y):
    return np.minimum(x, y), np.maximum(x, y)


def step(g, P, d, strategy, finalize, seed, mut, cr, tol, atol, kind, a, b, pop_u, pop_f, trial_u, trial_f):
    """One launch at state g.  Returns a dict of the arrays it leaves behind (u, values, theta, state, record, hist) --
    theta as sampler_np.transform of the u it is made from."""
    pop_u, pop_f, trial_u = pop_u.copy(), pop_f.copy(), trial_u.copy()
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    tf = lambda u: np.stack([snp.transform(kind[j], a[j], b[j], u[:, j]) for j in range(d)], axis=1)   # noqa: E731
    out = dict(pop_u=pop_u, pop_f=pop_f, trial_u=trial_u, state=g, record=None, hist=None)
    if g == 0:
        if finalize:
            return out
        trial_u[:] = np.minimum(np.maximum(trial_u, 2.0 ** -53), 1.0 - 2.0 ** -53)
        out.update(theta=tf(trial_u), state=1, record=np.array([-np.inf, -1.0, 0.0]))
        return out
    take = (rank_key(trial_f) > rank_key(pop_f)) | (g == 1)
    pop_u[take] = trial_u[take]
    pop_f[take] = trial_f[take]
    f = pop_f
    best = int(np.argmax(rank_key(f)))
    with np.errstate(invalid='ignore', over='ignore'):
        mean = block_sum(f, P) / float(P)
        dev = f - mean
        sd = np.sqrt(block_sum(dev * dev, P) / float(P))
        conv = 1.0 if sd <= atol + tol * abs(mean) else 0.0
    out.update(record=np.array([rank_key(f)[best], float(best), conv]), hist=rank_key(f)[best])
    if finalize:
        out.update(theta=tf(pop_u))
        return out
    i = np.arange(P, dtype=np.uint64)
    dz = snp.philox4x32_10(0, g, DITHER, 0, k0, k1)
    F = mut[0] + (mut[1] - mut[0]) * float(snp.u53(dz[0], dz[1]))
    pk = snp.philox4x32_10(i, g, PICK, 0, k0, k1)
    ii = np.arange(P)
    r0 = below(pk[0], P - 1)
    r0 = r0 + (r0 >= ii)
    e0, e1 = _sort2(ii, r0)
    r1 = below(pk[1], P - 2)
    r1 = r1 + (r1 >= e0)
    r1 = r1 + (r1 >= e1)
    base, da, db = np.full(P, best), r0, r1
    if strategy == RAND1BIN:
        e1, e2 = _sort2(e1, r1)
        e0, e1 = _sort2(e0, e1)
        r2 = below(pk[2], P - 3)
        r2 = r2 + (r2 >= e0)
        r2 = r2 + (r2 >= e1)
        r2 = r2 + (r2 >= e2)
        base, da, db = r0, r1, r2
    assert np.all(da != ii) and np.all(db != ii) and np.all(da != db) and (strategy == BEST1BIN or np.all(base != ii))
    fill = below(pk[3], d)
    new = pop_u.copy()
    redrawn = 0
    for j in range(d):
        cx = snp.philox4x32_10(i, g, CROSS, j // 2, k0, k1)
        uc = snp.u53(cx[0], cx[1]) if j % 2 == 0 else snp.u53(cx[2], cx[3])
        mutate = (uc < cr) | (fill == j)
        t = pop_u[da, j] - pop_u[db, j]
        t = F * t
        x = np.where(mutate, pop_u[base, j] + t, pop_u[:, j])
        bad = ~((x > 0.0) & (x < 1.0))
        if bad.any():
            rd = snp.philox4x32_10(i, g, REDRAW, j // 2, k0, k1)
            x = np.where(bad, u_open(rd[0], rd[1]) if j % 2 == 0 else u_open(rd[2], rd[3]), x)
            redrawn += int(bad.sum())
        new[:, j] = x
    out.update(trial_u=new, theta=tf(new), state=g + 1, redrawn=redrawn)
    return out
