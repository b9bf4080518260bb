"""numpy restatement of one `pem_ensemble_step_f64_dev` launch (csrc/pem_ensemble.hip): the same Philox counters, the same IEEE
operations in the same order (products and sums rounded separately), so that proposals, walkers, counters and traces compare
bit for bit once the device's z / g are handed over (g goes through ndtri, log q through numpy's log: the library's can differ
in the last bit, and with it an accept decision whose two sides all but tie).  `run` drives a numpy log posterior through whole
steps, which is what the CPU tests of the algorithm's own properties use.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import sampler_np as snp

MOVE, PROPOSE, ACCEPT = 0x454E0000, 0x454E0001, 0x454E0002
_U = np.uint64


def u_open(hi, lo):
    k = ((np.asarray(hi, dtype=_U) >> _U(6)) << _U(26)) | (np.asarray(lo, dtype=_U) >> _U(6))
    return (_U(2) * k + _U(1)).astype(np.float64) * 2.0 ** -53


def draws(seed, s, E, H, normals=True):
    """the random numbers of half-step s: u_move (E,), and per moving walker (E, H) the partners j1, j2 (j2 as the DE move
    takes it), the stretch uniform u, the DE normal n (None unless `normals`) and the accept uniform u_acc"""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    s = int(s) & 0xFFFFFFFF
    ens, m = np.arange(E, dtype=_U)[:, None], np.arange(H, dtype=_U)[None, :]
    mv = snp.philox4x32_10(np.arange(E, dtype=_U), s, MOVE, 0, k0, k1)
    r = snp.philox4x32_10(ens, s, PROPOSE, m, k0, k1)
    ac = snp.philox4x32_10(ens, s, ACCEPT, m, k0, k1)
    j1 = ((r[0] * _U(H)) >> _U(32)).astype(np.int64)
    j2 = ((r[1] * _U(max(H - 1, 0))) >> _U(32)).astype(np.int64)
    j2 = j2 + (j2 >= j1)
    n = None
    if normals:
        from scipy.special import ndtri
        n = ndtri(u_open(r[2], r[3]))
    return dict(u_move=snp.u53(mv[0], mv[1]), j1=j1, j2=j2, u=snp.u53(r[2], r[3]), n=n, u_acc=snp.u53(ac[0], ac[1]))


def moves(dr, a, de_fraction, g0, sigma):
    """what the half does with its draws: de (E,) and per moving walker coef = g (DE) or z (stretch), j1, j2 (-1: stretch)"""
    de = dr['u_move'] < de_fraction
    t = (a - 1.0) * dr['u'] + 1.0
    z = t * t / a
    g = g0 * (1.0 + sigma * dr['n']) if dr['n'] is not None else np.full_like(z, np.nan)
    return dict(de=de, coef=np.where(de[:, None], g, z), j1=dr['j1'], j2=np.where(de[:, None], dr['j2'], -1), u_move=dr['u_move'])


def propose(theta, half, mv):
    """(prop (E, H, d), log_q (E, H)) of the half `half` of theta (E, K, d) against the other one"""
    E, K, d = theta.shape
    H = K // 2
    mb, cb = half * H, H - half * H
    xw, comp = theta[:, mb:mb + H], theta[:, cb:cb + H]
    c = mv['coef'][:, :, None]
    x1 = np.take_along_axis(comp, mv['j1'][:, :, None], axis=1)
    x2 = np.take_along_axis(comp, np.clip(mv['j2'], 0, H - 1)[:, :, None], axis=1)
    with np.errstate(all='ignore'):
        stretch = x1 + c * (xw - x1)
        de = xw + c * (x1 - x2)
        log_q = np.where(mv['de'][:, None], 0.0, float(d - 1) * np.log(mv['coef']))
    return np.where(mv['de'][:, None, None], de, stretch), log_q


def decide(lp_old, lp_new, log_q, u_acc):
    """the accept decisions of a half-step and the two numbers each compares (for a test to recognise a near-tie)"""
    with np.errstate(all='ignore'):
        lhs = np.log(u_acc)
        rhs = log_q + (lp_new - lp_old)
        return dict(acc=lhs < rhs, lhs=lhs, rhs=rhs, u_acc=u_acc)


def step(st, prop_logp, seed, a=2.0, de_fraction=0.0, g0=None, sigma=1e-5, trace_first=0, trace_len=0, thin=1, coef=None,
         decisions=None):
    """One launch.  st: dict of theta (E, K, d), logp (E, K), prop (E, H, d), log_q (E, H), state (E,) -- one value: the
    ensembles are launched together --, accepted (E, K) and optionally trace (T, E, K, d) / logp_trace (T, E, K); prop_logp:
    (E, H).  coef: (E, H) z / g to propose with in place of this file's own (a device's); decisions: (E, H) to impose in place
    of this file's own.  Returns the new dict, the `decide` record (None at launch 0) and the `moves` of the half-step proposed."""
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    theta, logp = out['theta'], out['logp']
    E, K, d = theta.shape
    H = K // 2
    g0 = 2.38 / np.sqrt(2.0 * d) if g0 is None else g0
    s = int(np.asarray(st['state']).reshape(-1)[0])
    assert np.all(np.asarray(st['state']) == s)
    rec = None
    if s >= 1:
        base = ((s - 1) % 2) * H
        rec = decide(logp[:, base:base + H], prop_logp, st['log_q'], draws(seed, s, E, H, normals=False)['u_acc'])
        acc = rec['acc'] if decisions is None else np.asarray(decisions, dtype=bool)
        moving_lp, moving = logp[:, base:base + H], theta[:, base:base + H]          # views
        moving_lp[acc] = prop_logp[acc]
        moving[acc] = st['prop'][acc]
        out['accepted'][:, base:base + H] += acc.astype(out['accepted'].dtype)
        if s % 2 == 0:
            r = s // 2 - 1 - trace_first
            if r >= 0 and r % thin == 0 and r // thin < trace_len:
                if out.get('trace') is not None:
                    out['trace'][r // thin] = theta
                if out.get('logp_trace') is not None:
                    out['logp_trace'][r // thin] = logp
    mv = moves(draws(seed, s + 1, E, H, normals=de_fraction > 0.0), a, de_fraction, g0, sigma)
    if coef is not None:
        mv['coef'] = np.asarray(coef, dtype=np.float64)
    out['prop'], out['log_q'] = propose(theta, s % 2, mv)
    out['state'] = np.full_like(np.asarray(st['state']), s + 1)
    return out, rec, mv


def run(f, theta0, n_steps, seed=0, a=2.0, de_fraction=0.0, g0=None, sigma=1e-5, thin=1):
    """n_steps whole steps of E ensembles from theta0 (E, K, d) with the numpy log posterior f: (E H, d) -> (E H,), as
    calibration.DeviceEnsemble drives the kernel.  Returns the final state dict; its trace is (ceil(n_steps / thin), E, K, d)."""
    theta0 = np.array(theta0, dtype=np.float64)
    E, K, d = theta0.shape
    H = K // 2
    rows = -(-n_steps // thin)
    logp = np.concatenate([np.asarray(f(theta0[:, h * H:(h + 1) * H].reshape(E * H, d))).reshape(E, H) for h in (0, 1)], axis=1)
    st = dict(theta=theta0, logp=logp, prop=np.zeros((E, H, d)), log_q=np.zeros((E, H)), state=np.zeros(E, dtype=np.int64),
              accepted=np.zeros((E, K), dtype=np.int64), trace=np.full((rows, E, K, d), np.nan),
              logp_trace=np.full((rows, E, K), np.nan))
    kw = dict(seed=seed, a=a, de_fraction=de_fraction, g0=g0, sigma=sigma, trace_first=0, trace_len=rows, thin=thin)
    st, _, _ = step(st, np.zeros((E, H)), **kw)
    for _ in range(2 * n_steps):
        st, _, _ = step(st, np.asarray(f(st['prop'].reshape(E * H, d)), dtype=np.float64).reshape(E, H), **kw)
    return st
