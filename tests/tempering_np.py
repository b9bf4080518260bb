"""numpy restatement of one `pem_tempered_ensemble_step_f64_dev` launch (csrc/pem_tempering.hip), state word for state word: the
moves are tests/ensemble_np.py's own functions (the same Philox counters, the ensemble index e = r T + t in the counter), judged
by the tempered ratio, and the even-odd swaps follow with their own purpose word.  The same IEEE operations in the same order
(products and sums rounded separately; log q of the stretch through `log_restated`, the launch's own log written in IEEE
operations for this purpose), so that given the device's g everything compares bit for bit, log q included, up to a decision
whose two sides tie within the last bit of the library log of a uniform.  `run` drives two numpy callables through whole steps,
which is what the CPU tests of the algorithm's own properties and the margins of the device tests use.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import ensemble_np
from oracle import sampler_np as snp

SWAP = 0x454E0003
_U = np.uint64


_H = float.fromhex
LN2_HI, LN2_LO = _H('0x1.62e42fee00000p-1'), _H('0x1.a39ef35793c76p-33')
LG = [_H(v) for v in ('0x1.5555555555593p-1', '0x1.999999997fa04p-2', '0x1.2492494229359p-2', '0x1.c71c51d8e78afp-3',
                      '0x1.7466496cb03dep-3', '0x1.39a09d078c69fp-3', '0x1.2f112df3e5244p-3')]


def log_restated(x):
    """log_restatable of csrc/pem_ensemble_moves.h (fdlibm's e_log.c), operation for operation: every branch is evaluated for
    every element and the device's is selected.  x positive, finite, normal (anything else: numpy's log, as the device asks
    its library)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = x.view(_U)
    hx = (bits >> _U(32)).astype(np.int64)
    k = (hx >> 20) - 1023
    hx = hx & 0x000fffff
    i = (hx + 0x95f64) & 0x100000
    k = k + (i >> 20)
    m = (((hx | (i ^ 0x3ff00000)).astype(_U) << _U(32)) | (bits & _U(0xffffffff))).view(np.float64)
    with np.errstate(all='ignore'):
        f, dk = m - 1.0, k.astype(np.float64)
        r_small = f * f * (0.5 - 0.33333333333333333 * f)
        small = np.where(f == 0.0, np.where(k == 0, 0.0, dk * LN2_HI + dk * LN2_LO),
                         np.where(k == 0, f - r_small, dk * LN2_HI - ((r_small - dk * LN2_LO) - f)))
        s = f / (2.0 + f)
        z = s * s
        w = z * z
        t1 = w * (LG[1] + w * (LG[3] + w * LG[5]))
        t2 = z * (LG[0] + w * (LG[2] + w * (LG[4] + w * LG[6])))
        r = t2 + t1
        hfsq = 0.5 * f * f
        mid = np.where(k == 0, f - (hfsq - s * (hfsq + r)), dk * LN2_HI - ((hfsq - (s * (hfsq + r) + dk * LN2_LO)) - f))
        ends = np.where(k == 0, f - s * (f - r), dk * LN2_HI - ((s * (f - r) - dk * LN2_LO) - f))
        out = np.where((0x000fffff & (2 + hx)) < 3, small, np.where(((hx - 0x6147a) | (0x6b851 - hx)) > 0, mid, ends))
        return np.where((x >= 2.0 ** -1022) & (x < np.inf), out, np.log(x))


def swap_draws(seed, n, R, T, K):
    """u_swap (R, T, K) of step n: row t belongs to the pair (t, t + 1); only the rows of the pairs that are due are used"""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    e = np.arange(R * T, dtype=_U).reshape(R, T, 1)
    x = snp.philox4x32_10(e, int(n) & 0xFFFFFFFF, SWAP, np.arange(K, dtype=_U)[None, None, :], k0, k1)
    return snp.u53(x[0], x[1])


def pairs_due(n, T):
    """the lower temperatures t of the pairs (t, t + 1) that step n (n = 1, 2, ...) visits"""
    return list(range(int(n) % 2, T - 1, 2))


def decide(l_old, p_old, l_new, p_new, log_q, beta, u_acc):
    """the accept decisions of a half-step: beta (E, 1); a value that is not finite is refused whatever beta is"""
    with np.errstate(all='ignore'):
        lhs = np.log(u_acc)
        rhs = (log_q + (p_new - p_old)) + beta * (l_new - l_old)
        return dict(acc=np.isfinite(l_new) & np.isfinite(p_new) & (lhs < rhs), lhs=lhs, rhs=rhs, u_acc=u_acc)


def step(st, prop_loglik, prop_logprior, beta, seed, a=2.0, de_fraction=0.0, g0=None, sigma=1e-5, trace_first=0, trace_len=0, thin=1,
         coef=None, decisions=None, copy=True):
    """One launch.  st: dict of theta (E, K, d), loglik (E, K), logprior (E, K), prop (E, H, d), log_q (E, H), state (R,),
    accepted (E, K), swap_attempts / swap_accepted (R, T - 1) and optionally trace (rows, E, K, d), loglik_trace, logprior_trace
    (rows, E, K), E = R T with T = len(beta); prop_loglik, prop_logprior: (E, H).  coef: (E, H) z / g to propose with in place of
    this file's own (a device's: g goes through the library's normcdfinv); decisions: (E, H) to impose in place of this file's
    own; copy=False works in place.  Returns the new dict, the `decide` record (None at launch 0), the `moves` of the half-step proposed and the swap record (None unless
    a step ended: dict of the pairs visited and acc (R, T - 1, K), False where no pair was due)."""
    out = {k: np.array(v, copy=True) for k, v in st.items()} if copy else st
    beta = np.asarray(beta, dtype=np.float64)
    theta, ll, lp = out['theta'], out['loglik'], out['logprior']
    E, K, d = theta.shape
    T = beta.size
    R, H = E // T, K // 2
    assert R * T == E
    g0 = 2.38 / np.sqrt(2.0 * d) if g0 is None else g0
    s = int(np.asarray(st['state']).reshape(-1)[0])
    assert np.all(np.asarray(st['state']) == s)
    prop, pending_q = np.asarray(st['prop']), np.asarray(st['log_q'])
    rec = swaps = None
    if s >= 1:
        base = ((s - 1) % 2) * H
        rec = decide(ll[:, base:base + H], lp[:, base:base + H], prop_loglik, prop_logprior, pending_q, np.tile(beta, R)[:, None],
                     ensemble_np.draws(seed, s, E, H, normals=False)['u_acc'])
        acc = rec['acc'] if decisions is None else np.asarray(decisions, dtype=bool)
        ll[:, base:base + H][acc] = prop_loglik[acc]                      # (views: the writes land in ll, lp and theta)
        lp[:, base:base + H][acc] = prop_logprior[acc]
        theta[:, base:base + H][acc] = prop[acc]
        out['accepted'][:, base:base + H] += acc.astype(out['accepted'].dtype)
        if s % 2 == 0:
            n = s // 2
            swaps = dict(pairs=pairs_due(n, T), acc=np.zeros((R, max(T - 1, 0), K), dtype=bool))
            u = swap_draws(seed, n, R, T, K)
            th4, ll3, lp3 = theta.reshape(R, T, K, d), ll.reshape(R, T, K), lp.reshape(R, T, K)      # views
            for t in swaps['pairs']:
                with np.errstate(all='ignore'):
                    sw = np.log(u[:, t]) < (beta[t] - beta[t + 1]) * (ll3[:, t + 1] - ll3[:, t])
                swaps['acc'][:, t] = sw
                for arr in (th4, ll3, lp3):
                    lo, hi = arr[:, t].copy(), arr[:, t + 1].copy()
                    arr[:, t][sw], arr[:, t + 1][sw] = hi[sw], lo[sw]
                out['swap_attempts'][:, t] += K
                out['swap_accepted'][:, t] += sw.sum(axis=1).astype(out['swap_accepted'].dtype)
            q = n - 1 - trace_first
            if q >= 0 and q % thin == 0 and q // thin < trace_len:
                for name, val in (('trace', theta), ('loglik_trace', ll), ('logprior_trace', lp)):
                    if out.get(name) is not None:
                        out[name][q // thin] = val
    mv = ensemble_np.moves(ensemble_np.draws(seed, s + 1, E, H, normals=de_fraction > 0.0), a, de_fraction, g0, sigma)
    if coef is not None:
        mv['coef'] = np.asarray(coef, dtype=np.float64)
    out['prop'], _ = ensemble_np.propose(theta, s % 2, mv)
    out['log_q'] = np.where(mv['de'][:, None], 0.0, float(d - 1) * log_restated(mv['coef']))
    out['state'] = np.full_like(np.asarray(st['state']), s + 1)
    return out, rec, mv, swaps


def run(loglik, logprior, theta0, beta, n_steps, seed=0, a=2.0, de_fraction=0.0, g0=None, sigma=1e-5, thin=1, keep_theta=True):
    """n_steps whole steps from theta0 (R, T, K, d) with the numpy callables loglik, logprior: (E H, d) -> (E H,), as
    calibration.DeviceTemperedEnsemble drives the kernel.  Returns the final state dict; its traces are (ceil(n_steps / thin), E,
    K[, d]) (no theta trace with keep_theta=False)."""
    theta0 = np.array(theta0, dtype=np.float64)
    R, T, K, d = theta0.shape
    E, H = R * T, K // 2
    theta0 = theta0.reshape(E, K, d)
    rows = -(-n_steps // thin)
    both = lambda f: np.concatenate([np.asarray(f(theta0[:, h * H:(h + 1) * H].reshape(E * H, d)), dtype=np.float64).reshape(E, H)  # noqa: E731
                                     for h in (0, 1)], axis=1)
    st = dict(theta=theta0, loglik=both(loglik), logprior=both(logprior), prop=np.zeros((E, H, d)), log_q=np.zeros((E, H)),
              state=np.zeros(R, dtype=np.int64), accepted=np.zeros((E, K), dtype=np.int64),
              swap_attempts=np.zeros((R, max(T - 1, 0)), dtype=np.int64), swap_accepted=np.zeros((R, max(T - 1, 0)), dtype=np.int64),
              loglik_trace=np.full((rows, E, K), np.nan), logprior_trace=np.full((rows, E, K), np.nan))
    if keep_theta:
        st['trace'] = np.full((rows, E, K, d), np.nan)
    assert np.isfinite(st['loglik']).all() and np.isfinite(st['logprior']).all()
    kw = dict(beta=beta, seed=seed, a=a, de_fraction=de_fraction, g0=g0, sigma=sigma, trace_first=0, trace_len=rows, thin=thin,
              copy=False)
    st, _, _, _ = step(st, np.zeros((E, H)), np.zeros((E, H)), **kw)
    for _ in range(2 * n_steps):
        flat = st['prop'].reshape(E * H, d)
        st, _, _, _ = step(st, np.asarray(loglik(flat), dtype=np.float64).reshape(E, H),
                           np.asarray(logprior(flat), dtype=np.float64).reshape(E, H), **kw)
    return st
