"""numpy restatement of one `pem_dram_step_f64_dev` launch (csrc/pem_dram.hip): the same Philox counters, the same IEEE
operations in the same order (every sum in index order, products and sums rounded separately, the Cholesky factor row by row
from the lower triangle), so that proposals, point, moments, factor, counters and traces compare bit for bit; the two accept
decisions go through numpy's exp / log / log1p and can differ from the device's in the last bit.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import sampler_np as snp

Z1, Z2, U = 0x44520000, 0x44520001, 0x44520002
_U = np.uint64


def u_open(hi, lo):
    k = ((np.asarray(hi, dtype=_U) >> _U(6)) << _U(26)) | (np.asarray(lo, dtype=_U) >> _U(6))
    return (_U(2) * k + _U(1)).astype(np.float64) * 2.0 ** -53


def draws(seed, s, K, d):
    """z1 (K, d), z2 (K, d), u1 (K,), u2 (K,) of step s (an int, or one per chain)"""
    from scipy.special import ndtri
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    chain = np.arange(K, dtype=_U)
    step = np.broadcast_to(np.asarray(s, dtype=_U) & _U(0xFFFFFFFF), (K,))
    z = []
    for purpose in (Z1, Z2):
        cols = []
        for j in range(d):
            r = snp.philox4x32_10(chain, step, purpose, j // 2, k0, k1)
            cols.append(ndtri(u_open(r[0], r[1]) if j % 2 == 0 else u_open(r[2], r[3])))
        z.append(np.stack(cols, axis=1))
    r = snp.philox4x32_10(chain, step, U, 0, k0, k1)
    return z[0], z[1], snp.u53(r[0], r[1]), snp.u53(r[2], r[3])


def propose(theta, L, z1, z2, gamma):
    """(2, K, d): y1 = x + L z1 and y2 = x + sqrt(gamma) L z2, each row's sum with i ascending"""
    K, d = theta.shape
    sg = np.sqrt(gamma)
    out = np.empty((2, K, d))
    for j in range(d):
        t1, t2 = np.zeros(K), np.zeros(K)
        for i in range(j + 1):
            t1 = t1 + L[:, j, i] * z1[:, i]
            t2 = t2 + L[:, j, i] * z2[:, i]
        out[0, :, j] = theta[:, j] + t1
        out[1, :, j] = theta[:, j] + sg * t2
    return out


def cholesky(C, L_old):
    """Row-by-row lower Cholesky factors of the lower triangles of C (K, d, d).  Returns (L, failed): where a pivot is not > 0
    the chain's row of L is L_old's, whole, and failed[k] is True."""
    K, d, _ = C.shape
    A = np.zeros_like(C)
    failed = np.zeros(K, dtype=bool)
    with np.errstate(all='ignore'):
        for c in range(d):                                   # column c: the pivot, then the entries below it
            acc = C[:, c:, c].copy()                         # (K, d - c)
            for i in range(c):
                acc = acc - A[:, c:, i] * A[:, c, i][:, None]
            pivot = acc[:, 0]
            failed |= ~(pivot > 0.0)
            r = np.sqrt(pivot)
            A[:, c, c] = r
            A[:, c + 1:, c] = acc[:, 1:] / r[:, None]
    A[failed] = L_old[failed]
    return A, failed


def decide(lp0, lp1, lp2, z1, z2, u1, u2, gamma):
    """the two accept decisions of a step and the numbers they compare (for a test to recognise a near-tie)"""
    K, d = z1.shape
    sg = np.sqrt(gamma)
    ww, zz = np.zeros(K), np.zeros(K)
    for i in range(d):
        w = z1[:, i] - sg * z2[:, i]
        ww = ww + w * w
        zz = zz + z1[:, i] * z1[:, i]
    with np.errstate(all='ignore'):
        clamp = lambda x: np.where(x > 0.0, 0.0, x)                                              # noqa: E731  (NaN stays NaN)
        a1 = np.exp(clamp(lp1 - lp0))
        acc1 = u1 < a1
        a1_rev = np.exp(clamp(lp1 - lp2))
        log_q = -0.5 * (ww - zz)
        log_a2 = (((lp2 - lp0) + log_q) + np.log1p(-a1_rev)) - np.log1p(-a1)
        log_u2 = np.log(u2)
        acc2 = ~acc1 & (log_u2 < log_a2)
    return dict(acc1=acc1, acc2=acc2, a1=a1, u1=u1, log_u2=log_u2, log_a2=log_a2)


def step(st, prop_logp, seed, gamma, eps, adapt_after, adapt_interval, trace_first=0, trace_len=0, thin=1, now=None, nxt=None,
         decisions=None):
    """One launch.  st: dict of theta (K, d), logp (K,), L (K, d, d), mean, scatter, prop (2, K, d), state (K,), accepted (2, K),
    flags (K,) and optionally trace (T, K, d) / logp_trace (T, K); prop_logp: (2, K).  now / nxt: (z1, z2, u1, u2) of the step
    being resolved / of the next one, in place of `draws` (the normals of a device, the draws of a torch generator);
    decisions: (acc1, acc2) to impose in place of this file's own.  Returns the new dict and the `decide` record (None where
    no chain had a step pending)."""
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    theta, logp, L, mean, scatter = out['theta'], out['logp'], out['L'], out['mean'], out['scatter']
    K, d = theta.shape
    s = np.broadcast_to(np.asarray(st['state'], dtype=np.int64), (K,)).copy()
    rec = None
    act = s >= 1
    if act.any():
        z1, z2, u1, u2 = draws(seed, s, K, d) if now is None else now
        rec = decide(logp, prop_logp[0], prop_logp[1], z1, z2, u1, u2, gamma)
        acc1, acc2 = (rec['acc1'], rec['acc2']) if decisions is None else decisions
        acc1, acc2 = acc1 & act, acc2 & act
        theta[acc1] = st['prop'][0][acc1]
        theta[acc2] = st['prop'][1][acc2]
        logp[acc1] = prop_logp[0][acc1]
        logp[acc2] = prop_logp[1][acc2]
        out['accepted'][0] += acc1.astype(out['accepted'].dtype)
        out['accepted'][1] += acc2.astype(out['accepted'].dtype)
        r = s - 1 - trace_first
        due = act & (r >= 0) & (r % thin == 0) & (r // thin < trace_len)
        for k in np.nonzero(due)[0]:
            if out.get('trace') is not None:
                out['trace'][r[k] // thin, k] = theta[k]
            if out.get('logp_trace') is not None:
                out['logp_trace'][r[k] // thin, k] = logp[k]
        count = (s + 1).astype(np.float64)
        with np.errstate(all='ignore'):
            delta = theta - mean
            new_mean = mean + delta / count[:, None]
            new_scatter = scatter + delta[:, :, None] * (theta - new_mean)[:, None, :]
            mean[act] = new_mean[act]
            scatter[act] = new_scatter[act]
            adapt = act & (s >= adapt_after) & ((s - adapt_after) % adapt_interval == 0)
            if adapt.any():
                cov = ((2.4 * 2.4) / d) * (scatter / (count - 1.0)[:, None, None] + eps * np.eye(d))
                A, failed = cholesky(cov, L)
                ok = adapt & ~failed
                L[ok] = A[ok]
                out['flags'][adapt & failed] |= 1
    z1, z2, _, _ = draws(seed, s + 1, K, d) if nxt is None else nxt
    out['prop'] = propose(theta, L, z1, z2, gamma)
    out['state'] = (s + 1).astype(np.asarray(st['state']).dtype)
    return out, rec
