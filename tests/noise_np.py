"""Plain numpy restatement of pem_loglik_marginal_scaled_f64_dev (csrc/pem_likelihood.hip) in the kernel's own order.  TEST
INFRASTRUCTURE.

float64 throughout, the sums in the order of the kernel: the weights w = (1 / s)^2, the per-draw sums by one fma per condition in
increasing e, the discharge sum as pem_loglik_marginal_f64_dev forms it, times w_d; draw m on lane m mod 256 of the row's
workgroup, streamed into the lane's (max, acc, acc2, cw) state, the 64 lanes of a wave merged by the xor butterfly 32, 16, .. 1,
the four waves in order by lane 0.  numpy's exp and log are not the device's, so the device is held to tests/hp_noise.py, as this
file is; what this file adds is the order (tests/test_noise_scale_host.py) and a reference a test can apply to a posterior's own
per-sample sums (tests/test_noise_scale.py)."""
import numpy as np

from hp_likelihood import Q_OVER_M, fma

BLOCK, WAVE = 256, 64


def weights(theta, scale_col, discharge_col):
    """(w [K][G + 1], log s [K][G + 1]): 1 / s^2 and log s of every group and, last, of the discharge term; 1 and 0 where the
    column is -1, NaN where the scale is not a finite number above 0"""
    cols = list(scale_col) + [discharge_col]
    K = 1 if theta is None else np.asarray(theta).shape[0]
    w, l = np.ones((K, len(cols))), np.zeros((K, len(cols)))
    for j, c in enumerate(cols):
        if c < 0:
            continue
        s = np.asarray(theta, dtype=np.float64)[:, c]
        ok = (s > 0.0) & (s < np.inf)
        with np.errstate(all='ignore'):
            inv = 1.0 / s
            w[:, j] = np.where(ok, inv * inv, np.nan)
            l[:, j] = np.where(ok, np.log(np.where(ok, s, 1.0)), np.nan)
    return w, l


def draw_sums(ll, group_end, w, mdot_a=None, a_1=None, discharge=0.0, sigma=1.0):
    """(S [K][M], C [K][M][G + 1]): the scaled sum of every draw and the unscaled sums of its groups (last: the discharge term)"""
    ll = np.asarray(ll, dtype=np.float64)
    K, M, E = ll.shape
    G = len(group_end)
    s, c = np.zeros((K, M)), np.zeros((K, M, G + 1))
    with np.errstate(all='ignore'):
        first = 0
        for g in range(G):
            for e in range(first, group_end[g]):
                s = fma(ll[:, :, e], np.broadcast_to(w[:, g, None], (K, M)), s)
                c[:, :, g] = c[:, :, g] + ll[:, :, e]
            first = group_end[g]
        if mdot_a is not None:
            inv_sigma = 1.0 / sigma
            t = np.zeros((K, M))
            for e in range(E):
                i_d = Q_OVER_M * mdot_a[:, :, e] / (1.0 - a_1[:, :, e] * 2.0)
                z = (discharge - i_d) * inv_sigma
                t = fma(-0.5 * z, z, t)
            s = fma(t, np.broadcast_to(w[:, G, None], (K, M)), s)
            c[:, :, G] = t
    return s, c


def _push(st, s, c, on):
    """lsew_push of every (row, lane) where `on`; st = (mx, acc, acc2, cw)"""
    mx, acc, acc2, cw = st
    with np.errstate(all='ignore'):
        up = on & (s > mx)
        e = np.exp(mx - s)
        empty = acc == 0.0
        acc_u = np.where(empty, 0.0, acc * e) + 1.0
        acc2_u = np.where(empty, 0.0, acc2 * e * e) + 1.0
        cw_u = np.where(empty[..., None], 0.0, cw * e[..., None]) + c
        add = on & ~up & (s != -np.inf)           # NaN s lands here and poisons every sum
        p = np.exp(s - mx)
        acc_a = acc + p
        acc2_a = fma(p, p, acc2)
        cw_a = fma(np.broadcast_to(p[..., None], c.shape), c, cw)
    pick = lambda u, a, old: np.where(up, u, np.where(add, a, old))      # noqa: E731
    pick3 = lambda u, a, old: np.where(up[..., None], u, np.where(add[..., None], a, old))      # noqa: E731
    return np.where(up, s, mx), pick(acc_u, acc_a, acc), pick(acc2_u, acc2_a, acc2), pick3(cw_u, cw_a, cw)


def _merge(a, b):
    amx, aacc, aacc2, acw = a
    bmx, bacc, bacc2, bcw = b
    with np.errstate(all='ignore'):
        m = np.fmax(amx, bmx)
        ea, eb = np.exp(amx - m), np.exp(bmx - m)
        za, zb = aacc == 0.0, bacc == 0.0
        acc = np.where(za, 0.0, aacc * ea) + np.where(zb, 0.0, bacc * eb)
        acc2 = np.where(za, 0.0, aacc2 * ea * ea) + np.where(zb, 0.0, bacc2 * eb * eb)
        cw = np.where(za[..., None], 0.0, acw * ea[..., None]) + np.where(zb[..., None], 0.0, bcw * eb[..., None])
    return m, acc, acc2, cw


def marginal_scaled(ll, group_end, group_count, theta=None, scale_col=None, discharge_col=-1, mdot_a=None, a_1=None, discharge=0.0,
                    sigma=1.0, log_prior=None):
    """(out [K], ess [K], chi [K][G + 1]) of pem_loglik_marginal_scaled_f64_dev for ll [K][M][E] float64"""
    ll = np.asarray(ll, dtype=np.float64)
    K, M, E = ll.shape
    G = len(group_end)
    scale_col = [-1] * G if scale_col is None else list(scale_col)
    w, logs = weights(theta, scale_col, discharge_col)
    w, logs = np.broadcast_to(w, (K, G + 1)), np.broadcast_to(logs, (K, G + 1))
    s, c = draw_sums(ll, group_end, w, mdot_a, a_1, discharge, sigma)
    st = (np.full((K, BLOCK), -np.inf), np.zeros((K, BLOCK)), np.zeros((K, BLOCK)), np.zeros((K, BLOCK, G + 1)))
    lane = np.arange(BLOCK)
    for r in range(-(-M // BLOCK)):
        m = r * BLOCK + lane
        on = np.broadcast_to(m < M, (K, BLOCK))
        mm = np.minimum(m, M - 1)
        st = _push(st, s[:, mm], c[:, mm], on)
    for sh in (32, 16, 8, 4, 2, 1):
        st = _merge(st, tuple(x[:, lane ^ sh] for x in st))
    tot = tuple(x[:, 0] for x in st)
    for wv in range(1, BLOCK // WAVE):
        tot = _merge(tot, tuple(x[:, wv * WAVE] for x in st))
    mx, acc, acc2, cw = tot
    with np.errstate(all='ignore'):
        cn = np.zeros(K)
        for g in range(G):
            cn = fma(np.full(K, float(group_count[g])), logs[:, g], cn)
        if discharge_col >= 0:
            cn = fma(np.full(K, float(E)), logs[:, G], cn)
        out = mx + np.log(acc) - cn
        out = np.where(np.isnan(acc), acc, out)
        if log_prior is not None:
            lp = np.asarray(log_prior, dtype=np.float64)
            out = np.where(np.isfinite(lp) & ~np.isnan(out), lp + out, -np.inf)
        ess = acc * acc / acc2
        chi = cw / acc[:, None]
    return out, ess, chi
