"""Long-double restatement of pem_loglik_marginal_scaled_f64_dev (csrc/pem_likelihood.hip) with per-entry error bounds.  TEST
INFRASTRUCTURE, in the manner of tests/hp_likelihood.py, whose helpers and conventions it uses: every result is held to its
formula in np.longdouble under a bound C * u * S, u = 2^-53, S the formula on absolute values, C the kernel's rounding count;
gamma_k <= 1.01 k u; the long double's own error is absorbed by the 1.01.

The formula (DESIGN.md "Noise scales"), per row k, s_g the double in theta or 1 where the column is -1:
    w_g = (1 / s_g)^2,   S_m = sum_e ll[m][e] w_g(e) + w_d sum_e t[m][e],   L = logsumexp_m S_m,
    out = L - sum_g n_g log s_g - n_cond log s_d   (+ log_prior),
    p_m = exp(S_m - max),   ess = (sum p)^2 / sum p^2,   chi_g = sum p C_mg / sum p,   C_mg = sum_{e in g} ll[m][e],  C_md = sum_e t.

Derivations:
  * w: the reciprocal rounds once, (1 + d)^-1 squared by a rounded product: three roundings, |dw| <= 3.03 u w.
  * a term ll_e w_g of S_m: w's three roundings, then one fma per condition after it (at most n_cond) and the fma that adds the
    discharge sum: at most n_cond + 5 roundings (the issue's count; n_cond + 4 by this reckoning).
  * the discharge sum T = sum_e t_e is formed as pem_loglik_marginal_f64_dev forms it: each t_e off by its own bound tb_e
    (hp_likelihood.discharge_terms) and through at most n_cond + 2 roundings as there; times w_d (three roundings more), added by
    the last fma: |err| <= w_d (sum tb_e + gamma_{n_cond + 5} sum |t_e|).  So, per draw,
        B_m = 1.01 (n_cond + 5) u (sum_e |ll_e| w_g + w_d sum_e |t_e|) + w_d sum_e tb_e.
  * log-sum-exp: hp_likelihood.marginal_ref's bound with this B_m (the same push / merge tree, R = ceil(M / 256) + 9 rescales of a
    term): max_m B_m + 1.01 [u sum_m q_m (2 |x_m| + 4 R) + u R] + 2 u |log acc| + u |max + log acc|, q_m = p_m / sum p.
  * the normaliser c = sum_g n_g log s_g: log within 1 ulp (2 u |log s|), the product inside the fma, and a chain of at most
    n_groups + 1 fma steps: |dc| <= 1.01 (n_groups + 3) u sum |n log s|.  One more rounding for L - c: u |out|; with the prior
    another u |out| as in marginal_ref.
  * p_m: S_m and the running maximum each move by at most max_m B_m, so exp(S_m - max) moves by the factor exp(2 max B) (ess and
    chi do not change when every p is scaled alike, so the maximum the kernel settled on need not be the exact one); the rescales
    add u (2 |x_m| + 4 R) as in the log-sum-exp: delta_m = expm1(2 max B) + 1.01 u (2 |x_m| + 4 R).  p_m^2 is rescaled by e e:
    twice the exp error and two products where p has one, below 2 x 4 u per rescale: 2 delta_m.  Every sum is at most
    D = ceil(M / 256) + 9 additions deep.
  * ess = A^2 / A2: |dA| / A <= eA = sum q_m delta_m + D u, |dA2| / A2 <= eA2 = sum (p_m^2 / A2) 2 delta_m + D u, a product and a
    quotient: |d ess| <= 1.01 ess (2 eA + eA2 + 2 u).
  * chi_g = N_g / A, N_g = sum p_m C_mg: C_mg is a chain of plain additions over the group's conditions, |dC| <= bC_mg =
    gamma_{n_cond} sum |ll_e| (for the discharge column sum tb_e + gamma_{n_cond + 2} sum |t_e|); the fma p C + N rounds once, a
    summation step: |dN_g| <= sum p_m ((delta_m + D u) |C_mg| + bC_mg), so
        |d chi_g| <= 1.01 [sum q_m ((delta_m + D u) |C_mg| + bC_mg) + |chi_g| (eA + 2 u)].
  * a draw at -inf is -inf exactly, adds exactly 0 to every sum and is left out; a NaN anywhere, or a scale that is not a finite
    number above 0, makes out, ess and chi NaN (out -inf with a prior); every draw at -inf: out -inf, ess and chi NaN (0 / 0).
    Bound 0 where the value is not finite: only its kind is held.
"""
import numpy as np

from hp_likelihood import LD, U, _ld, discharge_terms


def scale_weights(theta, scale_col, discharge_col, K):
    """(s, w, log s) [K][G + 1] in long double, the discharge term last; s = 1 where the column is -1, NaN where the scale is
    not a finite number above 0"""
    cols = list(scale_col) + [discharge_col]
    s = np.ones((K, len(cols)), dtype=LD)
    for j, c in enumerate(cols):
        if c >= 0:
            v = np.asarray(theta, dtype=np.float64)[:, c]
            s[:, j] = np.where((v > 0.0) & (v < np.inf), _ld(v), LD(np.nan))
    with np.errstate(all='ignore'):
        return s, (LD(1) / s) ** 2, np.log(s)


def weighted_ref(ll, group_end, w, c=None, mdot_a=None, a_1=None, discharge=0.0, sigma=1.0, log_prior=None, c_abs=None, n_groups_c=0):
    """The reference as a function of the weights themselves: ll [K][M][E] float64, w [K][G + 1] long double, c [K] the normaliser
    (c_abs [K]: the sum of its terms' absolute values).  Returns a dict of out, ess, chi and their bounds (long double)."""
    ll = np.asarray(ll, dtype=np.float64)
    K, M, E = ll.shape
    G = len(group_end)
    l = _ld(ll)
    w = np.broadcast_to(np.asarray(w, dtype=LD), (K, G + 1))
    gidx = np.searchsorted(np.asarray(group_end), np.arange(E), side='right')
    with np.errstate(all='ignore'):
        cg = np.zeros((K, M, G + 1), dtype=LD)
        cga = np.zeros((K, M, G + 1), dtype=LD)
        for e in range(E):
            cg[:, :, gidx[e]] += l[:, :, e]
            cga[:, :, gidx[e]] += np.abs(l[:, :, e])
        bC = 1.01 * E * U * cga
        if mdot_a is not None:
            t, tb = discharge_terms(mdot_a, a_1, discharge, 1.0 / sigma)
            cg[:, :, G] = t.sum(axis=-1)
            cga[:, :, G] = np.abs(t).sum(axis=-1)
            bC[:, :, G] = tb.sum(axis=-1) + 1.01 * (E + 2) * U * cga[:, :, G]
            b_t = w[:, None, G] * tb.sum(axis=-1)
        else:
            b_t = np.zeros((K, M), dtype=LD)
        used = np.ones(G + 1, dtype=bool)
        used[G] = mdot_a is not None
        wb = w[:, None, :]
        s = np.where(used, cg * wb, LD(0)).sum(axis=-1)          # (a weight the launch never applies may be anything)
        sa = np.where(used, cga * np.abs(wb), LD(0)).sum(axis=-1)
        B = 1.01 * (E + 5) * U * sa + b_t
    out = np.empty(K, dtype=LD)
    out_b = np.zeros(K, dtype=LD)
    ess = np.full(K, np.nan, dtype=LD)
    ess_b = np.zeros(K, dtype=LD)
    chi = np.full((K, G + 1), np.nan, dtype=LD)
    chi_b = np.zeros((K, G + 1), dtype=LD)
    R = D = -(-M // 256) + 9
    for k in range(K):
        sk = s[k]
        if np.isnan(sk).any() or (c is not None and np.isnan(c[k])):
            out[k] = LD(np.nan)
            continue
        mx = sk.max()
        if mx == -np.inf:
            out[k] = LD(-np.inf)
            continue
        live = sk > -np.inf
        x = sk[live] - mx
        p = np.exp(x)
        A, A2 = p.sum(), (p * p).sum()
        la = np.log(A)
        q = p / A
        Bmax = B[k][live].max()
        rescale = U * (2 * np.abs(x) + 4 * R)
        L = mx + la
        out[k] = L
        out_b[k] = Bmax + 1.01 * ((q * rescale).sum() + U * R) + 2 * U * abs(la) + U * abs(L)
        if c is not None:
            out[k] = L - c[k]
            out_b[k] += 1.01 * (n_groups_c + 3) * U * c_abs[k] + U * abs(out[k])
        delta = np.expm1(2 * Bmax) + 1.01 * rescale
        eA = (q * delta).sum() + D * U
        eA2 = ((p * p / A2) * 2 * delta).sum() + D * U
        ess[k] = A * A / A2
        ess_b[k] = 1.01 * ess[k] * (2 * eA + eA2 + 2 * U)
        Ck, bCk = cg[k][live], bC[k][live]
        chi[k] = (q[:, None] * Ck).sum(axis=0)
        chi_b[k] = 1.01 * ((q[:, None] * ((delta[:, None] + D * U) * np.abs(Ck) + bCk)).sum(axis=0) + np.abs(chi[k]) * (eA + 2 * U))
    if log_prior is not None:
        lp = _ld(log_prior)
        fin = np.isfinite(lp) & ~np.isnan(out)
        with np.errstate(invalid='ignore'):
            out = np.where(fin, lp + out, LD(-np.inf))
            out_b = np.where(fin & np.isfinite(out), out_b + U * np.abs(out), LD(0))
    return dict(out=out, out_bound=out_b, ess=ess, ess_bound=ess_b, chi=chi, chi_bound=chi_b)


def marginal_scaled_ref(ll, group_end, group_count, theta=None, scale_col=None, discharge_col=-1, mdot_a=None, a_1=None, discharge=0.0,
                        sigma=1.0, log_prior=None):
    """out, ess, chi of pem_loglik_marginal_scaled_f64_dev and their bounds (a dict, see weighted_ref) for ll [K][M][E] float64,
    theta [K][d] float64 (None: every column -1)"""
    ll = np.asarray(ll, dtype=np.float64)
    K, E = ll.shape[0], ll.shape[2]
    G = len(group_end)
    scale_col = [-1] * G if scale_col is None else list(scale_col)
    _, w, logs = scale_weights(theta, scale_col, discharge_col, K)
    counts = np.concatenate([np.asarray(group_count, dtype=np.float64), [float(E) if discharge_col >= 0 else 0.0]]).astype(LD)
    with np.errstate(invalid='ignore'):
        terms = counts[None, :] * logs
    return weighted_ref(ll, group_end, w, terms.sum(axis=1), mdot_a, a_1, discharge, sigma, log_prior, np.abs(terms).sum(axis=1), G)
