"""Long-double restatements of the calibration likelihood kernels, with per-entry error bounds.  TEST INFRASTRUCTURE.

The kernels held here: the stand-alone j_ion likelihood (pem_jion_loglik_f64_dev), the fused likelihood modes of
plume_r1_kernel (JMODE 3, 6 and 7: pem_coupled_loglik / pem_coupled_system_loglik / pem_coupled_system_predict), the
marginal (pem_loglik_marginal_f64_dev) and the prior (pem_log_prior_f64_dev), all in csrc/pem_likelihood.hip and
csrc/pem_kernels.hip.  As in tests/hp_reference.py, each result is held to its formula evaluated in np.longdouble (its own
error, 2^-11 of the double unit u = 2^-53, is absorbed by the factor 1.01) under a bound C * u * S, S the same formula on
absolute values, C derived from the rounding count of the kernel; gamma_k = k u / (1 - k u) <= 1.01 k u.

Derivations (one term t = -0.5 z^2 of a per-sample sum, z = (y - m) * inv_std, inv_std the kernel's own double):
  * z: y - m is one rounding, the product with inv_std a second: z (1 + theta_2), so z^2 carries theta_4.  -0.5 z is exact,
    the fma that adds -0.5 z * z to the running sum rounds once, which is a summation step.
  * the sum: a term passes through at most n + 2 additions (n records; the fma chains of the lanes are shorter, then two
    shuffle adds), so with the 4 of z^2 every term carries at most n + 6 roundings: |err| <= gamma_{n+6} sum |t|.
  * the model value m = fma(w, hi - lo, lo) from a profile (only where the reference is given the profile, not the kernel's
    m): the subtraction and the fma round once each, |dm| <= u (|w| |hi - lo| + |m|) (1 + u); it moves t by
    |z| |inv_std| |dm| to first order (the second-order term inv_std^2 dm^2 / 2 is below u^2 and is absorbed by 1.01).
  * discharge term of the marginal: I_d = Q mdot_a / (1 - 2 a_1), Q the kernel's folded double (Q_OVER_M), is three roundings
    (2 a_1 is exact); z = (D - I_d) inv_sigma two more: |dt| <= |z| inv_sigma 3.03 u |I_d| + 4.04 u |t|.  The per-draw sum
    s = sum_e ll_e + sum_e t_e takes every term through at most n_cond + 2 roundings.
  * log-sum-exp: the result moves by at most max_m B_m when every s_m moves by B_m (LSE is 1-Lipschitz in the max norm).
    acc = sum_m exp(s_m - mx) is formed by streaming pushes and tree merges: a term is rescaled at most R = ceil(n/256) + 9
    times (its own push, the pushes of later maxima in its lane, 6 shuffle levels, 3 workgroup merges), each an exp (<= 1 ulp
    = 2 u) and a product (u), and its arguments, rounded differences of the running maxima, telescope to mx - s_m: relative
    error u (2 |s_m - mx| + 4 R) per term; the additions are at most ceil(n/256) + 9 deep.  So
    |err| <= max_m B_m + 1.01 [u sum_m w_m (2 |x_m| + 4 R) + u (ceil(n/256) + 9)] + 2 u |log acc| + u |mx + log acc|,
    w_m = exp(x_m) / acc, x_m = s_m - mx; log is within 1 ulp.  A draw at -inf is -inf exactly and adds exactly 0: it is
    left out of both the max and the sum.
  * prior, per dimension (log within 1 ulp = 2 u of its value): uniform -log(b - a): u + 2 u |v|; log-uniform -log(x) -
    log(ln10_d (b - a)): 2 u |log x| + 2.5 u (b - a, the literal ln10_d = ln 10 (1 + u/2), the product) + 2 u |log(...)| +
    u |v|; normal -0.5 ((x - a) / b)^2 - log(b sqrt(2 pi)_d): 5 u |0.5 z^2| + 1.5 u + 2 u |log(...)| + u |v|; the ndim
    values are summed in a chain: gamma_ndim sum |v|.

j_ion records at several sweep radii (JMODE 8 / 9: pem_coupled_system_{loglik,predict}_radii_f64_dev), `radii_record_ref`:
  * the device forms the record's value as fma(base(r), fma(w, g[k+1] - g[k], g[k]), j_cex(r)) from the radius-free shape g;
    the reference states the same quantity from the pinned fp64 oracle's own terms (oracle_ctypes.plume_terms with the list of
    radii): the node value v_k = X1 exp(-(alpha_k / a1)^2) + X2 exp(-(alpha_k / a2)^2) + j_cex at the record's radius, alpha_k =
    k (pi/2) / 90 and alpha_90 = pi/2 (the doubles of the kernels' grid), in long double, and the model value
    v_k + w (v_{k+1} - v_k).  A sample the oracle flags invalid over ALL radii is 1e-20 at every record, exactly.
  * what a correct fp64 evaluation of a node may differ by is the project's j_ion rule and nothing new (tests/parity_rules.py,
    derived there): s_k = 1e-10 |v_k| + TAU sum |t_i| + 8 eps (1 + |decay|) |I_B0| / (2 pi r^2), the allowance
    parity_rules.j_ion_error applies to one entry with the term sizes of parity_rules.plume_bounds.  The prediction is a convex
    combination of two nodes (w in [0, 1]), so their errors combine as (1 - w) s_k + w s_{k+1}; the interpolation's own two
    roundings add model_error(w, v_k, v_{k+1}).  The 1e-20 fill is exact: slack 0.  Where the oracle's own terms are not finite
    the slack is not either and nothing is held but the kind of the value (NaN, +inf, -inf), as j_ion_error does.
  * a long double carries exponents a double does not: a term whose double exp() is exactly zero (argument below -745.13) is
    zero in the reference as well, so that an infinite amplitude times it is the NaN every fp64 evaluation gives, not inf.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
Q_OVER_M = 1.6e-19 / 2.18e-25           # the kernel's folded constant (the same correctly rounded double)
LN10_D = 2.302585092994045684           # the kernel's literals
SQRT2PI_D = 2.5066282746310002
UNIFORM, LOGUNIFORM, NORMAL = 0, 1, 2
assert np.finfo(LD).nmant >= 63, 'the reference needs an 80-bit long double'


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


# ---- the interpolated model value, bit for bit ------------------------------------------------------------------------
def fma(a, b, c):
    """correctly rounded a * b + c of float64 arrays (numpy has no fma): the long-double value, rounded to double, is
    exact wherever it lies farther than its own error from a rounding boundary; the few others are redone in rationals."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    p = _ld(a) * _ld(b)
    v = p + _ld(c)
    r = v.astype(np.float64)
    err = (np.abs(p) + np.abs(v)) * LD(2.0 ** -63)
    lo_mid = (_ld(r) + _ld(np.nextafter(r, -np.inf))) / 2
    hi_mid = (_ld(r) + _ld(np.nextafter(r, np.inf))) / 2
    with np.errstate(invalid='ignore'):
        unsure = np.isfinite(r) & ~((v - lo_mid > err) & (hi_mid - v > err))
    r = np.array(r, copy=True)
    for i in zip(*np.nonzero(unsure)):
        x = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        r[i] = float(x)
    return r


def interp_model(w, lo, hi):
    """the kernels' model value fma(w, hi - lo, lo), bit for bit"""
    w, lo, hi = (np.asarray(v, dtype=np.float64) for v in (w, lo, hi))
    return fma(w, hi - lo, lo)


# ---- per-sample sums --------------------------------------------------------------------------------------------------
def record_sum(m, y, inv_std, valid=None, dm=None):
    """(sum, bound) over the last axis of -0.5 ((y - m) inv_std)^2, m the model values (float64; where `dm` is given, the
    bound on their own error), `valid` a mask of the records that count.  Long double; the bound of the module docstring."""
    m, y, s = _ld(m), _ld(y), _ld(inv_std)
    z = (y - m) * s
    t = LD(-0.5) * z * z
    if valid is None:
        valid = np.ones(t.shape, dtype=bool)
    t = np.where(valid, t, LD(0))
    n = valid.sum(axis=-1)
    total = t.sum(axis=-1)
    bound = 1.01 * (n + 6) * U * np.abs(t).sum(axis=-1)
    if dm is not None:
        bound = bound + 1.01 * np.where(valid, np.abs(z) * np.abs(s) * _ld(dm), LD(0)).sum(axis=-1)
    return total, bound


def model_error(w, lo, hi):
    """bound on |fma(w, hi - lo, lo) - (lo + w (hi - lo))|, the exact interpolation of the same doubles"""
    w, lo, hi = (_ld(v) for v in (w, lo, hi))
    d = hi - lo                                  # signed: an interval whose ends differ in sign spans |hi| + |lo|
    return LD(1.01 * U) * (np.abs(w) * np.abs(d) + np.abs(lo + w * d))


def profile_sum(prof, k, w, y, inv_std, valid=None):
    """(sum, bound) of the j_ion records of a sample against its profile, interpolated exactly in long double:
    prof [..., 91] float64; k, w, y, inv_std [..., n_rec] (broadcast)."""
    prof = np.asarray(prof, dtype=np.float64)
    k = np.asarray(k, dtype=np.int64)
    kb = np.broadcast_to(k, prof.shape[:-1] + k.shape[-1:])
    lo = np.take_along_axis(prof, kb, axis=-1)
    hi = np.take_along_axis(prof, kb + 1, axis=-1)
    wl = _ld(w)
    m = _ld(lo) + wl * (_ld(hi) - _ld(lo))
    dm = model_error(w, lo, hi)
    yt, st = _ld(y), _ld(inv_std)
    z = (yt - m) * st
    t = LD(-0.5) * z * z
    if valid is None:
        valid = np.ones(t.shape, dtype=bool)
    t = np.where(valid, t, LD(0))
    n = valid.sum(axis=-1)
    bound = 1.01 * (n + 6) * U * np.abs(t).sum(axis=-1) + 1.01 * np.where(valid, np.abs(z) * np.abs(st) * dm, LD(0)).sum(axis=-1)
    return t.sum(axis=-1), bound


# ---- j_ion records at several sweep radii ---------------------------------------------------------------------------------
def _radii_nodes(terms, invalid, k, ridx, slack_tab):
    """(v, s): the long-double node values v_k at angle nodes k and radius indices ridx (integer arrays that broadcast against
    (n, 1)) and their allowances s_k, slack_tab the (n, 91, R) table parity_rules.plume_bounds(...)['j_slack']"""
    import parity_rules as pr
    n = terms['a1'].shape[0]
    k, ridx = np.broadcast_arrays(np.asarray(k, dtype=np.int64), np.asarray(ridx, dtype=np.int64))
    shape = np.broadcast_shapes(k.shape, (n, 1))
    k, ridx = np.broadcast_to(k, shape), np.broadcast_to(ridx, shape)
    rows = np.arange(n)[:, None]
    alpha = pr.angle_grid()[k]                                     # the doubles k (pi/2) / 90, and pi/2 itself at k = 90
    bad = np.asarray(invalid, dtype=bool)[:, None]
    with np.errstate(all='ignore'):
        v = _ld(terms['j_cex'])[rows, ridx]
        for X, a in (('X1', 'a1'), ('X2', 'a2')):
            u = _ld(alpha) / _ld(terms[a])[:, None]
            g = np.exp(-(u * u))
            g = np.where(np.exp(-(alpha / terms[a][:, None]) ** 2) == 0.0, LD(0), g)     # (module docstring, last bullet)
            v = v + _ld(terms[X])[rows, ridx] * g
        v = np.where(bad, LD(1e-20), v)
        s = LD(pr.TOL) * np.abs(v) + _ld(slack_tab[rows, k, ridx])
        s = np.where(bad, LD(0), s)
    return v, s


def radii_node_values(terms, invalid, *, I_B0):
    """(v, s) [n][91][R]: every node value of every radius and its allowance (the whole profile oracle_ctypes.plume(...,
    radii=...)['j_ion'] states in fp64)"""
    import parity_rules as pr
    R = terms['X1'].shape[1]
    slack = pr.plume_bounds(terms, I_B0)['j_slack']
    v, s = zip(*(_radii_nodes(terms, invalid, np.arange(91)[None, :], np.full((1, 91), r), slack) for r in range(R)))
    return np.stack(v, axis=-1), np.stack(s, axis=-1)


def radii_record_ref(terms, invalid, k, w, ridx, *, I_B0):
    """(model, slack) [n][n_rec] of j_ion records {k, w, ridx} (arrays that broadcast against (n, n_rec)): the long-double
    model value v_k + w (v_{k+1} - v_k) at radius ridx of samples whose oracle terms are `terms` (oracle_ctypes.plume_terms
    with the radii) and whose all-radii flag is `invalid`, and the slack of the module docstring.  I_B0 (n,): the beam current
    the terms were made with (parity_rules.plume_bounds scales the j_cex floor by it)."""
    import parity_rules as pr
    slack_tab = pr.plume_bounds(terms, I_B0)['j_slack']
    k = np.asarray(k, dtype=np.int64)
    lo, s_lo = _radii_nodes(terms, invalid, k, ridx, slack_tab)
    hi, s_hi = _radii_nodes(terms, invalid, k + 1, ridx, slack_tab)
    wl = np.broadcast_to(_ld(w), lo.shape)
    with np.errstate(all='ignore'):
        model = lo + wl * (hi - lo)
        slack = (LD(1) - wl) * s_lo + wl * s_hi + model_error(wl, lo, hi)
    bad = np.broadcast_to(np.asarray(invalid, dtype=bool)[:, None], lo.shape)
    return np.where(bad, LD(1e-20), model), np.where(bad, LD(0), slack)


def assert_model_within(got, want, slack, what=''):
    """`got` against (want, slack) of radii_record_ref: the kind of every value (finite, NaN, +inf, -inf) identical; every
    finite value with a finite slack inside it.  Returns the largest |got - want| / slack among those (what the slack is used
    to, for a measurement; 0 where nothing was held)."""
    got = np.asarray(got, dtype=np.float64)
    want, slack = np.asarray(want, dtype=LD), np.asarray(slack, dtype=LD)
    assert got.shape == want.shape == slack.shape, (what, got.shape, want.shape, slack.shape)
    w64 = want.astype(np.float64)                                   # (a long double past the double range is an fp64 inf)
    kind = lambda a: np.where(np.isnan(a), 2, np.where(np.isinf(a), np.sign(a), 0))      # noqa: E731
    with np.errstate(all='ignore'):
        differ = kind(got) != kind(w64)
        if differ.any():
            i = np.unravel_index(np.argmax(differ), differ.shape)
            raise AssertionError(f'{what}: {int(differ.sum())} values of the wrong kind; first at {i}: got {got[i]!r} want {w64[i]!r}')
        held = np.isfinite(w64) & np.isfinite(slack)
        err = np.where(held, np.abs(got.astype(LD) - want), LD(0))
        bad = held & (err > slack)
        ratio = np.where(held & (slack > 0), err / np.where(slack > 0, slack, LD(1)), LD(0))
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(slack, LD(1e-300)), LD(0))), err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} values outside the slack; worst at {i}: got {got[i]!r} want {w64[i]!r} '
                             f'err {float(err[i]):.3e} slack {float(slack[i]):.3e}')
    return float(ratio.max(initial=0.0))


# ---- marginal ---------------------------------------------------------------------------------------------------------
def discharge_terms(mdot_a, a_1, discharge, inv_sigma):
    """(t, bound) [..., n_cond] of the discharge-current weight, inv_sigma the kernel's double 1 / sigma"""
    i_d = LD(Q_OVER_M) * _ld(mdot_a) / (LD(1) - LD(2) * _ld(a_1))
    isg = LD(inv_sigma)
    z = (LD(discharge) - i_d) * isg
    t = LD(-0.5) * z * z
    return t, np.abs(z) * isg * LD(3.03 * U) * np.abs(i_d) + LD(4.04 * U) * np.abs(t)


def marginal_ref(ll, ll_bound=None, mdot_a=None, a_1=None, discharge=0.0, sigma=1.0, log_prior=None):
    """(out, bound) [n_chains] of pem_loglik_marginal_f64_dev: ll [n_chains][n_draws][n_cond] float64 (ll_bound: the bound on
    each entry's own error, or None when the entries are the kernel's input).  Non-finite rows: NaN anywhere gives NaN, all
    -inf gives -inf; with the prior, -inf where it is not finite or the likelihood is NaN.  Bound 0 where the result is not
    finite."""
    ll = np.asarray(ll)
    K, M, E = ll.shape
    l = ll if ll.dtype == LD else _ld(ll)
    with np.errstate(invalid='ignore'):
        s = l.sum(axis=-1)
        sa = np.abs(l).sum(axis=-1)
        b_in = np.zeros_like(s) if ll_bound is None else _ld(ll_bound).sum(axis=-1)
        if mdot_a is not None:
            t, tb = discharge_terms(mdot_a, a_1, discharge, 1.0 / sigma)
            s = s + t.sum(axis=-1)
            sa = sa + np.abs(t).sum(axis=-1)
            b_in = b_in + tb.sum(axis=-1)
        B = 1.01 * (E + 2) * U * sa + b_in                          # per draw
        out = np.empty(K, dtype=LD)
        bound = np.zeros(K, dtype=LD)
        R = -(-M // 256) + 9
        for k in range(K):
            sk = s[k]
            if np.isnan(sk).any():
                out[k] = LD(np.nan)
                continue
            mx = sk.max()
            if mx == -np.inf:
                out[k] = LD(-np.inf)
                continue
            x = sk - mx
            e = np.exp(x)
            acc = e.sum()
            la = np.log(acc)
            out[k] = mx + la
            live = e > 0                       # a -inf draw is -inf exactly and adds exactly 0 (0 * inf would be NaN)
            rel = U * ((e[live] / acc) * (2 * np.abs(x[live]) + 4 * R)).sum() + U * R
            bound[k] = B[k][live].max() + 1.01 * rel + 2 * U * abs(la) + U * abs(out[k])
        if log_prior is not None:
            lp = _ld(log_prior)
            fin = np.isfinite(lp) & ~np.isnan(out)
            out = np.where(fin, lp + out, LD(-np.inf))
            bound = np.where(fin & np.isfinite(out), bound + U * np.abs(out), LD(0))
    return out, bound


# ---- prior ------------------------------------------------------------------------------------------------------------
def prior_ref(theta, kind, a, b):
    """(lp, bound) [n] of pem_log_prior_f64_dev; the support of a log-uniform entry is [10.0 ** a, 10.0 ** b] as the host
    (calibration.log_prior) decides it."""
    th = np.asarray(theta, dtype=np.float64)
    n, ndim = th.shape
    lp = np.zeros(n, dtype=LD)
    sv = np.zeros(n, dtype=LD)
    eb = np.zeros(n, dtype=LD)
    with np.errstate(divide='ignore', invalid='ignore'):
        for d in range(ndim):
            x, xa, xb = th[:, d], float(a[d]), float(b[d])
            xl = _ld(x)
            if kind[d] == UNIFORM:
                inside = (x >= xa) & (x <= xb)
                c = -np.log(LD(xb) - LD(xa))
                v = np.where(inside, c, LD(-np.inf))
                e = U * (1 + 2 * abs(c)) + U * np.abs(v)
            elif kind[d] == LOGUNIFORM:
                inside = (x >= 10.0 ** xa) & (x <= 10.0 ** xb)
                c = np.log(LD('2.30258509299404568401799145468')) + np.log(LD(xb) - LD(xa))
                lx = np.log(np.where(inside, xl, LD(1)))
                v = np.where(inside, -lx - c, LD(-np.inf))
                e = 2 * U * np.abs(lx) + 2.5 * U + 2 * U * abs(c) + U * np.abs(v)
            else:
                z = (xl - LD(xa)) / LD(xb)
                c = np.log(LD(xb)) + LD(0.5) * np.log(LD(2) * LD('3.14159265358979323846264338328'))
                v = LD(-0.5) * z * z - c
                e = 5 * U * LD(0.5) * z * z + 1.5 * U + 2 * U * abs(c) + U * np.abs(v)
            lp = lp + v
            sv = sv + np.where(np.isfinite(v), np.abs(v), LD(0))
            eb = eb + np.where(np.isfinite(v), e, LD(0))
    bound = 1.01 * (eb + 1.01 * ndim * U * sv)
    return lp, np.where(np.isfinite(lp), bound, LD(0))


# ---- checks -----------------------------------------------------------------------------------------------------------
def assert_within(got, want, bound, what=''):
    """every finite `want` met within `bound`; non-finite entries must match in kind (NaN, +inf, -inf) exactly"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=LD)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fw = np.isfinite(want)
    same_kind = np.where(fw, np.isfinite(got), (np.isnan(got) == np.isnan(want)) & (got.astype(LD) == want) | (np.isnan(got) & np.isnan(want)))
    if not same_kind.all():
        i = np.argmin(same_kind)
        raise AssertionError(f'{what}: {int((~same_kind).sum())} entries of the wrong kind; first at {i}: got {got.flat[i]!r} '
                             f'want {float(want.flat[i])!r}')
    with np.errstate(invalid='ignore'):
        err = np.where(fw, np.abs(got.astype(LD) - want), LD(0))
    bound = np.asarray(bound, dtype=LD)
    unbounded = fw & ~np.isfinite(bound)         # a NaN bound would accept anything (err > NaN is False)
    if unbounded.any():
        raise AssertionError(f'{what}: {int(unbounded.sum())} finite reference values without a finite bound; first at '
                             f'{np.argmax(unbounded.ravel())}')
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(fw, err / np.maximum(bound, LD(1e-300)), LD(0))), err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} entries outside the bound; worst at {i}: got {got[i]!r} want '
                             f'{float(want[i])!r} err {float(err[i]):.3e} bound {float(bound[i]):.3e}')
