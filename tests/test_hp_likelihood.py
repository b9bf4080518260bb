"""The long-double likelihood reference of tests/hp_likelihood.py checked on its own (no GPU): against mpmath at 60 digits on
a few rows, its exact fma against rational arithmetic, and its bounds tight enough that one planted record error breaks them."""
from fractions import Fraction

import mpmath
import numpy as np

import hp_likelihood as hl

mpmath.mp.dps = 60


def _mp(x):
    return mpmath.mpf(float(x))


def test_fma_is_correctly_rounded():
    rng = np.random.default_rng(0)
    a = rng.uniform(0, 1, 4000)
    b = rng.choice([-1.0, 1.0], 4000) * 10.0 ** rng.uniform(-8, 8, 4000)
    c = rng.choice([-1.0, 1.0], 4000) * 10.0 ** rng.uniform(-8, 8, 4000)
    a[:3], b[:3], c[:3] = [0.5, 1.0, 2.0 ** -30], [2.0 ** -53, -1.0, 1.0 + 2.0 ** -52], [1.0, 1.0, 1.0]   # ties, exact zero
    got = hl.fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_record_sums_agree_with_mpmath():
    rng = np.random.default_rng(1)
    prof = rng.choice([-1.0, 1.0], (4, 91)) * 10.0 ** rng.uniform(-6, 6, (4, 91))
    k = rng.integers(0, 90, 13)
    w = rng.uniform(0, 1, 13)
    y, s = rng.lognormal(0, 2, 13), 10.0 ** rng.uniform(-2, 1, 13)
    got, bound = hl.profile_sum(prof, k, w, y, s)
    for i in range(4):
        exact = mpmath.fsum(-0.5 * ((_mp(y[r]) - (_mp(prof[i, k[r]]) + _mp(w[r]) * (_mp(prof[i, k[r] + 1]) - _mp(prof[i, k[r]]))))
                                    * _mp(s[r])) ** 2 for r in range(13))
        assert abs(mpmath.mpf(str(got[i])) - exact) <= 2.0 ** -60 * abs(exact), (i, got[i], exact)
        assert bound[i] > 0
    m = hl.interp_model(w, prof[0, k], prof[0, k + 1])
    got, _ = hl.record_sum(m, y, s)
    exact = mpmath.fsum(-0.5 * ((_mp(y[r]) - _mp(m[r])) * _mp(s[r])) ** 2 for r in range(13))
    assert abs(mpmath.mpf(str(got)) - exact) <= 2.0 ** -60 * abs(exact)


def test_marginal_and_prior_agree_with_mpmath():
    rng = np.random.default_rng(2)
    ll = -rng.exponential(100.0, (3, 40, 4))
    md, a1 = rng.uniform(2e-6, 7e-6, (3, 40, 4)), 10.0 ** rng.uniform(-2.5, -1, (3, 40, 4))
    got, bound = hl.marginal_ref(ll, None, md, a1, 4.5, 0.2)
    inv = 1.0 / 0.2
    for k in range(3):
        s = [mpmath.fsum(_mp(ll[k, m, e]) - 0.5 * ((mpmath.mpf(4.5) - _mp(hl.Q_OVER_M) * _mp(md[k, m, e]) / (1 - 2 * _mp(a1[k, m, e])))
                                                  * _mp(inv)) ** 2 for e in range(4)) for m in range(40)]
        exact = mpmath.log(mpmath.fsum(mpmath.exp(v) for v in s))
        assert abs(mpmath.mpf(str(got[k])) - exact) <= 2.0 ** -58 * abs(exact), (k, got[k], exact)
        assert 0 < float(bound[k]) < 1e-12 * float(abs(exact))
    theta = np.array([[2.0, 3e19, 31.0], [0.5, 3e19, 31.0], [2.0, 1e23, 25.0]])
    kind, a, b = [0, 1, 2], [1.0, 18.0, 30.0], [5.0, 22.0, 5.0]
    lp, _ = hl.prior_ref(theta, kind, a, b)
    exact = (-mpmath.log(4) - mpmath.log(_mp(3e19)) - mpmath.log(mpmath.log(10) * 4)
             - mpmath.mpf(1) / 50 - mpmath.log(5 * mpmath.sqrt(2 * mpmath.pi)))
    assert abs(mpmath.mpf(str(lp[0])) - exact) <= 2.0 ** -58 * abs(exact)
    assert np.isneginf(lp[1]) and np.isneginf(lp[2])


def test_a_planted_record_error_breaks_the_bound_by_orders_of_magnitude():
    """one record counted twice, one dropped, one read from the wrong condition: each misses by far more than the bound"""
    rng = np.random.default_rng(3)
    prof = 10.0 ** rng.uniform(-3, 2, (64, 91))
    k, w = rng.integers(0, 90, 17), rng.uniform(0, 1, 17)
    y, s = rng.uniform(200, 400, 17), rng.uniform(0.3, 3, 17)       # every term far from 0
    want, bound = hl.profile_sum(prof, k, w, y, s)
    m = hl.interp_model(w, prof[:, k], prof[:, k + 1])
    t = -0.5 * ((y - m) * s) ** 2
    for planted in (t.sum(axis=1) + t[:, 0], t[:, 1:].sum(axis=1), t.sum(axis=1) - t[:, 5] + np.roll(t[:, 5], 1)):
        err = np.abs(planted.astype(hl.LD) - want)
        assert np.all(err > 1e6 * bound)
    honest = t.sum(axis=1)
    hl.assert_within(honest, want, bound, 'the same sum in double')


def test_marginal_bound_is_finite_with_some_minus_inf_draws_and_catches_a_miscount():
    """draws at -inf add nothing and carry no error; counting them as exp(0) misses the bound"""
    rng = np.random.default_rng(4)
    ll = -rng.exponential(5.0, (1, 257, 3))
    ll[0, :200] = -np.inf
    want, bound = hl.marginal_ref(ll)
    assert np.isfinite(want).all() and np.isfinite(bound).all() and bound[0] > 0
    s = ll[0].sum(axis=1)
    fin = s[np.isfinite(s)]
    miscounted = fin.max() + np.log(np.exp(fin - fin.max()).sum() + 200)       # each -inf draw taken as exp(mx - mx)
    assert abs(float(miscounted) - float(want[0])) > 1e6 * float(bound[0])
    try:
        hl.assert_within(np.array([want[0] + 1.0]), want, np.array([np.nan], dtype=hl.LD), 'NaN bound')
    except AssertionError as e:
        assert 'without a finite bound' in str(e)
    else:
        raise AssertionError('a NaN bound must not accept a value')
