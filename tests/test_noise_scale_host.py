"""Noise scales without a GPU: the numpy restatement in the kernel's order (tests/noise_np.py) is held to the long-double reference
(tests/hp_noise.py) on the cases the device is held on (tests/noise_cases.py); the reference has the identities the scaled
marginal is defined by; pem_loglik_marginal_scaled_f64_dev is declared, bound, built and exported and refuses every malformed
call before it looks for a device; calibration's bookkeeping of names, priors and groups runs on the host."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import hp_likelihood as hl
import hp_noise
import noise_cases as nc
import noise_np

ROOT = Path(__file__).resolve().parents[1]
NAME = 'pem_loglik_marginal_scaled_f64_dev'
LD = hl.LD
FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host


def _np(case):
    return noise_np.marginal_scaled(case['ll'], case['group_end'], case['group_count'], case['theta'], case['scale_col'],
                                    case['discharge_col'], case['mdot_a'], case['a_1'], *nc.DISCHARGE, case['log_prior'])


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('E, G', nc.COND_GROUPS)
def test_the_restatement_in_kernel_order_is_within_the_bounds(E, G):
    for case in nc.shape_cases(E, G):
        out, ess, chi = _np(case)
        nc.check(case, out, ess, chi)


def test_the_restatement_on_non_finite_sums_and_bad_scales():
    for case, ninf, nan, void in nc.value_cases():
        out, ess, chi = _np(case)
        nc.check(case, out, ess, chi)
        assert np.all(out[ninf] == -np.inf) and np.all(np.isnan(out[nan])), case['name']
        assert np.all(np.isnan(ess[void])) and np.all(np.isnan(chi[void])), case['name']
        live = [k for k in range(out.size) if k not in void]
        assert np.all(np.isfinite(ess[live])) and np.all(np.isfinite(chi[live])), case['name']
        rest = [k for k in range(out.size) if k not in ninf + nan]
        assert np.all(np.isfinite(out[rest])), case['name']


@pytest.mark.parametrize('E, G', nc.COND_GROUPS)
def test_at_scale_one_the_restatement_is_the_unscaled_marginal_bit_for_bit(E, G):
    """the order argument of the contract, on the host: fma(x, 1.0, s) is s + x, x * 1.0 is x, c is 0 -- so the scaled order with
    unit weights gives the bits of the plain sums pushed through the same tree"""
    for case in nc.shape_cases(E, G):
        a = _np(nc.at_scale_one(case, False))
        b = _np(nc.at_scale_one(case, True))
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), case['name']
        ll, K = case['ll'], case['ll'].shape[0]
        s = np.zeros(ll.shape[:2])
        for e in range(E):
            s = s + ll[:, :, e]                                   # pem_loglik_marginal_f64_dev's own chain of additions
        if case['mdot_a'] is not None:
            t = np.zeros_like(s)
            for e in range(E):
                z = (nc.DISCHARGE[0] - hl.Q_OVER_M * case['mdot_a'][:, :, e] / (1.0 - case['a_1'][:, :, e] * 2.0)) * (1.0 / nc.DISCHARGE[1])
                t = hl.fma(-0.5 * z, z, t)
            s = s + t
        got, _ = noise_np.draw_sums(ll, case['group_end'], np.ones((K, G + 1)), case['mdot_a'], case['a_1'], *nc.DISCHARGE)
        assert got.tobytes() == s.tobytes(), case['name']
        want, bound = hl.marginal_ref(ll, None, case['mdot_a'], case['a_1'], *nc.DISCHARGE, case['log_prior'])
        hl.assert_within(a[0], want, bound, case['name'])


# ------------------------------------------------------------------------------------------------ the identities
@pytest.fixture(scope='module')
def smooth():
    rng = np.random.default_rng(5)
    K, M, E = 2, 40, 6
    ll = -rng.gamma(2.0, 1.5, size=(K, M, E))
    md, a1 = nc._discharge_inputs(rng, (K, M, E))
    w = rng.uniform(0.5, 2.0, (K, 4)).astype(LD)
    return ll, np.asarray([2, 3, 6]), md, a1, w


def test_chi_is_the_derivative_of_the_marginal_with_respect_to_the_weights(smooth):
    """d L / d w_g = sum_m p_m C_mg / sum_m p_m: a long-double central difference with h = 1e-6 has truncation error
    h^2 |L'''| / 6 ~ 1e-12 |C|^3-scale terms and rounding error 2^-63 |L| / h ~ 1e-11; held to 1e-8 (1 + |chi|)"""
    ll, ends, md, a1, w = smooth
    ref = hp_noise.weighted_ref(ll, ends, w, None, md, a1, *nc.DISCHARGE)
    h = LD(1e-6)
    for g in range(4):
        dw = np.zeros(4, dtype=LD)
        dw[g] = h
        up = hp_noise.weighted_ref(ll, ends, w + dw, None, md, a1, *nc.DISCHARGE)['out']
        dn = hp_noise.weighted_ref(ll, ends, w - dw, None, md, a1, *nc.DISCHARGE)['out']
        fd = (up - dn) / (2 * h)
        assert np.all(np.abs(fd - ref['chi'][:, g]) <= 1e-8 * (1 + np.abs(ref['chi'][:, g]))), (g, fd, ref['chi'][:, g])


def test_with_one_draw_the_marginal_peaks_where_the_scale_matches_the_misfit():
    """M = 1: out(s_g) = C_g / s_g^2 - n_g log s_g + const has its maximum at s_g^2 = -2 C_g / n_g = -2 chi_g / n_g, the scale at
    which the group's mean squared standardised residual is 1"""
    rng = np.random.default_rng(6)
    K, E = 3, 5
    ll = -rng.gamma(2.0, 4.0, size=(K, 1, E))
    ends, counts = np.asarray([2, 5], dtype=np.int32), np.asarray([7.0, 11.0])
    theta = np.ones((K, 2))
    theta[:, 0] = rng.uniform(0.5, 2.0, K)

    def out_at(s1, fn):
        th = theta.copy()
        th[:, 1] = s1
        r = fn(ll, ends, counts, th, [0, 1])
        return r['out'] if isinstance(r, dict) else r[0]
    chi = hp_noise.marginal_scaled_ref(ll, ends, counts, theta, [0, 1])['chi']
    assert np.array_equal(chi[:, 1].astype(np.float64), ll[:, 0, 2:].astype(LD).sum(axis=1).astype(np.float64))
    peak = np.sqrt((-2 * chi[:, 1] / counts[1]).astype(np.float64))
    for fn in (hp_noise.marginal_scaled_ref, noise_np.marginal_scaled):
        top = out_at(peak, fn)
        for f in (0.5, 0.99, 1.01, 2.0):
            assert np.all(out_at(peak * f, fn) < top), (fn.__name__, f)


def test_ess_counts_the_draws_that_carry_the_estimate():
    ll = np.zeros((2, 50, 1))
    ll[1, 1:, 0] = -800.0                                         # row 1: one draw carries everything
    r = hp_noise.marginal_scaled_ref(ll, [1], [3.0])
    assert abs(r['ess'][0] - 50) < 1e-15 and abs(r['ess'][1] - 1) < 1e-15
    assert abs(r['out'][0] - np.log(LD(50))) < 1e-17 and np.all(r['chi'][0] == 0)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_point_is_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % NAME, header)
    assert m and len(m.group(1).split(',')) == 22 == len(_lib.SIGNATURES[NAME][1])
    assert hasattr(_lib.load(), NAME)
    assert re.search(r'#define PEM_NOISE_MAX_GROUPS (\d+)', header).group(1) == str(_lib.NOISE_MAX_GROUPS) == '8'


def _call(n_chains=5, n_draws=7, n_cond=6, group_end=(2, 6), group_count=(3.0, 4.0), scale_col=(1, -1), discharge_col=-1, d=3,
          ld_theta=3, ld_chi=3, n_groups=None, sigma=0.2, with_discharge=True, with_chi=True, null=()):
    from hallthrusterpem_amd import _lib
    ge, gc, sc = np.asarray(group_end, dtype=np.int32), np.asarray(group_count, dtype=np.float64), np.asarray(scale_col, dtype=np.int32)
    n_groups = ge.size if n_groups is None else n_groups
    p = {k: None if k in null else FAKE for k in ('loglik', 'mdot_a', 'a_1', 'theta', 'out')}
    h = lambda a, k: None if k in null else C.c_void_p(a.ctypes.data)      # noqa: E731
    if not with_discharge:
        p['mdot_a'] = p['a_1'] = None
    return _lib.load().pem_loglik_marginal_scaled_f64_dev(
        n_chains, n_draws, n_cond, p['loglik'], p['mdot_a'], p['a_1'], 4.5, sigma, None, n_groups, h(ge, 'group_end'),
        h(gc, 'group_count'), p['theta'], d, ld_theta, h(sc, 'scale_col'), discharge_col, FAKE, FAKE if with_chi else None, ld_chi,
        p['out'], None)


BAD = [dict(n_groups=0), dict(group_end=tuple(range(1, 10)), group_count=(1.0,) * 9, scale_col=(-1,) * 9, n_cond=9, ld_chi=10),
       dict(group_end=(0, 6)), dict(group_end=(3, 3, 6), group_count=(1.0,) * 3, scale_col=(-1,) * 3, ld_chi=4),
       dict(group_end=(4, 2, 6), group_count=(1.0,) * 3, scale_col=(-1,) * 3, ld_chi=4), dict(group_end=(2, 5)), dict(group_end=(2, 7)),
       dict(group_end=(-1, 6)), dict(group_count=(-1.0, 4.0)), dict(group_count=(np.nan, 4.0)), dict(group_count=(3.0, np.inf)),
       dict(scale_col=(3, -1)), dict(scale_col=(-2, 0)), dict(scale_col=(1, 3)), dict(discharge_col=3), dict(discharge_col=-2),
       dict(discharge_col=2, with_discharge=False), dict(ld_theta=2), dict(d=0), dict(d=4), dict(ld_chi=2),
       dict(null=('theta',)), dict(null=('theta',), scale_col=(-1, -1), discharge_col=0),
       dict(null=('group_end',)), dict(null=('group_count',)), dict(null=('scale_col',)), dict(null=('loglik',)), dict(null=('out',)), dict(null=('a_1',)),
       dict(n_draws=0), dict(n_cond=0, group_end=(0,), group_count=(1.0,), scale_col=(-1,)), dict(sigma=0.0), dict(sigma=np.nan),
       dict(n_chains=2 ** 31)]


@pytest.mark.parametrize('bad', BAD)
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_loglik_marginal_scaled' in _lib.load().pem_last_error()


def test_well_formed_calls_get_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _call() == _lib.PEM_ERR_NO_DEVICE
    assert _call(discharge_col=2, ld_theta=9) == _lib.PEM_ERR_NO_DEVICE
    assert _call(null=('theta',), scale_col=(-1, -1)) == _lib.PEM_ERR_NO_DEVICE                  # no table, every column -1
    assert _call(with_chi=False, ld_chi=0, with_discharge=False) == _lib.PEM_ERR_NO_DEVICE
    assert _call(group_end=tuple(range(1, 9)), group_count=(0.0,) * 8, scale_col=(2,) * 8, n_cond=8, ld_chi=9) == _lib.PEM_ERR_NO_DEVICE
    assert _call(n_chains=0, null=('loglik', 'out')) == _lib.PEM_OK                          # nothing to do, as the unscaled entry


# ------------------------------------------------------------------------------------------------ the Python layer
def test_names_and_priors_of_the_scales():
    from hallthrusterpem_amd.calibration import NOISE_PRIOR, noise_scale_table
    from hallthrusterpem_amd.sampling import LOGUNIFORM, PEM_V0_PRIORS, UNIFORM, Prior
    qois = ('V_cc', 'T', 'uion', 'jion')
    scaled, merged = noise_scale_table(('jion', 'V_cc'), qois, True)
    assert scaled == ('jion', 'V_cc') and merged['noise_jion'] is NOISE_PRIOR and merged['noise_V_cc'] is NOISE_PRIOR
    assert (NOISE_PRIOR.kind, NOISE_PRIOR.a, NOISE_PRIOR.b) == (LOGUNIFORM, -1.0, 1.0)
    assert all(merged[k] is v for k, v in PEM_V0_PRIORS.items()) and 'noise_jion' not in PEM_V0_PRIORS     # a copy
    mine = Prior(UNIFORM, 0.5, 4.0, 'mine')
    scaled, merged = noise_scale_table({'I_D': mine, 'uion': NOISE_PRIOR}, qois, True, {'c0': PEM_V0_PRIORS['c0']})
    assert scaled == ('I_D', 'uion') and merged['noise_I_D'] is mine and set(merged) == {'c0', 'noise_I_D', 'noise_uion'}
    assert noise_scale_table('jion', ('jion',), False)[0] == ('jion',)


@pytest.mark.parametrize('scales, has_discharge, match', [
    (('jion', 'thrust'), True, "unknown name 'thrust'"), (('I_D',), False, "unknown name 'I_D'"), (('jion', 'T', 'jion'), True, 'given twice'),
    ((), True, 'at least one'), ({'jion': (0, 1.0, 2.0)}, True, 'sampling.Prior'), ({'jion': 'NORMAL'}, True, 'NORMAL prior'),
    ({'jion': 'U0'}, True, 'reaches 0 or below'), ({'jion': 'UNEG'}, True, 'reaches 0 or below'), ({'jion': 'UREV'}, True, 'finite a < b'),
    ({'jion': 'LINF'}, True, 'finite a < b')])
def test_scales_that_cannot_be_sampled_are_refused(scales, has_discharge, match):
    from hallthrusterpem_amd.calibration import noise_scale_table
    from hallthrusterpem_amd.sampling import LOGUNIFORM, NORMAL, UNIFORM, Prior
    named = dict(NORMAL=Prior(NORMAL, 1.0, 0.1, ''), U0=Prior(UNIFORM, 0.0, 2.0, ''), UNEG=Prior(UNIFORM, -1.0, 2.0, ''),
                 UREV=Prior(UNIFORM, 2.0, 1.0, ''), LINF=Prior(LOGUNIFORM, -np.inf, 1.0, ''))
    if isinstance(scales, dict):
        scales = {k: named.get(v, v) if isinstance(v, str) else v for k, v in scales.items()}
    with pytest.raises(ValueError, match=match):
        noise_scale_table(scales, ('V_cc', 'T', 'uion', 'jion'), has_discharge)


def _stub_table():
    """V_cc at 2 conditions, uion at 1 condition x 3 positions, jion at 3 conditions x 4 angles of which one block has 2 records"""
    import torch
    from hallthrusterpem_amd import _lib
    span = np.zeros((6, 4, 2), dtype=np.int32)
    span[0, _lib.SYS_VCC], span[1, _lib.SYS_VCC] = (0, 1), (1, 1)
    span[2, _lib.SYS_UION] = (2, 3)
    for e, n in enumerate((4, 2, 4)):
        span[3 + e, _lib.SYS_JION] = (5 + 5 * e, n)
    return SimpleNamespace(qois=('V_cc', 'uion', 'jion'), conditions={'V_cc': slice(0, 2), 'uion': slice(2, 3), 'jion': slice(3, 6)},
                           span=torch.as_tensor(span), n_cond=6)


def test_the_groups_of_a_table_are_its_qois_with_their_measured_records():
    from hallthrusterpem_amd.calibration import noise_groups
    qois, ends, counts = noise_groups(_stub_table())
    assert qois == ('V_cc', 'uion', 'jion') and ends.tolist() == [2, 3, 6] and counts.tolist() == [2.0, 3.0, 10.0]
    assert ends.dtype == np.int32 and counts.dtype == np.float64
    qois, ends, counts = noise_groups(SimpleNamespace(n_cond=3, n_ang=9))                  # a JionLikelihood: one group
    assert qois == ('jion',) and ends.tolist() == [3] and counts.tolist() == [27.0]
    lik = _stub_table()
    lik.conditions['uion'] = slice(3, 4)
    with pytest.raises(ValueError, match='contiguous ascending block'):
        noise_groups(lik)


def test_a_posterior_refuses_bad_scales_before_it_touches_a_device():
    from hallthrusterpem_amd.calibration import JionPosterior, SurrogatePosterior, SystemPosterior
    lik = SimpleNamespace(use_discharge=True, qois=('V_cc', 'jion'), operating=np.zeros((2, 3)), sweep_radius=1.0, sweep_radii=(1.0,))
    with pytest.raises(ValueError, match="unknown name 'uion'"):
        SystemPosterior(('c0',), lik, n_chains=2, noise_scales=('uion',))
    lik.use_discharge = False
    with pytest.raises(ValueError, match="unknown name 'I_D'"):
        SystemPosterior(('c0',), lik, n_chains=2, noise_scales=('I_D',))
    with pytest.raises(ValueError, match="unknown name 'T'"):
        JionPosterior(('c0',), np.zeros((1, 3)), np.zeros((1, 2)), np.ones((1, 2)), np.ones((1, 2)), n_chains=2, noise_scales=('T',))
    lik.use_discharge = True
    with pytest.raises(ValueError, match='noise_scales needs discharge=None'):
        SurrogatePosterior(('c0',), lik, None, n_chains=2, noise_scales=('jion',))
