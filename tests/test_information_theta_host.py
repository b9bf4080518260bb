"""The gain about a subset of the inputs without a GPU: the long double restatement (tests/information_theta_np.py) recovers a
closed form and obeys the chain rule per draw; the entry point of csrc/pem_information_theta.hip is declared, bound, built and
exported and refuses every malformed call before it looks for a device; `InformationGain`'s rules for `about` raise as stated."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import information_np as inf
import information_theta_np as th
from test_information_host import _stub_predictive

ROOT = Path(__file__).resolve().parents[1]
NAME = 'pem_conditional_lse_f64_dev'
FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host


# ------------------------------------------------------------------------------------------------ the estimator
@pytest.fixture(scope='module')
def closed_form():
    return th.estimate(*th.closed_form_case(seed=0, n=2048, m=2048, l=256)), th.closed_form_exact()


def test_the_restatement_recovers_the_closed_form_gain_about_theta(closed_form):
    """theta, eta ~ N(0, 1), g = a theta + b eta, a = (1, 1, 1, 1, 2), b = (.5, -1, 2, 0, 1), unit sigma, groups {0, 1, 2}, {3, 4}
    and their union: EIG_theta = 1/2 [log det(I + a a^T + b b^T) - log det(I + b b^T)] on each set; N = M = 2048, L = 256,
    within 4 standard errors (seeds 0-5 were all within 2)."""
    est, (about, joint, rest) = closed_form
    for key, exact in (('eig_about', about), ('eig', joint), ('eig_rest', rest)):
        got, se = est[key].astype(np.float64), est[key.replace('eig', 'stderr')].astype(np.float64)
        print(key, 'estimate - exact', got - exact, 'stderr', se)
        assert np.all(np.abs(got - exact) <= 4.0 * se), (key, got - exact, se)
        assert np.all(se > 0.002) and np.all(se < 0.05), (key, se)
    assert np.all(about > 0.3) and np.all(rest > 0.2)                              # the case splits the gain both ways
    assert est['dropped_conditional'] == 0 and np.all(est['used'] == 256)
    assert np.all(est['ess_cond'] >= 1.0) and np.all(est['ess_cond'] <= 256 * (1 + 1e-12))
    assert np.all(np.median(est['ess_cond'], axis=0) > 8.0)                        # the conditional sums are not saturated


def test_the_chain_rule_holds_for_every_draw(closed_form):
    """u = u_about + u_rest: lse_cond cancels, up to the roundings of two long double additions"""
    est, _ = closed_form
    scale = np.abs(est['u']) + np.abs(est['lse_cond']) + np.abs(est['lse'])
    assert np.all(np.abs(est['u_about'] + est['u_rest'] - est['u']) <= 4 * np.finfo(inf.LD).eps * scale)
    tol = 64 * np.finfo(inf.LD).eps * 2048
    assert np.all(np.abs(est['eig_about'] + est['eig_rest'] - est['eig']) <= tol)


def test_a_set_of_the_outer_rows_themselves_gives_no_rest():
    """every row of the conditional set equal to the outer prediction: d2c = |eps|^2 for every row, lse_cond = -|eps|^2 / 2, ess = L,
    so u_rest = 0 and u_about = u"""
    rng = np.random.default_rng(21)
    z_o, eps, z_i = rng.normal(size=(9, 7)) * 2.0, rng.normal(size=(9, 7)), rng.normal(size=(13, 7)) * 2.0
    est = th.estimate(z_o, eps, z_i, np.repeat(z_o[:, None, :], 6, axis=1), [2, 3, 7])
    assert np.all(np.abs(est['ess_cond'] - 6) <= 1e-15) and np.all(est['used'] == 6)
    # (the observations are the fp64 numbers z + eps: d2c is |eps|^2 up to their rounding, 2 K u |eps| |Zo| per d2)
    zo = np.abs(z_o + eps)
    slack = 2 * 7 * inf.U * np.stack([(np.abs(eps) * zo)[:, sl].sum(axis=1) for sl in inf.group_slices([2, 3, 7])]
                                     + [(np.abs(eps) * zo).sum(axis=1)], axis=1)
    assert np.all(np.abs(est['u_rest']) <= slack) and np.all(np.abs(est['u_about'] - est['u']) <= slack)


def test_rows_that_are_not_finite_are_left_out_of_every_set():
    rng = np.random.default_rng(22)
    z_o, eps, z_i, z_c = rng.normal(size=(4, 5)), rng.normal(size=(4, 5)), rng.normal(size=(6, 5)), rng.normal(size=(4, 7, 5))
    z_c[0, 2, 4], z_c[0, 5, 0], z_c[1, :, 3], z_c[2, 0, 1] = np.nan, np.inf, np.nan, -np.inf
    est = th.estimate(z_o, eps, z_i, z_c, [1, 5])
    assert est['used'].tolist() == [5, 0, 6, 7] and est['dropped_conditional'] == 1
    assert np.all(np.isnan(est['lse_cond'][1])) and np.all(np.isfinite(est['lse_cond'][[0, 2, 3]]))
    clean = th.estimate(z_o[[0]], eps[[0]], z_i, z_c[[0]][:, [0, 1, 3, 4, 6]], [1, 5])      # group 0 does not hold the bad columns
    assert np.array_equal(clean['lse_cond'][0], est['lse_cond'][0]) and np.array_equal(clean['ess_cond'][0], est['ess_cond'][0])
    assert np.all(np.isfinite(est['eig_about'])) and np.all(np.isfinite(est['eig']))
    keep = [0, 2, 3]
    assert np.array_equal(est['eig'], est['u'][keep].mean(axis=0)) and np.array_equal(est['eig_rest'], est['u_rest'][keep].mean(axis=0))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_point_is_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % NAME, header)
    assert m and len(m.group(1).split(',')) == 15 == len(_lib.SIGNATURES[NAME][1])
    assert [a.split()[-1].lstrip('*') for a in m.group(1).split(',')] == [
        'n_out', 'n_per', 'n_col', 'z_out', 'ld_out', 'pred', 'ld_pred', 'col', 'scale', 'n_groups', 'group_end', 'lse', 'ess', 'used',
        'stream']
    assert _lib.SIGNATURES[NAME][0] is C.c_int and hasattr(_lib.load(), NAME)
    assert re.search(r'#define PEM_CONDITIONAL_CHUNK (\d+)', header).group(1) == str(_lib.CONDITIONAL_CHUNK)
    src = build.PKG / 'csrc' / 'pem_information_theta.hip'
    assert src in build.SRCS and build.SRCS.count(src) == 1 and src.exists()
    assert 'extern "C" int %s(' % NAME in src.read_text()
    assert NAME not in (build.PKG / 'csrc' / 'pem_information.hip').read_text()


def _call(n_out=5, n_per=7, n_col=6, ld_out=6, ld_pred=9, group_end=(2, 6), n_groups=None, **null):
    from hallthrusterpem_amd import _lib
    ge = np.asarray(group_end, dtype=np.int32)
    p = {k: None if null.get(k) else FAKE for k in ('z_out', 'pred', 'col', 'scale', 'lse', 'ess', 'used')}
    return _lib.load().pem_conditional_lse_f64_dev(n_out, n_per, n_col, p['z_out'], ld_out, p['pred'], ld_pred, p['col'], p['scale'],
                                                   ge.size if n_groups is None else n_groups,
                                                   None if null.get('group_end_null') else C.c_void_p(ge.ctypes.data), p['lse'], p['ess'],
                                                   p['used'], None)


BAD = [dict(n_out=0), dict(n_per=0), dict(n_col=0), dict(n_col=-1), dict(ld_out=5), dict(ld_pred=0), dict(n_groups=0), dict(n_groups=33),
       dict(group_end=tuple(range(1, 34)), n_col=33, ld_out=33, ld_pred=33), dict(group_end=(0, 6)), dict(group_end=(3, 3, 6)),
       dict(group_end=(4, 2, 6)), dict(group_end=(2, 5)), dict(group_end=(2, 7)), dict(group_end=(6, 7)), dict(group_end=(-1, 6)),
       dict(z_out=True), dict(pred=True), dict(group_end_null=True), dict(lse=True), dict(ess=True), dict(used=True),
       dict(ld_pred=5, col=True),                                                   # the identity needs a record per column
       dict(n_out=2 ** 33, n_per=2 ** 33), dict(n_out=2 ** 31, n_per=2 ** 31, ld_pred=2 ** 2), dict(n_out=2 ** 30, n_per=2 ** 30, ld_pred=2),
       dict(n_out=2 ** 40, ld_out=2 ** 24), dict(n_out=2 ** 61, n_per=1, ld_pred=1, ld_out=6)]


@pytest.mark.parametrize('bad', BAD)
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert NAME[:-len('_f64_dev')].encode() in _lib.load().pem_last_error()


def test_well_formed_calls_get_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _call() == _lib.PEM_ERR_NO_DEVICE
    assert _call(col=True, scale=True) == _lib.PEM_ERR_NO_DEVICE                   # both are optional
    assert _call(n_out=1, n_per=1, n_col=1, ld_out=1, ld_pred=1, group_end=(1,)) == _lib.PEM_ERR_NO_DEVICE
    assert _call(ld_pred=1) == _lib.PEM_ERR_NO_DEVICE                              # with col any row length
    assert _call(group_end=tuple(range(1, 33)), n_col=32, ld_out=40, ld_pred=32, col=True) == _lib.PEM_ERR_NO_DEVICE


# ------------------------------------------------------------------------------------------------ the Python layer
def test_about_is_a_non_empty_set_of_non_operating_inputs():
    from hallthrusterpem_amd.information import InformationGain
    ig = InformationGain(_stub_predictive())
    ig.pred.names = ('c0', 'T_e')
    assert ig.check_about('c0') == ('c0',) and ig.check_about(['T_e', 'sigma_cex']) == ('T_e', 'sigma_cex')
    for about, match in (((), 'at least one'), (('P_b',), 'not a non-operating input'), (('nonsense',), 'not a non-operating input'),
                         (('c0', 'c0'), 'repeat')):
        with pytest.raises(ValueError, match=match):
            ig.check_about(about)
        with pytest.raises(ValueError, match=match):
            ig.run(about=about)


def test_with_a_theta_table_about_must_hold_every_theta_name():
    from hallthrusterpem_amd.information import InformationGain
    ig = InformationGain(_stub_predictive())
    ig.pred.names = ('c0', 'T_e')
    table = np.zeros((4, 2))
    assert ig.check_about(('T_e', 'c0'), table) == ('T_e', 'c0')
    assert ig.check_about(('c0', 'sigma_cex', 'T_e'), table) == ('c0', 'sigma_cex', 'T_e')      # it may add prior-drawn inputs
    with pytest.raises(ValueError, match=r"missing \['T_e'\]"):
        ig.check_about(('c0',), table)
    with pytest.raises(ValueError, match=r"missing \['c0', 'T_e'\]"):
        ig.run(samples=table, about=('sigma_cex',))
    with pytest.raises(ValueError, match=r"missing \['T_e'\]"):
        ig.by_parameter(samples=table)
    assert ig.check_about(('c0',), None) == ('c0',)                                # independent priors: any subset


def test_run_refuses_bad_conditional_counts_before_any_launch():
    from hallthrusterpem_amd.information import InformationGain
    ig = InformationGain(_stub_predictive())
    ig.pred.names = ('c0',)
    for kw in (dict(n_conditional=0), dict(n_conditional=1.5), dict(chunk_samples=0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ig.run(about='c0', **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            ig.by_parameter(**kw)


def test_the_low_level_entry_checks_its_operands_on_the_host():
    import torch
    from hallthrusterpem_amd.information import conditional_information
    z, p = torch.zeros((4, 6), dtype=torch.float64), torch.zeros((12, 9), dtype=torch.float64)
    col = torch.arange(6)
    for args, kw, match in (((z.float(), p, 3, [6]), {}, 'z_out: a 2-D float64'), ((z, p.float(), 3, [6]), {}, 'pred: a 2-D float64'),
                            ((z, p, 0, [6]), {}, 'n_per'), ((z, p, 4, [6]), {}, 'rows'), ((z, p, 3, [2, 5]), {}, 'end at'),
                            ((z, p[:, :5], 3, [6]), {}, 'no col'), ((z, p, 3, [6]), dict(col=col[:5]), 'col: one int32 or int64'),
                            ((z, p, 3, [6]), dict(col=col.double()), 'col: one int32 or int64'),
                            ((z, p, 3, [6]), dict(scale=torch.ones(5, dtype=torch.float64)), 'scale: one float64'),
                            ((z[:0], p[:0], 3, [6]), {}, 'empty operands'), ((z, p, 3, [6]), dict(col=col), 'no CPU path')):
        with pytest.raises(ValueError, match=match):
            conditional_information(*args, **kw)


def test_the_table_prints_the_new_columns_only_when_they_are_present():
    import torch
    from hallthrusterpem_amd.information import InformationGain
    ig = InformationGain(_stub_predictive())
    res = dict(eig=torch.tensor([0.5, 2.0]), stderr=torch.tensor([0.01, 0.05]), ess_median=torch.tensor([40.0, 30.0]),
               ess_min=torch.tensor([3.0, 2.0]), labels=['V_cc', 'all'], log_M=4.0, reuse=False)
    plain = ig.table(res)
    assert 'about' not in plain and 'ess cond' not in plain and len(plain.splitlines()[1].split()) == 5
    more = dict(res, about=('c0', 'T_e'), n_conditional=64, eig_about=torch.tensor([0.125, 1.5]), stderr_about=torch.tensor([0.02, 0.04]),
                eig_rest=torch.tensor([0.375, 0.5]), stderr_rest=torch.tensor([0.03, 0.06]), ess_cond_median=torch.tensor([20.0, 10.0]))
    text = ig.table(more).splitlines()
    assert 'about = c0, T_e' in text[0] and 'L = 64' in text[0] and 'ess cond' in text[0]
    assert text[1].split() == ['all', '2.000', '0.050', '30.0', '2.00', '1.500', '0.040', '0.500', '0.060', '10.0']
    assert text[2].split()[5:] == ['0.125', '0.020', '0.375', '0.030', '20.0']
