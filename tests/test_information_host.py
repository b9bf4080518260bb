"""Expected information gain without a GPU: the long double restatement (tests/information_np.py) is the estimator -- it recovers a
closed form and has the stated identities; the entry points of csrc/pem_information.hip are declared, bound, built and exported
and refuse every malformed call before they look for a device; hallthrusterpem_amd.information refuses what it cannot run on the
host."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import information_np as inf

ROOT = Path(__file__).resolve().parents[1]
NAME, WORK = 'pem_pairwise_lse_f64_dev', 'pem_pairwise_lse_work_len'
FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host


# ------------------------------------------------------------------------------------------------ the estimator
@pytest.fixture(scope='module')
def closed_form():
    z_o, eps, z_i, ge, exact = inf.closed_form_case(seed=0, n=2048, m=2048)
    return inf.estimate(z_o, eps, z_i, ge), exact


def test_the_restatement_recovers_the_closed_form_gain(closed_form):
    """theta ~ N(0, 1), g_k = a_k theta, a = (1, 1, 1, 1, 2), unit sigma: EIG = 1/2 log(1 + sum a^2) = 1/2 log 4, 1/2 log 6 and
    1/2 log 9 for {0, 1, 2}, {3, 4} and all five.  Seed 0, N = M = 2048: off by +0.008, -0.020 and -0.013 against standard
    errors of 0.019, 0.021 and 0.022; over seeds 0-3 and N = M = 1024, 2048 the worst case was 2.2 standard errors."""
    est, exact = closed_form
    err = np.abs(est['eig'].astype(np.float64) - exact)
    print('EIG - exact', est['eig'].astype(np.float64) - exact, 'stderr', est['stderr'].astype(np.float64))
    assert np.all(err <= 4.0 * est['stderr'].astype(np.float64)), (err, est['stderr'])
    assert np.all(est['stderr'] > 0.005) and np.all(est['stderr'] < 0.05)
    assert np.all(est['ess_min'] >= 1.0) and np.all(est['ess'] <= 2048 * (1 + 1e-12))
    assert np.all(est['eig'] < np.log(2048.0))


@pytest.fixture(scope='module')
def small():
    rng = np.random.default_rng(11)
    z_o, eps, z_i = rng.normal(size=(9, 7)) * 2.0, rng.normal(size=(9, 7)), rng.normal(size=(13, 7)) * 2.0
    return z_o, eps, z_i


def test_the_unions_d2_is_the_sum_of_the_groups(small):
    z_o, eps, z_i = small
    d2 = inf.pairwise_d2(z_o + eps, z_i, [2, 3, 7])
    assert d2.shape == (4, 9, 13)
    assert np.array_equal(d2[3], d2[0] + d2[1] + d2[2])
    direct = (((z_o + eps)[:, None, :].astype(inf.LD) - z_i[None].astype(inf.LD)) ** 2).sum(axis=2)
    assert np.max(np.abs(d2[3] - direct)) <= 16 * np.finfo(inf.LD).eps * direct.max()


def test_one_group_of_everything_is_the_union(small):
    z_o, eps, z_i = small
    one = inf.estimate(z_o, eps, z_i, [7])
    for k in ('lse', 'ess', 'u'):
        assert np.array_equal(one[k][:, 0], one[k][:, 1]), k
    many = inf.estimate(z_o, eps, z_i, [2, 3, 7])
    tol = 64 * np.finfo(inf.LD).eps
    assert np.max(np.abs(many['lse'][:, 3] - one['lse'][:, 0])) <= tol * np.abs(one['lse']).max()
    assert np.max(np.abs(many['eig'][3] - one['eig'][0])) <= tol * abs(one['eig'][0])


def test_scaling_a_column_with_its_sigma_changes_nothing():
    """a column g_k with sigma_k and 8 g_k with 8 sigma_k standardise to the same bits (a power of two), so the estimate is the same"""
    rng = np.random.default_rng(12)
    g_o, g_i, sigma = rng.normal(size=(9, 5)), rng.normal(size=(13, 5)), rng.uniform(0.5, 2.0, 5)
    eps = rng.normal(size=(9, 5))
    scale = np.array([1.0, 8.0, 1.0, 0.25, 1.0])
    a = inf.estimate(g_o / sigma, eps, g_i / sigma, [2, 5])
    b = inf.estimate((g_o * scale) / (sigma * scale), eps, (g_i * scale) / (sigma * scale), [2, 5])
    for k in ('lse', 'ess', 'eig', 'stderr'):
        assert np.array_equal(a[k], b[k]), k


def test_an_outer_row_next_to_one_inner_row_only_has_ess_one():
    z_i = np.arange(6, dtype=np.float64)[:, None] * 100.0 * np.ones((1, 3))
    z_o = z_i[[2]] + 0.01
    lse, ess, low = inf.lse_ess(z_o, z_i, [1, 3])
    assert np.all(np.abs(ess - 1.0) <= 1e-18)
    assert np.allclose((lse + low / 2 + np.log(inf.LD(6))).astype(np.float64), 0.0, atol=1e-18)


def test_a_reused_inner_set_bounds_the_estimate_by_log_m_and_a_separate_one_does_not():
    """with the term j = i in the sum d2(i, i) = |eps_i|^2 <= every other way to write d2_min, so u_i <= log M; with a separate
    inner set a saturated group (here: 30 columns, 64 draws) goes far above log M -- it is no lower bound"""
    rng = np.random.default_rng(13)
    z, eps, z_other = rng.normal(size=(64, 30)) * 3.0, rng.normal(size=(64, 30)), rng.normal(size=(64, 30)) * 3.0
    reused = inf.estimate(z, eps, z, [1, 30])
    assert np.all(reused['u'] <= np.log(inf.LD(64)) + 1e-12) and np.all(reused['eig'] <= np.log(64.0) + 1e-12)
    assert np.median(reused['ess'][:, 2]) < 1.01 and reused['eig'][2] > np.log(64.0) - 0.01          # saturated: the bound is met
    separate = inf.estimate(z, eps, z_other, [1, 30])
    assert np.median(separate['ess'][:, 2]) < 1.5 and separate['eig'][2] > 10.0 * np.log(64.0)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_points_are_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % NAME, header)
    assert m and len(m.group(1).split(',')) == 14 == len(_lib.SIGNATURES[NAME][1])
    m = re.search(r'\bsize_t\s+%s\s*\(([^)]*)\)' % WORK, header)
    assert m and len(m.group(1).split(',')) == 3 == len(_lib.SIGNATURES[WORK][1])
    assert hasattr(_lib.load(), NAME) and hasattr(_lib.load(), WORK)
    for macro, value in (('PEM_INFORMATION_MAX_GROUPS', _lib.INFORMATION_MAX_GROUPS), ('PEM_INFORMATION_CHUNK', _lib.INFORMATION_CHUNK),
                         ('PEM_INFORMATION_INNER_BLOCK', _lib.INFORMATION_INNER_BLOCK)):
        assert re.search(r'#define %s (\d+)' % macro, header).group(1) == str(value)
    assert _lib.INFORMATION_MAX_GROUPS == 32
    assert build.PKG / 'csrc' / 'pem_information.hip' in build.SRCS


def _call(n_out=5, n_in=7, n_col=6, ld_out=6, ld_in=8, group_end=(2, 6), n_groups=None, work_len=None, **null):
    from hallthrusterpem_amd import _lib
    lib = _lib.load()
    ge = np.asarray(group_end, dtype=np.int32)
    n_groups = ge.size if n_groups is None else n_groups
    if work_len is None:
        work_len = max(int(lib.pem_pairwise_lse_work_len(n_out, n_in, n_groups)), 1)
    p = {k: None if null.get(k) else FAKE for k in ('z_out', 'z_in', 'lse', 'ess', 'work')}
    return lib.pem_pairwise_lse_f64_dev(n_out, n_in, n_col, p['z_out'], ld_out, p['z_in'], ld_in, n_groups,
                                        None if null.get('group_end_null') else C.c_void_p(ge.ctypes.data), p['lse'], p['ess'], p['work'],
                                        work_len, None)


BAD = [dict(n_out=0), dict(n_in=0), dict(n_col=0), dict(n_col=-1), dict(ld_out=5), dict(ld_in=5), dict(n_groups=0),
       dict(group_end=tuple(range(1, 34)), n_col=33, ld_out=33, ld_in=33), dict(group_end=(0, 6)), dict(group_end=(3, 3, 6)),
       dict(group_end=(4, 2, 6)), dict(group_end=(2, 5)), dict(group_end=(2, 7)), dict(group_end=(6, 7)), dict(group_end=(-1, 6)),
       dict(work_len=5 * 3 * 3 - 1), dict(n_in=1025, work_len=2 * 5 * 3 * 3), dict(n_in=65536 * 512),
       dict(n_col=2 ** 31 - 1, ld_out=2 ** 31, ld_in=2 ** 31, group_end=(2, 2 ** 31 - 1)),
       dict(z_out=True), dict(z_in=True), dict(group_end_null=True), dict(lse=True), dict(ess=True), dict(work=True)]


@pytest.mark.parametrize('bad', BAD)
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_pairwise_lse' in _lib.load().pem_last_error()


def test_well_formed_calls_get_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _call() == _lib.PEM_ERR_NO_DEVICE
    assert _call(n_out=1, n_in=1, n_col=1, ld_out=1, ld_in=1, group_end=(1,)) == _lib.PEM_ERR_NO_DEVICE
    assert _call(group_end=tuple(range(1, 33)), n_col=32, ld_out=40, ld_in=32) == _lib.PEM_ERR_NO_DEVICE
    assert _call(n_in=1025, work_len=3 * 5 * 3 * 3) == _lib.PEM_ERR_NO_DEVICE


def test_the_work_length_is_one_state_per_block_row_and_set():
    from hallthrusterpem_amd import _lib
    f = _lib.load().pem_pairwise_lse_work_len
    block = _lib.INFORMATION_INNER_BLOCK
    assert f(5, 7, 2) == 5 * 3 * 3 and f(5, block, 2) == 5 * 3 * 3 and f(5, block + 1, 2) == 2 * 5 * 3 * 3
    assert f(4096, 4096, 16) == (4096 // block) * 4096 * 17 * 3
    assert f(0, 7, 2) == 0 and f(5, 0, 2) == 0 and f(5, 7, 0) == 0 and f(5, 7, 33) == 0 and f(2 ** 62, 7, 2) == 0


# ------------------------------------------------------------------------------------------------ the Python layer
def test_group_columns_makes_the_groups_contiguous():
    from hallthrusterpem_amd.information import check_group_end, group_columns
    perm, ge, values = group_columns([1, 0, 1, 2, 0, 1])
    assert perm.tolist() == [1, 4, 0, 2, 5, 3] and ge.tolist() == [2, 5, 6] and values.tolist() == [0, 1, 2]
    assert ge.dtype == np.int32 and check_group_end(ge, 6).tolist() == [2, 5, 6]
    perm, ge, _ = group_columns(np.arange(32))
    assert perm.tolist() == list(range(32)) and ge.tolist() == list(range(1, 33))


@pytest.mark.parametrize('labels, match', [(np.arange(33), 'at most PEM_INFORMATION_MAX_GROUPS'), ([0, 2, 2], 'group 1 is empty'),
                                           ([0, -1], '0 ... G-1'), ([0.0, 1.0], 'one integer per column'), ([], 'one integer per column'),
                                           ([[0, 1]], 'one integer per column')])
def test_group_columns_refuses_too_many_and_empty_groups(labels, match):
    from hallthrusterpem_amd.information import group_columns
    with pytest.raises(ValueError, match=match):
        group_columns(labels)


@pytest.mark.parametrize('ge, n_col, match', [([], 4, 'non-empty'), ([2.0, 4.0], 4, 'integers'), (list(range(1, 34)), 33, 'at most'),
                                              ([0, 4], 4, 'ascend'), ([2, 2, 4], 4, 'ascend'), ([3, 2, 4], 4, 'ascend'),
                                              ([2, 3], 4, 'end at'), ([2, 5], 4, 'end at')])
def test_group_ends_are_checked_on_the_host(ge, n_col, match):
    from hallthrusterpem_amd.information import check_group_end
    with pytest.raises(ValueError, match=match):
        check_group_end(ge, n_col)


def _stub_predictive():
    """the fields InformationGain reads, on the host: V_cc at 2 conditions, jion at 3 conditions x 4 angles (blocks padded to odd)"""
    import torch
    from hallthrusterpem_amd import _lib
    span = np.zeros((5, 4, 2), dtype=np.int32)
    span[0, _lib.SYS_VCC], span[1, _lib.SYS_VCC] = (0, 1), (1, 1)
    for e in range(3):
        span[2 + e, _lib.SYS_JION] = (2 + 5 * e, 4)
    rec = np.zeros((17, 4))
    rec[:, 2] = 1.0 / np.arange(1, 18)
    cols = [0, 1] + [2 + 5 * e + a for e in range(3) for a in range(4)]
    lik = SimpleNamespace(qois=('V_cc', 'jion'), conditions={'V_cc': slice(0, 2), 'jion': slice(2, 5)}, span=torch.as_tensor(span),
                          rec=torch.as_tensor(rec), n_cond=5)
    return SimpleNamespace(lik=lik, cols=torch.as_tensor(cols), sigma=torch.full((14,), 7.0))


def test_the_groups_of_a_table_and_its_own_standard_deviations():
    from hallthrusterpem_amd.information import InformationGain
    ig = InformationGain(_stub_predictive())
    want = 1.0 / (1.0 + np.array([0, 1] + [2 + 5 * e + a for e in range(3) for a in range(4)]))
    assert np.array_equal(ig.inv_std.numpy(), want)                       # the records' own 1 / std, not Predictive.sigma
    perm, ge, labels = ig.groups('qoi')
    assert perm.tolist() == list(range(14)) and ge.tolist() == [2, 14] and labels == ['V_cc', 'jion']
    perm, ge, labels = ig.groups('condition')
    assert perm.tolist() == list(range(14)) and ge.tolist() == [1, 2, 6, 10, 14]
    assert labels == ['V_cc[0]', 'V_cc[1]', 'jion[0]', 'jion[1]', 'jion[2]']
    perm, ge, labels = ig.groups(np.arange(14) % 3)
    assert perm.tolist() == [0, 3, 6, 9, 12, 1, 4, 7, 10, 13, 2, 5, 8, 11] and ge.tolist() == [5, 10, 14] and labels == [0, 1, 2]
    for by, match in (('dataset', "by: 'qoi', 'condition'"), (np.arange(13), 'one label per compact column'),
                      (np.arange(14) * 2, 'is empty'), (np.arange(14) + 20, 'at most')):
        with pytest.raises(ValueError, match=match):
            ig.groups(by)


def test_a_block_without_measured_records_makes_no_group():
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd.information import InformationGain
    pred = _stub_predictive()
    span = pred.lik.span.numpy().copy()
    span[3, _lib.SYS_JION] = (7, 0)                                       # jion[1] has no measured record
    pred.lik.span = torch.as_tensor(span)
    pred.cols = torch.as_tensor([0, 1] + [2 + 5 * e + a for e in (0, 2) for a in range(4)])
    ig = InformationGain(pred)
    perm, ge, labels = ig.groups('condition')
    assert ge.tolist() == [1, 2, 6, 10] and labels == ['V_cc[0]', 'V_cc[1]', 'jion[0]', 'jion[2]'] and perm.tolist() == list(range(10))


def test_the_table_says_what_a_saturated_number_means_for_the_inner_set_used():
    import torch
    from hallthrusterpem_amd.information import InformationGain
    ig = InformationGain(_stub_predictive())
    res = dict(eig=torch.tensor([0.5, 9.0]), stderr=torch.tensor([0.01, 0.5]), ess_median=torch.tensor([40.0, 1.0]),
               ess_min=torch.tensor([3.0, 1.0]), labels=['V_cc', 'all'], log_M=4.0)
    text = ig.table(dict(res, reuse=False)).splitlines()
    assert 'all' in text[1] and 'biased upward, unreliable' in text[1] and 'lower bound' not in text[1] and 'saturated' not in text[2]
    text = ig.table(dict(res, reuse=True)).splitlines()
    assert 'saturated: a lower bound' in text[1] and 'saturated' not in text[2]


def test_run_refuses_bad_counts_before_any_launch():
    from hallthrusterpem_amd.information import InformationGain
    ig = InformationGain(_stub_predictive())
    for kw in (dict(n_outer=0), dict(n_inner=0), dict(n_outer=2.5), dict(first_index=-1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ig.run(**kw)
    with pytest.raises(ValueError, match="by: 'qoi'"):
        ig.run(by='record')


def test_the_low_level_entry_checks_its_operands_on_the_host():
    import torch
    from hallthrusterpem_amd.information import pairwise_information
    z = torch.zeros((4, 6), dtype=torch.float64)
    for args, match in (((z.float(), z, z, [6]), 'z_in_outer: a 2-D float64'), ((z, z[:3], z, [6]), 'shapes'),
                        ((z, z, z[:, :5], [6]), 'shapes'), ((z, z, z, [2, 5]), 'end at'), ((z, z, z, [6, 6]), 'ascend'),
                        ((z[:0], z[:0], z, [6]), 'empty operands'), ((z, z, z, [6]), 'no CPU path')):
        with pytest.raises(ValueError, match=match):
            pairwise_information(*args)


def test_non_finite_draws_are_dropped_from_both_sets_and_counted():
    import torch
    from hallthrusterpem_amd.information import finite_draws
    g = torch.Generator().manual_seed(3)
    z_o, eps, z_i = (torch.randn((n, 4), dtype=torch.float64, generator=g) for n in (6, 6, 5))
    z_o[2, 1], z_i[0, 3], z_i[4, 0] = float('nan'), float('inf'), float('-inf')
    a, e, b, dropped = finite_draws(z_o, eps, z_i)
    keep = [0, 1, 3, 4, 5]
    assert dropped == (1, 2) and torch.equal(a, z_o[keep]) and torch.equal(e, eps[keep]) and torch.equal(b, z_i[1:4])
    a, e, b, dropped = finite_draws(z_o, eps, z_i, reuse=True)
    assert dropped == (1, 1) and b is a and torch.equal(a, z_o[keep])
    a, e, b, dropped = finite_draws(z_i[1:4], eps[:3], z_o[3:])
    assert dropped == (0, 0) and a.shape == (3, 4) and b.shape == (3, 4)
    z_i[1:3] = float('nan')
    with pytest.raises(ValueError, match='fewer than two draws'):
        finite_draws(z_o, eps, z_i)
