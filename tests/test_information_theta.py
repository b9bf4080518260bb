"""The gain about a subset of the inputs on the device (csrc/pem_information_theta.hip, hallthrusterpem_amd/information.py `about=`):
the conditional launch against the long double restatement (tests/information_theta_np.py) over the shapes at which its tiling
changes path, rows that are not finite, its determinism, the closed-form case, and `InformationGain.run` / `by_parameter` on a
small measurement table."""
from functools import lru_cache

import numpy as np
import pytest

import information_np as inf
import information_theta_np as th
from test_information import LAYOUTS, NAMES, THETA, _check, _device, _ends, _table, _vcc_table

pytestmark = pytest.mark.gpu

N_OUT = (1, 5, 33)
N_PER = (1, 63, 64, 65, 257)                     # one tile short, one tile, one tile and a row, five tiles
PAD = 7                                          # records of a row that are no column: NaN, and must not be read


@lru_cache(maxsize=None)
def _operands(layout, n_per):
    """(z_out (33, K), pred (33 n_per, K + PAD), col (K,), scale (K,), z_cond (33, n_per, K), reference lse, ess, used, d2_min):
    computed once, shared, read only.  `col` is a non-monotone choice of K of the K + PAD records, the others are NaN."""
    k, n = int(sum(LAYOUTS[layout])), max(N_OUT)
    rng = np.random.default_rng([17, sorted(LAYOUTS).index(layout), n_per])
    col = rng.permutation(k + PAD)[:k].astype(np.int32)
    assert np.any(np.diff(col) < 0)
    scale = rng.uniform(0.5, 2.0, k)
    pred = np.full((n * n_per, k + PAD), np.nan)
    pred[:, col] = rng.normal(size=(n * n_per, k)) / scale
    z_cond = (pred[:, col] * scale).reshape(n, n_per, k)                           # fp64 products, as the launch rounds them
    z_out = rng.normal(size=(n, k))
    z_out[3] = z_cond[3, n_per // 2]                                               # a row with d2 = 0
    lse, ess, used, low = th.conditional_lse(z_out, z_cond, _ends(LAYOUTS[layout]))
    assert np.all(used == n_per)
    for a in (z_out, pred, col, scale, z_cond, lse, ess, low):
        a.setflags(write=False)
    return z_out, pred, col, scale, z_cond, lse, ess, used, low


def _launch(z_out, pred, n_per, group_end, n_col, col=None, scale=None):
    """pem_conditional_lse_f64_dev on device tensors (any row stride): (lse, ess, used) as numpy"""
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    ge = np.ascontiguousarray(group_end, dtype=np.int32)
    n = z_out.shape[0]
    assert pred.shape[0] == n * n_per
    lse = torch.full((n, ge.size + 1), 7.0, dtype=torch.float64, device='cuda')
    ess = torch.full_like(lse, 7.0)
    used = torch.full((n,), -1, dtype=torch.int32, device='cuda')
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                                            # noqa: E731
    _lib.check(_lib.load().pem_conditional_lse_f64_dev(n, n_per, n_col, p(z_out), z_out.stride(0), p(pred), pred.stride(0), p(col),
                                                       p(scale), ge.size, C.c_void_p(ge.ctypes.data), p(lse), p(ess), p(used),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return lse.cpu().numpy(), ess.cpu().numpy(), used.cpu().numpy()


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.array(a), device='cuda') if dtype is None else torch.as_tensor(np.array(a), device='cuda').to(dtype)


@pytest.mark.parametrize('n_per', N_PER)
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_the_launch_equals_the_long_double_restatement(layout, n_per):
    import torch
    z_out, pred, col, scale, z_cond, ref_lse, ref_ess, ref_used, low = _operands(layout, n_per)
    ge, k = _ends(LAYOUTS[layout]), z_out.shape[1]
    d_pred, d_col, d_scale = _dev(pred), _dev(col), _dev(scale)
    plain = _device(z_cond.reshape(-1, k), pad=2)                    # the products themselves: record k is column k, NaN beyond
    for n_out in N_OUT:
        zo = _device(z_out[:n_out], pad=5)                           # ld_out > n_col, NaN beyond the used columns
        lse, ess, used = _launch(zo, d_pred[:n_out * n_per], n_per, ge, k, d_col, d_scale)
        _check(lse, ess, ref_lse[:n_out], ref_ess[:n_out], low[:n_out], ge, (layout, n_out, n_per))
        assert np.array_equal(used, ref_used[:n_out]) and used.dtype == np.int32
        assert np.all(ess >= 1.0 - 1e-12) and np.all(ess <= n_per * (1 + 1e-12))
        other = _launch(zo, plain[:n_out * n_per], n_per, ge, k)     # null col and scale: the same numbers, so the same bits
        for a, b in zip(other, (lse, ess, used)):
            assert np.array_equal(a, b), (layout, n_out, n_per)
    wide = torch.cat([d_pred, torch.full_like(d_pred[:, :3], float('nan'))], dim=1)[:, :pred.shape[1]]      # ld_pred > the records
    assert wide.stride(0) == pred.shape[1] + 3
    again = _launch(zo, wide, n_per, ge, k, d_col, d_scale)
    assert np.array_equal(again[0], lse) and np.array_equal(again[1], ess)


def test_identical_rows_give_minus_half_d2_and_ess_l():
    rng = np.random.default_rng(31)
    row, z_out = rng.normal(size=(1, 21)), rng.normal(size=(4, 21))
    pred, ge = np.repeat(row, 4 * 130, axis=0), _ends([4, 16, 1])
    lse, ess, used = _launch(_device(z_out), _device(pred), 130, ge, 21)
    ref_lse, ref_ess, ref_used, low = th.conditional_lse(z_out, pred.reshape(4, 130, 21), ge)
    assert np.all(used == 130) and np.all(np.abs(ref_ess - 130) <= 1e-15)
    _check(lse, ess, ref_lse, ref_ess, low, ge, 'identical')


def test_rows_that_are_not_finite_are_left_out_of_every_set_and_counted():
    """NaN, +inf or -inf in ONE column of a row of the set: the row leaves every set, that column's group or not; `used` is exact;
    an outer row whose rows are all bad gives NaN while its neighbours keep their bits.  (Arithmetic on NaN is no fault.)"""
    z_out, pred, col, scale, z_cond, *_ = _operands('straddle', 65)
    ge, k, L = _ends(LAYOUTS['straddle']), z_out.shape[1], 65
    n = 6
    clean = _launch(_device(z_out[:n]), _dev(pred[:n * L]), L, ge, k, _dev(col), _dev(scale))
    bad = np.array(pred[:n * L])
    rng = np.random.default_rng(32)
    rows = {0: [0, 17, 63, 64], 2: list(range(L)), 3: [5], 5: [64]}                # outer row -> its bad rows; row 2: all of them
    for i, ls in rows.items():
        for l in ls:
            bad[i * L + l, col[rng.integers(k)]] = [np.nan, np.inf, -np.inf][l % 3]
    got = _launch(_device(z_out[:n]), _dev(bad), L, ge, k, _dev(col), _dev(scale))
    assert got[2].tolist() == [L - 4, L, 0, L - 1, L, L - 1]
    assert np.all(np.isnan(got[0][2])) and np.all(np.isnan(got[1][2]))
    for i in (1, 4):                                                               # the neighbours of the row without a used row
        assert np.array_equal(got[0][i], clean[0][i]) and np.array_equal(got[1][i], clean[1][i])
    z_bad = (bad[:, col] * scale).reshape(n, L, k)
    ref_lse, ref_ess, ref_used, low = th.conditional_lse(z_out[:n], z_bad, ge)
    assert np.array_equal(got[2], ref_used)
    ok = [0, 1, 3, 4, 5]
    _check(got[0][ok], got[1][ok], ref_lse[ok], ref_ess[ok], low[ok], ge, 'non-finite')
    for i, ls in rows.items():                                                     # and the rows that stay are the whole story
        if i == 2:
            continue
        keep = [l for l in range(L) if l not in ls]
        only = th.conditional_lse(z_out[[i]], z_cond[[i]][:, keep], ge)
        _check(got[0][[i]], got[1][[i]], only[0], only[1], only[3], ge, ('kept rows', i))


def test_a_non_finite_observation_gives_a_row_without_used_rows():
    z_out, pred, col, scale, *_ = _operands('one', 63)
    zo = np.array(z_out[:3])
    zo[1, 4] = np.nan
    lse, ess, used = _launch(_device(zo), _dev(pred[:3 * 63]), 63, _ends(LAYOUTS['one']), zo.shape[1], _dev(col), _dev(scale))
    assert used.tolist() == [63, 0, 63] and np.all(np.isnan(lse[1])) and np.all(np.isfinite(lse[[0, 2]]))


def test_two_calls_give_equal_bits_and_a_row_does_not_depend_on_the_other_rows():
    z_out, pred, col, scale, *_ = _operands('straddle', 257)
    ge, k, L = _ends(LAYOUTS['straddle']), z_out.shape[1], 257
    zo, dp, dc, ds = _device(z_out), _dev(pred), _dev(col), _dev(scale)
    a, b = _launch(zo, dp, L, ge, k, dc, ds), _launch(zo, dp, L, ge, k, dc, ds)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for lo, hi in ((0, 5), (32, 33), (7, 20)):                                     # rows alone: another grid, other strides
        alone = _launch(_device(z_out[lo:hi], pad=1), _device(pred[lo * L:hi * L], pad=2), L, ge, k, dc, ds)
        for x, y in zip(alone, a):
            assert np.array_equal(x, y[lo:hi]), (lo, hi)


def test_the_closed_form_gain_about_theta_through_the_low_level_entries():
    """tests/information_theta_np.py's case, N = M = 2048, L = 256: within 4 standard errors of the exact gains"""
    import torch
    from hallthrusterpem_amd.information import conditional_information, pairwise_information
    z_o, eps, z_i, z_c, ge = th.closed_form_case(seed=0, n=2048, m=2048, l=256)
    about, joint, rest = th.closed_form_exact()
    out = pairwise_information(_dev(z_o), _dev(eps), _dev(z_i), ge)
    cond = conditional_information(_dev(z_o) + _dev(eps), _dev(z_c.reshape(-1, 5)), 256, ge)
    assert int(cond['used'].min()) == 256 == int(cond['used'].max()) and cond['used'].dtype == torch.int32
    half = torch.as_tensor(th.noise_norms(eps, ge).astype(np.float64), device='cuda')
    for name, u, exact in (('about', cond['lse'] - out['lse'], about), ('rest', -0.5 * half - cond['lse'], rest)):
        eig, se = u.mean(dim=0).cpu().numpy(), (u.std(dim=0, unbiased=True) / np.sqrt(2048.0)).cpu().numpy()
        print(name, 'EIG - exact', eig - exact, 'stderr', se)
        assert np.all(np.abs(eig - exact) <= 4.0 * se), (name, eig - exact, se)
    few = slice(0, 48)
    ref = th.conditional_lse((z_o + eps)[few], z_c[few], ge)
    _check(cond['lse'][few].cpu().numpy(), cond['ess'][few].cpu().numpy(), ref[0], ref[1], ref[3], ge, 'closed form')


# ------------------------------------------------------------------------------------------------ InformationGain
@pytest.fixture(scope='module')
def gain():
    from hallthrusterpem_amd.information import InformationGain
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    return InformationGain(Predictive(SystemLikelihood(_table()), NAMES, seed=17))


RUN = dict(n_outer=96, n_inner=160, n_conditional=24, first_index=6)
TENSORS = ('eig', 'stderr', 'lse', 'ess', 'eig_about', 'stderr_about', 'eig_rest', 'stderr_rest', 'lse_cond', 'ess_cond', 'used',
           'ess_cond_median', 'u_about', 'u_rest')


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('samples, about', [(None, ('c0',)), (None, ('T_e', 'c0', 'sigma_cex')), (THETA, NAMES)],
                         ids=['prior-c0', 'prior-three', 'table'])
def test_run_equals_the_restatement_of_what_it_returns(gain, samples, about):
    import torch
    out = gain.run(samples=samples, by='condition', about=about, keep=True, **RUN)
    ge, n, L = out['group_end'], out['n_outer'], 24
    assert out['about'] == tuple(about) and out['n_conditional'] == L and out['z_cond'].shape == (n, L, 19)
    assert out['dropped_conditional'] == 0 and out['used_min'] == L and torch.all(out['used'] == L)
    z_outer, eps, z_inner, z_cond = (_np(out[k]) for k in ('z_outer', 'eps', 'z_inner', 'z_cond'))
    assert np.all(np.isfinite(z_cond))
    ref_lse, ref_ess, low = inf.lse_ess(z_outer, z_inner, ge)
    c_lse, c_ess, c_used, c_low = th.conditional_lse(z_outer, z_cond, ge)
    _check(_np(out['lse_cond']), _np(out['ess_cond']), c_lse, c_ess, c_low, ge, ('run', about))
    # the per-draw gains and their means: each carries the two lse bounds and the roundings of a K_c-term sum of squares, a mean
    # and a standard deviation of N such values carry that and N more roundings (as test_information._stats_equal)
    half = th.noise_norms(eps, ge)
    u_about, u_rest = c_lse - ref_lse, -half / 2 - c_lse
    bound = inf.lse_bound(ge, low) + inf.lse_bound(ge, c_low)
    scale = (half / 2 + np.abs(ref_lse) + np.abs(c_lse)).astype(np.float64)
    tol = bound + 64.0 * inf.U * scale               # (K + 1 <= 20 roundings of |eps_c|^2 in fp64, and the subtractions)
    assert np.all(np.abs(_np(out['u_about']) - u_about) <= tol) and np.all(np.abs(_np(out['u_rest']) - u_rest) <= tol)
    tol_mean = tol.max(axis=0) + (n + 40.0) * inf.U * scale.max(axis=0)
    for key, u in (('about', u_about), ('rest', u_rest)):
        mean, se = th.mean_stderr(u)
        assert np.all(np.abs(_np(out['eig_' + key]) - mean.astype(np.float64)) <= tol_mean), key
        assert np.all(np.abs(_np(out['stderr_' + key]) - se.astype(np.float64)) <= 2.0 * tol_mean / np.sqrt(n)), key
    want = np.median(c_ess, axis=0).astype(np.float64)
    assert np.all(np.abs(_np(out['ess_cond_median']) - want) <= 4.0 * bound.max(axis=0) * want)
    # the chain rule per draw, in fp64: u_about + u_rest = -|eps_c|^2 / 2 - lse up to three roundings
    u = -0.5 * half.astype(np.float64) - _np(out['lse'])
    assert np.all(np.abs(_np(out['u_about']) + _np(out['u_rest']) - u) <= 8.0 * inf.U * scale)
    # the conditional set of draw d: the A-rows of outer draw d, fresh rows for the others, one vector for all conditions,
    # at design indices first_index + (n_outer + n_inner + d L + l) n_cond; the predictions are Predictive's own launch on them
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    pp, nc = gain.pred, gain.pred.lik.n_cond
    table = pp.theta_table(samples)
    with torch.cuda.device(pp.device):
        outer = gain.assemble_shared(table, 96, 6)[:, :96 * nc:nc].clone()
        x = gain.assemble_shared(table, 96 * L, 6 + (96 + 160) * nc)
        fresh = x.clone()
        rows = [COUPLED_INPUTS.index(a) for a in about]
        v = x[:, :96 * L * nc].view(x.shape[0], 96, L * nc)
        v[rows] = outer[rows][:, :, None]
        others = [r for r, name in enumerate(COUPLED_INPUTS) if name not in about]
        assert torch.equal(x[others], fresh[others]) and not torch.equal(x[rows], fresh[rows])
        want = pp.predict(96 * L).index_select(1, pp.cols) * pp.lik.rec[:, 2].index_select(0, pp.cols)
    want = want.index_select(1, torch.as_tensor(out['perm'], device=pp.device)).view(96, L, 19)
    assert out['dropped'][0] == 0 and torch.equal(out['z_cond'], want)


def test_chunks_with_a_ragged_last_one_give_the_bits_of_one_chunk(gain):
    import torch
    nc = gain.pred.lik.n_cond
    one = gain.run(by='qoi', about=('c0', 'T_e'), keep=True, **RUN)
    many = gain.run(by='qoi', about=('c0', 'T_e'), keep=True, chunk_samples=40 * 24 * nc + 5, **RUN)      # 40 + 40 + 16 outer draws
    single = gain.run(by='qoi', about=('c0', 'T_e'), keep=True, chunk_samples=1, **RUN)                    # a draw at a time
    for k in TENSORS + ('z_cond', 'z_outer', 'z_inner', 'eps'):
        assert torch.equal(one[k], many[k]) and torch.equal(one[k], single[k]), k
    assert gain.pred.batch.n == 160 * nc                                           # Predictive's batch kept the inner set's size


def test_without_about_nothing_new_runs_and_every_number_keeps_its_bits(gain):
    import torch
    from hallthrusterpem_amd.information import finite_draws, pairwise_information
    plain = gain.run(samples=THETA, by='condition', keep=True, **RUN)
    assert not {'about', 'eig_about', 'lse_cond', 'used', 'z_cond', 'n_conditional'} & set(plain)
    # the pieces `run` was made of before it knew `about`, composed here
    pp, nc = gain.pred, gain.pred.lik.n_cond
    table = pp.theta_table(THETA)
    with torch.cuda.device(pp.device):
        perm = torch.as_tensor(plain['perm'], device=pp.device)
        z_o, eps = gain.standardised(table, 96, 6, perm), gain.noise(96, 6 // nc, perm)
        z_i = gain.standardised(table, 160, 6 + 96 * nc, perm)
        z_o, eps, z_i, dropped = finite_draws(z_o, eps, z_i, False)
        want = pairwise_information(z_o, eps, z_i, plain['group_end'])
    more = gain.run(samples=THETA, by='condition', keep=True, about=NAMES, **RUN)
    for k in ('eig', 'stderr', 'ess_median', 'ess_min', 'lse', 'ess'):
        assert torch.equal(plain[k], want[k]) and torch.equal(plain[k], more[k]), k
    for k in ('z_outer', 'eps', 'z_inner'):
        assert torch.equal(plain[k], more[k]), k
    assert plain['dropped'] == dropped == more['dropped'] and plain['log_M'] == want['log_M']


def test_about_every_input_leaves_nothing_for_the_rest(gain):
    """about = every non-operating input: every vector of a conditional set IS the outer draw's, so d2c = |Zo - z_o|^2 for every
    row: ess_cond = L, and with Zo = fl(z_o + eps) d2c is |eps_c|^2 up to the rounding of Zo, 2 K u |eps| |Zo| per d2.  So
    u_rest = 0 and u_about = u within information_np.lse_bound plus that (plus the fp64 sum of squares of eps, (K_c + 2) u)."""
    import torch
    from hallthrusterpem_amd.calibration import OPERATING
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    everything = tuple(k for k in COUPLED_INPUTS if k not in OPERATING)
    out = gain.run(by='condition', about=everything, keep=True, **RUN)
    ge, L = out['group_end'], 24
    z_outer, eps, z_cond = (_np(out[k]) for k in ('z_outer', 'eps', 'z_cond'))
    assert np.array_equal(z_cond, np.repeat(z_cond[:, :1], L, axis=1))             # one vector, one prediction
    assert np.array_equal(z_cond[:, 0] + eps, z_outer)                             # and it is the outer draw's
    half = th.noise_norms(eps, ge).astype(np.float64)
    widths = np.diff(np.concatenate([[0], ge, [0]]))
    widths[-1] = ge[-1]
    worst = (np.abs(eps) * np.abs(z_outer)).max(axis=1, keepdims=True)
    tol = inf.lse_bound(ge, half) + 2.0 * widths * inf.U * worst + (widths + 2.0) * inf.U * half / 2
    assert np.all(np.abs(_np(out['ess_cond']) - L) <= 2.0 * inf.lse_bound(ge, half) * L)
    print('max |u_rest| / tol', float((np.abs(_np(out['u_rest'])) / tol).max()))
    assert np.all(np.abs(_np(out['u_rest'])) <= tol)
    u = -0.5 * half - _np(out['lse'])
    slack = tol + 4.0 * inf.U * (np.abs(_np(out['lse'])) + np.abs(_np(out['lse_cond'])) + half)
    assert np.all(np.abs(_np(out['u_about']) - u) <= slack)
    assert np.all(np.abs(_np(out['eig_rest'])) <= tol.max(axis=0))
    assert np.all(np.abs(_np(out['eig_about']) - _np(out['eig'])) <= slack.max(axis=0) + 200 * inf.U * np.abs(u).max(axis=0))


def test_a_parameter_the_group_cannot_see_has_no_gain():
    """about = ('c0',), a plume parameter, against one V_cc record, with n_conditional == n_inner = 256 and N = 1024: lse and
    lse_cond are then log-means of equally many draws of ONE distribution (V_cc does not depend on c0), so the expectation of
    u_about is exactly 0, the nested estimator's bias included"""
    from hallthrusterpem_amd.information import InformationGain
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    ig = InformationGain(Predictive(SystemLikelihood(_vcc_table(1, 4.0)), ('c0', 'T_e'), seed=29))
    out = ig.run(n_outer=1024, n_inner=256, n_conditional=256, by='qoi', about=('c0',))
    eig, se = _np(out['eig_about']), _np(out['stderr_about'])
    print('eig_about', eig, 'stderr', se, 'eig', _np(out['eig']), 'eig_rest', _np(out['eig_rest']), 'ess_cond', _np(out['ess_cond_median']))
    assert out['labels'] == ['V_cc', 'all'] and out['dropped_conditional'] == 0
    assert np.all(se > 0) and np.all(np.abs(eig) <= 4.0 * se), (eig, se)


def test_by_parameter_rows_are_separate_runs(gain):
    import torch
    kw = dict(by='condition', **RUN)
    both = gain.by_parameter(**kw)
    assert both['names'] == list(NAMES) and both['labels'] == ['V_cc[0]', 'jion[0]', 'jion[1]', 'all']
    assert both['eig_about'].shape == (2, 4) and both['n_conditional'] == 24
    for p, name in enumerate(NAMES):
        one = gain.run(about=(name,), **kw)
        for k in ('eig_about', 'stderr_about', 'eig_rest', 'stderr_rest', 'ess_cond_median'):
            assert torch.equal(both[k][p], one[k]), (name, k)
        assert both['used_min'][p] == one['used_min'] and both['dropped_conditional'][p] == one['dropped_conditional']
        for k in ('eig', 'stderr', 'lse'):
            assert torch.equal(both['joint'][k], one[k]), k
    lines = both['table'].splitlines()
    assert len(lines) == 4 and lines[1].split()[0] == 'c0' and lines[2].split()[0] == 'T_e' and 'jion[1]' in lines[0]
    with pytest.raises(ValueError, match='missing'):
        gain.by_parameter(samples=THETA, **kw)
    text = gain.table(gain.run(about=NAMES, **kw))
    assert 'about = c0, T_e' in text and 'ess cond' in text and 'about' not in gain.table(both['joint'])


def test_the_example_runs():
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    out = subprocess.run([sys.executable, str(root / 'examples' / 'parameter_information.py'), '256', '32'], capture_output=True, text=True,
                         timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    for text in ('which measurement informs which parameter', 'EIG about', 'gain about the calibrated parameters together'):
        assert text in out.stdout, (text, out.stdout)
