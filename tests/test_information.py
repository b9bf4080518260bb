"""Expected information gain on the device (csrc/pem_information.hip, hallthrusterpem_amd/information.py): the fused pairwise
launch against the long double restatement (tests/information_np.py) over the shapes at which its tiling changes path, its
determinism, the closed-form case, and `InformationGain.run` on a small measurement table."""
from functools import lru_cache

import numpy as np
import pytest

import information_np as inf

pytestmark = pytest.mark.gpu

CHUNK = 16                                       # PEM_INFORMATION_CHUNK (asserted below)
# group widths: straddling the staging chunk; one group; 32 groups; groups that end on the chunk boundaries
LAYOUTS = {
    'straddle': [CHUNK - 1, CHUNK, CHUNK + 1, 1],
    'one': [2 * CHUNK + 1],
    'thirty-two': [1] * 14 + [CHUNK - 1, CHUNK, CHUNK + 1, 2] + [1] * 14,
    'aligned': [CHUNK, CHUNK, 1, CHUNK + 1, CHUNK - 2],
}
N_OUT = (1, 63, 65, 130)
N_IN = (1, 63, 65, 257, 1025)


def _ends(widths):
    return np.cumsum(widths).astype(np.int32)


@lru_cache(maxsize=None)
def _operands(layout, n_in):
    """(z_out (130, K), z_in (n_in, K), reference lse, ess, d2_min): computed once, shared, read only"""
    k = int(sum(LAYOUTS[layout]))
    rng = np.random.default_rng([sorted(LAYOUTS).index(layout), n_in])
    z_out, z_in = rng.normal(size=(max(N_OUT), k)), rng.normal(size=(n_in, k))
    z_out[3] = z_in[n_in // 2]                                     # a pair with d2 = 0
    lse, ess, low = inf.lse_ess(z_out, z_in, _ends(LAYOUTS[layout]))
    for a in (z_out, z_in, lse, ess, low):
        a.setflags(write=False)
    return z_out, z_in, lse, ess, low


def _device(a, pad=3):
    """a as the leading columns of a wider device tensor (ld > n_col); what lies beyond is NaN and must not be read"""
    import torch
    wide = torch.full((a.shape[0], a.shape[1] + pad), float('nan'), dtype=torch.float64, device='cuda')
    wide[:, :a.shape[1]] = torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')
    return wide


def _launch(z_out, z_in, group_end, n_col):
    """pem_pairwise_lse_f64_dev on device tensors (any row stride): (lse, ess) as numpy"""
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    lib = _lib.load()
    ge = np.ascontiguousarray(group_end, dtype=np.int32)
    n, m = z_out.shape[0], z_in.shape[0]
    lse = torch.full((n, ge.size + 1), float('nan'), dtype=torch.float64, device='cuda')
    ess = torch.full_like(lse, float('nan'))
    work = torch.empty(int(lib.pem_pairwise_lse_work_len(n, m, ge.size)), dtype=torch.float64, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())                                                                  # noqa: E731
    _lib.check(lib.pem_pairwise_lse_f64_dev(n, m, n_col, p(z_out), z_out.stride(0), p(z_in), z_in.stride(0), ge.size,
                                            C.c_void_p(ge.ctypes.data), p(lse), p(ess), p(work), work.numel(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return lse.cpu().numpy(), ess.cpu().numpy()


def _check(lse, ess, ref_lse, ref_ess, low, group_end, what):
    """|lse - ref| <= 2^-50 (K_c + 8) (1 + min_j d2_c / 2) (information_np.lse_bound); twice that, relative, for ess"""
    bound = inf.lse_bound(group_end, low)
    err = np.abs(lse.astype(inf.LD) - ref_lse).astype(np.float64)
    rel = (np.abs(ess.astype(inf.LD) - ref_ess) / ref_ess).astype(np.float64)
    print(what, 'lse err / bound', float((err / bound).max()), 'ess rel err / bound', float((rel / (2 * bound)).max()))
    assert np.all(err <= bound), (what, float((err / bound).max()))
    assert np.all(rel <= 2.0 * bound), (what, float((rel / (2 * bound)).max()))


def test_the_staging_chunk_is_the_one_the_shapes_straddle():
    from hallthrusterpem_amd import _lib
    assert _lib.INFORMATION_CHUNK == CHUNK and _lib.INFORMATION_MAX_GROUPS == len(LAYOUTS['thirty-two']) == 32
    assert max(N_IN) > 2 * _lib.INFORMATION_INNER_BLOCK                        # more than two workspace partials per row


@pytest.mark.parametrize('n_in', N_IN)
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_the_launch_equals_the_long_double_restatement(layout, n_in):
    z_out, z_in, ref_lse, ref_ess, low = _operands(layout, n_in)
    ge = _ends(LAYOUTS[layout])
    zi = _device(z_in)
    for n_out in N_OUT:
        lse, ess = _launch(_device(z_out[:n_out], pad=5), zi, ge, z_out.shape[1])
        _check(lse, ess, ref_lse[:n_out], ref_ess[:n_out], low[:n_out], ge, (layout, n_out, n_in))
        assert np.all(ess >= 1.0 - 1e-12) and np.all(ess <= n_in * (1 + 1e-12))


def test_identical_rows_give_lse_zero_and_ess_m():
    rng = np.random.default_rng(5)
    row = rng.normal(size=(1, 21))
    z_in, z_out, ge = np.repeat(row, 130, axis=0), np.repeat(row, 7, axis=0), _ends([4, CHUNK, 1])
    lse, ess = _launch(_device(z_out), _device(z_in), ge, 21)
    ref_lse, ref_ess, low = inf.lse_ess(z_out, z_in, ge)
    assert np.all(low == 0) and np.all(ref_ess == 130)
    _check(lse, ess, ref_lse, ref_ess, low, ge, 'identical')
    assert np.all(np.abs(lse) <= 2.0 ** -50 * 9)


def test_a_row_next_to_one_inner_row_only_has_ess_one():
    """inner rows 40 apart in every column, the outer row 0.25 from one of them: every other term underflows to exactly 0"""
    k, m = 19, 600
    z_in = np.arange(m, dtype=np.float64)[:, None] * 40.0 + np.linspace(0.0, 1.0, k)[None, :]
    z_out = z_in[[0, 127, 128, 599]] + 0.25
    ge = _ends([1, 17, 1])
    lse, ess = _launch(_device(z_out), _device(z_in), ge, k)
    assert np.array_equal(ess, np.ones_like(ess))
    widths = np.array([1, 17, 1, 19])
    np.testing.assert_allclose(lse, np.broadcast_to(-0.5 * widths * 0.0625 - np.log(m), lse.shape), rtol=0, atol=2.0 ** -50 * 27 * 2)
    ref_lse, ref_ess, low = inf.lse_ess(z_out, z_in, ge)
    _check(lse, ess, ref_lse, ref_ess, low, ge, 'isolated')


def test_distances_up_to_a_million_leave_the_largest_term_alone():
    """entries scaled so that d2 reaches 1e6: every term but the largest underflows, and the largest must not"""
    rng = np.random.default_rng(6)
    k = 2 * CHUNK + 3
    s = np.sqrt(1e6 / (2 * k))
    z_out, z_in, ge = rng.normal(size=(33, k)) * s, rng.normal(size=(140, k)) * s, _ends([CHUNK + 1, CHUNK + 2])
    ref_lse, ref_ess, low = inf.lse_ess(z_out, z_in, ge)
    assert low.max() > 1e5 and inf.pairwise_d2(z_out, z_in, ge).max() > 1e6
    lse, ess = _launch(_device(z_out), _device(z_in), ge, k)
    assert np.all(np.isfinite(lse)) and np.all(np.isfinite(ess))
    _check(lse, ess, ref_lse, ref_ess, low, ge, 'far')


def test_the_reused_set_keeps_the_term_j_equal_i():
    rng = np.random.default_rng(7)
    z, eps, ge = rng.normal(size=(130, 20)) * 3.0, rng.normal(size=(130, 20)), _ends([3, CHUNK, 1])
    ref_lse, ref_ess, low = inf.lse_ess(z + eps, z, ge)
    own = np.stack([(eps[:, sl] ** 2).sum(axis=1) for sl in inf.group_slices(ge)] + [(eps ** 2).sum(axis=1)], axis=1)
    assert np.all(low <= own * (1 + 1e-9) + 1e-12)                                    # the term j = i is in: d2(i, i) = |eps_i|^2
    lse, ess = _launch(_device(z + eps), _device(z), ge, 20)
    _check(lse, ess, ref_lse, ref_ess, low, ge, 'reuse')


def test_two_calls_give_equal_bits_and_a_row_does_not_depend_on_the_other_rows():
    z_out, z_in, *_ = _operands('straddle', 1025)
    ge, k = _ends(LAYOUTS['straddle']), z_out.shape[1]
    zo, zi = _device(z_out), _device(z_in)
    a, b = _launch(zo, zi, ge, k), _launch(zo, zi, ge, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    alone = _launch(_device(z_out[:5], pad=1), zi, ge, k)                       # rows 0-4 alone: another grid, another stride
    assert np.array_equal(alone[0], a[0][:5]) and np.array_equal(alone[1], a[1][:5])
    tail = _launch(_device(z_out[37:70]), zi, ge, k)                            # rows in other lanes of another tile
    assert np.array_equal(tail[0], a[0][37:70]) and np.array_equal(tail[1], a[1][37:70])


@pytest.fixture(scope='module')
def closed_form():
    import torch
    from hallthrusterpem_amd.information import pairwise_information
    z_o, eps, z_i, ge, exact = inf.closed_form_case(seed=0, n=2048, m=2048)
    dev = lambda a: torch.as_tensor(a, device='cuda')                                                       # noqa: E731
    out = pairwise_information(dev(z_o), dev(eps), dev(z_i), ge)
    return out, inf.estimate(z_o, eps, z_i, ge), exact, ge


def test_the_closed_form_gain_through_the_low_level_entry(closed_form):
    out, ref, exact, ge = closed_form
    eig, se = out['eig'].cpu().numpy(), out['stderr'].cpu().numpy()
    print('EIG - exact', eig - exact, 'stderr', se)
    assert np.all(np.abs(eig - exact) <= 4.0 * se), (eig - exact, se)
    assert out['log_M'] == np.log(2048.0) and out['eig'].shape == (3,)


def test_the_low_level_entry_equals_the_restatement(closed_form):
    out, ref, exact, ge = closed_form
    _check(out['lse'].cpu().numpy(), out['ess'].cpu().numpy(), ref['lse'], ref['ess'], ref['d2_min'], ge, 'closed form')
    _stats_equal(out, ref, ge)


def _stats_equal(out, ref, ge):
    """eig, stderr and the ess summaries against the restatement: u = -|eps_c|^2 / 2 - lse carries lse's bound and the roundings of
    a K_c-term sum of squares; a mean and a standard deviation of N such values carry that and N more roundings"""
    g = lambda k: out[k].cpu().numpy()                                                                     # noqa: E731
    bound = inf.lse_bound(ge, ref['d2_min']).max(axis=0)
    n = ref['u'].shape[0]
    scale = (np.abs(ref['u'] + ref['lse']) + np.abs(ref['lse'])).max(axis=0).astype(np.float64)     # |eps_c|^2 / 2 and |lse|
    tol = bound + (n + 40.0) * 2.0 ** -53 * scale
    assert np.all(np.abs(g('eig') - ref['eig'].astype(np.float64)) <= tol), (g('eig'), ref['eig'])
    # d std / d u_i = (u_i - mean) / ((N - 1) std): |d std| <= sqrt(N / (N - 1)) max |d u|
    assert np.all(np.abs(g('stderr') - ref['stderr'].astype(np.float64)) <= 2.0 * tol / np.sqrt(n)), (g('stderr'), ref['stderr'])
    rel = 2.0 * bound
    for key in ('ess_median', 'ess_min'):
        want = ref[key].astype(np.float64)
        assert np.all(np.abs(g(key) - want) <= 2.0 * rel * want), (key, g(key), want)


# ------------------------------------------------------------------------------------------------ InformationGain
def _table():
    """two quantities, three conditions, 19 records: V_cc at one condition, j_ion at two conditions x 9 angles"""
    rng = np.random.default_rng(8)
    ops = lambda ne: np.stack([10.0 ** rng.uniform(-6, -4.5, ne), rng.uniform(250, 350, ne), rng.uniform(4e-6, 6e-6, ne)], 1)   # noqa: E731
    alpha = np.concatenate([[0.0, np.pi / 2], rng.uniform(-np.pi / 2, np.pi / 2, 7)])
    return {'V_cc': {'x': ops(1), 'y': np.array([30.0]), 'var_y': np.array([4.0])},
            'jion': {'x': ops(2), 'y': rng.lognormal(0.0, 1.0, (2, 9)), 'var_y': rng.uniform(0.5, 4.0, (2, 9)),
                     'loc': np.stack([np.ones(9), alpha], axis=1)}}


NAMES = ('c0', 'T_e')


@pytest.fixture(scope='module')
def gain():
    from hallthrusterpem_amd.information import InformationGain
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    lik = SystemLikelihood(_table())
    return InformationGain(Predictive(lik, NAMES, seed=17))


THETA = np.random.default_rng(9).uniform([0.1, 1.5], [0.9, 4.5], size=(50, 2))


@pytest.mark.parametrize('by', ['qoi', 'condition'])
@pytest.mark.parametrize('samples', [None, THETA], ids=['prior', 'table'])
def test_run_equals_the_restatement_of_what_it_returns(gain, samples, by):
    import torch
    ig = gain
    out = ig.run(samples=samples, n_outer=96, n_inner=160, by=by, first_index=6, keep=True)
    again = ig.run(samples=samples, n_outer=96, n_inner=160, by=by, first_index=6, keep=True)
    for k in ('eig', 'stderr', 'ess_median', 'ess_min', 'lse', 'ess', 'z_outer', 'eps', 'z_inner'):
        assert torch.equal(out[k], again[k]), k                                # the same seed, the same bits
    n_groups = 2 if by == 'qoi' else 3
    assert out['labels'] == (['V_cc', 'jion'] if by == 'qoi' else ['V_cc[0]', 'jion[0]', 'jion[1]']) + ['all']
    assert out['group_end'].tolist() == ([1, 19] if by == 'qoi' else [1, 10, 19]) and out['eig'].shape == (n_groups + 1,)
    assert out['n_outer'] + out['dropped'][0] == 96 and out['n_inner'] + out['dropped'][1] == 160
    assert out['z_outer'].shape == (out['n_outer'], 19) and out['z_inner'].shape == (out['n_inner'], 19)
    z_outer, eps, z_inner = (out[k].cpu().numpy() for k in ('z_outer', 'eps', 'z_inner'))
    assert np.all(np.isfinite(z_outer)) and np.all(np.isfinite(z_inner))
    assert abs(eps.mean()) < 5.0 / np.sqrt(eps.size) and abs(eps.std() - 1.0) < 0.1
    # the estimator on the returned arrays: the observations are z_outer, so the outer predictions are z_outer - eps up to one
    # rounding of the observations; the restatement takes the observations themselves
    ref_lse, ref_ess, low = inf.lse_ess(z_outer, z_inner, out['group_end'])
    _check(out['lse'].cpu().numpy(), out['ess'].cpu().numpy(), ref_lse, ref_ess, low, out['group_end'], ('run', by))
    e2 = eps.astype(inf.LD) ** 2
    half = np.stack([e2[:, sl].sum(axis=1) for sl in inf.group_slices(out['group_end'])] + [e2.sum(axis=1)], axis=1)
    u = -half / 2 - ref_lse
    ref = {'u': u, 'lse': ref_lse, 'eig': u.mean(axis=0), 'stderr': u.std(axis=0, ddof=1) / np.sqrt(inf.LD(u.shape[0])), 'd2_min': low,
           'ess_median': np.median(ref_ess, axis=0), 'ess_min': ref_ess.min(axis=0)}
    _stats_equal(out, ref, out['group_end'])
    # the inner predictions: Predictive's own prediction launch on the shared inputs of the same design indices, over the records'
    # own standard deviations
    pp = ig.pred
    table = pp.theta_table(samples)
    with torch.cuda.device(pp.device):
        ig.assemble_shared(table, 160, 6 + 96 * pp.lik.n_cond)
        want = pp.predict(160).index_select(1, pp.cols) * pp.lik.rec[:, 2].index_select(0, pp.cols)
    want = want[torch.isfinite(want).all(dim=1)].index_select(1, torch.as_tensor(out['perm'], device=pp.device))
    assert torch.equal(out['z_inner'], want)


def test_run_with_reuse_takes_the_outer_draws_as_the_inner_set(gain):
    import torch
    out = gain.run(samples=THETA, n_outer=96, by='condition', reuse=True, keep=True)
    assert out['n_inner'] == out['n_outer'] and out['log_M'] == np.log(out['n_outer']) and out['dropped'][0] == out['dropped'][1]
    assert torch.equal(out['z_inner'] + out['eps'], out['z_outer'])            # z_inner is z_outer less its noise
    z_outer, z_inner = out['z_outer'].cpu().numpy(), out['z_inner'].cpu().numpy()
    ref_lse, ref_ess, low = inf.lse_ess(z_outer, z_inner, out['group_end'])
    _check(out['lse'].cpu().numpy(), out['ess'].cpu().numpy(), ref_lse, ref_ess, low, out['group_end'], 'run reuse')
    # the term j = i is in the sum and d2(i, i) = |eps_i|^2 up to the rounding of z + eps: u_i <= log M, so EIG <= log M
    u = -0.5 * np.stack([(out['eps'].cpu().numpy()[:, sl] ** 2).sum(axis=1) for sl in inf.group_slices(out['group_end'])]
                        + [(out['eps'].cpu().numpy() ** 2).sum(axis=1)], axis=1) - out['lse'].cpu().numpy()
    assert np.all(u <= out['log_M'] + 1e-9) and np.all(out['eig'].cpu().numpy() <= out['log_M'] + 1e-9) and out['reuse'] is True
    other = gain.run(samples=THETA, n_outer=96, by='condition', reuse=False, n_inner=96, keep=True)
    assert other['reuse'] is False
    assert torch.equal(other['z_outer'], out['z_outer']) and not torch.equal(other['z_inner'], out['z_inner'])


def test_the_noise_does_not_depend_on_the_grouping(gain):
    import torch
    a = gain.run(samples=THETA, n_outer=32, n_inner=32, by='qoi', keep=True)
    lab = np.arange(19) % 4
    b = gain.run(samples=THETA, n_outer=32, n_inner=32, by=lab, keep=True)
    assert b['labels'] == [0, 1, 2, 3, 'all'] and a['dropped'] == b['dropped']
    perm = torch.as_tensor(b['perm'], device=a['eps'].device)
    for k in ('eps', 'z_outer', 'z_inner'):
        assert torch.equal(a[k].index_select(1, perm), b[k]), k


def test_a_non_finite_prediction_row_is_dropped_and_counted(gain):
    """one injected non-finite row of predictions, through the filter `run` uses: nothing is provoked on the device"""
    import torch
    from hallthrusterpem_amd.information import finite_draws, pairwise_information
    out = gain.run(samples=THETA, n_outer=40, n_inner=48, by='qoi', keep=True)
    z_o, eps, z_i = out['z_outer'] - out['eps'], out['eps'], out['z_inner'].clone()
    z_o[7, 3] = float('nan')
    z_i[11, 0] = float('inf')
    a, e, b, dropped = finite_draws(z_o, eps, z_i)
    assert dropped == (1, 1) and a.shape[0] == out['n_outer'] - 1 and b.shape[0] == out['n_inner'] - 1
    got = pairwise_information(a, e, b, out['group_end'])
    keep_o = [i for i in range(out['n_outer']) if i != 7]
    keep_i = [j for j in range(out['n_inner']) if j != 11]
    ref = inf.estimate(z_o.cpu().numpy()[keep_o], eps.cpu().numpy()[keep_o], out['z_inner'].cpu().numpy()[keep_i], out['group_end'])
    _check(got['lse'].cpu().numpy(), got['ess'].cpu().numpy(), ref['lse'], ref['ess'], ref['d2_min'], out['group_end'], 'dropped')
    _stats_equal(got, ref, out['group_end'])
    assert np.all(np.isfinite(got['eig'].cpu().numpy()))


def test_the_conditions_of_a_draw_share_one_input_vector(gain):
    import torch
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    pp, nc = gain.pred, gain.pred.lik.n_cond
    table = pp.theta_table(THETA)
    with torch.cuda.device(pp.device):
        raw = pp.assemble_inputs(table, 11, 5).clone().cpu().numpy()
        got = gain.assemble_shared(table, 11, 5).cpu().numpy()
    assert got.shape == raw.shape == (len(COUPLED_INPUTS), 11 * nc) and nc == 3
    assert not np.array_equal(got, raw)                                          # (`assemble_inputs` alone draws every sample anew)
    for r, name in enumerate(COUPLED_INPUTS):
        if name in ('P_b', 'V_a', 'mdot_a'):
            assert np.array_equal(got[r], raw[r]), name                         # each condition keeps its operating row
            assert np.array_equal(got[r], np.tile(pp.lik.operating[:, ('P_b', 'V_a', 'mdot_a').index(name)], 11)), name
        else:
            assert np.array_equal(got[r], np.repeat(raw[r, ::nc], nc)), name     # the draw's first sample, for every condition


def _vcc_table(n_cond, var):
    x = np.repeat(np.array([[2e-5, 300.0, 5e-6]]), n_cond, axis=0)
    return {'V_cc': {'x': x, 'y': np.full(n_cond, 30.0), 'var_y': np.full(n_cond, var)}}


def test_two_conditions_that_share_the_inputs_are_one_measurement_of_half_the_variance():
    """V_cc measured twice at the same operating condition with variance s^2: given the inputs the two records are independent
    observations of one number, so their mean (variance s^2 / 2) is sufficient and EIG_all = the gain of ONE record of variance
    s^2 / 2 -- far below EIG_0 + EIG_1, which is what independent inputs per condition would give.  N = M = 2048; the two tables
    use different design indices, so the comparison is within 4 combined standard errors."""
    import torch
    from hallthrusterpem_amd.information import InformationGain
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    names = ('T_e', 'V_vac')
    twin = InformationGain(Predictive(SystemLikelihood(_vcc_table(2, 4.0)), names, seed=23))
    one = InformationGain(Predictive(SystemLikelihood(_vcc_table(1, 2.0)), names, seed=23))
    a = twin.run(n_outer=2048, n_inner=2048, by='condition', keep=True)
    b = one.run(n_outer=2048, n_inner=2048, by='condition')
    assert a['labels'] == ['V_cc[0]', 'V_cc[1]', 'all'] and b['labels'] == ['V_cc[0]', 'all']
    assert torch.equal(a['z_inner'][:, 0], a['z_inner'][:, 1])                   # one input vector, one operating row: one value
    eig, se = a['eig'].cpu().numpy(), a['stderr'].cpu().numpy()
    eig1, se1 = b['eig'].cpu().numpy(), b['stderr'].cpu().numpy()
    print('twin', eig, se, 'ess', a['ess_median'].cpu().numpy(), 'one record of half the variance', eig1, se1)
    assert float(a['ess_median'].min()) > 8.0 and float(b['ess_median'].min()) > 8.0      # neither estimate is saturated
    assert abs(eig[2] - eig1[1]) <= 4.0 * np.hypot(se[2], se1[1]), (eig, eig1)
    assert eig[2] < eig[0] + eig[1] - 4.0 * (se[0] + se[1] + se[2]), (eig, se)
    assert eig[2] > max(eig[0], eig[1])                                          # and a second record still adds something


def test_the_example_runs():
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    out = subprocess.run([sys.executable, str(root / 'examples' / 'information_gain.py'), '60', '512'], capture_output=True, text=True,
                         timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    for text in ('expected gain from the prior, by qoi', 'expected gain from the prior, by condition',
                 'expected gain relative to the posterior, by qoi', 'expected gain relative to the posterior, by condition'):
        assert text in out.stdout, (text, out.stdout)
