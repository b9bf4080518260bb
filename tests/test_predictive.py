"""Predictive checks on the device (hallthrusterpem_amd/predictive.py; scripts/pem_v0/monte_carlo.py:42-60,63-336): the input
assembly against the numpy sampler and a restated theta index, the record predictions (`pem_coupled_system_predict_f64_dev`)
against the oracle + np.interp and against the likelihood launch, the bands against np.percentile bit for bit, prior against
posterior on data made by the model, and determinism.  The reference's driver layer is stale and third-party: parity unpinned."""
from types import SimpleNamespace

import numpy as np
import pytest

from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS

GRID = np.linspace(0, np.pi / 2, 91)
UION = (0.0, 0.08, 200)
OP_ROWS = [COUPLED_INPUTS.index(k) for k in ('P_b', 'V_a', 'mdot_a')]
SENTINEL = -12345.5


def _operating(rng, ne):
    return np.stack([10.0 ** rng.uniform(-6, -4.5, ne), rng.uniform(250, 350, ne), rng.uniform(4e-6, 6e-6, ne)], axis=1)


def _device_grid():
    import torch
    from hallthrusterpem_amd.models.thruster import thruster_analytic
    one = torch.ones(1, dtype=torch.float64, device='cuda')
    out = thruster_analytic({'V_a': one * 300, 'V_cc': one * 20, 'mdot_a': one * 5e-6, 'a_1': one * 0.05}, num_cells=UION[2],
                            domain=UION[:2])
    return out['u_ion_coords'].cpu().numpy()


def _data(seed=0, n_vcc=3, n_t=4, n_u=2, n_j=3, na=12):
    """every kind, with the edge positions: angles 0 and pi/2, an exact u_ion node, both sides of z = 0.04, the grid ends"""
    rng = np.random.default_rng(seed)
    z = _device_grid()
    zq = np.array([UION[0], 0.011, z[50], 0.0399, 0.0401, 0.06, UION[1]])
    alpha = np.concatenate([[0.0, np.pi / 2, -0.3], rng.uniform(-np.pi / 2, np.pi / 2, na - 3)])
    return {
        'V_cc': {'x': _operating(rng, n_vcc), 'y': rng.uniform(15, 35, n_vcc), 'var_y': rng.uniform(0.5, 4, n_vcc)},
        'T': {'x': _operating(rng, n_t), 'y': rng.uniform(0.05, 0.12, n_t), 'var_y': rng.uniform(1e-5, 1e-4, n_t)},
        'uion': {'x': _operating(rng, n_u), 'y': rng.uniform(1e3, 2e4, (n_u, zq.size)),
                 'var_y': rng.uniform(1e5, 1e7, (n_u, zq.size)), 'loc': zq},
        'jion': {'x': _operating(rng, n_j), 'y': rng.lognormal(0.0, 1.0, (n_j, na)), 'var_y': rng.uniform(0.1, 2, (n_j, na)),
                 'loc': np.stack([np.ones(na), alpha], axis=1)},
    }


def _reference_shaped(seed=0):
    """16 conditions, 348 records: 3 V_cc, 3 T, 2 u_ion x 7 positions, 8 j_ion x 40 angles (tools/system_loglik_probe.py)"""
    rng = np.random.default_rng(seed)
    ne, na = 8, 40
    alpha = np.sort(rng.uniform(-np.pi / 2, np.pi / 2, na))
    zq = np.array([0.0, 0.011, 0.02, 0.0399, 0.0401, 0.06, 0.08])
    return {
        'V_cc': {'x': _operating(rng, 3), 'y': rng.uniform(15, 35, 3), 'var_y': np.ones(3)},
        'T': {'x': _operating(rng, 3), 'y': rng.uniform(0.05, 0.1, 3), 'var_y': np.full(3, 1e-4)},
        'uion': {'x': _operating(rng, 2), 'y': rng.uniform(1e3, 2e4, (2, 7)), 'var_y': np.full((2, 7), 1e6), 'loc': zq},
        'jion': {'x': _operating(rng, ne), 'y': rng.lognormal(0, 1, (ne, na)), 'var_y': rng.uniform(0.1, 2, (ne, na)) ** 2,
                 'loc': np.stack([np.ones(na), alpha], 1)}}


def _every_kind(lik):
    """lik's records regrouped so that every condition holds records of every kind (1 V_cc, 1 T, 7 u_ion, its j_ion)"""
    import torch
    from hallthrusterpem_amd import _lib
    rec, span = lik.rec.cpu().numpy(), lik.span.cpu().numpy()
    pick = lambda q, kind: rec[span[lik.conditions[q].start, kind, 0]:][:span[lik.conditions[q].start, kind, 1]]   # noqa: E731
    extra = [(_lib.SYS_VCC, pick('V_cc', _lib.SYS_VCC)), (_lib.SYS_T, pick('T', _lib.SYS_T)), (_lib.SYS_UION, pick('uion', _lib.SYS_UION))]
    jc = range(lik.conditions['jion'].start, lik.conditions['jion'].stop)
    blocks, out_span, first = [], np.zeros((len(jc), 4, 2), dtype=np.int32), 0
    for i, c in enumerate(jc):
        f0, cnt = span[c, _lib.SYS_JION]
        for kind, r in [(_lib.SYS_JION, rec[f0:f0 + cnt])] + extra:
            out_span[i, kind] = (first, r.shape[0])
            blocks.append(r)
            first += r.shape[0]
        blocks.append(np.full((1, 4), 7.0))      # a padding record between conditions
        first += 1
    return SimpleNamespace(sweep_radius=lik.sweep_radius, uion_grid=lik.uion_grid, n_cond=len(jc), n_rec=first,
                           rec=torch.as_tensor(np.concatenate(blocks), device=lik.device),
                           span=torch.as_tensor(out_span, device=lik.device), n_node=lik.n_node, node=lik.node)


def _restate_records(x, lik, n_draws):
    """(n_draws, n_rec) model values of every record, NaN-free sentinel at padding: oracle + np.interp per kind"""
    from oracle import oracle_ctypes as oc
    from hallthrusterpem_amd import _lib, constants
    ref = oc.coupled(dict(zip(COUPLED_INPUTS, x)), torr2pa=constants.TORR_2_PA)
    th = oc.thruster(x[COUPLED_INPUTS.index('V_a')], ref['V_cc'], x[COUPLED_INPUTS.index('mdot_a')], x[COUPLED_INPUTS.index('a_1')])
    z, u = oc.thruster_uion(th['v_exh'], *lik.uion_grid)
    rec, span, node = lik.rec.cpu().numpy(), lik.span.cpu().numpy(), lik.node.cpu().numpy()
    out = np.full((n_draws, lik.n_rec), SENTINEL)
    for i in range(x.shape[1]):
        d, c = divmod(i, lik.n_cond)
        for kind in range(4):
            f, cnt = span[c, kind]
            r = rec[f:f + cnt]
            if kind == _lib.SYS_VCC:
                out[d, f:f + cnt] = ref['V_cc'][i]
            elif kind == _lib.SYS_T:
                out[d, f:f + cnt] = th['T'][i]
            elif kind == _lib.SYS_JION:
                k = r[:, 3].view(np.int64)
                alpha = (k + r[:, 0]) * GRID[1]
                out[d, f:f + cnt] = np.interp(alpha, GRID, ref['j_ion'][i])
            elif cnt:
                p = r[:, 3].view(np.int64)
                za, zb = z[node[p]], z[node[p + 1]]
                out[d, f:f + cnt] = np.interp(za + r[:, 0] * (zb - za), z, u[i])
    return out


def _close(got, want, rtol=1e-10):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    assert np.all((err <= rtol) | (got[ok] == want[ok])), float(np.max(err))


@pytest.mark.gpu
@pytest.mark.parametrize('S', [None, 1, 7, 64])
def test_inputs_restate_the_design_the_operating_rows_and_the_theta_index(S):
    import torch
    from oracle import sampler_np as snp
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import THETA_STREAM_OFFSET, Predictive
    data = _data()
    lik = SystemLikelihood(data, uion_grid=UION)
    names = ('T_e', 'c0', 'a_1', 'sigma_cex')                   # uniform and log-uniform rows
    pp = Predictive(lik, names, seed=(7 << 32) + 11)
    rng = np.random.default_rng(3)
    table = None if S is None else torch.as_tensor(rng.uniform(size=(S, len(names))), device='cuda')
    n_draws, first = 37, 1_000_003
    x = pp.assemble_inputs(table, n_draws, first_index=first).cpu().numpy()
    n = n_draws * lik.n_cond
    ds = pp.design
    want = snp.sample(n, first, ds.seed, ds.stream, ds.kind, ds.a, ds.b)
    theta_rows = [COUPLED_INPUTS.index(k) for k in names]
    for d in range(15):
        if d in OP_ROWS:
            assert np.array_equal(x[d], lik.operating[np.arange(n) % lik.n_cond, OP_ROWS.index(d)])
        elif d in theta_rows and S is not None:
            g = np.arange(first, first + n, dtype=np.uint64)
            w = snp.philox4x32_10(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), 0, ds.stream + THETA_STREAM_OFFSET,
                                  ds.seed & 0xFFFFFFFF, ds.seed >> 32)[0]
            idx = ((w * np.uint64(S)) >> np.uint64(32)).astype(np.int64)
            assert np.array_equal(x[d], table.cpu().numpy()[idx, theta_rows.index(d)])
            if S > 1:
                assert len(np.unique(idx)) > 1
        elif ds.kind[d] == 0:
            assert np.array_equal(x[d], want[d])
        else:
            assert np.max(np.abs(x[d] / want[d] - 1)) < 4e-15


@pytest.mark.gpu
@pytest.mark.parametrize('qois', ['System', 'Cathode', 'Thruster', ('T', 'jion')])
def test_record_predictions_match_the_oracle_and_leave_padding_alone(qois):
    import torch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    lik = SystemLikelihood(_data(seed=1), uion_grid=UION, qois=qois)
    pp = Predictive(lik, ('c0', 'V_vac'), seed=5)
    n_draws = 29                                                   # a ragged last tile
    # non-physical draws: c0 = NaN (profile), V_vac = NaN (V_cc, v_exh)
    table = torch.tensor([[0.5, 20.0], [float('nan'), 20.0], [0.3, float('nan')], [0.7, 40.0]], dtype=torch.float64, device='cuda')
    x = pp.assemble_inputs(table, n_draws)
    pred = torch.full((n_draws, lik.n_rec), SENTINEL, dtype=torch.float64, device='cuda')
    pp.predict(n_draws, out=pred)
    got = pred.cpu().numpy()
    want = _restate_records(x.cpu().numpy(), lik, n_draws)
    _close(got, want)
    pad = np.ones(lik.n_rec, dtype=bool)
    pad[pp.cols.cpu().numpy()] = False
    assert np.all(got[:, pad] == SENTINEL)
    assert pad.any() == ('jion' in lik.qois)                      # (12 j_ion angles: padded to 13 records per condition)
    assert np.isfinite(got).any()
    if 'jion' in lik.qois:
        assert np.isnan(got).any()                                 # c0 = NaN reaches the profile


def _records_loglik(pred, lik):
    rec, span = lik.rec.cpu().numpy(), lik.span.cpu().numpy()
    n_draws = pred.shape[0]
    ll = np.zeros(n_draws * lik.n_cond)
    with np.errstate(invalid='ignore'):
        for i in range(ll.size):
            d, c = divmod(i, lik.n_cond)
            for kind in range(4):
                f, cnt = span[c, kind]
                z = (rec[f:f + cnt, 1] - pred[d, f:f + cnt]) * rec[f:f + cnt, 2]
                ll[i] += np.sum(-0.5 * z * z)
    return ll


@pytest.mark.gpu
@pytest.mark.parametrize('table', ['reference', 'stress'])
def test_predictions_are_what_the_likelihood_launch_compares(table):
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    lik = SystemLikelihood(_reference_shaped(), uion_grid=UION)
    assert lik.n_cond == 16 and lik.n_rec == 348
    pp = Predictive(lik, ('c0',), seed=9)
    n_draws = 45
    x = pp.assemble_inputs(None, n_draws).clone()
    x[COUPLED_INPUTS.index('c0'), 5::13] = float('nan')            # some non-physical samples
    x[COUPLED_INPUTS.index('V_a'), 3::17] = float('nan')
    tab = lik if table == 'reference' else _every_kind(lik)
    n = n_draws * tab.n_cond if table == 'stress' else x.shape[1]
    b = CoupledBatch(n, profile=False, thruster_qoi=False)
    b.inputs.copy_(x[:, :n])
    pred = torch.full((-(-n // tab.n_cond), tab.n_rec), SENTINEL, dtype=torch.float64, device='cuda')
    b.run_system_predict(tab, pred, qoi=True)
    vcc_fused = b.qoi[0].clone()
    ll = b.run_system_loglik(tab).cpu().numpy()
    assert torch.equal(vcc_fused.isnan(), b.qoi[0].isnan()) and torch.equal(vcc_fused[~vcc_fused.isnan()], b.qoi[0][~b.qoi[0].isnan()])
    want = _records_loglik(pred.cpu().numpy(), tab)
    assert np.array_equal(np.isnan(ll), np.isnan(want)) and np.array_equal(np.isneginf(ll), np.isneginf(want))
    ok = np.isfinite(want)
    assert ok.sum() > n // 2 and (~ok).any()
    assert np.allclose(ll[ok], want[ok], rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_bands_equal_numpy_percentiles_bit_for_bit_with_non_physical_draws():
    import torch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    lik = SystemLikelihood(_data(seed=2), uion_grid=UION)
    pp = Predictive(lik, ('c0', 'T_e'), seed=4)
    trace = np.random.default_rng(0).uniform([0.1, 1.5], [0.9, 4.5], size=(40, 6, 2))
    trace[20:22, :, 0] = np.nan                                     # non-physical posterior samples (c0 = NaN)
    out = pp.run(samples=trace, n_draws=301, noise=True)
    saw_nan = False
    for q, r in out.items():
        pred = r['pred'].cpu().numpy()
        saw_nan |= bool(np.isnan(pred).any())
        want = np.percentile(pred, (5, 50, 95), axis=0)
        got = r['bands'].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), q
        noisy = r['noisy'].cpu().numpy()
        wn = np.percentile(noisy, (5, 95), axis=0)
        gn = r['bands_noisy'].cpu().numpy()
        assert np.array_equal(gn[~np.isnan(wn)], wn[~np.isnan(wn)]) and np.array_equal(np.isnan(gn), np.isnan(wn))
        y = np.asarray(lik.data[q]['y'])
        with np.errstate(invalid='ignore'):
            np.testing.assert_allclose(r['rel_l2'].cpu().numpy(),
                                       np.sqrt(np.mean((pred - y) ** 2, axis=-1) / np.mean(y ** 2, axis=-1)), rtol=1e-12)
    assert saw_nan


@pytest.mark.gpu
def test_noise_restates_counter_based_normals():
    import torch
    from scipy.special import ndtri
    from oracle import sampler_np as snp
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import NOISE_STREAM_OFFSET, Predictive
    lik = SystemLikelihood(_data(seed=2), uion_grid=UION)
    pp = Predictive(lik, ('c0',), seed=21)
    compact = torch.as_tensor(np.random.default_rng(1).normal(size=(50, pp.n_cols)), device='cuda')
    got = (pp.add_noise(compact, first_row=3) - compact).cpu().numpy()
    g = np.arange(3, 53, dtype=np.uint64)[:, None]
    j = np.arange(pp.n_cols, dtype=np.uint64)[None, :]
    w = snp.philox4x32_10(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), j, pp.design.stream + NOISE_STREAM_OFFSET, 21, 0)
    want = pp.sigma.cpu().numpy() * ndtri(snp.u53(w[0], w[1]))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * float(pp.sigma.max()))


@pytest.mark.gpu
def test_posterior_at_the_truth_beats_the_prior_and_its_bands_hold_the_truth():
    import torch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    names = ('T_e', 'V_vac', 'Pstar', 'P_T', 'a_1', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')   # every free input
    star = np.array([3.0, 30.0, 4e-5, 5e-5, 0.02, 0.5, 0.5, 1.0, 0.8, 1e20, 1e16, 54e-20])
    data = _data(seed=6)
    pp0 = Predictive(SystemLikelihood(data, uion_grid=UION), names, seed=1)
    truth = pp0.run(samples=star[None], n_draws=1)
    rng = np.random.default_rng(2)
    for q in data:
        t = truth[q]['pred'][0].cpu().numpy()
        data[q]['y'] = t * (1 + 0.01 * rng.standard_normal(t.shape))
        data[q]['var_y'] = (0.01 * np.abs(t)) ** 2 + 1e-30
    pp = Predictive(SystemLikelihood(data, uion_grid=UION), names, seed=2)
    chain = star * (1 + 1e-3 * rng.standard_normal((20, 4, len(names))))
    post = pp.run(samples=chain, n_draws=400, noise=True)
    prior = pp.run(samples=None, n_draws=400)
    for q in data:
        e_post, e_prior = float(post[q]['rel_l2'].mean()), float(torch.nanmean(prior[q]['rel_l2']))
        assert e_post < 0.5 * e_prior, (q, e_post, e_prior)
        t = truth[q]['pred'][0].cpu().numpy()
        lo, hi = post[q]['bands_noisy'].cpu().numpy()
        assert np.mean((lo <= t) & (t <= hi)) >= 0.9, q
    text = pp.table(prior, post, {'V_cc': 0.01, 'T': 0.01, 'uion': 0.05, 'jion': 0.2})
    assert len(text.splitlines()) == 5


@pytest.mark.gpu
def test_runs_are_deterministic_per_seed():
    import torch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    lik = SystemLikelihood(_data(seed=4), uion_grid=UION)
    trace = np.random.default_rng(0).uniform([0.1, 1.5], [0.9, 4.5], size=(10, 3, 2))
    runs = [Predictive(lik, ('c0', 'T_e'), seed=s).run(samples=trace, n_draws=64, noise=True) for s in (3, 3, 4)]
    for q in lik.qois:
        for key in ('pred', 'noisy', 'bands', 'bands_noisy', 'rel_l2'):
            assert torch.equal(runs[0][q][key], runs[1][q][key]), (q, key)
        assert not torch.equal(runs[0][q]['pred'], runs[2][q]['pred'])
