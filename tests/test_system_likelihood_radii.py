"""The fused multi-QoI likelihood against ion current density measured at several sweep radii
(`pem_coupled_system_{loglik,predict}_radii_f64_dev`, `SystemLikelihood(sweep_radii=...)`): one model evaluation per sample serves
the records of every radius.  Held to the oracle's multi-radius plume (`oracle_ctypes.plume(..., radii=...)`) + numpy with the
tolerances of tests/test_system_likelihood.py (`_close`: rtol 1e-10, atol 1e-9, identical NaN / inf patterns); the decomposition
j_ion(r, alpha) = base(r) g(alpha) + j_cex(r) itself agrees with the oracle to 5e-13 relative per value and 2e-15 on the sums."""
import numpy as np
import pytest

from hallthrusterpem_amd import constants
from hallthrusterpem_amd.calibration import OPERATING
from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
from test_system_likelihood import GRID, UION, _close, _data, _marginal, _operating

RADII = (0.55, 1.0, 1.37)
PLUME_ROWS = ('P_b', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')


def _data_radii(seed=0, per_radius=5, radii=RADII, n_j=3):
    """`_data` of the one-radius tests (3 V_cc, 4 T, 2 u_ion x 7 positions) with n_j j_ion conditions at radii x per_radius angles
    (0, pi/2, one negative, random ones), radius-major"""
    data = _data(seed=seed)
    rng = np.random.default_rng(seed + 100)
    alpha = np.concatenate([[0.0, np.pi / 2, -0.3], rng.uniform(-np.pi / 2, np.pi / 2, per_radius - 3)])
    loc = np.stack([np.repeat(radii, per_radius), np.tile(alpha, len(radii))], axis=1)
    na = loc.shape[0]
    # (current densities of the size the model gives between 0.55 and 1.37 m, so that the j_ion terms are not all alike)
    data['jion'] = {'x': _operating(rng, n_j), 'y': rng.lognormal(0.0, 1.0, (n_j, na)), 'var_y': rng.uniform(0.1, 2, (n_j, na)),
                    'loc': loc}
    return data


def _restate(x, data, qois, radii):
    """numpy + oracle restatement of the per-sample sums for the [15][n] inputs x -- tests/test_system_likelihood.py's, with the
    j_ion model of every record taken from the oracle's profile at the record's radius -- and the oracle's all-radii invalid flag"""
    from oracle import oracle_ctypes as oc
    row = lambda k: x[COUPLED_INPUTS.index(k)]                                                           # noqa: E731
    ref = oc.coupled(dict(zip(COUPLED_INPUTS, x)), torr2pa=constants.TORR_2_PA)
    th = oc.thruster(row('V_a'), ref['V_cc'], row('mdot_a'), row('a_1'))
    z, u = oc.thruster_uion(th['v_exh'], *UION)
    pl = oc.plume(*[row(k) for k in PLUME_ROWS], ref['I_B0'], constants.TORR_2_PA, radii=radii)
    n = x.shape[1]
    n_cond = sum(np.asarray(data[q]['x']).shape[0] for q in qois)
    ll = np.zeros(n)
    c = 0
    with np.errstate(invalid='ignore'):
        for q in qois:
            d = data[q]
            std = np.sqrt(np.asarray(d['var_y'], dtype=np.float64))
            for e in range(np.asarray(d['x']).shape[0]):
                idx = np.arange(c, n, n_cond)
                if q == 'V_cc':
                    ll[idx] += -0.5 * ((d['y'][e] - ref['V_cc'][idx]) / std[e]) ** 2
                elif q == 'T':
                    ll[idx] += -0.5 * ((d['y'][e] - th['T'][idx]) / std[e]) ** 2
                elif q == 'uion':
                    model = np.stack([np.interp(d['loc'], z, u[i]) for i in idx])
                    ll[idx] += np.sum(-0.5 * ((d['y'][e] - model) / std[e]) ** 2, axis=1)
                else:
                    ridx = np.searchsorted(radii, d['loc'][:, 0])
                    assert np.array_equal(np.asarray(radii)[ridx], d['loc'][:, 0])
                    model = np.array([[np.interp(abs(a), GRID, pl['j_ion'][i, :, r]) for a, r in zip(d['loc'][:, 1], ridx)] for i in idx])
                    ll[idx] += np.sum(-0.5 * ((d['y'][e] - model) / std[e]) ** 2, axis=1).reshape(idx.shape)
                c += 1
    return ll, pl['invalid']


def _batch(x, radius=1.0):
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    b = CoupledBatch(x.shape[1], profile=False, thruster_qoi=False, sweep_radius=radius)
    b.inputs.copy_(torch.as_tensor(x, device='cuda'))
    return b


def _inputs(lik, n, seed):
    """n prior draws (numpy) of the [15][n] inputs, the operating columns of sample i those of condition i mod n_cond"""
    from _inputs import coupled_inputs
    d = coupled_inputs(n, seed=seed)
    for j, k in enumerate(OPERATING):
        d[k] = np.resize(lik.operating[:, j], n)
    return np.stack([d[k] for k in COUPLED_INPUTS])


# ---------------------------------------------------------------------------------------------------------- 1. oracle parity
@pytest.mark.gpu
@pytest.mark.parametrize('per_radius', [5, 4])                   # 15 and 12 j_ion records per condition: odd and even counts
@pytest.mark.parametrize('component', ['System', 'Plume'])       # 780 and 195 samples: full tiles and a partial one
def test_log_likelihood_matches_the_oracle_per_sample_and_marginal(component, per_radius):
    import torch
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.likelihood import QOI_MAP, SystemLikelihood
    K, M = 5, 13
    data = _data_radii(per_radius=per_radius)
    lik = SystemLikelihood(data, sweep_radii=RADII, uion_grid=UION, qois=component)
    qois = QOI_MAP[component]
    ne = sum(data[q]['x'].shape[0] for q in qois)
    assert lik.n_cond == ne and lik.sweep_radii == RADII
    names = ('T_e', 'P_T', 'c0', 'c3')
    post = SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=4, fresh_nuisance=False)
    assert post.n == K * M * ne and post.batch.radius == RADII[-1]
    theta = torch.tensor([[2.5, 5e-5, 0.3, 0.6], [4.0, 2e-5, 0.6, 1.2], [1.5, 9e-5, 0.1, 0.3],
                          [3.0, 5e-5, 1.5, 0.6],                      # c0 outside U(0, 1): prior -inf
                          [3.5, 3e-5, 0.5, 0.9]], dtype=torch.float64, device='cuda')
    got = post.log_likelihood(theta).cpu().numpy()
    per_sample = post.loglik.cpu().numpy()
    x = post.batch.inputs.cpu().numpy()
    want_ll, invalid = _restate(x, data, qois, RADII)
    _close(per_sample, want_ll)
    _close(got, _marginal(want_ll, x, K, M, ne, component != 'Cathode'))
    assert np.array_equal(post.batch.invalid.cpu().numpy().astype(bool), invalid)
    # the other per-sample outputs: V_cc as ever; div_angle and T_c those of the last (largest) radius
    from oracle import oracle_ctypes as oc
    last = oc.coupled(dict(zip(COUPLED_INPUTS, x)), torr2pa=constants.TORR_2_PA, radius=RADII[-1])
    _close(post.batch.qoi[0].cpu().numpy(), last['V_cc'])
    _close(post.batch.qoi[1].cpu().numpy(), last['div_angle'])
    _close(post.batch.qoi[2].cpu().numpy(), last['T_c'])
    eager = post.log_posterior(theta).clone()
    assert torch.isneginf(eager[3]) and torch.isfinite(eager[[0, 1, 2, 4]]).all()


# ---------------------------------------------------------------------------------------------------------- 2. predictions
@pytest.mark.gpu
@pytest.mark.parametrize('n', [2 * 64 + 12, 61])                 # whole rows of pred, and a last row that is partly absent
def test_predictions_are_the_values_the_likelihood_compares(n):
    import torch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    data = _data_radii(seed=2)
    lik = SystemLikelihood(data, sweep_radii=RADII, uion_grid=UION)
    x = _inputs(lik, n, seed=5)
    b = _batch(x)
    ll = b.run_system_loglik(lik).cpu().numpy()
    vcc, div, tc, inv = (t.clone() for t in (b.qoi[0], b.qoi[1], b.qoi[2], b.invalid))
    rows = -(-n // lik.n_cond)
    sentinel = -12345.678
    pred = torch.full((rows, lik.n_rec + 3), sentinel, dtype=torch.float64, device='cuda')
    b.qoi.fill_(sentinel)
    b.run_system_predict(lik, pred)
    assert (b.qoi == sentinel).all()                               # optional outputs not asked for: not written
    b.run_system_predict(lik, pred, qoi=True)
    same = lambda u, v: np.array_equal(u.cpu().numpy(), v.cpu().numpy(), equal_nan=True)                 # noqa: E731
    assert same(b.qoi[0], vcc) and same(b.qoi[1], div) and same(b.qoi[2], tc) and same(b.invalid, inv)
    p = pred.cpu().numpy()
    rec, span = lik.rec.cpu().numpy(), lik.span.cpu().numpy()
    written = np.zeros(p.shape, dtype=bool)
    for i in range(n):
        d, c = divmod(i, lik.n_cond)
        cols = np.concatenate([np.arange(f, f + k) for f, k in span[c]])
        written[d, cols] = True
        z = (rec[cols, 1] - p[d, cols]) * rec[cols, 2]
        terms = -0.5 * z * z
        bound = cols.size * 2.0 ** -52 * np.abs(terms).sum()       # summation order only
        assert abs(ll[i] - terms.sum()) <= bound, (i, ll[i], terms.sum(), bound)
    assert written.sum() == sum(span[i % lik.n_cond, :, 1].sum() for i in range(n))
    assert np.all(p[~written] == sentinel) and not np.any(p[written] == sentinel)     # padding and absent samples untouched


# ---------------------------------------------------------------------------------------------------------- 3. non-physical samples
def _far_radius_only_c5(I_B0):
    """a c5 at which the sample of the issue (no pressure dependence: c2 = c4 = 0; negative density, so decay > 1 and j_cex < 0) is
    valid at the first radius alone and non-physical over all three, from a scan of the oracle at this I_B0"""
    from oracle import oracle_ctypes as oc
    scan = np.linspace(-6e17, -0.2e17, 59)
    kw = dict(P_b=np.full(scan.size, 1e-5), c0=0.3, c1=0.5, c2=0.0, c3=0.6, c4=0.0, c5=scan, sigma_cex=55e-20, I_B0=I_B0,
              torr2pa=constants.TORR_2_PA)
    far = oc.plume(**kw, radii=RADII)['invalid'] & ~oc.plume(**kw, radii=RADII[:1])['invalid']
    hit = np.nonzero(far)[0]
    assert hit.size >= 3
    pick = hit[hit.size // 2]
    assert 0 < pick < scan.size - 1 and far[pick]
    return scan[pick]


@pytest.mark.gpu
def test_non_physical_samples_follow_numpy_over_all_radii():
    from oracle import oracle_ctypes as oc
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    data = _data_radii(seed=3)
    lik = SystemLikelihood(data, sweep_radii=RADII, uion_grid=UION)
    ne = lik.n_cond
    n = 2 * 64 + 12
    x = _inputs(lik, n, seed=8)
    row = COUPLED_INPUTS.index
    rng = np.random.default_rng(9)
    x[row('c3')] = rng.uniform(-0.05, 1.57, n)                      # about 3 % of the draws have alpha1 <= 0
    i = np.arange(n)
    bad_va, bad_c0 = i % 5 == 1, i % 7 == 3
    x[row('V_a'), bad_va] = np.nan
    x[row('c0'), bad_c0] = np.nan
    # valid at 0.55 m alone, non-physical through the far radii: in the three j_ion conditions and in one that measured thrust
    far = np.array([9, 12 + 10, 24 + 11, 40])
    assert not (bad_va[far] | bad_c0[far]).any() and np.array_equal(far % ne, [9, 10, 11, 4])
    I_B0 = oc.coupled(dict(zip(COUPLED_INPUTS, x[:, far])), torr2pa=constants.TORR_2_PA)['I_B0']
    for k, v in dict(P_b=1e-5, c0=0.3, c1=0.5, c2=0.0, c3=0.6, c4=0.0, sigma_cex=55e-20).items():
        x[row(k), far] = v
    for j, s in enumerate(far):
        x[row('c5'), s] = _far_radius_only_c5(I_B0[j])
    I_far = oc.coupled(dict(zip(COUPLED_INPUTS, x[:, far])), torr2pa=constants.TORR_2_PA)['I_B0']
    assert np.array_equal(I_far, I_B0)                               # (the thruster does not see the plume's inputs)
    g = lambda k: x[row(k), far]                                                                         # noqa: E731
    args = [g(k) for k in PLUME_ROWS] + [I_B0, constants.TORR_2_PA]
    assert oc.plume(*args, radii=RADII)['invalid'].all() and not oc.plume(*args, radii=RADII[:1])['invalid'].any()

    # a negative beam current with a negative density: base < 0 and j_cex > 0 at every radius, so j_ion is positive in the wings and
    # negative on the axis -- the flag is decided by the LARGEST value of the shape, which only the value-by-value path sees
    neg = 4 * ne + 10
    assert not (bad_va[neg] | bad_c0[neg]) and neg % ne == 10
    for k, v in dict(P_b=1e-5, c0=0.3, c1=0.5, c2=0.0, c3=0.6, c4=0.0, c5=-6e17, sigma_cex=55e-20, mdot_a=-5e-6).items():
        x[row(k), neg] = v
    one = oc.coupled(dict(zip(COUPLED_INPUTS, x[:, neg:neg + 1])), torr2pa=constants.TORR_2_PA)
    pn = oc.plume(*[x[row(k), neg:neg + 1] for k in PLUME_ROWS], one['I_B0'], constants.TORR_2_PA, radii=RADII)
    assert one['I_B0'][0] < 0 and pn['invalid'][0]
    tm = oc.plume_terms(*[x[row(k), neg:neg + 1] for k in PLUME_ROWS], one['I_B0'], constants.TORR_2_PA, radii=RADII)
    wing = tm['X1'][0] * np.exp(-(np.pi / 2 / tm['a1'][0]) ** 2) + tm['X2'][0] * np.exp(-(np.pi / 2 / tm['a2'][0]) ** 2) + tm['j_cex'][0]
    axis = tm['X1'][0] + tm['X2'][0] + tm['j_cex'][0]
    assert (tm['X1'] < 0).all() and (tm['j_cex'] > 0).all() and (wing > 0).all() and (axis < 0).all()

    b = _batch(x)
    got = b.run_system_loglik(lik).cpu().numpy()
    want, invalid = _restate(x, data, lik.qois, RADII)
    assert invalid.any() and not invalid.all() and invalid[far].all() and invalid[neg]
    a1_nonpos = x[row('c2')] * (x[row('P_b')] * constants.TORR_2_PA) + x[row('c3')] <= 0
    assert a1_nonpos.any() and invalid[a1_nonpos].all()
    assert np.array_equal(b.invalid.cpu().numpy().astype(bool), invalid)
    assert np.isnan(want).any() and np.isfinite(want).any()
    _close(got, want)
    cond = i % ne
    kinds = {q: np.isin(cond, np.arange(ne)[lik.conditions[q]]) for q in lik.qois}
    assert np.isfinite(got[bad_c0 & ~kinds['jion'] & ~bad_va]).all()                     # a NaN profile did not leak
    assert np.isnan(got[bad_c0 & kinds['jion'] & ~invalid]).all()
    assert np.isfinite(got[bad_va & kinds['V_cc']]).all() and np.isnan(got[bad_va & (kinds['T'] | kinds['uion'])]).all()
    # every j_ion record of a non-physical sample sees 1e-20, those at the first radius included
    pred = _pred(b, lik)
    d = data['jion']
    for s in far[:3]:
        first, count = lik.span.cpu().numpy()[s % ne, 0]
        assert np.array_equal(pred[s // ne, first:first + count], np.full(count, 1e-20))
        z = (d['y'][s % ne - lik.conditions['jion'].start] - 1e-20) / np.sqrt(d['var_y'][s % ne - lik.conditions['jion'].start])
        assert np.isclose(got[s], np.sum(-0.5 * z * z), rtol=1e-13, atol=0)


def _pred(b, lik):
    import torch
    pred = torch.full((-(-b.n // lik.n_cond), lik.n_rec), np.nan, dtype=torch.float64, device='cuda')
    return b.run_system_predict(lik, pred).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------- 4. radius counts
@pytest.mark.gpu
@pytest.mark.parametrize('R', [2, 5, 8])
def test_two_five_and_eight_radii_against_the_oracle(R):
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    radii = tuple(np.linspace(0.4, 1.6, R))
    data = {'jion': _data_radii(seed=R, per_radius=3, radii=radii, n_j=1)['jion']}
    lik = SystemLikelihood(data, sweep_radii=radii)
    assert lik.n_cond == 1 and lik.n_rec == (3 * R) | 1
    x = _inputs(lik, 67, seed=20 + R)
    b = _batch(x, radius=radii[-1])
    got = b.run_system_loglik(lik).cpu().numpy()
    want, invalid = _restate(x, data, lik.qois, radii)
    _close(got, want)
    assert np.array_equal(b.invalid.cpu().numpy().astype(bool), invalid)


@pytest.mark.gpu
@pytest.mark.parametrize('ridx', [0, 1, 2])
def test_records_at_one_radius_of_three_agree_with_the_one_radius_likelihood(ridx):
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    r = RADII[ridx]
    data = _data(seed=6)
    data['jion']['loc'][:, 0] = r
    one = SystemLikelihood(data, sweep_radius=r, uion_grid=UION)
    three = SystemLikelihood(data, sweep_radii=RADII, uion_grid=UION)
    bits = np.ascontiguousarray(three.rec.cpu().numpy()[:, 3]).view(np.int64)
    assert np.array_equal(one.span.cpu().numpy(), three.span.cpu().numpy()) and ridx in set(bits >> 8)
    x = _inputs(one, 2 * 64 + 12, seed=30 + ridx)
    want = _batch(x, radius=r).run_system_loglik(one).cpu().numpy()
    got = _batch(x, radius=RADII[-1]).run_system_loglik(three).cpu().numpy()
    assert np.isfinite(want).all()
    _close(got, want)


# ---------------------------------------------------------------------------------------------------------- 5. graph replay
@pytest.mark.gpu
def test_graph_replay_equals_eager_for_two_thetas():
    import torch
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    lik = SystemLikelihood(_data_radii(seed=5), sweep_radii=RADII, uion_grid=UION)
    post = SystemPosterior(('T_e', 'P_T', 'c0', 'c3'), lik, n_chains=5, n_nuisance=13, seed=1)
    replay = post.capture()
    for theta in (torch.tensor([[2.5, 5e-5, 0.3, 0.6]] * 5, dtype=torch.float64, device='cuda'),
                  torch.tensor([[4.0, 2e-5, 0.6, 1.2], [1.5, 9e-5, 0.1, 0.3], [3.0, 5e-5, 1.5, 0.6], [3.5, 3e-5, 0.5, 0.9],
                                [2.0, 6e-5, 0.4, 0.7]], dtype=torch.float64, device='cuda')):
        got = replay(theta).clone()
        fresh, post.fresh = post.fresh, False
        eager = post.log_posterior(theta)
        post.fresh = fresh
        assert torch.equal(got, eager)


# ---------------------------------------------------------------------------------------------------------- 6. recovery
@pytest.mark.gpu
def test_differential_evolution_recovers_c0_and_c3_from_data_at_three_radii():
    """tests/test_optimize.py's end-to-end check on a table of three radii: data made through `Predictive` at theta* with the
    nuisance inputs of draw block 0 of the posteriors' design, the DE MAP (default population) at least as good as theta* and
    within 4 Laplace standard deviations of it"""
    import torch
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.optimize import DifferentialEvolution, Laplace, is_positive_definite, stencil_size
    from hallthrusterpem_amd.predictive import Predictive
    rng = np.random.default_rng(0)
    per_radius = 9
    loc = np.stack([np.repeat(RADII, per_radius), np.tile(np.linspace(-1.5, 1.5, per_radius), 3)], axis=1)
    data = {'jion': {'x': _operating(rng, 3), 'y': np.zeros((3, loc.shape[0])), 'var_y': np.ones((3, loc.shape[0])), 'loc': loc}}
    names, star = ('c0', 'c3'), np.array([0.5, 0.8])
    truth = Predictive(SystemLikelihood(data, sweep_radii=RADII), names, seed=1).run(samples=star[None], n_draws=1)
    t = truth['jion']['pred'][0].cpu().numpy()
    assert t.shape == (3, loc.shape[0]) and np.isfinite(t).all() and (t > 1e-20).all()
    near, far = t[:, :per_radius], t[:, 2 * per_radius:]
    assert (near > far).all()                                              # the beam thins out with the radius
    data['jion']['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
    data['jion']['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
    lik = SystemLikelihood(data, sweep_radii=RADII)
    d, M = len(names), 20
    mk = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)
    de = DifferentialEvolution(None, names, seed=3, tol=1e-4, use_graph=True)
    post = mk(de.P)
    de.f = post.log_posterior
    res = de.run(600, check_every=20)
    one = mk(1)
    at = lambda th: float(one.log_posterior(torch.as_tensor(np.asarray(th)[None], device='cuda'))[0])   # noqa: E731
    assert at(res.theta) == res.value
    assert res.value >= at(star), (res.value, at(star), res.theta)
    lap = Laplace.fit(mk(stencil_size(d)).log_posterior, res.theta, names, device='cuda')
    assert np.array_equal(lap.cov, lap.cov.T) and is_positive_definite(lap.cov)
    assert np.all(np.abs(res.theta - star) <= 4 * lap.std), ((res.theta - star) / lap.std)
