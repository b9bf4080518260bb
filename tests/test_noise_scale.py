"""Noise scales through the Python layer, on the device: `SystemPosterior(noise_scales=...)` and `JionPosterior` against the
restatements applied to the posterior's own per-sample sums, the path without scales unchanged, a captured replay, and one
end-to-end run of `DeviceEnsemble` against quadrature of the same posterior."""
import ctypes as C

import numpy as np
import pytest

import hp_likelihood as hl
import hp_noise
import noise_np

gpu = pytest.mark.gpu
NAMES = ('V_vac', 'c0')
REL = 0.05                     # the stated std of every record, as a fraction of the true value
M = 4


def tight_priors(free=()):
    """PEM_V0_PRIORS with every input not in `free` confined to the middle thousandth of its prior: the nuisance draws then hardly
    move the model, and the data made at their centre are fitted by every draw"""
    from hallthrusterpem_amd.sampling import PEM_V0_PRIORS, Prior
    out = {}
    for k, p in PEM_V0_PRIORS.items():
        mid, half = 0.5 * (p.a + p.b), 5e-4 * (p.b - p.a)
        out[k] = p if k in free else Prior(p.kind, mid - half, mid + half, 'the middle thousandth of ' + p.source)
    return out


def small_table(names, star, seed=0, jion_factor=2.0, rel=REL):
    """V_cc and T at 3 conditions each, u_ion 2 x 5, j_ion 2 x 9, made by the model at `star` with Gaussian noise of the stated std
    rel |y| -- for j_ion drawn at jion_factor times the stated std"""
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    rng = np.random.default_rng(seed)
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
    data = {'V_cc': {'x': op(3), 'y': np.zeros(3), 'var_y': np.ones(3)},
            'T': {'x': op(3), 'y': np.zeros(3), 'var_y': np.ones(3)},
            'uion': {'x': op(2), 'y': np.zeros((2, 5)), 'var_y': np.ones((2, 5)), 'loc': np.linspace(0.005, 0.075, 5)},
            'jion': {'x': op(2), 'y': np.zeros((2, 9)), 'var_y': np.ones((2, 9)), 'loc': np.stack([np.ones(9), np.linspace(-1.4, 1.4, 9)], 1)}}
    pri = tight_priors(names)
    truth = Predictive(SystemLikelihood(data), names, priors=pri, seed=1).run(samples=np.asarray(star)[None], n_draws=1)
    for q, d in data.items():
        t = truth[q]['pred'][0].cpu().numpy()
        d['var_y'] = (rel * np.abs(t)) ** 2 + 1e-30
        d['y'] = t + (jion_factor if q == 'jion' else 1.0) * rel * np.abs(t) * rng.standard_normal(t.shape)
    return SystemLikelihood(data), pri


@pytest.fixture(scope='module')
def table():
    return small_table(NAMES, (30.0, 0.5))


def _theta(post, rows):
    import torch
    return torch.as_tensor(np.asarray(rows, dtype=np.float64), device=post.device)


def _sums(post):
    """the posterior's own per-sample sums and discharge inputs of its last evaluation, [K][M][Ne]"""
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    x = post.batch.inputs.cpu().numpy()
    md, a1 = (x[COUPLED_INPUTS.index(k)].reshape(post.K, post.M, post.Ne) for k in ('mdot_a', 'a_1'))
    return post.loglik.cpu().numpy().reshape(post.K, post.M, post.Ne), md, a1


def _held(post, theta, got, log_prior=None):
    """(out, ess, chi) of the device against both restatements applied to post's own sums: inside the long-double bounds, and
    within twice the bound of the numpy restatement, which lies inside them as well"""
    ll, md, a1 = _sums(post)
    d = post.discharge
    args = (ll, post._group_end, post._group_count, theta, post._scale_col, post._discharge_col, md if d else None, a1 if d else None,
            *(d or (0.0, 1.0)), log_prior)
    ref = hp_noise.marginal_scaled_ref(*args)
    mine = noise_np.marginal_scaled(*args)
    for name, g, m in zip(('out', 'ess', 'chi'), got, mine):
        if g is None:
            continue
        g = g.cpu().numpy()
        hl.assert_within(g, ref[name], ref[name + '_bound'], name)
        hl.assert_within(m, ref[name], ref[name + '_bound'], name + ' (numpy)')
        fin = np.isfinite(ref[name].astype(np.float64))
        assert np.all(np.abs(g[fin] - m[fin]) <= 2 * ref[name + '_bound'].astype(np.float64)[fin]), name


ROWS = [[30.0, 0.5, 1.0, 1.0, 1.0], [25.0, 0.45, 2.0, 0.5, 1.5], [35.0, 0.6, 0.25, 3.0, 0.8], [30.0, 0.5, 9.0, 0.11, 4.0],
        [30.0, 0.5, 11.0, 1.0, 1.0], [70.0, 0.5, 1.0, 1.0, 1.0]]         # the last two: a scale, a model input outside the prior


@gpu
def test_system_posterior_with_scales_against_the_restatements(table):
    import torch
    from hallthrusterpem_amd.calibration import NOISE_PRIOR, SystemPosterior, log_prior
    lik, pri = table
    post = SystemPosterior(NAMES, lik, n_chains=len(ROWS), n_nuisance=M, priors=pri, seed=1, fresh_nuisance=False,
                           noise_scales=('jion', 'V_cc', 'I_D'))
    assert post.names == NAMES + ('noise_jion', 'noise_V_cc', 'noise_I_D') and post.model_names == NAMES
    assert post.priors['noise_jion'] is NOISE_PRIOR and post.priors is not pri and 'noise_jion' not in pri
    assert post.noise_groups == lik.qois == ('V_cc', 'T', 'uion', 'jion')
    assert post._group_end.tolist() == [3, 6, 8, 10] and post._group_count.tolist() == [3.0, 3.0, 10.0, 18.0]
    assert post._scale_col.tolist() == [3, -1, -1, 2] and post._discharge_col == 4
    theta = _theta(post, ROWS)
    th = theta.cpu().numpy()
    lp = post.log_prior(theta).cpu().numpy()
    want, bound = hl.prior_ref(th, post._kind, post._a, post._b)
    hl.assert_within(lp, want, bound, 'log_prior over all columns')
    assert np.array_equal(np.isfinite(lp), [True] * 4 + [False] * 2)
    assert np.allclose(lp[:4], log_prior(th, post.names, post.priors)[:4], rtol=1e-13)
    out, ess, chi = post.log_likelihood(theta, diagnostics=True)
    assert chi.shape == (len(ROWS), 5) and torch.all(ess[:4] >= 1.0) and torch.all(ess[:4] <= M * (1 + 1e-12))
    _held(post, th, (out, ess, chi))
    assert post.log_likelihood(theta).cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    both = post.log_posterior(theta)
    _held(post, th, (both, None, None), log_prior=lp)
    assert np.array_equal(np.isfinite(both.cpu().numpy()), np.isfinite(lp))
    replay = post.capture()
    again = replay(theta)
    torch.cuda.synchronize()
    assert again.cpu().numpy().tobytes() == both.cpu().numpy().tobytes()
    assert replay.theta.shape == (len(ROWS), 5)


@gpu
def test_without_scales_the_path_and_its_bits_are_the_unscaled_ones(table):
    """noise_scales=None: names and priors as given and the value pem_loglik_marginal_f64_dev gives on the same sums; a posterior
    with scales, evaluated at scale 1, gives those bits too (the scale-1 contract, through the Python layer)"""
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    lik, pri = table
    make = lambda **kw: SystemPosterior(NAMES, lik, n_chains=4, n_nuisance=M, priors=pri, seed=1, fresh_nuisance=False, **kw)   # noqa: E731
    plain, scaled = make(), make(noise_scales=('jion', 'T', 'I_D'))
    assert plain.names == plain.model_names == NAMES and plain.priors is pri and plain.noise is None
    theta = _theta(plain, [r[:2] for r in ROWS[:4]])
    got = plain.log_posterior(theta)
    p = lambda t: C.c_void_p(t.data_ptr())                                                                   # noqa: E731
    x, direct, lp = plain.batch.inputs, torch.empty_like(got), plain.log_prior(theta)
    _lib.check(_lib.load().pem_loglik_marginal_f64_dev(4, M, plain.Ne, p(plain.loglik), p(x[COUPLED_INPUTS.index('mdot_a')]),
                                                       p(x[COUPLED_INPUTS.index('a_1')]), *plain.discharge, p(lp),
                                                       p(direct), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == direct.cpu().numpy().tobytes()
    ones = torch.cat([theta, torch.ones((4, 3), dtype=torch.float64, device=theta.device)], dim=1)
    assert scaled.log_likelihood(ones).cpu().numpy().tobytes() == plain.log_likelihood(theta).cpu().numpy().tobytes()
    with pytest.raises(ValueError, match='build the posterior with noise_scales'):
        plain.log_likelihood(theta, diagnostics=True)


@gpu
def test_jion_posterior_is_one_group():
    from hallthrusterpem_amd.calibration import JionPosterior
    rng = np.random.default_rng(2)
    op = np.stack([10.0 ** rng.uniform(-6, -4.5, 3), rng.uniform(250, 350, 3), rng.uniform(4e-6, 6e-6, 3)], 1)
    alpha = np.broadcast_to(np.linspace(-1.4, 1.4, 7), (3, 7))
    y, std = rng.uniform(0.5, 2.0, (3, 7)), np.full((3, 7), 0.7)
    post = JionPosterior(('c0',), op, alpha, y, std, n_chains=3, n_nuisance=5, seed=1, fresh_nuisance=False, noise_scales=('jion', 'I_D'))
    assert post.names == ('c0', 'noise_jion', 'noise_I_D') and post.noise_groups == ('jion',)
    assert post._group_end.tolist() == [3] and post._group_count.tolist() == [21.0] and post._discharge_col == 2
    theta = _theta(post, [[0.5, 1.0, 1.0], [0.4, 3.0, 0.5], [0.6, 0.2, 2.0]])
    got = post.log_likelihood(theta, diagnostics=True)
    assert got[2].shape == (3, 2)
    _held(post, theta.cpu().numpy(), got)


def test_surrogate_posterior_refuses_scales_next_to_its_own_discharge_term():
    from types import SimpleNamespace
    from hallthrusterpem_amd.calibration import SurrogatePosterior
    lik = SimpleNamespace(use_discharge=True, qois=('V_cc', 'jion'), sweep_radii=(1.0,))
    with pytest.raises(ValueError, match='the chained launch adds the discharge term into the per-sample sums'):
        SurrogatePosterior(('c0',), lik, None, n_chains=2, noise_scales=('jion',))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
E2E_SEED, E2E_STEPS, GRID = 0, 3000, 64


def quadrature(post_grid):
    """(mean of s, 5 % and 95 % points of s, std of c0) of the posterior over (c0, s) by the midpoint rule on GRID x GRID cells of
    the prior box, uniform in c0 and in log10 s (where the log-uniform prior is flat: the density there is exp(log_posterior) s)"""
    import torch
    c0 = (np.arange(GRID) + 0.5) / GRID
    s = 10.0 ** (-1.0 + 2.0 * (np.arange(GRID) + 0.5) / GRID)
    theta = np.stack(np.meshgrid(c0, s, indexing='ij'), axis=-1).reshape(-1, 2)
    lp = post_grid.log_posterior(torch.as_tensor(theta, device=post_grid.device)).cpu().numpy().astype(np.longdouble)
    w = np.exp(lp + np.log(theta[:, 1]) - np.max(lp + np.log(theta[:, 1]))).reshape(GRID, GRID)
    ws, wc = w.sum(axis=0), w.sum(axis=1)
    cdf = np.cumsum(ws) / ws.sum()
    mean_c = (wc * c0).sum() / wc.sum()
    return (float((ws * s).sum() / ws.sum()), float(s[np.searchsorted(cdf, 0.05)]), float(s[np.searchsorted(cdf, 0.95)]),
            float(np.sqrt((wc * (c0 - mean_c) ** 2).sum() / wc.sum())))


@gpu
def test_the_ensemble_sampler_recovers_the_scale_the_data_were_drawn_with():
    """theta = (c0, noise_jion); the j_ion data are drawn at twice their stated std.  The trace's mean of the scale against the
    quadrature of the same device posterior, within 5 MCSE.  With E2E_SEED = 0 (18 j_ion records) the quadrature posterior has
    mean 2.3496 and 90 % interval [1.715, 3.051] for the scale, inside [1.2, 3.2], and std 0.047 = 3 grid cells for c0: a property
    of the drawn data, asserted below all the same.  Measured once: 3000 steps of 4 x 8 walkers gave mean 2.3445, MCSE 0.0092
    (ESS 263 of the ensemble means), 0.55 MCSE from the quadrature; the samplers are deterministic."""
    import torch
    from hallthrusterpem_amd import diagnostics
    from hallthrusterpem_amd.calibration import DeviceEnsemble, SystemPosterior
    lik, pri = small_table(('c0',), (0.5,), seed=E2E_SEED)
    make = lambda rows: SystemPosterior(('c0',), lik, n_chains=rows, n_nuisance=M, priors=pri, seed=1, fresh_nuisance=False,   # noqa: E731
                                        shared_nuisance=True, noise_scales=('jion',))
    mean_s, lo, hi, std_c = quadrature(make(GRID * GRID))
    print(f'quadrature: mean of noise_jion {mean_s:.4f}, 90 % interval [{lo:.3f}, {hi:.3f}], std of c0 {std_c:.4f}')
    assert 1.2 <= lo and hi <= 3.2, (lo, hi)
    assert std_c >= 2.0 / GRID, std_c                        # the grid resolves c0's marginal: the quadrature is a reference
    n_ens, walkers = 4, 8
    post = make(n_ens * walkers // 2)
    theta0 = DeviceEnsemble.ball([0.5, 1.5], [0.02, 0.2], walkers, n_ensembles=n_ens, seed=4)
    sampler = DeviceEnsemble(post.log_posterior, theta0, seed=2, device=post.device)
    trace = sampler.run(E2E_STEPS)
    torch.cuda.synchronize()
    diag = diagnostics.summary(trace.mean(dim=2), names=post.names, burnin=0.1)
    mean, mcse = float(diag['mean'][1]), float(diag['mcse'][1])
    print(f'trace: mean of noise_jion {mean:.4f}, MCSE {mcse:.4f}, ESS {float(diag["ess"][1]):.0f}, R-hat {float(diag["rhat"][1]):.4f}')
    assert abs(mean - mean_s) <= 5.0 * mcse, (mean, mean_s, mcse)
