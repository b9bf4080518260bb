"""optimize on the MI355X: shared nuisance draws, the DE launch against its numpy restatement (tests/de_np.py) bit for bit, the
DE driver (optimum, graph replay, repeatability), MAP -> Laplace -> DRAM end to end on synthetic System data, slices."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import de_np
from hallthrusterpem_amd.sampling import LOGUNIFORM, NORMAL, UNIFORM, Prior

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------------- shared nuisance
@pytest.mark.gpu
def test_shared_nuisance_rows_agree_bit_for_bit_and_match_the_oracle():
    import torch
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from test_system_likelihood import UION, _close, _data, _marginal, _restate
    data = _data()
    lik = SystemLikelihood(data, uion_grid=UION)
    names = ('T_e', 'P_T', 'c0', 'c3')
    M, ne = 13, lik.n_cond
    rows = torch.tensor([[2.5, 5e-5, 0.3, 0.6], [4.0, 2e-5, 0.6, 1.2], [2.5, 5e-5, 0.3, 0.6], [1.5, 9e-5, 0.1, 0.3],
                         [3.0, 5e-5, 1.5, 0.6], [2.5, 5e-5, 0.3, 0.6]], dtype=torch.float64, device='cuda')
    K = rows.shape[0]
    post = SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=4, fresh_nuisance=False, shared_nuisance=True)
    got = post.log_likelihood(rows).cpu().numpy()
    assert got[0] == got[2] == got[5] and got[0] != got[1]                      # equal theta in different rows: same bits
    x = post.batch.inputs.cpu().numpy()
    _close(post.loglik.cpu().numpy(), _restate(x, data, lik.qois))
    _close(got, _marginal(_restate(x, data, lik.qois), x, K, M, ne, True))
    # the draws are those of the first row of an unshared posterior, in every row
    plain = SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=4, fresh_nuisance=False)
    plain.log_likelihood(rows)
    nuisance = [i for i in range(15) if i not in post.theta_rows]
    xs, xp = post.batch.inputs.view(15, K, M, ne)[nuisance], plain.batch.inputs.view(15, K, M, ne)[nuisance]
    assert all(torch.equal(xs[:, k], xp[:, 0]) for k in range(K)) and not torch.equal(xp[:, 1], xp[:, 0])
    # K = 1 and K = 64 agree bit for bit at the same theta
    one = SystemPosterior(names, lik, n_chains=1, n_nuisance=M, seed=4, fresh_nuisance=False, shared_nuisance=True)
    many = SystemPosterior(names, lik, n_chains=64, n_nuisance=M, seed=4, fresh_nuisance=False, shared_nuisance=True)
    big = rows[torch.arange(64, device='cuda') % K]
    lp64 = many.log_posterior(big).cpu().numpy()
    for k in range(K):
        lp1 = one.log_posterior(rows[k:k + 1]).cpu().numpy()
        assert np.array_equal(lp1, lp64[k:k + 1]) and np.array_equal(lp64[k::K], np.full(lp64[k::K].shape, lp1[0]))
    # a captured graph replays the same values
    replay = many.capture()
    assert np.array_equal(replay(big).cpu().numpy(), lp64)


# --------------------------------------------------------------------------------------------------------- DE kernel
def _launch(P, d, strategy, finalize, seed, mut, cr, tol, atol, kind, a, b, t):
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    p = lambda x: C.c_void_p(x.data_ptr())                                                  # noqa: E731
    ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                           # noqa: E731
    _lib.check(_lib.load().pem_de_step_f64_dev(P, d, strategy, finalize, seed, mut[0], mut[1], cr, tol, atol, ptr(kind), ptr(a),
                                               ptr(b), p(t['pop_u']), p(t['pop_f']), p(t['trial_u']), p(t['trial_f']), p(t['theta']),
                                               p(t['state']), p(t['record']), p(t['hist']), t['hist'].numel(),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _theta_close(got, want, kind):
    """the sampler tests' tolerances: uniform bit for bit, log-uniform to 4e-15 relative, normal to 1e-12 absolute"""
    for j, k in enumerate(kind):
        if k == UNIFORM:
            assert np.array_equal(got[:, j], want[:, j]), j
        elif k == LOGUNIFORM:
            assert np.max(np.abs(got[:, j] / want[:, j] - 1)) < 4e-15, j
        else:
            assert np.max(np.abs(got[:, j] - want[:, j])) < 1e-12, j


def _values(rng, P, g):
    """trial values with ties, NaN and -inf among them"""
    f = np.round(rng.normal(size=P), 1)                      # few distinct values: many ties
    f[rng.random(P) < 0.1] = np.nan
    f[rng.random(P) < 0.1] = -np.inf
    if g % 3 == 2:
        f[:] = np.nan                                         # nothing can win
        f[P // 2] = -np.inf
    return f


@pytest.mark.gpu
@pytest.mark.parametrize('P', [4, 5, 64, 255, 1024])
@pytest.mark.parametrize('d', [1, 5, 12])
def test_de_kernel_matches_the_numpy_restatement_bit_for_bit(P, d):
    import torch
    rng = np.random.default_rng(P * 100 + d)
    kinds = np.array([UNIFORM, LOGUNIFORM, NORMAL], dtype=np.int32)
    kind = np.ascontiguousarray(kinds[np.arange(d) % 3])
    a = np.where(kind == UNIFORM, -2.0, np.where(kind == LOGUNIFORM, 14.0, 30.0)) + np.arange(d)
    b = np.where(kind == UNIFORM, 3.0, np.where(kind == LOGUNIFORM, 18.0, 2.0)) + np.where(kind == NORMAL, 0.0, np.arange(d))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    redrawn = 0
    for strategy in (de_np.BEST1BIN, de_np.RAND1BIN):
        for seed in (0, 2026, (7 << 32) + 5):
            mut, cr, tol = ((0.5, 1.0), 0.7, 0.01) if seed != 2026 else ((0.8, 0.8), 0.3, 0.5)
            u0 = rng.random((P, d))
            u0[0, 0] = 0.0                                     # clamped into (0, 1)
            u0[-1, -1] = 1.0
            z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')                # noqa: E731
            t = dict(pop_u=z(P, d), pop_f=z(P), trial_u=torch.as_tensor(u0, device='cuda'), trial_f=z(P), theta=z(P, d),
                     state=torch.zeros(1, dtype=torch.int64, device='cuda'), record=z(3), hist=torch.full((6,), -7.0, device='cuda',
                                                                                                            dtype=torch.float64))
            np_state = dict(pop_u=np.zeros((P, d)), pop_f=np.zeros(P), trial_u=u0.copy(), trial_f=np.zeros(P))
            hist = np.full(6, -7.0)
            for g in range(9):
                finalize = g == 8
                _launch(P, d, strategy, int(finalize), seed, mut, cr, tol, 0.0, kind, a, b, t)
                want = de_np.step(g, P, d, strategy, finalize, seed, mut, cr, tol, 0.0, kind, a, b, np_state['pop_u'],
                                  np_state['pop_f'], np_state['trial_u'], np_state['trial_f'])
                torch.cuda.synchronize()
                assert int(t['state'][0]) == want['state']
                assert np.array_equal(t['trial_u'].cpu().numpy(), want['trial_u'])
                _theta_close(t['theta'].cpu().numpy(), want['theta'], kind)
                if g >= 1:
                    assert np.array_equal(t['pop_u'].cpu().numpy(), want['pop_u'])
                    assert np.array_equal(t['pop_f'].cpu().numpy(), want['pop_f'], equal_nan=True)
                    if g - 1 < hist.size:
                        hist[g - 1] = want['hist']
                assert np.array_equal(t['record'].cpu().numpy(), want['record']), (g, t['record'], want['record'])
                assert np.all((want['trial_u'] > 0) & (want['trial_u'] < 1))
                redrawn += want.get('redrawn', 0)
                f = _values(rng, P, g)
                np_state = dict(pop_u=want['pop_u'], pop_f=want['pop_f'], trial_u=want['trial_u'], trial_f=f)
                t['trial_f'].copy_(torch.as_tensor(f, device='cuda'))
            assert np.array_equal(t['hist'].cpu().numpy(), hist)
    assert redrawn > 0                                          # the out-of-bounds rule was exercised


# -------------------------------------------------------------------------------------------------------- DE driver
def _quadratic():
    """a correlated Gaussian in u over a uniform, a log-uniform and a normal prior (and two more uniforms)"""
    import torch
    names = ('T_e', 'c4', 'V_vac', 'c0', 'c3')
    pri = {'T_e': Prior(UNIFORM, 1.0, 5.0, 't'), 'c4': Prior(LOGUNIFORM, 18.0, 22.0, 't'), 'V_vac': Prior(NORMAL, 30.0, 2.0, 't'),
           'c0': Prior(UNIFORM, 0.0, 1.0, 't'), 'c3': Prior(UNIFORM, 0.2, 1.570796, 't')}
    ustar = np.array([0.3, 0.62, 0.45, 0.8, 0.15])
    rng = np.random.default_rng(0)
    Q = np.linalg.qr(rng.standard_normal((5, 5)))[0]
    A = torch.as_tensor(Q @ np.diag([1.0, 3.0, 10.0, 30.0, 100.0]) @ Q.T, device='cuda')
    us = torch.as_tensor(ustar, device='cuda')

    def f(theta):
        u = torch.stack([(theta[:, 0] - 1.0) / 4.0, (torch.log10(theta[:, 1]) - 18.0) / 4.0,
                         torch.special.ndtr((theta[:, 2] - 30.0) / 2.0), theta[:, 3], (theta[:, 4] - 0.2) / (1.570796 - 0.2)], 1)
        dd = u - us
        return -0.5 * torch.einsum('ki,ij,kj->k', dd, A, dd)
    return f, names, pri, ustar


@pytest.mark.gpu
def test_de_driver_reaches_the_optimum_repeats_itself_and_replays_as_a_graph():
    from hallthrusterpem_amd.optimize import DifferentialEvolution
    f, names, pri, ustar = _quadratic()
    runs = {}
    for key, kw in (('eager', {}), ('again', {}), ('graph', dict(use_graph=True))):
        de = DifferentialEvolution(f, names, pri, seed=11, tol=0.0, **kw)
        runs[key] = de.run(200, check_every=25)
    r = runs['eager']
    assert r.generations == 200 and not r.converged and r.history.shape == (201,)
    assert np.abs(r.u - ustar).max() < 1e-3, r.u - ustar
    assert np.all(np.diff(r.history) >= 0)                                # the best value never gets worse
    for other in ('again', 'graph'):
        o = runs[other]
        assert np.array_equal(o.u, r.u) and np.array_equal(o.theta, r.theta) and o.value == r.value, other
        assert np.array_equal(o.history, r.history) and o.generations == r.generations, other
    # the graph runs again from the start, and a loose tolerance stops the search early
    de = DifferentialEvolution(f, names, pri, seed=11, tol=0.0, use_graph=True)
    a, b = de.run(50, check_every=7), de.run(50, check_every=7)
    assert np.array_equal(a.history, b.history)
    loose = DifferentialEvolution(f, names, pri, seed=11, tol=10.0, atol=1.0).run(200, check_every=1)
    assert loose.converged and loose.generations < 200


# ------------------------------------------------------------------------------------------------------- end to end
def _synthetic():
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    rng = np.random.default_rng(0)
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
    na = 25
    data = {'V_cc': {'x': op(4), 'y': np.zeros(4), 'var_y': np.ones(4)},
            'T': {'x': op(3), 'y': np.zeros(3), 'var_y': np.ones(3)},
            'uion': {'x': op(2), 'y': np.zeros((2, 6)), 'var_y': np.ones((2, 6)), 'loc': np.linspace(0.005, 0.075, 6)},
            'jion': {'x': op(5), 'y': np.zeros((5, na)), 'var_y': np.ones((5, na)),
                     'loc': np.stack([np.ones(na), np.linspace(-1.5, 1.5, na)], 1)}}
    # T_e and P_T are left out: the cathode's V_cc is the only data on them and hardly constrains them (calibrated, T_e and P_T
    # trade off along a ridge; T_e alone runs to a bound of its prior), so the MAP lies far from theta* in those two
    names = ('V_vac', 'c0', 'c3')
    star = np.array([30.0, 0.5, 0.8])
    # the data are made at theta* with the nuisance inputs of draw block 0 of the posteriors' design (seed 1): one of the M
    # nuisance draws below reproduces them up to the noise, so theta* is identifiable
    truth = Predictive(SystemLikelihood(data), names, seed=1).run(samples=star[None], n_draws=1)
    for q, dd in data.items():
        t = truth[q]['pred'][0].cpu().numpy()
        dd['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
        dd['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
    return SystemLikelihood(data), names, star


@pytest.mark.gpu
def test_map_laplace_and_dram_on_synthetic_system_data():
    import torch
    from hallthrusterpem_amd.calibration import DRAM, SystemPosterior
    from hallthrusterpem_amd.optimize import DifferentialEvolution, Laplace, is_positive_definite, stencil_size
    lik, names, star = _synthetic()
    d, M = len(names), 50
    mk = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)
    de = DifferentialEvolution(None, names, seed=3, tol=1e-4, use_graph=True)
    post = mk(de.P)
    de.f = post.log_posterior
    res = de.run(1000, check_every=20)
    one = mk(1)
    at = lambda th: float(one.log_posterior(torch.as_tensor(np.asarray(th)[None], device='cuda'))[0])   # noqa: E731
    assert at(res.theta) == res.value                                     # shared draws: the value does not depend on the row
    assert res.value >= at(star), (res.value, at(star), res.theta)
    lap = Laplace.fit(mk(stencil_size(d)).log_posterior, res.theta, names, device='cuda')
    assert np.array_equal(lap.cov, lap.cov.T) and is_positive_definite(lap.cov)
    assert np.all(np.abs(res.theta - star) <= 4 * lap.std), ((res.theta - star) / lap.std)
    theta0, cov0 = lap.dram_start()
    chains = mk(16)                                                        # the target the Laplace approximation describes
    dram = DRAM(chains.log_posterior, theta0, cov0=cov0, n_chains=16, seed=2, adapt_after=100, adapt_interval=50,
                device=chains.device)
    dram.run(200, keep=False)
    acc = float(dram.acceptance[0].mean())
    assert 0.05 <= acc <= 0.9, acc


@pytest.mark.gpu
def test_calibration_start_example_runs():
    out = subprocess.run([sys.executable, str(ROOT / 'examples' / 'calibration_start.py'), '100'], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    assert 'MAP' in out.stdout and 'Laplace' in out.stdout and 'DRAM' in out.stdout, out.stdout


# ------------------------------------------------------------------------------------------------------------ slices
@pytest.mark.gpu
def test_slices_equal_row_by_row_evaluations():
    import torch
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.optimize import slice_points, slices
    lik, names, star = _synthetic()
    n = 5
    post = SystemPosterior(names, lik, n_chains=len(names) * n, n_nuisance=20, seed=1, fresh_nuisance=False, shared_nuisance=True)
    x0 = star
    s = slices(post, x0, n_steps=n)
    rows = slice_points(names, x0, n)
    assert np.array_equal(s['grid'], np.stack([rows[j * n:(j + 1) * n, j] for j in range(3)]))
    one = SystemPosterior(names, lik, n_chains=1, n_nuisance=20, seed=1, fresh_nuisance=False, shared_nuisance=True)
    for r in range(rows.shape[0]):
        th = torch.as_tensor(rows[r:r + 1], device='cuda')
        j, k = divmod(r, n)
        assert float(one.log_prior(th)[0]) == s['prior'][j, k]
        assert float(one.log_likelihood(th)[0]) == s['likelihood'][j, k]
        want = float(one.log_posterior(th)[0])
        assert want == s['posterior'][j, k] or (np.isneginf(want) and np.isneginf(s['posterior'][j, k]))
    assert np.isfinite(s['posterior']).all()
    with pytest.raises(ValueError, match='rows'):
        slices(post, x0, n_steps=4)
