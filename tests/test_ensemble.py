"""The affine-invariant ensemble sampler on the MI355X: the launch against its numpy restatement (tests/ensemble_np.py) launch by
launch, the driver on a closed-form target (moments, graph replay, repeatability, continuation, thinning, exact affine invariance)
and on a SystemPosterior."""
import ctypes as C

import numpy as np
import pytest

import ensemble_np
from test_ensemble_host import COV_TOL, E_G, K_G, MEAN_TOL, MU, N_G, PREC, _starts, moment_errors

ARRAYS = ('theta', 'logp', 'prop', 'prop_logp', 'log_q', 'state', 'accepted', 'trace', 'logp_trace', 'draws')


# ------------------------------------------------------------------------------------------------------------ the kernel
def _launch(t, E, K, d, seed, a, fraction, g0, sigma, first, length, thin):
    import torch
    from hallthrusterpem_amd import _lib
    _lib.check(_lib.load().pem_ensemble_step_f64_dev(E, K, d, seed, a, fraction, g0, sigma, first, length, thin,
                                                     *[C.c_void_p(t[n].data_ptr()) for n in ARRAYS],
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _near_tie(rec, i):
    """a decision that the last bit of the library log can turn: the two compared numbers within 8 ulp"""
    with np.errstate(invalid='ignore'):
        return bool(abs(rec['lhs'][i] - rec['rhs'][i]) <= 8 * np.spacing(abs(rec['rhs'][i])))


@pytest.mark.gpu
@pytest.mark.parametrize('E, K, d', [(1, 2, 1), (3, 4, 2), (2, 34, 17), (1, 64, 32), (5, 130, 5), (1, 1024, 3)])
def test_ensemble_kernel_matches_the_numpy_restatement_launch_by_launch(E, K, d):
    """24 launches with trace_first=1, trace_len=4, thin=2 and two guard rows of NaN, for de_fraction 0, 1 and 0.5 (K >= 4).  The
    test writes prop_logp itself: finite values on both sides of logp, 10 % -inf, 10 % NaN; walker 0 of ensemble 0 starts at
    -inf; the last walker of every ensemble is only ever offered -inf and must never move.  The numpy state is re-read from the
    device before every launch.  Uniforms and partners bit-equal to numpy's Philox, z / g within 1e-12 relative; with the
    device's z / g handed to the restatement the proposals, and given equal decisions everything else, bit for bit (log_q, which
    goes through the library log, within 8 ulp).  Decisions equal, except at most one near-tie per shape."""
    import torch
    seed, a, sigma, first, length, thin, n_launch = (9 << 32) + 1234 + K, 2.0, 1e-5, 1, 4, 2, 24
    H = K // 2
    g0 = 2.38 / np.sqrt(2.0 * d)
    rng = np.random.default_rng(100 * K + d)
    near_ties = 0
    for fraction in ((0.0, 1.0, 0.5) if K >= 4 else (0.0,)):
        theta0 = rng.normal(size=(E, K, d))
        logp0 = rng.normal(size=(E, K)) - 3.0
        logp0[0, 0] = -np.inf                                   # everything finite is better than the start
        host = dict(theta=theta0, logp=logp0, prop=np.zeros((E, H, d)), prop_logp=np.zeros((E, H)), log_q=np.zeros((E, H)),
                    state=np.zeros(E, dtype=np.int64), accepted=np.zeros((E, K), dtype=np.int64),
                    trace=np.full((length + 2, E, K, d), np.nan), logp_trace=np.full((length + 2, E, K), np.nan),
                    draws=np.full((E, H, 6), np.nan))
        t = {k: torch.as_tensor(v, device='cuda').contiguous() for k, v in host.items()}
        read = lambda: {k: v.cpu().numpy() for k, v in t.items()}                                # noqa: E731
        kw = dict(seed=seed, a=a, de_fraction=fraction, g0=g0, sigma=sigma, trace_first=first, trace_len=length, thin=thin)
        seen = set()
        for s in range(n_launch):
            before = read()
            half = (s - 1) % 2                                  # the half whose values this launch resolves (s >= 1)
            current = before['logp'][:, half * H:(half + 1) * H]
            lp = np.where(np.isfinite(current), current, -3.0) + rng.normal(size=(E, H)) * 2.0
            lp[rng.random((E, H)) < 0.1] = -np.inf
            lp[rng.random((E, H)) < 0.1] = np.nan
            if half == 1:
                lp[:, H - 1] = -np.inf                          # walker K - 1: never anything to move to
            t['prop_logp'].copy_(torch.as_tensor(lp, device='cuda'))
            before['prop_logp'] = lp
            _launch(t, E, K, d, seed, a, fraction, g0, sigma, first, length, thin)
            got = read()
            dr = got['draws']
            if s >= 1:
                assert np.array_equal(dr[:, :, 4], ensemble_np.draws(seed, s, E, H, normals=False)['u_acc']), s
            else:
                assert np.isnan(dr[:, :, 4]).all()              # nothing was resolved: no accept uniform is reported
            # what the launch proposed with: the draws of half-step s + 1
            mv = ensemble_np.moves(ensemble_np.draws(seed, s + 1, E, H), a, fraction, g0, sigma)
            assert np.array_equal(dr[:, :, 5], np.broadcast_to(mv['u_move'][:, None], (E, H))), s
            assert np.array_equal(dr[:, :, 0], np.broadcast_to(mv['de'][:, None], (E, H)).astype(np.float64)), s
            assert np.array_equal(dr[:, :, 2], mv['j1']) and np.array_equal(dr[:, :, 3], mv['j2']), s
            assert np.all(mv['j1'] < H) and np.all(mv['j2'] < H) and np.all(mv['j2'] != mv['j1'])
            assert np.max(np.abs(dr[:, :, 1] - mv['coef']) / np.abs(mv['coef'])) < 1e-12, s
            seen |= set(mv['de'].tolist())
            dec = (got['accepted'] - before['accepted']).astype(bool)
            assert not dec[:, (1 - half) * H:(2 - half) * H].any()                               # the other half stood still
            dec = dec[:, half * H:(half + 1) * H]
            want, rec, _ = ensemble_np.step(before, lp, coef=dr[:, :, 1], **kw)
            if rec is not None:
                for i in zip(*np.nonzero(rec['acc'] != dec)):
                    assert _near_tie(rec, i), (s, i, {n: v[i] for n, v in rec.items()}, dec[i])
                    near_ties += 1
                want, _, _ = ensemble_np.step(before, lp, coef=dr[:, :, 1], decisions=dec, **kw)
            for name in ('theta', 'logp', 'prop', 'accepted', 'state', 'trace', 'logp_trace'):
                assert np.array_equal(got[name], want[name], equal_nan=True), (s, name)
            assert np.allclose(got['log_q'], want['log_q'], rtol=8 * np.finfo(float).eps, atol=0.0), s
            assert np.all(got['state'] == s + 1)
        final = read()
        assert seen == {0.0: {False}, 1.0: {True}, 0.5: {False, True}}[fraction]                 # both moves were met
        assert not final['accepted'][:, K - 1].any() and np.array_equal(final['theta'][:, K - 1], theta0[:, K - 1])
        assert np.isfinite(final['logp'][0, 0]) and final['accepted'][0, 0] >= 1                 # the -inf start was left
        assert final['accepted'].sum() > 0
        # rows due: steps 2, 4, 6, 8 (launches 4, 8, 12, 16); the two guard rows keep their NaN
        rows_written = ~np.isnan(final['trace']).all(axis=(1, 2, 3))
        assert rows_written.tolist() == [True] * length + [False, False]
        assert np.array_equal(np.isnan(final['logp_trace']).all(axis=(1, 2)), ~rows_written)
        assert not np.isnan(final['trace'][:length]).any()
    assert near_ties <= 1, near_ties


# ------------------------------------------------------------------------------------------------------------ the driver
def _gaussian(scale=None, bound=False):
    """the target of test_ensemble_host.py on the device, seen through x / scale; with `bound` one coordinate has a hard edge"""
    import torch
    mu = torch.as_tensor(MU, device='cuda')
    prec = torch.as_tensor(PREC, device='cuda')
    sc = None if scale is None else torch.as_tensor(scale, device='cuda')

    def logp(t):
        r = (t if sc is None else t / sc) - mu
        lp = -0.5 * torch.einsum('ki,ij,kj->k', r, prec, r)
        return torch.where(r[:, 2] > -1.0, lp, torch.full_like(lp, -float('inf'))) if bound else lp
    return logp


@pytest.mark.gpu
@pytest.mark.parametrize('de_fraction', [0.0, 1.0, 0.5])
def test_device_ensemble_recovers_a_correlated_gaussian(de_fraction):
    """the target, shape, schedule and tolerances of test_the_restatement_recovers_a_correlated_gaussian"""
    import torch
    from hallthrusterpem_amd.calibration import DeviceEnsemble
    logp = _gaussian()
    s = DeviceEnsemble(logp, _starts(1), seed=2, de_fraction=de_fraction)
    trace, lp_trace = s.run(N_G, keep_logp=True)
    assert trace.shape == (N_G, E_G, K_G, 5) and lp_trace.shape == (N_G, E_G, K_G) and s.steps == N_G
    mean_err, cov_err = moment_errors(trace.cpu().numpy())
    acc = s.acceptance
    print(f'de_fraction {de_fraction}: mean error {mean_err:.4f}, covariance error {cov_err:.4f}, acceptance {float(acc.mean()):.3f}')
    assert mean_err <= MEAN_TOL and cov_err <= COV_TOL, (mean_err, cov_err)
    assert acc.shape == (E_G, K_G) and float(acc.min()) > 0.1 and float(acc.max()) < 0.9
    assert torch.equal(s.theta, trace[-1]) and torch.equal(s.logp, lp_trace[-1])
    assert torch.allclose(s.logp.reshape(-1), logp(s.theta.reshape(-1, 5)), rtol=1e-12, atol=0)
    assert torch.allclose(lp_trace[-50:].reshape(-1), logp(trace[-50:].reshape(-1, 5)), rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_device_ensemble_replays_as_a_graph_repeats_itself_continues_and_thins():
    import torch
    from hallthrusterpem_amd.calibration import DeviceEnsemble
    logp = _gaussian(bound=True)
    E, K = 3, 12
    x0 = DeviceEnsemble.ball(MU, 0.5, K, n_ensembles=E, seed=8)
    mk = lambda seed=5, **kw: DeviceEnsemble(logp, x0, seed=seed, de_fraction=0.5, **kw)      # noqa: E731
    graph = mk()
    whole, whole_lp = graph.run(100, keep_logp=True)
    assert whole.shape == (100, E, K, 5) and whole_lp.shape == (100, E, K) and not torch.isnan(whole).any()
    assert torch.allclose(whole_lp.reshape(-1), logp(whole.reshape(-1, 5)), rtol=1e-12, atol=0)
    eager = mk(use_graph=False)
    assert torch.equal(eager.run(100), whole)                               # eager and graph: the same bits
    assert torch.equal(mk().run(100), whole)                                # one seed: one trace
    split = mk()
    a, b = split.run(60), split.run(40)
    assert torch.equal(torch.cat([a, b]), whole) and split.steps == 100     # run continues across calls
    for other in (eager, split):
        for name in ('theta', 'logp', 'prop', 'log_q', 'state', 'accepted'):
            assert torch.equal(getattr(other, name), getattr(graph, name)), name
    assert int(graph.state[0]) == 201                                       # launch 0 and two launches per step
    thinned = mk().run(100, thin=4)
    assert thinned.shape == (25, E, K, 5) and torch.equal(thinned, whole[::4])
    odd = mk()
    assert odd.run(0).shape == (0, E, K, 5)
    assert torch.equal(odd.run(10, thin=4), whole[:10:4])                   # ceil(10 / 4) = 3 rows
    assert torch.equal(odd.run(90, keep=True), whole[10:])
    assert odd.run(5, keep=False) is None and odd.steps == 105
    assert not torch.equal(mk().run(20), mk(seed=6).run(20))


@pytest.mark.gpu
@pytest.mark.parametrize('de_fraction', [0.0, 1.0])
def test_device_ensemble_is_affine_invariant_bit_for_bit(de_fraction):
    """what the sampler is for: coordinates scaled by 2^-60 ... 2^66 and the target with them, E = 2, K = 20, 200 steps: the
    trace is the unscaled trace times the scale, bit for bit, with no proposal covariance to retune"""
    import torch
    from hallthrusterpem_amd.calibration import DeviceEnsemble
    scale = 2.0 ** np.array([-60.0, 66.0, 0.0, 13.0, -7.0])
    x0 = DeviceEnsemble.ball(MU, 1.0, 20, n_ensembles=2, seed=3)
    plain = DeviceEnsemble(_gaussian(), x0, seed=11, de_fraction=de_fraction)
    scaled = DeviceEnsemble(_gaussian(scale), x0 * scale, seed=11, de_fraction=de_fraction)
    tp, lp = plain.run(200, keep_logp=True)
    ts, ls = scaled.run(200, keep_logp=True)
    assert tp.shape == (200, 2, 20, 5)
    assert torch.equal(ts, tp * torch.as_tensor(scale, device='cuda')) and torch.equal(ls, lp)
    assert torch.equal(plain.accepted, scaled.accepted) and 0.1 < float(plain.acceptance.mean()) < 0.9


@pytest.mark.gpu
def test_device_ensemble_refuses_a_start_outside_the_support():
    from hallthrusterpem_amd.calibration import DeviceEnsemble
    x0 = DeviceEnsemble.ball(MU, 0.1, 10, seed=1)
    x0[0, 7, 2] = MU[2] - 2.0                                               # past the hard edge of coordinate 2
    with pytest.raises(ValueError, match='1 of the 10 starts'):
        DeviceEnsemble(_gaussian(bound=True), x0)


# --------------------------------------------------------------------------------------------------------- on a posterior
@pytest.mark.gpu
def test_device_ensemble_on_a_shared_nuisance_system_posterior():
    """E = 2 ensembles of K = 2 d walkers, 40 steps from a 0.5 % ball round the truth on the synthetic System data of
    tests/test_optimize.py: shared draws make the posterior a function of theta alone, so every kept logp equals a fresh
    evaluation at the kept point, bit for bit"""
    import torch
    from hallthrusterpem_amd import diagnostics
    from hallthrusterpem_amd.calibration import DeviceEnsemble, SystemPosterior
    from test_optimize import _synthetic
    lik, names, star = _synthetic()
    star = np.asarray(star, dtype=np.float64)
    d, E, n = len(names), 2, 40
    K = 2 * d
    rows = E * K // 2
    post = SystemPosterior(names, lik, n_chains=rows, n_nuisance=50, seed=1, fresh_nuisance=False, shared_nuisance=True)
    s = DeviceEnsemble(post.log_posterior, DeviceEnsemble.ball(star, 0.005 * np.abs(star), K, n_ensembles=E, seed=3), seed=2,
                       device=post.device)
    trace, lp_trace = s.run(n, keep_logp=True)
    assert trace.shape == (n, E, K, d) and lp_trace.shape == (n, E, K)
    flat = trace.reshape(-1, d)
    again = torch.cat([post.log_posterior(flat[i:i + rows].contiguous()).clone() for i in range(0, flat.shape[0], rows)])
    assert torch.equal(again, lp_trace.reshape(-1))
    prior = torch.cat([post.log_prior(flat[i:i + rows].contiguous()).clone() for i in range(0, flat.shape[0], rows)])
    assert torch.isfinite(lp_trace).all() and torch.isfinite(prior).all()   # no row leaves the prior support
    acc = float(s.acceptance.mean())
    assert 0.0 < acc < 1.0, acc
    summary = diagnostics.summary(trace.mean(dim=2), names=names)
    assert 'c3' in diagnostics.format_summary(summary)
