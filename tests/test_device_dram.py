"""The device-resident DRAM sampler on the MI355X: the launch against its numpy restatement (tests/dram_np.py) launch by launch,
the driver on a closed-form target (moments, graph replay, repeatability, continuation, thinning) and on a SystemPosterior."""
import ctypes as C

import numpy as np
import pytest

import dram_np

ARRAYS = ('theta', 'logp', 'L', 'mean', 'scatter', 'prop', 'prop_logp', 'state', 'accepted', 'flags', 'trace', 'logp_trace', 'draws')


# ------------------------------------------------------------------------------------------------------------ the kernel
def _launch(t, K, d, seed, gamma, eps, after, every, first, length, thin):
    import torch
    from hallthrusterpem_amd import _lib
    _lib.check(_lib.load().pem_dram_step_f64_dev(K, d, seed, gamma, eps, after, every, first, length, thin,
                                                 *[C.c_void_p(t[a].data_ptr()) for a in ARRAYS],
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _near_tie(rec, k):
    """a decision of chain k that the last bit of exp / log / log1p can turn: the two compared numbers within 8 ulp"""
    with np.errstate(invalid='ignore'):
        return bool(abs(rec['u1'][k] - rec['a1'][k]) <= 8 * np.spacing(abs(rec['a1'][k]))
                    or abs(rec['log_u2'][k] - rec['log_a2'][k]) <= 8 * np.spacing(abs(rec['log_a2'][k])))


@pytest.mark.gpu
@pytest.mark.parametrize('K, d', [(1, 1), (3, 2), (5, 17), (2, 32), (130, 5)])
def test_dram_kernel_matches_the_numpy_restatement_launch_by_launch(K, d):
    """40 launches with adapt_after=6, adapt_interval=4, thin=3; the test writes prop_logp itself (finite values on both sides of
    logp, -inf, NaN, a chain that starts at logp = -inf, a chain whose proposals are all -inf: with eps = 0 its adaptation must
    fail and leave L alone, with eps = 1e-12 it must adapt).  The numpy state is re-read from the device before every launch.
    u1, u2 bit-equal to numpy's Philox, the normals within 1e-12 of ndtri; with the device's normals handed to the restatement
    the proposals, and given equal decisions everything else, bit for bit.  Decisions equal, except at most one near-tie."""
    import torch
    seed, gamma, after, every, first, length, thin, n_launch = (9 << 32) + 1234 + K, 0.1, 6, 4, 5, 8, 3, 40
    variants = [(0.0, True), (1e-12, True)] + ([(1e-12, False)] if K == 1 else [])
    rng = np.random.default_rng(100 * K + d)
    near_ties = 0
    for eps, stuck_chain in variants:
        stuck = K - 1 if stuck_chain else -1
        B = np.tril(rng.normal(size=(K, d, d))) * 0.3 + np.eye(d)
        theta0 = rng.normal(size=(K, d))
        logp0 = rng.normal(size=K) - 3.0
        if K >= 3 or not stuck_chain:
            logp0[0] = -np.inf                                  # everything is better than the start
        host = dict(theta=theta0, logp=logp0, L=B, mean=theta0.copy(), scatter=np.zeros((K, d, d)), prop=np.zeros((2, K, d)),
                    prop_logp=np.zeros((2, K)), state=np.zeros(K, dtype=np.int64), accepted=np.zeros((2, K), dtype=np.int64),
                    flags=np.zeros(K, dtype=np.int32), trace=np.full((length + 2, K, d), np.nan),
                    logp_trace=np.full((length + 2, K), np.nan), draws=np.full((K, 2 * d + 2), np.nan))
        t = {k: torch.as_tensor(v, device='cuda').contiguous() for k, v in host.items()}
        read = lambda: {k: v.cpu().numpy() for k, v in t.items()}                                # noqa: E731
        kw = dict(seed=seed, gamma=gamma, eps=eps, adapt_after=after, adapt_interval=every, trace_first=first, trace_len=length,
                  thin=thin)
        adapted = failed = 0
        for s in range(n_launch):
            before = read()
            base = np.where(np.isfinite(before['logp']), before['logp'], -3.0)
            lp = base[None, :] + rng.normal(size=(2, K)) * 2.0
            lp[rng.random((2, K)) < 0.1] = -np.inf
            lp[rng.random((2, K)) < 0.1] = np.nan
            if stuck >= 0:
                lp[:, stuck] = -np.inf
            t['prop_logp'].copy_(torch.as_tensor(lp, device='cuda'))
            before['prop_logp'] = lp
            _launch(t, K, d, seed, gamma, eps, after, every, first, length, thin)
            got = read()
            now = None
            if s >= 1:
                z1w, z2w, u1w, u2w = dram_np.draws(seed, s, K, d)
                dr = got['draws']
                assert np.array_equal(dr[:, 2 * d], u1w) and np.array_equal(dr[:, 2 * d + 1], u2w), s
                assert np.max(np.abs(dr[:, :d] - z1w)) < 1e-12 and np.max(np.abs(dr[:, d:2 * d] - z2w)) < 1e-12, s
                now = (dr[:, :d], dr[:, d:2 * d], dr[:, 2 * d], dr[:, 2 * d + 1])
                # the proposals pending before this launch were drawn by the last one from these normals
                assert np.array_equal(before['prop'], dram_np.propose(before['theta'], before['L'], now[0], now[1], gamma)), s
            else:
                assert np.isnan(got['draws']).all()             # nothing was resolved: nothing is reported
            dec = (got['accepted'] - before['accepted']).astype(bool)
            want, rec = dram_np.step(before, lp, now=now, nxt=(np.zeros((K, d)), np.zeros((K, d)), None, None), **kw)
            if rec is not None:
                for k in np.nonzero((rec['acc1'] != dec[0]) | (rec['acc2'] != dec[1]))[0]:
                    assert _near_tie(rec, k), (s, k, {n: v[k] for n, v in rec.items()}, dec[:, k])
                    near_ties += 1
                want, _ = dram_np.step(before, lp, now=now, nxt=(np.zeros((K, d)), np.zeros((K, d)), None, None),
                                       decisions=(dec[0], dec[1]), **kw)
            for name in ('theta', 'logp', 'mean', 'scatter', 'L', 'accepted', 'flags', 'state', 'trace', 'logp_trace'):
                assert np.array_equal(got[name], want[name], equal_nan=name in ('logp', 'trace', 'logp_trace')), (s, name)
            assert np.all(got['state'] == s + 1)
            if s >= after and (s - after) % every == 0:
                changed = np.any(got['L'] != before['L'], axis=(1, 2))
                flagged = (got['flags'] & 1).astype(bool)
                newly = flagged & ~(before['flags'] & 1).astype(bool)    # the flag is sticky: a later success leaves it set
                assert not np.any(changed & newly)
                adapted += int(changed.sum())
                failed += int(newly.sum())
                if stuck >= 0:                                  # zero scatter: no factor with eps = 0, sqrt(scale eps) I otherwise
                    assert not got['scatter'][stuck].any()
                    assert flagged[stuck] == (eps == 0.0), (s, eps)
                    want_L = B[stuck] if eps == 0.0 else np.sqrt((2.4 * 2.4) / d * eps) * np.eye(d)
                    assert np.array_equal(got['L'][stuck], want_L), (s, eps)
            else:
                assert np.array_equal(got['L'], before['L'])
        final = read()
        assert adapted > 0 if eps > 0.0 else failed > 0       # both outcomes of an adaptation were met
        assert final['accepted'][0].sum() > 0 and final['accepted'][1].sum() > 0 or stuck_chain and K == 1
        if stuck >= 0:
            assert not final['accepted'][:, stuck].any() and np.array_equal(final['theta'][stuck], theta0[stuck])
        # rows due: r = s - 1 - first in {0, 3, ...} below 3 * length; the others (and the two guard rows) keep their NaN
        rows_written = ~np.isnan(final['trace']).all(axis=(1, 2))
        assert rows_written.tolist() == [True] * length + [False, False]
        assert np.array_equal(np.isnan(final['logp_trace']).all(axis=1), ~rows_written)
        assert not np.isnan(final['trace'][:length]).any()
    assert near_ties <= 1, near_ties


# ------------------------------------------------------------------------------------------------------------ the driver
def _gaussian():
    import torch
    mu = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64, device='cuda')
    A = torch.tensor([[1.0, 0.0, 0.0], [0.8, 0.6, 0.0], [-0.3, 0.2, 0.4]], dtype=torch.float64, device='cuda')
    sigma = A @ A.T
    prec = torch.linalg.inv(sigma)

    def logp(t):
        r = t - mu
        lp = -0.5 * torch.einsum('ki,ij,kj->k', r, prec, r)
        return torch.where(t[:, 2] > -1.0, lp, torch.full_like(lp, -float('inf')))      # a hard bound on one coordinate
    return logp, mu, sigma


@pytest.mark.gpu
def test_device_dram_recovers_a_correlated_gaussian():
    """the target, the start, the schedule and the bounds of test_dram_recovers_a_correlated_gaussian_and_its_delayed_stage_accepts"""
    import torch
    from hallthrusterpem_amd.calibration import DeviceDRAM
    logp, mu, sigma = _gaussian()
    s = DeviceDRAM(logp, [0.0, 0.0, 0.0], cov0=np.diag([4.0, 4.0, 4.0]), n_chains=48, seed=3, adapt_after=400, adapt_interval=100,
                   gamma=0.1)
    assert s.run(800, keep=False) is None
    trace = s.run(3000)
    assert trace.shape == (3000, 48, 3) and s.steps == 3800 and s.adaptation_failures == 0
    flat = trace.reshape(-1, 3)
    assert float(flat[:, 2].min()) > -1.0
    assert torch.allclose(flat.mean(dim=0), mu, atol=0.08)
    assert torch.allclose(torch.cov(flat.T), sigma, atol=0.12)
    acc = s.acceptance
    assert acc.shape == (2, 48)
    assert 0.15 < float(acc[0].mean()) < 0.6 and float(acc[1].mean()) > 0.02
    assert torch.equal(s.theta, trace[-1]) and torch.allclose(s.logp, logp(s.theta), rtol=1e-12, atol=0)
    assert torch.equal(s.L, torch.tril(s.L)) and s.L.shape == (48, 3, 3)


@pytest.mark.gpu
def test_device_dram_replays_as_a_graph_repeats_itself_continues_and_thins():
    import torch
    from hallthrusterpem_amd.calibration import DeviceDRAM
    logp, _, _ = _gaussian()
    mk = lambda **kw: DeviceDRAM(logp, [0.0, 0.0, 0.0], cov0=np.diag([4.0, 4.0, 4.0]), n_chains=48, seed=5, adapt_after=30,  # noqa: E731
                                 adapt_interval=10, **kw)
    graph = mk()
    whole, whole_lp = graph.run(100, keep_logp=True)
    assert whole.shape == (100, 48, 3) and whole_lp.shape == (100, 48) and not torch.isnan(whole).any()
    assert torch.allclose(whole_lp, logp(whole.reshape(-1, 3)).reshape(100, 48), rtol=1e-12, atol=0)
    eager = mk(use_graph=False)
    assert torch.equal(eager.run(100), whole)                               # eager and graph: the same bits
    assert torch.equal(mk().run(100), whole)                                # one seed: one trace
    split = mk()
    a, b = split.run(60), split.run(40)
    assert torch.equal(torch.cat([a, b]), whole) and split.steps == 100     # run continues across calls
    for other in (eager, split):
        for name in ('theta', 'logp', 'L', 'mean', 'scatter', 'accepted'):
            assert torch.equal(getattr(other, name), getattr(graph, name)), name
    thinned = mk().run(100, thin=4)
    assert thinned.shape == (25, 48, 3) and torch.equal(thinned, whole[::4])
    odd = mk()
    assert odd.run(0).shape == (0, 48, 3)
    assert torch.equal(odd.run(10, thin=4), whole[:10:4])                   # ceil(10 / 4) = 3 rows
    assert torch.equal(odd.run(90, keep=True), whole[10:])
    assert all(x.adaptation_failures == 0 for x in (graph, eager, split, odd))
    assert not torch.equal(mk().run(20), DeviceDRAM(logp, [0.0, 0.0, 0.0], cov0=np.diag([4.0, 4.0, 4.0]), n_chains=48, seed=6,
                                                    adapt_after=30, adapt_interval=10).run(20))


# --------------------------------------------------------------------------------------------------------- on a posterior
@pytest.mark.gpu
def test_device_dram_on_a_shared_nuisance_system_posterior():
    """K = 8 chains, 60 steps from the truth on the synthetic System data of tests/test_optimize.py: shared draws make the
    posterior a function of theta alone, so every kept logp equals a fresh evaluation at the kept point, bit for bit"""
    import torch
    from hallthrusterpem_amd import diagnostics
    from hallthrusterpem_amd.calibration import DeviceDRAM, SystemPosterior
    from test_optimize import _synthetic
    lik, names, star = _synthetic()
    K, n = 8, 60
    post = SystemPosterior(names, lik, n_chains=2 * K, n_nuisance=50, seed=1, fresh_nuisance=False, shared_nuisance=True)
    s = DeviceDRAM(post.log_posterior, star, cov0=np.diag((0.005 * star) ** 2), n_chains=K, seed=2, adapt_after=20, adapt_interval=10,
                   device=post.device)
    trace, lp_trace = s.run(n, keep_logp=True)
    assert trace.shape == (n, K, len(names)) and lp_trace.shape == (n, K)
    flat = trace.reshape(-1, len(names))
    again = torch.cat([post.log_posterior(flat[i:i + 2 * K].contiguous()).clone() for i in range(0, n * K, 2 * K)])
    assert torch.equal(again, lp_trace.reshape(-1))
    assert torch.isfinite(lp_trace).all() and torch.isfinite(post.log_prior(flat[:2 * K].contiguous())).all()
    prior = torch.cat([post.log_prior(flat[i:i + 2 * K].contiguous()).clone() for i in range(0, n * K, 2 * K)])
    assert torch.isfinite(prior).all()                                      # no row leaves the prior support
    acc1 = float(s.acceptance[0].mean())
    assert 0.0 < acc1 < 1.0, acc1
    assert s.adaptation_failures == 0
    summary = diagnostics.summary(trace, names=names, acceptance=s.acceptance)
    assert 'T_e' not in diagnostics.format_summary(summary) and 'c3' in diagnostics.format_summary(summary)
