"""Tempered sequential Monte Carlo on the device (csrc/pem_smc.hip, calibration.DeviceSMC): every launch against the numpy
restatement (tests/smc_np.py), graph replay against eager launches, a closed-form evidence, two modes from prior draws, and the
state's consistency on a real posterior."""
import numpy as np
import pytest

import dram_np
import smc_cases as cases
import smc_np

pytestmark = pytest.mark.gpu
U = 2.0 ** -53                                  # unit roundoff of a double
LD = np.longdouble
EXACT = ('theta', 'loglik', 'logprior', 'beta', 'stage', 'L', 'prop', 'accept_count', 'accepted', 'flags', 'moves_active',
         'hist_beta', 'hist_accept')
STATE = EXACT + ('log_evidence', 'hist_ess', 'hist_dlogz')


def _sampler(theta, loglik, logprior, history_len=2, **kw):
    """a DeviceSMC whose starts have the given values (its callables hand them out), without a graph, history allocated"""
    import torch
    from hallthrusterpem_amd.calibration import DeviceSMC
    dev = torch.device('cuda', torch.cuda.current_device())
    ll, lp = (torch.as_tensor(a.reshape(-1), device=dev) for a in (loglik, logprior))
    kw = dict(dict(tau=cases.TAU, n_mcmc=cases.N_MCMC, eps=cases.EPS, seed=cases.SEED), **kw)
    sm = DeviceSMC(lambda x: ll, lambda x: lp, theta, n_populations=theta.shape[0], use_graph=False, device=dev, **kw)
    sm._prepare(history_len)
    return sm


def _pull(sm):
    import torch
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy().copy()                                                             # noqa: E731
    h = g(sm._hist)
    return dict(theta=g(sm.theta), loglik=g(sm.loglik), logprior=g(sm.logprior), beta=g(sm.beta), log_evidence=g(sm.log_evidence),
                stage=g(sm.stage), L=g(sm.L), prop=g(sm.prop), accept_count=g(sm.accept_count).view(np.uint32),
                accepted=g(sm.accepted), flags=g(sm.flags).view(np.uint32), moves_active=g(sm.moves_active).view(np.uint32),
                hist_beta=h[0], hist_ess=h[1], hist_accept=h[2], hist_dlogz=h[3])


def _same(a, b, keys=STATE):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _stage_launch(sm):
    import torch
    R, N, d = sm.R, sm.N, sm.d
    rec = torch.zeros((R, 3 * N + N * d + 1 + d + d * d), dtype=torch.float64, device=sm.device)
    sm._launch_stage(record=rec)
    rec = rec.cpu().numpy()
    o = 3 * N + N * d
    return dict(w=rec[:, :N], W=rec[:, N:2 * N], anc=rec[:, 2 * N:3 * N].astype(np.int64), z=rec[:, 3 * N:o].reshape(R, N, d), u=rec[:, o],
                mean=rec[:, o + 1:o + 1 + d], cov=rec[:, o + 1 + d:].reshape(R, d, d))


def _check_stage(before, after, rec, sm):
    """one stage launch: the device's beta', weights, moments and factor against numpy / long double, then every other word
    against the restatement given those"""
    R, N, d = sm.R, sm.N, sm.d
    tau_n = sm.tau * N
    scale2 = sm.scale * sm.scale
    tol_inc = np.zeros(R)
    for r in range(R):
        if not before['beta'][r] < 1.0:
            continue
        dl, lmax, fin = smc_np.shifted(before['loglik'][r])
        b0, b1 = before['beta'][r], after['beta'][r]
        assert b0 < b1 <= 1.0
        # the weights: exp of the restated argument, 4 ulp
        want = np.where(fin, np.exp(smc_np.weight_argument(dl, b0, b1)), 0.0)
        w = rec['w'][r]
        assert np.all(np.abs(w - want) <= 4.0 * np.spacing(want)), np.abs(w - want).max()
        # the ESS at the device's beta', in long double.  Bisection resolves beta to 2^-52 (1 - beta); the finite log likelihoods
        # of these inputs lie within 1.2e3 of each other (smc_cases.launch_inputs; asserted here), so |d ESS / d beta| <= 2 x 1.2e3 N and the ESS
        # at beta' is within 2^-52 x 2.4e3 N = 5e-13 N of the crossing; the device's own sums add about N 2^-53 relative: 1e-9 N
        # covers both with room
        assert -dl[fin].min() <= cases.SPREAD, (r, dl[fin].min())
        wl = np.where(fin, np.exp(LD(b1 - b0) * dl.astype(LD)), LD(0))
        ess = float(wl.sum() ** 2 / (wl * wl).sum())
        if b1 < 1.0:
            assert abs(ess - tau_n) <= 1e-9 * N, (r, ess, tau_n)
        else:
            assert ess >= tau_n - 1e-9 * N, (r, ess, tau_n)
        # the moments against long double sums of the device's weights.  The device's mean is a chain of at most N + 2 rounded
        # additions of rounded products divided by a sum of N rounded additions: first order (2 N + 6) u sum W |x|.  A covariance
        # entry is invariant under the mean's error dm up to dm_j dm_k; its terms carry 4 roundings each (two subtractions, two
        # products), its sum N + 2, the normalisation N + 1: (2 N + 10) u sum W (|y_j| + dm_j)(|y_k| + dm_k) + dm_j dm_k.
        # 1.01 stands for the higher orders.
        x = before['theta'][r].astype(LD)
        Wl = w.astype(LD) / w.astype(LD).sum()
        mean_l = Wl @ x
        b_mean = 1.01 * (2 * N + 6) * U * (Wl @ np.abs(x)).astype(np.float64)
        assert np.all(np.abs(rec['mean'][r] - mean_l.astype(np.float64)) <= b_mean + 1e-300), (r, rec['mean'][r], mean_l)
        y = x - mean_l
        cov_l = (Wl[:, None] * y).T @ y
        ya = np.abs(y) + b_mean
        b_cov = 1.01 * (2 * N + 10) * U * ((Wl[:, None] * ya).T @ ya).astype(np.float64) + np.outer(b_mean, b_mean)
        low = np.tril(np.ones((d, d), dtype=bool))
        assert np.all(np.abs(rec['cov'][r] - cov_l.astype(np.float64))[low] <= b_cov[low] + 1e-300), r
        # the factor: bit for bit the column-by-column factor of what the device factorised, and backward stable against the
        # long double matrix: |A - L L^T| <= (d + 1) u |L| |L|^T (Higham, Accuracy and Stability, thm 10.3) + the error of A
        A = scale2 * rec['cov'][r] + sm.eps * np.eye(d)
        Lr, failed = dram_np.cholesky(A[None], before['L'][r][None])
        assert not failed[0] and not after['flags'][r] & 1
        assert np.array_equal(after['L'][r], Lr[0])
        Ll = after['L'][r].astype(LD)
        A_l = LD(scale2) * cov_l + LD(sm.eps) * np.eye(d)
        b_A = 1.01 * (d + 1) * U * (np.abs(Ll) @ np.abs(Ll).T).astype(np.float64) + scale2 * b_cov + 3 * U * np.abs(A)
        assert np.all(np.abs((Ll @ Ll.T - A_l).astype(np.float64))[low] <= b_A[low] + 1e-300), r
        # the normals: the library's normcdfinv against scipy's ndtri on the same counters; 1e-12 is thousands of ulp, what it
        # guards is the counter and the pairing (a wrong one is off by O(1))
        z_np = smc_np.draw_normals(sm.seed, r * N, N, d, (int(before['stage'][r]) + 1) * sm.n_mcmc + 1)
        assert np.all(np.abs(rec['z'][r] - z_np) <= 1e-12 * np.maximum(1.0, np.abs(z_np)))
        tol_inc[r] = (N + 8) * U * (1.0 + abs(np.log(w.sum() / N)) + abs((b1 - b0) * lmax))
    # every other word, given the device's beta', w, L and normals
    st, recs = smc_np.stage(before, sm.seed, sm.tau, sm.scale, sm.eps, sm.n_mcmc, beta_next=after['beta'], w=rec['w'], L=after['L'],
                            normals=rec['z'])
    _same(after, st, EXACT)
    H = before['hist_beta'].shape[1]
    for r in range(R):
        if recs[r] is None:
            assert after['log_evidence'][r] == before['log_evidence'][r]
            assert np.array_equal(after['hist_ess'][r], before['hist_ess'][r]) and np.array_equal(after['hist_dlogz'][r], before['hist_dlogz'][r])
            continue
        assert np.array_equal(rec['anc'][r], recs[r]['anc']) and rec['u'][r] == recs[r]['u']
        assert np.all(np.abs(rec['W'][r] - recs[r]['W']) <= (N + 2) * U * recs[r]['W'])
        s0 = int(before['stage'][r])
        assert abs(after['log_evidence'][r] - st['log_evidence'][r]) <= tol_inc[r] + U * abs(st['log_evidence'][r])
        if s0 < H:
            assert abs(after['hist_dlogz'][r, s0] - recs[r]['inc']) <= tol_inc[r]
            assert abs(after['hist_ess'][r, s0] - recs[r]['ess']) <= 4 * N * U * recs[r]['ess']
            assert after['log_evidence'][r] == before['log_evidence'][r] + after['hist_dlogz'][r, s0]
        untouched = np.arange(H) != s0
        assert np.array_equal(after['hist_ess'][r, untouched], before['hist_ess'][r, untouched])
        assert np.array_equal(after['hist_dlogz'][r, untouched], before['hist_dlogz'][r, untouched])


def _check_move(sm, before, m, kind, rng):
    import torch
    R, N, d = sm.R, sm.N, sm.d
    ll, lp = cases.proposal_values(before['prop'], kind, rng)
    sm.prop_loglik.copy_(torch.as_tensor(ll, device=sm.device))
    sm.prop_logprior.copy_(torch.as_tensor(lp, device=sm.device))
    rec_t = torch.zeros((R, N, d + 2), dtype=torch.float64, device=sm.device)
    propose = m < sm.n_mcmc
    sm._launch_move(m, propose, record=rec_t)
    after, rec = _pull(sm), rec_t.cpu().numpy()
    dec = rec[:, :, d + 1] != 0.0
    st, own = smc_np.move(before, ll, lp, sm.seed, sm.n_mcmc, m, propose_next=propose, normals=rec[:, :, :d], decisions=dec)
    _same(after, st)
    active = before['moves_active'].astype(bool)
    assert np.array_equal(rec[active][:, :, d], own['u'][active])
    # a decision may differ from numpy's lhs < rhs only where the two sides agree to 4 ulp of log(u): at most 2 per launch
    tie = cases.ties(own) & active[:, None]
    assert not ((dec != own['acc']) & active[:, None] & ~tie).any()
    assert int(tie.sum()) <= 2
    assert not dec[~active].any()
    if propose:
        for r in np.nonzero(active)[0]:
            z_np = smc_np.draw_normals(sm.seed, r * N, N, d, int(before['stage'][r]) * sm.n_mcmc + m + 1)
            assert np.all(np.abs(rec[r, :, :d] - z_np) <= 1e-12 * np.maximum(1.0, np.abs(z_np)))
    return after


@pytest.mark.parametrize('shape', cases.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['smooth', 'hostile'])
def test_every_launch_of_three_stages_against_the_restatement(shape, kind):
    """three consecutive stages with n_mcmc = 2 and a history of TWO rows (the third stage is past it and is not recorded): a
    stage launch and two move launches each, every state word after every launch"""
    R, N, d = shape
    theta, loglik, logprior = cases.launch_inputs(R, N, d, kind)
    sm = _sampler(theta, loglik, logprior)
    rng = np.random.default_rng(5)
    state = _pull(sm)
    _same(state, smc_np.new_state(theta, loglik, logprior, history_len=2))
    for _ in range(3):
        rec = _stage_launch(sm)
        after = _pull(sm)
        _check_stage(state, after, rec, sm)
        state = after
        for m in range(1, sm.n_mcmc + 1):
            state = _check_move(sm, state, m, kind, rng)
    assert np.all(state['stage'] >= 1) and np.all(np.isfinite(state['loglik']))       # resampling left no weight-0 particle


def test_a_population_without_a_finite_log_likelihood_raises_bit_1_and_nothing_else():
    theta, loglik, logprior = cases.launch_inputs(2, 65, 2, 'smooth')
    sm = _sampler(theta, loglik, logprior)
    import torch
    sm.loglik[1] = torch.as_tensor(np.resize([np.nan, -np.inf, np.inf], 65), device=sm.device)
    before = _pull(sm)
    rec = _stage_launch(sm)
    after = _pull(sm)
    assert after['flags'].tolist() == [0, 2] and after['moves_active'].tolist() == [1, 0] and after['stage'].tolist() == [1, 0]
    for k in STATE:
        if k not in ('flags',):
            assert np.array_equal(after[k][1], before[k][1], equal_nan=True), k
    assert not rec['w'][1].any()
    # the move launch leaves that population alone as well
    state = _check_move(sm, after, 1, 'smooth', np.random.default_rng(1))
    for k in STATE:
        assert np.array_equal(state[k][1], after[k][1], equal_nan=True), k
    from hallthrusterpem_amd.calibration import DeviceSMC
    with pytest.raises(ValueError, match='no start with a finite log likelihood'):
        ll = torch.as_tensor(np.where(np.arange(130) < 65, np.nan, 0.0), device=sm.device)
        DeviceSMC(lambda x: ll, lambda x: torch.zeros_like(ll), theta, n_populations=2, device=sm.device)


def test_a_refused_factor_keeps_the_old_one_and_raises_bit_0():
    """every particle at the origin and eps = 0: mean and covariance are exactly 0, the first pivot is not > 0"""
    R, N, d = 1, 130, 3
    theta = np.zeros((R, N, d))
    _, loglik, logprior = cases.launch_inputs(R, N, d, 'smooth')
    sm = _sampler(theta, loglik, logprior, eps=0.0)
    import torch
    old = torch.as_tensor(np.tril(np.arange(1.0, 10.0).reshape(3, 3)), device=sm.device)
    sm.L[0] = old
    before = _pull(sm)
    rec = _stage_launch(sm)
    after = _pull(sm)
    assert after['flags'].tolist() == [1] and np.array_equal(after['L'], before['L']) and not rec['cov'].any()
    st, _ = smc_np.stage(before, sm.seed, sm.tau, sm.scale, sm.eps, sm.n_mcmc, beta_next=after['beta'], w=rec['w'], normals=rec['z'])
    assert st['flags'].tolist() == [1]                                   # the restatement's own factorisation refuses it too
    _same(after, st, EXACT)


def test_a_finished_population_ignores_further_launches():
    """N = 2 reaches beta = 1 in its first stage (ESS >= 1 = tau N): the stage launch after its moves closes the acceptance
    count and lowers moves_active; every launch after that changes no word"""
    theta, loglik, logprior = cases.launch_inputs(1, 2, 1, 'smooth')
    sm = _sampler(theta, loglik, logprior)
    rng = np.random.default_rng(2)
    _stage_launch(sm)
    state = _pull(sm)
    assert state['beta'].tolist() == [1.0] and state['moves_active'].tolist() == [1]
    for m in (1, 2):
        state = _check_move(sm, state, m, 'smooth', rng)
    _stage_launch(sm)
    closed = _pull(sm)
    assert closed['moves_active'].tolist() == [0] and closed['accepted'][0] == state['accept_count'].sum()
    assert closed['hist_accept'][0, 0] == float(closed['accepted'][0]) / (2.0 * 2.0)
    _same(closed, dict(state, moves_active=closed['moves_active'], accepted=closed['accepted'], hist_accept=closed['hist_accept']))
    rec = _stage_launch(sm)
    for m in (1, 2):
        sm._launch_move(m, m < 2)
    _same(_pull(sm), closed)
    assert not rec['w'].any()


# ------------------------------------------------------------------------------------------------------------ whole runs
def _t(f):
    """a numpy closed form of smc_cases as a torch callable on the device (its constants are on the device before any capture)"""
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    lik_mean, mode_a, mode_b = (torch.as_tensor(m, device=dev) for m in (cases.LIK_MEAN, cases.MODE_A, cases.MODE_B))

    def gauss_loglik(x):
        return -0.5 * (((x - lik_mean) / cases.LIK_STD) ** 2).sum(dim=-1)

    def gauss_logprior(x):
        return -0.5 * ((x / cases.PRIOR_STD) ** 2).sum(dim=-1) - 2.0 * float(np.log(cases.PRIOR_STD * np.sqrt(2.0 * np.pi)))

    def modes_loglik(x):
        qa = -0.5 * (((x - mode_a) / cases.MODE_STD) ** 2).sum(dim=-1) + float(np.log(cases.MASS_A))
        qb = -0.5 * (((x - mode_b) / cases.MODE_STD) ** 2).sum(dim=-1) + float(np.log(1.0 - cases.MASS_A))
        return torch.logaddexp(qa, qb)

    def modes_logprior(x):
        inside = (x.abs() <= cases.BOX).all(dim=-1)
        return torch.where(inside, torch.full_like(x[:, 0], -float(np.log((2.0 * cases.BOX) ** 2))), torch.full_like(x[:, 0], -np.inf))
    return locals()[f]


def _result_words(res):
    return dict(theta=res.theta.cpu().numpy(), loglik=res.loglik.cpu().numpy(), logprior=res.logprior.cpu().numpy(),
                log_evidence=res.log_evidence, betas=res.betas, ess=res.ess, acceptance=res.acceptance,
                increments=res.log_evidence_increments, stages=res.stages, converged=res.converged, flags=res.flags)


def test_graph_replay_equals_eager_and_the_result_does_not_depend_on_check_every():
    from hallthrusterpem_amd.calibration import DeviceSMC
    theta0 = cases.gauss_starts(4, 257, seed=21)
    runs = []
    for use_graph, check_every in ((False, 1), (True, 1), (True, 4), (True, 50), (False, 50)):
        sm = DeviceSMC(_t('gauss_loglik'), _t('gauss_logprior'), theta0, n_populations=4, seed=9, use_graph=use_graph)
        runs.append(_result_words(sm.run(max_stages=100, check_every=check_every)))
    first = runs[0]
    assert first['converged'].all() and first['stages'].min() >= 2 and not first['flags'].any()
    assert np.all((first['acceptance'][~np.isnan(first['acceptance'])] > 0.0))
    for other in runs[1:]:
        for k, v in first.items():
            assert np.array_equal(v, other[k], equal_nan=True), k


R_RUN, N_RUN = 16, 1024


def test_the_closed_form_evidence_on_the_device():
    """tests/test_smc_host.py's Gaussian problem, R = 16, N = 1024, the same starts and seed on the device and in the restatement:
    the two differ only through last bits of exp / log / normcdfinv, so they are two draws of one estimator and their means lie
    within 5 s_ref sqrt(2 / R), s_ref the restatement's population spread.  The exact value is held as in the host test."""
    from hallthrusterpem_amd.calibration import DeviceSMC
    theta0 = cases.gauss_starts(R_RUN, N_RUN)
    ref = smc_np.run(cases.gauss_loglik, cases.gauss_logprior, theta0, seed=3, tau=0.5, n_mcmc=3)
    s_ref = ref['log_evidence'].std(ddof=1)
    sm = DeviceSMC(_t('gauss_loglik'), _t('gauss_logprior'), theta0, n_populations=R_RUN, seed=3, tau=0.5, n_mcmc=3)
    res = sm.run()
    print(f'log Z exact {cases.GAUSS_LOG_Z:.4f} device {res.log_evidence.mean():.4f} restatement {ref["log_evidence"].mean():.4f} '
          f's_ref {s_ref:.4f} stages {res.stages.tolist()}')
    assert res.converged.all() and not res.flags.any()
    assert abs(res.log_evidence.mean() - ref['log_evidence'].mean()) <= 5.0 * s_ref * np.sqrt(2.0 / R_RUN)
    assert abs(res.log_evidence.mean() - cases.GAUSS_LOG_Z) <= 5.0 * s_ref / np.sqrt(R_RUN)
    st = dict(theta=res.theta.cpu().numpy(), stage=res.stages, beta=np.where(res.converged, 1.0, 0.0), log_evidence=res.log_evidence,
              hist_beta=np.nan_to_num(res.betas), hist_ess=np.nan_to_num(res.ess), hist_dlogz=np.nan_to_num(res.log_evidence_increments))
    cases.check_run(st, 0.5, N_RUN)
    assert res.as_trace().shape == (N_RUN, R_RUN, 2)


def test_two_modes_from_prior_draws_on_the_device():
    """no start is given: Sobol' draws of the uniform prior through DeviceSMC.prior_draws.  The share of the heavier mode is
    within 5 standard errors of 0.7, the standard error from the restatement's population spread"""
    from hallthrusterpem_amd.calibration import DeviceSMC
    from hallthrusterpem_amd.sampling import UNIFORM, Prior
    priors = {k: Prior(UNIFORM, -cases.BOX, cases.BOX, 'test') for k in ('x0', 'x1')}
    ref = smc_np.run(cases.modes_loglik, cases.modes_logprior, cases.modes_starts(R_RUN, N_RUN), seed=4, tau=0.5, n_mcmc=3)
    s_ref = (ref['theta'][:, :, 0] < 0.0).mean(axis=1).std(ddof=1)
    theta0 = DeviceSMC.prior_draws(('x0', 'x1'), priors, n_particles=N_RUN, n_populations=R_RUN, seed=5, method='sobol')
    assert theta0.shape == (R_RUN, N_RUN, 2) and bool((theta0.abs() <= cases.BOX).all())
    assert not bool((theta0[0] == theta0[1]).all())                       # every population has its own shift
    mc = DeviceSMC.prior_draws(('x0', 'x1'), priors, n_particles=64, n_populations=2, seed=5, method='mc')
    assert mc.shape == (2, 64, 2) and bool((mc.abs() <= cases.BOX).all())
    sm = DeviceSMC(_t('modes_loglik'), _t('modes_logprior'), theta0, n_populations=R_RUN, seed=4)
    res = sm.run()
    share = (res.theta[:, :, 0] < 0.0).double().mean(dim=1).cpu().numpy()
    print(f'share of the heavier mode {share.mean():.4f} s_ref {s_ref:.4f} stages {res.stages.tolist()}')
    assert res.converged.all()
    assert abs(share.mean() - cases.MASS_A) <= 5.0 * s_ref / np.sqrt(R_RUN)
    assert bool((res.theta.abs() <= cases.BOX).all())


def test_the_state_is_consistent_on_a_shared_nuisance_system_posterior():
    """N = 64 particles from prior draws on the synthetic System data of tests/test_optimize.py (three calibrated inputs, M = 8
    shared nuisance draws): the run ends at beta = 1 with a finite evidence, every particle is inside the support, and the stored
    values are the functions re-evaluated at the stored points, bit for bit -- a gather or an accept that moved theta without its
    values would show"""
    import torch
    from hallthrusterpem_amd.calibration import DeviceSMC, SystemPosterior
    from test_optimize import _synthetic
    lik, names, _ = _synthetic()
    N = 64
    post = SystemPosterior(names, lik, n_chains=N, n_nuisance=8, seed=1, fresh_nuisance=False, shared_nuisance=True)
    theta0 = DeviceSMC.prior_draws(names, n_particles=N, seed=2, device=post.device)
    sm = DeviceSMC(post.log_likelihood, post.log_prior, theta0, seed=3, device=post.device)
    res = sm.run(max_stages=200)
    assert res.converged.all() and np.isfinite(res.log_evidence).all() and res.betas[0, res.stages[0] - 1] == 1.0
    flat = res.theta.reshape(N, len(names))
    ll, lp = post.log_likelihood(flat).clone(), post.log_prior(flat).clone()
    assert torch.isfinite(lp).all() and torch.isfinite(ll).all()          # inside the support
    for j, k in enumerate(names):
        p = post.priors[k]
        assert bool(((flat[:, j] >= p.a) & (flat[:, j] <= p.b)).all()), k  # (V_vac, c0, c3 have uniform priors)
    assert torch.equal(res.loglik.reshape(-1), ll) and torch.equal(res.logprior.reshape(-1), lp)
    assert res.as_trace().shape == (N, 1, len(names))
