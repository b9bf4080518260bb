"""The invariance tests of tests/stationarity_cases.py on the numpy restatements of the samplers, without a GPU: started from exact
draws of its target, each restatement as committed leaves every statistic within 4 exact-null standard errors, and each with one
slip in its accept rule -- applied here by wrapping the restatement, whose file stays as it is -- is at least 10 off.  The cases,
sizes and seeds are those of tests/test_stationarity.py, so what passes here is what the device must reproduce, and what fails
here is what the device test would catch in a kernel."""
import numpy as np
import pytest

import dram_np
import ensemble_np
import smc_np
import stationarity_cases as sc
import tempering_np

HUGE = 1 << 40                                         # adapt_after: no adaptation within any run here


# ------------------------------------------------------------------------------------------------------------------ drivers
def run_dram(target, theta0, n_steps=sc.DRAM_STEPS, seed=sc.DRAM_SEED):
    """launch 0 and n_steps launches of tests/dram_np.py as calibration.DeviceDRAM drives the kernel, never adapting"""
    K, d = theta0.shape
    L = np.broadcast_to(np.linalg.cholesky(sc.DRAM_COV0), (K, d, d)).copy()
    st = dict(theta=theta0.copy(), logp=target.logp(theta0), L=L, mean=theta0.copy(), scatter=np.zeros((K, d, d)), prop=np.zeros((2, K, d)),
              state=np.zeros(K, dtype=np.int64), accepted=np.zeros((2, K), dtype=np.int64), flags=np.zeros(K, dtype=np.int32))
    kw = dict(seed=seed, gamma=sc.GAMMA, eps=1e-12, adapt_after=HUGE, adapt_interval=1)
    st, _ = dram_np.step(st, np.zeros((2, K)), **kw)
    for _ in range(n_steps):
        st, _ = dram_np.step(st, target.logp(st['prop']), **kw)
    return st


def run_smc_moves(beta, theta0, n_moves=sc.SMC_MOVES, seed=sc.SMC_SEED):
    """n_moves move launches of tests/smc_np.py on particles at a fixed beta and factor: the pending proposal of move 1 is every
    particle itself with its own values (accepted, changing nothing), so moves 2 ... n_moves are random-walk Metropolis steps"""
    R, N, d = theta0.shape
    flat = theta0.reshape(R * N, d)
    st = smc_np.new_state(theta0, sc.gauss_loglik(flat), sc.gauss_logprior(flat), history_len=1)
    st.update(beta=np.full(R, beta), L=np.broadcast_to(sc.SMC_L, (R, d, d)).copy(), stage=np.ones(R, dtype=np.int64),
              moves_active=np.ones(R, dtype=np.uint32), prop=theta0.copy())
    for m in range(1, n_moves + 1):
        flat = st['prop'].reshape(R * N, d)
        st, _ = smc_np.move(st, sc.gauss_loglik(flat), sc.gauss_logprior(flat), seed, n_moves, m, propose_next=m < n_moves)
    return st


def _holds(label, z):
    assert sc.report(label, z) <= sc.Z_HOST, z


def _breaks(label, z):
    assert sc.report(label, z) >= sc.Z_MUTANT, z


# ------------------------------------------------------------------------------------------------------------- the yardstick
def test_the_statistics_know_exact_draws_from_draws_of_a_neighbouring_law():
    """an edge that cuts 31 % of the mass away (c = -0.5; target B's cuts 0.27 %, too little to tell a wrong truncated moment from
    a right one): the closed-form moments are scipy's, exact draws pass, and the same draws judged without the edge, or draws
    5 % too wide judged as the Gaussian, do not"""
    from scipy.stats import truncnorm
    low = sc.MU[2] - 0.5 * np.linalg.norm(sc.CHOL[2])
    cut = sc.Target(sc.MU, sc.CHOL, edge=(2, low))
    want = [truncnorm.moment(k, -0.5, np.inf) for k in (1, 2, 3, 4)]
    assert np.allclose(cut.moments[:, 0], want, rtol=1e-12, atol=0) and np.array_equal(cut.moments[:, 1], [0.0, 1.0, 0.0, 3.0])
    assert np.allclose(cut.reflect @ cut.reflect.T, np.eye(3), atol=1e-15) and np.allclose(cut.reflect[0] * np.linalg.norm(sc.CHOL[2]), sc.CHOL[2])
    n = 1 << 16
    x = cut.draw(np.random.default_rng(1), n)
    assert x.shape == (n, 3) and cut.inside(x).all() and np.isneginf(cut.logp(x - [0.0, 0.0, 10.0])).all()
    assert sc.worst(sc.z_scores(cut, x, n))[1] <= sc.Z_HOST
    assert sc.worst(sc.z_scores(sc.TARGET_A, x, n))[1] >= sc.Z_MUTANT
    y = sc.TARGET_A.draw(np.random.default_rng(2), n)
    assert sc.worst(sc.z_scores(sc.TARGET_A, y, n, pearson=True))[1] <= sc.Z_HOST
    wide = sc.MU + 1.05 * (y - sc.MU)
    assert sc.worst(sc.z_scores(sc.TARGET_A, wide, n, pearson=True))[1] >= sc.Z_MUTANT
    # K copies of every point are K fully dependent walkers: with the unit's standard error the z of the n points comes back
    assert sc.z_scores(sc.TARGET_A, np.repeat(y, 6, axis=0), n, pearson=True) == pytest.approx(sc.z_scores(sc.TARGET_A, y, n, pearson=True), abs=1e-9)


# --------------------------------------------------------------------------------------------------------------------- DRAM
def dram_decide_with(log_q=True, log1p=True, reverse_from_lp1=True):
    """tests/dram_np.py's `decide` with terms of the delayed stage's ratio left out, or its reverse first-stage ratio taken
    as lp2 - lp1"""
    committed = dram_np.decide

    def decide(lp0, lp1, lp2, z1, z2, u1, u2, gamma):
        rec = committed(lp0, lp1, lp2, z1, z2, u1, u2, gamma)
        w = z1 - np.sqrt(gamma) * z2
        with np.errstate(all='ignore'):
            rev = (lp1 - lp2) if reverse_from_lp1 else (lp2 - lp1)
            a1_rev = np.exp(np.where(rev > 0.0, 0.0, rev))
            log_a2 = lp2 - lp0
            if log_q:
                log_a2 = log_a2 + -0.5 * ((w * w).sum(axis=1) - (z1 * z1).sum(axis=1))
            if log1p:
                log_a2 = (log_a2 + np.log1p(-a1_rev)) - np.log1p(-rec['a1'])
            return dict(rec, log_a2=log_a2, acc2=~rec['acc1'] & (rec['log_u2'] < log_a2))
    return decide


@pytest.mark.parametrize('target', [sc.TARGET_A, sc.TARGET_B], ids=['A', 'B'])
def test_the_dram_restatement_preserves_its_target(target):
    st = run_dram(target, sc.dram_starts(target))
    _holds('DRAM restatement', sc.dram_z(st['theta'], target))
    assert st['accepted'][0].sum() > 0 and st['accepted'][1].sum() > 0 and target.inside(st['theta']).all()


def test_the_wrapper_that_makes_the_dram_mutants_is_the_committed_rule_when_nothing_is_left_out(monkeypatch):
    target = sc.TARGET_B
    theta0 = sc.dram_starts(target)[:4096]
    want = run_dram(target, theta0, n_steps=3)
    monkeypatch.setattr(dram_np, 'decide', dram_decide_with())
    got = run_dram(target, theta0, n_steps=3)
    assert np.array_equal(got['theta'], want['theta']) and np.array_equal(got['accepted'], want['accepted'])


@pytest.mark.parametrize('left_out', ['log_q', 'log1p'])
def test_a_dram_restatement_without_a_term_of_the_delayed_ratio_does_not(left_out, monkeypatch):
    monkeypatch.setattr(dram_np, 'decide', dram_decide_with(**{left_out: False}))
    st = run_dram(sc.TARGET_A, sc.dram_starts(sc.TARGET_A))
    _breaks(f'DRAM without {left_out}', sc.dram_z(st['theta'], sc.TARGET_A))


def test_the_torch_dram_preserves_its_target_on_the_cpu():
    """calibration.DRAM is torch operations and runs anywhere: the case of tests/test_stationarity.py with the CPU's generator.  It
    has no restatement to differ from in a last bit, so its bound is the pass condition itself."""
    import torch
    from hallthrusterpem_amd.calibration import DRAM
    target = sc.TARGET_A
    mu, prec = torch.as_tensor(target.mean), torch.as_tensor(target.prec)

    def logp(t):
        r = t - mu
        return -0.5 * torch.einsum('ki,ij,kj->k', r, prec, r)
    s = DRAM(logp, sc.dram_starts(target), cov0=sc.DRAM_COV0, seed=sc.DRAM_SEED, adapt_after=HUGE, gamma=sc.GAMMA)
    s.run(sc.DRAM_STEPS, keep=False)
    assert sc.report('DRAM (torch, CPU)', sc.dram_z(s.theta.numpy(), target)) <= sc.Z_DEVICE
    assert int(s.accepted[0].sum()) > 0 and int(s.accepted[1].sum()) > 0


# ----------------------------------------------------------------------------------------------------------------- ensemble
def stretch_weight(power):
    """tests/ensemble_np.py's `propose` with z^power in place of z^(d - 1) as the stretch move's weight"""
    committed = ensemble_np.propose

    def propose(theta, half, mv):
        prop, log_q = committed(theta, half, mv)
        return prop, log_q * (float(power) / float(theta.shape[2] - 1))          # (the DE move's 0 stays 0)
    return propose


@pytest.mark.parametrize('de_fraction', [0.0, 1.0, 0.5])
@pytest.mark.parametrize('target', [sc.TARGET_A, sc.TARGET_B], ids=['A', 'B'])
def test_the_ensemble_restatement_preserves_its_target(target, de_fraction):
    st = ensemble_np.run(target.logp, sc.ensemble_starts(target), sc.ENS_STEPS, seed=sc.ENS_SEED, de_fraction=de_fraction)
    _holds(f'ensemble restatement, de_fraction {de_fraction}', sc.ensemble_z(st['theta'], target))
    assert st['accepted'].sum() > 0 and target.inside(st['theta']).all()


@pytest.mark.parametrize('power', [sc.D, sc.D - 2])
def test_an_ensemble_restatement_with_another_power_of_z_does_not(power, monkeypatch):
    monkeypatch.setattr(ensemble_np, 'propose', stretch_weight(power))
    st = ensemble_np.run(sc.TARGET_A.logp, sc.ensemble_starts(sc.TARGET_A), sc.ENS_STEPS, seed=sc.ENS_SEED)
    _breaks(f'stretch move with z^{power}', sc.ensemble_z(st['theta'], sc.TARGET_A))


# ---------------------------------------------------------------------------------------------------------------- tempering
def run_tempering(betas=sc.TEMP_BETAS):
    return tempering_np.run(sc.gauss_loglik, sc.gauss_logprior, sc.tempering_starts(), np.asarray(betas), sc.TEMP_STEPS, seed=sc.TEMP_SEED,
                            keep_theta=False)


def test_the_tempering_restatement_preserves_every_rung(monkeypatch):
    st = run_tempering()
    _holds('tempering restatement', sc.tempering_z(st['theta']))
    assert (st['swap_attempts'] > 0).all() and (st['swap_accepted'].sum(axis=0) > 0).all()


def test_a_tempering_restatement_whose_swap_ratio_has_the_other_sign_does_not(monkeypatch):
    """`run` is handed the ladder negated, which turns the sign of (beta_t - beta_t+1) in the swap rule, and `decide` gets it back"""
    committed = tempering_np.decide
    monkeypatch.setattr(tempering_np, 'decide', lambda lo, po, ln, pn, log_q, beta, u: committed(lo, po, ln, pn, log_q, -beta, u))
    _breaks('tempering, swap sign', sc.tempering_z(run_tempering(-np.asarray(sc.TEMP_BETAS))['theta']))


def test_a_tempering_restatement_that_tempers_the_prior_as_well_does_not(monkeypatch):
    committed = tempering_np.decide
    monkeypatch.setattr(tempering_np, 'decide',
                        lambda lo, po, ln, pn, log_q, beta, u: committed(lo, beta * po, ln, beta * pn, log_q, beta, u))
    _breaks('tempering, prior tempered', sc.tempering_z(run_tempering()['theta']))


# ----------------------------------------------------------------------------------------------------------------- SMC move
@pytest.mark.parametrize('beta', sc.SMC_BETAS)
def test_the_smc_move_restatement_preserves_the_tempered_target(beta):
    st = run_smc_moves(beta, sc.smc_starts(beta))
    _holds(f'SMC move restatement, beta {beta}', sc.smc_z(st['theta'], beta))
    moved = st['accept_count'].astype(np.int64) - 1                                 # (move 1 accepts the particle itself)
    assert (moved >= 0).all() and 0 < moved.sum() < moved.size * (sc.SMC_MOVES - 1)


def test_an_smc_move_restatement_that_forgets_beta_does_not(monkeypatch):
    committed = smc_np.move

    def move(st, *args, **kw):
        out, rec = committed(dict(st, beta=np.ones_like(st['beta'])), *args, **kw)
        out['beta'] = np.array(st['beta'], copy=True)
        return out, rec
    monkeypatch.setattr(smc_np, 'move', move)
    beta = sc.SMC_BETAS[0]
    _breaks('SMC move without beta', sc.smc_z(run_smc_moves(beta, sc.smc_starts(beta))['theta'], beta))
