"""Every sampler's transition kernel on the MI355X against the target it must preserve: the cases, sizes, seeds and statistics of
tests/stationarity_cases.py, which tests/test_stationarity_host.py proves the numpy restatements to pass and one-slip mutants of
them to fail.  Starts are exact draws of a closed-form target made on the host; a few steps of a non-adaptive kernel later every
point must still be one, and every statistic within 5 of its exact-null standard errors.  No number here comes from a device run."""
import numpy as np
import pytest

import stationarity_cases as sc

pytestmark = pytest.mark.gpu
HUGE = 1 << 40                                         # adapt_after: no adaptation within any run here
TARGETS = pytest.mark.parametrize('target', [sc.TARGET_A, sc.TARGET_B], ids=['A', 'B'])


def _device():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def _logp(target):
    """`target.logp` as a torch callable on the device (its constants are on the device before any capture)"""
    import torch
    dev = _device()
    mu, prec = torch.as_tensor(target.mean, device=dev), torch.as_tensor(target.prec, device=dev)

    def logp(t):
        r = t - mu
        lp = -0.5 * torch.einsum('ki,ij,kj->k', r, prec, r)
        if target.edge is None:
            return lp
        return torch.where(t[:, target.edge[0]] > target.edge[1], lp, torch.full_like(lp, -float('inf')))
    return logp


def _gauss():
    """sc.gauss_loglik and sc.gauss_logprior as torch callables on the device"""
    import torch
    lik_mean = torch.as_tensor(sc.LIK_MEAN, device=_device())
    return (lambda x: -0.5 * (((x - lik_mean) / sc.LIK_STD) ** 2).sum(dim=-1)), (lambda x: -0.5 * ((x / sc.PRIOR_STD) ** 2).sum(dim=-1))


def _holds(label, z):
    assert sc.report(label, z) <= sc.Z_DEVICE, z


@TARGETS
def test_device_dram_preserves_its_target(target):
    from hallthrusterpem_amd.calibration import DeviceDRAM
    s = DeviceDRAM(_logp(target), sc.dram_starts(target), cov0=sc.DRAM_COV0, seed=sc.DRAM_SEED, adapt_after=HUGE, gamma=sc.GAMMA)
    assert s.run(sc.DRAM_STEPS, keep=False) is None and s.steps == sc.DRAM_STEPS
    theta = s.theta.cpu().numpy()
    _holds('DeviceDRAM', sc.dram_z(theta, target))
    accepted = s.accepted.cpu().numpy()
    assert accepted[0].sum() > 0 and accepted[1].sum() > 0 and s.adaptation_failures == 0
    assert target.inside(theta).all()


def test_the_torch_dram_preserves_its_target():
    """calibration.DRAM, the sampler written in torch operations, on the device with torch's generator: the same function"""
    from hallthrusterpem_amd.calibration import DRAM
    target = sc.TARGET_A
    s = DRAM(_logp(target), sc.dram_starts(target), cov0=sc.DRAM_COV0, seed=sc.DRAM_SEED, adapt_after=HUGE, gamma=sc.GAMMA, device=_device())
    s.run(sc.DRAM_STEPS, keep=False)
    _holds('DRAM (torch)', sc.dram_z(s.theta.cpu().numpy(), target))
    accepted = s.accepted.cpu().numpy()
    assert accepted[0].sum() > 0 and accepted[1].sum() > 0


@pytest.mark.parametrize('de_fraction', [0.0, 1.0, 0.5])
@TARGETS
def test_device_ensemble_preserves_its_target(target, de_fraction):
    from hallthrusterpem_amd.calibration import DeviceEnsemble
    s = DeviceEnsemble(_logp(target), sc.ensemble_starts(target), n_ensembles=sc.ENS_E, seed=sc.ENS_SEED, de_fraction=de_fraction)
    s.run(sc.ENS_STEPS, keep=False)
    theta = s.theta.cpu().numpy()
    _holds(f'DeviceEnsemble, de_fraction {de_fraction}', sc.ensemble_z(theta, target))
    assert int(s.accepted.sum()) > 0 and target.inside(theta).all()


def test_device_tempered_ensemble_preserves_every_rung():
    from hallthrusterpem_amd.calibration import DeviceTemperedEnsemble
    loglik, logprior = _gauss()
    s = DeviceTemperedEnsemble(loglik, logprior, sc.tempering_starts(), betas=sc.TEMP_BETAS, n_replicas=sc.TEMP_R, seed=sc.TEMP_SEED)
    s.run(sc.TEMP_STEPS, keep=False)
    _holds('DeviceTemperedEnsemble', sc.tempering_z(s.theta.cpu().numpy()))
    attempts, taken = s.swap_attempts.cpu().numpy(), s.swap_accepted.cpu().numpy()
    assert (attempts > 0).all() and (taken.sum(axis=0) > 0).all()
    assert int(s.accepted.sum()) > 0


@pytest.mark.parametrize('beta', sc.SMC_BETAS)
def test_the_smc_move_kernel_preserves_the_tempered_target(beta):
    """tests/test_smc.py's way to the move launch: a DeviceSMC without a graph, `_prepare`, the state words written by the test
    (beta, the factor, stage 1, moves on) and `_launch_move`.  The pending proposal of move 1 is every particle itself with its
    own values: it is accepted and changes nothing, and moves 2 ... SMC_MOVES are random-walk Metropolis steps on exact draws of
    prior x likelihood^beta."""
    import torch
    from hallthrusterpem_amd.calibration import DeviceSMC
    loglik, logprior = _gauss()
    sm = DeviceSMC(loglik, logprior, sc.smc_starts(beta), n_populations=sc.SMC_R, n_mcmc=sc.SMC_MOVES, seed=sc.SMC_SEED, use_graph=False,
                   device=_device())
    sm._prepare(1)
    sm.beta.fill_(beta)
    sm.L.copy_(torch.as_tensor(sc.SMC_L, device=sm.device).expand(sm.R, sm.d, sm.d))
    sm.stage.fill_(1)
    sm.moves_active.fill_(1)
    sm.prop.copy_(sm.theta)
    sm.prop_loglik.copy_(sm.loglik)
    sm.prop_logprior.copy_(sm.logprior)
    flat = sm.prop.view(sm.R * sm.N, sm.d)
    for m in range(1, sc.SMC_MOVES + 1):
        if m > 1:
            sm.prop_loglik.view(-1).copy_(loglik(flat))
            sm.prop_logprior.view(-1).copy_(logprior(flat))
        sm._launch_move(m, m < sc.SMC_MOVES)
    torch.cuda.synchronize()
    _holds(f'SMC move kernel, beta {beta}', sc.smc_z(sm.theta.cpu().numpy(), beta))
    moved = sm.accept_count.cpu().numpy().astype(np.int64) - 1                      # (move 1 accepts the particle itself)
    assert (moved >= 0).all() and 0 < moved.sum() < moved.size * (sc.SMC_MOVES - 1)
    assert sm.beta.cpu().numpy().tolist() == [beta] * sc.SMC_R and not sm.flags.any()
