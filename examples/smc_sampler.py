#!/usr/bin/env python3
"""Calibration without a start: samplers.DeviceSMC (tempered sequential Monte Carlo) on one MI355X.

  1. a closed form with two modes -- 0.3 N((-5, 0), I) + 0.7 N((5, 0), I) as the likelihood, a uniform prior on [-15, 15]^2 -- from
     Sobol' draws of the prior: no start, no covariance, no ladder.  The particles at beta = 1 are equally weighted posterior
     draws (the share of the 0.7 mode, the marginals through marginals.corner) and the run returns the log evidence,
     log Z = -log 900 = -6.8024, with its spread over the populations;
  2. a SystemPosterior (the data of ensemble_sampler.py): prior draws of three calibrated inputs -> DeviceSMC -> marginals.corner
     and log_evidence.  The two callables are post.log_likelihood and post.log_prior of a posterior with R N rows and shared
     nuisance draws; a stage -- a stage launch, n_mcmc evaluations and move launches -- is one graph replay.

    python examples/smc_sampler.py [n_particles]          (default: 1024 particles of the closed form, a quarter on the model)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import marginals                                                            # noqa: E402
from hallthrusterpem_amd.calibration import DeviceSMC, SystemPosterior                               # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                                          # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                                # noqa: E402
from hallthrusterpem_amd.sampling import UNIFORM, Prior                                              # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
dev = torch.device('cuda')
m1, m2 = torch.tensor([-5.0, 0.0], dtype=torch.float64, device=dev), torch.tensor([5.0, 0.0], dtype=torch.float64, device=dev)


def loglik(x):
    a = np.log(0.3) - 0.5 * ((x - m1) ** 2).sum(-1)
    b = np.log(0.7) - 0.5 * ((x - m2) ** 2).sum(-1)
    return torch.logaddexp(a, b) - np.log(2.0 * np.pi)


def logprior(x):
    inside = (x.abs() <= 15.0).all(-1)
    return torch.where(inside, torch.zeros_like(x[:, 0]) - np.log(900.0), torch.zeros_like(x[:, 0]) - np.inf)


# 1. two modes from prior draws
R = 8
box = {k: Prior(UNIFORM, -15.0, 15.0, 'example') for k in ('x', 'y')}
theta0 = DeviceSMC.prior_draws(('x', 'y'), box, n_particles=N, n_populations=R, seed=1)
smc = DeviceSMC(loglik, logprior, theta0, n_populations=R, seed=2)
torch.cuda.synchronize()
t0 = time.perf_counter()
res = smc.run()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f'DeviceSMC, {R} populations x {N} particles: beta = 1 after {res.stages.tolist()} stages in {1e3 * dt:.1f} ms (recording the graph '
      f'included), {R * N * (1 + smc.n_mcmc * int(res.stages.max()))} evaluations')
print('  betas of population 0       ' + ' '.join(f'{b:.4g}' for b in res.betas[0, :res.stages[0]]))
print('  acceptance of population 0  ' + ' '.join(f'{a:.2f}' for a in res.acceptance[0, :res.stages[0]]))
share = (res.theta[:, :, 0] > 0).double().mean(dim=1).cpu().numpy()
print(f'  share of the particles in the 0.7 mode {share.mean():.3f} +- {share.std(ddof=1) / np.sqrt(R):.3f}')
print(f'  log evidence {res.log_evidence.mean():.4f} +- {res.log_evidence.std(ddof=1) / np.sqrt(R):.4f} (populations '
      f'{np.round(res.log_evidence, 3).tolist()}); exact {-np.log(900.0):.4f}')
c = marginals.corner(res.as_trace(), names=('x', 'y'), burnin=0, bins=30, points=256)   # particles, not a chain: nothing to burn
print(f'  marginal of x: mean {float(c["mean"][0]):+.3f} (exact +2.000), std {float(c["cov"][0, 0]) ** 0.5:.3f} (exact 4.690)')

# 2. on the model: the data of ensemble_sampler.py, from draws of the PEM-v0 priors
rng = np.random.default_rng(0)
op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
na = 25
data = {'V_cc': {'x': op(4), 'y': np.zeros(4), 'var_y': np.ones(4)},
        'T': {'x': op(3), 'y': np.zeros(3), 'var_y': np.ones(3)},
        'uion': {'x': op(2), 'y': np.zeros((2, 6)), 'var_y': np.ones((2, 6)), 'loc': np.linspace(0.005, 0.075, 6)},
        'jion': {'x': op(5), 'y': np.zeros((5, na)), 'var_y': np.ones((5, na)),
                 'loc': np.stack([np.ones(na), np.linspace(-1.5, 1.5, na)], 1)}}
names = ('V_vac', 'c0', 'c3')
star = np.array([30.0, 0.5, 0.8])
truth = Predictive(SystemLikelihood(data), names, seed=1).run(samples=star[None], n_draws=1)
for q, d in data.items():
    t = truth[q]['pred'][0].cpu().numpy()
    d['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
    d['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
R, n = 2, max(64, N // 4)
post = SystemPosterior(names, SystemLikelihood(data), n_chains=R * n, n_nuisance=50, seed=1, fresh_nuisance=False, shared_nuisance=True)
theta0 = DeviceSMC.prior_draws(names, n_particles=n, n_populations=R, seed=4, device=post.device)
smc = DeviceSMC(post.log_likelihood, post.log_prior, theta0, n_populations=R, seed=2, device=post.device)
torch.cuda.synchronize()
t0 = time.perf_counter()
res = smc.run()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
c = marginals.corner(res.as_trace(), names=names, burnin=0, bins=30, points=256)
print(f'SystemPosterior, {R} populations x {n} particles from prior draws: {res.stages.tolist()} stages in {1e3 * dt:.1f} ms, converged '
      f'{res.converged.tolist()}, flags {res.flags.tolist()}')
print(f'  posterior mean {np.round(torch.as_tensor(c["mean"]).cpu().numpy(), 4).tolist()} (theta* = {star.tolist()}), log evidence '
      f'{np.round(res.log_evidence, 3).tolist()}')
