#!/usr/bin/env python3
"""A posterior with more than one mode: samplers.DeviceTemperedEnsemble (replica exchange over the ensemble sampler) on one
MI355X.

  1. a closed form with two modes -- 0.3 N((-5, 0), I) + 0.7 N((5, 0), I) as the likelihood, a uniform prior on [-15, 15]^2 --
     with every walker started in the 0.3 mode.  DeviceEnsemble from those starts stays there; DeviceTemperedEnsemble (R = 4
     replicas of a ladder of T = 6 temperatures with a final beta = 0, K = 16 walkers) finds the weights, and its swap rates say
     whether the ladder is dense enough;
  2. the log evidence of that problem by thermodynamic integration: 1 / 900 of the mixture's mass, log Z = -log 900 = -6.8024;
  3. a SystemPosterior smoke run (the data of ensemble_sampler.py): the two callables are post.log_likelihood and post.log_prior
     of a posterior with E H rows and shared nuisance draws, a step -- four evaluations and two launches -- is one graph replay.

    python examples/tempered_ensemble.py [n_steps]          (default: 2000 steps of the closed form, n_steps / 10 on the model)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import diagnostics, marginals                                              # noqa: E402
from hallthrusterpem_amd.calibration import DeviceEnsemble, DeviceTemperedEnsemble, SystemPosterior  # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                                          # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                                # noqa: E402

n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
dev = torch.device('cuda')
m1, m2 = torch.tensor([-5.0, 0.0], dtype=torch.float64, device=dev), torch.tensor([5.0, 0.0], dtype=torch.float64, device=dev)


def loglik(x):
    a = np.log(0.3) - 0.5 * ((x - m1) ** 2).sum(-1)
    b = np.log(0.7) - 0.5 * ((x - m2) ** 2).sum(-1)
    return torch.logaddexp(a, b) - np.log(2.0 * np.pi)


def logprior(x):
    inside = (x.abs() <= 15.0).all(-1)
    return torch.where(inside, torch.zeros_like(x[:, 0]) - np.log(900.0), torch.zeros_like(x[:, 0]) - np.inf)


# 1. two modes, every walker started in the lighter one
R, T, K = 4, 6, 16
x0 = DeviceTemperedEnsemble.ball([-5.0, 0.0], 1.0, K, n_temperatures=T + 1, n_replicas=R, seed=1)
plain = DeviceEnsemble(lambda x: loglik(x) + logprior(x), x0[:, 0], seed=2)
share = lambda t: float((t[n_steps // 4:, ..., 0] > 0).double().mean())                              # noqa: E731
print(f'DeviceEnsemble, {R} ensembles x {K} walkers, {n_steps} steps: share of draws in the 0.7 mode {share(plain.run(n_steps)):.3f}')
pt = DeviceTemperedEnsemble(loglik, logprior, x0, n_temperatures=T, beta_min=0.01, include_prior=True, n_replicas=R, seed=2)
torch.cuda.synchronize()
t0 = time.perf_counter()
pt.run(n_steps)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f'DeviceTemperedEnsemble, {R} replicas x {pt.T} temperatures x {K} walkers, {n_steps} steps in {1e3 * dt:.1f} ms '
      f'({1e6 * dt / max(1, n_steps):.1f} us per step, recording the graph included): share in the 0.7 mode {share(pt.cold()):.3f}')
print('  ladder      ' + ' '.join(f'{b:7.4f}' for b in pt.betas))
print('  move rates  ' + ' '.join(f'{v:7.2f}' for v in pt.move_rates().mean(dim=0).tolist()))
print('  swap rates      ' + ' '.join(f'{v:7.2f}' for v in pt.swap_rates().mean(dim=0).tolist()) + '   (t with t + 1; near 0: add a temperature)')
rows = pt.trace.shape[0]
print(diagnostics.format_summary(diagnostics.summary(pt.cold(means=True), names=('x', 'y'), burnin=0.25)))
c = marginals.corner(pt.cold().reshape(rows, R * K, 2), names=('x', 'y'), burnin=0.25, bins=30, points=256)
print(f'  cold marginal of x: mean {float(c["mean"][0]):+.3f} (exact +2.000), std {float(c["cov"][0, 0]) ** 0.5:.3f} (exact 4.690)')

# 2. the evidence
ev = pt.log_evidence(burn=rows // 4)
print(f'log evidence {ev["mean"]:.4f} (replicas {np.round(ev["log_z"], 4).tolist()}, spread {ev["spread"]:.4f}, discretisation '
      f'{float(ev["discretisation"].mean()):.4f}); exact {-np.log(900.0):.4f}')

# 3. on the model: the data of ensemble_sampler.py, two temperatures
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
R, T, K, n = 2, 3, 12, max(1, n_steps // 10)
post = SystemPosterior(names, SystemLikelihood(data), n_chains=R * T * K // 2, n_nuisance=50, seed=1, fresh_nuisance=False,
                       shared_nuisance=True)
pt = DeviceTemperedEnsemble(post.log_likelihood, post.log_prior,
                            DeviceTemperedEnsemble.ball(star, 0.01 * np.abs(star), K, n_temperatures=T, n_replicas=R, seed=4),
                            betas=[1.0, 0.3, 0.1], n_replicas=R, seed=2, de_fraction=0.2, device=post.device)
torch.cuda.synchronize()
t0 = time.perf_counter()
pt.run(n)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
cold = pt.cold()[n // 4:].reshape(-1, len(names))
print(f'SystemPosterior, {R} replicas x {T} temperatures x {K} walkers, {n} steps in {1e3 * dt:.1f} ms ({1e6 * dt / n:.1f} us per step): '
      f'cold mean {cold.mean(0).cpu().numpy()} (theta* = {star}); swap rates {np.round(pt.swap_rates().mean(dim=0).cpu().numpy(), 2).tolist()}, '
      f'mean log likelihood per temperature {np.round(pt.mean_loglik(n // 4).mean(dim=0).cpu().numpy(), 2).tolist()}')
