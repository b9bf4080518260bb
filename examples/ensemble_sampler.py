#!/usr/bin/env python3
"""Sampling without a proposal covariance: samplers.DeviceEnsemble (the affine-invariant ensemble sampler) on one MI355X.

  1. the synthetic V_cc, thrust, ion velocity and ion current density data of calibration_start.py (theta* plus 2 % noise);
  2. where the walkers start: the final population of a differential-evolution MAP search (default: it already has the
     posterior's shape, and nothing else is needed), or with `ball` a 1 % ball round theta*;
  3. DeviceEnsemble: E ensembles of K walkers; half an ensemble's walkers are the E K / 2 rows of ONE posterior evaluation with
     shared nuisance draws, and a step -- two evaluations and two pem_ensemble_step_f64_dev launches -- is one graph replay;
  4. diagnostics of the E ensemble-mean series (the walkers of one ensemble are not independent chains), then
     marginals.corner of all walkers pooled.

    python examples/ensemble_sampler.py [de|ball] [n_steps]          (default: de, 2000 steps of 2 ensembles x 22 walkers)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import diagnostics, marginals                                # noqa: E402
from hallthrusterpem_amd.calibration import DeviceEnsemble, SystemPosterior            # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                            # noqa: E402
from hallthrusterpem_amd.optimize import DifferentialEvolution                         # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                  # noqa: E402

start = sys.argv[1] if len(sys.argv) > 1 else 'de'
n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
if start not in ('de', 'ball'):
    sys.exit(__doc__)
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

# 1. data from the model at theta* with 2 % noise (calibration_start.py, step 1)
truth = Predictive(SystemLikelihood(data), names, seed=1).run(samples=star[None], n_draws=1)
for q, d in data.items():
    t = truth[q]['pred'][0].cpu().numpy()
    d['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
    d['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
lik = SystemLikelihood(data)
M = 50
shared = lambda rows: SystemPosterior(names, lik, n_chains=rows, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                      shared_nuisance=True)

# 2. the starts: no MAP, no Hessian, no cov0
E, K = 2, 22
if start == 'de':
    de = DifferentialEvolution(None, names, seed=3, use_graph=True)              # P = 15 d = 45 members
    de.f = shared(de.P).log_posterior
    res = de.run(200, check_every=20)
    theta0 = de.theta[:E * K].reshape(E, K, len(names)).cpu().numpy()
    print(f'starts: {E * K} members of the DE population after {res.generations} generations (best member '
          + ' '.join(f'{k}={v:.5g}' for k, v in zip(names, res.theta)) + ')')
else:
    theta0 = DeviceEnsemble.ball(star, 0.01 * np.abs(star), K, n_ensembles=E, seed=4)
    print(f'starts: a 1 % ball round theta* = {star}')

# 3. DeviceEnsemble: the posterior has E K / 2 rows and its value must not depend on the row: shared nuisance draws
post = shared(E * K // 2)
sampler = DeviceEnsemble(post.log_posterior, theta0, seed=2, de_fraction=0.2, device=post.device)
torch.cuda.synchronize()
t0 = time.perf_counter()
trace = sampler.run(n_steps)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
keep = trace[n_steps // 10:]
print(f'DeviceEnsemble: {n_steps} steps x {E} ensembles x {K} walkers in {1e3 * dt:.1f} ms ({1e6 * dt / max(1, n_steps):.1f} us per step, '
      f'recording the graph included), acceptance {float(sampler.acceptance.mean()):.2f}; posterior mean '
      f'{keep.reshape(-1, len(names)).mean(0).cpu().numpy()} (theta* = {star})')

# 4. can the trace be trusted?  R-hat and ESS of the ensemble MEANS; the marginals of every walker pooled
diag = diagnostics.summary(trace.mean(dim=2), names=names, burnin=0.1)
print(diagnostics.format_summary(diag))
c = marginals.corner(trace.reshape(n_steps, E * K, len(names)), names=names, burnin=0.1, bins=15, points=256)
dens, grid = c['density'].cpu().numpy(), c['grid'].cpu().numpy()
for i, k in enumerate(c['names']):
    print(f'  {k:>6}: mean {float(c["mean"][i]):.5g}, KDE mode {grid[i, dens[i].argmax()]:.5g}, std {float(c["cov"][i, i]) ** 0.5:.3g}, '
          f'theta* {star[i]:.5g}')
for i in range(len(names)):
    for j in range(i + 1, len(names)):
        print(f'  ({names[i]}, {names[j]}): correlation {float(c["corr"][i, j]):+.3f}, 50 % / 90 % levels {c["levels"][i, j].tolist()}')
