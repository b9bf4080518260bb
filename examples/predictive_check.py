#!/usr/bin/env python3
"""Does the calibrated model reproduce the data?  The validation step of scripts/pem_v0/monte_carlo.py on one MI355X:

  1. synthetic V_cc, thrust, ion velocity and ion current density data, made by the model at a known theta* plus 2 % noise;
  2. a short DRAM run of the `System` posterior (calibration.SystemPosterior: all four quantities in one fused launch);
  3. prior and posterior predictive runs (predictive.Predictive): predictions at every dataset's conditions and locations,
     5 / 50 / 95 % bands, noisy bands and the relative L2 table of print_l2_error.

    python examples/predictive_check.py [n_steps]          (default 300 DRAM steps of 16 chains)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd.calibration import DRAM, SystemPosterior      # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood            # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                  # noqa: E402

n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rng = np.random.default_rng(0)
op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
na = 25
data = {'V_cc': {'x': op(4), 'y': np.zeros(4), 'var_y': np.ones(4)},
        'T': {'x': op(3), 'y': np.zeros(3), 'var_y': np.ones(3)},
        'uion': {'x': op(2), 'y': np.zeros((2, 6)), 'var_y': np.ones((2, 6)), 'loc': np.linspace(0.005, 0.075, 6)},
        'jion': {'x': op(5), 'y': np.zeros((5, na)), 'var_y': np.ones((5, na)),
                 'loc': np.stack([np.ones(na), np.linspace(-1.5, 1.5, na)], 1)}}
names = ('T_e', 'V_vac', 'P_T', 'c0', 'c3')
star = np.array([3.0, 30.0, 5e-5, 0.5, 0.8])

# 1. data from the model at theta* (every other input at its prior draw), 2 % noise
truth = Predictive(SystemLikelihood(data), names, seed=7).run(samples=star[None], n_draws=1)
for q, d in data.items():
    t = truth[q]['pred'][0].cpu().numpy()
    d['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
    d['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
lik = SystemLikelihood(data)

# 2. a short DRAM run from the middle of the priors
K = 16
post = SystemPosterior(names, lik, n_chains=K, n_nuisance=50, seed=1)
t0 = time.perf_counter()
sampler = DRAM(post.log_posterior, np.array([2.5, 25.0, 4e-5, 0.4, 0.9]), cov0=np.array([0.1, 4.0, 1e-11, 1e-3, 4e-3]) / 10,
               n_chains=K, seed=2, adapt_after=100, adapt_interval=50, device=post.device)
trace = sampler.run(n_steps)
torch.cuda.synchronize()
print(f'DRAM: {n_steps} steps x {K} chains in {time.perf_counter() - t0:.1f} s, stage-1 acceptance '
      f'{float(sampler.acceptance[0].mean()):.2f}; posterior mean {trace[n_steps // 10:].reshape(-1, len(names)).mean(0).cpu().numpy()}'
      f' (theta* = {star})')

# 3. prior and posterior predictive checks
pp = Predictive(lik, names, seed=3)
t0 = time.perf_counter()
prior = pp.run(samples=None, n_draws=2000)
posterior = pp.run(samples=trace, n_draws=2000, burnin=0.1, noise=True)
torch.cuda.synchronize()
print(f'predictive runs: {1e3 * (time.perf_counter() - t0):.1f} ms for 2 x 2000 draws x {lik.n_cond} conditions')
print(pp.table(prior, posterior, noise={'V_cc': 0.02, 'T': 0.02, 'uion': 0.02, 'jion': 0.02}))
lo, med, hi = posterior['V_cc']['bands'].cpu().numpy()
nlo, nhi = posterior['V_cc']['bands_noisy'].cpu().numpy()
for e in range(len(med)):
    print(f'V_cc condition {e}: data {data["V_cc"]["y"][e]:7.3f} V   posterior 5/50/95 % {lo[e]:7.3f} {med[e]:7.3f} {hi[e]:7.3f}'
          f'   with noise {nlo[e]:7.3f} {nhi[e]:7.3f}')
