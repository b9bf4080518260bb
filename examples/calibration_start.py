#!/usr/bin/env python3
"""Where to start the chains, with no hand-typed numbers: the steps of scripts/pem_v0/mcmc.py before run_mcmc on one MI355X.

  1. synthetic V_cc, thrust, ion velocity and ion current density data at a known theta* plus 2 % noise (as predictive_check.py);
  2. the maximum a posteriori point by differential evolution over the prior's quantiles (optimize.DifferentialEvolution:
     the whole population is the rows of one posterior launch with shared nuisance draws, a generation is one graph replay);
  3. the Laplace approximation there (optimize.Laplace: a 2 d^2 + 1 point central-difference Hessian in one launch);
  4. DRAM started from Laplace.dram_start();
  5. the chains' diagnostics (diagnostics.summary: split R-hat, ESS and MCSE beside the posterior's percentiles).

    python examples/calibration_start.py [n_steps]          (default 300 DRAM steps of 16 chains)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import diagnostics                                           # noqa: E402
from hallthrusterpem_amd.calibration import DRAM, SystemPosterior                      # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                            # noqa: E402
from hallthrusterpem_amd.optimize import DifferentialEvolution, Laplace, stencil_size  # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                  # noqa: E402

n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
t_start = time.perf_counter()
rng = np.random.default_rng(0)
op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
na = 25
data = {'V_cc': {'x': op(4), 'y': np.zeros(4), 'var_y': np.ones(4)},
        'T': {'x': op(3), 'y': np.zeros(3), 'var_y': np.ones(3)},
        'uion': {'x': op(2), 'y': np.zeros((2, 6)), 'var_y': np.ones((2, 6)), 'loc': np.linspace(0.005, 0.075, 6)},
        'jion': {'x': op(5), 'y': np.zeros((5, na)), 'var_y': np.ones((5, na)),
                 'loc': np.stack([np.ones(na), np.linspace(-1.5, 1.5, na)], 1)}}
# predictive_check.py's inputs without T_e and P_T: the cathode's V_cc is the only data on them and hardly constrains them
# (calibrated, the two trade off along a ridge, and T_e alone runs to a bound of its prior)
names = ('V_vac', 'c0', 'c3')
star = np.array([30.0, 0.5, 0.8])

# 1. data from the model at theta* with 2 % noise; every other input at the first nuisance draw of the posterior's own design
#    (seed 1), so that one of the M draws below reproduces the data and theta* is identifiable
truth = Predictive(SystemLikelihood(data), names, seed=1).run(samples=star[None], n_draws=1)
for q, d in data.items():
    t = truth[q]['pred'][0].cpu().numpy()
    d['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
    d['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
lik = SystemLikelihood(data)
M = 50
shared = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)

# 2. MAP by differential evolution (scipy's defaults: popsize 15, best1bin, F ~ U(0.5, 1), CR 0.7; tol is relative to
#    |mean log posterior|, and scipy's 0.01 would stop a few units of log posterior short of the maximum here)
de = DifferentialEvolution(None, names, seed=3, tol=1e-4, use_graph=True)
de.f = shared(de.P).log_posterior
torch.cuda.synchronize()
t0 = time.perf_counter()
res = de.run(1000, check_every=20)
torch.cuda.synchronize()
t_de = time.perf_counter() - t0
print(f'MAP: differential evolution, population {de.P}, {res.generations} generations (converged: {res.converged}) in '
      f'{1e3 * t_de:.1f} ms; log posterior {res.value:.3f}')
print(f'  {"":>6} {"MAP":>12} {"theta*":>12}')
for k, m, s in zip(names, res.theta, star):
    print(f'  {k:>6} {m:12.5g} {s:12.5g}')

# 3. Laplace approximation at the MAP
hess_post = shared(stencil_size(len(names)))
torch.cuda.synchronize()
t0 = time.perf_counter()
lap = Laplace.fit(hess_post.log_posterior, res.theta, names, device=hess_post.device)
t_lap = time.perf_counter() - t0
print(f'Laplace: Hessian over {stencil_size(len(names))} points in {1e3 * t_lap:.1f} ms; nearest-PD fall-back: {lap.nearest_pd}')
print('  standard deviations ' + ' '.join(f'{k}={s:.3g}' for k, s in zip(names, lap.std)))
print('  (MAP - theta*) / std ' + ' '.join(f'{z:+.2f}' for z in (res.theta - star) / lap.std))

# 4. DRAM from the Laplace approximation, on the posterior it approximates
K = 16
post = shared(K)
theta0, cov0 = lap.dram_start()
t0 = time.perf_counter()
sampler = DRAM(post.log_posterior, theta0, cov0=cov0, n_chains=K, seed=2, adapt_after=100, adapt_interval=50, device=post.device)
trace = sampler.run(n_steps)
torch.cuda.synchronize()
print(f'DRAM: {n_steps} steps x {K} chains in {time.perf_counter() - t0:.1f} s, stage-1 acceptance '
      f'{float(sampler.acceptance[0].mean()):.2f}; posterior mean '
      f'{trace[n_steps // 10:].reshape(-1, len(names)).mean(0).cpu().numpy()} (theta* = {star})')

# 5. can the trace be trusted?  show_mcmc / journal_plots with split R-hat, ESS and MCSE (10 % burn-in)
t0 = time.perf_counter()
diag = diagnostics.summary(trace, names=names, burnin=0.1, acceptance=sampler.acceptance)
print(f'diagnostics in {1e3 * (time.perf_counter() - t0):.1f} ms')
print(diagnostics.format_summary(diag))
print(f'total {time.perf_counter() - t_start:.1f} s')
