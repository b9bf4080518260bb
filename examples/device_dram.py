#!/usr/bin/env python3
"""The sampler of examples/calibration_start.py step 4 with nothing left on the host: samplers.DeviceDRAM on one MI355X.

  1. the synthetic V_cc, thrust, ion velocity and ion current density data of calibration_start.py (theta* plus 2 % noise);
  2. MAP by differential evolution and the Laplace approximation there, as steps 2 and 3 of that example;
  3. DeviceDRAM started from Laplace.dram_start(): K chains, both proposals of every chain are the 2K rows of ONE posterior
     evaluation with shared nuisance draws, and a step -- that evaluation and one pem_dram_step_f64_dev launch -- is one
     graph replay;
  4. the chains' diagnostics (diagnostics.summary / format_summary), which take the device trace as it is.

    python examples/device_dram.py [n_steps]          (default 2000 steps of 16 chains)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import diagnostics                                           # noqa: E402
from hallthrusterpem_amd.calibration import DeviceDRAM, SystemPosterior                # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                            # noqa: E402
from hallthrusterpem_amd.optimize import DifferentialEvolution, Laplace, stencil_size  # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                  # noqa: E402

n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
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
shared = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)

# 2. where to start: the MAP and the Laplace covariance there
de = DifferentialEvolution(None, names, seed=3, tol=1e-4, use_graph=True)
de.f = shared(de.P).log_posterior
res = de.run(1000, check_every=20)
hess_post = shared(stencil_size(len(names)))
lap = Laplace.fit(hess_post.log_posterior, res.theta, names, device=hess_post.device)
print(f'MAP after {res.generations} generations: ' + ' '.join(f'{k}={v:.5g}' for k, v in zip(names, res.theta))
      + '; Laplace std ' + ' '.join(f'{s:.3g}' for s in lap.std))

# 3. DeviceDRAM: rows k and K + k of the posterior are chain k's two proposals, so the posterior has 2K rows, and its value
#    must not depend on the row: shared nuisance draws
K = 16
post = shared(2 * K)
theta0, cov0 = lap.dram_start()
sampler = DeviceDRAM(post.log_posterior, theta0, cov0=cov0, n_chains=K, seed=2, adapt_after=100, adapt_interval=50,
                     device=post.device)
torch.cuda.synchronize()
t0 = time.perf_counter()
trace = sampler.run(n_steps)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f'DeviceDRAM: {n_steps} steps x {K} chains in {1e3 * dt:.1f} ms ({1e6 * dt / max(1, n_steps):.1f} us per step, recording the '
      f'graph included), stage-1 acceptance {float(sampler.acceptance[0].mean()):.2f}, adaptations skipped: '
      f'{sampler.adaptation_failures}; posterior mean {trace[n_steps // 10:].reshape(-1, len(names)).mean(0).cpu().numpy()} '
      f'(theta* = {star})')

# 4. can the trace be trusted?
diag = diagnostics.summary(trace, names=names, burnin=0.1, acceptance=sampler.acceptance)
print(diagnostics.format_summary(diag))
