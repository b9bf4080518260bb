#!/usr/bin/env python3
"""Which measurements constrain the inputs, and which operating condition is worth measuring next?  The expected information gain
of groups of measurements of the `System` table (information.InformationGain: nested Monte Carlo, one fused all-pairs launch per
estimate) on one MI355X:

  1. synthetic V_cc, thrust, ion velocity and ion current density data, made by the model at a known theta* plus 2 % noise;
  2. the gain expected from the data before any is used (draws from the prior), per quantity and per operating condition;
  3. a short DRAM run of the `System` posterior, and the gain that is left relative to it.

The gain is about the calibrated and the nuisance inputs jointly, in nats: every draw is one input vector shared by all operating
conditions.  A group whose inner sums are single terms (median ess near 1) is flagged: with the separate inner set used here its
number is biased upward and unreliable -- it wants more draws or narrower groups (with reuse=True it would be a lower bound, at
most log M).

    python examples/information_gain.py [n_steps] [n_draws]          (default 300 DRAM steps of 16 chains, 4096 x 4096 draws)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd.calibration import DRAM, SystemPosterior      # noqa: E402
from hallthrusterpem_amd.information import InformationGain            # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood            # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                  # noqa: E402

n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
n_draws = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
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
ig = InformationGain(Predictive(lik, names, seed=3))


def report(title, samples):
    for by in ('qoi', 'condition'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ig.run(samples=samples, n_outer=n_draws, n_inner=n_draws, by=by)
        torch.cuda.synchronize()
        print(f'\n{title}, by {by}: {res["n_outer"]} x {res["n_inner"]} draws ({res["dropped"]} dropped), '
              f'{1e3 * (time.perf_counter() - t0):.1f} ms')
        print(ig.table(res))


# 2. before any data is used
report('expected gain from the prior', None)

# 3. a short DRAM run from the middle of the priors, and what is left to gain
K = 16
post = SystemPosterior(names, lik, n_chains=K, n_nuisance=50, seed=1)
sampler = DRAM(post.log_posterior, np.array([2.5, 25.0, 4e-5, 0.4, 0.9]), cov0=np.array([0.1, 4.0, 1e-11, 1e-3, 4e-3]) / 10,
               n_chains=K, seed=2, adapt_after=100, adapt_interval=50, device=post.device)
trace = sampler.run(n_steps)
print(f'\nDRAM: {n_steps} steps x {K} chains, posterior mean {trace[n_steps // 10:].reshape(-1, len(names)).mean(0).cpu().numpy()} '
      f'(theta* = {star})')
report('expected gain relative to the posterior', trace)
