#!/usr/bin/env python3
"""Which measurement informs which calibrated parameter?  `examples/information_gain.py` ranks the measurements by the gain about
the calibrated AND the nuisance inputs jointly; the calibration itself works with the likelihood with the nuisance inputs averaged
out.  This example splits the gain (information.InformationGain with `about=`: a third nest, one conditional launch per chunk of
outer draws) on one MI355X:

  1. synthetic V_cc, thrust, ion velocity and ion current density data, made by the model at a known theta* plus 2 % noise;
  2. the gain about the calibrated parameters together, per quantity: `eig_about` of the total, the rest being what the data
     say about the nuisance inputs once theta is known;
  3. the gain about every parameter alone, per quantity (`by_parameter`: one outer and one inner set for all of them).

All from the prior, in nats.  `ess cond` is the number of vectors that carry a conditional sum: near 1, n_conditional is too small.

    python examples/parameter_information.py [n_draws] [n_conditional]          (default 2048 x 2048 draws, 128 per outer draw)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd.information import InformationGain            # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood            # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                  # noqa: E402

n_draws = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
n_conditional = int(sys.argv[2]) if len(sys.argv) > 2 else 128
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
ig = InformationGain(Predictive(SystemLikelihood(data), names, seed=3))


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


# 2. the calibrated parameters together
res, ms = timed(lambda: ig.run(n_outer=n_draws, n_inner=n_draws, by='qoi', about=names, n_conditional=n_conditional))
print(f'\ngain about the calibrated parameters together, by qoi: {res["n_outer"]} x {res["n_inner"]} draws, {n_conditional} per outer draw '
      f'({res["dropped"]} + {res["dropped_conditional"]} dropped, fewest used rows {res["used_min"]}), {ms:.1f} ms')
print(ig.table(res))

# 3. every parameter alone
res, ms = timed(lambda: ig.by_parameter(n_outer=n_draws, n_inner=n_draws, by='qoi', n_conditional=n_conditional))
print(f'\nwhich measurement informs which parameter, by qoi: {len(names)} conditional nests on one outer and one inner set, {ms:.1f} ms')
print(res['table'])
