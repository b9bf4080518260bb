#!/usr/bin/env python3
"""Calibrating against a probe sweep taken at several distances from the thruster, on one MI355X.

The reference's data schema gives ion current density the coordinates (r, theta) (hallmd/data.py); here the j_ion dataset holds
three radii, and every evaluation of the posterior is still ONE model evaluation per sample
(`pem_coupled_system_loglik_radii_f64_dev`: the 91-point shape of the profile does not depend on the radius).

  1. synthetic current densities at r = 0.55, 1.0 and 1.37 m from a known theta* = (c0, c3) plus 2 % noise;
  2. the maximum a posteriori point by differential evolution through `SystemPosterior`, unchanged;
  3. `Predictive` at the MAP: the 5 / 50 / 95 % bands of the model at every measured (r, alpha), printed per radius.

    python examples/multi_radius_calibration.py [n_draws]          (default 400 predictive draws)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd.calibration import SystemPosterior            # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood            # noqa: E402
from hallthrusterpem_amd.optimize import DifferentialEvolution         # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                  # noqa: E402

n_draws = int(sys.argv[1]) if len(sys.argv) > 1 else 400
radii = (0.55, 1.0, 1.37)
rng = np.random.default_rng(0)
ne, na = 3, 9
alpha = np.linspace(-1.5, 1.5, na)
loc = np.stack([np.repeat(radii, na), np.tile(alpha, len(radii))], 1)          # (Na, 2) rows (r, alpha), any order
x = np.stack([10.0 ** rng.uniform(-6, -4.5, ne), rng.uniform(250, 350, ne), rng.uniform(4e-6, 6e-6, ne)], 1)
data = {'jion': {'x': x, 'y': np.zeros((ne, loc.shape[0])), 'var_y': np.ones((ne, loc.shape[0])), 'loc': loc}}
names = ('c0', 'c3')
star = np.array([0.5, 0.8])

# 1. data from the model at theta* with 2 % noise; every other input at the first nuisance draw of the posterior's own design
truth = Predictive(SystemLikelihood(data, sweep_radii=radii), names, seed=1).run(samples=star[None], n_draws=1)
t = truth['jion']['pred'][0].cpu().numpy()
data['jion']['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
data['jion']['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
lik = SystemLikelihood(data, sweep_radii=radii)
print(f'{lik.n_cond} conditions x {loc.shape[0]} current densities at radii {lik.sweep_radii} m: {lik.n_rec} records')

# 2. MAP by differential evolution: the population is the rows of one posterior launch with shared nuisance draws
de = DifferentialEvolution(None, names, seed=3, tol=1e-4, use_graph=True)
post = SystemPosterior(names, lik, n_chains=de.P, n_nuisance=20, seed=1, fresh_nuisance=False, shared_nuisance=True)
de.f = post.log_posterior
torch.cuda.synchronize()
t0 = time.perf_counter()
res = de.run(600, check_every=20)
torch.cuda.synchronize()
print(f'MAP: population {de.P}, {res.generations} generations (converged: {res.converged}) in '
      f'{1e3 * (time.perf_counter() - t0):.1f} ms; log posterior {res.value:.3f}')
for k, m, s in zip(names, res.theta, star):
    print(f'  {k:>4} MAP {m:10.5g}   theta* {s:10.5g}')

# 3. predictive bands at the MAP, per radius (first condition)
pp = Predictive(lik, names, seed=5).run(samples=res.theta[None], n_draws=n_draws)
bands, y = pp['jion']['bands'].cpu().numpy(), data['jion']['y']
print(f'Predictive: {n_draws} draws, mean relative L2 error {float(torch.as_tensor(pp["jion"]["rel_l2"]).mean()):.3f}')
for r, radius in enumerate(radii):
    cols = slice(r * na, (r + 1) * na)
    print(f'  r = {radius} m   alpha [rad]      5 %      50 %      95 %      data')
    for a_, lo, mid, hi, d in zip(alpha, bands[0, 0, cols], bands[1, 0, cols], bands[2, 0, cols], y[0, cols]):
        print(f'               {a_:+10.3f} {lo:9.4g} {mid:9.4g} {hi:9.4g} {d:9.4g}')
