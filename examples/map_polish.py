#!/usr/bin/env python3
"""A MAP to the optimiser's tolerance: differential evolution stopped early, then Nelder-Mead, then Laplace, on one MI355X.

  1. the synthetic V_cc, thrust, ion velocity and ion current density data of calibration_start.py (a known theta*, 2 % noise);
  2. differential evolution with a loose tol (optimize.DifferentialEvolution): it stops when the population's values agree to
     1 %, a few units of log posterior short of the maximum;
  3. bounded, adaptive Nelder-Mead (optimize.NelderMead, run_mle's default optimizer) from the best d + 1 members of that
     population, and from a few Latin-hypercube starts beside it: the d + 4 points an iteration can ask for are the rows of
     one posterior launch, S simplices share it, an iteration is one graph replay;
  4. the Laplace approximation at the better of the two (optimize.Laplace).

    python examples/map_polish.py [n_starts]          (default 4 Latin-hypercube starts)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd.calibration import SystemPosterior                                         # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                                         # noqa: E402
from hallthrusterpem_amd.optimize import DifferentialEvolution, Laplace, NelderMead, stencil_size   # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                               # noqa: E402

n_starts = int(sys.argv[1]) if len(sys.argv) > 1 else 4
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
d = len(names)

# 1. data from the model at theta* with 2 % noise, as calibration_start.py
truth = Predictive(SystemLikelihood(data), names, seed=1).run(samples=star[None], n_draws=1)
for q, dd in data.items():
    t = truth[q]['pred'][0].cpu().numpy()
    dd['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
    dd['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
lik = SystemLikelihood(data)
M = 50
shared = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)


def timed(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


# 2. differential evolution, stopped at scipy's default tol
de = DifferentialEvolution(None, names, seed=3, tol=1e-2, use_graph=True)
de.f = shared(de.P).log_posterior
res, ms = timed(lambda: de.run(1000, check_every=5))
print(f'MAP by differential evolution (tol 1e-2): population {de.P}, {res.generations} generations in {ms:.1f} ms; '
      f'log posterior {res.value:.4f}')

# 3. Nelder-Mead from the best d + 1 members (after `run`, de.theta is the population and de.pop_f its values) ...
members = torch.argsort(de.pop_f, descending=True, stable=True)[:d + 1]
nm = NelderMead(None, names, initial_simplex=de.theta[members].cpu().numpy(), use_graph=True)
nm.f = shared(nm.rows).log_posterior
polish, ms = timed(nm.run)
print(f'Nelder-Mead from its best {d + 1} members: nit {int(polish.nit[0])}, nfev {int(polish.nfev[0])} (converged: '
      f'{bool(polish.converged[0])}) in {ms:.1f} ms, recording the graph included; log posterior {polish.value[0]:.4f}')
# ... and from Latin-hypercube starts, all in the same launches: a start may stall on a face of the box, `best` picks the winner
lhs = NelderMead(None, names, n_starts=n_starts, seed=3, use_graph=True)
lhs.f = shared(lhs.rows).log_posterior
multi, ms = timed(lhs.run)
print(f'Nelder-Mead from {n_starts} Latin-hypercube starts ({lhs.rows} rows per launch) in {ms:.1f} ms, graph included; log posterior '
      + ' '.join(f'{v:.4f}' for v in multi.value) + f'; best: start {multi.best}')
theta = polish.theta[0] if polish.value[0] >= multi.value[multi.best] else multi.theta[multi.best]
print(f'  {"":>6} {"DE":>12} {"Nelder-Mead":>12} {"theta*":>12}')
for k, m0, m1, s in zip(names, res.theta, theta, star):
    print(f'  {k:>6} {m0:12.6g} {m1:12.6g} {s:12.6g}')

# 4. Laplace at the polished MAP
hess_post = shared(stencil_size(d))
lap = Laplace.fit(hess_post.log_posterior, theta, names, device=hess_post.device)
print(f'Laplace at the Nelder-Mead MAP: nearest-PD fall-back: {lap.nearest_pd}')
print('  standard deviations ' + ' '.join(f'{k}={s:.3g}' for k, s in zip(names, lap.std)))
print('  (MAP - theta*) / std ' + ' '.join(f'{z:+.2f}' for z in (theta - star) / lap.std))
