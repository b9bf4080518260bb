#!/usr/bin/env python3
"""run_mle(optimizer='powell') on one MI355X: differential evolution stopped early, then bounded Powell from its best members.

  1. the synthetic V_cc, thrust, ion velocity and ion current density data of calibration_start.py (a known theta*, 2 % noise);
  2. differential evolution with a loose tol (optimize.DifferentialEvolution): it stops when the population's values agree to
     1 %, a few units of log posterior short of the maximum;
  3. scipy's bounded Powell (optimize.Powell) from the best d + 1 members of that population: a line search wants one value at
     a time, so one launch advances every search by one value, the searches' points are the rows of one posterior launch, and a
     step is one graph replay.  Powell's own value can go down (a line search never evaluates its base point), so the best
     point a search has had a value for is reported beside scipy's result.

    python examples/powell_search.py [max_iterations]          (default 20 iterations per search)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd.calibration import SystemPosterior                                         # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                                         # noqa: E402
from hallthrusterpem_amd.optimize import POWELL_STATUS, DifferentialEvolution, Powell               # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                               # noqa: E402

max_iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 20
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

# 3. Powell from the best d + 1 members (after `run`, de.theta is the population and de.pop_f its values), all in the same launches
members = torch.argsort(de.pop_f, descending=True, stable=True)[:d + 1]
po = Powell(None, names, x0=de.theta[members].cpu().numpy(), use_graph=True)
po.f = shared(po.rows).log_posterior
r, ms = timed(lambda: po.run(max_iterations=max_iterations))
print(f'Powell from its best {d + 1} members ({po.rows} rows per launch, at most {max_iterations} iterations) in {ms:.1f} ms, '
      f'recording the graph included; best: start {r.best}')
for s in range(po.rows):
    print(f'  start {s}: nit {int(r.nit[s]):3d} nfev {int(r.nfev[s]):5d} ({POWELL_STATUS[int(r.status[s])]}); log posterior '
          f'{r.history[0, s]:.4f} at x0, {r.value[s]:.4f} at scipy\'s x, {r.best_value[s]:.4f} at the best point')
print(f'  {"":>6} {"DE":>12} {"Powell":>12} {"theta*":>12}')
for k, m0, m1, s in zip(names, res.theta, r.best_theta[r.best], star):
    print(f'  {k:>6} {m0:12.6g} {m1:12.6g} {s:12.6g}')
c = {k: int(v.sum()) for k, v in r.counters.items()}
print(f'  {c["lines"]} line searches: {c["golden"]} golden and {c["parabolic"]} parabolic steps, {c["extra"]} extra line searches, '
      f'{c["replaced"]} directions replaced, {c["worse"]} line searches that returned a worse value than they started from')
