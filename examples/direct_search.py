#!/usr/bin/env python3
"""run_mle(optimizer='direct') on one MI355X: DIRECT over the whole prior box, then a Nelder-Mead polish from its result.

  1. the synthetic V_cc, thrust, ion velocity and ion current density data of calibration_start.py (a known theta*, 2 % noise);
  2. DIRECT as the reference calls it, `direct(obj_fun, bds, eps=1, maxiter=...)` (optimize.Direct): no start, no random
     numbers; a selection round asks for the 2 |I| points of every rectangle it divides at once, so they are the rows of one
     posterior launch, and a step is one graph replay.  DIRECT finds the basin, not the digits: its rectangles shrink by thirds;
  3. scipy's bounded Nelder-Mead (optimize.NelderMead) from that point.

    python examples/direct_search.py [max_iterations]          (default 100 iterations, the reference's setting)
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd.calibration import SystemPosterior                                         # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                                         # noqa: E402
from hallthrusterpem_amd.optimize import DIRECT_STATUS, Direct, NelderMead                          # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                               # noqa: E402

max_iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 100
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


# 2. DIRECT over the box of the priors, the reference's eps
di = Direct(None, names, eps=1.0, use_graph=True)
di.f = shared(di.rows).log_posterior
r, ms = timed(lambda: di.run(max_iterations=max_iterations))
print(f'DIRECT (eps 1, {di.rows} rows per launch): nit {r.nit}, nfev {r.nfev} in {r.launches} launches and {ms:.1f} ms, recording the '
      f'graph included ({DIRECT_STATUS[r.status]}); log posterior {r.history[0, 0]:.4f} at the centre of the box, {r.value:.4f} '
      f'at the best centre')

# 3. Nelder-Mead from there
nm = NelderMead(None, names, x0=r.theta, use_graph=True)
nm.f = shared(nm.rows).log_posterior
p, ms = timed(lambda: nm.run())
print(f'Nelder-Mead from it: nit {int(p.nit[0])}, nfev {int(p.nfev[0])} in {ms:.1f} ms '
      f'({"converged" if p.converged[0] else "not converged"}); log posterior {p.value[0]:.4f}')
print(f'  {"":>6} {"DIRECT":>12} {"Nelder-Mead":>12} {"theta*":>12}')
for k, m0, m1, s in zip(names, r.theta, p.theta[0], star):
    print(f'  {k:>6} {m0:12.6g} {m1:12.6g} {s:12.6g}')
