#!/usr/bin/env python3
"""The marginal posteriors the calibration publishes, on one MI355X: journal_plots of scripts/pem_v0/mcmc.py without a host copy.

  1. synthetic V_cc, thrust, ion velocity and ion current density data at a known theta* plus 2 % noise, and the posterior
     over them, set up as examples/calibration_start.py does;
  2. a short DRAM run started around theta*;
  3. the chains' diagnostics (diagnostics.summary / format_summary);
  4. marginals.corner for the three parameter groups of journal_plots (cathode / thruster / plume): pair counts with 15 bins,
     cells under int(0.0015 * n_draws) draws blanked, a Gaussian KDE of every parameter, 50 % / 90 % credible levels, the pooled
     mean and covariance; the arrays are saved to posterior_marginals.npz;
  5. the three figures, only if matplotlib imports (it is not a dependency).

    python examples/posterior_marginals.py [--hex] [n_steps] [out.npz]          (default 600 DRAM steps of 16 chains)

--hex: the pair panels as journal_plots draws them, hexagonal bins (corner(plot2d='hex'), matplotlib's hexbin rule at gridsize =
bins); for the first pair of every group the number of hexagons at or above cmin and its 50 % / 90 % levels are printed, and the
tables are saved with the rest.
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import diagnostics, marginals                                 # noqa: E402
from hallthrusterpem_amd.calibration import DRAM, SystemPosterior                      # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                            # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                  # noqa: E402

hexagons = '--hex' in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != '--hex']
n_steps = int(argv[0]) if len(argv) > 0 else 600
out = Path(argv[1]) if len(argv) > 1 else Path('posterior_marginals.npz')
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
# journal_plots' three figures, with the calibrated parameters each one holds here
groups = {'cathode': ['V_vac'], 'thruster': [], 'plume': ['c0', 'c3']}
groups['all'] = list(names)

# 1. data at theta* with 2 % noise (examples/calibration_start.py, step 1)
truth = Predictive(SystemLikelihood(data), names, seed=1).run(samples=star[None], n_draws=1)
for q, d in data.items():
    t = truth[q]['pred'][0].cpu().numpy()
    d['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
    d['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
K = 16
post = SystemPosterior(names, SystemLikelihood(data), n_chains=K, n_nuisance=50, seed=1, fresh_nuisance=False, shared_nuisance=True)

# 2. DRAM around theta*
cov0 = np.diag((0.01 * np.abs(star)) ** 2)
theta0 = star + rng.multivariate_normal(np.zeros(len(names)), cov0, size=K)
t0 = time.perf_counter()
sampler = DRAM(post.log_posterior, theta0, cov0=cov0, n_chains=K, seed=2, adapt_after=100, adapt_interval=50, device=post.device)
trace = sampler.run(n_steps)
torch.cuda.synchronize()
print(f'DRAM: {n_steps} steps x {K} chains in {time.perf_counter() - t0:.1f} s')

# 3. diagnostics
print(diagnostics.format_summary(diagnostics.summary(trace, names=names, burnin=0.1, acceptance=sampler.acceptance)))

# 4. the marginals, group by group
n_draws = (n_steps - int(0.1 * n_steps)) * K
saved = {}
for g, sel in groups.items():
    if not sel:
        print(f'{g}: none of its parameters is calibrated here')
        continue
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cmin = int(0.0015 * n_draws)
    c = marginals.corner(trace, names=names, select=sel, burnin=0.1, bins=15, cmin=cmin, points=256,
                         plot2d='hex' if hexagons and len(sel) > 1 else 'hist')
    torch.cuda.synchronize()
    print(f'{g}: corner() of {len(sel)} parameters over {c["n_draws"]} draws in {1e3 * (time.perf_counter() - t0):.1f} ms')
    dens, grid = c['density'].cpu().numpy(), c['grid'].cpu().numpy()
    for i, k in enumerate(c['names']):
        print(f'  {k:>6}: mean {float(c["mean"][i]):.5g}, KDE mode {grid[i, dens[i].argmax()]:.5g}, bandwidth {float(c["bandwidth"][i]):.3g}, '
              f'theta* {star[names.index(k)]:.5g}')
    for i in range(len(sel)):
        for j in range(i + 1, len(sel)):
            print(f'  ({c["names"][i]}, {c["names"][j]}): correlation {float(c["corr"][i, j]):+.3f}, 50 % / 90 % levels {c["levels"][i, j].tolist()}, '
                  f'{int(c["mask"][i, j].sum())} of {15 * 15} cells blanked')
    hx = c.pop('hex', None)
    if hx is not None:
        i, j = hx['pairs'][0].tolist()
        print(f'  ({c["names"][i]}, {c["names"][j]}) in hexagons, gridsize ({hx["nx"]}, {hx["ny"]}): {int((~hx["mask"][0]).sum())} of '
              f'{hx["counts"].shape[1]} hold at least cmin = {cmin} draws, 50 % / 90 % levels {hx["levels"][0].tolist()}')
        for k, v in hx.items():
            if k not in ('nx', 'ny', 'n_draws'):
                saved[f'{g}/hex/{k}'] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    for k, v in c.items():
        if k not in ('names', 'mass', 'n_draws'):
            saved[f'{g}/{k}'] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    saved[f'{g}/names'] = np.array(c['names'])
np.savez(out, **saved)
print(f'arrays saved to {out}')

# 5. the figures, if matplotlib is there
try:
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
except ImportError:
    print('matplotlib is not installed: no figure drawn')
    sys.exit(0)
for g, sel in groups.items():
    if not sel:
        continue
    d = len(sel)
    fig, ax = plt.subplots(d, d, figsize=(2.2 * d, 2.2 * d), squeeze=False)
    e, h2, mask = (saved[f'{g}/{k}'] for k in ('edges', 'hist2d', 'mask'))
    for i in range(d):
        for j in range(d):
            a = ax[i, j]
            if j > i:
                a.axis('off')
            elif i == j:
                a.plot(saved[f'{g}/grid'][i], saved[f'{g}/density'][i])
            else:                                             # row i, column j < i: x = parameter j, y = parameter i
                a.pcolormesh(e[j], e[i], np.ma.masked_array(h2[j, i].T, mask[j, i].T))
                a.contour(0.5 * (e[j][1:] + e[j][:-1]), 0.5 * (e[i][1:] + e[i][:-1]), h2[j, i].T,
                          levels=sorted(set(saved[f'{g}/levels'][j, i].tolist())), colors='w', linewidths=0.8)
            if i == d - 1:
                a.set_xlabel(sel[j])
    fig.savefig(out.with_name(f'mcmc-{g}.png'), bbox_inches='tight')
    plt.close(fig)
print('figures saved beside the arrays')
