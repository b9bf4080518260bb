#!/usr/bin/env python3
"""Calibrate through the trained surrogate, as scripts/pem_v0/mcmc.py does (`SURR.predict` inside `spt100_log_likelihood`), next to
the same calibration through the true model, on one MI355X.

  1. fit(components=True): one surrogate per component over the calibrated, the operating and the nuisance inputs, the rest fixed;
  2. synthetic V_cc, thrust and ion current density data from the TRUE model at a known theta* (a_1 at its nominal value);
  3. the MAP by differential evolution through `SurrogatePosterior` (one `pem_chain_system_loglik_f64_dev` per evaluation) and
     through `SystemPosterior` (one `pem_coupled_system_loglik_f64_dev`), same data, box, seed and nuisance draws;
  4. both printed with the time per evaluation, and the surrogate's test errors beside them.

With the analytic thruster test double the model is far cheaper than its surrogate: the point of the surrogate route is a plugged-in
solver that costs seconds per sample.

    python examples/surrogate_calibration.py [refinement iterations] [--uion]          (default 60)

--uion: the thruster surrogate also carries the ion velocity profile (its SVD latents, `fit(targets=(..., 'u_ion'))`), the data gain
ion velocities at measured axial positions -- all four quantities of the reference's `System` calibration, one
`pem_chain_fields_loglik_f64_dev` per evaluation -- and the replay through the surrogate is timed with and without them.
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd.calibration import OPERATING, SurrogatePosterior, SystemPosterior   # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                                  # noqa: E402
from hallthrusterpem_amd.models.coupled import pem_v0_coupled                                # noqa: E402
from hallthrusterpem_amd.models.thruster import thruster_analytic                            # noqa: E402
from hallthrusterpem_amd.optimize import DifferentialEvolution                               # noqa: E402
from hallthrusterpem_amd.sampling import NORMAL, PEM_V0_PRIORS, Prior                        # noqa: E402
from hallthrusterpem_amd.system import PemV0System                                           # noqa: E402

UION = '--uion' in sys.argv[1:]
args = [v for v in sys.argv[1:] if v != '--uion']
n_iter = int(args[0]) if args else 60
NAMES = ('T_e', 'V_vac', 'c0', 'c3')
STAR = {'T_e': 3.0, 'V_vac': 30.0, 'c0': 0.35, 'c3': 0.6}
FIXED = {'Pstar': 5e-5, 'P_T': 5e-5, 'c1': 0.3, 'c2': 5.0, 'c4': 1e20, 'c5': 1e16, 'sigma_cex': 55e-20}
A_1 = 0.02                                                       # the one nuisance input: drawn from its prior by both posteriors

# 1. the component surrogates: theta, the operating inputs and a_1 varied, the rest fixed
system = PemV0System(seed=0)
xt = system.sample_inputs(2000, normalize=False)
xt.update({k: np.full(2000, v) for k, v in FIXED.items()})
yt = system.predict(xt, use_model='best', normalized_inputs=False)
if UION:
    yt['u_ion'] = thruster_analytic({'V_a': xt['V_a'], 'V_cc': yt['V_cc'], 'mdot_a': xt['mdot_a'], 'a_1': xt['a_1']}, num_cells=200)['u_ion']
t0 = time.perf_counter()
hist = system.fit(targets=['V_cc', 'div_angle', 'T_c', 'j_ion'] + (['u_ion'] if UION else []), fixed=FIXED, max_iter=n_iter, max_tol=0.0,
                  num_refine=1000, test_set=(xt, yt), components=True)
surr = system.surrogate
print(f'fit(components=True): {len(hist)} iterations in {time.perf_counter() - t0:.1f} s, evaluations per component {surr.model_evals}, '
      f'j_ion rank {surr.compression.rank}')
print('  test errors (relative L2 over 2000 points; j_ion in log10): ' + ' '.join(f'{k}={v:.2e}' for k, v in hist[-1]['test_error'].items()))

# 2. data from the true model at theta*
rng = np.random.default_rng(0)
op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
alpha = np.linspace(-1.5, 1.5, 25)
grid = np.linspace(0, np.pi / 2, 91)


def model(o):
    x = {k: np.full(o.shape[0], v) for k, v in {**FIXED, **STAR, 'a_1': A_1}.items()}
    x.update({k: o[:, j] for j, k in enumerate(OPERATING)})
    out = pem_v0_coupled(x)
    th = thruster_analytic({'V_a': x['V_a'], 'V_cc': out['V_cc'], 'mdot_a': x['mdot_a'], 'a_1': x['a_1']}, num_cells=200 if UION else None)
    return out, th


ops = {'V_cc': op(4), 'T': op(3), 'jion': op(5)}
out, _ = model(ops['V_cc'])
data = {'V_cc': {'x': ops['V_cc'], 'y': np.asarray(out['V_cc']), 'var_y': np.full(4, 0.3 ** 2)}}
_, th = model(ops['T'])
data['T'] = {'x': ops['T'], 'y': np.asarray(th['T']), 'var_y': (0.02 * np.asarray(th['T'])) ** 2}
out, _ = model(ops['jion'])
j = np.stack([np.interp(np.abs(alpha), grid, np.asarray(out['j_ion'])[e]) for e in range(5)])
data['jion'] = {'x': ops['jion'], 'y': j, 'var_y': (0.05 * j + 1e-3) ** 2, 'loc': np.stack([np.ones(alpha.size), alpha], 1)}
lik_few = SystemLikelihood(data)
if UION:                                                         # ion velocities at 20 axial positions of 4 more conditions
    ops['uion'] = op(4)
    zloc = np.linspace(0.002, 0.078, 20)
    _, th = model(ops['uion'])
    u = np.stack([np.interp(zloc, np.asarray(th['u_ion_coords']), np.asarray(th['u_ion'])[e]) for e in range(4)])
    data['uion'] = {'x': ops['uion'], 'y': u, 'var_y': (0.05 * u + 100.0) ** 2, 'loc': zloc}
lik = SystemLikelihood(data)

# 3. the MAP through the surrogate and through the model: the model's posterior pins what the surrogate holds fixed
M = 50
pinned = dict(PEM_V0_PRIORS)
pinned.update({k: Prior(NORMAL, v, 1e-9 * abs(v), 'pinned') for k, v in FIXED.items()})
routes = {
    'surrogate': lambda K: SurrogatePosterior(NAMES, lik, surr, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False, shared_nuisance=True),
    'model': lambda K: SystemPosterior(NAMES, lik, n_chains=K, n_nuisance=M, priors=pinned, seed=1, fresh_nuisance=False, shared_nuisance=True),
}
res = {}
for name, make in routes.items():
    de = DifferentialEvolution(None, NAMES, seed=3, tol=1e-4, use_graph=True)
    post = make(de.P)
    de.f = post.log_posterior
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = de.run(400, check_every=20)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res[name] = r
    print(f'MAP through the {name}: {r.generations} generations of {de.P} rows x {M} draws x {lik.n_cond} conditions (converged: '
          f'{r.converged}) in {1e3 * dt:.1f} ms = {1e6 * dt / (r.generations + 1):.0f} us per evaluation, the recording of the graph '
          f'included; log posterior {r.value:.3f}')

# 4. side by side
print(f'  {"":>6} {"surrogate":>12} {"model":>12} {"theta*":>12}')
for i, k in enumerate(NAMES):
    print(f'  {k:>6} {res["surrogate"].theta[i]:12.5g} {res["model"].theta[i]:12.5g} {STAR[k]:12.5g}')
# one graph replay of each posterior at the population's size, interleaved
if UION:                                                         # the same surrogate on the data without the ion velocities
    routes['surrogate, no u_ion data'] = lambda K: SurrogatePosterior(NAMES, lik_few, surr, n_chains=K, n_nuisance=M, seed=1,
                                                                      fresh_nuisance=False, shared_nuisance=True)
posts = {name: make(res['model'].theta.size * 15) for name, make in routes.items()}
replays = {name: p.capture() for name, p in posts.items()}
theta = torch.from_numpy(np.broadcast_to(res['model'].theta, (posts['model'].K, len(NAMES))).copy()).to(posts['model'].device)
us = {name: [] for name in replays}
for _ in range(3 + 5):                                           # three warm-up rounds
    for name, rp in replays.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            rp(theta)
        e1.record()
        e1.synchronize()
        us[name].append(1e3 * e0.elapsed_time(e1) / 20)
for name, v in us.items():
    print(f'log_posterior replay through the {name} ({posts[name].n} samples): {np.median(v[3:]):.1f} us [{min(v[3:]):.1f}, {max(v[3:]):.1f}]')
# the two posteriors over 256 prior draws
K = 256
ps, pm = routes['surrogate'](K), routes['model'](K)
theta = torch.from_numpy(np.stack([rng.uniform(PEM_V0_PRIORS[k].a, PEM_V0_PRIORS[k].b, K) for k in NAMES], 1)).to(ps.device)
d = (ps.log_posterior(theta) - pm.log_posterior(theta)).abs()
print(f'max |log posterior (surrogate) - log posterior (model)| over {K} prior draws: {float(d.max()):.3g} (median {float(d.median()):.3g})')
