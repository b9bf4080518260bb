#!/usr/bin/env python3
"""Calibrating when the stated measurement noise is wrong: a noise scale per measured quantity, sampled with theta, on one MI355X.

  1. synthetic V_cc, thrust, ion velocity and ion current density data from the model at theta* (ensemble_sampler.py, step 1): every
     dataset states a std of 2 % of its values, and the noise is drawn at that std -- except the ion current density, whose noise
     is drawn at TWICE its stated std;
  2. samplers.DeviceEnsemble on `SystemPosterior` as it always was: the stated std taken as exact;
  3. the same with noise_scales=('jion',): theta gains the column 'noise_jion', a multiplier of the stated j_ion std with a
     log-uniform prior on [0.1, 10], and the marginalisation carries its normaliser -n_jion log s;
  4. diagnostics.format_summary of both traces: with the scale the plume parameters' intervals widen to what the misfit justifies
     and 'noise_jion' settles near 2; then, at the posterior mean, which dataset carries the likelihood (chi) and how many of the
     nuisance draws stand behind the value (ess).

    python examples/noise_scale_calibration.py [n_steps]          (default: 2000 steps of 2 ensembles x 16 walkers)
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import diagnostics                                            # noqa: E402
from hallthrusterpem_amd.calibration import DeviceEnsemble, SystemPosterior            # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                            # noqa: E402
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
TRUE_SCALE = {'jion': 2.0}

# 1. data from the model at theta*: stated std 2 %, the j_ion noise drawn at twice that
truth = Predictive(SystemLikelihood(data), names, seed=1).run(samples=star[None], n_draws=1)
for q, d in data.items():
    t = truth[q]['pred'][0].cpu().numpy()
    d['y'] = t * (1 + TRUE_SCALE.get(q, 1.0) * 0.02 * rng.standard_normal(t.shape))
    d['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
lik = SystemLikelihood(data)
M, E, K = 50, 2, 16


def sample(noise_scales):
    """the posterior with E K / 2 rows and shared nuisance draws, the sampler on it, and the summary of the ensemble means"""
    post = SystemPosterior(names, lik, n_chains=E * K // 2, n_nuisance=M, seed=1, fresh_nuisance=False, shared_nuisance=True,
                           noise_scales=noise_scales)
    centre = np.concatenate([star, np.ones(len(post.names) - len(names))])
    theta0 = DeviceEnsemble.ball(centre, 0.01 * np.abs(centre), K, n_ensembles=E, seed=4)
    sampler = DeviceEnsemble(post.log_posterior, theta0, seed=2, de_fraction=0.2, device=post.device)
    trace = sampler.run(n_steps)
    torch.cuda.synchronize()
    print(f'\nnoise_scales={noise_scales}: theta = {post.names}, acceptance {float(sampler.acceptance.mean()):.2f}')
    print(diagnostics.format_summary(diagnostics.summary(trace.mean(dim=2), names=post.names, burnin=0.1)))
    return post, trace


# 2. the stated noise held exact; 3. a scale on the j_ion std
_, fixed = sample(None)
post, free = sample(('jion',))

# 4. what the scale did to the plume parameters, and what stands behind the likelihood at the posterior mean
keep = lambda t: t[n_steps // 10:].reshape(-1, t.shape[-1])                              # noqa: E731
sd_fixed, sd_free = keep(fixed).std(dim=0).cpu().numpy(), keep(free).std(dim=0).cpu().numpy()
for i, k in enumerate(names):
    print(f'  {k:>6}: posterior std {sd_fixed[i]:.3g} with the stated noise, {sd_free[i]:.3g} with noise_jion free (theta* {star[i]:.5g})')
mean = keep(free).mean(dim=0)
print(f'  noise_jion: mean {float(mean[-1]):.3f} (drawn with {TRUE_SCALE["jion"]})')
_, ess, chi = post.log_likelihood(mean.expand(post.K, -1).contiguous(), diagnostics=True)
print(f'  at the posterior mean: {float(ess[0]):.1f} of the {M} nuisance draws carry the likelihood; weighted sums of -0.5 z^2 per dataset: '
      + ', '.join(f'{q} {float(chi[0, g]):.1f}' for g, q in enumerate(post.noise_groups)) + f', I_D {float(chi[0, -1]):.1f}')
n_jion = float(post.noise_counts[post.noise_groups.index('jion')])
print(f'  the scale that makes the mean squared j_ion residual 1 there: sqrt(-2 chi_jion / n_jion) = '
      f'{(-2 * float(chi[0, -2]) / n_jion) ** 0.5:.3f}')
