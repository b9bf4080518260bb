#!/usr/bin/env python3
"""Times of the calibration-start machinery on the synthetic System data of examples/calibration_start.py (needs the GPU):
one DE generation (pem_de_step_f64_dev + the posterior over the population) eager and as a graph replay, and the Hessian's
single posterior launch over 2 d^2 + 1 rows.  Host clock around work that ends in a device synchronise, after warm-up.

    python tools/calibration_start_probe.py [--reps 200]        -> one JSON line
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
from hallthrusterpem_amd.calibration import SystemPosterior                # noqa: E402
from hallthrusterpem_amd.optimize import DifferentialEvolution, stencil, stencil_size, theta_steps   # noqa: E402
from test_optimize import _synthetic                                       # noqa: E402


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) / reps * 1e6)
    return float(np.median(t)), float(min(t)), float(max(t))


ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=200)
args = ap.parse_args()
lik, names, star = _synthetic()
M = 50
mk = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False, shared_nuisance=True)  # noqa: E731
out = {'n_nuisance': M, 'n_cond': lik.n_cond, 'd': len(names)}
for use_graph in (False, True):
    de = DifferentialEvolution(None, names, seed=3, use_graph=use_graph)
    post = mk(de.P)
    de.f = post.log_posterior
    de._prepare(10 ** 6)
    step = de._graph.replay if use_graph else de._generation
    med, lo, hi = timed(step, args.reps)
    out['graph' if use_graph else 'eager'] = {'population': de.P, 'us_per_generation_median': med, 'min': lo, 'max': hi}
    out['samples_per_generation'] = de.P * M * lik.n_cond
    # the DE launch alone, eager (launch + enqueue cost of one generation's own kernel)
    if not use_graph:
        out['de_launch_only_eager'] = dict(zip(('median', 'min', 'max'), timed(lambda: de._launch(False), args.reps)))
hp = mk(stencil_size(len(names)))
pts = torch.as_tensor(stencil(star, theta_steps(star, names)), device='cuda')
med, lo, hi = timed(lambda: hp.log_posterior(pts), args.reps)
out['hessian_launch'] = {'rows': stencil_size(len(names)), 'us_median': med, 'min': lo, 'max': hi}
print(json.dumps(out))
