#!/usr/bin/env python3
"""Time per iteration of optimize.NelderMead, and scipy's own Nelder-Mead on the same posterior (needs the GPU).

Workload: the posterior of examples/calibration_start.py (synthetic System data, 3 calibrated inputs, M = 50 shared nuisance
draws), S = 8 Latin-hypercube starts -> 8 x (3 + 4) = 56 rows per launch.

  1. one iteration (pem_nm_step_f64_dev, the posterior's launches, the copy of the values), eager and as a graph replay: host
     clock over `--iterations` iterations ending in a device synchronise, warm, `--repeats` times, alternating;
  2. the mean of nm_step_kernel per dispatch, from a `rocprofv3 --kernel-trace --stats` run of its own (this script started
     again as the profiled child, before this process opens the GPU);
  3. scipy.optimize.minimize(method='Nelder-Mead', bounds=..., options={'adaptive': True}) on the host, the way the reference
     runs it: the same posterior with n_chains = 1, one point per call, from the same x0 as start 0, over the same search
     coordinates; alternated with a one-simplex NelderMead from that x0.  Time per function value and time to convergence;
  4. one generation of DifferentialEvolution (population 45) from the same run, as context.

    python tools/nelder_mead_probe.py [--iterations 200] [--repeats 3] [--out profiles/nelder_mead_r01.txt]
"""
import argparse
import csv
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
NAMES = ('V_vac', 'c0', 'c3')
S, M = 8, 50


def posterior_factory():
    """examples/calibration_start.py's synthetic data; returns K -> SystemPosterior with shared nuisance draws"""
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive
    rng = np.random.default_rng(0)
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
    na = 25
    data = {'V_cc': {'x': op(4), 'y': np.zeros(4), 'var_y': np.ones(4)},
            'T': {'x': op(3), 'y': np.zeros(3), 'var_y': np.ones(3)},
            'uion': {'x': op(2), 'y': np.zeros((2, 6)), 'var_y': np.ones((2, 6)), 'loc': np.linspace(0.005, 0.075, 6)},
            'jion': {'x': op(5), 'y': np.zeros((5, na)), 'var_y': np.ones((5, na)),
                     'loc': np.stack([np.ones(na), np.linspace(-1.5, 1.5, na)], 1)}}
    star = np.array([30.0, 0.5, 0.8])
    truth = Predictive(SystemLikelihood(data), NAMES, seed=1).run(samples=star[None], n_draws=1)
    for q, dd in data.items():
        t = truth[q]['pred'][0].cpu().numpy()
        dd['y'] = t * (1 + 0.02 * rng.standard_normal(t.shape))
        dd['var_y'] = (0.02 * np.abs(t)) ** 2 + 1e-30
    lik = SystemLikelihood(data)
    return lambda K: SystemPosterior(NAMES, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False, shared_nuisance=True)


def searcher(mk, **kw):
    from hallthrusterpem_amd.optimize import NelderMead
    nm = NelderMead(None, NAMES, seed=3, **kw)
    nm.f = mk(nm.rows).log_posterior
    return nm


def child(iterations):
    """the profiled run: eager iterations of the 8-start search (every dispatch of nm_step_kernel is one iteration)"""
    import torch
    nm = searcher(posterior_factory(), n_starts=S)
    nm.reset()
    for _ in range(iterations):
        nm._iteration()
    torch.cuda.synchronize()


def profile_kernel(iterations):
    """(calls, mean us) of nm_step_kernel from rocprofv3's kernel statistics, or a note why not"""
    exe = shutil.which('rocprofv3')
    if exe is None:
        return None, 'rocprofv3 not found'
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [exe, '--kernel-trace', '--stats', '-f', 'csv', '-d', tmp, '-o', 'nm', '--', sys.executable, str(Path(__file__).resolve()),
               '--child', '--iterations', str(iterations)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            return None, f'rocprofv3 exited with {out.returncode}: {out.stderr[-300:]}'
        for f in Path(tmp).rglob('*kernel_stats.csv'):
            for r in csv.DictReader(open(f)):
                if 'nm_step_kernel' in r['Name']:
                    return (int(r['Calls']), float(r['AverageNs']) / 1e3), None
    return None, 'nm_step_kernel not in the kernel statistics'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'nelder_mead_r01.txt'))
    a = ap.parse_args()
    if a.child:
        return child(a.iterations)
    prof, why = profile_kernel(a.iterations)              # before this process opens the GPU

    import torch
    from scipy.optimize import minimize
    from hallthrusterpem_amd.optimize import DifferentialEvolution, quantile, search_bounds
    from hallthrusterpem_amd.sampling import LOGUNIFORM, PEM_V0_PRIORS, UNIFORM
    mk = posterior_factory()
    sync = torch.cuda.synchronize

    def clock(body, n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            body()
        sync()
        return (time.perf_counter() - t0) / n * 1e6

    # 1. one iteration, eager and replayed
    eager, graph = searcher(mk, n_starts=S), searcher(mk, n_starts=S, use_graph=True)
    graph._prepare(1)                                                      # records the graph
    eager.reset()
    forms = {'eager': eager._iteration, 'graph replay': graph._graph.replay}
    for body in forms.values():
        clock(body, 50)
    times = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, body in forms.items():
            (eager if k == 'eager' else graph).reset()                     # every timing starts from the initial simplices
            times[k].append(clock(body, a.iterations))
    full = graph.run()
    rows = eager.rows

    # 3. scipy on the host, one point per call, against a one-simplex search from the same x0
    one = mk(1)
    kind = [PEM_V0_PRIORS[k] for k in NAMES]
    eager.reset()
    eager._launch(False)
    sync()
    x0_theta = eager.theta[0].cpu().numpy()                               # vertex 0 of start 0, in theta
    x0 = quantile(x0_theta, NAMES)
    lb, ub = search_bounds(NAMES)
    from scipy.special import ndtri
    buf = torch.zeros(1, len(NAMES), dtype=torch.float64, device=one.device)

    def to_theta(x):
        out = np.empty(len(NAMES))
        for j, p in enumerate(kind):
            if p.kind == UNIFORM:
                out[j] = p.a + (p.b - p.a) * x[j]
            elif p.kind == LOGUNIFORM:
                out[j] = 10.0 ** (p.a + (p.b - p.a) * x[j])
            else:
                out[j] = p.a + p.b * ndtri(x[j])
        return out

    def objective(x):
        buf.copy_(torch.as_tensor(to_theta(x)[None]))
        v = float(one.log_posterior(buf)[0])
        return -v if v == v else np.inf

    single = searcher(mk, x0=x0_theta, use_graph=True)
    single.run()                                                           # records its graph
    sp, dv = [], []
    for _ in range(a.repeats):
        sync()
        t0 = time.perf_counter()
        res = minimize(objective, x0, method='Nelder-Mead', bounds=list(zip(lb, ub)), tol=1e-4, options={'adaptive': True})
        sp.append((time.perf_counter() - t0, res.nfev, res.nit, -res.fun, res.status == 0))
        sync()
        t0 = time.perf_counter()
        r1 = single.run()
        dv.append((time.perf_counter() - t0, int(r1.nfev[0]), int(r1.nit[0]), float(r1.value[0]), bool(r1.converged[0])))

    # 4. one DE generation
    de = DifferentialEvolution(None, NAMES, seed=3, tol=1e-4, use_graph=True)
    de.f = mk(de.P).log_posterior
    de._prepare(1)
    clock(de._graph.replay, 50)
    t_de = [clock(de._graph.replay, a.iterations) for _ in range(a.repeats)]

    med = lambda t: float(np.median(t))                                    # noqa: E731
    lines = [f'optimize.NelderMead on one MI355X ({torch.cuda.get_device_name(0)}), python tools/nelder_mead_probe.py',
             f'Workload: the posterior of examples/calibration_start.py (d = {len(NAMES)} calibrated inputs, M = {M} shared nuisance draws); '
             f'S = {S} Latin-hypercube starts -> {rows} rows per launch.',
             f'Host clock over the first {a.iterations} iterations from the initial simplices, ending in a device synchronise, warm; the forms',
             f'alternate, {a.repeats} repeats each.',
             'us per iteration: median [min, max], repeats', '']
    for k, t in times.items():
        lines.append(f'  one iteration, {k:14s} {med(t):8.1f}  [{min(t):.1f}, {max(t):.1f}]   ' + ' '.join(f'{v:.1f}' for v in t))
    lines.append(f'  one DE generation, graph replay (population {de.P}) {med(t_de):8.1f}  [{min(t_de):.1f}, {max(t_de):.1f}]   '
                 + ' '.join(f'{v:.1f}' for v in t_de))
    lines.append('')
    if prof is not None:
        lines.append(f'  nm_step_kernel, rocprofv3 --kernel-trace --stats (a run of its own, {a.iterations} eager iterations): '
                     f'{prof[0]} dispatches, mean {prof[1]:.2f} us')
    else:
        lines.append(f'  nm_step_kernel under rocprofv3: NOT MEASURED ({why})')
    lines += ['', f'  the {S}-start search to the end (graph replay): nit {full.nit.tolist()}, nfev {full.nfev.tolist()}, converged '
              f'{full.converged.tolist()}', f'    log posterior {np.array2string(full.value, precision=4)}; best: start {full.best}', '',
              "scipy.optimize.minimize(method='Nelder-Mead', bounds, tol=1e-4, adaptive) on the host: the same posterior with n_chains = 1,",
              'one point per call, from vertex 0 of start 0; alternated with NelderMead(x0=the same point, use_graph=True), one simplex,',
              f'{len(NAMES) + 4} rows per launch.  wall time to convergence, function values, time per function value:', '']
    for name, runs in (('scipy, one point per call', sp), ('NelderMead, one simplex', dv)):
        for t, nfev, nit, val, ok in runs:
            lines.append(f'  {name:28s} {1e3 * t:9.2f} ms   nit {nit:4d}  nfev {nfev:4d}  {1e6 * t / nfev:8.1f} us per value   '
                         f'log posterior {val:.6f}  ({"converged" if ok else "not converged"})')
    lines.append('')
    lines.append(f'  time to convergence, scipy / NelderMead (medians): {med([r[0] for r in sp]) / med([r[0] for r in dv]):.2f}')
    lines.append("  (NelderMead's nfev is what the sequential form would have spent; it evaluates d + 4 rows per iteration.)")
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)


if __name__ == '__main__':
    main()
