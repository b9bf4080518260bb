#!/usr/bin/env python3
"""Time per step of optimize.Powell, and scipy's own Powell on the same posterior (needs the GPU).

Workload: the posterior of examples/calibration_start.py (synthetic System data, 3 calibrated inputs, M = 50 shared nuisance
draws), S = 8 Latin-hypercube starts -> 8 rows per launch (one value per search and launch).

  1. one step (pem_powell_step_f64_dev, the posterior's launches, the copy of the values), eager and as a graph replay: host
     clock over `--steps` steps ending in a device synchronise, warm, `--repeats` times, alternating; one Nelder-Mead iteration
     (8 starts, 56 rows) as a graph replay measured in the same run beside it;
  2. the mean of powell_step_kernel per dispatch, from a `rocprofv3 --kernel-trace --stats` run of its own (this script started
     again as the profiled child, before this process opens the GPU);
  3. scipy.optimize.minimize(method='Powell', bounds=..., options={'xtol': 1e-4, 'ftol': 1e-4}) on the host, the way the
     reference runs it: the same posterior with n_chains = 1, one point per call, from the same x0 as start 0, over the same
     search coordinates; alternated with a one-start Powell from that x0.  Both report nit / nfev;
  4. the 8-start and a 64-start search to the end, as context.

    python tools/powell_probe.py [--steps 400] [--repeats 3] [--out profiles/powell_r01.txt]
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
sys.path.insert(0, str(ROOT / 'tools'))
from nelder_mead_probe import NAMES, M, S, posterior_factory                       # noqa: E402
from nelder_mead_probe import searcher as nm_searcher                              # noqa: E402


def searcher(mk, **kw):
    from hallthrusterpem_amd.optimize import Powell
    po = Powell(None, NAMES, seed=3, **kw)
    po.f = mk(po.rows).log_posterior
    return po


def child(steps):
    """the profiled run: eager steps of the 8-start search (every dispatch of powell_step_kernel is one step)"""
    import torch
    po = searcher(posterior_factory(), n_starts=S)
    po.reset()
    for _ in range(steps):
        po._step()
    torch.cuda.synchronize()


def profile_kernel(steps):
    """(calls, mean us) of powell_step_kernel from rocprofv3's kernel statistics, or a note why not"""
    exe = shutil.which('rocprofv3')
    if exe is None:
        return None, 'rocprofv3 not found'
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [exe, '--kernel-trace', '--stats', '-f', 'csv', '-d', tmp, '-o', 'powell', '--', sys.executable,
               str(Path(__file__).resolve()), '--child', '--steps', str(steps)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            return None, f'rocprofv3 exited with {out.returncode}: {out.stderr[-300:]}'
        for f in Path(tmp).rglob('*kernel_stats.csv'):
            for r in csv.DictReader(open(f)):
                if 'powell_step_kernel' in r['Name']:
                    return (int(r['Calls']), float(r['AverageNs']) / 1e3), None
    return None, 'powell_step_kernel not in the kernel statistics'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'powell_r01.txt'))
    a = ap.parse_args()
    if a.child:
        return child(a.steps)
    prof, why = profile_kernel(a.steps)                   # before this process opens the GPU

    import torch
    from scipy.optimize import minimize
    from scipy.special import ndtri
    from hallthrusterpem_amd.optimize import search_bounds
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

    # 1. one step, eager and replayed; one Nelder-Mead iteration beside it
    eager, graph = searcher(mk, n_starts=S), searcher(mk, n_starts=S, use_graph=True)
    graph._prepare(1, 0)                                                   # records the graph
    eager.reset()
    nm = nm_searcher(mk, n_starts=S, use_graph=True)
    nm._prepare(1)
    forms = {'Powell step, eager': (eager, eager._step), 'Powell step, graph replay': (graph, graph._graph.replay),
             'Nelder-Mead iteration, graph replay': (nm, nm._graph.replay)}
    for _, body in forms.values():
        clock(body, 50)
    times = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, (obj, body) in forms.items():
            obj.reset()                                                    # every timing starts from the starts
            times[k].append(clock(body, a.steps))

    # 4. the searches to the end
    graph.run()                                                            # records the graph again, with room for the history
    t0 = time.perf_counter()
    full = graph.run()
    t_full = time.perf_counter() - t0
    wide = searcher(mk, n_starts=64, use_graph=True)
    wide.run()                                                             # records its graph
    t0 = time.perf_counter()
    full64 = wide.run()
    t_full64 = time.perf_counter() - t0

    # 3. scipy on the host, one point per call, against a one-start search from the same x0
    one = mk(1)
    kind = [PEM_V0_PRIORS[k] for k in NAMES]
    x0 = eager.u0[0].cpu().numpy()                                         # start 0 in search coordinates
    lb, ub = search_bounds(NAMES)
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

    single = searcher(mk, x0=to_theta(x0), use_graph=True)
    single.run()                                                           # records its graph
    sp, dv = [], []
    for _ in range(a.repeats):
        sync()
        t0 = time.perf_counter()
        res = minimize(objective, x0, method='Powell', bounds=list(zip(lb, ub)), options={'xtol': 1e-4, 'ftol': 1e-4})
        sp.append((time.perf_counter() - t0, res.nfev, res.nit, -res.fun, res.status == 0))
        sync()
        t0 = time.perf_counter()
        r1 = single.run()
        dv.append((time.perf_counter() - t0, int(r1.nfev[0]), int(r1.nit[0]), float(r1.value[0]), bool(r1.converged[0])))

    med = lambda t: float(np.median(t))                                    # noqa: E731
    lines = [f'optimize.Powell on one MI355X ({torch.cuda.get_device_name(0)}), python tools/powell_probe.py',
             f'Workload: the posterior of examples/calibration_start.py (d = {len(NAMES)} calibrated inputs, M = {M} shared nuisance draws); '
             f'S = {S} Latin-hypercube starts -> {eager.rows} rows per launch (Nelder-Mead: {nm.rows}).',
             f'Host clock over the first {a.steps} steps from the starts, ending in a device synchronise, warm; the forms alternate,',
             f'{a.repeats} repeats each.', 'us per step: median [min, max], repeats', '']
    for k, t in times.items():
        lines.append(f'  {k:38s} {med(t):8.1f}  [{min(t):.1f}, {max(t):.1f}]   ' + ' '.join(f'{v:.1f}' for v in t))
    lines.append('')
    if prof is not None:
        lines.append(f'  powell_step_kernel, rocprofv3 --kernel-trace --stats (a run of its own, {a.steps} eager steps): '
                     f'{prof[0]} dispatches, mean {prof[1]:.2f} us')
    else:
        lines.append(f'  powell_step_kernel under rocprofv3: NOT MEASURED ({why})')
    for n, r, t in ((S, full, t_full), (64, full64, t_full64)):
        lines += ['', f'  the {n}-start search to the end (graph replay, check_every 50): {1e3 * t:.2f} ms, {r.history.shape[0] + 1} launches; '
                  f'nit {r.nit.min()} ... {r.nit.max()}, nfev {r.nfev.min()} ... {r.nfev.max()}, ftol met by {int(r.converged.sum())} of {n}',
                  f'    best log posterior {r.best_value[r.best]:.6f} (start {r.best}); searches within 1e-3 of it: '
                  f'{int((r.best_value >= r.best_value[r.best] - 1e-3).sum())}']
    lines += ['', "scipy.optimize.minimize(method='Powell', bounds, xtol=1e-4, ftol=1e-4) on the host: the same posterior with n_chains = 1,",
              'one point per call, from start 0; alternated with Powell(x0=the same point, use_graph=True), one search, one row per launch.',
              'wall time to the end, function values, time per function value:', '']
    for name, runs in (('scipy, one point per call', sp), ('Powell, one search', dv)):
        for t, nfev, nit, val, ok in runs:
            lines.append(f'  {name:28s} {1e3 * t:9.2f} ms   nit {nit:4d}  nfev {nfev:4d}  {1e6 * t / nfev:8.1f} us per value   '
                         f'log posterior {val:.6f}  ({"ftol met" if ok else "not converged"})')
    lines.append('')
    lines.append(f'  time to the end, scipy / Powell (medians): {med([r[0] for r in sp]) / med([r[0] for r in dv]):.2f}')
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)


if __name__ == '__main__':
    main()
