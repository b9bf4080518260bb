#!/usr/bin/env python3
"""What optimize.Direct costs on the `System` posterior, and scipy's own DIRECT on the same posterior (needs the GPU).

Workload: the `System` table of tools/dram_step_probe.py (16 conditions, 348 records), the six calibrated inputs of
tools/ensemble_probe.py, M = 50 shared nuisance draws, 64 rows per launch; the reference's setting, eps = 1 and maxiter = 100.

  1. the launch alone: device events around every pem_direct_step_f64_dev launch of one eager search (the scan grows with the
     rectangles stored, so the launches of a search do not cost the same: median and maximum);
  2. one step (the launch, the posterior's launches, the copy of the values) as a graph replay: the whole search below
     divided by its launches;
  3. the whole search, graph replays with the host reading the status every 10 launches, warm (the graph recorded before);
  4. scipy.optimize.direct(eps=1, maxiter=100, locally_biased=False) on the host, the way the reference runs it: the same
     posterior with n_chains = 1, one point per call, over the same box of search coordinates; alternated with 3.

    python tools/direct_probe.py [--repeats 3] [--out profiles/direct_r01.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))

NAMES = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')
M, EPS, MAXITER = 50, 1.0, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'direct_r01.txt'))
    a = ap.parse_args()

    import torch
    from scipy.optimize import direct
    from scipy.special import ndtri
    from dram_step_probe import system_table
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.optimize import DIRECT_STATUS, Direct, search_bounds
    from hallthrusterpem_amd.sampling import LOGUNIFORM, PEM_V0_PRIORS, UNIFORM
    lik = system_table()
    assert lik.n_cond == 16 and lik.n_rec == 348
    mk = lambda K: SystemPosterior(NAMES, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)
    sync = torch.cuda.synchronize
    d = len(NAMES)

    def searcher(**kw):
        di = Direct(None, NAMES, eps=EPS, **kw)
        di.f = mk(di.rows).log_posterior
        return di

    # 1. the launch alone, inside an eager search
    eager = searcher()
    alone = []
    launch = eager._launch

    def timed_launch(finalize):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        launch(finalize)
        ev[1].record()
        alone.append(ev)
    eager._launch = timed_launch
    eager.run(max_iterations=MAXITER)                                       # warm
    alone.clear()
    ref = eager.run(max_iterations=MAXITER)
    sync()
    alone_us = np.array([e[0].elapsed_time(e[1]) * 1e3 for e in alone[:ref.launches]])

    # 3. / 4. the whole search against scipy on the host, alternating
    graph = searcher(use_graph=True)
    graph.run(max_iterations=MAXITER)                                       # records the graph
    one = mk(1)
    kind = [PEM_V0_PRIORS[k] for k in NAMES]
    lb, ub = search_bounds(NAMES)
    buf = torch.zeros(1, d, dtype=torch.float64, device=one.device)

    def to_theta(x):
        out = np.empty(d)
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
        return -float(one.log_posterior(buf)[0])

    sp, dv = [], []
    for _ in range(a.repeats):
        sync()
        t0 = time.perf_counter()
        res = direct(objective, list(zip(lb, ub)), eps=EPS, maxiter=MAXITER, locally_biased=False)
        sp.append((time.perf_counter() - t0, res.nfev, res.nit, -res.fun, res.status))
        sync()
        t0 = time.perf_counter()
        r = graph.run(max_iterations=MAXITER)
        dv.append((time.perf_counter() - t0, r.nfev, r.nit, r.value, r.status, r.launches))

    med = lambda t: float(np.median(t))                                    # noqa: E731
    t_dev = med([v[0] for v in dv])
    lines = [f'optimize.Direct on one MI355X ({torch.cuda.get_device_name(0)}), python tools/direct_probe.py',
             f'Workload: the System table of tools/dram_step_probe.py (16 conditions, 348 records), d = {d} calibrated inputs, M = {M} shared '
             f'nuisance draws, {graph.rows} rows per launch; eps = {EPS:g}, maxiter = {MAXITER}.', '',
             f'  the search: nit {ref.nit}, nfev {ref.nfev} in {ref.launches} launches ({DIRECT_STATUS[ref.status]}); '
             f'{ref.nfev / max(ref.launches - 1, 1):.1f} of {graph.rows} rows used per launch on average; log posterior {ref.value:.6f}',
             f'  pem_direct_step_f64_dev alone (device events around every launch of one eager search): median {np.median(alone_us):.2f} us, '
             f'maximum {alone_us.max():.2f} us, the last launch {alone_us[-1]:.2f} us',
             f'  one step as a graph replay (the whole search / its launches): {1e6 * t_dev / dv[0][5]:.1f} us', '',
             'the whole search, graph replays (check_every 10), against scipy.optimize.direct on the host calling the same posterior',
             f'with n_chains = 1 one point at a time over the same box; alternating, {a.repeats} repeats:', '']
    for name, runs in (('scipy, one point per call', sp), ('Direct, 64 rows per launch', dv)):
        for v in runs:
            lines.append(f'  {name:28s} {1e3 * v[0]:9.2f} ms   nit {v[2]:4d}  nfev {v[1]:5d}  {1e6 * v[0] / v[1]:8.1f} us per value   '
                         f'log posterior {v[3]:.6f}  (status {v[4]})')
    lines += ['', f'  time to the end, scipy / Direct (medians): {med([v[0] for v in sp]) / t_dev:.2f}',
              '  (the two searches need not be the same search: the host posterior evaluates one row per call, the device one 64, and the',
              '  rows of a batch see the same nuisance draws but are summed in another order; tests/test_direct.py holds the device search to',
              '  scipy on a function whose value does not depend on the batch)']
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)


if __name__ == '__main__':
    main()
