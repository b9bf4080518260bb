#!/usr/bin/env python3
"""Time per step of calibration.DeviceDRAM against calibration.DRAM(use_graph=True) on the same SystemPosterior (needs the GPU).

Workload: the `System` table of the README (tools/predictive_probe.py: 3 V_cc, 3 T, 2 u_ion x 7 positions, 8 j_ion x 40 angles =
16 conditions, 348 records), K = 64 chains, M = 50 shared nuisance draws (examples/calibration_start.py), six calibrated inputs.
DRAM evaluates K = 64 rows twice per step, DeviceDRAM 2K = 128 rows once: 2 x 64 x 50 x 16 = 102 400 coupled samples per step
either way.  The two samplers alternate in one process, each `--repeats` times for `--steps` steps after `--warmup` steps,
host clock around a run that ends in a device synchronise; nothing is kept (keep=False).  adapt_after = adapt_interval = 1000:
one adaptation per thousand steps, the ratio of the reference's production run.  The DRAM launch alone is timed as a graph of
its own (one kernel node) and as a plain launch (enqueue-bound).

    python tools/dram_step_probe.py [--steps 2000] [--warmup 200] [--repeats 3] [--out profiles/device_dram_r01.txt]
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
from hallthrusterpem_amd.calibration import DRAM, DeviceDRAM, SystemPosterior, capture_graph   # noqa: E402
from hallthrusterpem_amd.likelihood import SystemLikelihood                                     # noqa: E402


def system_table():
    rng = np.random.default_rng(0)
    ne, na = 8, 40
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
    alpha = np.sort(rng.uniform(-np.pi / 2, np.pi / 2, na))
    zq = np.array([0.0, 0.011, 0.02, 0.0399, 0.0401, 0.06, 0.08])
    return SystemLikelihood({
        'V_cc': {'x': op(3), 'y': rng.uniform(15, 35, 3), 'var_y': np.ones(3)},
        'T': {'x': op(3), 'y': rng.uniform(0.05, 0.1, 3), 'var_y': np.full(3, 1e-4)},
        'uion': {'x': op(2), 'y': rng.uniform(1e3, 2e4, (2, 7)), 'var_y': np.full((2, 7), 1e6), 'loc': zq},
        'jion': {'x': op(ne), 'y': rng.lognormal(0, 1, (ne, na)), 'var_y': rng.uniform(0.3, 1.5, (ne, na)) ** 2,
                 'loc': np.stack([np.ones(na), alpha], 1)}})


def per_step(run, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'device_dram_r01.txt'))
    a = ap.parse_args()
    lik = system_table()
    assert lik.n_cond == 16 and lik.n_rec == 348
    names = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')
    theta0 = np.array([3.0, 30.0, 5e-5, 0.03, 0.5, 0.9])
    cov0 = np.diag((0.01 * theta0) ** 2)
    K, M = 64, 50
    mk = lambda rows: SystemPosterior(names, lik, n_chains=rows, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                      shared_nuisance=True)
    kw = dict(cov0=cov0, n_chains=K, seed=2, adapt_after=1000, adapt_interval=1000)
    post_k, post_2k = mk(K), mk(2 * K)
    host = DRAM(post_k.log_posterior, theta0, device=post_k.device, use_graph=True, **kw)
    dev = DeviceDRAM(post_2k.log_posterior, theta0, device=post_2k.device, use_graph=True, **kw)
    samplers = {'DRAM(use_graph=True)': lambda n: host.run(n, keep=False), 'DeviceDRAM': lambda n: dev.run(n, keep=False)}
    for run in samplers.values():
        run(a.warmup)
    times = {k: [] for k in samplers}
    for _ in range(a.repeats):
        for k, run in samplers.items():
            times[k].append(per_step(run, a.steps))
    acc = {'DRAM(use_graph=True)': float(host.acceptance[0].mean()), 'DeviceDRAM': float(dev.accepted[0].double().mean() / dev.steps)}
    # the posterior evaluations alone, as graph replays: what either step cannot go below
    ev_k, ev_2k = post_k.capture(), post_2k.capture()
    th_k, th_2k = host.theta.clone(), dev.prop.view(2 * K, -1).clone()

    def two_evals(n):
        for _ in range(n):
            ev_k(th_k)
            ev_k(th_k)

    def one_eval(n):
        for _ in range(n):
            ev_2k(th_2k)
    evals = {'2 x posterior(64 rows)': two_evals, '1 x posterior(128 rows)': one_eval}
    for k, run in evals.items():
        run(a.warmup)
        times[k] = [per_step(run, a.steps) for _ in range(a.repeats)]
    # the DRAM launch alone (it resolves against the values of the last evaluation again and again: same work, other states)
    lone, _ = capture_graph(dev._launch, dev.device)

    def replay(n):
        for _ in range(n):
            lone.replay()

    def eager(n):
        for _ in range(n):
            dev._launch()
    for k, run in (('pem_dram_step_f64_dev alone, graph replay', replay), ('pem_dram_step_f64_dev alone, plain launch', eager)):
        run(a.warmup)
        times[k] = [per_step(run, a.steps) for _ in range(a.repeats)]
    lines = [f'DeviceDRAM against DRAM(use_graph=True) on one MI355X ({torch.cuda.get_device_name(0)}), python tools/dram_step_probe.py',
             f'Workload: System table of {lik.n_cond} conditions, {lik.n_rec} records; d = {len(names)} calibrated inputs; K = {K} chains; '
             f'M = {M} shared nuisance draws.',
             f'Samples per step: DRAM 2 evaluations x {K} rows x {M} x {lik.n_cond} = {2 * K * M * lik.n_cond}; '
             f'DeviceDRAM 1 evaluation x {2 * K} rows x {M} x {lik.n_cond} = {2 * K * M * lik.n_cond}.',
             f'{a.steps} steps per timing after {a.warmup} warm-up steps, keep=False, adapt_after = adapt_interval = 1000; host clock around a',
             f'run ending in a device synchronise; the samplers alternate, {a.repeats} repeats each.  us per step: median [min, max], repeats',
             '']
    for k, t in times.items():
        lines.append(f'  {k:44s} {np.median(t):8.1f}  [{min(t):.1f}, {max(t):.1f}]   ' + ' '.join(f'{v:.1f}' for v in t))
    h, d_ = times['DRAM(use_graph=True)'], times['DeviceDRAM']
    lines += ['', f'  step time ratio DRAM / DeviceDRAM (medians): {np.median(h) / np.median(d_):.2f}; slowest DeviceDRAM repeat '
              f'{max(d_):.1f} us against fastest DRAM repeat {min(h):.1f} us',
              f'  stage-1 acceptance over the run: DRAM {acc["DRAM(use_graph=True)"]:.2f}, DeviceDRAM {acc["DeviceDRAM"]:.2f}; '
              f'DeviceDRAM adaptations skipped: {dev.adaptation_failures}']
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median_us': float(np.median(t)), 'repeats_us': t} for k, t in times.items()}))


if __name__ == '__main__':
    main()
