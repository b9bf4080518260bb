#!/usr/bin/env python3
"""Time per step and ESS per posterior evaluation of calibration.DeviceEnsemble against calibration.DeviceDRAM on the same
SystemPosterior (needs the GPU).

Workload: the `System` table of the README (tools/dram_step_probe.py: 16 conditions, 348 records), six calibrated inputs, M = 50
shared nuisance draws.  DeviceDRAM runs K = 64 chains: 2K = 128 posterior rows per step, in one evaluation.  DeviceEnsemble runs
E = 4 ensembles of K = 32 walkers: E K = 128 posterior rows per step, in two evaluations of 64.  Either step is one graph replay
of 128 x 50 x 16 = 102 400 coupled samples.  The two samplers alternate in one process, each `--repeats` times for `--steps` steps
after `--warmup` steps, host clock around a run that ends in a device synchronise; nothing is kept (keep=False).  The ensemble
launch alone is timed as a graph of its own (one kernel node) and as a plain launch (enqueue-bound).

Then both samplers run `--ess-steps` further steps with the trace kept -- the same number of posterior evaluations -- and
diagnostics.ess reads them: the K chains for DeviceDRAM, the E ensemble-mean series for DeviceEnsemble (the walkers of one ensemble
are not independent chains).  Both start from a 1 % ball / 1 % diagonal covariance round the same point; DeviceDRAM adapts after
200 steps and every 100, the ensemble has nothing to tune.

    python tools/ensemble_probe.py [--steps 2000] [--warmup 200] [--repeats 3] [--ess-steps 4000] [--out profiles/ensemble_r01.txt]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
from dram_step_probe import per_step, system_table                                              # noqa: E402
from hallthrusterpem_amd import diagnostics                                                      # noqa: E402
from hallthrusterpem_amd.calibration import DeviceDRAM, DeviceEnsemble, SystemPosterior, capture_graph   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ess-steps', type=int, default=4000)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'ensemble_r01.txt'))
    a = ap.parse_args()
    lik = system_table()
    assert lik.n_cond == 16 and lik.n_rec == 348
    names = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')
    theta0 = np.array([3.0, 30.0, 5e-5, 0.03, 0.5, 0.9])
    K_dram, E, K, M = 64, 4, 32, 50
    mk = lambda rows: SystemPosterior(names, lik, n_chains=rows, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                      shared_nuisance=True)
    post_dram, post_ens = mk(2 * K_dram), mk(E * K // 2)
    dram = DeviceDRAM(post_dram.log_posterior, theta0, cov0=np.diag((0.01 * theta0) ** 2), n_chains=K_dram, seed=2, adapt_after=200,
                      adapt_interval=100, device=post_dram.device)
    ens = DeviceEnsemble(post_ens.log_posterior, DeviceEnsemble.ball(theta0, 0.01 * theta0, K, n_ensembles=E, seed=3), seed=2,
                         device=post_ens.device)
    samplers = {'DeviceDRAM, 1 x posterior(128 rows)': lambda n: dram.run(n, keep=False),
                'DeviceEnsemble, 2 x posterior(64 rows)': lambda n: ens.run(n, keep=False)}
    for run in samplers.values():
        run(a.warmup)
    times = {k: [] for k in samplers}
    for _ in range(a.repeats):
        for k, run in samplers.items():
            times[k].append(per_step(run, a.steps))
    # the ensemble launch alone (it resolves against the values of the last evaluation again and again: same work, other states)
    lone, _ = capture_graph(ens._launch, ens.device)

    def replay(n):
        for _ in range(n):
            lone.replay()

    def eager(n):
        for _ in range(n):
            ens._launch()
    for k, run in (('pem_ensemble_step_f64_dev alone, graph replay', replay), ('pem_ensemble_step_f64_dev alone, plain launch', eager)):
        run(a.warmup)
        times[k] = [per_step(run, a.steps) for _ in range(a.repeats)]
    # ESS per posterior evaluation, on fresh samplers (the launches above left `ens` between two half-steps of no run)
    dram = DeviceDRAM(post_dram.log_posterior, theta0, cov0=np.diag((0.01 * theta0) ** 2), n_chains=K_dram, seed=2, adapt_after=200,
                      adapt_interval=100, device=post_dram.device)
    ens = DeviceEnsemble(post_ens.log_posterior, DeviceEnsemble.ball(theta0, 0.01 * theta0, K, n_ensembles=E, seed=3), seed=2,
                         device=post_ens.device)
    n = a.ess_steps
    ess_dram, _ = diagnostics.ess(dram.run(n), burnin=0.25)
    ess_ens, _ = diagnostics.ess(ens.run(n).mean(dim=2), burnin=0.25)
    ess_dram, ess_ens = np.asarray(ess_dram.cpu(), dtype=np.float64), np.asarray(ess_ens.cpu(), dtype=np.float64)
    evals = {'DeviceDRAM': n * 2 * K_dram, 'DeviceEnsemble': n * E * K}
    lines = [f'DeviceEnsemble against DeviceDRAM on one MI355X ({torch.cuda.get_device_name(0)}), python tools/ensemble_probe.py',
             f'Workload: System table of {lik.n_cond} conditions, {lik.n_rec} records; d = {len(names)} calibrated inputs; M = {M} shared '
             'nuisance draws.',
             f'Posterior rows per step (one graph replay): DeviceDRAM 1 evaluation x {2 * K_dram} rows ({K_dram} chains); DeviceEnsemble '
             f'2 evaluations x {E * K // 2} rows ({E} ensembles x {K} walkers).',
             f'{a.steps} steps per timing after {a.warmup} warm-up steps, keep=False; host clock around a run ending in a device synchronise;',
             f'the samplers alternate, {a.repeats} repeats each.  us per step: median [min, max], repeats', '']
    for k, t in times.items():
        lines.append(f'  {k:48s} {np.median(t):8.1f}  [{min(t):.1f}, {max(t):.1f}]   ' + ' '.join(f'{v:.1f}' for v in t))
    d_, e_ = times['DeviceDRAM, 1 x posterior(128 rows)'], times['DeviceEnsemble, 2 x posterior(64 rows)']
    lines += ['', f'  step time ratio DeviceEnsemble / DeviceDRAM (medians): {np.median(e_) / np.median(d_):.2f}', '',
              f'ESS (diagnostics.ess, burnin 0.25) of {n} steps from a 1 % start, {evals["DeviceDRAM"]} = {evals["DeviceEnsemble"]} posterior '
              'evaluations each;', f'DeviceDRAM over its {K_dram} chains, DeviceEnsemble over its {E} ensemble-mean series.  Per parameter '
              + ' '.join(names) + ':',
              '  DeviceDRAM      ESS ' + ' '.join(f'{v:9.1f}' for v in ess_dram) + f'   per 1000 evaluations: min {1e3 * ess_dram.min() / evals["DeviceDRAM"]:.3f}',
              '  DeviceEnsemble  ESS ' + ' '.join(f'{v:9.1f}' for v in ess_ens) + f'   per 1000 evaluations: min {1e3 * ess_ens.min() / evals["DeviceEnsemble"]:.3f}',
              f'  acceptance: DeviceDRAM stage 1 {float(dram.acceptance[0].mean()):.2f}, stage 2 {float(dram.acceptance[1].mean()):.2f}; '
              f'DeviceEnsemble {float(ens.acceptance.mean()):.2f}']
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median_us': float(np.median(t)), 'repeats_us': t} for k, t in times.items()}))


if __name__ == '__main__':
    main()
