#!/usr/bin/env python3
"""Time per step of calibration.DeviceTemperedEnsemble against calibration.DeviceEnsemble on the same SystemPosterior rows (needs
the GPU).

Workload: the `System` table of the README (tools/dram_step_probe.py: 16 conditions, 348 records), the six calibrated inputs of
tools/ensemble_probe.py, M = 50 shared nuisance draws.  DeviceTemperedEnsemble runs R = 1 replica of a ladder of T = 4 temperatures
(1, 0.5, 0.25, 0.125) with K = 32 walkers; DeviceEnsemble runs E = 4 ensembles of K = 32 walkers: either step is two evaluations
of 64 posterior rows, 2 x 64 x 50 x 16 = 102 400 coupled samples, and two sampler launches, in one graph replay.  What differs is
that the tempered sampler calls log_likelihood and log_prior (the prior launch and the marginalisation run apart, the prior is
not added inside the marginalisation launch) where the ensemble calls log_posterior, and that its launch decides the swaps.
(d = 6 is the ensemble probe's workload: the coupled model has 12 calibratable inputs and the samplers ask K >= 2 d, so K = 32
walkers cannot carry the reference's 17 parameters.)

The two samplers alternate in one process, each `--repeats` times for `--steps` steps after `--warmup` steps, host clock around a
run that ends in a device synchronise; nothing is kept (keep=False).  Each sampler launch alone is timed as a graph of its own
(one kernel node).

    python tools/tempering_probe.py [--steps 2000] [--warmup 200] [--repeats 3] [--out profiles/tempering_r01.txt]
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
from hallthrusterpem_amd.calibration import DeviceEnsemble, DeviceTemperedEnsemble, SystemPosterior, capture_graph   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'tempering_r01.txt'))
    a = ap.parse_args()
    lik = system_table()
    assert lik.n_cond == 16 and lik.n_rec == 348
    names = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')
    theta0 = np.array([3.0, 30.0, 5e-5, 0.03, 0.5, 0.9])
    T, K, M = 4, 32, 50
    betas = [1.0, 0.5, 0.25, 0.125]
    mk = lambda: SystemPosterior(names, lik, n_chains=T * K // 2, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                 shared_nuisance=True)
    post_ens, post_pt = mk(), mk()
    x0 = DeviceEnsemble.ball(theta0, 0.01 * theta0, K, n_ensembles=T, seed=3)
    ens = DeviceEnsemble(post_ens.log_posterior, x0, seed=2, device=post_ens.device)
    pt = DeviceTemperedEnsemble(post_pt.log_likelihood, post_pt.log_prior, x0, betas=betas, seed=2, device=post_pt.device)
    samplers = {'DeviceEnsemble, 4 ensembles, 2 x log_posterior(64 rows)': lambda n: ens.run(n, keep=False),
                'DeviceTemperedEnsemble, T = 4, 2 x [log_likelihood, log_prior](64 rows)': lambda n: pt.run(n, keep=False)}
    for run in samplers.values():
        run(a.warmup)
    times = {k: [] for k in samplers}
    for _ in range(a.repeats):
        for k, run in samplers.items():
            times[k].append(per_step(run, a.steps))
    swap_rates = pt.swap_rates().mean(dim=0).tolist()
    # each launch alone (it resolves against the values of the last evaluation again and again: same work, other states)
    lone = {'pem_ensemble_step_f64_dev alone, graph replay': capture_graph(ens._launch, ens.device)[0],
            'pem_tempered_ensemble_step_f64_dev alone, graph replay': capture_graph(pt._launch, pt.device)[0]}

    def replay(graph):
        def run(n):
            for _ in range(n):
                graph.replay()
        return run
    for k in lone:
        times[k] = []
    for _ in range(a.repeats):
        for k, graph in lone.items():
            replay(graph)(a.warmup)
            times[k].append(per_step(replay(graph), a.steps))
    lines = [f'DeviceTemperedEnsemble against DeviceEnsemble on one MI355X ({torch.cuda.get_device_name(0)}), python tools/tempering_probe.py',
             f'Workload: System table of {lik.n_cond} conditions, {lik.n_rec} records; d = {len(names)} calibrated inputs; M = {M} shared '
             'nuisance draws.',
             f'Posterior rows per step (one graph replay): 2 evaluations x {T * K // 2} rows either way -- DeviceEnsemble {T} ensembles x {K} '
             f'walkers, DeviceTemperedEnsemble 1 replica x {T} temperatures {betas} x {K} walkers.',
             f'{a.steps} steps per timing after {a.warmup} warm-up steps, keep=False; host clock around a run ending in a device synchronise;',
             f'the samplers alternate, {a.repeats} repeats each.  us per step (per replay for a launch alone): median [min, max], repeats', '']
    for k, t in times.items():
        lines.append(f'  {k:76s} {np.median(t):8.1f}  [{min(t):.1f}, {max(t):.1f}]   ' + ' '.join(f'{v:.1f}' for v in t))
    e_, p_ = (times[k] for k in samplers)
    lines += ['', f'  step time ratio DeviceTemperedEnsemble / DeviceEnsemble (medians): {np.median(p_) / np.median(e_):.2f}',
              f'  swap rates of the timed run, per pair (t, t + 1): ' + ' '.join(f'{v:.2f}' for v in swap_rates)]
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median_us': float(np.median(t)), 'repeats_us': t} for k, t in times.items()}))


if __name__ == '__main__':
    main()
