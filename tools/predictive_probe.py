#!/usr/bin/env python3
"""Time the record-prediction launch (`pem_coupled_system_predict_f64_dev`) against the multi-QoI likelihood launch
(`pem_coupled_system_loglik_f64_dev`) on the same batch and table at n = 1.25e6, interleaved with device events, and a whole
`predictive.Predictive.run` (inputs, predictions, column gather, noise, bands) at the same n.

    python tools/predictive_probe.py [--n 1250000] [--reps 20] [--rounds 5] [--json OUT]

Table: the reference-shaped one of tools/system_loglik_probe.py -- 3 V_cc, 3 T, 2 u_ion x 7 positions and 8 j_ion x 40 angles,
16 conditions, 348 records (22 per sample on average).  The predict launch writes pred[n / 16][348] (the padding records are not
written): 8 n_rec bytes per draw, ~174 B per sample, on top of the likelihood launch's traffic.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_250_000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.predictive import Predictive

    rng = np.random.default_rng(0)
    ne, na = 8, 40
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
    alpha = np.sort(rng.uniform(-np.pi / 2, np.pi / 2, na))
    zq = np.array([0.0, 0.011, 0.02, 0.0399, 0.0401, 0.06, 0.08])
    lik = SystemLikelihood({
        'V_cc': {'x': op(3), 'y': rng.uniform(15, 35, 3), 'var_y': np.ones(3)},
        'T': {'x': op(3), 'y': rng.uniform(0.05, 0.1, 3), 'var_y': np.full(3, 1e-4)},
        'uion': {'x': op(2), 'y': rng.uniform(1e3, 2e4, (2, 7)), 'var_y': np.full((2, 7), 1e6), 'loc': zq},
        'jion': {'x': op(ne), 'y': rng.lognormal(0, 1, (ne, na)), 'var_y': rng.uniform(0.3, 1.5, (ne, na)) ** 2,
                 'loc': np.stack([np.ones(na), alpha], 1)}})
    assert lik.n_cond == 16 and lik.n_rec == 348
    n_draws = a.n // lik.n_cond
    n = n_draws * lik.n_cond
    names = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')
    pp = Predictive(lik, names, seed=1)
    chain = torch.as_tensor(rng.uniform([2, 20, 3e-5, 0.01, 0.3, 0.6], [4, 40, 7e-5, 0.05, 0.7, 1.2], (200, 8, len(names))))
    table = pp.theta_table(chain)
    pp.assemble_inputs(table, n_draws)
    b = pp.batch
    dev = b.device
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    pred = torch.empty((n_draws, lik.n_rec), dtype=torch.float64, device=dev)
    runs = {
        'pem_coupled_system_loglik_f64_dev': lambda: b.run_system_loglik(lik, out=ll),
        'pem_coupled_system_predict_f64_dev': lambda: b.run_system_predict(lik, pred),
        'pem_coupled_system_predict_f64_dev[+qoi]': lambda: b.run_system_predict(lik, pred, qoi=True),
        'pem_predictive_inputs_f64_dev': lambda: pp.assemble_inputs(table, n_draws),
    }
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            ev0.record()
            for _ in range(a.reps):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            times[k].append(ev0.elapsed_time(ev1) * 1e3 / a.reps)
    # a whole run (host wall clock, synchronised): bands of 348 columns (696 with the noisy copy) over n_draws draws
    run_ms = {}
    for noise in (False, True):
        pp.run(samples=chain, n_draws=n_draws, noise=noise)
        torch.cuda.synchronize()
        w = []
        for _ in range(3):
            t0 = time.perf_counter()
            pp.run(samples=chain, n_draws=n_draws, noise=noise)
            torch.cuda.synchronize()
            w.append((time.perf_counter() - t0) * 1e3)
        run_ms['noise' if noise else 'plain'] = {'median': float(np.median(w)), 'min': float(np.min(w))}
    res = {'n': n, 'n_draws': n_draws, 'reps': a.reps, 'rounds': a.rounds,
           'table': {'n_cond': lik.n_cond, 'n_rec': lik.n_rec, 'n_cols': pp.n_cols, 'n_node': lik.n_node},
           'us_per_launch': {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()},
           'pred_bytes_per_sample': 8 * pp.n_cols / lik.n_cond,
           'run_ms': run_ms}
    base = res['us_per_launch']['pem_coupled_system_loglik_f64_dev']['median']
    res['ratio_to_loglik_launch'] = {k: v['median'] / base for k, v in res['us_per_launch'].items()}
    print(json.dumps(res, indent=1))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
