#!/usr/bin/env python3
"""The fused second-order Saltelli launch against the composed path and against the first-order launch, one process, one GPU,
interleaved (needs the GPU).

The fixed-operating-point study (P_b, V_a, mdot_a pinned: 12 varied inputs), `--n-base` base samples (default 1e6), per design
('mc', 'sobol'):
  launches   `fp32.saltelli2_sums` (2 nv + 2 = 26 evaluations per base sample) and `fp32.saltelli_sums` (nv + 2 = 14), fp64 and
             fp32 model: one launch and the sum of its partials between two HIP events, the variants alternating launch by launch.
  drivers    `drivers.sobol_indices(second_order=True)` fused (pilot + one launch) and composed (`fused=False`: 26 design blocks
             written out and evaluated per batch, the sums by torch), fp64: host clock around a call that ends in a device
             synchronise, the two alternating call by call.
median [min, max]; evaluations per second from the medians.

    python tools/saltelli2_probe.py [--n-base 1000000] [--repeats 10] [--warmup 2] [--out profiles/saltelli2_r01.txt]
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
from hallthrusterpem_amd import drivers, sampling                          # noqa: E402
from hallthrusterpem_amd.fp32 import saltelli2_sums, saltelli_sums         # noqa: E402

FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6}


def interleaved(variants: dict, repeats: int, warmup: int, host_clock: bool = False):
    """{name: [us per call]}: the variants take turns, one call each per round"""
    times = {k: [] for k in variants}
    for r in range(warmup + repeats):
        for k, run in variants.items():
            if host_clock:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                us = (time.perf_counter() - t0) * 1e6
            else:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run()
                t1.record()
                t1.synchronize()
                us = t0.elapsed_time(t1) * 1e3
            if r >= warmup:
                times[k].append(us)
    return times


def call_key(how, method):
    return f'sobol_indices(second_order=True), {how:8s}, fp64, {method:5s} design'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-base', type=int, default=1_000_000)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'saltelli2_r01.txt'))
    a = ap.parse_args()
    n = a.n_base
    pri = dict(sampling.PEM_V0_PRIORS)
    for k, v in FIXED.items():
        pri[k] = sampling.Prior(sampling.UNIFORM, v, v, 'fixed')
    design = sampling.Design(priors=pri, seed=1)
    varied = [i for i, k in enumerate(design.names) if k not in FIXED]
    nv = len(varied)
    centre = (saltelli_sums(design, varied[:1], 4096, precision='fp64')[0][0] / 8192).cpu().numpy()

    launches, evals = {}, {}
    for precision in ('fp64', 'fp32'):
        group = {}
        for m in ('mc', 'sobol'):
            k2, k1 = f'second-order launch, {precision} model, {m:5s} design', f'first-order  launch, {precision} model, {m:5s} design'
            group[k2] = lambda m=m, p=precision: saltelli2_sums(design, varied, n, centre, precision=p, method=m)
            group[k1] = lambda m=m, p=precision: saltelli_sums(design, varied, n, precision=p, method=m)
            evals[k2], evals[k1] = n * (2 * nv + 2), n * (nv + 2)
        launches.update(interleaved(group, a.repeats, a.warmup))
    calls = {}
    for m in ('mc', 'sobol'):
        group = {call_key('fused', m): lambda m=m: drivers.sobol_indices(n, seed=1, fixed=FIXED, design=m, second_order=True),
                 call_key('composed', m): lambda m=m: drivers.sobol_indices(n, seed=1, fixed=FIXED, design=m, second_order=True, fused=False)}
        calls.update(interleaved(group, a.repeats, a.warmup, host_clock=True))

    med = lambda t: float(np.median(t))                                                            # noqa: E731
    lines = [f'The fused second-order Saltelli launch on one MI355X ({torch.cuda.get_device_name(0)}), python tools/saltelli2_probe.py',
             f'{n} base samples, {nv} varied inputs (P_b, V_a, mdot_a fixed); {a.repeats} timings each after {a.warmup} warm-up rounds, the '
             'variants of a group alternating.', 'us: median [min, max]', '',
             '1. one launch and the sum of its partials, between two HIP events']
    for k, t in launches.items():
        lines.append(f'  {k:58s} {med(t):10.1f}  [{min(t):.1f}, {max(t):.1f}]   {evals[k] / med(t) * 1e6:.3e} evaluations/s')
    lines += ['', '  evaluations/s, second-order over first-order (medians):']
    for precision in ('fp64', 'fp32'):
        for m in ('mc', 'sobol'):
            k2, k1 = f'second-order launch, {precision} model, {m:5s} design', f'first-order  launch, {precision} model, {m:5s} design'
            lines.append(f'    {precision} {m:5s} {(evals[k2] / med(launches[k2])) / (evals[k1] / med(launches[k1])):.2f}'
                         f'   (time ratio {med(launches[k2]) / med(launches[k1]):.2f} for {evals[k2] / evals[k1]:.2f} x the evaluations)')
    lines += ['', '2. the whole driver call (pilot, launches, reductions, the indices), host clock around a call that ends in a synchronise']
    for k, t in calls.items():
        lines.append(f'  {k:66s} {med(t):11.1f}  [{min(t):.1f}, {max(t):.1f}]')
    lines += ['', '  composed over fused (medians):']
    for m in ('mc', 'sobol'):
        f_, c_ = med(calls[call_key('fused', m)]), med(calls[call_key('composed', m)])
        lines.append(f'    fp64 {m:5s} {c_ / f_:.1f}')
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median_us': med(t), 'us': t} for k, t in {**launches, **calls}.items()}))


if __name__ == '__main__':
    main()
