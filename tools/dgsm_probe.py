#!/usr/bin/env python3
"""The fused gradient-sums launch against the composed path and against the Saltelli study, one process, one GPU, interleaved
(needs the GPU).

All 15 inputs over the PEM-v0 priors, `--n` samples (default 1e6), per design ('mc': Philox, 'sobol'):
  launch     `derivatives.gradient_sums` alone (one evaluation with its Jacobian per sample) and the sum of its partials, between
             two HIP events.
  calls      `drivers.derivative_sensitivity` (pilot + one launch + the measures); the composed path -- `Design.sample`, the explicit
             launch `derivatives.jacobian`, the same terms and sums by torch, the same pilot and the same `derivatives.measures`; and
             `drivers.sobol_indices` at the same n as n_base (n (d + 2) evaluations, no Jacobian): host clock around a call that
             ends in a device synchronise, the three alternating call by call.  The allocator's peak of each is taken in a call of
             its own after the timings.
median [min, max].

    python tools/dgsm_probe.py [--n 1000000] [--repeats 10] [--warmup 2] [--out profiles/dgsm_r01.txt]
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
from hallthrusterpem_amd import derivatives, drivers, sampling           # noqa: E402

LN10 = float(np.log(10.0))
KEYS = ('nu', 'nu_se', 'bound_ST', 'eigenvalues', 'activity')


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


def composed(n, design, method):
    """drivers.derivative_sensitivity's measures from a written-out design, a written-out Jacobian and torch reductions"""
    d = len(design.names)
    n_pilot = min(n, 4096)
    xp = design.sample(n_pilot, method=method)
    fp = derivatives.jacobian(design.as_dict(xp), wrt=[])
    c = torch.stack([fp[q] for q in derivatives.QOI_NAMES]).sum(dim=1) / n_pilot
    x = design.sample(n, method=method)
    res = derivatives.jacobian(design.as_dict(x))
    f = torch.stack([res[q] for q in derivatives.QOI_NAMES])
    g = res['jacobian']
    for i in range(d):
        if design.kind[i] == sampling.LOGUNIFORM:
            g[:, i] *= x[i] * LN10
    v = f - c[:, None]
    pairs = torch.einsum('qin,qjn->ijq', g, g)
    iu = torch.triu_indices(d, d, device=g.device)
    sums = torch.cat([v.sum(dim=1)[None], (v * v).sum(dim=1)[None], g.sum(dim=2).T, (g * g).square().sum(dim=2).T, pairs[iu[0], iu[1]]])
    return derivatives.measures(sums, n, design.kind, design.a, design.b)


def peak_mib(run):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'dgsm_r01.txt'))
    a = ap.parse_args()
    n = a.n
    design = sampling.Design(seed=1)
    varied = list(range(len(design.names)))
    d = len(varied)

    launches, calls, peaks, agree = {}, {}, {}, {}
    for method in ('mc', 'sobol'):
        centre = torch.tensor([float(v) for v in drivers.derivative_sensitivity(4096, seed=1, design=method)['centre'].values()], dtype=torch.float64)
        key = f'launch alone, design {method:5s}'
        launches.update(interleaved({key: lambda method=method, centre=centre: derivatives.gradient_sums(design, varied, n, centre, method=method)},
                                    a.repeats, a.warmup))
        group = {f'drivers.derivative_sensitivity, {method:5s}': lambda method=method: drivers.derivative_sensitivity(n, seed=1, design=method),
                 f'composed path,                  {method:5s}': lambda method=method: composed(n, design, method),
                 f'drivers.sobol_indices,          {method:5s}': lambda method=method: drivers.sobol_indices(n, seed=1, design=method)}
        calls.update(interleaved(group, a.repeats, a.warmup, host_clock=True))
        runs = list(group.values())
        fused, comp = runs[0](), runs[1]()
        agree[method] = max(float(((torch.stack(list(fused[k].values())) - comp[k]).abs() / comp[k].abs().clamp_min(1.0)).max()) for k in KEYS)
        del fused, comp
        for k, run in group.items():
            peaks[k] = peak_mib(run)

    med = lambda t: float(np.median(t))                                                            # noqa: E731
    lines = [f'The fused gradient-sums launch on one MI355X ({torch.cuda.get_device_name(0)}), python tools/dgsm_probe.py',
             f'{n} samples, {d} varied inputs over the PEM-v0 priors, {derivatives.n_rows(d)} sums per QoI; {a.repeats} timings each after '
             f'{a.warmup} warm-up rounds, the variants of a group alternating.', 'us: median [min, max]', '',
             '1. one launch and the sum of its partials, between two HIP events']
    for k, t in launches.items():
        lines.append(f'  {k:44s} {med(t):10.1f}  [{min(t):.1f}, {max(t):.1f}]   {n / med(t) * 1e6:.3e} evaluations with Jacobian/s')
    lines += ['', '2. the whole call, host clock around a call that ends in a synchronise (sobol_indices: n (d + 2) evaluations, no Jacobian)']
    for k, t in calls.items():
        lines.append(f'  {k:44s} {med(t):11.1f}  [{min(t):.1f}, {max(t):.1f}]   allocator peak {peaks[k]:9.1f} MiB')
    lines += ['', '  composed over fused and sobol_indices over fused (medians), and the largest difference between the fused and the composed',
              '  nu, nu_se, bound_ST, eigenvalues, activity, relative to max(1, |value|):']
    for method in ('mc', 'sobol'):
        f_, c_, s_ = (med(calls[k]) for k in calls if k.endswith(f'{method:5s}'))
        lines.append(f'    design {method:5s} {c_ / f_:.1f}   {s_ / f_:.2f}   max |fused - composed| {agree[method]:.2e}')
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median_us': med(t), 'us': t} for k, t in {**launches, **calls}.items()}))


if __name__ == '__main__':
    main()
