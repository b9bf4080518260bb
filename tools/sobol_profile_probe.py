#!/usr/bin/env python3
"""The fused profile Saltelli launch against the composed path, one process, one GPU, interleaved (needs the GPU).

The fixed-operating-point study (P_b, V_a, mdot_a pinned: 12 varied inputs), `--n-base` base samples (default 1e6), per norm
('log10', 'none'), Philox design:
  launch     `sobol_profile.profile_sums` alone (nv + 2 = 14 evaluations per base sample) and the sum of its partials, between two
             HIP events.
  drivers    `drivers.sobol_profile` (pilot + one launch + the indices) and the composed path -- per batch `Design.fill` for every
             one of the 14 blocks, `CoupledBatch(profile=True)`, the same terms and sums by torch, the same pilot and the same
             arithmetic for the indices: host clock around a call that ends in a device synchronise, the two alternating call by
             call.  The allocator's peak of each is taken in a call of its own after the timings.
median [min, max].  exp/s: the exponentials the launch executes (2 for A, 2 for B, and per AB_j one per beam width that differs from
A's: c1 moves one, c2 and c3 both, the other inputs none -- 9 per base sample and angle in this study) over the launch's median,
beside the 2 per evaluation and angle (28) a launch without the reuse would execute.

    python tools/sobol_profile_probe.py [--n-base 1000000] [--repeats 10] [--warmup 2] [--out profiles/sobol_profile_r01.txt]
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
from hallthrusterpem_amd import drivers, sampling, sobol_profile           # noqa: E402
from hallthrusterpem_amd.batch import CoupledBatch                         # noqa: E402

FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6}
NA = 91
KDE_EXP_PER_S = 1.23e12                      # what the KDE kernel reaches (the marginals' kernel (b))
WIDTHS_MOVED = {'P_b': 2, 'c1': 1, 'c2': 2, 'c3': 2}


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


def composed(n, design, varied, norm, batch_size=1 << 20):
    """drivers.sobol_profile's result from written-out blocks, stored profiles and torch reductions"""
    dev = torch.device('cuda', torch.cuda.current_device())
    nv = len(varied)

    def profile(b, first, swap):
        design.fill(b.inputs, first_index=first, swap_dim=swap)
        b.run()
        return torch.log10_(b.j_ion) if norm == 'log10' else b.j_ion

    n_pilot = min(n, 4096)
    bA, bB = (CoupledBatch(n_pilot, device=dev, profile=True, thruster_qoi=False) for _ in range(2))
    c = (profile(bA, 0, -1) + profile(bB, 0, -2)).sum(dim=0) / (2 * n_pilot)
    acc = torch.zeros((2 + 4 * nv, NA), dtype=torch.float64, device=dev)
    bX = None
    for off in range(0, n, batch_size):
        m = min(batch_size, n - off)
        if bX is None or bX.n != m:
            bA, bB, bX = (CoupledBatch(m, device=dev, profile=True, thruster_qoi=False) for _ in range(3))
        fA, fB = profile(bA, off, -1), profile(bB, off, -2)
        vA, vB = fA - c, fB - c
        acc[0] += (vA + vB).sum(dim=0)
        acc[1] += (vA * vA + vB * vB).sum(dim=0)
        for j, d in enumerate(varied):
            dd = profile(bX, off, d) - fA
            t1, t2 = vB * dd, dd * dd
            acc[2 + 4 * j] += t1.sum(dim=0)
            acc[3 + 4 * j] += (t1 * t1).sum(dim=0)
            acc[4 + 4 * j] += t2.sum(dim=0)
            acc[5 + 4 * j] += (t2 * t2).sum(dim=0)
    return sobol_profile.indices(acc, n, c)


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
    ap.add_argument('--n-base', type=int, default=1_000_000)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'sobol_profile_r01.txt'))
    a = ap.parse_args()
    n = a.n_base
    pri = dict(sampling.PEM_V0_PRIORS)
    for k, v in FIXED.items():
        pri[k] = sampling.Prior(sampling.UNIFORM, v, v, 'fixed')
    design = sampling.Design(priors=pri, seed=1)
    varied = [i for i, k in enumerate(design.names) if k not in FIXED]
    nv = len(varied)
    exps = 4 + sum(WIDTHS_MOVED.get(design.names[i], 0) for i in varied)

    launches, calls, peaks, agree = {}, {}, {}, {}
    for norm in ('log10', 'none'):
        centre = drivers.sobol_profile(4096, seed=1, fixed=FIXED, norm=norm)['centre']
        key = f'launch alone, norm {norm:5s}'
        launches.update(interleaved({key: lambda norm=norm, centre=centre: sobol_profile.profile_sums(design, varied, n, centre, norm=norm)},
                                    a.repeats, a.warmup))
        group = {f'drivers.sobol_profile, norm {norm:5s}': lambda norm=norm: drivers.sobol_profile(n, seed=1, fixed=FIXED, norm=norm),
                 f'composed path,         norm {norm:5s}': lambda norm=norm: composed(n, design, varied, norm)}
        calls.update(interleaved(group, a.repeats, a.warmup, host_clock=True))
        fused, comp = (run() for run in group.values())
        agree[norm] = max(float((fused[k] - comp[k]).abs().max()) for k in ('S1', 'ST', 'GS1', 'GST'))
        del fused, comp
        for k, run in group.items():
            peaks[k] = peak_mib(run)

    med = lambda t: float(np.median(t))                                                            # noqa: E731
    lines = [f'The fused profile Saltelli launch on one MI355X ({torch.cuda.get_device_name(0)}), python tools/sobol_profile_probe.py',
             f'{n} base samples, {nv} varied inputs (P_b, V_a, mdot_a fixed), Philox design, {n * (nv + 2)} evaluations of 91 angles; '
             f'{a.repeats} timings each after {a.warmup} warm-up rounds, the variants of a group alternating.', 'us: median [min, max]', '',
             '1. one launch and the sum of its partials, between two HIP events']
    for k, t in launches.items():
        lines.append(f'  {k:40s} {med(t):10.1f}  [{min(t):.1f}, {max(t):.1f}]   {n * (nv + 2) / med(t) * 1e6:.3e} evaluations/s   '
                     f'{exps * NA * n / med(t) * 1e6:.3e} exp/s executed ({exps} per base sample and angle; '
                     f'{exps * NA * n / med(t) * 1e6 / KDE_EXP_PER_S:.2f} of the KDE kernel\'s 1.23e12), '
                     f'{2 * (nv + 2) * NA * n / med(t) * 1e6:.3e} exp/s at 2 per evaluation')
    lines += ['', '2. the whole call (pilot, launches, reductions, the indices), host clock around a call that ends in a synchronise']
    for k, t in calls.items():
        lines.append(f'  {k:40s} {med(t):11.1f}  [{min(t):.1f}, {max(t):.1f}]   allocator peak {peaks[k]:9.1f} MiB')
    lines += ['', '  composed over fused (medians), and the largest difference between their S1, ST, GS1, GST:']
    for norm in ('log10', 'none'):
        f_, c_ = med(calls[f'drivers.sobol_profile, norm {norm:5s}']), med(calls[f'composed path,         norm {norm:5s}'])
        lines.append(f'    norm {norm:5s} {c_ / f_:.1f}    max |fused - composed| {agree[norm]:.2e}')
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median_us': med(t), 'us': t} for k, t in {**launches, **calls}.items()}))


if __name__ == '__main__':
    main()
