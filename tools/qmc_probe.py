#!/usr/bin/env python3
"""The Sobol' design's kernels against their Monte-Carlo twins, same shapes, same GPU, interleaved, by HIP events (needs the GPU).

  1. pem_sample_sobol_f64_dev against pem_sample_f64_dev: the 15 PEM-v0 priors x 1e7 samples into one resident [15][1e7] tensor
     (1.2 GB written per launch).
  2. the fused Saltelli launch on either design, fp64 and fp32 model: BASELINE configs[4]'s 2e7-evaluation design (1 428 572 base
     samples x 14, three inputs fixed), the grid sizes fp32.saltelli_sums picks.

Each timing is one launch between two events on the current stream; the variants of a group alternate launch by launch, `--repeats`
launches each after `--warmup`; median [min, max] in microseconds.

    python tools/qmc_probe.py [--repeats 20] [--warmup 3] [--out profiles/qmc_r01.txt]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from hallthrusterpem_amd import sampling                       # noqa: E402
from hallthrusterpem_amd.fp32 import saltelli_sums             # noqa: E402


def interleaved(variants: dict, repeats: int, warmup: int):
    """{name: [us per launch]}: the variants take turns, one launch each per round"""
    times = {k: [] for k in variants}
    for r in range(warmup + repeats):
        for k, run in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            t1.synchronize()
            if r >= warmup:
                times[k].append(t0.elapsed_time(t1) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'qmc_r01.txt'))
    a = ap.parse_args()
    n = 10_000_000
    design = sampling.Design(seed=1)
    x = torch.empty((design.ndim, n), dtype=torch.float64, device='cuda')
    fills = {
        "pem_sample_f64_dev       (mc)": lambda: design.fill(x),
        "pem_sample_sobol_f64_dev (sobol, shifted)": lambda: design.fill(x, method='sobol'),
        "pem_sample_sobol_f64_dev (sobol, first_index 12345)": lambda: design.fill(x, first_index=12345, method='sobol'),
    }
    t_fill = interleaved(fills, a.repeats, a.warmup)

    fixed = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6}
    pri = dict(sampling.PEM_V0_PRIORS)
    for k, v in fixed.items():
        pri[k] = sampling.Prior(sampling.UNIFORM, v, v, 'fixed')
    sdesign = sampling.Design(priors=pri, seed=1)
    varied = [i for i, k in enumerate(sdesign.names) if k not in fixed]
    n_base = 1_428_572
    t_salt = {}
    for precision in ('fp64', 'fp32'):
        launches = {f'{precision} model, {m:5s} design': (lambda m=m: saltelli_sums(sdesign, varied, n_base, precision=precision, method=m))
                    for m in ('mc', 'sobol')}
        t_salt.update(interleaved(launches, a.repeats, a.warmup))

    def row(k, t):
        return f'  {k:54s} {np.median(t):9.1f}  [{min(t):.1f}, {max(t):.1f}]'
    lines = [f"Sobol' design kernels against their Monte-Carlo twins on one MI355X ({torch.cuda.get_device_name(0)}), python tools/qmc_probe.py",
             f'One launch between two HIP events; the variants of a group alternate launch by launch; {a.repeats} launches each after '
             f'{a.warmup} warm-up rounds.',
             'us per launch: median [min, max]', '',
             f'1. the design alone: 15 PEM-v0 priors x {n} samples, [15][n] fp64 written ({15 * n * 8 / 1e9:.2f} GB)']
    lines += [row(k, t) for k, t in t_fill.items()]
    lines += ['', f'2. the fused Saltelli launch: {n_base} base samples x {len(varied) + 2} = {n_base * (len(varied) + 2):.3g} evaluations '
                  f'(saltelli_sums: one launch and the sum of its partials)']
    lines += [row(k, t) for k, t in t_salt.items()]
    med = lambda d, k: float(np.median(d[k]))                                                     # noqa: E731
    keys = list(t_fill)
    lines += ['', f'  sobol / mc (medians): design {med(t_fill, keys[1]) / med(t_fill, keys[0]):.2f}; '
                  + '; '.join(f"fused {p} {med(t_salt, f'{p} model, sobol design') / med(t_salt, f'{p} model, mc    design'):.2f}"
                              for p in ('fp64', 'fp32'))]
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median_us': float(np.median(t)), 'us': t} for k, t in {**t_fill, **t_salt}.items()}))


if __name__ == '__main__':
    main()
