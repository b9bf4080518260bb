#!/usr/bin/env python3
"""What information.InformationGain costs on the `System` table of the README's DRAM row (needs the GPU).

Workload: the `System` table of tools/dram_step_probe.py (16 conditions, 348 records of which 340 are measured), draws from the
prior, 4096 outer x 4096 inner draws, by='condition' (16 groups and their union).  Alternating in one process, `--repeats` times:

  the pairwise launches alone    device events around `--launches` calls of pem_pairwise_lse_f64_dev (partial + merge) on the
                                 standardised values of a run
  a whole run                    InformationGain.run: 2 x (inputs, predictions, gather), the noise, the filter, the pairwise launches
                                 and the statistics; host clock around a device synchronise
  the same numbers composed      per group torch.cdist(zo[:, c], zi[:, c]) ** 2 through the matrix product (compute_mode=
                                 'use_mm_for_euclid_dist': cdist's own direct kernel refuses a 4096 x 4096 launch, "invalid
                                 configuration argument", which is what its default picks for groups of up to 25 columns), and once
                                 with the direct form (a - b)^2 accumulated column by column in torch; then logsumexp over the inner
                                 draws and the sums for ess; the union from the running sum of the groups' matrices

with the peak of the allocator over each and the largest difference between the composed lse and the launch's.

    python tools/information_probe.py [--repeats 3] [--out profiles/information_r01.txt]
"""
import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
from dram_step_probe import system_table                                                        # noqa: E402
from hallthrusterpem_amd import _lib                                                            # noqa: E402
from hallthrusterpem_amd.information import InformationGain                                     # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                           # noqa: E402

NAMES = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')


class Launch:
    """pem_pairwise_lse_f64_dev on fixed operands with its outputs and workspace allocated once"""

    def __init__(self, z_out, z_in, ge):
        self.lib = _lib.load()
        self.z_out, self.z_in, self.ge = z_out, z_in, np.ascontiguousarray(ge, dtype=np.int32)
        n, m = z_out.shape[0], z_in.shape[0]
        self.lse = torch.empty((n, self.ge.size + 1), dtype=torch.float64, device=z_out.device)
        self.ess = torch.empty_like(self.lse)
        self.work = torch.empty(int(self.lib.pem_pairwise_lse_work_len(n, m, self.ge.size)), dtype=torch.float64, device=z_out.device)

    def __call__(self):
        p = lambda t: C.c_void_p(t.data_ptr())                                                  # noqa: E731
        zo, zi = self.z_out, self.z_in
        _lib.check(self.lib.pem_pairwise_lse_f64_dev(zo.shape[0], zi.shape[0], zo.shape[1], p(zo), zo.stride(0), p(zi), zi.stride(0),
                                                     self.ge.size, C.c_void_p(self.ge.ctypes.data), p(self.lse), p(self.ess),
                                                     p(self.work), self.work.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def events_us(self, launches):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(launches):
            self()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / launches


def composed(z_out, z_in, ge, mode):
    """(lse, ess) of every group and the union from torch.cdist, logsumexp and sums"""
    log_m = math.log(z_in.shape[0])
    lse, ess, total = [], [], None

    def stats(d2):
        l = -0.5 * d2
        a = torch.logsumexp(l, dim=1)
        lse.append(a - log_m)
        ess.append(torch.exp(2.0 * a - torch.logsumexp(2.0 * l, dim=1)))

    for a, b in zip([0] + ge[:-1].tolist(), ge.tolist()):
        if mode == 'mm':
            d2 = torch.cdist(z_out[:, a:b], z_in[:, a:b], compute_mode='use_mm_for_euclid_dist') ** 2
        else:
            d2 = torch.zeros((z_out.shape[0], z_in.shape[0]), dtype=torch.float64, device=z_out.device)
            for k in range(a, b):
                d = z_out[:, k:k + 1] - z_in[:, k].unsqueeze(0)
                d2.addcmul_(d, d)
        total = d2.clone() if total is None else total.add_(d2)
        stats(d2)
    stats(total)
    return torch.stack(lse, dim=1), torch.stack(ess, dim=1)


def timed_ms(f):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--draws', type=int, default=4096)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'information_r01.txt'))
    a = ap.parse_args()
    lik = system_table()
    assert lik.n_cond == 16 and lik.n_rec == 348
    ig = InformationGain(Predictive(lik, NAMES, seed=3))
    run = lambda by: ig.run(samples=None, n_outer=a.draws, n_inner=a.draws, by=by, keep=True)     # noqa: E731
    res = run('condition')
    z_out, z_in, ge = res['z_outer'], res['z_inner'], res['group_end']
    n, m, k = z_out.shape[0], z_in.shape[0], z_out.shape[1]
    launch = Launch(z_out, z_in, ge)
    modes = {'torch.cdist through the matrix product': 'mm', 'direct form, a column at a time': 'direct'}
    for _ in range(2):                                                   # warm every shape of the timed windows
        launch()
        run('condition')
        for mode in modes.values():
            composed(z_out, z_in, ge, mode)
    torch.cuda.synchronize()
    times, peaks, diff = {}, {}, {}
    add = lambda d, key, v: d.setdefault(key, []).append(v)                                          # noqa: E731
    for _ in range(a.repeats):
        add(times, 'pem_pairwise_lse_f64_dev alone, device events (ms)', launch.events_us(a.launches) / 1e3)
        t, peak, _ = timed_ms(lambda: run('condition'))
        add(times, "InformationGain.run(by='condition'), host clock (ms)", t)
        add(peaks, "InformationGain.run(by='condition'), host clock (ms)", peak)
        for label, mode in modes.items():
            t, peak, (lse, ess) = timed_ms(lambda: composed(z_out, z_in, ge, mode))
            add(times, f'composed, {label} (ms)', t)
            add(peaks, f'composed, {label} (ms)', peak)
            diff[label] = (float((lse - launch.lse).abs().max()), float(((ess - launch.ess).abs() / launch.ess).max()))
    pair_cols = float(n) * m * k
    t_kernel = float(np.median(times['pem_pairwise_lse_f64_dev alone, device events (ms)'])) * 1e-3
    lines = [f'InformationGain on one MI355X ({torch.cuda.get_device_name(0)}), python tools/information_probe.py, {time.strftime("%Y-%m-%d")}',
             f'Workload: System table of {lik.n_cond} conditions, {lik.n_rec} records ({k} measured); draws from the prior, {n} outer x {m} inner '
             f'({res["dropped"]} dropped of {a.draws} + {a.draws}); by=\'condition\': {ge.size} groups and their union.',
             f'The measurements alternate, {a.repeats} repeats each: median [min, max], repeats; the launches alone are the mean of '
             f'{a.launches} back-to-back calls per repeat.', '']
    for key, t in times.items():
        lines.append(f'  {key:64s} {np.median(t):10.3f}  [{min(t):.3f}, {max(t):.3f}]   ' + ' '.join(f'{v:.3f}' for v in t)
                     + (f'   allocator peak {max(peaks[key]):.0f} MiB' if key in peaks else ''))
    lines += ['', f'  the launches: {pair_cols:.3g} pair-columns (one subtraction and one fma each) and {float(n) * m * (ge.size + 1):.3g} '
                  f'exponentials in {t_kernel * 1e3:.3f} ms: {pair_cols / t_kernel / 1e12:.2f} T pair-columns/s; workspace '
                  f'{launch.work.numel() * 8 / 2 ** 20:.1f} MiB, no {n} x {m} matrix ({n * m * 8 / 2 ** 20:.0f} MiB each, '
                  f'{(ge.size + 1) * n * m * 8 / 2 ** 20:.0f} MiB for all sets)']
    for label, (d_lse, d_ess) in diff.items():
        lines.append(f'  composed, {label}: max |lse - launch| {d_lse:.3g}, max relative ess difference {d_ess:.3g}')
    eig, se, med = (res[key].cpu().numpy() for key in ('eig', 'stderr', 'ess_median'))
    lines += ['', '  the estimate of that run (nats; log M = %.3f):' % res['log_M']]
    lines += [f'    {str(lab):>10s}  EIG {eig[c]:8.3f} +- {se[c]:.3f}   median ess {med[c]:8.1f}' for c, lab in enumerate(res['labels'])]
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({key: {'median': float(np.median(t)), 'repeats': t} for key, t in times.items()}))


if __name__ == '__main__':
    main()
