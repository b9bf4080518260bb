#!/usr/bin/env python3
"""What the gain about theta alone (information.InformationGain.run(about=theta)) costs on the `System` table of the README's DRAM
row (needs the GPU).

Workload: the `System` table of tools/dram_step_probe.py (16 conditions, 348 records of which 340 are measured), draws from the
prior, 4096 outer x 4096 inner draws, L = 128 vectors per outer draw, by='condition' (16 groups and their union), about = the six
calibrated inputs.  Alternating in one process, `--repeats` times:

  the conditional launch alone   device events around `--launches` calls of pem_conditional_lse_f64_dev on the raw predictions of
                                 ALL conditional sets, (n_outer L, 348) doubles in one tensor, with the bytes of that tensor over the
                                 time beside the 8 TB/s of the HBM
  the same numbers composed      index_select of the measured records, multiply by 1 / std, broadcast subtract of the observations,
                                 square, per-group sums, logsumexp over the L rows and the sums for ess; the union from the sum of
                                 the groups' sums -- on the same tensor
  a whole run                    InformationGain.run(about=theta): the joint estimate (2 x inputs, predictions, gather, the noise,
                                 the pairwise launches) and per chunk of 512 outer draws inputs, predictions and the launch; host
                                 clock around a device synchronise, and the same run without `about` beside it

with the peak of the allocator over each and the largest difference between the composed numbers and the launch's.

    python tools/information_theta_probe.py [--repeats 3] [--out profiles/information_theta_r01.txt]
"""
import argparse
import ctypes as C
import json
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
from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS                                   # noqa: E402
from hallthrusterpem_amd.predictive import Predictive                                           # noqa: E402
from information_probe import timed_ms                                                          # noqa: E402

NAMES = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')
HBM_TBS = 8.0


class Launch:
    """pem_conditional_lse_f64_dev on fixed operands with its outputs allocated once"""

    def __init__(self, z_out, raw, n_per, ge, col, scale):
        self.lib = _lib.load()
        self.z_out, self.raw, self.n_per, self.ge = z_out, raw, n_per, np.ascontiguousarray(ge, dtype=np.int32)
        self.col, self.scale = col.to(torch.int32).contiguous(), scale.contiguous()
        n = z_out.shape[0]
        self.lse = torch.empty((n, self.ge.size + 1), dtype=torch.float64, device=z_out.device)
        self.ess = torch.empty_like(self.lse)
        self.used = torch.empty(n, dtype=torch.int32, device=z_out.device)

    def __call__(self):
        p = lambda t: C.c_void_p(t.data_ptr())                                                  # noqa: E731
        zo, raw = self.z_out, self.raw
        _lib.check(self.lib.pem_conditional_lse_f64_dev(zo.shape[0], self.n_per, zo.shape[1], p(zo), zo.stride(0), p(raw), raw.stride(0),
                                                        p(self.col), p(self.scale), self.ge.size, C.c_void_p(self.ge.ctypes.data),
                                                        p(self.lse), p(self.ess), p(self.used),
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def events_ms(self, launches):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(launches):
            self()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / launches


def composed(z_out, raw, n_per, ge, col, scale):
    """(lse, ess) of every group and the union from index_select, multiply, broadcast subtract, per-group sums and logsumexp"""
    n, k = z_out.shape
    z = (raw.index_select(1, col) * scale).view(n, n_per, k)
    d = z_out.unsqueeze(1) - z
    d = d * d
    lse, ess, total = [], [], None

    def stats(d2):
        l = -0.5 * d2
        a = torch.logsumexp(l, dim=1)
        lse.append(a - np.log(n_per))
        ess.append(torch.exp(2.0 * a - torch.logsumexp(2.0 * l, dim=1)))

    for a, b in zip([0] + ge[:-1].tolist(), ge.tolist()):
        d2 = d[:, :, a:b].sum(dim=2)
        total = d2.clone() if total is None else total.add_(d2)
        stats(d2)
    stats(total)
    return torch.stack(lse, dim=1), torch.stack(ess, dim=1)


def conditional_predictions(ig, res, n_draws, n_per, chunk):
    """the raw predictions of every outer draw's conditional set as `InformationGain._conditional` makes them, in one tensor"""
    pp, nc = ig.pred, ig.pred.lik.n_cond
    rows = torch.as_tensor([COUPLED_INPUTS.index(k) for k in NAMES], device=pp.device)
    outer = ig.assemble_shared(None, n_draws, 0)[:, :n_draws * nc:nc].clone()
    raw = torch.empty((n_draws * n_per, pp.lik.n_rec), dtype=torch.float64, device=pp.device)
    for d0 in range(0, n_draws, chunk):
        x = ig.assemble_shared(None, chunk * n_per, (2 * n_draws + d0 * n_per) * nc)
        v = x[:, :chunk * n_per * nc].view(x.shape[0], chunk, n_per * nc)
        v[rows] = outer[rows, d0:d0 + chunk, None]
        pp.predict(chunk * n_per, out=raw[d0 * n_per:(d0 + chunk) * n_per])
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--draws', type=int, default=4096)
    ap.add_argument('--conditional', type=int, default=128)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'information_theta_r01.txt'))
    a = ap.parse_args()
    lik = system_table()
    assert lik.n_cond == 16 and lik.n_rec == 348
    ig = InformationGain(Predictive(lik, NAMES, seed=3))
    n_per = a.conditional
    chunk = max(1, 2 ** 20 // (n_per * lik.n_cond))
    assert a.draws % chunk == 0
    run = lambda about: ig.run(samples=None, n_outer=a.draws, n_inner=a.draws, by='condition', about=about,     # noqa: E731
                               n_conditional=n_per)
    res = ig.run(samples=None, n_outer=a.draws, n_inner=a.draws, by='condition', about=NAMES, n_conditional=n_per, keep=True)
    assert res['dropped'][0] == 0, 'the probe takes every outer draw'
    ge = res['group_end']
    perm = torch.as_tensor(res['perm'], device=ig.pred.device)
    col, scale = ig.pred.cols.index_select(0, perm), ig.inv_std.index_select(0, perm)
    z_out = res['z_outer']
    raw = conditional_predictions(ig, res, a.draws, n_per, chunk)
    launch = Launch(z_out, raw, n_per, ge, col, scale)
    launch()
    assert torch.equal(launch.lse, res['lse_cond']) and torch.equal(launch.ess, res['ess_cond'])      # one launch = the run's chunks
    del res['z_cond']
    for _ in range(2):                                                   # warm every shape of the timed windows
        launch()
        run(NAMES)
        run(None)
        composed(z_out, raw, n_per, ge, col, scale)
    torch.cuda.synchronize()
    times, peaks = {}, {}
    add = lambda d, key, v: d.setdefault(key, []).append(v)                                          # noqa: E731
    keys = ('pem_conditional_lse_f64_dev alone, device events (ms)', 'composed in torch, host clock (ms)',
            'InformationGain.run(about=theta), host clock (ms)', 'InformationGain.run(about=None), host clock (ms)')
    for _ in range(a.repeats):
        add(times, keys[0], launch.events_ms(a.launches))
        t, peak, (lse, ess) = timed_ms(lambda: composed(z_out, raw, n_per, ge, col, scale))
        add(times, keys[1], t)
        add(peaks, keys[1], peak)
        diff = (float((lse - launch.lse).abs().max()), float(((ess - launch.ess).abs() / launch.ess).max()))
        del lse, ess
        for key, about in ((keys[2], NAMES), (keys[3], None)):
            t, peak, _ = timed_ms(lambda: run(about))
            add(times, key, t)
            add(peaks, key, peak)
    nbytes = float(raw.numel()) * 8
    t_kernel = float(np.median(times[keys[0]])) * 1e-3
    n, k = z_out.shape
    lines = [f'InformationGain about theta on one MI355X ({torch.cuda.get_device_name(0)}), python tools/information_theta_probe.py, '
             f'{time.strftime("%Y-%m-%d")}',
             f'Workload: System table of {lik.n_cond} conditions, {lik.n_rec} records ({k} measured); draws from the prior, {n} outer x '
             f'{res["n_inner"]} inner ({res["dropped"]} dropped), L = {n_per} vectors per outer draw ({res["dropped_conditional"]} outer draws '
             f'without a used row, fewest used rows {res["used_min"]}); by=\'condition\': {ge.size} groups and their union; about = {NAMES}.',
             f'The measurements alternate, {a.repeats} repeats each: median [min, max], repeats; the launch alone is the mean of '
             f'{a.launches} back-to-back calls per repeat on all {n} x {n_per} rows at once; a run launches {a.draws // chunk} chunks of '
             f'{chunk} outer draws.', '']
    for key in keys:
        t = times[key]
        lines.append(f'  {key:64s} {np.median(t):10.3f}  [{min(t):.3f}, {max(t):.3f}]   ' + ' '.join(f'{v:.3f}' for v in t)
                     + (f'   allocator peak {max(peaks[key]):.0f} MiB' if key in peaks else ''))
    lines += ['', f'  the launch: a streaming read of {nbytes / 2 ** 30:.2f} GiB ({n} x {n_per} x {lik.n_rec} doubles) in {t_kernel * 1e3:.3f} ms: '
                  f'{nbytes / t_kernel / 1e12:.2f} TB/s of {HBM_TBS:.0f} TB/s; it allocates {(launch.lse.numel() * 16 + n * 4) / 2 ** 20:.1f} MiB '
                  f'(lse, ess, used) and no gathered or scaled tensor ({n * n_per * k * 8 / 2 ** 20:.0f} MiB each)',
              f'  composed: max |lse - launch| {diff[0]:.3g}, max relative ess difference {diff[1]:.3g}',
              f'  composed / launch: {np.median(times[keys[1]]) / np.median(times[keys[0]]):.1f} x']
    ea, sa, er, sr, eig, se, med = (res[key].cpu().numpy() for key in ('eig_about', 'stderr_about', 'eig_rest', 'stderr_rest', 'eig',
                                                                      'stderr', 'ess_cond_median'))
    lines += ['', '  the estimate of that run (nats):']
    lines += [f'    {str(lab):>10s}  EIG {eig[c]:8.3f} +- {se[c]:.3f}   about theta {ea[c]:8.3f} +- {sa[c]:.3f}   rest {er[c]:8.3f} +- {sr[c]:.3f}'
              f'   median ess_cond {med[c]:6.1f}' for c, lab in enumerate(res['labels'])]
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({key: {'median': float(np.median(t)), 'repeats': t} for key, t in times.items()}))


if __name__ == '__main__':
    main()
