#!/usr/bin/env python3
"""What a noise scale per measured quantity costs in a posterior evaluation (needs the GPU).

Workload: the `System` table of the README (tools/dram_step_probe.py: 16 conditions, 348 records), K = 128 chains, M = 50 nuisance
draws, six calibrated inputs; with scales: one per quantity and one for the discharge term (theta has 11 columns).  Alternating in
one process, `--repeats` times:

  the marginal launches alone   `--launches` calls on the per-sample sums of one evaluation recorded into one hipGraph (a chain on
                                one stream: no enqueue cost, every launch waits for the one before), device events around a
                                replay: pem_loglik_marginal_f64_dev, pem_loglik_marginal_scaled_f64_dev without and with ess / chi
  a posterior evaluation        one graph replay of `capture()` without and with noise_scales, host clock around `--replays`
                                replays and a device synchronise

The unscaled launch is the yardstick; the spread is max - min over the repeats.

    python tools/noise_scale_probe.py [--repeats 5] [--out profiles/noise_scale_r01.txt]
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
from hallthrusterpem_amd._device_loop import capture_graph                                      # noqa: E402
from hallthrusterpem_amd.calibration import SystemPosterior                                     # noqa: E402
from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS                                   # noqa: E402

NAMES = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')
THETA0 = (3.0, 30.0, 5e-5, 0.03, 0.5, 0.9)
SCALES = ('V_cc', 'T', 'uion', 'jion', 'I_D')


def chain(call, launches, device):
    """`launches` calls of `call` as one recorded graph"""
    def body():
        for _ in range(launches):
            call()
    return capture_graph(body, device)[0]


def events_us(graph, launches):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    graph.replay()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / launches


def replay_us(replay, theta, replays):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        replay(theta)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / replays * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'noise_scale_r01.txt'))
    a = ap.parse_args()
    lik = system_table()
    assert lik.n_cond == 16 and lik.n_rec == 348
    K, M = 128, 50
    mk = lambda **kw: SystemPosterior(NAMES, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False, **kw)   # noqa: E731
    plain, scaled = mk(), mk(noise_scales=SCALES)
    dev = plain.device
    rng = np.random.default_rng(0)
    th = np.asarray(THETA0) * (1 + 0.01 * rng.standard_normal((K, len(NAMES))))
    theta = torch.as_tensor(th, device=dev)
    theta_s = torch.cat([theta, torch.as_tensor(rng.uniform(0.5, 2.0, (K, len(SCALES))), device=dev)], dim=1).contiguous()
    lp, lp_s = plain.log_prior(theta).clone(), scaled.log_prior(theta_s).clone()
    ref = plain.log_posterior(theta).clone()
    ones = torch.cat([theta, torch.ones((K, len(SCALES)), dtype=torch.float64, device=dev)], dim=1).contiguous()
    same = bool((scaled.log_likelihood(ones) == plain.log_likelihood(theta)).all())                  # the scale-1 contract, here too
    scaled.log_posterior(theta_s)

    lib = _lib.load()
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)                        # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                               # noqa: E731
    hp = lambda arr: C.c_void_p(arr.ctypes.data)                                                    # noqa: E731
    d = plain.discharge
    out = torch.empty(K, dtype=torch.float64, device=dev)
    ess, chi = torch.empty_like(out), torch.empty((K, 5), dtype=torch.float64, device=dev)

    def common(post):
        x = post.batch.inputs
        return (K, M, post.Ne, p(post.loglik), p(x[COUPLED_INPUTS.index('mdot_a')]), p(x[COUPLED_INPUTS.index('a_1')]), d[0], d[1])

    def scaled_call(e, c):
        return lambda: _lib.check(lib.pem_loglik_marginal_scaled_f64_dev(
            *common(scaled), p(lp_s), 4, hp(scaled._group_end), hp(scaled._group_count), p(theta_s), theta_s.shape[1], theta_s.stride(0),
            hp(scaled._scale_col), scaled._discharge_col, p(e), p(c), 5, p(out), stream()))
    calls = {'pem_loglik_marginal_f64_dev': lambda: _lib.check(lib.pem_loglik_marginal_f64_dev(*common(plain), p(lp), p(out), stream())),
             'pem_loglik_marginal_scaled_f64_dev': scaled_call(None, None),
             'pem_loglik_marginal_scaled_f64_dev with ess and chi': scaled_call(ess, chi)}
    replays = {'log_posterior replay, noise_scales=None': (plain.capture(), theta),
               'log_posterior replay, noise_scales on': (scaled.capture(), theta_s)}
    calls = {k: chain(call, a.launches, dev) for k, call in calls.items()}
    for _ in range(3):                                                   # warm every shape of the timed windows
        for call in calls.values():
            events_us(call, a.launches)
        for r, t in replays.values():
            replay_us(r, t, 20)
    times = {k: [] for k in list(calls) + list(replays)}
    for _ in range(a.repeats):
        for k, call in calls.items():
            times[k].append(events_us(call, a.launches))
        for k, (r, t) in replays.items():
            times[k].append(replay_us(r, t, a.replays))
    unchanged = bool((replays['log_posterior replay, noise_scales=None'][0](theta) == ref).all())
    n = K * M * lik.n_cond
    lines = [f'Noise scales on one MI355X ({torch.cuda.get_device_name(0)}), python tools/noise_scale_probe.py, {time.strftime("%Y-%m-%d")}',
             f'Workload: System table of {lik.n_cond} conditions, {lik.n_rec} records; K = {K} chains x M = {M} draws x {lik.n_cond} conditions = '
             f'{n} per-sample sums ({n * 8 / 1024:.0f} KiB, {3 * n * 8 / 1024:.0f} KiB with the discharge inputs); scales: {", ".join(SCALES)}.',
             f'The measurements alternate, {a.repeats} repeats each: median [min, max] in us; a launch figure is the mean over a recorded '
             f'chain of {a.launches} calls between two device events (the launch and the gap to the next graph node), a replay figure '
             f'the mean of {a.replays} graph replays on the host clock.', '']
    for k, t in times.items():
        lines.append(f'  {k:56s} {np.median(t):9.2f}  [{min(t):.2f}, {max(t):.2f}]   ' + ' '.join(f'{v:.2f}' for v in t))
    base, new = times['pem_loglik_marginal_f64_dev'], times['pem_loglik_marginal_scaled_f64_dev']
    rb, rn = times['log_posterior replay, noise_scales=None'], times['log_posterior replay, noise_scales on']
    lines += ['', f'  scaled - unscaled launch: {np.median(new) - np.median(base):+.2f} us (spread of the unscaled launch {max(base) - min(base):.2f} us, '
                  f'of the scaled one {max(new) - min(new):.2f} us)',
              f'  replay with - without scales: {np.median(rn) - np.median(rb):+.2f} us (spreads {max(rb) - min(rb):.2f} / {max(rn) - min(rn):.2f} us)',
              f'  at scale 1 the scaled posterior gives the unscaled bits: {same}; the unscaled replay gives log_posterior\'s bits: {unchanged}']
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median': float(np.median(t)), 'repeats': t} for k, t in times.items()}))


if __name__ == '__main__':
    main()
