#!/usr/bin/env python3
"""Time the chain + likelihood launch (`pem_chain_system_loglik_f64_dev`) against the composition it replaces
(`pem_sparse_predict_chain_f64_dev` with the 91-point field written, then `pem_jion_loglik_f64_dev`), interleaved with device
events after a warm-up past the clock ramp, on the configs[3] box of tools/chain_probe.py with a j_ion-only
table of 8 conditions x 40 angles (the 'Plume' component), at 5e5 points and at one calibration-sized batch.

    python tools/surrogate_posterior_probe.py [--iters 200] [--reps 20] [--rounds 5] [--out FILE]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6, 'a_1': 0.01, 'sigma_cex': 55e-20, 'c4': 1e20, 'c5': 1e16}
VARIED = ('T_e', 'V_vac', 'Pstar', 'P_T', 'c0', 'c1', 'c2', 'c3')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='+', default=[500_000, 30_000])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from hallthrusterpem_amd.chain import ChainedSurrogate
    from hallthrusterpem_amd.likelihood import JionLikelihood, SystemLikelihood
    lines = []

    def say(*x):
        s = ' '.join(str(v) for v in x)
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    s = ChainedSurrogate(VARIED, FIXED)
    for it in range(a.iters):
        s.refine_step(num_refine=1000, seed=it + 1)
    st, _ = s.stage_tables()
    say(f'chain: {a.iters} iterations in {time.perf_counter() - t0:.1f} s; stages n_beta {[g.n_beta for g in st]}, n_out {[g.n_out for g in st]}, '
        f'max_active {[g.max_active for g in st]}, max_level {[g.max_level for g in st]}; j_ion rank {s.compression.rank}')
    rng = np.random.default_rng(0)
    ne, na = 8, 40
    alpha = np.linspace(-1.5, 1.5, na)
    y, std = rng.lognormal(0.0, 1.0, (ne, na)), rng.uniform(0.3, 1.5, (ne, na))
    x = np.stack([np.full(ne, FIXED['P_b']), np.full(ne, FIXED['V_a']), np.full(ne, FIXED['mdot_a'])], 1)
    lik = SystemLikelihood({'jion': {'x': x, 'y': y, 'var_y': std ** 2, 'loc': np.stack([np.ones(na), alpha], 1)}}, qois='Plume')
    jl = JionLikelihood(np.broadcast_to(alpha, (ne, na)), y, std)
    say(f'table: {lik.n_cond} conditions, {lik.n_rec} records (each block padded to an odd count)')
    for n in a.sizes:
        g = torch.Generator(device='cuda')
        g.manual_seed(1)
        t = torch.rand((len(VARIED), n), dtype=torch.float64, device='cuda', generator=g) * 2 - 1
        ll = torch.empty(n, dtype=torch.float64, device='cuda')
        fused = lambda: s.run_system_loglik(t, lik, out=ll)                                   # noqa: E731
        comp = lambda: jl.per_sample(s.predict(t)[1])                                         # noqa: E731
        ref = comp()
        fused()
        torch.cuda.synchronize()
        say(f'\nn = {n}: max |fused - composition| / |composition| = {float(((ll - ref).abs() / ref.abs()).max()):.2e}')
        variants = {'fused': fused, 'composition': comp}
        end = time.perf_counter() + 3.0                                                       # past the clock ramp
        while time.perf_counter() < end:
            for f in variants.values():
                f()
            torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, f in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.reps)
        say(f'  {a.rounds} interleaved rounds x {a.reps} calls, device events; ms per call: median [min, max]')
        for k, v in ms.items():
            say(f'  {k:12s} {np.median(v):8.4f}  [{min(v):.4f}, {max(v):.4f}]  spread {100 * (max(v) - min(v)) / np.median(v):.2f} %')
        say(f'  fused / composition = {np.median(ms["fused"]) / np.median(ms["composition"]):.4f}')
    say(f'device: {torch.cuda.get_device_name()}')
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    sys.exit(main())
