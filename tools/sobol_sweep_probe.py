#!/usr/bin/env python3
"""Wall time of the whole Sobol' study over the pressure sweep (drivers.sobol_sweep: the group launches, the Plume pre-pass and
its percentile), N base samples per pressure, the five default pressures, all four QoIs.

    python tools/sobol_sweep_probe.py [--n 1000000] [--reps 10]
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    import numpy as np
    import torch

    from hallthrusterpem_amd import drivers
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    drivers.sobol_sweep(4096, seed=args.seed)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = drivers.sobol_sweep(args.n, seed=args.seed)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = np.array(times) * 1e3
    print(f'N = {args.n} per pressure x {res["P_b"].size} pressures, QoIs V_cc T uion jion: {res["evaluations"]:.3e} evaluations')
    print(f'driver call: median {np.median(t):.2f} ms, min {t.min():.2f} ms, max {t.max():.2f} ms over {args.reps} calls '
          f'({res["evaluations"] / (np.median(t) * 1e-3):.3g} evaluations/s)')
    print(f'rejected draws per pressure {res["jion"]["rejected"].tolist()}, clip thresholds {res["jion"]["clip"].cpu().numpy().tolist()}')
    print(f'non_physical {res["non_physical"]}, invalid {res["invalid"]}')
    for q in ('V_cc', 'T', 'uion', 'jion'):
        r = res[q]
        print(q, 'inputs', list(r['inputs']))
        for p, pb in enumerate(res['P_b']):
            print(f'  P_b {pb:.3e}  S1 ' + ' '.join(f'{v:+.4f}' for v in r['S1'][p].tolist()) +
                  '  ST ' + ' '.join(f'{v:+.4f}' for v in r['ST'][p].tolist()))


if __name__ == '__main__':
    main()
