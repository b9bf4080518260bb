#!/usr/bin/env python3
"""Hexagonal pair bins at the middle size of tools/marginals_probe.py (K = 64, d = 17, n' = 2e4: 1.28e6 pooled draws, 136 pairs,
the same rejecting sampler's trace): the hex launch (pem_chain_hex_f64_dev, gridsize 15 = 15 x 8) and the square launch
(pem_chain_hist_f64_dev, 15 bins: the same bytes read, 136 of its 153 tables are pair tables with one LDS add per pair and row)
on the same tensor, timed warm with HIP events in interleaved rounds of one process; the counts checked against matplotlib's
hexbin for three pairs; matplotlib's hexbin over the 136 pairs on the host, timed on a subsample and scaled by draws;
`profiles/hexbin_r01.txt`.

    python tools/hexbin_probe.py [out.txt]
    python tools/hexbin_probe.py --kernel          # two warm hex launches alone, for a counter run
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from hallthrusterpem_amd import marginals  # noqa: E402
from marginals_probe import events, make_trace  # noqa: E402

K, D, N = 64, 17, 20_000
GRIDSIZE, BINS, ROUNDS, REPS = 15, 15, 5, 20


def main():
    rng = np.random.default_rng(0)
    trace = make_trace(rng, K, D, N)
    repeated = float((trace[1:] == trace[:-1]).all(axis=2).mean())
    xh = trace.reshape(-1, D)
    pooled = torch.as_tensor(xh, device='cuda')
    m = pooled.shape[0]
    nx, ny = marginals._check_gridsize(GRIDSIZE, D)
    extent = marginals._hex_extent(pooled, None)
    table = marginals._hex_table(extent, nx, ny)
    edges = marginals._edges(pooled, BINS, None)
    hex_launch = lambda: marginals._hex_dev(pooled, nx, ny, table)          # noqa: E731
    hist_launch = lambda: marginals._hist_dev(pooled, edges, True)         # noqa: E731
    if len(sys.argv) > 1 and sys.argv[1] == '--kernel':
        for _ in range(2):
            hex_launch()
        torch.cuda.synchronize()
        return
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else None
    lines = [f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}',
             f'K={K} d={D} n\'={N}: {m} pooled draws, trace {8 * m * D / 1e6:.0f} MB, {D * (D - 1) // 2} pairs, repeated rows '
             f'{100 * repeated:.0f} %']
    counts = hex_launch().cpu().numpy()
    same = None
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots()
        pairs = [(i, j) for i in range(D) for j in range(i + 1, D)]
        same = all(np.array_equal(np.asarray(ax.hexbin(xh[:, i], xh[:, j], gridsize=(nx, ny), extent=(*extent[i], *extent[j])).get_array()),
                                  counts[pairs.index((i, j))]) for i, j in ((0, 1), (3, 11), (15, 16)))
    except ImportError:
        ax = None
    t_hex, t_hist = [], []
    for _ in range(ROUNDS):                                                 # interleaved rounds, both on the same clock
        t_hex.append(events(hex_launch, REPS))
        t_hist.append(events(hist_launch, REPS))
    inc = m * D * (D - 1) // 2
    fmt = lambda ts: ' / '.join(f'{1e3 * t:.3f}' for t in ts)               # noqa: E731
    lines.append(f'hex launch, gridsize {GRIDSIZE} = {nx} x {ny}, {counts.shape[1]} cells per pair (HIP events, warm, {REPS} launches per timing, '
                 f'{ROUNDS} rounds): {fmt(t_hex)} ms; median {1e3 * np.median(t_hex):.3f}, min {1e3 * min(t_hex):.3f} ms = '
                 f'{inc / min(t_hex) / 1e9:.1f} G pair increments/s; equal to matplotlib on three pairs: {same}')
    lines.append(f'square launch, bins {BINS}, 17 + 136 tables (same tensor, interleaved with the above): {fmt(t_hist)} ms; median '
                 f'{1e3 * np.median(t_hist):.3f}, min {1e3 * min(t_hist):.3f} ms; hex / square = {np.median(t_hex) / np.median(t_hist):.2f} (medians)')
    lines.append(f'draws in no cell of pair (0, 1): {m - int(counts[0].sum())}')
    if ax is not None:
        sub = min(m, 200_000)
        xs = xh[:sub]
        t0 = time.perf_counter()
        for i in range(D):
            for j in range(i + 1, D):
                ax.hexbin(xs[:, i], xs[:, j], gridsize=(nx, ny), extent=(*extent[i], *extent[j]))
        t_mpl = (time.perf_counter() - t0) * m / sub
        lines.append(f'{D * (D - 1) // 2} matplotlib hexbin calls on the host (the collection built, nothing drawn): {1e3 * t_mpl:.0f} ms '
                     f'(timed on {sub} draws, scaled by draws)')
    text = '\n'.join(lines)
    print(text)
    if out:
        out.write_text(text + '\n')


if __name__ == '__main__':
    main()
