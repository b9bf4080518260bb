#!/usr/bin/env python3
"""Corner-plot marginals at the three sizes of profiles/chain_diagnostics_r01.txt: the histogram launch (pem_chain_hist_f64_dev,
bins = 15) timed warm with HIP events beside the obvious torch formulation on the device (torch.bucketize per column,
torch.bincount of ki * bins + kj per pair; three interleaved pairs of timings, HIP events and the same repetition count on
both sides) and one plain read of the trace; the density
launch sequence (pem_chain_kde_f64_dev, 256 points) and its exp rate; scipy.stats.gaussian_kde and the np.histogram2d calls on
the host; the wall time of corner() for the three parameter groups of journal_plots; `profiles/marginals_r01.txt`.

    python tools/marginals_probe.py [out.txt]
    python tools/marginals_probe.py --kernel hist|kde      # one warm launch at the middle size, for a counter run

(a) K = 16, d = 3, n' = 1.8e4; (b) K = 64, d = 17, n' = 2e4; (c) K = 1024, d = 17, n' = 1e4.  The draws are a rejecting
sampler's: AR(1) rows with phi = 0.95, each repeated a geometric number of times (acceptance 0.3), so whole rows repeat.
Increments: d (d + 1) / 2 per row.  exp: n_rows * d * 256.  The fp64 vector rate is taken as the 78.6 TF/s vendor figure
with an FMA counted as two flops: 39.3e12 lane-instructions per second chip-wide.  One value costs EXP_INSTR = 25 fp64
arithmetic instructions in chain_kde_partial_kernel's inner loop (disassembly, gfx950, -O3: subtract, three multiplies, the
library exp's range reduction, degree-11 polynomial and v_ldexp_f64, two compares, the add), beside 9 v_mov_b64 and 3 selects
that are not counted.
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import marginals  # noqa: E402

LANE_INSTR_PER_S = 78.6e12 / 2
EXP_INSTR = 25            # fp64 arithmetic instructions per grid point and draw in the inner loop
CASES = [('a', 16, 3, 18_000), ('b', 64, 17, 20_000), ('c', 1024, 17, 10_000)]
GROUPS = {'cathode': [0, 1, 2], 'thruster': [3, 4, 5, 6, 7, 8, 9], 'plume': [10, 11, 12, 13, 14, 15, 16]}
BINS, POINTS = 15, 256


def make_trace(rng, K, d, n):
    """(n, K, d) float64 on the host: AR(1) proposals accepted with probability 0.3, the row repeated otherwise"""
    e = rng.standard_normal((n, K, d))
    acc = rng.random((n, K)) < 0.3
    x = np.empty_like(e)
    x[0] = e[0]
    cur = e[0].copy()
    for t in range(1, n):
        prop = 0.95 * cur + e[t]
        cur = np.where(acc[t][:, None], prop, cur)
        x[t] = cur
    return x * np.linspace(0.5, 3.0, d) + np.arange(d)


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def wall(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = np.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def torch_hist(pooled, edges_d, bins):
    """the obvious device formulation: bucketize per column, bincount per pair (values in the last bin's right edge and
    outside the range handled as the kernel does)"""
    m, d = pooled.shape
    ks = []
    for i in range(d):
        v = pooled[:, i].contiguous()
        k = torch.bucketize(v, edges_d[i], right=True) - 1
        k = torch.where(v == edges_d[i, -1], torch.full_like(k, bins - 1), k)
        ks.append(torch.where((k < 0) | (k >= bins), torch.full_like(k, -1), k))
    h1 = [torch.bincount(k[k >= 0], minlength=bins) for k in ks]
    h2 = []
    for i in range(d):
        for j in range(i + 1, d):
            ok = (ks[i] >= 0) & (ks[j] >= 0)
            h2.append(torch.bincount((ks[i] * bins + ks[j])[ok], minlength=bins * bins))
    return torch.stack(h1), (torch.stack(h2) if h2 else None)


def one_kernel(which):
    rng = np.random.default_rng(0)
    _, K, d, n = CASES[1]
    pooled = torch.as_tensor(make_trace(rng, K, d, n).reshape(-1, d), device='cuda')
    edges = marginals._edges(pooled, BINS, None)
    grid = np.stack([np.linspace(a, b, POINTS) for a, b in zip(edges[:, 0], edges[:, -1])])
    h, inv_h, scale = marginals._bandwidth(pooled, 'scott')
    for _ in range(2):
        if which == 'hist':
            marginals._hist_dev(pooled, edges, True)
        else:
            marginals._kde_dev(pooled, grid, inv_h, scale)
    torch.cuda.synchronize()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--kernel':
        return one_kernel(sys.argv[2])
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else None
    lines = [f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}']
    try:
        from scipy import stats
    except ImportError:
        stats = None
    rng = np.random.default_rng(0)
    for tag, K, d, n in CASES:
        xh = make_trace(rng, K, d, n)
        trace = torch.as_tensor(xh, device='cuda')
        pooled = trace.reshape(-1, d)
        m = pooled.shape[0]
        reps = 10 if tag != 'c' else 3
        edges = marginals._edges(pooled, BINS, None)
        edges_d = torch.as_tensor(edges, device='cuda')
        grid = np.stack([np.linspace(a, b, POINTS) for a, b in zip(edges[:, 0], edges[:, -1])])
        h, inv_h, scale = marginals._bandwidth(pooled, 'scott')
        inc = m * d * (d + 1) // 2
        n_exp = m * d * POINTS

        got = marginals._hist_dev(pooled, edges, True)
        want = torch_hist(pooled, edges_d, BINS)
        same = torch.equal(got[0], want[0]) and (want[1] is None or torch.equal(got[1].reshape(want[1].shape), want[1]))
        t_k, t_t = [], []
        for _ in range(3):                                           # interleaved pairs, both sides on the same clock
            t_k.append(events(lambda: marginals._hist_dev(pooled, edges, True), reps))
            t_t.append(events(lambda: torch_hist(pooled, edges_d, BINS), reps))
        t_read = events(lambda: pooled.sum(), reps)
        t_kde = events(lambda: marginals._kde_dev(pooled, grid, inv_h, scale), reps if tag != 'c' else 2)

        lines.append(f'({tag}) K={K} d={d} n\'={n}: {m} pooled draws, trace {8 * m * d / 1e6:.0f} MB, repeated rows '
                     f'{100 * float((xh[1:] == xh[:-1]).all(axis=2).mean()):.0f} %')
        lines.append(f'    histogram launch, bins {BINS} (HIP events, warm, 3 runs): ' + ' / '.join(f'{1e3 * t:.3f}' for t in t_k)
                     + f' ms = {inc / min(t_k) / 1e9:.1f} G increments/s; equal to the torch formulation: {same}')
        lines.append('    torch.bucketize + torch.bincount per pair on the device (HIP events, warm, same repetitions, interleaved with the above): '
                     + ' / '.join(f'{1e3 * t:.2f}' for t in t_t) + f' ms = {min(t_t) / min(t_k):.1f} x the kernel')
        lines.append(f'    one plain read of the trace (torch sum): {1e3 * t_read:.3f} ms')
        lines.append(f'    density launch sequence, {POINTS} points (HIP events, warm): {1e3 * t_kde:.3f} ms = {n_exp / t_kde / 1e12:.3f} T exp/s '
                     f'= {100 * n_exp * EXP_INSTR / t_kde / LANE_INSTR_PER_S:.0f} % of the fp64 vector rate at {EXP_INSTR} fp64 instructions per exp')
        if d == 17:
            names = [f'p{i}' for i in range(d)]
            for g, idx in GROUPS.items():
                t_c = wall(lambda: marginals.corner(trace, names=names, select=idx, burnin=0.0, bins=BINS, cmin=int(0.0015 * m)), 2)
                lines.append(f'    corner() of the {g} group ({len(idx)} parameters, burnin 0): wall {1e3 * t_c:.2f} ms')
        else:
            t_c = wall(lambda: marginals.corner(trace, burnin=0.0, bins=BINS, cmin=int(0.0015 * m)), 2)
            lines.append(f'    corner() of all {d} parameters (burnin 0): wall {1e3 * t_c:.2f} ms')
        # host yardsticks, on a subsample where the full size would take minutes
        sub = min(m, 20_000)
        xs = xh.reshape(-1, d)[:sub]
        if stats is not None:
            t0 = time.perf_counter()
            stats.gaussian_kde(xs[:, 0])(grid[0, :64])
            t_sp = (time.perf_counter() - t0) * (m / sub) * (POINTS / 64) * d
            lines.append(f'    scipy.stats.gaussian_kde on the host: {t_sp:.1f} s for the {d} diagonals (timed on {sub} draws x 64 points of one '
                         f'parameter, scaled by draws, points and parameters)')
        sub2 = min(m, 200_000)
        xs = xh.reshape(-1, d)[:sub2]
        t0 = time.perf_counter()
        for i in range(d):
            for j in range(i + 1, d):
                np.histogram2d(xs[:, i], xs[:, j], bins=BINS, range=[(edges[i, 0], edges[i, -1]), (edges[j, 0], edges[j, -1])])
        t_np = (time.perf_counter() - t0) * m / sub2
        lines.append(f'    {d * (d - 1) // 2} np.histogram2d calls on the host: {1e3 * t_np:.0f} ms'
                     + ('' if sub2 == m else f' (timed on {sub2} draws, scaled)'))
        del trace, pooled
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if out:
        out.write_text(text + '\n')


if __name__ == '__main__':
    main()
