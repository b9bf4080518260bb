#!/usr/bin/env python3
"""MCMC chain diagnostics at three sizes: the autocovariance launch sequence (pem_chain_autocov_f64_dev: means, lag partials,
reduction) timed warm with HIP events, its fp64 FMA rate against the 78.6 TF/s vendor figure, the wall time of summary(),
and, for comparison, numpy's FFT autocovariance on the host and torch.fft on the device with its transposing copy;
`profiles/chain_diagnostics_r01.txt`.

    python tools/chain_diag_probe.py [out.txt]

(a) K = 16, d = 3, n' = 1.8e4, maxlag 500, step 20 (show_mcmc's call at the example's size); (b) K = 64, d = 17, n' = 2e4,
lags 0..999; (c) K = 1024, d = 17, n' = 1e4, lags 0..999.  The draws are AR(1) series with phi = 0.95
(IAC 39).  Useful FMAs: n_series * sum_{l<L} (N - l).
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from hallthrusterpem_amd import diagnostics  # noqa: E402

PEAK = 78.6e12
CASES = [('a', 16, 3, 18_000, 500), ('b', 64, 17, 20_000, 1000), ('c', 1024, 17, 10_000, 1000)]


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


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else None
    lines = [f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}']
    rng = np.random.default_rng(0)
    for tag, K, d, n, L in CASES:
        S = K * d
        xh = rng.standard_normal((n, S))                          # AR(1), phi = 0.95: IAC 39, a slowly mixing DRAM chain
        for t in range(1, n):
            xh[t] += 0.95 * xh[t - 1]
        x = torch.as_tensor(xh, device='cuda')
        fma = S * (L * n - L * (L - 1) / 2)
        t_k = events(lambda: diagnostics.autocovariance(x, L), 10 if tag != 'c' else 3)
        trace = x.reshape(n, K, d)
        t_sum = wall(lambda: diagnostics.summary(trace, burnin=0.0))
        t_ac = wall(lambda: diagnostics.autocorrelation(trace, maxlag=L, step=20))
        m = 1 << int(np.ceil(np.log2(2 * n)))

        def torch_fft():
            y = (x - x.mean(0)).T.contiguous()                      # the transposing copy: series contiguous
            f = torch.fft.rfft(y, m, dim=1)
            return torch.fft.irfft(f * f.conj(), m, dim=1)[:, :L] / n
        t_tf = wall(torch_fft)
        cols = S if S <= 1088 else 1088
        t0 = time.perf_counter()
        y = xh[:, :cols] - xh[:, :cols].mean(0)
        f = np.fft.rfft(y, m, axis=0)
        np.fft.irfft(f * np.conj(f), m, axis=0)[:L]
        t_np = (time.perf_counter() - t0) * S / cols
        lines.append(f'({tag}) K={K} d={d} n\'={n} lags 0..{L - 1}: {S} series, {fma:.3e} useful FMAs, trace {8 * n * S / 1e6:.0f} MB')
        lines.append(f'    autocovariance launch sequence (HIP events, warm): {1e3 * t_k:.3f} ms = {2 * fma / t_k / 1e12:.1f} TF/s fp64 '
                     f'= {100 * 2 * fma / t_k / PEAK:.0f} % of 78.6 TF/s')
        lines.append(f'    summary() wall {1e3 * t_sum:.2f} ms; autocorrelation(maxlag={L}, step=20) wall {1e3 * t_ac:.2f} ms')
        lines.append(f'    torch.fft on the device incl. transposing copy {1e3 * t_tf:.2f} ms; numpy FFT on the host '
                     f'{1e3 * t_np:.0f} ms' + ('' if cols == S else f' (timed on {cols} series, scaled)'))
        del x, trace
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if out:
        out.write_text(text + '\n')


if __name__ == '__main__':
    main()
