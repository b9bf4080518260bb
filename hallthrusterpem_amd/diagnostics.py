"""MCMC chain diagnostics: autocorrelation, integrated autocorrelation time (IAC), effective sample size (ESS), split R-hat.

The last step of scripts/pem_v0/mcmc.py: `show_mcmc` (mcmc.py:299-313) drops 10 % of the trace as burn-in, calls
`uq.autocorrelation(samples, step=20, maxlag=500)` -> (lags, autos, iac, ess) and prints the averages; `journal_plots`
(mcmc.py:388-398) prints min / 5 % / 50 % / 95 % / max / std per parameter.  `uqtils` is third-party and absent: parity with
its formulas is UNPINNED, and parity with Stan or ArviZ is not claimed (no rank normalisation).  The estimators, stated once
here and once in tests/chain_diag_np.py:

  burn-in       drop b = int(burnin * n) rows; n' rows remain.
  gamma         gamma(l) = (1/N) sum_{t=0}^{N-1-l} (x_t - xbar)(x_{t+l} - xbar) over a segment of N rows
                (pem_chain_autocov_f64_dev, csrc/pem_chains.hip: one launch sequence over every chain and parameter).
  per chain     rho(l) = gamma(l) / gamma(0) over the whole chain, N = n'.
  across chains each chain split in two: M = 2K chains of N = floor(n'/2) rows (the middle row dropped when n' is odd);
                s2_m = gamma_m(0) N / (N - 1),  W = mean_m s2_m,  B/N = sample variance (ddof 1) of the M segment means,
                var+ = (N - 1)/N W + B/N,  R-hat = sqrt(var+ / W),
                rho^(l) = 1 - (W - mean_m gamma_m(l)) / var+.
  IAC (Geyer 1992, initial monotone sequence) on rho or rho^ over the lags l < L = min(maxlag, N):
                P_k = rho(2k) + rho(2k+1) for 2k+1 < L;  k* = the last k with P_0 ... P_k all > 0;
                tau = -1 + 2 sum_{k <= k*} min(P_0 ... P_k), floored at 1/log10(M N) (ESS <= M N log10(M N)); M = 1 for
                one chain.  ESS = M N / tau.  `truncated`: the sequence is still positive at the last complete pair below
                L (tau is then a lower bound).  `step` only thins the returned curve, never this sum.
  MCSE          of the mean: pooled std / sqrt(ESS).
  degenerate    gamma(0) = 0 makes rho, tau and ESS NaN for that chain; for a parameter, W = 0 or any non-finite draw makes
                R-hat and ESS NaN.  One stuck chain among moving ones is not degenerate: it shows as a large R-hat.

Inputs: `samples` is (n, K, d) or (n, d) for one chain.  A CUDA fp64 tensor whose (K, d) block is contiguous (unit column
stride) is read in place and the results stay on its device; another CUDA tensor is copied once on its device.  Anything
else is copied once to the current device and the results come back as numpy.  There is no CPU path.
"""
import ctypes as C

import numpy as np

from . import _lib

__all__ = ['autocovariance', 'autocorrelation', 'split_rhat', 'ess', 'summary', 'format_summary']

FIRST_LAG_BLOCK = 64        # lags of the first launch of the adaptive ESS window; each later launch doubles the window


def autocovariance(x, n_lags: int, lag0: int = 0, lag_step: int = 1, n_seg: int = 1, seg_len: int | None = None,
                   seg_stride: int = 0):
    """pem_chain_autocov_f64_dev on a CUDA fp64 tensor `x` of shape (n_rows, n_series) with unit column stride (any row
    stride >= n_series).  Returns CUDA tensors (mean (n_seg, n_series), acov (n_seg, n_lags, n_series)): segment s is rows
    s*seg_stride ... + seg_len (default: all rows), lags lag0 + i*lag_step.  See include/pem_hip.h for the definitions."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.stride(1) == 1):
        raise ValueError('autocovariance: x must be a CUDA float64 tensor (n_rows, n_series) with unit column stride')
    n_rows, n_series = x.shape
    seg_len = n_rows if seg_len is None else int(seg_len)
    ld = int(x.stride(0))
    n_tb = -(-seg_len // _lib.CHAIN_TIME_BLOCK)
    dev = x.device
    mean = torch.empty((n_seg, n_series), dtype=torch.float64, device=dev)
    acov = torch.empty((n_seg, n_lags, n_series), dtype=torch.float64, device=dev)
    work = torch.empty(max(1, n_seg * n_tb * n_lags * n_series), dtype=torch.float64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.pem_chain_autocov_f64_dev(n_rows, n_series, ld, C.c_void_p(x.data_ptr()), int(n_seg), seg_len, int(seg_stride),
                                                 int(lag0), int(lag_step), int(n_lags), C.c_void_p(mean.data_ptr()),
                                                 C.c_void_p(acov.data_ptr()), C.c_void_p(work.data_ptr()), work.numel(), stream))
    return mean, acov


# ---------------------------------------------------------------------------------------------------------------- inputs

def _shape(samples):
    shape = tuple(samples.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f'samples must be (n, K, d) or (n, d), got shape {shape}')
    return shape if len(shape) == 3 else (shape[0], 1, shape[1])


def _check(samples, burnin, maxlag=100, step=1):
    n, K, d = _shape(samples)
    if not 0.0 <= burnin < 1.0:
        raise ValueError(f'burnin must be in [0, 1), got {burnin}')
    if maxlag is not None and maxlag < 2:
        raise ValueError(f'maxlag must be >= 2, got {maxlag}')
    if step < 1:
        raise ValueError(f'step must be >= 1, got {step}')
    b = int(burnin * n)
    if n - b < 4:
        raise ValueError(f'{n - b} rows after burn-in: at least 4 are needed')
    return n, K, d, b


def _device_view(samples, b):
    """(rows after burn-in seen as (n', K*d) on the device, K, d, whether results go back as numpy)"""
    import torch
    n, K, d = _shape(samples)
    if isinstance(samples, torch.Tensor) and samples.is_cuda:
        x, host = samples, False
    else:
        _lib.require_device()
        x, host = torch.as_tensor(np.asarray(samples, dtype=np.float64), device='cuda'), True
    x = x.reshape(n, K, d)
    if x.dtype != torch.float64 or x.stride(2) != 1 or (K > 1 and x.stride(1) != d):
        x = x.to(torch.float64).contiguous()
    return x[b:].reshape(n - b, K * d), K, d, host


def _out(v, host, like):
    """numpy results back as they are; device results as tensors on `like`'s device"""
    import torch
    if host:
        return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v), device=like.device)


# ------------------------------------------------------------------------------------------------------------ estimators

def _geyer(rho, mn):
    """tau and `truncated` of Geyer's initial monotone sequence, column by column; rho: (L, m) numpy, mn: M N per column.
    The sum over k <= k* is a running sum down the column (np.add.accumulate adds row after row), so tau depends on the
    terms up to k* only, not on how many lags follow them (the adaptive ESS relies on it)."""
    L, m = rho.shape
    npair = L // 2
    P = rho[0:2 * npair:2] + rho[1:2 * npair:2]
    kstar = np.logical_and.accumulate(P > 0, axis=0).sum(axis=0)     # number of terms: k* + 1
    csum = np.add.accumulate(np.minimum.accumulate(P, axis=0), axis=0) if npair else np.zeros((1, m))
    total = np.where(kstar > 0, csum[np.maximum(kstar - 1, 0), np.arange(m)], 0.0)
    tau = np.maximum(-1.0 + 2.0 * total, 1.0 / np.log10(mn))
    tau[~np.isfinite(rho[0])] = np.nan
    return tau, (kstar == npair) & (npair > 0)


def _split(flat, n_lags, lag0=0):
    """split-half gamma: mean (2, K*d), acov (2, n_lags, K*d), N"""
    rows = flat.shape[0]
    N = rows // 2
    mean, acov = autocovariance(flat, n_lags, lag0=lag0, n_seg=2, seg_len=N, seg_stride=rows - N)
    return mean, acov, N


def _between_within(mean, g0, N, K, d):
    """W, var+ and R-hat per parameter from the split-half means and gamma(0) (numpy, (d,) each)"""
    means = mean.reshape(2 * K, d)
    W = (g0.reshape(2 * K, d) * (N / (N - 1))).mean(axis=0)
    BN = means.var(axis=0, ddof=1)
    var_plus = (N - 1) / N * W + BN
    with np.errstate(divide='ignore', invalid='ignore'):
        rhat = np.sqrt(var_plus / W)
    bad = ~np.isfinite(W) | (W == 0)
    rhat[bad] = np.nan
    return W, var_plus, rhat, bad


def _chain_mean(acov, K, d):
    """mean over the 2K split chains of gamma (2, L, K*d) on the device -> (L, d) numpy.  A fixed pairwise tree of
    element-wise adds: a lag's value does not depend on how many lags the launch held (the adaptive ESS relies on it)."""
    import torch
    g = acov.reshape(2, -1, K, d).permute(1, 0, 2, 3).reshape(-1, 2 * K, d)
    while g.shape[1] > 1:
        h = g.shape[1] // 2
        top = g[:, :h] + g[:, h:2 * h]
        g = torch.cat([top, g[:, 2 * h:]], dim=1) if g.shape[1] % 2 else top
    return (g[:, 0] / (2 * K)).cpu().numpy()


def _rho_hat(g_mean, W, var_plus):
    """cross-chain rho^(l) (L, d) from the mean over chains of gamma (L, d)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return 1.0 - (W[None, :] - g_mean) / var_plus[None, :]


def autocorrelation(samples, maxlag: int = 100, step: int = 1):
    """`uq.autocorrelation(samples, step, maxlag)` as used at mcmc.py:310 and 324: (lags (nlags,), autos (nlags, K, d),
    iac (K, d), ess (K, d)) per chain, no burn-in dropped here.  lags = range(0, L, step), L = min(maxlag, n); the IAC uses
    every lag below L."""
    n, K, d, _ = _check(samples, 0.0, maxlag, step)
    one = len(samples.shape) == 2
    flat, K, d, host = _device_view(samples, 0)
    L = min(int(maxlag), n)
    _, acov = autocovariance(flat, L)
    rho = acov[0] / acov[0, 0:1]                                 # (L, K*d) on the device; gamma(0) = 0 gives NaN
    tau, _ = _geyer(rho.cpu().numpy(), float(n))
    lags = np.arange(0, L, step)
    autos = rho[::step].reshape(lags.size, K, d)
    iac, ess_ = tau.reshape(K, d), n / tau.reshape(K, d)
    if one:
        autos, iac, ess_ = autos[:, 0], iac[0], ess_[0]
    return lags, _out(autos, host, flat), _out(iac, host, flat), _out(ess_, host, flat)


def split_rhat(samples, burnin: float = 0.1):
    """split R-hat (d,) of the rows after burn-in"""
    n, K, d, b = _check(samples, burnin)
    flat, K, d, host = _device_view(samples, b)
    mean, acov, N = _split(flat, 1)
    _, _, rhat, _ = _between_within(mean.cpu().numpy(), acov[:, 0].cpu().numpy(), N, K, d)
    return _out(rhat, host, flat)


def _ess(flat, K, d, maxlag):
    """(ess, truncated, tau, rhat) numpy (d,) each, from split halves; maxlag None grows the lag window launch by launch"""
    rows = flat.shape[0]
    N = rows // 2
    L_full = N if maxlag is None else min(int(maxlag), N)
    L = L_full if maxlag is not None else min(FIRST_LAG_BLOCK, N)
    mean, acov, _ = _split(flat, L)
    W, var_plus, rhat, bad = _between_within(mean.cpu().numpy(), acov[:, 0].cpu().numpy(), N, K, d)
    rho = _rho_hat(_chain_mean(acov, K, d), W, var_plus)
    while True:
        tau, truncated = _geyer(rho, float(2 * K * N))
        if L >= L_full or not (truncated & ~bad).any():          # every sequence has ended, or N is reached
            break
        L_next = min(2 * L, L_full)                               # the next launch starts where this one ended
        _, more, _ = _split(flat, L_next - L, lag0=L)
        rho = np.concatenate([rho, _rho_hat(_chain_mean(more, K, d), W, var_plus)])
        L = L_next
    tau[bad] = np.nan
    return 2 * K * N / tau, truncated & ~bad, tau, rhat


def ess(samples, burnin: float = 0.1, maxlag: int | None = None):
    """cross-chain ESS (d,) and `truncated` (d,) of the rows after burn-in.  maxlag None: the lag window doubles, one
    launch and one host check per window, until every parameter's sequence has ended or N is reached."""
    n, K, d, b = _check(samples, burnin, maxlag)
    flat, K, d, host = _device_view(samples, b)
    e, trunc, _, _ = _ess(flat, K, d, maxlag)
    return _out(e, host, flat), _out(trunc, host, flat)


def summary(samples, names=None, burnin: float = 0.1, percentiles=(5, 50, 95), acceptance=None):
    """Per-parameter table of the rows after burn-in, pooled over chains (journal_plots, mcmc.py:388-398): min, the
    percentiles (np.percentile's, bit for bit), max, std (ddof 0), mean, and mcse, rhat, ess, iac, truncated.  `acceptance`
    ((K,) from Metropolis, (2, K) from DRAM): its mean over chains, per stage for DRAM."""
    import torch
    n, K, d, b = _check(samples, burnin)
    if names is not None and len(names) != d:
        raise ValueError(f'{len(names)} names for {d} parameters')
    from .drivers import column_percentiles
    flat, K, d, host = _device_view(samples, b)
    pooled = flat.reshape(-1, d) if flat.is_contiguous() else flat.contiguous().reshape(-1, d)
    e, trunc, tau, rhat = _ess(flat, K, d, None)
    pct = column_percentiles(pooled, list(percentiles))
    std = pooled.std(dim=0, correction=0)
    out = {'names': list(names) if names is not None else [f'x{i}' for i in range(d)],
           'min': pooled.amin(dim=0), 'max': pooled.amax(dim=0), 'mean': pooled.mean(dim=0), 'std': std,
           'rhat': rhat, 'ess': e, 'iac': tau, 'truncated': trunc, 'percentiles': tuple(percentiles),
           'n_draws': (n - b) * K}
    for p, row in zip(percentiles, pct):
        out[f'p{p:g}'] = row
    out['mcse'] = std / torch.sqrt(torch.as_tensor(e, device=std.device))
    if acceptance is not None:
        a = acceptance.double().cpu().numpy() if isinstance(acceptance, torch.Tensor) else np.asarray(acceptance, dtype=np.float64)
        out['acceptance'] = a.mean(axis=-1)
    for k in ('min', 'max', 'mean', 'std', 'rhat', 'ess', 'iac', 'truncated', 'mcse') + tuple(f'p{p:g}' for p in percentiles):
        out[k] = _out(out[k], host, flat)
    return out


def format_summary(s) -> str:
    """show_mcmc's 'Average acceptance ratio / IAC / ESS' lines, then journal_plots' table with R-hat, ESS and MCSE"""
    def num(v):
        return np.asarray(v.cpu() if hasattr(v, 'cpu') else v, dtype=np.float64)
    lines = []
    if 'acceptance' in s:
        a = np.atleast_1d(s['acceptance'])
        extra = f' (stage 1 {a[0]:.4f}, delayed stage {a[1]:.4f})' if a.size == 2 else ''
        lines.append(f'Average acceptance ratio: {a.sum():.4f}{extra}')
    lines.append(f'Average IAC: {np.mean(num(s["iac"])):.4f}')
    lines.append(f'Average ESS: {np.mean(num(s["ess"])):.4f}')
    cols = ['min'] + [f'p{p:g}' for p in s['percentiles']] + ['max', 'std']
    heads = ['Minimum'] + [f'{p:g}th percentile' for p in s['percentiles']] + ['Maximum', 'Std deviation']
    lines.append(f'{"Variable": <10} ' + ' '.join(f'{h: <20}' for h in heads) + f' {"R-hat": <8} {"ESS": <10} {"MCSE": <12}')
    vals = {k: num(s[k]) for k in cols + ['rhat', 'ess', 'mcse']}
    trunc = num(s['truncated'])
    for i, name in enumerate(s['names']):
        row = ' '.join(f'{vals[k][i]: <20.5f}' for k in cols)
        ess_txt = f'{vals["ess"][i]:.0f}' + ('+' if trunc[i] else '')
        lines.append(f'{str(name): <10} {row} {vals["rhat"][i]: <8.4f} {ess_txt: <10} {vals["mcse"][i]: <12.4g}')
    if trunc.any():
        lines.append('+ the autocorrelation sequence had not ended at the last lag: ESS is an upper bound')
    return '\n'.join(lines)

