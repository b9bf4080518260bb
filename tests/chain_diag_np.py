"""numpy restatement of hallthrusterpem_amd/diagnostics.py (the estimators its docstring states), for the tests.

  burn-in       drop b = int(burnin * n) rows; n' rows remain.
  gamma         gamma(l) = (1/N) sum_{t=0}^{N-1-l} (x_t - xbar)(x_{t+l} - xbar) over a segment of N rows.
  per chain     rho(l) = gamma(l) / gamma(0), N = n'.
  across chains M = 2K split halves of N = floor(n'/2) rows (second half starts at row ceil(n'/2));
                s2_m = gamma_m(0) N / (N - 1), W = mean s2_m, B/N = var(ddof 1) of the M means, var+ = (N - 1)/N W + B/N,
                R-hat = sqrt(var+ / W), rho^(l) = 1 - (W - mean_m gamma_m(l)) / var+.
  IAC           Geyer's initial monotone sequence over l < L = min(maxlag, N): P_k = rho(2k) + rho(2k+1), 2k+1 < L;
                k* = last k with P_0..P_k > 0; tau = -1 + 2 sum_{k<=k*} min(P_0..P_k), floored at 1/log10(M N);
                ESS = M N / tau; truncated when P_k > 0 for every complete pair below L.
  degenerate    gamma(0) = 0 -> rho, tau, ESS NaN (one chain); W = 0 or a non-finite draw -> R-hat, ESS NaN (a parameter).

`gamma_direct` is the long-double restatement the kernel is held to; `gamma_fft` the float64 one the host tests use.
"""
import numpy as np


def gamma_direct(x, lags, n_seg=1, seg_len=None, seg_stride=0, dtype=np.longdouble):
    """x (n_rows, S) -> mean (n_seg, S), gamma (n_seg, len(lags), S), and for the error bound: sabs (n_seg, nl, S) =
    sum_t |y_t y_{t+l}|, aabs (n_seg, nl, S) = sum_t (|y_t| + |y_{t+l}|), xabs (n_seg, S) = sum_t |x_t|, all in `dtype`"""
    x = np.asarray(x)
    seg_len = x.shape[0] if seg_len is None else seg_len
    S, nl = x.shape[1], len(lags)
    mean = np.empty((n_seg, S), dtype)
    gam, sabs, aabs = (np.empty((n_seg, nl, S), dtype) for _ in range(3))
    xabs = np.empty((n_seg, S), dtype)
    N = seg_len
    for s in range(n_seg):
        xs = x[s * seg_stride:s * seg_stride + N].astype(dtype)
        mean[s] = xs.sum(axis=0) / dtype(N)
        xabs[s] = np.abs(xs).sum(axis=0)
        y = xs - mean[s]
        for i, l in enumerate(lags):
            p = y[:N - l] * y[l:]
            gam[s, i] = p.sum(axis=0) / dtype(N)
            sabs[s, i] = np.abs(p).sum(axis=0)
            aabs[s, i] = (np.abs(y[:N - l]) + np.abs(y[l:])).sum(axis=0)
    return mean, gam, sabs, aabs, xabs


def gamma_fft(x, n_lags):
    """x (N, S) float64 -> gamma (n_lags, S) by a zero-padded FFT"""
    N = x.shape[0]
    y = x - x.mean(axis=0)
    m = 1 << int(np.ceil(np.log2(2 * N)))
    f = np.fft.rfft(y, m, axis=0)
    return np.fft.irfft(f * np.conj(f), m, axis=0)[:n_lags] / N


def geyer(rho, mn):
    """rho (L, m) -> tau (m,), truncated (m,)"""
    rho = np.asarray(rho, dtype=np.float64)
    L, m = rho.shape
    tau, trunc = np.full(m, np.nan), np.zeros(m, bool)
    for j in range(m):
        if not np.isfinite(rho[0, j]):
            continue
        s, run, k, npair = 0.0, np.inf, 0, L // 2
        terms = []
        while k < npair:
            p = rho[2 * k, j] + rho[2 * k + 1, j]
            if not p > 0:
                break
            run = min(run, p)
            terms.append(run)
            k += 1
        s = np.sum(np.array(terms)) if terms else 0.0
        trunc[j] = npair > 0 and k == npair
        tau[j] = max(-1.0 + 2.0 * s, 1.0 / np.log10(mn))
    return tau, trunc


def per_chain(gamma, N):
    """gamma (L, m) of whole chains -> rho (L, m), tau (m,), ess (m,)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        rho = gamma / gamma[0:1]
    tau, _ = geyer(rho, float(N))
    return rho, tau, N / tau


def cross_chain(mean, gamma, N):
    """split-half means (M, d) and gamma (L, M, d) -> dict(rhat, rho_hat (L, d), tau, ess, truncated, W, var_plus)"""
    M = mean.shape[0]
    W = (gamma[0] * (N / (N - 1))).mean(axis=0)
    var_plus = (N - 1) / N * W + mean.var(axis=0, ddof=1)
    bad = ~np.isfinite(W) | (W == 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        rhat = np.where(bad, np.nan, np.sqrt(var_plus / W))
        rho_hat = 1.0 - (W - gamma.mean(axis=1)) / var_plus
    tau, trunc = geyer(rho_hat, float(M * N))
    tau[bad] = np.nan
    return dict(rhat=rhat, rho_hat=rho_hat, tau=tau, ess=M * N / tau, truncated=trunc & ~bad, W=W, var_plus=var_plus)


def split(samples, burnin):
    """(n, K, d) -> the split halves (N, 2K, d): chain k's first half is chain k, its second half chain K + k"""
    s = np.asarray(samples, dtype=np.float64)
    s = s[int(burnin * s.shape[0]):]
    n = s.shape[0]
    N = n // 2
    return np.concatenate([s[:N], s[n - N:]], axis=1), N


def split_stats(samples, burnin=0.1, maxlag=None):
    """cross_chain from data, gamma by FFT"""
    h, N = split(samples, burnin)
    M, d = h.shape[1], h.shape[2]
    L = N if maxlag is None else min(maxlag, N)
    g = gamma_fft(h.reshape(N, M * d), L).reshape(L, M, d)
    return cross_chain(h.mean(axis=0), g, N)


def autocorrelation(samples, maxlag=100, step=1):
    """(lags, autos (nlags, K, d), iac (K, d), ess (K, d)) of whole chains, gamma by FFT"""
    s = np.asarray(samples, dtype=np.float64)
    n, K, d = s.shape
    L = min(maxlag, n)
    g = gamma_fft(s.reshape(n, K * d), L)
    rho, tau, e = per_chain(g, n)
    lags = np.arange(0, L, step)
    return lags, rho[::step].reshape(lags.size, K, d), tau.reshape(K, d), e.reshape(K, d)
