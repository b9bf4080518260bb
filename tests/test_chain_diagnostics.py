"""MCMC chain diagnostics on the MI355X: pem_chain_autocov_f64_dev against a long-double restatement over its dispatch space,
its determinism and lag-block independence, NaN isolation; diagnostics.py against tests/chain_diag_np.py fed with the
device's gamma; DRAM end to end; case (b) of the probe against numpy's FFT.

Error bound of the kernel (u = 2^-53, gamma_k = k u / (1 - k u)).  With y_t = x_t - xbar (exact mean), the device mean m^
sums every x_t through at most N + 32 additions and one division, so |delta| = |m^ - xbar| <= D = gamma_{N+33} sum|x| / N
+ u |xbar|.  A staged value is (y_t - delta)(1 + e), |e| <= u; the product of two is (y_t - delta)(y_{t+l} - delta)(1 + e2),
|e2| <= gamma_2; the products are accumulated by one fma chain per time block and the n_tb block sums added in order, at most
K = N + n_tb roundings per term.  With S = sum|y_t y_{t+l}|, A = sum(|y_t| + |y_{t+l}|), n_l = N - l terms and
Q = S + D A + n_l D^2 (a bound on sum|(y_t - delta)(y_{t+l} - delta)|):
    N |gamma^ - gamma| <= D A + n_l D^2 + (gamma_2 + gamma_K (1 + gamma_2)) Q,
and the division by N adds u |gamma^|.  The reference values S, A, sum|x| and gamma are computed in np.longdouble.
"""
import time

import numpy as np
import pytest

import chain_diag_np as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TB = 4096


def _g(k):
    return k * U / (1 - k * U)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _run(x, lags, n_seg=1, seg_len=None, seg_stride=0):
    from hallthrusterpem_amd import diagnostics
    lag0, step = int(lags[0]), int(lags[1] - lags[0]) if len(lags) > 1 else 1
    m, g = diagnostics.autocovariance(x, len(lags), lag0=lag0, lag_step=step, n_seg=n_seg, seg_len=seg_len, seg_stride=seg_stride)
    return m.cpu().numpy(), g.cpu().numpy()


def _check_against_long_double(xh, x, lags, n_seg=1, seg_len=None, seg_stride=0):
    N = xh.shape[0] if seg_len is None else seg_len
    m, g = _run(x, lags, n_seg, seg_len, seg_stride)
    mean, gam, sabs, aabs, xabs = ref.gamma_direct(xh, lags, n_seg, N, seg_stride)
    D = _g(N + 33) * xabs / N + U * np.abs(mean)
    assert np.all(np.abs(m - mean) <= D), 'mean outside its bound'
    n_l = (N - np.asarray(lags, dtype=np.longdouble))[None, :, None]
    Dl = D[:, None, :]
    Q = sabs + Dl * aabs + n_l * Dl * Dl
    bound = (Dl * aabs + n_l * Dl * Dl + (_g(2) + _g(N + -(-N // TB)) * (1 + _g(2))) * Q) / N + U * np.abs(g)
    err = np.abs(g - gam)
    assert np.all(np.isfinite(g)) and np.all(err <= bound), float(np.max(err / bound))


# (n_rows, n_series, extra ld, column offset, n_seg, seg_len, seg_stride, lags): every tile constant (32 series, 128 lags,
# 64-row stage, 4096-row time block) at and one past its size, one series, odd n, ld > n_series, an 8-byte aligned view
CASES = [
    (4096, 32, 0, 0, 1, None, 0, range(0, 129)),
    (4097, 33, 7, 1, 1, None, 0, range(0, 128)),
    (129, 1, 0, 0, 1, None, 0, range(0, 129)),
    (8193, 7, 0, 0, 2, 4096, 4097, range(5, 5 + 3 * 50, 3)),
    (210, 5, 2, 3, 3, 65, 70, range(64, 65)),
    (64, 31, 0, 0, 1, None, 0, range(0, 64)),
    (8193, 2, 0, 1, 1, None, 0, range(0, 258)),
    (1200, 5, 0, 0, 1, None, 0, range(3, 3 + 130 * 8, 130)),
    (2, 3, 0, 0, 1, None, 0, range(0, 2)),
]


@pytest.mark.parametrize('case', CASES, ids=[f'n{c[0]}_s{c[1]}_seg{c[4]}_l{c[7].start}+{c[7].step}x{len(c[7])}' for c in CASES])
def test_kernel_against_long_double(case):
    n, S, pad, off, n_seg, seg_len, stride, lags = case
    rng = np.random.default_rng(n + S)
    wide = 3.0 + rng.standard_normal((n, S + pad + off)) * rng.uniform(0.1, 10, S + pad + off)
    xh = wide[:, off:off + S]
    x = _dev(wide)[:, off:off + S]
    assert x.stride(0) == S + pad + off and (x.data_ptr() % 16 == 8) == (off % 2 == 1)
    _check_against_long_double(xh, x, list(lags), n_seg, seg_len, stride)


def test_repeat_runs_give_the_same_bits():
    import torch
    from hallthrusterpem_amd import diagnostics
    x = _dev(np.random.default_rng(1).standard_normal((9000, 70)))
    a = diagnostics.autocovariance(x, 300, n_seg=2, seg_len=4500, seg_stride=4500)
    for _ in range(3):
        b = diagnostics.autocovariance(x, 300, n_seg=2, seg_len=4500, seg_stride=4500)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_lags_do_not_depend_on_the_lag_blocks():
    import torch
    from hallthrusterpem_amd import diagnostics
    x = _dev(np.random.default_rng(2).standard_normal((9001, 45)) + 7.0)
    _, whole = diagnostics.autocovariance(x, 300)
    _, lo = diagnostics.autocovariance(x, 100)
    _, hi = diagnostics.autocovariance(x, 200, lag0=100)
    assert torch.equal(whole[:, :100], lo) and torch.equal(whole[:, 100:], hi)
    _, odd = diagnostics.autocovariance(x, 20, lag0=37, lag_step=13)
    assert torch.equal(odd[0], whole[0, 37:37 + 13 * 20:13])


def test_a_non_finite_value_poisons_its_series_only():
    import torch
    from hallthrusterpem_amd import diagnostics
    xh = np.random.default_rng(3).standard_normal((5000, 40))
    m0, g0 = diagnostics.autocovariance(_dev(xh), 150, n_seg=2, seg_len=2500, seg_stride=2500)
    xh[100, 3] = np.nan
    xh[4000, 17] = np.inf
    m1, g1 = diagnostics.autocovariance(_dev(xh), 150, n_seg=2, seg_len=2500, seg_stride=2500)
    keep = [c for c in range(40) if c not in (3, 17)]
    assert torch.equal(m0[:, keep], m1[:, keep]) and torch.equal(g0[..., keep], g1[..., keep])
    for s, c in ((0, 3), (1, 17)):
        assert torch.isnan(m1[s, c]) and torch.isnan(g1[s, :, c]).all()
    assert torch.equal(g0[1, :, 3], g1[1, :, 3]) and torch.equal(g0[0, :, 17], g1[0, :, 17])   # the other segment


def test_abi_refusals_with_device_buffers():
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    x = torch.zeros((100, 3), dtype=torch.float64, device='cuda')
    out = torch.zeros(4000, dtype=torch.float64, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731
    lib = _lib.load()
    ok = dict(n_rows=100, n_series=3, ld=3, n_seg=1, seg_len=100, seg_stride=0, lag0=0, lag_step=1, n_lags=10, work_len=30)
    for bad in (dict(ld=2), dict(seg_len=1), dict(n_lags=101), dict(lag_step=0), dict(work_len=29), dict(n_seg=2, seg_stride=1),
                dict(n_series=0), dict(lag0=100)):
        a = {**ok, **bad}
        rc = lib.pem_chain_autocov_f64_dev(a['n_rows'], a['n_series'], a['ld'], p(x), a['n_seg'], a['seg_len'], a['seg_stride'], a['lag0'],
                                           a['lag_step'], a['n_lags'], p(out), p(out[100:]), p(out[1000:]), a['work_len'], None)
        assert rc == _lib.PEM_ERR_INVALID_ARG, bad
    assert lib.pem_chain_autocov_f64_dev(100, 3, 3, p(x), 1, 100, 0, 0, 1, 10, p(out), p(out[100:]), p(out[1000:]), 30, None) == 0
    torch.cuda.synchronize()


# ---- the Python layer against the restatement, fed with the device's gamma

def _ar1_trace(n=3001, K=6, d=3, seed=4):
    rng = np.random.default_rng(seed)
    phi = np.array([0.2, 0.6, 0.9])[:d]
    e = rng.standard_normal((n, K, d))
    x = np.empty_like(e)
    x[0] = e[0]
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    return x + np.arange(d)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    f = np.isfinite(b)
    return float(np.max(np.abs(a[f] - b[f]) / np.maximum(np.abs(b[f]), 1e-300))) if f.any() else 0.0


def test_python_layer_matches_the_restatement_on_device_gamma():
    from hallthrusterpem_amd import diagnostics
    xh = _ar1_trace()
    n, K, d = xh.shape
    x = _dev(xh)
    lags, autos, iac, e = diagnostics.autocorrelation(x, maxlag=200, step=7)
    _, g = diagnostics.autocovariance(x.reshape(n, K * d), 200)
    rho, tau, e_ref = ref.per_chain(g[0].cpu().numpy(), n)
    assert np.array_equal(lags, np.arange(0, 200, 7))
    assert _rel(autos.cpu().numpy(), rho[::7].reshape(-1, K, d)) <= 1e-13
    assert _rel(iac.cpu().numpy(), tau.reshape(K, d)) <= 1e-13 and _rel(e.cpu().numpy(), e_ref.reshape(K, d)) <= 1e-13
    b = int(0.1 * n)
    rows = n - b
    N = rows // 2
    for maxlag in (150, None):
        L = N if maxlag is None else maxlag
        m, gs = diagnostics.autocovariance(x[b:].reshape(rows, K * d), L, n_seg=2, seg_len=N, seg_stride=rows - N)
        want = ref.cross_chain(m.cpu().numpy().reshape(2 * K, d), gs.cpu().numpy().transpose(1, 0, 2).reshape(L, 2 * K, d), N)
        got_e, got_t = diagnostics.ess(x, maxlag=maxlag)
        assert _rel(got_e.cpu().numpy(), want['ess']) <= 1e-13 and np.array_equal(got_t.cpu().numpy(), want['truncated'])
    assert _rel(diagnostics.split_rhat(x).cpu().numpy(), want['rhat']) <= 1e-13


def test_numpy_in_numpy_out_and_device_in_device_out():
    import torch
    from hallthrusterpem_amd import diagnostics
    xh = _ar1_trace(n=800, K=4)
    for f in (lambda s: diagnostics.autocorrelation(s, maxlag=50)[1:], lambda s: (diagnostics.split_rhat(s),),
              lambda s: diagnostics.ess(s), lambda s: tuple(v for k, v in diagnostics.summary(s).items()
                                                            if k in ('min', 'p50', 'std', 'rhat', 'ess', 'mcse'))):
        host, dev = f(xh), f(_dev(xh))
        assert all(isinstance(v, np.ndarray) for v in host)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev)
        for h, g in zip(host, dev):
            assert np.array_equal(h, g.cpu().numpy(), equal_nan=True)
    one = diagnostics.autocorrelation(xh[:, 0], maxlag=30)                     # (n, d): one chain
    assert one[1].shape == (30, 3) and one[2].shape == (3,)


def test_summary_statistics():
    from hallthrusterpem_amd import diagnostics
    xh = _ar1_trace(n=1501, K=8)
    s = diagnostics.summary(xh, names=['a', 'b', 'c'], burnin=0.2, percentiles=(5, 50, 95), acceptance=np.full((2, 8), 0.25))
    pooled = xh[int(0.2 * 1501):].reshape(-1, 3)
    for p in (5, 50, 95):
        assert np.array_equal(s[f'p{p}'], np.percentile(pooled, p, axis=0))
    assert np.array_equal(s['min'], pooled.min(0)) and np.array_equal(s['max'], pooled.max(0))
    assert _rel(s['std'], pooled.std(0)) <= 1e-13 and _rel(s['mean'], pooled.mean(0)) <= 1e-13
    assert np.allclose(s['mcse'], s['std'] / np.sqrt(s['ess']), rtol=1e-15, atol=0)
    assert np.array_equal(s['acceptance'], [0.25, 0.25])
    text = diagnostics.format_summary(s)
    assert text.startswith('Average acceptance ratio: 0.5000') and 'Average IAC' in text and 'R-hat' in text
    assert len(text.splitlines()) == 3 + 1 + 3 + ('upper bound' in text)


def test_adaptive_ess_equals_the_full_window():
    import torch
    from hallthrusterpem_amd import diagnostics
    x = _dev(_ar1_trace(n=6001, K=16))
    rows = 6001 - 600
    e_ad, t_ad = diagnostics.ess(x, maxlag=None)
    e_full, t_full = diagnostics.ess(x, maxlag=rows // 2)
    assert not t_ad.any() and not t_full.any()
    assert torch.equal(e_ad, e_full)


# ---- end to end

def _dram_trace(K=32, n_steps=3000):
    import torch
    from hallthrusterpem_amd.calibration import DRAM
    mu = np.array([1.0, -2.0, 0.5])
    sd = np.array([1.0, 0.3, 2.0])
    corr = np.array([[1.0, 0.6, -0.3], [0.6, 1.0, 0.2], [-0.3, 0.2, 1.0]])
    cov = corr * np.outer(sd, sd)
    prec = torch.as_tensor(np.linalg.inv(cov), device='cuda')
    mu_d = torch.as_tensor(mu, device='cuda')

    def logp(theta):
        z = theta - mu_d
        return -0.5 * ((z @ prec) * z).sum(dim=1)
    theta0 = np.random.default_rng(7).multivariate_normal(mu, cov, size=K)
    s = DRAM(logp, theta0, cov0=cov, n_chains=K, seed=11, adapt_after=500, adapt_interval=100, device='cuda')
    return s.run(n_steps), mu, sd


def test_dram_on_a_gaussian_mixes_and_a_stuck_chain_shows():
    import torch
    from hallthrusterpem_amd import diagnostics
    trace, mu, sd = _dram_trace()
    rhat = diagnostics.split_rhat(trace).cpu().numpy()
    assert np.all(rhat < 1.02), rhat
    stuck = trace[:, :1].clone()
    stuck[:, 0, :2] = torch.as_tensor(mu[:2] + 5 * sd[:2], device='cuda')       # stuck 5 sd away in parameters 0 and 1
    rhat2 = diagnostics.split_rhat(torch.cat([trace, stuck], dim=1)).cpu().numpy()
    assert np.all(rhat2[:2] > 1.2) and rhat2[2] < 1.05, rhat2
    s = diagnostics.summary(trace, names=['a', 'b', 'c'])
    assert np.all(np.abs(s['mean'].cpu().numpy() - mu) < 6 * s['mcse'].cpu().numpy())


def test_case_b_against_numpy_fft():
    import torch
    from hallthrusterpem_amd import diagnostics
    K, d, n = 64, 17, 20_000
    xh = np.random.default_rng(9).standard_normal((n, K * d)).cumsum(axis=0) * 1e-2 + 5.0
    x = _dev(xh)
    diagnostics.autocovariance(x[:4096], 1000)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, g = diagnostics.autocovariance(x, 1000)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    want = ref.gamma_fft(xh, 1000)
    err = np.abs(g[0].cpu().numpy() - want)
    assert np.all(err <= 1e-12 * want[0]), float(np.max(err / want[0]))
    assert dt < 0.5, dt
