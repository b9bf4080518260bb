"""MCMC chain diagnostics without a GPU: pem_chain_autocov_f64_dev is declared, bound, built and exported, refuses every
malformed call before it looks for a device, compiles without scratch or spills; diagnostics.py refuses bad arguments before
it touches a device; tests/chain_diag_np.py gives the known answers (a hand-worked example, AR(1), R-hat, degenerate cases)."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import chain_diag_np as ref

ROOT = Path(__file__).resolve().parents[1]
NAME = 'pem_chain_autocov_f64_dev'


def test_symbol_is_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % NAME, header)
    assert m and len(m.group(1).split(',')) == 15
    assert len(_lib.SIGNATURES[NAME][1]) == 15
    assert re.search(r'#define PEM_CHAIN_TIME_BLOCK (\d+)', header).group(1) == str(_lib.CHAIN_TIME_BLOCK)
    assert build.PKG / 'csrc' / 'pem_chains.hip' in build.SRCS
    assert hasattr(_lib.load(), NAME)


def _call(n_rows=100, n_series=3, ld=3, x=True, n_seg=1, seg_len=100, seg_stride=0, lag0=0, lag_step=1, n_lags=10, mean=True,
          acov=True, work=True, work_len=None):
    from hallthrusterpem_amd import _lib
    fake = C.c_void_p(4096)                     # never dereferenced: every check runs on the host
    if work_len is None:
        work_len = n_seg * -(-seg_len // _lib.CHAIN_TIME_BLOCK) * n_lags * n_series
    return _lib.load().pem_chain_autocov_f64_dev(n_rows, n_series, ld, fake if x else None, n_seg, seg_len, seg_stride, lag0, lag_step,
                                                 n_lags, fake if mean else None, fake if acov else None, fake if work else None,
                                                 work_len, None)


@pytest.mark.parametrize('bad', [
    dict(n_rows=0), dict(n_series=0), dict(n_seg=0, work_len=10), dict(n_lags=0, work_len=10), dict(seg_len=0, work_len=10),
    dict(ld=2), dict(seg_len=1), dict(seg_len=101),
    dict(n_seg=2, seg_len=50, seg_stride=51), dict(n_seg=3, seg_len=34, seg_stride=34),
    dict(lag0=100), dict(n_lags=101), dict(lag0=91), dict(lag_step=0), dict(lag_step=12),
    dict(x=False), dict(mean=False), dict(acov=False), dict(work=False), dict(work_len=29),
])
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_chain_autocov' in _lib.load().pem_last_error()



@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_chain_kernels_have_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_chains.hip')],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    assert sorted(rows) == ['chain_acov_partial_kernel', 'chain_acov_reduce_kernel', 'chain_mean_kernel'], rows
    for name, r in rows.items():
        assert r['vspill'] == 0 and r['sspill'] == 0 and r['scratch'] == 0, (name, r)
    assert rows['chain_acov_partial_kernel']['vgpr'] <= 256          # two waves per SIMD


# ---- Python refusals: raised from shapes and arguments alone, before any device is looked for

@pytest.mark.parametrize('call', [
    lambda d, x: d.split_rhat(x, burnin=1.0), lambda d, x: d.split_rhat(x, burnin=-0.1), lambda d, x: d.ess(x, burnin=1.5),
    lambda d, x: d.split_rhat(x[:4], burnin=0.5), lambda d, x: d.ess(x[:3], burnin=0.0),
    lambda d, x: d.autocorrelation(x[:3]), lambda d, x: d.autocorrelation(x, maxlag=1), lambda d, x: d.autocorrelation(x, step=0),
    lambda d, x: d.ess(x, maxlag=1), lambda d, x: d.split_rhat(x[..., None]), lambda d, x: d.split_rhat(x[:, 0, 0]),
    lambda d, x: d.summary(x, names=['a', 'b']), lambda d, x: d.summary(x, burnin=1.0),
])
def test_python_refusals_come_before_the_device(call, monkeypatch):
    from hallthrusterpem_amd import _lib, diagnostics
    monkeypatch.setattr(_lib, 'require_device', lambda: pytest.fail('a device was looked for'))
    with pytest.raises(ValueError):
        call(diagnostics, np.zeros((20, 4, 3)))


# ---- the restatement's known answers

A = np.array([1, 3, 2, 4, 3, 5], float)
B = np.array([2, 2, 4, 4, 6, 6], float)


def test_hand_worked_two_chains_of_six_rows():
    x = np.stack([A, B], 1)[:, :, None]                       # (6, 2, 1)
    r = ref.split_stats(x, burnin=0.0)
    # halves (1,3,2) (2,2,4) | (4,3,5) (4,6,6): means 2, 8/3, 4, 16/3; gamma(0) 2/3, 8/9, 2/3, 8/9; W = 7/6; B/N = 59/27
    assert np.isclose(r['W'][0], 7 / 6, rtol=1e-14, atol=0)
    assert np.isclose(r['var_plus'][0], 80 / 27, rtol=1e-14, atol=0)
    assert np.isclose(r['rhat'][0], np.sqrt(160 / 63), rtol=1e-14, atol=0)
    # mean gamma(l) = 7/9, -13/54, -4/27  ->  rho^ = 0.86875, 0.525, 0.55625; L = 3: one pair, positive -> truncated
    assert np.allclose(r['rho_hat'][:, 0], [0.86875, 0.525, 0.55625], rtol=1e-14, atol=0)
    assert r['truncated'][0]
    assert np.isclose(r['tau'][0], -1 + 2 * 1.39375, rtol=1e-14) and np.isclose(r['ess'][0], 12 / 1.7875, rtol=1e-14)
    # chain A whole, maxlag 4: rho = 1, -0.1, 0.4, -0.4; P_0 = 0.9, P_1 = 0: tau = 0.8, floored at 1/log10(6)
    lags, autos, iac, e = ref.autocorrelation(A[:, None, None], maxlag=4)
    assert np.array_equal(lags, [0, 1, 2, 3])
    assert np.allclose(autos[:, 0, 0], [1, -0.1, 0.4, -0.4], rtol=1e-13, atol=1e-15)
    assert np.isclose(iac[0, 0], 1 / np.log10(6), rtol=1e-14) and np.isclose(e[0, 0], 6 * np.log10(6), rtol=1e-14)


def _ar1(phi, K, n, seed=0, d=1):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, K, d))
    x = np.empty_like(e)
    x[0] = e[0] / np.sqrt(1 - phi * phi)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    return x


@pytest.mark.parametrize('phi', [-0.5, 0.0, 0.5, 0.9])
def test_ar1_iac_and_ess(phi):
    K, n = 8, 200_000
    x = _ar1(phi, K, n, seed=int(10 * phi) + 11)
    tau_true = (1 + phi) / (1 - phi)
    _, _, iac, _ = ref.autocorrelation(x, maxlag=2000)
    assert np.all(np.abs(iac / tau_true - 1) < 0.15), (iac.ravel(), tau_true)
    r = ref.split_stats(x, burnin=0.1)
    want = K * int(0.9 * n) * (1 - phi) / (1 + phi)
    assert abs(r['ess'][0] / want - 1) < 0.05, (r['ess'], want)
    assert not r['truncated'][0]


def test_rhat_separates_a_shifted_chain():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4000, 2, 2))
    assert np.all(ref.split_stats(x)['rhat'] < 1.01)
    x[:, 1, 1] += 1.0                                          # one chain's mean moved by one sd in parameter 1
    r = ref.split_stats(x)['rhat']
    assert r[0] < 1.01 and r[1] > 1.1, r


def test_truncated_when_maxlag_is_shorter_than_the_sequence():
    x = _ar1(0.99, 4, 20_000, seed=3)
    assert ref.split_stats(x, maxlag=20)['truncated'][0]
    assert not ref.split_stats(x)['truncated'][0]


def test_degenerate_cases():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((400, 4, 3))
    x[:, :, 0] = 2.5                                           # constant parameter: gamma(0) = 0, W = 0
    x[207, 2, 1] = np.nan                                      # one non-finite draw after the burn-in
    x[:, 1, 2] = 9.0                                           # one stuck chain among moving ones: not degenerate
    r = ref.split_stats(x)
    assert np.isnan(r['rhat'][0]) and np.isnan(r['ess'][0]) and np.isnan(r['rhat'][1]) and np.isnan(r['ess'][1])
    assert np.isfinite(r['ess'][2]) and r['rhat'][2] > 2
    _, autos, iac, e = ref.autocorrelation(x, maxlag=50)
    assert np.all(np.isnan(iac[:, 0])) and np.all(np.isnan(e[:, 0])) and np.all(np.isnan(autos[:, :, 0]))
    assert np.isnan(iac[1, 2]) and np.isfinite(iac[0, 2])      # the stuck chain alone has gamma(0) = 0
