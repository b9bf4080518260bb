"""The device-resident DRAM sampler without a GPU: pem_dram_step_f64_dev is declared, bound, built and exported, refuses every
malformed call before it looks for a device and compiles without scratch; DeviceDRAM refuses what it cannot run before it
touches a device; the numpy restatement of the launch (tests/dram_np.py) makes the accept decisions of calibration.DRAM on
CPU tensors on identical draws and ends in the same state; its Cholesky leaves L alone at a zero pivot."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import dram_np

ROOT = Path(__file__).resolve().parents[1]
NAME = 'pem_dram_step_f64_dev'


def test_the_entry_point_is_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % NAME, header)
    assert m and len(m.group(1).split(',')) == 24
    assert len(_lib.SIGNATURES[NAME][1]) == 24
    assert hasattr(_lib.load(), NAME)
    assert re.search(r'#define PEM_DRAM_MAX_DIM (\d+)', header).group(1) == str(_lib.DRAM_MAX_DIM) == '32'
    assert build.PKG / 'csrc' / 'pem_dram.hip' in build.SRCS


FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host
ARRAYS = ('theta', 'logp', 'L', 'mean', 'scatter', 'prop', 'prop_logp', 'state', 'accepted', 'flags', 'trace', 'logp_trace', 'draws')
OPTIONAL = ('trace', 'logp_trace', 'draws')


def _call(K=4, d=3, seed=1, gamma=0.1, eps=1e-12, adapt_after=10, adapt_interval=5, trace_first=0, trace_len=8, thin=1, **null):
    from hallthrusterpem_amd import _lib
    ptrs = [None if null.get(a, a in ('logp_trace', 'draws')) else FAKE for a in ARRAYS]      # name=True: that array is NULL
    return _lib.load().pem_dram_step_f64_dev(K, d, seed, gamma, eps, adapt_after, adapt_interval, trace_first, trace_len, thin,
                                             *ptrs, None)


@pytest.mark.parametrize('bad', [
    dict(K=0), dict(d=0), dict(d=-1), dict(d=33), dict(gamma=0.0), dict(gamma=-0.1), dict(gamma=float('nan')), dict(eps=-1e-12),
    dict(eps=float('nan')), dict(adapt_interval=0), dict(thin=0), dict(trace_len=0),
    dict(trace_len=0, trace=True, logp_trace=False),                     # a logp trace alone needs rows as well
] + [{a: True} for a in ARRAYS if a not in OPTIONAL])
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_dram_step' in _lib.load().pem_last_error()


def test_a_well_formed_call_gets_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _call() == _lib.PEM_ERR_NO_DEVICE
    assert _call(trace=True, trace_len=0) == _lib.PEM_ERR_NO_DEVICE      # no trace: trace_len is not looked at
    assert _call(d=32, K=1, eps=0.0, adapt_after=0) == _lib.PEM_ERR_NO_DEVICE


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_dram_kernel_has_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_dram.hip')],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+) kernarg\s+(\d+) lds\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)),
                                    lds=int(m.group(8)))
    assert list(rows) == ['dram_step_kernel'], rows
    r = rows['dram_step_kernel']                # one wave per chain; the factor is built in 32 x 33 doubles of LDS
    assert r['sspill'] == 0 and r['vspill'] == 0 and r['scratch'] == 0 and r['vgpr'] <= 128 and r['lds'] <= 16 * 1024, r


def _f(theta):
    raise AssertionError('log_posterior must not be called')


@pytest.mark.parametrize('kw, match', [
    (dict(theta0=np.zeros(33)), '1 to 32 parameters'),
    (dict(theta0=np.zeros((4, 40))), '1 to 32 parameters'),
    (dict(theta0=np.zeros(3), device='cpu'), 'GPU only'),
    (dict(theta0='tensor'), 'GPU only'),                                  # a CPU tensor as the start point
    (dict(theta0=np.zeros(3), gamma=0.0), 'gamma > 0'),
    (dict(theta0=np.zeros(3), adapt_interval=0), 'adapt_interval >= 1'),
    (dict(theta0=np.zeros(3), cov0=np.eye(2)), 'cov0'),
])
def test_the_driver_refuses_what_it_cannot_run_before_touching_a_device(kw, match, monkeypatch):
    import torch
    from hallthrusterpem_amd.calibration import DeviceDRAM
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    if isinstance(kw['theta0'], str):
        kw = dict(kw, theta0=torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match=match):
        DeviceDRAM(_f, **kw)


# -------------------------------------------------------------------------------- the restatement against calibration.DRAM
def _target(d):
    """the correlated Gaussian of test_dram_recovers_a_correlated_gaussian... (its leading d x d block), one hard bound"""
    import torch
    mu = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)[:d]
    A = torch.tensor([[1.0, 0.0, 0.0], [0.8, 0.6, 0.0], [-0.3, 0.2, 0.4]], dtype=torch.float64)[:d, :d]
    prec = torch.linalg.inv(A @ A.T)

    def logp(t):
        r = t - mu
        lp = -0.5 * torch.einsum('ki,ij,kj->k', r, prec, r)
        return torch.where(t[:, -1] > -1.0, lp, torch.full_like(lp, -float('inf')))
    return logp


def _scaled(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny))


# measured: the worst scaled difference of theta, logp, mean, scatter and L after the free run; asserted at 100 x that
MEASURED = {(8, 3): 1.23e-15, (3, 1): 0.0}


@pytest.mark.parametrize('K, d, n_steps', [(8, 3, 300), (3, 1, 200)])
def test_the_restatement_makes_the_decisions_of_dram_on_identical_draws(K, d, n_steps):
    """tests/dram_np.py against calibration.DRAM (CPU tensors), both free-running on the draws of twin torch generators: every
    accept decision is equal, and the states agree to rounding.  DRAM forms L z by einsum and w by a triangular solve, the
    restatement in index order and as z1 - sqrt(gamma) z2.  Measured worst scaled difference (max |a - b| / max |b| over theta,
    logp, mean, scatter, L) at the end of the run: 1.23e-15 at (8, 3, 300 steps) and 0 at (3, 1, 200 steps); the bound is 100 x
    that (for the exact case: equality).  This pins the restatement to the existing sampler, not to the kernel."""
    import torch
    from hallthrusterpem_amd.calibration import DRAM
    logp = _target(d)
    seed, gamma, eps, after, every = 7, 0.1, 1e-12, 50, 25
    cov0 = np.diag(np.full(d, 4.0))
    ref = DRAM(logp, np.zeros(d), cov0=cov0, n_chains=K, seed=seed, adapt_after=after, adapt_interval=every, eps=eps, gamma=gamma)
    twin = torch.Generator()
    twin.manual_seed(seed)
    zs, us = [], []
    for _ in range(n_steps + 1):
        zs.append(torch.randn((2, K, d), dtype=torch.float64, generator=twin).numpy())
        us.append(torch.rand((2, K), dtype=torch.float64, generator=twin).numpy())
    f = lambda x: logp(torch.as_tensor(x)).numpy()                                           # noqa: E731
    theta0 = np.zeros((K, d))
    st = dict(theta=theta0, logp=f(theta0), L=np.broadcast_to(np.linalg.cholesky(cov0), (K, d, d)).copy(), mean=theta0.copy(),
              scatter=np.zeros((K, d, d)), prop=np.zeros((2, K, d)), state=np.zeros(K, dtype=np.int64),
              accepted=np.zeros((2, K), dtype=np.int64), flags=np.zeros(K, dtype=np.int32))
    kw = dict(seed=seed, gamma=gamma, eps=eps, adapt_after=after, adapt_interval=every)
    st, rec = dram_np.step(st, np.zeros((2, K)), nxt=(zs[0][0], zs[0][1], None, None), **kw)
    assert rec is None
    outside = 0
    for t in range(1, n_steps + 1):
        lp = f(st['prop'].reshape(2 * K, d)).reshape(2, K)
        outside += int(np.isneginf(lp).sum())
        st, rec = dram_np.step(st, lp, now=(zs[t - 1][0], zs[t - 1][1], us[t - 1][0], us[t - 1][1]),
                               nxt=(zs[t][0], zs[t][1], None, None), **kw)
        ref.run(1, keep=False)
        assert np.array_equal(st['accepted'], ref.accepted.numpy()), t       # equal running counts: every decision equal
    assert np.all(st['state'] == n_steps + 1) and not st['flags'].any()
    assert st['accepted'][0].sum() > 0 and st['accepted'][1].sum() > 0 and outside > 0   # the bound was met
    worst = max(_scaled(st[k], getattr(ref, k).numpy()) for k in ('theta', 'logp', 'mean', 'scatter', 'L'))
    print(f'K = {K}, d = {d}, {n_steps} steps: worst scaled difference {worst:.3g}')
    assert worst <= 100.0 * MEASURED[(K, d)], worst


# --------------------------------------------------------------------------------------------------------- the Cholesky
def test_the_restated_cholesky_leaves_the_factor_alone_at_a_zero_pivot():
    rng = np.random.default_rng(1)
    B = rng.standard_normal((4, 4))
    good = B @ B.T + 4.0 * np.eye(4)
    singular = np.array([[4.0, 2.0, 0.0, 0.0], [2.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])   # second pivot 1 - 1 = 0
    zero = np.zeros((4, 4))
    old = np.tril(rng.standard_normal((3, 4, 4)))
    L, failed = dram_np.cholesky(np.stack([good, singular, zero]), old)
    assert failed.tolist() == [False, True, True]
    assert np.array_equal(L[1], old[1]) and np.array_equal(L[2], old[2])
    assert np.allclose(L[0], np.linalg.cholesky(good), rtol=1e-14, atol=0) and np.array_equal(L[0], np.tril(L[0]))
    # only the lower triangle is read, as torch.linalg.cholesky reads it
    upper_garbage = good.copy()
    upper_garbage[np.triu_indices(4, 1)] = 99.0
    assert np.array_equal(dram_np.cholesky(upper_garbage[None], old[:1])[0][0], L[0])
    # through a launch: a chain that never moved has zero scatter; with eps = 0 its adaptation fails, with eps > 0 it succeeds
    K, d = 2, 3
    st = dict(theta=np.ones((K, d)), logp=np.zeros(K), L=np.broadcast_to(np.eye(d), (K, d, d)).copy(), mean=np.ones((K, d)),
              scatter=np.zeros((K, d, d)), prop=np.zeros((2, K, d)), state=np.full(K, 4, dtype=np.int64),
              accepted=np.zeros((2, K), dtype=np.int64), flags=np.zeros(K, dtype=np.int32))
    lp = np.full((2, K), -np.inf)
    for eps, flag in ((0.0, 1), (1e-12, 0)):
        out, _ = dram_np.step(st, lp, seed=3, gamma=0.1, eps=eps, adapt_after=4, adapt_interval=2)
        assert out['flags'].tolist() == [flag, flag] and not out['accepted'].any()
        want = np.eye(d) if flag else np.sqrt((2.4 * 2.4) / d * eps) * np.eye(d)
        assert np.array_equal(out['L'], np.broadcast_to(want, (K, d, d)))
