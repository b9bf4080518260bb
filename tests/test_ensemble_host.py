"""The affine-invariant ensemble sampler without a GPU: pem_ensemble_step_f64_dev is declared, bound, built and exported, refuses
every malformed call before it looks for a device and compiles without scratch; DeviceEnsemble refuses what it cannot run before
it touches a device; the numpy restatement of the launch (tests/ensemble_np.py) has the algorithm's own exact properties: its
trace scales bit for bit with the parameters, it recovers a correlated Gaussian, and its rare outcomes are the stated ones.

    python tests/test_ensemble_host.py        prints the errors of a plain Goodman-Weare sampler that MEAN_TOL / COV_TOL come from
"""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAME = 'pem_ensemble_step_f64_dev'


def test_the_entry_point_is_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % NAME, header)
    assert m and len(m.group(1).split(',')) == 22
    assert len(_lib.SIGNATURES[NAME][1]) == 22
    assert hasattr(_lib.load(), NAME)
    assert re.search(r'#define PEM_ENSEMBLE_MAX_DIM (\d+)', header).group(1) == str(_lib.ENSEMBLE_MAX_DIM) == '32'
    assert re.search(r'#define PEM_ENSEMBLE_MAX_WALKERS (\d+)', header).group(1) == str(_lib.ENSEMBLE_MAX_WALKERS) == '1024'
    assert build.PKG / 'csrc' / 'pem_ensemble.hip' in build.SRCS


FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host
ARRAYS = ('theta', 'logp', 'prop', 'prop_logp', 'log_q', 'state', 'accepted', 'trace', 'logp_trace', 'draws')
OPTIONAL = ('trace', 'logp_trace', 'draws')


def _call(E=2, K=8, d=3, seed=1, a=2.0, de_fraction=0.5, g0=0.9, sigma=1e-5, trace_first=0, trace_len=8, thin=1, **null):
    from hallthrusterpem_amd import _lib
    ptrs = [None if null.get(n, n in ('logp_trace', 'draws')) else FAKE for n in ARRAYS]      # name=True: that array is NULL
    return _lib.load().pem_ensemble_step_f64_dev(E, K, d, seed, a, de_fraction, g0, sigma, trace_first, trace_len, thin, *ptrs, None)


NAN, INF = float('nan'), float('inf')


@pytest.mark.parametrize('bad', [
    dict(E=0), dict(K=7), dict(K=0), dict(K=1), dict(K=-2), dict(K=1026), dict(K=2, d=1, de_fraction=0.5), dict(K=2, d=1, de_fraction=1.0),
    dict(d=0), dict(d=-1), dict(d=33), dict(a=1.0), dict(a=0.5), dict(a=NAN), dict(a=INF), dict(de_fraction=-0.1),
    dict(de_fraction=1.5), dict(de_fraction=NAN), dict(g0=0.0), dict(g0=-1.0), dict(g0=NAN), dict(g0=INF), dict(sigma=-1e-5),
    dict(sigma=NAN), dict(sigma=INF), dict(thin=0), dict(trace_len=0),
    dict(trace_len=0, trace=True, logp_trace=False),                     # a logp trace alone needs rows as well
] + [{n: True} for n in ARRAYS if n not in OPTIONAL])
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_ensemble_step' in _lib.load().pem_last_error()


def test_a_well_formed_call_gets_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _call() == _lib.PEM_ERR_NO_DEVICE
    assert _call(trace=True, trace_len=0) == _lib.PEM_ERR_NO_DEVICE      # no trace: trace_len is not looked at
    assert _call(E=1, K=2, d=1, de_fraction=0.0) == _lib.PEM_ERR_NO_DEVICE
    assert _call(K=1024, d=32, de_fraction=1.0, sigma=0.0) == _lib.PEM_ERR_NO_DEVICE


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_ensemble_kernel_cross_compiles_without_scratch_and_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'),
                          str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_ensemble.hip')], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+) kernarg\s+(\d+) lds\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)),
                                    lds=int(m.group(8)))
    assert list(rows) == ['ensemble_step_kernel'], rows
    r = rows['ensemble_step_kernel']            # decisions and partners of up to 512 moving walkers in LDS
    assert r['sspill'] == 0 and r['vspill'] == 0 and r['scratch'] == 0 and r['lds'] <= 16 * 1024, r


def _f(theta):
    raise AssertionError('log_posterior must not be called')


@pytest.mark.parametrize('kw, match', [
    (dict(theta0=np.zeros((7, 2))), 'even number of walkers'),
    (dict(theta0=np.zeros((2, 7, 2))), 'even number of walkers'),
    (dict(theta0=np.zeros((8, 5))), '2 d = 10 <= K'),
    (dict(theta0=np.zeros((80, 33))), '1 to 32 parameters'),
    (dict(theta0=np.zeros((1026, 3))), 'K <= 1024'),
    (dict(theta0=np.zeros((8, 3)), device='cpu'), 'GPU only'),
    (dict(theta0='tensor'), 'GPU only'),                                  # a CPU tensor as the start points
    (dict(theta0=np.zeros((8, 3)), de_fraction=-0.1), r'de_fraction must be in \[0, 1\]'),
    (dict(theta0=np.zeros((8, 3)), de_fraction=1.1), r'de_fraction must be in \[0, 1\]'),
    (dict(theta0=np.zeros((8, 3)), de_fraction=float('nan')), r'de_fraction must be in \[0, 1\]'),
    (dict(theta0=np.zeros((2, 1)), de_fraction=0.5), 'K >= 4'),
    (dict(theta0=np.zeros((8, 3)), a=1.0), 'a > 1'),
    (dict(theta0=np.zeros((8, 3)), n_ensembles=2), r'\(E, K, d\)'),
    (dict(theta0=np.zeros(3)), r'\(E, K, d\)'),
])
def test_the_driver_refuses_what_it_cannot_run_before_touching_a_device(kw, match, monkeypatch):
    import torch
    from hallthrusterpem_amd.calibration import DeviceEnsemble
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    if isinstance(kw['theta0'], str):
        kw = dict(kw, theta0=torch.zeros((8, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match=match):
        DeviceEnsemble(_f, **kw)


def test_ball_draws_its_starts_from_default_rng():
    from hallthrusterpem_amd.calibration import DeviceEnsemble
    c, s = np.array([1.0, -2.0, 1e20]), np.array([0.1, 0.2, 1e18])
    got = DeviceEnsemble.ball(c, s, 6, n_ensembles=2, seed=5)
    assert got.shape == (2, 6, 3)
    assert np.array_equal(got, c + s * np.random.default_rng(5).standard_normal((2, 6, 3)))
    assert DeviceEnsemble.ball(c, 0.5, 4).shape == (1, 4, 3)


# --------------------------------------------------------------------------------------------- the restatement is the algorithm
MU = np.array([1.0, -2.0, 0.5, 3.0, -1.0])
STD = np.array([1.0, 0.9, 1.1, 1.0, 0.95])
SIGMA = np.outer(STD, STD) * 0.7 ** np.abs(np.subtract.outer(np.arange(5), np.arange(5)))
PREC = np.linalg.inv(SIGMA)
E_G, K_G, N_G, BURN_G = 4, 32, 2500, 500
# twice the largest error of the plain sampler below over seeds 101 ... 108 and de_fraction 0, 1, 0.5 (its output is in the
# docstring of test_the_restatement_recovers_a_correlated_gaussian)
MEAN_TOL, COV_TOL = 2 * 0.0364, 2 * 0.0352


def gaussian_logp(x):
    r = x - MU
    return -0.5 * np.einsum('ki,ij,kj->k', r, PREC, r)


def moment_errors(trace):
    """(largest error of a mean, largest error of a covariance entry) of the pooled rows after the burn-in"""
    flat = np.asarray(trace)[BURN_G:].reshape(-1, MU.size)
    return float(np.max(np.abs(flat.mean(axis=0) - MU))), float(np.max(np.abs(np.cov(flat.T) - SIGMA)))


def plain_goodman_weare(logp, x0, n_steps, rng, a=2.0, de_fraction=0.0, sigma=1e-5, drop_weight=False):
    """Goodman & Weare's sampler as its paper and emcee's documentation state it, written without tests/ensemble_np.py and on
    numpy's own generator: x0 (K, d); the halves take turns; the half's move is DE with probability de_fraction.  drop_weight
    leaves z^(d - 1) out (the mistake the tolerance must catch).  Returns the (n_steps, K, d) trace."""
    x = np.array(x0, dtype=np.float64)
    K, d = x.shape
    H = K // 2
    lp = logp(x)
    g0 = 2.38 / np.sqrt(2 * d)
    out = np.empty((n_steps, K, d))
    for t in range(n_steps):
        for half in (0, 1):
            mine = slice(0, H) if half == 0 else slice(H, K)
            other = x[H:] if half == 0 else x[:H]
            if rng.random() < de_fraction:
                pairs = np.array([rng.choice(H, size=2, replace=False) for _ in range(H)])
                g = g0 * (1.0 + sigma * rng.standard_normal(H))
                y = x[mine] + g[:, None] * (other[pairs[:, 0]] - other[pairs[:, 1]])
                log_q = np.zeros(H)
            else:
                z = ((a - 1.0) * rng.random(H) + 1.0) ** 2 / a
                partner = other[rng.integers(0, H, size=H)]
                y = partner + z[:, None] * (x[mine] - partner)
                log_q = np.zeros(H) if drop_weight else (d - 1) * np.log(z)
            lp_y = logp(y)
            accept = np.log(rng.random(H)) < log_q + lp_y - lp[mine]
            x[mine] = np.where(accept[:, None], y, x[mine])
            lp[mine] = np.where(accept, lp_y, lp[mine])
        out[t] = x
    return out


def _starts(seed):
    return np.random.default_rng(seed).standard_normal((E_G, K_G, MU.size))


@pytest.mark.parametrize('de_fraction', [0.0, 1.0])
def test_the_restatement_is_affine_invariant_bit_for_bit(de_fraction):
    """each coordinate scaled by a power of two, the target scaled the same way: every product and sum of the launch scales
    exactly and every decision is the same, so the trace is the unscaled trace times the scale, bit for bit"""
    import ensemble_np
    scale = 2.0 ** np.array([-60.0, 66.0, 0.0, 13.0, -7.0])
    x0 = np.random.default_rng(3).standard_normal((2, 10, 5)) + MU
    kw = dict(n_steps=300, seed=11, de_fraction=de_fraction)
    plain = ensemble_np.run(gaussian_logp, x0, **kw)
    scaled = ensemble_np.run(lambda x: gaussian_logp(x / scale), x0 * scale, **kw)
    assert plain['trace'].shape == (300, 2, 10, 5) and not np.isnan(plain['trace']).any()
    assert np.array_equal(scaled['trace'], plain['trace'] * scale)
    assert np.array_equal(scaled['logp_trace'], plain['logp_trace']) and np.array_equal(scaled['accepted'], plain['accepted'])
    acc = plain['accepted'].mean() / 300
    assert 0.1 < acc < 0.9, acc                                          # it moved, and it refused


@pytest.mark.parametrize('de_fraction', [0.0, 1.0, 0.5])
def test_the_restatement_recovers_a_correlated_gaussian(de_fraction):
    """d = 5, E = 4, K = 32, 2500 steps, the first 500 dropped; the pooled mean within MEAN_TOL and the pooled covariance within
    COV_TOL, entry by entry.  The tolerances are twice the largest error of `plain_goodman_weare` (above: numpy's generator,
    nothing of ensemble_np) on the same target, shape and schedule over 8 other seeds and the three move mixtures:

        python tests/test_ensemble_host.py
        de_fraction 0.0: mean error 0.0105 ... 0.0364 (seed 107), covariance error 0.0164 ... 0.0352 (seed 105)
        de_fraction 1.0: mean error 0.0059 ... 0.0262 (seed 106), covariance error 0.0063 ... 0.0172 (seed 108)
        de_fraction 0.5: mean error 0.0094 ... 0.0268 (seed 106), covariance error 0.0073 ... 0.0183 (seed 105)
        largest: mean 0.0364 covariance 0.0352 -> MEAN_TOL 0.073 COV_TOL 0.070 (limit 0.243)
        without z^(d-1), de_fraction 0.0: variances / truth [0.34 0.34 0.36 0.34 0.34] covariance error 0.770
        without z^(d-1), de_fraction 0.5: variances / truth [0.6  0.6  0.58 0.58 0.57] covariance error 0.505

    COV_TOL stays below 0.3 x the smallest variance (0.81), so a sampler that drops z^(d - 1) -- whose variances the same
    command measures at about a third of the truth -- fails."""
    import ensemble_np
    assert COV_TOL < 0.3 * SIGMA.diagonal().min()
    st = ensemble_np.run(gaussian_logp, _starts(1), N_G, seed=2, de_fraction=de_fraction)
    mean_err, cov_err = moment_errors(st['trace'])
    acc = st['accepted'].mean() / N_G
    print(f'de_fraction {de_fraction}: mean error {mean_err:.4f}, covariance error {cov_err:.4f}, acceptance {acc:.3f}')
    assert mean_err <= MEAN_TOL and cov_err <= COV_TOL, (mean_err, cov_err)
    assert 0.1 < acc < 0.9, acc


def test_the_restatement_handles_the_rare_outcomes():
    """a walker that starts at -inf takes the first finite proposal; a NaN proposal never enters; -inf is never accepted"""
    import ensemble_np
    E, K, d = 1, 8, 2
    H = K // 2
    rng = np.random.default_rng(4)
    theta = rng.standard_normal((E, K, d))
    logp = np.zeros((E, K))
    logp[0, 1] = -np.inf
    st = dict(theta=theta, logp=logp, prop=np.zeros((E, H, d)), log_q=np.zeros((E, H)), state=np.zeros(E, dtype=np.int64),
              accepted=np.zeros((E, K), dtype=np.int64))
    st, rec, _ = ensemble_np.step(st, np.zeros((E, H)), seed=9)
    assert rec is None and np.array_equal(st['theta'], theta)
    # half-step 1 moves half 0: walker 0 is offered NaN, walker 1 (at -inf) a very low finite value, walker 2 -inf, walker 3 +1e3
    lp = np.array([[np.nan, -1e300, -np.inf, 1e3]])
    prop = st['prop'].copy()
    st, rec, _ = ensemble_np.step(st, lp, seed=9)
    assert rec['acc'].tolist() == [[False, True, False, True]]
    assert np.array_equal(st['theta'][0, [0, 2]], theta[0, [0, 2]]) and np.array_equal(st['theta'][0, [1, 3]], prop[0, [1, 3]])
    assert st['logp'][0, :4].tolist() == [0.0, -1e300, 0.0, 1e3] and st['accepted'][0].tolist() == [0, 1, 0, 1, 0, 0, 0, 0]
    assert np.array_equal(st['theta'][0, H:], theta[0, H:])             # the other half stood still
    # NaN as the CURRENT value is never left either (both sides of the comparison are NaN): the constructor refuses such starts
    st['logp'][0, H] = np.nan
    st, rec, _ = ensemble_np.step(st, np.full((E, H), 1e3), seed=9)
    assert rec['acc'].tolist() == [[False, True, True, True]]


if __name__ == '__main__':
    worst_mean = worst_cov = 0.0
    for fraction in (0.0, 1.0, 0.5):
        for seed in range(101, 109):
            rng = np.random.default_rng(seed)
            trace = np.stack([plain_goodman_weare(gaussian_logp, rng.standard_normal((K_G, MU.size)), N_G, rng, de_fraction=fraction)
                              for _ in range(E_G)], axis=1)
            m, c = moment_errors(trace)
            worst_mean, worst_cov = max(worst_mean, m), max(worst_cov, c)
            print(f'de_fraction {fraction} seed {seed}: mean error {m:.4f} covariance error {c:.4f}')
    print(f'largest: mean {worst_mean:.4f} covariance {worst_cov:.4f} -> MEAN_TOL {2 * worst_mean:.3f} COV_TOL {2 * worst_cov:.3f} '
          f'(limit {0.3 * SIGMA.diagonal().min():.3f})')
    for fraction in (0.0, 0.5):
        rng = np.random.default_rng(101)
        trace = np.stack([plain_goodman_weare(gaussian_logp, rng.standard_normal((K_G, MU.size)), N_G, rng, de_fraction=fraction,
                                              drop_weight=True) for _ in range(E_G)], axis=1)
        flat = trace[BURN_G:].reshape(-1, MU.size)
        print(f'without z^(d-1), de_fraction {fraction}: variances / truth {np.round(np.cov(flat.T).diagonal() / SIGMA.diagonal(), 2)} '
              f'covariance error {moment_errors(trace)[1]:.3f}')
