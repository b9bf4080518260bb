"""optimize on the host (no GPU): the C ABI of pem_de_step_f64_dev, the kernel's resources, what the drivers refuse before they
touch a device, the central-difference Hessian on a closed-form Gaussian, the nearest positive-definite matrix, the stencil,
and the numpy restatement of the DE launch (tests/de_np.py) driving a search to the optimum."""
import math
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from hallthrusterpem_amd import _lib
from hallthrusterpem_amd.optimize import (DifferentialEvolution, Laplace, hessian, is_positive_definite, nearest_positive_definite,
                                          slice_points, stencil, stencil_size, theta_steps)
from hallthrusterpem_amd.sampling import NORMAL, PEM_V0_PRIORS, Prior

ROOT = Path(__file__).resolve().parents[1]
GAUSS_NAMES = ('T_e', 'V_vac', 'P_T', 'c0', 'c4')


def test_the_new_entry_point_is_declared_bound_and_exported():
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    assert re.search(r'\bint pem_de_step_f64_dev\(', header)
    assert 'pem_de_step_f64_dev' in _lib.SIGNATURES
    assert getattr(_lib.load(), 'pem_de_step_f64_dev') is not None
    assert len(_lib.SIGNATURES['pem_de_step_f64_dev'][1]) == 23
    for name, value in (('PEM_DE_MAX_POP', _lib.DE_MAX_POP), ('PEM_DE_MAX_DIM', _lib.DE_MAX_DIM),
                        ('PEM_DE_BEST1BIN', _lib.DE_BEST1BIN), ('PEM_DE_RAND1BIN', _lib.DE_RAND1BIN)):
        assert re.search(rf'#define {name} {value}\b', header), name
    assert 'pem_de.hip' in [s.name for s in __import__('hallthrusterpem_amd.build', fromlist=['SRCS']).SRCS]


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_de_kernel_has_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_de.hip')],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    assert list(rows) == ['de_step_kernel'], rows
    r = rows['de_step_kernel']                  # 1024 threads = 4 waves per SIMD: at most 128 registers
    assert r['sspill'] == 0 and r['vspill'] == 0 and r['scratch'] == 0 and r['vgpr'] <= 128, r


def _f(theta):
    raise AssertionError('f must not be called')


@pytest.mark.parametrize('kw, err, match', [
    (dict(names=('T_e',), popsize=3), ValueError, r'\[4, 1024\]'),           # P = 3
    (dict(names=('T_e', 'c0'), popsize=513), ValueError, r'\[4, 1024\]'),    # P = 1026
    (dict(names=tuple(f'x{i}' for i in range(17))), ValueError, 'at most 16'),
    (dict(names=('T_e', 'T_e')), ValueError, 'distinct'),
    (dict(names=('T_e', 'nope')), KeyError, 'no prior'),
    (dict(names=('T_e', 'c0'), strategy='best2bin'), ValueError, 'strategy'),
    (dict(names=('T_e', 'c0'), mutation=(1.0, 0.5)), ValueError, 'mutation'),
    (dict(names=('T_e', 'c0'), recombination=1.5), ValueError, 'recombination'),
])
def test_de_driver_rejects_bad_arguments_before_touching_a_device(kw, err, match, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    with pytest.raises(err, match=match):
        DifferentialEvolution(_f, **kw)


def test_shared_nuisance_with_fresh_nuisance_is_refused_before_touching_a_device(monkeypatch):
    from hallthrusterpem_amd import calibration
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    monkeypatch.setattr(calibration, 'CoupledBatch', lambda *a, **k: pytest.fail('touched a device'))
    rng = np.random.default_rng(0)
    x = np.stack([10.0 ** rng.uniform(-6, -4.5, 2), rng.uniform(250, 350, 2), rng.uniform(4e-6, 6e-6, 2)], 1)
    lik = SystemLikelihood({'V_cc': {'x': x, 'y': rng.uniform(15, 35, 2), 'var_y': np.ones(2)}}, device='cpu')
    with pytest.raises(ValueError, match='fresh_nuisance=False'):
        calibration.SystemPosterior(('T_e',), lik, n_chains=4, shared_nuisance=True)
    with pytest.raises(ValueError, match='fresh_nuisance=False'):
        calibration.JionPosterior(('c0',), x, np.zeros((2, 3)), np.ones((2, 3)), np.ones((2, 3)), n_chains=4,
                                  shared_nuisance=True, device='cpu')


@pytest.mark.parametrize('bounds, match', [
    ([(0.5, 6.0), (0.0, 60.0)], "'T_e'"),                 # T_e ~ U(1, 5)
    ([(1.0, 5.0), (-1.0, 60.0)], "'V_vac'"),
    ([(3.0, 2.0), (0.0, 60.0)], "'T_e'"),                 # not an interval
])
def test_slice_bounds_outside_the_prior_support_are_refused(bounds, match):
    with pytest.raises(ValueError, match=match):
        slice_points(('T_e', 'V_vac'), [3.0, 30.0], 5, bounds)


def test_slice_points_sweep_one_axis_at_a_time_over_the_support():
    pri = dict(PEM_V0_PRIORS, V_vac=Prior(NORMAL, 30.0, 2.0, 'test'))
    x0 = np.array([3.0, 30.0, 1e20])
    rows = slice_points(('T_e', 'V_vac', 'c4'), x0, 4, priors=pri)
    assert rows.shape == (12, 3)
    assert np.array_equal(rows[0:4, 0], np.linspace(1.0, 5.0, 4)) and np.all(rows[0:4, 1:] == x0[1:])
    assert np.allclose(rows[4:8, 1], [24.0, 28.0, 32.0, 36.0]) and np.all(rows[4:8, [0, 2]] == x0[[0, 2]])
    assert np.allclose(rows[8:12, 2], [1e18, 1e19 * 10 ** (1 / 3), 1e21 / 10 ** (1 / 3), 1e22], rtol=1e-12)
    assert rows[8, 2] == 1e18 and rows[11, 2] == 1e22


def test_stencil_is_2d2_plus_1_rows():
    for d in (1, 2, 5, 12):
        t = np.arange(1.0, d + 1)
        h = 0.1 * np.arange(1.0, d + 1)
        pts = stencil(t, h)
        assert pts.shape == (stencil_size(d), d) == (2 * d * d + 1, d)
        assert np.array_equal(pts[0], t)
        assert len({tuple(p) for p in pts}) == pts.shape[0]                 # no point twice
        assert np.allclose(np.abs(pts - t).sum(1)[1:1 + 2 * d], np.repeat(h, 2))


def test_steps_follow_the_prior_transform():
    pri = dict(PEM_V0_PRIORS, V_vac=Prior(NORMAL, 30.0, 2.0, 'test'))
    h = theta_steps([3.0, 32.0, 1e20], ('T_e', 'V_vac', 'c4'), pri, step=1e-3)
    z = 1.0
    assert np.allclose(h, 1e-3 * np.array([4.0, 2.0 * math.sqrt(2 * math.pi) * math.exp(0.5 * z * z), 1e20 * math.log(10) * 4.0]),
                       rtol=1e-14)


def _gaussian(scale):
    rng = np.random.default_rng(5)
    C = rng.standard_normal((5, 5))
    corr = C @ C.T + 5 * np.eye(5)
    sd = np.sqrt(np.diag(corr))
    corr = corr / np.outer(sd, sd)
    sigma = np.outer(scale * 0.05, scale * 0.05) * corr
    return sigma


def test_hessian_recovers_a_gaussian_covariance_over_twelve_decades():
    import torch
    scale = np.array([1.0, 10.0, 1e-5, 1.0, 1e20])                     # T_e, V_vac, P_T, c0, c4
    mu = np.array([3.0, 30.0, 5e-5, 0.5, 1e20])
    sigma = _gaussian(scale)
    prec = torch.as_tensor(np.linalg.inv(sigma / np.outer(scale, scale)))  # inverted in scaled units, where it is well conditioned
    mu_t = torch.as_tensor(mu)
    calls = []

    def f(theta):
        calls.append(theta.shape)
        dd = (theta - mu_t) / torch.as_tensor(scale)
        return -0.5 * torch.einsum('ki,ij,kj->k', dd, prec, dd)

    H = hessian(f, mu, GAUSS_NAMES)
    assert calls == [(stencil_size(5), 5)]                                # ONE call over the whole stencil
    lap = Laplace(mu, H)
    err = np.abs(lap.cov - sigma) / np.sqrt(np.outer(np.diag(sigma), np.diag(sigma)))
    assert err.max() <= 1e-6, err.max()
    assert not lap.nearest_pd and np.array_equal(lap.cov, lap.cov.T) and is_positive_definite(lap.cov)
    theta0, cov0 = lap.dram_start()
    assert np.array_equal(theta0, mu) and np.array_equal(cov0, lap.cov)
    s = lap.sample(20000, seed=1)
    assert s.shape == (20000, 5)
    assert np.all(np.abs(s.mean(0) - mu) < 0.05 * np.sqrt(np.diag(sigma)))
    assert np.array_equal(lap.sample(10, seed=3), lap.sample(10, seed=3))


def test_hessian_refuses_a_stencil_outside_the_support():
    with pytest.raises(ValueError, match="'c0'"):
        hessian(_f, [3.0, 30.0, 5e-5, 1.0, 1e20], GAUSS_NAMES)             # c0 ~ U(0, 1) at its bound
    with pytest.raises(ValueError, match="'c4'"):
        hessian(_f, [3.0, 30.0, 5e-5, 0.5, 1e22], GAUSS_NAMES)


def test_nearest_positive_definite():
    rng = np.random.default_rng(2)
    Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    indefinite = Q @ np.diag([3.0, 2.0, 1.0, 0.5, -0.2, -1e-3]) @ Q.T
    assert not is_positive_definite(indefinite)
    X = nearest_positive_definite(indefinite)
    assert is_positive_definite(X) and np.array_equal(X, X.T)
    assert np.linalg.norm(X - indefinite) < 0.3                          # the negative part is removed, little else
    pd = Q @ np.diag([3.0, 2.0, 1.0, 0.5, 0.2, 1e-3]) @ Q.T
    pd = 0.5 * (pd + pd.T)
    assert np.array_equal(nearest_positive_definite(pd), pd)
    lap = Laplace(np.zeros(6), -np.linalg.pinv(indefinite))               # cov = pinv(-H) = indefinite
    assert lap.nearest_pd and is_positive_definite(lap.cov)


def test_restated_search_reaches_the_optimum_of_a_correlated_gaussian():
    """tests/de_np.py driving best1bin and rand1bin to the maximum: the algorithm the GPU tests hold the kernel to"""
    import de_np
    from oracle import sampler_np as snp
    d, P = 5, 75
    rng = np.random.default_rng(0)
    ustar = np.array([0.3, 0.62, 0.45, 0.8, 0.15])
    Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    A = Q @ np.diag([1.0, 3.0, 10.0, 30.0, 100.0]) @ Q.T
    kind, a, b = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    for strategy, gens, want in ((de_np.BEST1BIN, 200, 1e-6), (de_np.RAND1BIN, 200, 1e-3)):
        pop_u, pop_f, trial_f = np.zeros((P, d)), np.zeros(P), np.zeros(P)
        trial_u = snp.sample(P, 0, 3, 0, kind, a, b, mode='lhs', n_total=P).T.copy()
        g = 0
        for _ in range(gens + 1):
            o = de_np.step(g, P, d, strategy, False, 3, (0.5, 1.0), 0.7, 0.01, 0.0, kind, a, b, pop_u, pop_f, trial_u, trial_f)
            pop_u, pop_f, trial_u, g = o['pop_u'], o['pop_f'], o['trial_u'], o['state']
            dd = o['theta'] - ustar
            trial_f = -0.5 * np.einsum('ki,ij,kj->k', dd, A, dd)
        o = de_np.step(g, P, d, strategy, True, 3, (0.5, 1.0), 0.7, 0.01, 0.0, kind, a, b, pop_u, pop_f, trial_u, trial_f)
        assert np.abs(o['pop_u'][int(o['record'][1])] - ustar).max() < want, strategy
