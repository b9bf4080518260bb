"""optimize.NelderMead on the host (no GPU): the C ABI of pem_nm_step_f64_dev and what it refuses, the kernel's resources, the
numpy restatement of the launch (tests/nm_np.py) against scipy's own Nelder-Mead bit for bit, multi-start on a bounded
quadratic, the inverse prior transform, and what the driver refuses before it touches a device."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import nm_np
from hallthrusterpem_amd import _lib
from hallthrusterpem_amd.optimize import NelderMead, nm_coefficients, nm_simplex, quantile, search_bounds
from hallthrusterpem_amd.sampling import LOGUNIFORM, NORMAL, UNIFORM, Prior

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------------------------------- ABI and bindings
def test_the_entry_point_is_declared_bound_and_exported():
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    assert re.search(r'\bint pem_nm_step_f64_dev\(', header)
    assert 'pem_nm_step_f64_dev' in _lib.SIGNATURES
    assert getattr(_lib.load(), 'pem_nm_step_f64_dev') is not None
    assert len(_lib.SIGNATURES['pem_nm_step_f64_dev'][1]) == 23
    for name, value in (('PEM_NM_MAX_DIM', _lib.NM_MAX_DIM), ('PEM_NM_STATE_WORDS', _lib.NM_STATE_WORDS)):
        assert re.search(rf'#define {name} {value}\b', header), name
    assert _lib.NM_MAX_DIM == 32 and _lib.NM_STATE_WORDS == nm_np.STATE_WORDS == 10
    assert 'pem_nm.hip' in [s.name for s in __import__('hallthrusterpem_amd.build', fromlist=['SRCS']).SRCS]


def _call(**over):
    """pem_nm_step_f64_dev with valid host-side arguments (the device pointers are never followed: every case is refused
    before the device is looked at), one of them replaced"""
    d = over.pop('ndim', 3)
    n = max(d, 1)
    kw = dict(n_simplex=2, ndim=d, finalize=0, rho=1.0, chi=2.0, psi=0.5, sigma=0.5, xatol=1e-4, fatol=1e-4,
              kind=np.zeros(n, np.int32), a=np.zeros(n), b=np.ones(n), lb=np.zeros(n), ub=np.ones(n))
    dev = dict(sim=8, fsim=8, cand_x=8, cand_f=8, theta=8, state=8, history=None)   # non-NULL stand-ins
    hist_len = over.pop('history_len', 0)
    for k, v in over.items():
        (dev if k in dev else kw)[k] = v
    ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)              # noqa: E731
    dp = lambda v: None if v is None else C.c_void_p(v)                           # noqa: E731
    return _lib.load().pem_nm_step_f64_dev(kw['n_simplex'], kw['ndim'], kw['finalize'], kw['rho'], kw['chi'], kw['psi'], kw['sigma'],
                                           kw['xatol'], kw['fatol'], *(ptr(kw[k]) for k in ('kind', 'a', 'b', 'lb', 'ub')),
                                           *(dp(dev[k]) for k in ('sim', 'fsim', 'cand_x', 'cand_f', 'theta', 'state', 'history')),
                                           hist_len, None)


@pytest.mark.parametrize('over', [
    dict(n_simplex=0), dict(ndim=0), dict(ndim=33), dict(ndim=-1),
    dict(kind=None), dict(a=None), dict(b=None), dict(lb=None), dict(ub=None),
    dict(sim=None), dict(fsim=None), dict(cand_x=None), dict(cand_f=None), dict(theta=None), dict(state=None),
    dict(lb=np.array([0.0, 0.6, 0.0]), ub=np.array([1.0, 0.5, 1.0])), dict(lb=np.array([0.0, np.nan, 0.0])),
    dict(xatol=-1e-9), dict(fatol=-1.0), dict(xatol=float('nan')), dict(fatol=float('nan')),
    dict(history=8, history_len=0),
    dict(kind=np.array([0, 3, 0], np.int32)),
], ids=lambda o: '-'.join(o))
def test_the_entry_point_refuses_bad_arguments_before_looking_at_the_device(over):
    assert _call(**over) == _lib.PEM_ERR_INVALID_ARG, over


# ---------------------------------------------------------------------------------------------------- kernel resources
@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_nm_kernel_has_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_nm.hip')],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    assert list(rows) == ['nm_step_kernel'], rows
    r = rows['nm_step_kernel']
    assert r['sspill'] == 0 and r['vspill'] == 0 and r['scratch'] == 0, r


# ----------------------------------------------------------------------------------- the restatement against scipy
def _quadratic(d, seed, outside=False):
    """a correlated quadratic with condition number 100 over the unit cube; `outside` puts its optimum past a bound"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    A = Q @ np.diag(np.logspace(0.0, 2.0, d) if d > 1 else np.array([100.0])) @ Q.T
    xs = rng.uniform(0.2, 0.8, d)
    if outside:
        xs[d // 2] = 1.3
    return (lambda x: -0.5 * float((x - xs) @ A @ (x - xs))), np.zeros(d), np.ones(d)


def _rosenbrock(d):
    return (lambda x: -float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2))), np.full(d, -1.5), np.full(d, 1.2)


def _rough(d):
    return (lambda x: -float(np.sum(np.abs(x - 0.37)) + np.sum(np.sin(1000.0 * x) * np.cos(1700.0 * x[::-1])))), np.zeros(d), np.ones(d)


def _start(seed, d, lb, ub):
    return lb + (ub - lb) * np.random.default_rng(seed).uniform(0.1, 0.9, d)


def _cases():
    out = []
    for d in (1, 2, 3, 5, 12, 17, 32):
        out.append((f'quadratic-d{d}', _quadratic(d, d), dict(seed=d)))
        if d >= 2:                                       # in one dimension the Rosenbrock sum is empty
            out.append((f'rosenbrock-d{d}', _rosenbrock(d), dict(seed=d)))
    out.append(('quadratic-outside-d5', _quadratic(5, 50, outside=True), dict(seed=1)))
    out.append(('quadratic-outside-d12', _quadratic(12, 51, outside=True), dict(seed=2)))
    for d in (2, 3, 5, 8):
        for seed in (0, 1, 2):
            out.append((f'rough-d{d}-s{seed}', _rough(d), dict(seed=seed, rough=True)))
    out.append(('zero-component-d3', _quadratic(3, 7), dict(x0=np.array([0.4, 0.0, 0.7]))))
    out.append(('near-upper-bound-d3', _quadratic(3, 8), dict(x0=np.array([0.5, 0.97, 0.3]))))      # 0.97 > ub / 1.05
    out.append(('near-upper-bound-rosenbrock-d5', _rosenbrock(5), dict(x0=np.array([0.1, 1.19, -0.4, 1.16, 0.5]))))
    out.append(('not-adaptive-d5', _quadratic(5, 9), dict(seed=3, adaptive=False)))
    out.append(('not-adaptive-rough-d5', _rough(5), dict(seed=1, adaptive=False)))
    return out


CASES = _cases()


@pytest.mark.parametrize('name, problem, kw', CASES, ids=[c[0] for c in CASES])
def test_the_restatement_equals_scipy_bit_for_bit(name, problem, kw):
    """final_simplex (both halves), nit and nfev of scipy.optimize.minimize(method='Nelder-Mead', bounds=...).  scipy's argsort
    is not stable, so no case may ever sort two equal values: that is asserted."""
    from scipy.optimize import minimize
    f1, lb, ub = problem
    d = lb.size
    adaptive = kw.get('adaptive', True)
    x0 = kw['x0'] if 'x0' in kw else _start(kw['seed'], d, lb, ub)
    m = 200 * d if d <= 5 else 500                     # the larger ones end at maxiter, the smaller ones converge
    f = lambda X: np.array([f1(x) for x in X])         # noqa: E731  (row by row: the bits scipy's calls see)
    got = nm_np.minimize(f, x0, lb, ub, adaptive=adaptive, xatol=1e-4, fatol=1e-4, max_iterations=m)
    assert not got['ties'], 'two equal values met in a sort: choose another start'
    want = minimize(lambda x: -f1(x), x0, method='Nelder-Mead', bounds=list(zip(lb, ub)), tol=1e-4,
                    options=dict(adaptive=adaptive, maxiter=m, maxfev=10 ** 9))
    st = got['state'][0]
    assert int(st[nm_np.NIT]) == want.nit and int(st[nm_np.NFEV]) == want.nfev, (st, want.nit, want.nfev)
    assert np.array_equal(got['sim'][0], want.final_simplex[0])
    assert np.array_equal(-got['fsim'][0], want.final_simplex[1])
    assert bool(st[nm_np.STATUS]) == (want.status == 0) or want.nit == m
    assert int(got['operations'].sum()) == want.nit - 1


def test_the_rough_cases_take_every_operation_and_shrink_at_least_three_times_each():
    total = np.zeros(5, dtype=np.int64)
    for name, (f1, lb, ub), kw in CASES:
        if not kw.get('rough'):
            continue
        ops = nm_np.minimize(lambda X: np.array([f1(x) for x in X]), _start(kw['seed'], lb.size, lb, ub), lb, ub)['operations']
        assert ops[4] >= 3, (name, ops)
        total += ops
    assert np.all(total > 0), total


def test_coefficients_and_the_initial_simplex_are_the_restatements():
    for d in (1, 2, 5, 32):
        for adaptive in (True, False):
            assert tuple(nm_coefficients(d, adaptive)) == tuple(float(c) for c in nm_np.coefficients(d, adaptive))
    rng = np.random.default_rng(0)
    lb, ub = np.array([0.0, 0.0013, 0.0, 0.0]), np.array([1.0, 0.9987, 1.0, 1.0])
    x0 = np.array([[0.5, 0.99, 0.0, 0.2], [1.2, 0.5, 0.96, -0.1]])
    got = nm_simplex(x0, lb, ub)
    for s in range(2):
        assert np.array_equal(got[s], nm_np.initial_simplex(x0[s], lb, ub))
    sim = rng.uniform(-0.1, 1.1, (3, 5, 4))
    got = nm_simplex(None, lb, ub, sim)
    for s in range(3):
        assert np.array_equal(got[s], nm_np.initial_simplex(None, lb, ub, sim[s]))
    assert np.all((got >= lb) & (got <= ub))


# ------------------------------------------------------------------------------------------------------ stalled starts
def test_the_best_of_eight_starts_reaches_the_optimum_though_a_start_may_stall_on_a_face():
    """The quadratic of test_optimize_host.py::test_restated_search_reaches_the_optimum_of_a_correlated_gaussian from 8
    Latin-hypercube starts.  A bounded simplex can be clipped flat onto a face of the cube and stall there (scipy does the
    same, bit for bit), so single starts may end far from the optimum: that is allowed here, and it is why the driver runs
    many starts and reports `best`."""
    from oracle import sampler_np as snp
    d, S = 5, 8
    rng = np.random.default_rng(0)
    ustar = np.array([0.3, 0.62, 0.45, 0.8, 0.15])
    Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
    A = Q @ np.diag([1.0, 3.0, 10.0, 30.0, 100.0]) @ Q.T
    kind, a, b = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    starts = snp.sample(S, 0, 3, 0, kind, a, b, mode='lhs', n_total=S).T
    f = lambda X: -0.5 * np.einsum('ki,ij,kj->k', X - ustar, A, X - ustar)   # noqa: E731
    runs = [nm_np.minimize(f, starts[s], np.zeros(d), np.ones(d)) for s in range(S)]
    value = np.array([r['fsim'][0, 0] for r in runs])
    err = np.array([np.abs(r['sim'][0, 0] - ustar).max() for r in runs])
    print('max|u - ustar| per start', err, 'values', value)
    best = int(np.argmax(value))
    assert err[best] < 1e-4, err                      # (two of these eight starts stall, at 0.15 and 0.2 from the optimum)


# ------------------------------------------------------------------------------------------------------------ quantile
def test_quantile_inverts_the_prior_transform():
    """theta -> quantile -> theta again, to the tolerances of _theta_close in tests/test_optimize.py: uniform bit for bit (the
    priors here have b - a a power of two, so theta - a, the division and the way back are all exact), log-uniform to 4e-15
    relative, normal to 1e-12 absolute.  A log-uniform theta is exp(ln10 w) with w = a + (b - a) u, and the image of the
    transform is spaced by one ulp of ln10 w: for P_T ~ 1e-5 that is 1.8e-15, inside the tolerance; for c4 ~ 1e20 the
    argument is 41 ... 51 and its ulp alone is 7.1e-15, so the round trip can land on the neighbouring image point.  For that
    prior the bound is that spacing plus the 4e-15 of the exponential: 1.2e-14."""
    from oracle import sampler_np as snp
    names = ('T_e', 'P_T', 'V_vac', 'c0', 'c4')
    pri = {'T_e': Prior(UNIFORM, 1.0, 5.0, 't'), 'P_T': Prior(LOGUNIFORM, -6.0, -4.0, 't'), 'V_vac': Prior(NORMAL, 30.0, 2.0, 't'),
           'c0': Prior(UNIFORM, 0.0, 1.0, 't'), 'c4': Prior(LOGUNIFORM, 18.0, 22.0, 't')}
    fwd = lambda u: np.stack([snp.transform(pri[k].kind, pri[k].a, pri[k].b, u[:, j]) for j, k in enumerate(names)], 1)  # noqa: E731
    rng = np.random.default_rng(1)
    u = rng.uniform(0.002, 0.998, (500, 5))
    u[0], u[1] = [0.0, 0.0, 0.5, 0.0, 0.0], [1.0, 1.0, 0.5, 1.0, 1.0]
    theta = fwd(u)
    back = quantile(theta, names, pri)
    assert back.shape == u.shape
    again = fwd(back)
    assert np.array_equal(again[:, 0], theta[:, 0]) and np.array_equal(again[:, 3], theta[:, 3])
    assert np.array_equal(back[:, 3], u[:, 3])                                                       # U(0, 1): u itself
    assert np.max(np.abs(again[:, 1] / theta[:, 1] - 1)) < 4e-15
    assert np.max(np.abs(again[:, 2] - theta[:, 2])) < 1e-12
    assert np.max(np.abs(again[:, 4] / theta[:, 4] - 1)) < 1.2e-14
    assert np.max(np.abs(back - u)) < 1e-13
    assert quantile(theta[:7].reshape(7, 1, 5), names, pri).shape == (7, 1, 5)
    lb, ub = search_bounds(names, pri)
    assert np.array_equal(lb[[0, 1, 3, 4]], np.zeros(4)) and np.array_equal(ub[[0, 1, 3, 4]], np.ones(4))
    assert abs(lb[2] - 0.0013498980316300946) < 2e-18 and abs(ub[2] - 0.9986501019683699) < 2e-16
    with pytest.raises(ValueError, match='one entry per name'):
        quantile(np.zeros(3), names, pri)
    with pytest.raises(KeyError, match='no prior'):
        quantile(np.zeros(1), ('nope',), pri)


# ---------------------------------------------------------------------------------------------- driver argument checks
def _f(theta):
    raise AssertionError('f must not be called')


@pytest.mark.parametrize('kw, err, match', [
    (dict(names=()), ValueError, 'distinct'),
    (dict(names=tuple(f'x{i}' for i in range(33))), ValueError, 'at most 32'),
    (dict(names=('T_e', 'T_e')), ValueError, 'distinct'),
    (dict(names=('T_e', 'nope')), KeyError, 'no prior'),
    (dict(names=('T_e', 'c0'), x0=[3.0, 0.5, 1.0]), ValueError, 'x0 must have'),
    (dict(names=('T_e', 'c0'), x0=np.zeros((2, 3))), ValueError, 'x0 must have'),
    (dict(names=('T_e', 'c0'), initial_simplex=np.ones((2, 2))), ValueError, 'initial_simplex must have'),
    (dict(names=('T_e', 'c0'), initial_simplex=np.ones((4, 2, 2))), ValueError, 'initial_simplex must have'),
    (dict(names=('T_e', 'c0'), x0=[3.0, 0.5], n_starts=4), ValueError, 'at most one'),
    (dict(names=('T_e', 'c0'), x0=[3.0, 0.5], initial_simplex=np.ones((3, 2))), ValueError, 'at most one'),
    (dict(names=('T_e', 'c0'), n_starts=2, initial_simplex=np.ones((3, 2))), ValueError, 'at most one'),
    (dict(names=('T_e', 'c0'), n_starts=0), ValueError, 'n_starts'),
    (dict(names=('T_e', 'c4'), x0=[3.0, -1e20]), ValueError, 'no finite quantile'),                  # log10 of a negative
    (dict(names=('T_e', 'c4'), x0=[float('nan'), 1e20]), ValueError, 'no finite quantile'),
    (dict(names=('T_e', 'c4'), x0=[[3.0, 1e20], [3.0, 0.0]]), ValueError, 'no finite quantile'),             # log10(0) = -inf
    (dict(names=('T_e', 'c4'), initial_simplex=[[3.0, 1e20], [3.1, 1e20], [3.0, float('nan')]]), ValueError, 'no finite quantile'),
    (dict(names=('T_e', 'c0'), xatol=-1e-4), ValueError, 'xatol'),
    (dict(names=('T_e', 'c0'), fatol=-1e-4), ValueError, 'fatol'),
    (dict(names=('T_e', 'c0'), fatol=float('nan')), ValueError, 'fatol'),
])
def test_nm_driver_rejects_bad_arguments_before_touching_a_device(kw, err, match, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    with pytest.raises(err, match=match):
        NelderMead(_f, **kw)
