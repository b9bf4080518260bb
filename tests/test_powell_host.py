"""optimize.Powell on the host (no GPU): the numpy restatement of the launch (tests/powell_np.py) against scipy's own bounded
Powell bit for bit -- every evaluated point in order, x, fun, nit, nfev and direc --, the branches of the algorithm those
functions do not reach driven by constructed inputs, hostile values, the C ABI of pem_powell_step_f64_dev and what it refuses,
the kernel's resources, and what the drivers refuse before they touch a device."""
import ctypes as C
import re
import shutil
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

import powell_np as pn
from hallthrusterpem_amd import _lib
from hallthrusterpem_amd.optimize import DifferentialEvolution, Powell
from test_nelder_mead_host import _quadratic, _rosenbrock, _rough, _start

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------------------------------- ABI and bindings
def test_the_entry_point_is_declared_bound_and_exported():
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    assert re.search(r'\bint pem_powell_step_f64_dev\(', header)
    assert 'pem_powell_step_f64_dev' in _lib.SIGNATURES
    assert getattr(_lib.load(), 'pem_powell_step_f64_dev') is not None
    assert len(_lib.SIGNATURES['pem_powell_step_f64_dev'][1]) == 22
    for name, value in (('PEM_POWELL_MAX_DIM', _lib.POWELL_MAX_DIM), ('PEM_POWELL_STATE_WORDS', _lib.POWELL_STATE_WORDS),
                        ('PEM_POWELL_SCALARS', _lib.POWELL_SCALARS), ('PEM_POWELL_VEC_ROWS', _lib.POWELL_VEC_ROWS)):
        assert re.search(rf'#define {name} {value}\b', header), name
    assert _lib.POWELL_MAX_DIM == 32 and _lib.POWELL_STATE_WORDS == pn.STATE_WORDS == 24
    assert _lib.POWELL_SCALARS == pn.SCALARS == 20 and _lib.POWELL_VEC_ROWS == pn.VEC_ROWS == 6
    assert 'pem_powell.hip' in [s.name for s in __import__('hallthrusterpem_amd.build', fromlist=['SRCS']).SRCS]
    from hallthrusterpem_amd.optimize import POWELL_COUNTERS
    assert POWELL_COUNTERS == pn.COUNTERS and pn.N_LINES == 8 and pn.BEST_F == 19 and pn.FVAL == 16 and pn.BEST_X == 4


def _call(**over):
    """pem_powell_step_f64_dev with valid host-side arguments (the device pointers are never followed: every case is refused
    before the device is looked at), one of them replaced"""
    d = over.pop('ndim', 3)
    n = max(d, 1)
    kw = dict(n_search=2, ndim=d, finalize=0, xtol=1e-4, ftol=1e-4, max_iter=0, sqrt_eps=pn.SQRT_EPS, golden_mean=pn.GOLDEN_MEAN,
              kind=np.zeros(n, np.int32), a=np.zeros(n), b=np.ones(n), lb=np.zeros(n), ub=np.ones(n))
    dev = dict(vec=8, direc=8, scal=8, cand_f=8, theta=8, state=8, history=None)          # non-NULL stand-ins
    hist_len = over.pop('history_len', 0)
    for k, v in over.items():
        (dev if k in dev else kw)[k] = v
    ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)              # noqa: E731
    dp = lambda v: None if v is None else C.c_void_p(v)                           # noqa: E731
    return _lib.load().pem_powell_step_f64_dev(kw['n_search'], kw['ndim'], kw['finalize'], kw['xtol'], kw['ftol'], kw['max_iter'],
                                               kw['sqrt_eps'], kw['golden_mean'], *(ptr(kw[k]) for k in ('kind', 'a', 'b', 'lb', 'ub')),
                                               *(dp(dev[k]) for k in ('vec', 'direc', 'scal', 'cand_f', 'theta', 'state', 'history')),
                                               hist_len, None)


@pytest.mark.parametrize('over', [
    dict(n_search=0), dict(ndim=0), dict(ndim=33), dict(ndim=-1), dict(finalize=3), dict(finalize=-1),
    dict(kind=None), dict(a=None), dict(b=None), dict(lb=None), dict(ub=None),
    dict(vec=None), dict(direc=None), dict(scal=None), dict(cand_f=None), dict(theta=None), dict(state=None),
    dict(lb=np.array([0.0, 0.6, 0.0]), ub=np.array([1.0, 0.5, 1.0])), dict(lb=np.array([0.0, np.nan, 0.0])),
    dict(ub=np.array([1.0, 1.0, np.nan])),
    dict(xtol=-1e-9), dict(ftol=-1.0), dict(xtol=float('nan')), dict(ftol=float('nan')),
    dict(sqrt_eps=0.0), dict(golden_mean=float('nan')), dict(golden_mean=1.0),
    dict(history=8, history_len=0),
    dict(kind=np.array([0, 3, 0], np.int32)), dict(kind=np.array([0, -1, 0], np.int32)),
], ids=lambda o: '-'.join(o))
def test_the_entry_point_refuses_bad_arguments_before_looking_at_the_device(over):
    assert _call(**over) == _lib.PEM_ERR_INVALID_ARG, over


# ---------------------------------------------------------------------------------------------------- kernel resources
@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_powell_kernel_has_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'),
                          str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_powell.hip')], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    assert list(rows) == ['powell_step_kernel'], rows
    r = rows['powell_step_kernel']
    assert r['sspill'] == 0 and r['vspill'] == 0 and r['scratch'] == 0, r


# ----------------------------------------------------------------------------------- the restatement against scipy
def _cases():
    """the 27 cases: name, (f, lb, ub), keywords (seed of the start, or x0; limits; xtol; direc)"""
    out = []
    for d in (1, 2, 3, 5, 12, 17, 32):
        if d != 2:                                       # (quadratic-d2 does not converge: it is run to limits below)
            out.append((f'quadratic-d{d}', _quadratic(d, d), dict(seed=d)))
        if d >= 2:                                       # in one dimension the Rosenbrock sum is empty
            out.append((f'rosenbrock-d{d}', _rosenbrock(d), dict(seed=d)))
    out.append(('quadratic-outside-d5', _quadratic(5, 50, outside=True), dict(seed=1)))
    out.append(('quadratic-outside-d12', _quadratic(12, 51, outside=True), dict(seed=2)))
    for d in (2, 3, 5, 8):
        for seed in (0, 1, 2):
            out.append((f'rough-d{d}-s{seed}', _rough(d), dict(seed=seed)))
    out.append(('quadratic-d2-maxiter7', _quadratic(2, 2), dict(seed=2, max_iterations=7, nfev=127)))
    out.append(('quadratic-d2-maxiter25', _quadratic(2, 2), dict(seed=2, max_iterations=25, nfev=469)))
    out.append(('quadratic-d2-maxfev2000', _quadratic(2, 2), dict(seed=2, nfev=2000, nit=105, status=3)))
    out.append(('quadratic-d5-maxfev100', _quadratic(5, 5), dict(seed=5, max_evaluations=100, nfev=100, status=3)))
    out.append(('start-on-a-bound-d3', _quadratic(3, 8), dict(x0=np.array([0.5, 1.0, 0.0]))))
    rot = np.linalg.qr(np.random.default_rng(11).standard_normal((5, 5)))[0]
    out.append(('caller-direc-d5', _quadratic(5, 9), dict(seed=3, direc=0.5 * rot)))
    # constructed: the branches the functions above do not reach (scipy reaches them too, and agrees)
    zero_row = np.eye(3)
    zero_row[1] = 0.0
    out.append(('zero-direction-d3', _quadratic(3, 7), dict(seed=4, direc=zero_row, reach=('zero_dir',))))
    out.append(('corner-pointing-out-d2', _quadratic(2, 6), dict(x0=np.zeros(2), direc=np.array([[1.0, -1.0], [0.0, 1.0]]),
                                                                 reach=('degenerate', 'one_eval'))))
    kink = (lambda x: -abs(float(x[0]))), np.array([-1.0]), np.array([2.0])
    out.append(('line-search-cap-d1', kink, dict(x0=np.array([0.0]), xtol=1e-300, reach=('cap',))))
    return out


CASES = _cases()
_RUNS = {}


def _run(name):
    """the restatement's run of a case, with every point it evaluated (computed once, shared by the tests below)"""
    if name not in _RUNS:
        (f1, lb, ub), kw = next((c[1], c[2]) for c in CASES if c[0] == name)
        x0 = kw['x0'] if 'x0' in kw else _start(kw['seed'], lb.size, lb, ub)
        rec = []
        got = pn.minimize(f1, x0, lb, ub, xtol=kw.get('xtol', 1e-4), ftol=1e-4, max_iterations=kw.get('max_iterations'),
                          max_evaluations=kw.get('max_evaluations'), direc=kw.get('direc'), record=rec)
        _RUNS[name] = (got, rec, x0)
    return _RUNS[name]


@pytest.mark.parametrize('name, problem, kw', CASES, ids=[c[0] for c in CASES])
def test_the_restatement_equals_scipy_bit_for_bit(name, problem, kw):
    """every evaluated point in order, x, fun, nit, nfev and direc of scipy.optimize.minimize(method='Powell', bounds=...,
    options=dict(xtol=1e-4, ftol=1e-4)); scipy minimises the function without its minus sign"""
    from scipy.optimize import minimize
    f1, lb, ub = problem
    got, rec, x0 = _run(name)
    pts = []

    def g(x):
        pts.append(np.array(x, dtype=np.float64))
        return -f1(x)
    opts = dict(xtol=kw.get('xtol', 1e-4), ftol=1e-4)
    for mine, theirs in (('max_iterations', 'maxiter'), ('max_evaluations', 'maxfev'), ('direc', 'direc')):
        if mine in kw:
            opts[theirs] = kw[mine]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                  # (a direc that is not of full rank, a run that ends at a limit)
        want = minimize(g, x0, method='Powell', bounds=list(zip(lb, ub)), options=opts)
    assert (got['nit'], got['nfev']) == (want.nit, want.nfev), (got['nit'], got['nfev'], want.nit, want.nfev)
    assert len(rec) == len(pts) and all(np.array_equal(p, q) for p, q in zip(rec, pts))
    assert np.array_equal(got['x'], want.x) and got['fun'] == want.fun
    assert np.array_equal(got['direc'][0], want.direc)
    assert got['status'] == {0: 1, 1: 3, 2: 2}[want.status], (got['status'], want.status)
    for key in ('nfev', 'nit', 'status'):
        if key in kw:
            assert got[key] == kw[key], (key, got[key])
    assert all(np.all((p >= lb) & (p <= ub)) for p in rec)
    for key in kw.get('reach', ()):
        assert got['counters'][key] > 0, (key, got['counters'])
    # finalize left the transform of x (the priors are U(0, 1): theta = x) and the best value consumed is at least scipy's
    assert np.array_equal(got['theta'][0], got['x']) and got['scal'][0, pn.BEST_F] >= -got['fun']


def test_the_cases_take_every_branch_of_the_table_and_the_constructed_ones_the_rest():
    total = {k: 0 for k in pn.COUNTERS}
    plain = {k: 0 for k in pn.COUNTERS}
    for name, _, kw in CASES:
        for k, v in _run(name)[0]['counters'].items():
            total[k] += v
            if 'reach' not in kw and 'direc' not in kw and 'x0' not in kw:
                plain[k] += v
    print(plain)
    assert all(plain[k] > 0 for k in pn.TABLE), plain
    # what no function of the 27 reaches
    assert all(plain[k] == 0 for k in ('zero_dir', 'zero_disp', 'degenerate', 'one_eval', 'cap')), plain
    assert all(total[k] > 0 for k in ('zero_dir', 'degenerate', 'one_eval', 'cap')), total
    # a line search can return a worse value than it started from: it never evaluates its base point
    assert plain['worse'] > 0 and plain['extra'] == plain['replaced']


def _steps(S, d, lb, ub, value, n, direc=None, x0=None, xtol=1e-4, max_iter=pn.UNBOUNDED):
    """n launches of S searches under value(launch, t) -> (S,); yields the dict after every launch"""
    kind, a, b = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    vec = np.zeros((S, pn.VEC_ROWS, d))
    vec[:, pn.X] = x0
    D = np.broadcast_to(np.eye(d) if direc is None else direc, (S, d, d)).copy()
    t = dict(vec=vec, direc=D, scal=np.zeros((S, pn.SCALARS)), theta=np.zeros((S, d)), state=np.zeros((S, pn.STATE_WORDS), np.uint64),
             history=np.full((n, S), np.nan))
    cand_f = np.zeros(S)
    for launch in range(n):
        t = pn.step(False, xtol, 1e-4, max_iter, kind, a, b, lb, ub, t['vec'], t['direc'], t['scal'], cand_f, t['theta'], t['state'],
                    t['history'])
        yield t
        cand_f = value(launch, t)


def test_an_all_zero_displacement_extrapolates_to_x_itself():
    """Directions of length 1e-30 and values that want alpha = 0: every line search ends where it began although its value fell
    from 1e40, so the iteration ends with x - x1 = 0 and the ftol test not met.  scipy raises there (max of an empty array);
    here lmax = 1 and the extrapolated point is x."""
    d = 2
    lb, ub = np.zeros(d), np.ones(d)
    x0 = np.array([[0.5, 0.25]])
    value = lambda launch, t: np.array([-1e40]) if launch == 0 else -np.abs(t['scal'][:, pn.ALPHA])   # noqa: E731
    seen = False
    for t in _steps(1, d, lb, ub, value, 600, direc=1e-30 * np.eye(d), x0=x0):
        pt = t['vec'][0, pn.CAND]
        assert np.all(np.isfinite(pt)) and np.all((pt >= lb) & (pt <= ub))
        if t['state'][0, pn.N_ZERO_DISP] > 0 and not seen:
            seen = True
            assert t['state'][0, pn.PHASE] == pn.PH_EXTRAP and np.array_equal(pt, x0[0]) and np.array_equal(t['vec'][0, pn.X], x0[0])
            assert not t['vec'][0, pn.XI].any()
    assert seen and t['state'][0, pn.N_ZERO_DIR] > 0      # and the extra line search along it, when asked for, is skipped


def _hostile(rng, S, launch):
    """the synthetic values of tests/test_nelder_mead.py: few distinct values, NaN, -inf, every third launch all NaN"""
    f = np.round(rng.normal(size=S), 1)
    f[rng.random(S) < 0.1] = np.nan
    f[rng.random(S) < 0.1] = -np.inf
    if launch % 3 == 2:
        f[:] = np.nan
    return f


@pytest.mark.parametrize('d', [1, 2, 5, 17])
def test_every_emitted_point_is_finite_and_inside_the_bounds_under_hostile_values(d):
    S, n = 12, 400
    rng = np.random.default_rng(d)
    lb, ub = np.where(np.arange(d) % 3 == 2, 0.0013498980316300957, 0.0), np.where(np.arange(d) % 3 == 2, 0.9986501019683699, 1.0)
    x0 = lb + (ub - lb) * rng.uniform(0.0, 1.0, (S, d))
    x0[0] = ub                                           # a start in a corner
    x0[1, 0] = lb[0]
    for t in _steps(S, d, lb, ub, lambda launch, t: _hostile(rng, S, launch), n, x0=x0, max_iter=50):
        pts = t['vec'][:, pn.CAND]
        assert np.all(np.isfinite(pts)) and np.all((pts >= lb) & (pts <= ub))
        assert np.all(np.isfinite(t['vec'])) and np.all(np.isfinite(t['direc'])) and np.all(np.isfinite(t['theta']))
        assert not np.isnan(t['scal'][:, [pn.A, pn.B, pn.XF, pn.ALPHA, pn.TOL1, pn.BEST_F]]).any()
    assert np.all(t['state'][:, pn.LAUNCHES] == n) and np.all(t['state'][:, pn.NIT] >= 1)
    running = t['state'][:, pn.STATUS] == 0
    assert np.all(t['state'][running, pn.NFEV] == n - 1)  # a running search consumes one value per launch


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
    (dict(names=('T_e', 'c0'), x0=np.zeros((0, 2))), ValueError, 'x0 must have'),
    (dict(names=('T_e', 'c0'), x0=[3.0, 0.5], n_starts=4), ValueError, 'at most one'),
    (dict(names=('T_e', 'c0'), n_starts=0), ValueError, 'n_starts'),
    (dict(names=('T_e', 'c4'), x0=[3.0, -1e20]), ValueError, 'no finite quantile'),                  # log10 of a negative
    (dict(names=('T_e', 'c4'), x0=[float('nan'), 1e20]), ValueError, 'no finite quantile'),
    (dict(names=('T_e', 'c4'), x0=[[3.0, 1e20], [3.0, 0.0]]), ValueError, 'no finite quantile'),             # log10(0) = -inf
    (dict(names=('T_e', 'c0'), direc=np.eye(3)), ValueError, 'direc must have'),
    (dict(names=('T_e', 'c0'), n_starts=3, direc=np.ones((2, 2, 2))), ValueError, 'direc must have'),
    (dict(names=('T_e', 'c0'), direc=[[1.0, 0.0], [0.0, float('inf')]]), ValueError, 'direc must be finite'),
    (dict(names=('T_e', 'c0'), xtol=-1e-4), ValueError, 'xtol'),
    (dict(names=('T_e', 'c0'), ftol=-1e-4), ValueError, 'ftol'),
    (dict(names=('T_e', 'c0'), ftol=float('nan')), ValueError, 'ftol'),
])
def test_powell_driver_rejects_bad_arguments_before_touching_a_device(kw, err, match, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    with pytest.raises(err, match=match):
        Powell(_f, **kw)


def test_differential_evolution_refuses_an_unknown_init_and_defaults_to_lhs(monkeypatch):
    import inspect
    import torch
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    with pytest.raises(ValueError, match='unknown init'):
        DifferentialEvolution(_f, ('T_e', 'c0'), init='bogus')
    assert inspect.signature(DifferentialEvolution.__init__).parameters['init'].default == 'lhs'
