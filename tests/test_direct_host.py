"""optimize.Direct on the host (no GPU): the numpy restatement of the launch (tests/direct_np.py) against scipy's own DIRECT bit
for bit -- every evaluated point in order, x, fun, nit, nfev and status, with no tie met --, the stops, the emission chopped
into other row counts, a NaN value, the C ABI of pem_direct_step_f64_dev and what it refuses, the kernel's resources, and what
the driver refuses before it touches a device."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import direct_np as dn
from hallthrusterpem_amd import _lib
from hallthrusterpem_amd.optimize import DIRECT_STATUS, Direct, direct_tables

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------------------------------- ABI and bindings
def test_the_entry_point_is_declared_bound_and_exported():
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    assert re.search(r'\bint pem_direct_step_f64_dev\(', header)
    assert 'pem_direct_step_f64_dev' in _lib.SIGNATURES
    assert getattr(_lib.load(), 'pem_direct_step_f64_dev') is not None
    assert len(_lib.SIGNATURES['pem_direct_step_f64_dev'][1]) == 29
    for name, value, mine in (('PEM_DIRECT_MAX_DIM', _lib.DIRECT_MAX_DIM, dn.MAX_DIM),
                              ('PEM_DIRECT_MAX_LEVELS', _lib.DIRECT_MAX_LEVELS, dn.MAX_LEVELS),
                              ('PEM_DIRECT_MAX_DEPTH', _lib.DIRECT_MAX_DEPTH, dn.MAX_DEPTH),
                              ('PEM_DIRECT_MAX_ROWS', _lib.DIRECT_MAX_ROWS, dn.MAX_ROWS),
                              ('PEM_DIRECT_STATE_WORDS', _lib.DIRECT_STATE_WORDS, dn.STATE_WORDS),
                              ('PEM_DIRECT_HISTORY_COLS', _lib.DIRECT_HISTORY_COLS, dn.HISTORY_COLS)):
        assert re.search(rf'#define {name} {value}\b', header) and value == mine, name
    assert re.search(rf'#define PEM_DIRECT_MAX_STORE {_lib.DIRECT_MAX_STORE}\b', header)
    assert 'pem_direct.hip' in [s.name for s in __import__('hallthrusterpem_amd.build', fromlist=['SRCS']).SRCS]
    assert DIRECT_STATUS.keys() == dn.STATUS_NAMES.keys()
    for d in (1, 2, 17, 32):                             # the driver's tables are the restatement's
        for got, want in zip(direct_tables(d), dn.tables(d)):
            assert np.array_equal(got, want)
    thirds, levels = dn.tables(17)
    assert thirds.size == 61 and levels.size == 60 * 17 and thirds[2] == 1.0 / 9.0 and np.all(np.diff(levels) < 0)


def _call(**over):
    """pem_direct_step_f64_dev with valid host-side arguments (the device pointers are never followed: every case is refused
    before the device is looked at), one of them replaced"""
    d = over.pop('ndim', 3)
    n = max(d, 1)
    kw = dict(ndim=d, rows=2 * n, cap=100, n_depth=8, finalize=0, eps=1e-4, vol_tol=1e-16, len_tol=1e-6, max_iter=1000, max_fun=3000,
              kind=np.zeros(n, np.int32), a=np.zeros(n), b=np.ones(n), lb=np.zeros(n), ub=np.ones(n))
    dev = dict(thirds=8, levels=8, centres=8, values=8, expo=8, level=8, queue=8, rowinfo=8, cand_f=8, theta=8, state=8,
               history=None)                                                          # non-NULL stand-ins
    hist_len = over.pop('history_len', 0)
    for k, v in over.items():
        (dev if k in dev else kw)[k] = v
    ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)              # noqa: E731
    dp = lambda v: None if v is None else C.c_void_p(v)                           # noqa: E731
    return _lib.load().pem_direct_step_f64_dev(
        kw['ndim'], kw['rows'], kw['cap'], kw['n_depth'], kw['finalize'], kw['eps'], kw['vol_tol'], kw['len_tol'], kw['max_iter'],
        kw['max_fun'], *(ptr(kw[k]) for k in ('kind', 'a', 'b', 'lb', 'ub')), *(dp(v) for v in dev.values()), hist_len, None)


@pytest.mark.parametrize('over', [
    dict(ndim=0), dict(ndim=33), dict(ndim=-1), dict(rows=5), dict(rows=0), dict(rows=1025), dict(cap=6), dict(cap=0),
    dict(cap=16777217), dict(n_depth=1), dict(n_depth=65), dict(ndim=32, n_depth=33), dict(finalize=2), dict(finalize=-1),
    dict(eps=-1e-9), dict(eps=float('nan')), dict(eps=float('inf')), dict(vol_tol=-1e-9), dict(vol_tol=1.5),
    dict(vol_tol=float('nan')), dict(len_tol=-1e-9), dict(len_tol=1.5), dict(len_tol=float('nan')), dict(max_iter=0),
    dict(kind=None), dict(a=None), dict(b=None), dict(lb=None), dict(ub=None),
    dict(thirds=None), dict(levels=None), dict(centres=None), dict(values=None), dict(expo=None), dict(level=None),
    dict(queue=None), dict(rowinfo=None), dict(cand_f=None), dict(theta=None), dict(state=None),
    dict(lb=np.array([0.0, 0.6, 0.0]), ub=np.array([1.0, 0.5, 1.0])), dict(lb=np.array([0.0, 1.0, 0.0])),
    dict(lb=np.array([0.0, np.nan, 0.0])), dict(ub=np.array([1.0, 1.0, np.nan])), dict(ub=np.array([1.0, np.inf, 1.0])),
    dict(lb=np.array([-np.inf, 0.0, 0.0])),
    dict(history=8, history_len=0),
    dict(kind=np.array([0, 3, 0], np.int32)), dict(kind=np.array([0, -1, 0], np.int32)),
], ids=lambda o: '-'.join(o))
def test_the_entry_point_refuses_bad_arguments_before_looking_at_the_device(over):
    assert _call(**over) == _lib.PEM_ERR_INVALID_ARG, over


# ---------------------------------------------------------------------------------------------------- kernel resources
@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_direct_kernel_has_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'),
                          str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_direct.hip')], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    assert list(rows) == ['direct_step_kernel'], rows
    r = rows['direct_step_kernel']
    assert r['sspill'] == 0 and r['vspill'] == 0 and r['scratch'] == 0, r


# ----------------------------------------------------------------------------------- the restatement against scipy
def a2(x):
    return (x[0] - 0.3) ** 2 + 2 * (x[1] + 0.7) ** 2 + 0.5 * np.sin(3 * x[0])


def r3(x):
    return 100 * (x[1] - x[0] ** 2) ** 2 + (1 - x[0]) ** 2 + np.pi * (x[2] - 0.37) ** 2


_C4 = np.random.default_rng(3).uniform(-1, 1, 4)
_RNG = np.random.default_rng(0)
_C6 = _RNG.uniform(-1, 1, 6)
_C17 = _RNG.uniform(-1, 1, 17)


def s4(x):
    return sum((i + 1) * abs(x[i] - _C4[i]) ** 1.5 for i in range(4)) + np.cos(2.3 * x[0] + x[1]) - 0.4


def q6(x):
    return sum((i + 1) * (x[i] - _C6[i]) ** 2 for i in range(6)) + 3487


def q17(x):
    return sum((i + 1) * (x[i] - _C17[i]) ** 2 for i in range(17)) + np.sin(x[0] * x[1]) - 5


PROBLEMS = {'a2': (a2, [-1.0, -3.0], [2.0, 1.5]), 'r3': (r3, [-2.0, -1.0, 0.0], [2.1, 3.3, 1.0]), 's4': (s4, [-2.0] * 4, [2.5] * 4),
            'q6': (q6, [-2.0] * 6, [2.0] * 6), 'q17': (q17, [-2.0] * 17, [2.2] * 17)}
_SCIPY = {}


def _scipy(name, **kw):
    """scipy's run of a problem with every point it evaluated (computed once per setting, shared by the tests below)"""
    from scipy.optimize import direct
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _SCIPY:
        f, lb, ub = PROBLEMS[name]
        pts = []

        def g(x):
            pts.append(np.array(x, dtype=np.float64))
            return f(x)
        _SCIPY[key] = (direct(g, list(zip(lb, ub)), locally_biased=False, **kw), pts)
    return _SCIPY[key]


def _equal(name, rows=None, **kw):
    f, lb, ub = PROBLEMS[name]
    want, pts = _scipy(name, **kw)
    rec = []
    got = dn.minimize(f, lb, ub, rows=rows, record=rec, **kw)
    print(name, kw, rows, 'scipy', want.nit, want.nfev, want.status, 'restatement', got['nit'], got['nfev'], got['status'],
          'launches', got['launches'], 'ties', got['ties'])
    assert (got['nit'], got['nfev'], got['status']) == (want.nit, want.nfev, want.status)
    assert len(rec) == len(pts) and all(np.array_equal(p, q) for p, q in zip(rec, pts))
    assert np.array_equal(got['x'], want.x) and got['fun'] == want.fun
    assert got['ties'] == 0
    assert all(np.all((p >= lb) & (p <= ub)) for p in rec)
    return got


@pytest.mark.parametrize('eps', [1, 1e-4])
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_the_restatement_equals_scipy_bit_for_bit(name, eps):
    """every evaluated point in order, x, fun, nit, nfev and status of scipy.optimize.direct(..., eps=eps, maxiter=30,
    locally_biased=False), and no tie on the way.  What scipy 1.15.3 gave: 435 / 831, 479 / 1159, 861 / 1849, 197 / 1975 and
    3445 / 5741 evaluations; the last run stops by vol_tol at nit 22."""
    got = _equal(name, eps=eps, maxiter=30)
    if name == 'q17' and eps == 1e-4:
        assert got['status'] == 4 and got['nit'] < 30
    else:
        assert got['status'] == 2 and got['nit'] == 30


@pytest.mark.parametrize('name, kw', [
    ('a2', dict(eps=1, maxfun=20)), ('a2', dict(eps=1, maxfun=30)),
    ('a2', dict(eps=1e-4, vol_tol=0, len_tol=1e-2)), ('a2', dict(eps=1e-4, vol_tol=0, len_tol=1e-3)),
    ('r3', dict(eps=1e-4, vol_tol=1e-9)),
    ('a2', dict(eps=1, maxiter=1)), ('a2', dict(eps=1, maxiter=2)), ('a2', dict(eps=1, maxiter=3)),
], ids=lambda v: v if isinstance(v, str) else '-'.join(f'{k}={x}' for k, x in v.items()))
def test_the_stops_are_scipys(name, kw):
    """the limits are looked at after a whole round: maxfun once nfev > maxfun (status 1), maxiter = M after M - 2 selection
    rounds with nit = M (2), vol_tol (4), len_tol (5).  What scipy 1.15.3 gave: nfev 29 / nit 5 and 41 / 6; nit 8 / nfev 75 and
    12 / 175; nit 26 / nfev 951."""
    got = _equal(name, **kw)
    assert got['status'] == (1 if 'maxfun' in kw else 5 if 'len_tol' in kw else 4 if 'vol_tol' in kw else 2)


@pytest.mark.parametrize('name, kw', [('r3', dict(eps=1e-4, maxiter=30)), ('q6', dict(eps=1e-4, maxiter=30)),
                                      ('q17', dict(eps=1, maxiter=30))], ids=['r3', 'q6', 'q17'])
def test_chopping_the_emission_into_other_row_counts_changes_nothing(name, kw):
    d = len(PROBLEMS[name][1])
    launches = [_equal(name, rows=rows, **kw)['launches'] for rows in (2 * d, 2 * d + 1, 64)]
    assert launches[0] >= launches[1] >= launches[2] and launches[0] > launches[2], launches


def test_a_whole_round_goes_into_one_launch_when_the_rows_hold_it():
    """q6 at eps = 1: the rounds are small, and with 64 rows most launches carry a whole round (nit moves with every launch)"""
    f, lb, ub = PROBLEMS['q6']
    got = dn.minimize(f, lb, ub, rows=64, eps=1, maxiter=30)
    assert got['nit'] == 30 and got['launches'] <= 30 + 3, got['launches']


# ------------------------------------------------------------------------------------------------------- hostile values
@pytest.mark.parametrize('at', [1, 2, 9])
def test_a_value_that_is_not_finite_ends_the_search_with_status_7_and_freezes_it(at):
    d, rows = 3, 7
    kind, a, b = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    lb, ub = np.array([-2.0, -1.0, 0.0]), np.array([2.1, 3.3, 1.0])
    thirds, levels = dn.tables(d)
    t = dn.new_state(d, rows, 400)
    hist = np.full((20, 3), -7.0)
    cand_f = np.zeros(rows)
    for launch in range(14):
        t = dn.step(0, 1e-4, 1e-16, 1e-6, 1000, 3000, kind, a, b, lb, ub, thirds, levels, t, cand_f, hist)
        hist = t.pop('history')
        st = t['state']
        assert np.all(np.isfinite(t['theta'])) and np.all((t['theta'] >= lb) & (t['theta'] <= ub))
        if launch < at:
            assert st[dn.STATUS] == 0 and st[dn.PEND] >= 2 - (launch == 0)
        else:
            assert st[dn.STATUS] == 7 and st[dn.PEND] == 0 and st[dn.END] == at + 1 and st[dn.LAUNCHES] == launch + 1
            if launch == at:
                frozen = {k: v.copy() for k, v in t.items()}
            else:                                        # only the launch counter moves
                for k in t:
                    same = t[k].copy()
                    if k == 'state':
                        same[dn.LAUNCHES] = frozen[k][dn.LAUNCHES]
                    assert np.array_equal(same, frozen[k]), k
            if at > 1:                                   # every row is the best point
                best = dn.point(t['centres'][int(st[dn.BEST])], lb, ub)
                assert np.all(t['theta'] == best)
        cand_f = np.array([-r3(x) for x in t['theta']])
        if launch + 1 == at:
            cand_f[int(st[dn.PEND]) - 1] = (np.nan, -np.inf, np.inf)[at % 3]
    assert np.array_equal(hist[at:13, 1], np.full(13 - at, hist[at - 1, 1] if at > 1 else 0.0))


def test_a_store_that_cannot_hold_the_next_round_gives_status_6():
    f, lb, ub = PROBLEMS['a2']
    got = dn.minimize(f, lb, ub, eps=1e-4, cap=60)
    assert got['status'] == 6 and got['nfev'] <= 60
    free = dn.minimize(f, lb, ub, eps=1e-4, maxfun=got['nfev'] - 1)      # the same search until then
    assert free['status'] == 1 and free['nfev'] == got['nfev'] and np.array_equal(free['x'], got['x'])
    # the level table: with room for 4 exponents a rectangle with k = 3 cannot be divided
    d = 2
    kind, a, b = np.zeros(d, np.int32), np.zeros(d), np.ones(d)
    thirds, levels = dn.tables(d, n_depth=4)
    t = dn.new_state(d, 4, 2000)
    cand_f = np.zeros(4)
    for _ in range(400):
        t = dn.step(0, 1e-4, 0.0, 0.0, 1000, 3000, kind, a, b, np.array(lb), np.array(ub), thirds, levels, t, cand_f)
        t.pop('history')
        if t['state'][dn.STATUS] != 0:
            break
        cand_f = np.array([-a2(x) for x in t['theta']])
    n = int(t['state'][dn.NFEV])
    assert t['state'][dn.STATUS] == 6 and t['level'][:n].max() < 4 * d and t['expo'][:n].max() <= 3


# ---------------------------------------------------------------------------------------------- driver argument checks
def _f(theta):
    raise AssertionError('f must not be called')


@pytest.mark.parametrize('kw, err, match', [
    (dict(names=()), ValueError, 'distinct'),
    (dict(names=tuple(f'x{i}' for i in range(33))), ValueError, 'at most 32'),
    (dict(names=('T_e', 'T_e')), ValueError, 'distinct'),
    (dict(names=('T_e', 'nope')), KeyError, 'no prior'),
    (dict(names=('T_e', 'c0'), rows=3), ValueError, 'rows must be'),
    (dict(names=('T_e', 'c0'), rows=1025), ValueError, 'rows must be'),
    (dict(names=('T_e', 'c0'), eps=-1e-4), ValueError, 'eps'),
    (dict(names=('T_e', 'c0'), eps=float('nan')), ValueError, 'eps'),
    (dict(names=('T_e', 'c0'), vol_tol=-1e-4), ValueError, 'vol_tol'),
    (dict(names=('T_e', 'c0'), vol_tol=1.5), ValueError, 'vol_tol'),
    (dict(names=('T_e', 'c0'), len_tol=float('nan')), ValueError, 'len_tol'),
    (dict(names=('T_e', 'c0'), len_tol=2.0), ValueError, 'len_tol'),
    (dict(names=('T_e', 'c0'), locally_biased=True), ValueError, 'locally_biased'),
])
def test_direct_driver_rejects_bad_arguments_before_touching_a_device(kw, err, match, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    with pytest.raises(err, match=match):
        Direct(_f, **kw)


def test_the_defaults_are_scipys():
    import inspect
    sig = inspect.signature(Direct.__init__).parameters
    assert [sig[k].default for k in ('rows', 'eps', 'vol_tol', 'len_tol', 'use_graph')] == [None, 1e-4, 1e-16, 1e-6, False]
    run = inspect.signature(Direct.run).parameters
    assert run['max_iterations'].default == 1000 and run['max_evaluations'].default is None
