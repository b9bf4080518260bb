"""The plan of the host-pointer entry points (pem_host_plan, include/pem_hip.h) against its restatement in plain Python
(tests/host_plan_cases.py), the table of sizes the GPU tests of tests/test_host_entry_points.py run at, and the calls the
four entry points refuse -- all without a device."""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import host_plan_cases as hc
from hallthrusterpem_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
RADII = (1, 2, 3, 8, 25, 64, 65, 256, 300)


def _zero_copy_allowed():
    """what the library makes of PEM_ZERO_COPY: off only when it is set and atoi() of it is 0"""
    v = os.environ.get('PEM_ZERO_COPY')
    if v is None:
        return True
    m = re.match(r'\s*([+-]?\d+)', v)
    return bool(m and int(m.group(1)) != 0)


def c_plan(entry, n, R=1, n_optional=8):
    out = [C.c_size_t(0) for _ in range(5)]
    regime = C.c_int(-9)
    rc = _lib.load().pem_host_plan(entry, n, R, n_optional, *[C.byref(o) for o in out], C.byref(regime))
    assert rc == _lib.PEM_OK, (entry, n, R, n_optional)
    return hc.Plan(*[int(o.value) for o in out], int(regime.value))


def _table_values():
    vals = set()
    for b in hc.BOUNDARIES:
        vals.add(b.low)
    for t in hc.TWO_CHUNKS:
        vals.add(t.chunk)
    return vals


def _sweep_sizes():
    grid = {int(round(10 ** e)) for e in np.linspace(0, 5.6, 57)}             # 1 .. 4e5, ten per decade
    table = {v for v in _table_values() if v < 10 ** 6}
    return sorted(n for v in grid | table for n in (v - 1, v, v + 1) if n >= 1)


def _configs():
    for entry in (hc.CATHODE, hc.COUPLED):
        yield entry, 1, 8
    for k in range(9):
        yield hc.THRUSTER, 1, k
    for R in RADII:
        yield hc.PLUME, R, 8


def test_the_plan_equals_its_restatement_over_the_sweep():
    zc = _zero_copy_allowed()
    sizes = _sweep_sizes()
    assert sizes[0] == 1 and sizes[-1] > 3 * 10 ** 5 and len(sizes) > 150
    regimes = set()
    for entry, R, k in _configs():
        for n in sizes:
            want = hc.plan(entry, n, R, k, zero_copy=zc)
            assert c_plan(entry, n, R, k) == want, (hc.NAMES[entry], n, R, k)
            regimes.add((entry, want.regime))
    assert regimes >= {(e, r) for e in hc.NAMES for r in (1, 2, 3)}           # the sweep reaches every regime of every entry point
    assert not zc or regimes >= {(e, 0) for e in hc.NAMES}


def test_the_optional_outputs_move_the_thruster_layout_only():
    """n_optional is the thruster stage's: the plume and the coupled model carve their optional arrays whether they are asked
    for or not, and the thruster stage reserves room for eight outputs however many it carves"""
    for n in (1, 2720, 2721, 30000, 70000):
        for entry, R in ((hc.CATHODE, 1), (hc.PLUME, 1), (hc.PLUME, 8), (hc.COUPLED, 1)):
            assert len({c_plan(entry, n, R, k) for k in (0, 3, 8)}) == 1
        plans = [c_plan(hc.THRUSTER, n, 1, k) for k in range(9)]
        assert len({p.reserve for p in plans}) == 1 and plans[8].reserve == plans[8].footprint
        assert [p.footprint - p.in_end for p in plans] == [k * hc.padded(8 * n) for k in range(9)]
        assert len({p.in_end for p in plans}) == 1


@pytest.mark.parametrize('b', hc.BOUNDARIES, ids=lambda b: f'{hc.NAMES[b.entry]}-R{b.R}-k{b.n_optional}-{b.low}')
def test_the_table_straddles_each_regime_boundary(b):
    k = b.n_optional if b.entry == hc.THRUSTER else 8
    low, high = c_plan(b.entry, b.low, b.R, k), c_plan(b.entry, b.low + 1, b.R, k)
    if not _zero_copy_allowed() and b.regime_low == 0:                         # PEM_ZERO_COPY=0 in this process: no such boundary
        assert low.regime == high.regime == 1 and low.reserve <= hc.ZC_BYTES < high.reserve
        return
    assert (low.regime, high.regime) == (b.regime_low, b.regime_high) and low.regime != high.regime
    assert low.n_chunks == high.n_chunks == 1
    limit, side = {0: (hc.ZC_BYTES, 'reserve'), 1: (hc.STAGE_BYTES, 'footprint'), 2: (hc.STAGE_BYTES, 'in_end')}[b.regime_low]
    if (b.regime_low, b.regime_high) == (1, 3):                                # no outputs: footprint and in_end cross together
        assert low.footprint == low.in_end <= hc.STAGE_BYTES < high.in_end
    else:
        assert getattr(low, side) <= limit < getattr(high, side)


def test_the_table_holds_every_boundary_a_call_can_reach():
    """nothing left out: for every configuration the table speaks of, bisecting the restated plan finds the table's rows"""
    configs = {(b.entry, b.R, b.n_optional) for b in hc.BOUNDARIES}
    assert configs >= {(hc.CATHODE, 1, 0), (hc.COUPLED, 1, 0)} | {(hc.THRUSTER, 1, k) for k in (0, 1, 8)} \
        | {(hc.PLUME, R, 0) for R in (1, 3, 8, 25)}
    for entry, R, k in sorted(configs):
        rows = [(b.low, b.regime_low, b.regime_high) for b in hc.boundaries(entry, R, k)]
        assert rows == hc.find_boundaries(entry, R, k), (hc.NAMES[entry], R, k)


def test_the_hand_derived_coupled_values():
    assert [(b.low, b.regime_low, b.regime_high) for b in hc.boundaries(hc.COUPLED)] == [(256, 0, 1), (2304, 1, 2), (17472, 2, 3)]
    assert c_plan(hc.COUPLED, 368768).n_chunks == 1 and c_plan(hc.COUPLED, 368769)[:2] == (368768, 2)


@pytest.mark.parametrize('t', hc.TWO_CHUNKS, ids=lambda t: f'{hc.NAMES[t.entry]}-R{t.R}')
def test_two_chunks_with_one_sample_in_the_last(t):
    one, two = c_plan(t.entry, t.chunk, t.R), c_plan(t.entry, t.chunk + 1, t.R)
    assert (one.chunk, one.n_chunks) == (t.chunk, 1)
    assert (two.chunk, two.n_chunks) == (t.chunk, 2) and (t.chunk + 1) - (two.n_chunks - 1) * two.chunk == 1
    assert one.regime == two.regime == t.regime
    assert one[2:] == two[2:]                                                 # the layout is the full chunk's on both sides
    assert {r.entry for r in hc.TWO_CHUNKS} == set(hc.NAMES)                  # every chunk rule; the plume's above and at its floor
    many = c_plan(t.entry, 5 * t.chunk + 7, t.R)
    assert (many.chunk, many.n_chunks) == (t.chunk, 6)


def test_the_plan_refuses_what_it_cannot_plan():
    lib = _lib.load()
    out = [C.c_size_t(7) for _ in range(5)]
    regime = C.c_int(-9)
    ptrs = [C.byref(o) for o in out] + [C.byref(regime)]
    bad = [(-1, 10, 1, 8), (4, 10, 1, 8), (hc.COUPLED, 0, 1, 8), (hc.PLUME, 10, 0, 8), (hc.PLUME, 10, -3, 8), (hc.CATHODE, 10, 0, 8),
           (hc.THRUSTER, 10, 1, 9), (hc.THRUSTER, 10, 1, -1)]
    for args in bad:
        assert lib.pem_host_plan(*args, *ptrs) == _lib.PEM_ERR_INVALID_ARG, args
        assert b'pem_host_plan' in lib.pem_last_error()
        assert [o.value for o in out] == [7] * 5 and regime.value == -9       # nothing written
    for i in range(6):
        with_null = list(ptrs)
        with_null[i] = None
        assert lib.pem_host_plan(hc.COUPLED, 10, 1, 8, *with_null) == _lib.PEM_ERR_INVALID_ARG
    assert lib.pem_host_plan(hc.CATHODE, 10, 1, 99, *ptrs) == _lib.PEM_OK         # n_optional is the thruster stage's alone


def test_zero_copy_switched_off_plans_regime_1():
    """PEM_ZERO_COPY is read once per process: a fresh one, with it set to 0, plans regime 1 where this one plans 0 -- and the
    same chunk and layout"""
    code = ('import sys; sys.path[:0] = [%r, %r]\n'
            'import host_plan_cases as hc, test_host_entry_points_host as t\n'
            'for e in hc.NAMES:\n'
            '    for n in (1, 64, 256):\n'
            '        print(e, n, *t.c_plan(e, n, 1, 8))\n') % (str(ROOT), str(ROOT / 'tests'))
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PEM_ZERO_COPY='0'), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    assert len(rows) == 12
    for e, n, *got in rows:
        want = hc.plan(e, n, 1, 8, zero_copy=False)
        assert hc.Plan(*got) == want and want.regime == 1 and hc.plan(e, n, 1, 8).regime == 0
        assert want[:5] == hc.plan(e, n, 1, 8)[:5]


@pytest.mark.parametrize('case', hc.malformed_calls(), ids=lambda c: c[0])
def test_malformed_calls_are_refused_before_a_device_is_looked_for(case):
    _, entry, R, x, wanted = case
    lib = _lib.load()
    n = 5
    outs = hc.alloc_outputs(entry, n, max(R, 1), wanted)
    before = lib.pem_host_last_regime()
    assert hc.call_host(lib, entry, n, x, outs, R) == _lib.PEM_ERR_INVALID_ARG
    assert NAMES_IN_ERRORS[entry] in lib.pem_last_error()
    assert all(hc.untouched(a) for a in outs.values())
    assert lib.pem_host_last_regime() == before


NAMES_IN_ERRORS = {hc.CATHODE: b'pem_cathode', hc.THRUSTER: b'pem_thruster', hc.PLUME: b'pem_plume', hc.COUPLED: b'pem_coupled'}


def test_the_malformed_calls_cover_every_array_that_must_not_be_null():
    labels = [c[0] for c in hc.malformed_calls()]
    assert len(labels) == len(set(labels)) == (6 + 1) + 4 + (9 + 2) + (15 + 3) + 4
    assert hc.call_host(_lib.load(), hc.THRUSTER, 0, {}, {}) == _lib.PEM_OK     # n == 0: nothing to do, nothing looked at
