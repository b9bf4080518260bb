"""The host-pointer entry points of the C ABI (pem_cathode_f64, pem_thruster_f64, pem_plume_f64, pem_coupled_f64) against the
device-pointer entry points of the same name, bit for bit, in every data-movement regime and across the chunk loop.

The reference of a call is pem_*_f64_dev on torch tensors holding the same inputs, launched once per chunk with the chunk sizes
pem_host_plan reports, so both sides see the same launch sizes.  (The device kernels themselves are held to the long-double
model by tests/test_model_kernels.py.)  Every call asserts the regime it ran in (pem_host_last_regime against the plan), that
the 17 guard rows behind every host output still hold the sentinel, and that no input changed a bit.  The sizes come from the
table of tests/host_plan_cases.py, which tests/test_host_entry_points_host.py holds to the plan without a GPU.

The second chunk of the cathode and of the thruster stage (n > 2^24: more than 900 MB of workspace) is not run: the chunk loop
they share is exercised by the coupled and the plume cases."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import host_plan_cases as hc
from _inputs import cathode_inputs, coupled_inputs, plume_inputs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DEV_FN = {e: name + '_dev' for e, name in hc.HOST_FN.items()}


@pytest.fixture(scope='module')
def lib():
    from hallthrusterpem_amd import _lib
    handle = _lib.load()
    _lib.require_device()          # fail loudly: the GPU tier must never pass on a fallback
    return handle


def c_plan(lib, entry, n, R=1, n_optional=8):
    out = [C.c_size_t(0) for _ in range(5)]
    regime = C.c_int(-9)
    assert lib.pem_host_plan(entry, n, R, n_optional, *[C.byref(o) for o in out], C.byref(regime)) == 0
    return hc.Plan(*[int(o.value) for o in out], int(regime.value))


# ---------------------------------------------------------------------------------------------- inputs
def make_inputs(entry, n, seed):
    """seeded inputs within the priors with wild rows mixed in (every 97th sample each): a NaN input, a negative thrust (a
    negative mass flow where the thrust is computed), a beam below the tables, a beam of no width (invalid)"""
    i = np.arange(n)
    nan, neg, narrow, dead = (i % 97 == 3), (i % 97 == 11), (i % 97 == 29), (i % 97 == 41)
    if entry == hc.CATHODE:
        x = cathode_inputs(n, seed=seed)
        x['T_e'][nan] = np.nan
        x['V_vac'][neg] = -25.0
        x['P_b'][narrow] = 0.0
    elif entry == hc.THRUSTER:
        c = coupled_inputs(n, seed=seed)
        x = {k: c[k] for k in ('V_a', 'mdot_a', 'a_1')}
        x['V_cc'] = c['V_vac'] * 0.5 + 5.0
        x['a_1'][nan] = np.nan
        x['mdot_a'][neg] = -3e-6
        x['V_cc'][narrow] = 500.0                                     # more than the anode voltage
    elif entry == hc.PLUME:
        x = plume_inputs(n, seed=seed)
        x['c1'][nan] = np.nan
        x['T'][neg] = -0.05
        x['c3'][narrow], x['c2'][narrow] = 0.01, 0.0
        x['c3'][dead], x['c2'][dead] = -0.1, 0.0
    else:
        x = coupled_inputs(n, seed=seed)
        x['c1'][nan] = np.nan
        x['mdot_a'][neg] = -3e-6
        x['c3'][narrow], x['c2'][narrow] = 0.01, 0.0
        x['c3'][dead], x['c2'][dead] = -0.3, 0.0
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in x.items()}


# ---------------------------------------------------------------------------------------------- the reference
def reference(lib, entry, n, x, R=1, chunk=None, wanted=None):
    """pem_*_f64_dev on torch tensors, one launch per chunk of `chunk` samples; wanted: names of the outputs passed (all)"""
    import torch
    chunk = chunk or n
    xt = {k: torch.from_numpy(v).cuda() for k, v in x.items() if k in hc.INPUTS[entry]}
    names = [k for k in hc.OUTPUTS[entry] if wanted is None or k in wanted]
    outs = {k: torch.zeros(n * hc.row_len(entry, k, R), dtype=torch.uint8 if k == 'invalid' else torch.float64, device='cuda')
            for k in names}
    radii = hc.radii_of(R)
    for off in range(0, n, chunk):
        m = min(chunk, n - off)
        i = [C.c_void_p(xt[k].data_ptr() + 8 * off) if k in xt else None for k in hc.INPUTS[entry]]
        o = [C.c_void_p(outs[k].data_ptr() + off * hc.row_len(entry, k, R) * outs[k].element_size()) if k in outs else None
             for k in hc.OUTPUTS[entry]]
        if entry == hc.CATHODE:
            args = [m] + i + [hc.TORR_2_PA] + o
        elif entry == hc.THRUSTER:
            args = [m] + i + o
        elif entry == hc.PLUME:
            args = [m, R, C.c_void_p(radii.ctypes.data), hc.TORR_2_PA] + i + o
        else:
            args = [m, hc.TORR_2_PA, hc.RADIUS] + i + o
        assert getattr(lib, DEV_FN[entry])(*args, None) == 0, lib.pem_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def assert_wild_rows_show(entry, ref):
    """the reference holds what the wild rows are there for"""
    doubles = [v for k, v in ref.items() if k != 'invalid']
    assert any(np.isnan(v).any() for v in doubles)
    assert all(np.isfinite(v).any() for v in doubles)
    if 'invalid' in ref:
        assert ref['invalid'].any() and not ref['invalid'].all()
    if 'T' in ref:
        assert (ref['T'] < 0).any()
    if entry == hc.PLUME:
        assert (ref['T_c'] < 0).any()


# ---------------------------------------------------------------------------------------------- one guarded host call
def host_call(lib, entry, n, x, R=1, wanted=None, regime=None):
    """run the host-pointer entry point on guarded outputs; returns the outputs without their guard rows"""
    names = [k for k in hc.OUTPUTS[entry] if wanted is None or k in wanted]
    x = {k: v for k, v in x.items() if not (entry == hc.PLUME and k == 'T' and 'T_c' not in names)}
    outs = hc.alloc_outputs(entry, n, R, names)
    before = {k: v.copy() for k, v in x.items()}
    assert hc.call_host(lib, entry, n, x, outs, R) == 0, lib.pem_last_error()
    n_opt = len(names) if entry == hc.THRUSTER else 8
    planned = c_plan(lib, entry, n, R, n_opt).regime
    assert lib.pem_host_last_regime() == planned
    assert regime is None or planned == regime, (planned, regime)
    for k, v in x.items():
        assert np.array_equal(v.view(np.uint64), before[k].view(np.uint64)), k          # inputs are never written
    got = {}
    for k, a in outs.items():
        used = n * hc.row_len(entry, k, R)
        assert a.size - used == hc.GUARD * hc.row_len(entry, k, R) and hc.untouched(a[used:]), k    # nothing behind the end
        got[k] = a[:used]
    return got


def assert_same_bits(got, ref, names=None):
    for k in (names or got):
        if k == 'invalid':
            assert np.array_equal(got[k], ref[k]), k
        else:
            assert np.array_equal(got[k], ref[k], equal_nan=True), k


def variants(entry):
    """the sets of outputs a case runs with: all of them first"""
    o = hc.OUTPUTS[entry]
    if entry == hc.CATHODE:
        return [o]
    if entry == hc.PLUME:
        return [o, ('j_ion', 'div_angle', 'invalid'), ('j_ion', 'div_angle', 'T_c'), ('j_ion', 'div_angle')]
    if entry == hc.COUPLED:
        return [o] + [tuple(k for k in o if k != drop) for drop in hc.OPTIONAL[entry]] + [('V_cc', 'div_angle', 'T_c')]
    raise ValueError(entry)


def check_call(lib, entry, n, x, R, wanted, ref, ref_reduced=None, regime=None):
    """one host call against the reference of all outputs.  A NULL output changes no other output's bits, with the one exception
    include/pem_hip.h documents: the coupled model without a profile takes div_angle and T_c from tables, so those two (and
    invalid) are held to the device entry point called without a profile as well, and the rest to the full reference."""
    got = host_call(lib, entry, n, x, R, wanted, regime)
    assert set(got) == set(wanted)
    if entry == hc.COUPLED and 'j_ion' not in wanted:
        assert_same_bits(got, ref_reduced, [k for k in got if k in ('div_angle', 'T_c', 'invalid')])
        assert_same_bits(got, ref, [k for k in got if k in ('V_cc', 'I_B0', 'T')])
    else:
        assert_same_bits(got, ref)


# ---------------------------------------------------------------------------------------------- 1. every regime boundary
def _boundary_cases():
    for b in hc.BOUNDARIES:
        if b.entry == hc.PLUME and b.R not in (1, 3, 8):
            continue
        for n, regime in ((b.low, b.regime_low), (b.low + 1, b.regime_high)):
            yield pytest.param(b.entry, b.R, b.n_optional, n, regime, id=f'{hc.NAMES[b.entry]}-R{b.R}-k{b.n_optional}-n{n}-regime{regime}')


@pytest.mark.parametrize('entry, R, k, n, regime', list(_boundary_cases()))
def test_both_sides_of_every_regime_boundary(lib, entry, R, k, n, regime):
    x = make_inputs(entry, n, seed=n % 1000 + 7 * entry)
    chunk = c_plan(lib, entry, n, R).chunk
    ref = reference(lib, entry, n, x, R, chunk)
    assert_wild_rows_show(entry, ref)
    if entry == hc.THRUSTER:                   # the boundary belongs to this number of outputs: eight, one (I_d) or none
        wanted = hc.OUTPUTS[entry][:k] if k != 1 else ('I_d',)
        check_call(lib, entry, n, x, R, wanted, ref, regime=regime)
        return
    reduced = reference(lib, entry, n, x, R, chunk, [o for o in hc.OUTPUTS[entry] if o != 'j_ion']) if entry == hc.COUPLED else None
    for wanted in variants(entry):
        check_call(lib, entry, n, x, R, wanted, ref, reduced, regime=regime)


# ---------------------------------------------------------------------------------------------- 2. the thruster's optional outputs
def _thruster_subsets():
    o = hc.OUTPUTS[hc.THRUSTER]
    return [o, ()] + [(k,) for k in o] + [o[1:], o[:-1]]


@pytest.mark.parametrize('n', [1000, 10000, 50000, 70000])
def test_thruster_output_subsets_in_every_regime(lib, n):
    """all eight (exactly the capacity of the staged copy-back), none, each alone, all but the first, all but the last: at 1000
    samples every subset is zero-copy, at 10 000 staged both ways, at 50 000 the subsets of at most one output are staged both
    ways and the larger ones have only their inputs staged, at 70 000 every array is copied on its own"""
    x = make_inputs(hc.THRUSTER, n, seed=n // 1000)
    ref = reference(lib, hc.THRUSTER, n, x)
    assert_wild_rows_show(hc.THRUSTER, ref)
    seen = set()
    for wanted in _thruster_subsets():
        check_call(lib, hc.THRUSTER, n, x, 1, wanted, ref)
        seen.add(lib.pem_host_last_regime())
    assert seen == {1000: {0}, 10000: {1}, 50000: {1, 2}, 70000: {3}}[n]


# ---------------------------------------------------------------------------------------------- 3. two chunks, a ragged last one
@pytest.mark.parametrize('entry, R, profile', [(hc.COUPLED, 1, True), (hc.COUPLED, 1, False), (hc.PLUME, 8, True), (hc.PLUME, 300, True)],
                         ids=['coupled-profile', 'coupled-reduced', 'plume-R8', 'plume-R300'])
def test_two_chunks_with_one_sample_in_the_last(lib, entry, R, profile):
    """the last sample of the first chunk and the only sample of the second; about 270 MB of host output where the profile is
    written.  R = 300 is more radii than the kernels of pem_radii.hip take: the generic kernel and its stream-ordered
    allocation run inside the chunk loop."""
    t, = [t for t in hc.TWO_CHUNKS if (t.entry, t.R) == (entry, R)]
    n = t.chunk + 1
    plan = c_plan(lib, entry, n, R)
    assert (plan.chunk, plan.n_chunks, plan.regime) == (t.chunk, 2, t.regime)
    x = make_inputs(entry, n, seed=11 + R)
    wanted = tuple(k for k in hc.OUTPUTS[entry] if profile or k != 'j_ion')
    ref = reference(lib, entry, n, x, R, plan.chunk, wanted)
    assert_wild_rows_show(entry, ref)
    got = host_call(lib, entry, n, x, R, wanted, regime=t.regime)
    assert_same_bits(got, ref)
    for k in got:                                                      # said once more for the two samples at the seam
        w = hc.row_len(entry, k, R)
        assert np.array_equal(got[k][(n - 2) * w:], ref[k][(n - 2) * w:], equal_nan=True), k
    if 'j_ion' in ref:
        assert np.isfinite(ref['j_ion'][-hc.NANG * R:]).all() and np.isfinite(ref['j_ion'][-2 * hc.NANG * R:-hc.NANG * R]).all()
    del got, ref, x


# ---------------------------------------------------------------------------------------------- 4. nothing stale across calls
@pytest.mark.parametrize('entry, sizes', [(hc.COUPLED, (20000, 100, 1000, 5000, 200)), (hc.CATHODE, (50000, 3000, 20000, 40000, 4000))],
                         ids=['coupled', 'cathode'])
def test_a_ladder_of_calls_leaves_nothing_stale(lib, entry, sizes):
    """regime 3, then 0, 1, 2 and 0 again in one process, each call on inputs of its own: the grow-only workspace, the pinned
    mirror and the zero-copy base change hands between them"""
    for step, (n, regime) in enumerate(zip(sizes, (3, 0, 1, 2, 0))):
        x = make_inputs(entry, n, seed=100 + step)
        ref = reference(lib, entry, n, x, 1, c_plan(lib, entry, n).chunk)
        assert_wild_rows_show(entry, ref)
        check_call(lib, entry, n, x, 1, hc.OUTPUTS[entry], ref, regime=regime)


# ---------------------------------------------------------------------------------------------- 5. PEM_ZERO_COPY=0
ZERO_COPY_CASES = [(hc.CATHODE, 1, 4672), (hc.THRUSTER, 1, 2720), (hc.PLUME, 1, 256), (hc.PLUME, 3, 64), (hc.COUPLED, 1, 256)]


def _zero_copy_run(lib):
    """the regime-0 sizes of the four entry points: {name: array}, with the regime every call reported"""
    out = {}
    for entry, R, n in ZERO_COPY_CASES:
        x = make_inputs(entry, n, seed=5 + entry)
        got = host_call(lib, entry, n, x, R)
        tag = f'{hc.NAMES[entry]}_R{R}'
        out[tag + '_regime'] = np.array(lib.pem_host_last_regime())
        for k, v in got.items():
            out[f'{tag}_{k}'] = v
    return out


def test_zero_copy_switched_off_gives_the_same_bits_through_regime_1(lib, tmp_path):
    """PEM_ZERO_COPY is read once per process: one fresh process with it set to 0 runs the regime-0 sizes"""
    if os.environ.get('PEM_ZERO_COPY') is not None:
        pytest.fail('PEM_ZERO_COPY is set in the test process: this test needs the default')
    mine = _zero_copy_run(lib)
    path = tmp_path / 'zero_copy_off.npz'
    child = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path)], env=dict(os.environ, PEM_ZERO_COPY='0'),
                           capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    with np.load(path) as z:
        theirs = {k: z[k] for k in z.files}
    assert set(theirs) == set(mine)
    for k, v in mine.items():
        if k.endswith('_regime'):
            assert (int(v), int(theirs[k])) == (0, 1), k
        elif v.dtype == np.uint8:
            assert np.array_equal(v, theirs[k]), k
        else:
            assert np.array_equal(v.view(np.uint64), theirs[k].view(np.uint64)), k


# ---------------------------------------------------------------------------------------------- 6. refusals launch nothing
def test_refusals_launch_nothing(lib):
    n = 5000                                                              # a cathode call staged both ways comes first
    x = make_inputs(hc.CATHODE, n, seed=1)
    host_call(lib, hc.CATHODE, n, x, regime=1)
    cases = hc.malformed_calls()
    assert len(cases) > 40
    for label, entry, R, xin, wanted in cases:
        outs = hc.alloc_outputs(entry, 5, max(R, 1), wanted)
        assert hc.call_host(lib, entry, 5, xin, outs, R) == 1, label            # PEM_ERR_INVALID_ARG
        assert all(hc.untouched(a) for a in outs.values()), label
        assert lib.pem_host_last_regime() == 1, label


if __name__ == '__main__':                                                # the child of the PEM_ZERO_COPY=0 test
    sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]
    from hallthrusterpem_amd import _lib as _l
    _handle = _l.load()
    _l.require_device()
    np.savez(sys.argv[1], **_zero_copy_run(_handle))
