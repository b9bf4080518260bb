"""The shifted Sobol' design without a GPU: the library's direction numbers are torch's, the numpy restatement (tests/qmc_np.py) is
torch.quasirandom.SobolEngine and scipy.stats.qmc.Sobol(bits=30) bit for bit, the entry points are declared, bound, built and
exported and refuse every malformed call before they look for a device, the Python layer refuses what it cannot run before it
touches one, the shifted points keep the net property, the new kernels compile without scratch -- and the point of the feature:
on this model the design's means and first-order indices are an order of magnitude closer than independent draws."""
import ctypes as C
import re
import shutil
import subprocess
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import pytest

import qmc_np
from oracle import sampler_np as snp

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {'pem_sobol_directions': 2, 'pem_sample_sobol_f64_dev': 13, 'pem_saltelli_qmc_f32_dev': 16, 'pem_saltelli_qmc_f64_dev': 16}
FAKE = C.c_void_p(4096)                        # a device pointer that is never dereferenced: every check runs on the host
SEED = (0x9E3779B9 << 32) | 0x7F4A7C15
U01 = dict(kind=[0] * 32, a=[0.0] * 32, b=[1.0] * 32)


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------
def test_the_librarys_direction_numbers_are_torchs_and_dimension_32_is_refused():
    import torch
    from hallthrusterpem_amd import _lib
    lib = _lib.load()
    state = torch.quasirandom.SobolEngine(32).sobolstate.numpy()
    out = np.zeros(31, dtype=np.uint32)
    for d in range(32):
        out[:] = 0xDEADBEEF
        assert lib.pem_sobol_directions(d, C.c_void_p(out.ctypes.data)) == _lib.PEM_OK
        assert np.array_equal(out[:30].astype(np.int64), state[d]), d
        assert out[30] == 0xDEADBEEF                                             # thirty words, no more
    for bad in (32, -1, 1000):
        assert lib.pem_sobol_directions(bad, C.c_void_p(out.ctypes.data)) == _lib.PEM_ERR_INVALID_ARG
        assert b'pem_sobol_directions' in lib.pem_last_error()
    assert lib.pem_sobol_directions(0, None) == _lib.PEM_ERR_INVALID_ARG
    # the committed header is what the generator writes from torch
    gen = subprocess.run([sys.executable, str(ROOT / 'tools' / 'gen_sobol_seq.py'), '--check'], capture_output=True, text=True)
    assert gen.returncode == 0, gen.stdout + gen.stderr


# ---- 2. the restatement against torch and scipy ---------------------------------------------------------------------------------
def test_the_restatement_is_sobolengine_and_scipy_plus_half_a_cell_from_index_0():
    import torch
    from scipy.stats import qmc
    n = 5000
    got = qmc_np.sample(n, 0, SEED, 3, scramble=False, **U01)
    assert np.array_equal(got, torch.quasirandom.SobolEngine(32).draw(n, dtype=torch.float64).numpy().T + 2.0 ** -31)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)                             # "n must be a power of 2"
        sp = qmc.Sobol(32, scramble=False, bits=30).random(n)
    assert np.array_equal(got, sp.T + 2.0 ** -31)
    assert got.min() > 0.0 and got.max() < 1.0
    # sharding: any slice is the same numbers; the shift moves every dimension, by its own amount
    parts = np.concatenate([qmc_np.sample(1234, 0, SEED, 3, **U01), qmc_np.sample(n - 1234, 1234, SEED, 3, **U01)], axis=1)
    whole = qmc_np.sample(n, 0, SEED, 3, **U01)
    assert np.array_equal(parts, whole) and not np.any(np.all(whole == got, axis=1))
    assert len({int(qmc_np.shift(SEED, 3, d)) for d in range(32)}) == 32 and qmc_np.shift(SEED, 3, 0) != qmc_np.shift(SEED, 4, 0)
    assert all(int(qmc_np.shift(SEED, 3, d)) < 1 << 30 for d in range(32))


def test_the_restatement_is_sobolengine_and_scipy_after_fast_forward_where_the_gray_code_flips_its_top_bit():
    """from 2^29 - 70 (bit 29 of the Gray code switches on at 2^29) and the last 64 points, 2^30 - 64 .. 2^30 - 1.  The engines walk
    there point by point (about a minute for the two of them); the closed form needs no walk."""
    import torch
    from scipy.stats import qmc
    eng, sp = torch.quasirandom.SobolEngine(32), qmc.Sobol(32, scramble=False, bits=30)
    at = 0
    for first, n in ((2 ** 29 - 70, 140), (2 ** 30 - 64, 64)):
        eng.fast_forward(first - at)
        sp.fast_forward(first - at)
        at = first + n
        got = qmc_np.sample(n, first, SEED, 3, scramble=False, **U01)
        assert np.array_equal(got, eng.draw(n, dtype=torch.float64).numpy().T + 2.0 ** -31), first
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)
            assert np.array_equal(got, sp.random(n).T + 2.0 ** -31), first
    with pytest.raises(AssertionError):
        qmc_np.points(65, 2 ** 30 - 64, [0])                                     # the sequence ends at 2^30


# ---- 3. the entry points --------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    for name, n_args in ENTRY_POINTS.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header)
        assert m and len(m.group(1).split(',')) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_lib.load(), name)
    assert build.PKG / 'csrc' / 'pem_qmc.hip' in build.SRCS


def _host(values, dtype):
    return None if values is None else np.ascontiguousarray(values, dtype=dtype)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _sample(n=10, first=0, scramble=1, ndim=3, kind=(0, 1, 2), a=(0.0,) * 33, b=(1.0,) * 33, swap_dim=-1, out=FAKE, ld=16):
    from hallthrusterpem_amd import _lib
    kind, a, b = _host(kind, np.int32), _host(a, np.float64), _host(b, np.float64)
    return _lib.load().pem_sample_sobol_f64_dev(n, first, SEED, 3, scramble, ndim, _ptr(kind), _ptr(a), _ptr(b), swap_dim, out, ld, None)


def _id(bad):
    return '-'.join(f'{k}={"tuple" if isinstance(v, tuple) and len(v) > 3 else v}' for k, v in bad.items())


# (arguments, malformed when n == 0 as well)
SAMPLE_BAD = [(bad, True) for bad in (
    dict(ndim=0), dict(ndim=33, kind=(0,) * 33), dict(ndim=-1), dict(kind=None), dict(a=None), dict(b=None), dict(out=None),
    dict(kind=(0, 1, -1)), dict(kind=(0, 1, 3)), dict(kind=(3, 1, 0)), dict(swap_dim=-3), dict(swap_dim=3),
    dict(ndim=17, kind=(0,) * 17, swap_dim=-2), dict(ndim=17, kind=(0,) * 17, swap_dim=0), dict(ndim=32, kind=(0,) * 32, swap_dim=31),
    dict(first=2 ** 30 + 1), dict(first=2 ** 64 - 5))]
SAMPLE_BAD += [(dict(ld=9), False), (dict(first=2 ** 30 - 9), False), (dict(first=2 ** 30), False)]
SAMPLE_CASES = [(bad, n) for bad, empty_too in SAMPLE_BAD for n in ((10, 0) if empty_too else (10,))]


@pytest.mark.parametrize('bad, n', SAMPLE_CASES, ids=[f'{_id(bad)}-n{n}' for bad, n in SAMPLE_CASES])
def test_malformed_sobol_design_calls_are_refused_without_a_device_whatever_n_is(bad, n):
    from hallthrusterpem_amd import _lib
    assert _sample(n=n, **bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_sample_sobol' in _lib.load().pem_last_error()


def _saltelli(entry='f64', n_base=10, first=0, kind=(0,) * 15, a=(0.0,) * 15, b=(1.0,) * 15, n_varied=2, varied=(2, 8), partial=FAKE,
              flags=FAKE, n_blocks=4):
    from hallthrusterpem_amd import _lib
    kind, a, b, varied = _host(kind, np.int32), _host(a, np.float64), _host(b, np.float64), _host(varied, np.int32)
    fn = getattr(_lib.load(), f'pem_saltelli_qmc_{entry}_dev')
    return fn(n_base, first, SEED, 3, 1, _ptr(kind), _ptr(a), _ptr(b), n_varied, _ptr(varied), 133.3, 1.0, partial, flags, n_blocks, None)


@pytest.mark.parametrize('entry', ['f32', 'f64'])
@pytest.mark.parametrize('bad', [dict(kind=None), dict(a=None), dict(b=None), dict(varied=None), dict(partial=None), dict(flags=None),
                                 dict(n_varied=0), dict(n_varied=16), dict(n_blocks=0), dict(first=2 ** 30 - 9), dict(first=2 ** 30 + 1),
                                 dict(n_base=0, first=2 ** 30 + 1), dict(first=2 ** 64 - 5)], ids=_id)
def test_malformed_fused_saltelli_calls_are_refused_without_a_device(entry, bad):
    from hallthrusterpem_amd import _lib
    assert _saltelli(entry, **bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert f'pem_saltelli_qmc_{entry}'.encode() in _lib.load().pem_last_error()


def test_well_formed_calls_get_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    assert _sample(n=0) == _lib.PEM_OK and _sample(n=0, first=2 ** 30) == _lib.PEM_OK     # an empty well-formed call needs no device
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    want = _lib.PEM_ERR_NO_DEVICE
    assert _sample() == want and _sample(scramble=0) == want and _sample(first=2 ** 30 - 10) == want       # ends exactly at 2^30
    assert _sample(ndim=32, kind=(2,) * 32, ld=10) == want and _sample(ndim=1, kind=(1,)) == want
    assert _sample(ndim=16, kind=(0,) * 16, swap_dim=-2) == want and _sample(ndim=16, kind=(0,) * 16, swap_dim=15) == want
    assert _sample(ndim=17, kind=(0,) * 17) == want                                                        # matrix A alone: 17 dimensions
    for entry in ('f32', 'f64'):
        assert _saltelli(entry) == want and _saltelli(entry, first=2 ** 30 - 10) == want
        assert _saltelli(entry, n_varied=15, varied=tuple(range(15)), n_blocks=1) == want


# ---- 4. the Python layer --------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    import torch
    from hallthrusterpem_amd import _lib
    for name in ('current_device', 'current_stream'):
        monkeypatch.setattr(torch.cuda, name, lambda *a, **k: pytest.fail('touched a device'))
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('loaded the library'))


@pytest.mark.parametrize('ndim, kw, match', [
    (33, dict(), '1 to 32 dimensions'),
    (17, dict(swap_dim=-2), '2 ndim <= 32'),
    (17, dict(swap_dim=3), '2 ndim <= 32'),
    (15, dict(swap_dim=15), 'out of range'),
    (15, dict(swap_dim=-3), 'out of range'),
    (15, dict(first_index=2 ** 30 - 99), '2\\^30 points'),
    (15, dict(first_index=-1), '2\\^30 points'),
])
def test_design_fill_refuses_a_sobol_design_it_cannot_write_before_touching_a_device(ndim, kw, match, monkeypatch):
    from hallthrusterpem_amd.sampling import Design, Prior, UNIFORM
    names = tuple(f'x{i}' for i in range(ndim))
    d = Design(priors={k: Prior(UNIFORM, 0.0, 1.0, 'test') for k in names}, names=names, seed=1)
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        d.fill(types.SimpleNamespace(shape=(ndim, 100)), method='sobol', **kw)


@pytest.mark.parametrize('kw, match', [
    (dict(design='lhs'), "'mc' or 'sobol'"),
    (dict(design='qmc'), "'mc' or 'sobol'"),
    (dict(design='sobol', n_base=2 ** 30 + 1), '2\\^30 points'),
])
def test_sobol_indices_and_saltelli_sums_refuse_bad_designs_before_touching_a_device(kw, match, monkeypatch):
    from hallthrusterpem_amd import drivers, fp32, sampling
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        drivers.sobol_indices(**dict(dict(n_base=100), **kw))
    d = sampling.Design(seed=1)
    with pytest.raises(ValueError, match=match):
        fp32.saltelli_sums(d, [2, 8], kw.get('n_base', 100), method=kw['design'])
    with pytest.raises(ValueError, match='2\\^30 points'):
        fp32.saltelli_sums(d, [2, 8], 100, first_index=2 ** 30 - 99, method='sobol')


# ---- 5. the net property --------------------------------------------------------------------------------------------------------
def test_the_shifted_points_of_an_aligned_block_fill_every_cell_of_every_dimension_once():
    n = 2 ** 10
    for seed in (SEED, 5):
        u = qmc_np.uniforms(n, 3 * n, seed, 3, list(range(15)))
        cells = np.floor(u * n).astype(np.int64)
        for d in range(15):
            assert np.array_equal(np.sort(cells[d]), np.arange(n)), d
        assert len({cells[d].tobytes() for d in range(15)}) == 15
    # matrix B of a 15-dimensional Saltelli block: sequence dimensions 15 .. 29, its own shifts
    assert qmc_np.seq_dims(15, -2) == list(range(15, 30)) and qmc_np.seq_dims(15, 4) == [0, 1, 2, 3, 19] + list(range(5, 15))
    kind, a, b = [0, 1, 2] * 5, [0.0, -8.0, 30.0] * 5, [1.0, -4.0, 2.0] * 5
    A, B = qmc_np.sample(200, 7, SEED, 3, kind, a, b), qmc_np.sample(200, 7, SEED, 3, kind, a, b, swap_dim=-2)
    for sd in (0, 7, 14):
        AB = qmc_np.sample(200, 7, SEED, 3, kind, a, b, swap_dim=sd)
        assert all(np.array_equal(AB[d], (B if d == sd else A)[d]) for d in range(15)) and not np.array_equal(A[sd], B[sd])
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(B))                      # the midpoint is never 0 or 1: Phi^-1 stays finite


# ---- 6. the point of the feature ------------------------------------------------------------------------------------------------
def _priors():
    from hallthrusterpem_amd.sampling import Design
    d = Design()
    return list(d.kind), list(d.a), list(d.b)


N = 4096


def test_means_of_a_4096_point_design_are_within_a_quarter_of_a_monte_carlo_standard_error():
    """15 PEM-v0 priors, n = 4096, seeds 1..8; truth = the unshifted 2^20-point mean by the oracle; sigma = the oracle's sample
    standard deviation over 2^16 Monte-Carlo points of oracle/sampler_np.py.  Every |mean - truth| <= 0.25 sigma / sqrt(n): the
    worst seen over 8 other shifts was 0.083, so the bound leaves a margin of 3 for the shift-to-shift spread (independent draws:
    about 1)."""
    kind, a, b = _priors()
    truth = np.zeros(3)
    for lo in range(0, 1 << 20, 1 << 17):
        truth += qmc_np.oracle_qois(qmc_np.sample(1 << 17, lo, 0, 0, kind, a, b, scramble=False)).sum(1)
    truth /= 1 << 20
    sigma = qmc_np.oracle_qois(snp.sample(1 << 16, 0, 1, 0, kind, a, b)).std(axis=1, ddof=1)
    se = sigma / np.sqrt(N)
    worst = np.zeros(3)
    for seed in range(1, 9):
        err = np.abs(qmc_np.oracle_qois(qmc_np.sample(N, 0, seed, 0, kind, a, b)).mean(1) - truth) / se
        print(f'seed {seed}: |mean - truth| / (sigma / sqrt n) = {err}')
        worst = np.maximum(worst, err)
        assert np.all(err <= 0.25), (seed, err)
    print('worst', worst)


# measured on the restatement with the oracle as the model: worst |S1 - ref| over the 15 inputs and seeds 1..4, per QoI
MEASURED_S1 = {'V_cc': 0.00118, 'div_angle': 0.00888, 'T_c': 0.01384}


def test_first_order_indices_of_a_4096_point_design_against_independent_draws():
    """Saltelli, n_base = 4096, all 15 inputs, seeds 1..4, against the unshifted 2^18-point design.  Measured here on the
    restatement, worst |S1 - ref| over inputs and seeds for V_cc / div_angle / T_c: 0.00118 / 0.00888 / 0.01384 (MEASURED_S1;
    per seed 0.00097 0.00574 0.01069 | 0.00084 0.00345 0.00955 | 0.00076 0.00888 0.01040 | 0.00118 0.00349 0.01384); asserted at
    3 x that (the shift-to-shift spread), and below half the same figure of the Monte-Carlo design of oracle/sampler_np.py at the
    same n and seeds (measured: 0.0432 / 0.1233 / 0.0529)."""
    kind, a, b = _priors()
    varied = list(range(15))
    ref = qmc_np.saltelli(qmc_np.oracle_qois, 1 << 18, 0, 0, 0, kind, a, b, varied, scramble=False)[0]
    worst_q, worst_mc = np.zeros(3), np.zeros(3)
    for seed in range(1, 5):
        S1, _, _, _ = qmc_np.saltelli(qmc_np.oracle_qois, N, 0, seed, 0, kind, a, b, varied)
        M1, _, _, _ = qmc_np.saltelli(qmc_np.oracle_qois, N, 0, seed, 0, kind, a, b, varied,
                                      sampler=lambda sd: snp.sample(N, 0, seed, 0, kind, a, b, swap_dim=sd))
        worst_q = np.maximum(worst_q, np.abs(S1 - ref).max(0))
        worst_mc = np.maximum(worst_mc, np.abs(M1 - ref).max(0))
    print("worst |S1 - ref| Sobol'", worst_q, 'Monte-Carlo', worst_mc)
    for i, q in enumerate(('V_cc', 'div_angle', 'T_c')):
        assert worst_q[i] <= 3.0 * MEASURED_S1[q], (q, worst_q[i])
        assert worst_q[i] < 0.5 * worst_mc[i], (q, worst_q[i], worst_mc[i])


# ---- 7. the kernels -------------------------------------------------------------------------------------------------------------
def _stats(src):
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / src)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+) kernarg\s+(\d+) lds\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), vspill=int(m.group(5)), scratch=int(m.group(6)), kernarg=int(m.group(7)))
    return rows


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_the_new_kernels_have_no_scratch_and_no_vector_spills():
    rows = _stats('pem_qmc.hip')
    assert list(rows) == ['sobol_sample_kernel'], rows
    r = rows['sobol_sample_kernel']
    assert r['vspill'] == 0 and r['scratch'] == 0 and r['vgpr'] <= 64, r       # the transform is out of line: as light as sample_kernel
    rows = _stats('pem_saltelli.hip')
    assert sorted(rows) == ['saltelli_kernel<Model32>', 'saltelli_kernel<Model64>', 'saltelli_qmc_kernel<Model32>', 'saltelli_qmc_kernel<Model64>'], rows
    for name, r in rows.items():
        assert r['vspill'] == 0 and r['scratch'] == 0, (name, r)
    assert rows['saltelli_qmc_kernel<Model64>']['vgpr'] <= 256 and rows['saltelli_qmc_kernel<Model32>']['vgpr'] <= 128, rows
    # the Monte-Carlo instantiations are what they were: 127 / 198 registers, 680 bytes of arguments
    assert rows['saltelli_kernel<Model32>'] == dict(vgpr=127, vspill=0, scratch=0, kernarg=680), rows
    assert rows['saltelli_kernel<Model64>'] == dict(vgpr=198, vspill=0, scratch=0, kernarg=680), rows
