"""The sampler's entry points without a GPU: the six of csrc/pem_sampler.hip and pem_thruster_filter_f64_dev are declared, bound,
built and exported, and refuse every malformed call before they look for a device -- whatever n is, an empty call included;
the numpy restatement (oracle/sampler_np.py) is pinned at the Latin-hypercube and stream edges where
tests/test_sampler_kernels.py leans on it."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import sampler_np as snp

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {'pem_sample_f64_dev': 12, 'pem_sample_tiled_f64_dev': 11, 'pem_sample_lhs_f64_dev': 12, 'pem_sobol_partial_f64_dev': 9,
                'pem_predictive_inputs_f64_dev': 17, 'pem_predictive_noise_f64_dev': 11, 'pem_thruster_filter_f64_dev': 10}
FAKE = C.c_void_p(4096)                        # a device pointer that is never dereferenced: every check runs on the host
SEED = (0x9E3779B9 << 32) | 0x7F4A7C15


def test_the_entry_points_are_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    for name, n_args in ENTRY_POINTS.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header)
        assert m and len(m.group(1).split(',')) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_lib.load(), name)
    assert re.search(r'#define PEM_SAMPLE_MAX_DIM (\d+)', header).group(1) == '32'
    assert build.PKG / 'csrc' / 'pem_sampler.hip' in build.SRCS and build.PKG / 'csrc' / 'pem_stages.hip' in build.SRCS


def _host(values, dtype):
    return None if values is None else np.ascontiguousarray(values, dtype=dtype)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _sample(entry, n=10, first=0, n_total=100, ndim=3, kind=(0, 1, 2), a=(0.0,) * 33, b=(1.0,) * 33, swap_dim=-1, out=FAKE, ld=16):
    """kind, a, b are host arrays (kind is read by the checks); `out` is the only device pointer"""
    from hallthrusterpem_amd import _lib
    lib = _lib.load()
    kind, a, b = _host(kind, np.int32), _host(a, np.float64), _host(b, np.float64)
    if entry == 'mc':
        return lib.pem_sample_f64_dev(n, first, SEED, 3, ndim, _ptr(kind), _ptr(a), _ptr(b), swap_dim, out, ld, None)
    if entry == 'tiled':
        return lib.pem_sample_tiled_f64_dev(n, first, SEED, 3, ndim, _ptr(kind), _ptr(a), _ptr(b), swap_dim, out, None)
    return lib.pem_sample_lhs_f64_dev(n, first, n_total, SEED, 3, ndim, _ptr(kind), _ptr(a), _ptr(b), out, ld, None)


def _id(bad):
    return '-'.join(f'{k}={"tuple" if isinstance(v, tuple) and len(v) > 3 else v}' for k, v in bad.items())


# (entry, arguments, malformed when n == 0 as well)
SAMPLE_BAD = [(e, bad, True) for e in ('mc', 'tiled', 'lhs') for bad in (
    dict(ndim=0), dict(ndim=33, kind=(0,) * 33), dict(ndim=-1), dict(kind=None), dict(a=None), dict(b=None), dict(out=None),
    dict(kind=(0, 1, -1)), dict(kind=(0, 1, 3)), dict(kind=(3, 1, 0)), dict(kind=(0, -1, 2)))]
SAMPLE_BAD += [(e, dict(ld=9), False) for e in ('mc', 'lhs')]
SAMPLE_BAD += [(e, dict(swap_dim=s), True) for e in ('mc', 'tiled') for s in (-3, 3)]
SAMPLE_BAD += [('lhs', dict(n_total=0), True), ('lhs', dict(first=101), True), ('lhs', dict(first=95), False),
               ('lhs', dict(first=91), False), ('lhs', dict(first=2 ** 64 - 5, n_total=2 ** 64 - 1), False)]   # first + n wraps
SAMPLE_CASES = [(e, bad, n) for e, bad, empty_too in SAMPLE_BAD for n in ((10, 0) if empty_too else (10,))]


@pytest.mark.parametrize('entry, bad, n', SAMPLE_CASES, ids=[f'{e}-{_id(bad)}-n{n}' for e, bad, n in SAMPLE_CASES])
def test_malformed_design_calls_are_refused_without_a_device_whatever_n_is(entry, bad, n):
    from hallthrusterpem_amd import _lib
    assert _sample(entry, n=n, **bad) == _lib.PEM_ERR_INVALID_ARG, (entry, bad)
    assert b'pem_sample' in _lib.load().pem_last_error()


def test_well_formed_design_calls_get_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    for entry in ('mc', 'tiled', 'lhs'):
        assert _sample(entry, n=0) == _lib.PEM_OK                              # an empty well-formed call needs no device
    assert _sample('lhs', n=0, first=100) == _lib.PEM_OK
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    for entry in ('mc', 'tiled', 'lhs'):
        assert _sample(entry) == _lib.PEM_ERR_NO_DEVICE
        assert _sample(entry, ndim=32, kind=(2,) * 32, ld=10) == _lib.PEM_ERR_NO_DEVICE
        assert _sample(entry, ndim=1, kind=(1,)) == _lib.PEM_ERR_NO_DEVICE
    for sd in (-2, 0, 2):
        assert _sample('mc', swap_dim=sd) == _lib.PEM_ERR_NO_DEVICE and _sample('tiled', swap_dim=sd) == _lib.PEM_ERR_NO_DEVICE
    assert _sample('lhs', first=90) == _lib.PEM_ERR_NO_DEVICE                  # ends exactly at n_total
    assert _sample('lhs', n=1, n_total=1) == _lib.PEM_ERR_NO_DEVICE


# ---- the other entry points -----------------------------------------------------------------------------------------------------
def _sobol(m=10, nq=3, ld=16, fA=FAKE, fB=FAKE, fAB=FAKE, partial=FAKE, n_blocks=4):
    from hallthrusterpem_amd import _lib
    return _lib.load().pem_sobol_partial_f64_dev(m, nq, ld, fA, fB, fAB, partial, n_blocks, None)


def _inputs(n=10, n_cond=2, kind=(0,) * 15, a=(0.0,) * 15, b=(1.0,) * 15, operating=FAKE, samples=FAKE, n_samples=50, n_theta=2,
            theta_rows=(2, 8), out=FAKE, ld=16):
    from hallthrusterpem_amd import _lib
    kind, a, b, rows = _host(kind, np.int32), _host(a, np.float64), _host(b, np.float64), _host(theta_rows, np.int32)
    return _lib.load().pem_predictive_inputs_f64_dev(n, n_cond, 0, SEED, 3, _ptr(kind), _ptr(a), _ptr(b), operating, samples, n_samples,
                                                     n_theta, _ptr(rows), 7, out, ld, None)


def _noise(n_rows=10, m=4, pred=FAKE, ld_pred=4, sigma=FAKE, out=FAKE, ld_out=6):
    from hallthrusterpem_amd import _lib
    return _lib.load().pem_predictive_noise_f64_dev(n_rows, m, pred, ld_pred, sigma, 0, SEED, 3, out, ld_out, None)


def _filter(n=10, ncells=20, u_ion=FAKE, z=FAKE, use_shock=1, T=FAKE, I_B0=FAKE, flags=FAKE):
    from hallthrusterpem_amd import _lib
    return _lib.load().pem_thruster_filter_f64_dev(n, ncells, u_ion, z, 0.04, use_shock, T, I_B0, flags, None)


OTHER_BAD = [(_sobol, 'pem_sobol_partial', bad) for bad in (
    dict(nq=0), dict(nq=9), dict(nq=-1), dict(n_blocks=0), dict(n_blocks=-2), dict(ld=9), dict(fA=None), dict(fB=None), dict(partial=None))]
OTHER_BAD += [(_inputs, 'pem_predictive_inputs', bad) for bad in (
    dict(n_cond=0), dict(n_theta=-1), dict(n_theta=16), dict(theta_rows=None), dict(n_samples=0), dict(n_samples=2 ** 32),
    dict(n_theta=0, theta_rows=None), dict(kind=None), dict(a=None), dict(b=None), dict(operating=None), dict(out=None), dict(ld=9),
    dict(kind=(0,) * 14 + (3,)), dict(kind=(-1,) + (0,) * 14), dict(theta_rows=(0, 8)), dict(theta_rows=(2, 6)), dict(theta_rows=(2, 15)),
    dict(theta_rows=(-1, 8)), dict(theta_rows=(8, 8)))]
OTHER_BAD += [(_noise, 'pem_predictive_noise', bad) for bad in (
    dict(m=-1), dict(ld_pred=3), dict(ld_out=3), dict(pred=None), dict(sigma=None), dict(out=None))]
OTHER_BAD += [(_filter, 'pem_thruster_filter', bad) for bad in (
    dict(flags=None), dict(u_ion=None), dict(z=None), dict(ncells=0), dict(flags=None, use_shock=0))]


@pytest.mark.parametrize('call, prefix, bad', OTHER_BAD, ids=[f'{prefix}-{_id(bad)}' for _, prefix, bad in OTHER_BAD])
def test_malformed_calls_of_the_other_entry_points_are_refused_without_a_device(call, prefix, bad):
    from hallthrusterpem_amd import _lib
    assert call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert prefix.encode() in _lib.load().pem_last_error()


def test_well_formed_calls_of_the_other_entry_points_get_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    assert _inputs(n=0) == _lib.PEM_OK and _noise(n_rows=0) == _lib.PEM_OK and _noise(m=0, ld_pred=0, ld_out=0) == _lib.PEM_OK
    assert _filter(n=0) == _lib.PEM_OK
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    want = _lib.PEM_ERR_NO_DEVICE
    assert _sobol() == want and _sobol(fAB=None) == want and _sobol(nq=1) == want and _sobol(nq=8, ld=10, n_blocks=1) == want
    assert _inputs() == want and _inputs(samples=None, n_samples=0) == want
    assert _inputs(samples=None, n_samples=0, n_theta=0, theta_rows=None) == want
    assert _inputs(n_theta=12, theta_rows=[d for d in range(15) if d not in (0, 1, 6)], n_samples=2 ** 32 - 1, ld=10) == want
    assert _noise() == want and _noise(m=1, ld_pred=1, ld_out=1) == want
    assert _filter() == want and _filter(T=None, I_B0=None) == want and _filter(u_ion=None, z=None, ncells=0, use_shock=0) == want


# ---- the numpy restatement where the GPU tests lean on it -----------------------------------------------------------------------
@pytest.mark.parametrize('n_total', [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4096, 4097])
def test_the_restated_latin_hypercube_hits_every_stratum_once_at_the_feistel_edges(n_total):
    """a seed with two non-zero words, stream 0xFFFFFFFE, three shards: every stratum once in every dimension, all below 1"""
    kw = dict(seed=SEED, stream=0xFFFFFFFE, kind=[0] * 5, a=[0.0] * 5, b=[1.0] * 5, mode='lhs', n_total=n_total)
    cuts = [0, n_total // 3, 2 * n_total // 3, n_total]
    L = np.concatenate([snp.sample(hi - lo, lo, **kw) for lo, hi in zip(cuts[:-1], cuts[1:])], axis=1)
    assert L.shape == (5, n_total) and L.min() >= 0.0 and L.max() < 1.0
    assert np.array_equal(L, snp.sample(n_total, 0, **kw))
    cells = np.floor(L * n_total).astype(np.int64)
    for d in range(5):
        assert np.array_equal(np.sort(cells[d]), np.arange(n_total)), d
    if n_total >= 15:
        assert len({cells[d].tobytes() for d in range(5)}) == 5                # five permutations
        other = snp.sample(n_total, 0, **dict(kw, seed=SEED ^ (0xFFFF << 32)))  # the high word of the seed keys them
        assert all(not np.array_equal(np.floor(other[d] * n_total), cells[d]) for d in range(5))


def test_the_restated_stream_plus_one_wraps_and_a_pair_splits_at_either_member():
    kind, a, b = [0, 1, 2, 0, 1], [0.0, -8.0, 30.0, 2.0, -3.0], [1.0, -4.0, 2.0, 5.0, 1.0]
    first = 2 ** 32 - 70
    B = snp.sample(130, first, SEED, 0xFFFFFFFF, kind, a, b, swap_dim=-2)
    assert np.array_equal(B, snp.sample(130, first, SEED, 0, kind, a, b))
    A = snp.sample(130, first, SEED, 0xFFFFFFFF, kind, a, b)
    for sd in range(5):                                                         # even members, odd members, the lone last dimension
        AB = snp.sample(130, first, SEED, 0xFFFFFFFF, kind, a, b, swap_dim=sd)
        assert all(np.array_equal(AB[d], (B if d == sd else A)[d]) for d in range(5)) and not np.array_equal(A[sd], B[sd])
    whole = snp.sample(130, first, SEED, 5, kind, a, b)                         # the index carries into its high word at column 70
    assert np.array_equal(whole[:, 70:], snp.sample(60, 2 ** 32, SEED, 5, kind, a, b))
    assert not np.array_equal(whole[:, 70:], snp.sample(60, 0, SEED, 5, kind, a, b))
