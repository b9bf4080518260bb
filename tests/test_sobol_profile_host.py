"""Sobol' indices of a vector output without a GPU: the numpy restatement (tests/sobol_profile_np.py) is held to
`scipy.stats.sobol_indices` on an analytic function with 4 outputs and 3 inputs, one of them inert; `sobol_profile.indices` (the
tensors the driver returns) is held to the restatement; the entry points are declared, bound, built and exported and refuse
malformed calls before they look for a device; `drivers.sobol_profile` refuses what it cannot run before it touches one."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import sobol_profile_np as sp

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {'pem_saltelli_profile_f64_dev': 17, 'pem_saltelli_profile_qmc_f64_dev': 18}
FAKE = C.c_void_p(4096)                        # a device pointer that is never dereferenced: every check runs on the host
N, D, K = 512, 3, 4


def _f(x):
    """[3][n] -> [4][n]; input 2 is inert"""
    k = np.arange(K, dtype=np.float64)[:, None]
    return 3.0 + (k + 1.0) * np.sin(2.0 * np.pi * x[0]) + (4.0 - k) * x[1] ** 2 + k * x[0] * x[1]


@pytest.fixture(scope='module')
def study():
    rng = np.random.default_rng(20240607)
    A, B = rng.random((D, N)), rng.random((D, N))
    fA, fB, fAB = sp.evaluate(_f, A, B, range(D))
    return fA, fB, fAB


@pytest.fixture(scope='module')
def scipy_result(study):
    from scipy.stats import sobol_indices
    fA, fB, fAB = study
    return sobol_indices(func={'f_A': fA, 'f_B': fB, 'f_AB': fAB}, n=N)


def test_total_order_equals_scipy(study, scipy_result):
    fA, fB, fAB = study
    for centre in (np.zeros(K), np.array([1.0, -2.0, 7.5, 3.0])):                     # ST does not see the centre
        rows, _, _ = sp.sums_of(fA, fB, fAB, centre)
        got = sp.indices(rows, N, centre)
        worst = np.max(np.abs(got['ST'] - scipy_result.total_order))
        print('max |ST - scipy|', worst)
        assert got['ST'].shape == (K, D) and worst <= 1e-12


def test_first_order_with_the_pooled_mean_as_centre_equals_scipy(study, scipy_result):
    fA, fB, fAB = study
    centre = np.mean([fA, fB], axis=(0, -1))                                          # scipy centres with exactly this mean
    rows, _, _ = sp.sums_of(fA, fB, fAB, centre)
    got = sp.indices(rows, N, centre)
    worst = np.max(np.abs(got['S1'] - scipy_result.first_order))
    print('max |S1 - scipy|', worst)
    assert worst <= 1e-12
    assert np.max(np.abs(got['mean'] - centre)) <= 1e-12 and np.max(np.abs(got['var'] - np.var([fA, fB], axis=(0, -1)))) <= 1e-12
    # the uncentred estimate is another number: the check above is not vacuous
    raw = sp.indices(sp.sums_of(fA, fB, fAB, np.zeros(K))[0], N, np.zeros(K))
    assert np.max(np.abs(raw['S1'] - scipy_result.first_order)) > 1e-3


def test_the_inert_input_has_exactly_zero_indices(study):
    fA, fB, fAB = study
    centre = sp.pilot_centre(fA, fB)
    rows, mag, _ = sp.sums_of(fA, fB, fAB, centre)
    assert not rows[2 + 4 * 2:6 + 4 * 2].any() and not mag[2 + 4 * 2:6 + 4 * 2].any()
    got = sp.indices(rows, N, centre)
    for key in ('S1', 'ST', 'S1_se', 'ST_se'):
        assert not got[key][:, 2].any(), key
    assert got['GS1'][2] == 0.0 and got['GST'][2] == 0.0
    assert np.all(got['ST'][:, :2] > 0)


def test_the_aggregates_are_the_stated_ratio_of_sums(study):
    fA, fB, fAB = study
    centre = sp.pilot_centre(fA, fB)
    rows, _, _ = sp.sums_of(fA, fB, fAB, centre)
    got = sp.indices(rows, N, centre)
    for j in range(D):
        assert got['GS1'][j] == (rows[2 + 4 * j] / N).sum() / got['var'].sum()
        assert got['GST'][j] == (rows[4 + 4 * j] / N).sum() / (2 * got['var'].sum())
    # ... which is the variance-weighted mean of the indices
    assert np.allclose(got['GS1'], (got['S1'] * got['var'][:, None]).sum(axis=0) / got['var'].sum(), rtol=1e-13, atol=1e-15)
    assert np.allclose(got['GST'], (got['ST'] * got['var'][:, None]).sum(axis=0) / got['var'].sum(), rtol=1e-13, atol=1e-15)


def test_the_standard_errors_equal_a_direct_computation(study):
    fA, fB, fAB = study
    centre = sp.pilot_centre(fA, fB)
    rows, _, _ = sp.sums_of(fA, fB, fAB, centre)
    got = sp.indices(rows, N, centre)
    c = centre[:, None]
    for j in range(2):
        t1 = (fB - c) * (fAB[j] - fA)
        t2 = (fA - fAB[j]) ** 2
        assert np.allclose(got['S1_se'][:, j], np.std(t1, axis=1) / np.sqrt(N) / got['var'], rtol=1e-10, atol=0)
        assert np.allclose(got['ST_se'][:, j], np.std(t2, axis=1) / np.sqrt(N) / (2 * got['var']), rtol=1e-10, atol=0)


def test_long_double_sums_and_the_terms_agree_with_the_plain_ones(study):
    fA, fB, fAB = study
    centre = sp.pilot_centre(fA, fB)
    rows, mag, form = sp.sums_of(fA, fB, fAB, centre)
    rows_ld, mag_ld, _ = sp.sums_of(fA, fB, fAB, centre, dtype=sp.LD)
    t, m, form_t = sp.terms(fA, fB, fAB, centre)
    assert rows_ld.dtype == sp.LD and rows.shape == (sp.n_rows(D), K) and form.tolist() == form_t.tolist() == [2, 4] + [3, 7, 3, 7] * D
    assert np.all(np.abs(rows - rows_ld) <= (N + 8) * 2.0 ** -53 * mag_ld)
    assert np.array_equal(t.sum(axis=2), rows) and np.array_equal(m.sum(axis=2), mag) and np.all(m >= np.abs(t))


def test_the_tensor_arithmetic_of_the_package_equals_the_restatement(study):
    import torch
    from hallthrusterpem_amd import sobol_profile
    fA, fB, fAB = study
    centre = sp.pilot_centre(fA, fB)
    rows, _, _ = sp.sums_of(fA, fB, fAB, centre)
    want = sp.indices(rows, N, centre)
    got = sobol_profile.indices(torch.from_numpy(rows), N, torch.from_numpy(centre))
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        assert got[key].shape == w.shape, key
        assert np.allclose(got[key].numpy(), w, rtol=1e-13, atol=1e-300), key
    # a constant output: the division's own NaN
    flat = sobol_profile.indices(torch.zeros((6, 5), dtype=torch.float64), 10, torch.ones(5, dtype=torch.float64))
    assert torch.isnan(flat['S1']).all() and torch.isnan(flat['ST']).all() and torch.equal(flat['mean'], torch.ones(5, dtype=torch.float64))


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    for name, n_args in ENTRY_POINTS.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header)
        assert m and len(m.group(1).split(',')) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_lib.load(), name)
        assert name in (ROOT / 'INTEGRATION.md').read_text(), name
    assert build.PKG / 'csrc' / 'pem_saltelli_profile.hip' in build.SRCS


def _host(values, dtype):
    return None if values is None else np.ascontiguousarray(values, dtype=dtype)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def launch(entry='f64', n_base=10, first=0, kind=(0,) * 15, a=(0.0,) * 15, b=(1.0,) * 15, n_varied=2, varied=(2, 8), norm=1, centre=None,
           radius=1.0, partial=FAKE, flags=FAKE, n_blocks=4):
    from hallthrusterpem_amd import _lib
    kind, a, b, varied = _host(kind, np.int32), _host(a, np.float64), _host(b, np.float64), _host(varied, np.int32)
    fn = getattr(_lib.load(), f'pem_saltelli_profile_{entry}_dev')
    head = (n_base, first, 12345, 3) + ((1,) if entry.startswith('qmc') else ())
    return fn(*head, _ptr(kind), _ptr(a), _ptr(b), n_varied, _ptr(varied), norm, centre, 133.3, radius, partial, flags, n_blocks, None)


BAD = [dict(n_varied=-1), dict(n_varied=16), dict(norm=-1), dict(norm=2), dict(n_blocks=0), dict(n_blocks=-3), dict(radius=0.0),
       dict(radius=-1.0), dict(radius=float('nan')), dict(partial=None), dict(flags=None), dict(kind=None), dict(a=None), dict(b=None),
       dict(varied=None), dict(partial=None, n_base=0)]
BAD_QMC = [dict(first=2 ** 30 - 9), dict(first=2 ** 30 + 1), dict(n_base=0, first=2 ** 30 + 1), dict(n_base=2 ** 30 + 1)]
CASES = [(e, bad) for e in ('f64', 'qmc_f64') for bad in BAD + (BAD_QMC if e.startswith('qmc') else [])]


@pytest.mark.parametrize('entry, bad', CASES, ids=[f'{e}-' + '-'.join(f'{k}={v}' for k, v in bad.items()) for e, bad in CASES])
def test_malformed_calls_are_refused_without_a_device(entry, bad):
    from hallthrusterpem_amd import _lib
    assert launch(entry, **bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert f'pem_saltelli_profile_{entry}'.encode() in _lib.load().pem_last_error()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    import torch
    from hallthrusterpem_amd import _lib
    for name in ('current_device', 'current_stream'):
        monkeypatch.setattr(torch.cuda, name, lambda *a, **k: pytest.fail('touched a device'))
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('loaded the library'))


@pytest.mark.parametrize('kw, match', [
    (dict(norm='ln'), "'log10' or 'none'"),
    (dict(design='lhs'), "'mc' or 'sobol'"),
    (dict(n_base=0), 'at least 1'),
    (dict(n_base=-5), 'at least 1'),
    (dict(radius=0.0), 'radius must be positive'),
    (dict(radius=-2.0), 'radius must be positive'),
    (dict(design='sobol', n_base=2 ** 30 + 1), '2\\^30 points'),
])
def test_sobol_profile_refuses_what_it_cannot_run_before_touching_a_device(kw, match, monkeypatch):
    from hallthrusterpem_amd import drivers
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        drivers.sobol_profile(**dict(dict(n_base=100), **kw))


def test_profile_sums_refuses_bad_arguments_before_touching_a_device(monkeypatch):
    from hallthrusterpem_amd import sampling, sobol_profile
    _no_device(monkeypatch)
    d = sampling.Design(seed=1)
    for kw, match in ((dict(method='lhs'), "'mc' or 'sobol'"), (dict(norm='ln'), "'log10' or 'none'"), (dict(radius=0.0), 'radius'),
                      (dict(method='sobol', first_index=2 ** 30 - 99), '2\\^30 points'), (dict(first_index=-1), 'negative')):
        with pytest.raises(ValueError, match=match):
            sobol_profile.profile_sums(d, [2, 8], 100, **kw)
    with pytest.raises(ValueError, match='at most 15'):
        sobol_profile.profile_sums(d, list(range(15)) + [0], 100)
