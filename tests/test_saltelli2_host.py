"""Second-order Sobol' indices without a GPU: the numpy restatement (tests/saltelli2_np.py) reproduces the figures the feature was
proposed with on the CPU oracle, behaves as the estimator must on functions with known indices, is invariant to its centre where
the algebra says so; the entry points are declared, bound, built and exported and refuse malformed calls before they look for a
device; the Python layer refuses what it cannot run before it touches one; and the default path never reaches the new code."""
import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import qmc_np
import saltelli2_np as s2
from oracle import sampler_np as snp

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {'pem_saltelli2_f32_dev': 16, 'pem_saltelli2_f64_dev': 16, 'pem_saltelli2_qmc_f32_dev': 17, 'pem_saltelli2_qmc_f64_dev': 17}
FAKE = C.c_void_p(4096)                        # a device pointer that is never dereferenced: every check runs on the host
SEED = (0x9E3779B9 << 32) | 0x7F4A7C15
FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6}
QOIS = ('V_cc', 'div_angle', 'T_c')
U01 = dict(kind=[0] * 15, a=[0.0] * 15, b=[1.0] * 15)


def _fixed_study(seed=11):
    from hallthrusterpem_amd import sampling
    pri = dict(sampling.PEM_V0_PRIORS)
    for k, v in FIXED.items():
        pri[k] = sampling.Prior(sampling.UNIFORM, v, v, 'fixed')
    design = sampling.Design(priors=pri, seed=seed)
    return design, [i for i, k in enumerate(design.names) if k not in FIXED]


# ---- 1. the figures of the proposal ---------------------------------------------------------------------------------------------
def test_the_restatement_reproduces_the_fixed_operating_point_study_at_4096_points_to_the_digits_printed():
    """Sobol' design, seed 11, P_b, V_a and mdot_a fixed, 12 varied inputs, the CPU oracle as the model, c = the mean over the same
    4096 points (the driver's pilot).  sum S1 = 0.9996 / 0.9126 / 0.9232, sum over pairs of S2 = 0.0023 / 0.0603 / 0.1109,
    max |S2| = 0.0003 / 0.0398 / 0.0275 (V_cc / div_angle / T_c), each to the four decimals given; the largest pair of div_angle is
    c1 x c3."""
    n = 4096
    d, varied = _fixed_study()
    A = qmc_np.sample(n, 0, d.seed, d.stream, d.kind, d.a, d.b)
    B = qmc_np.sample(n, 0, d.seed, d.stream, d.kind, d.a, d.b, swap_dim=-2)
    ev = s2.evaluate(qmc_np.oracle_qois, A, B, varied)
    centre = (ev[0] + ev[1]).sum(axis=1) / (2 * n)
    t, _, _ = s2.terms(*ev, centre, dtype=s2.LD)
    est = s2.indices(t.sum(axis=2).astype(np.float64), n, len(varied))
    iu = np.triu_indices(len(varied), 1)
    sum_s1, sum_s2 = est['S1'].sum(axis=0), est['S2'][:, iu[0], iu[1]].sum(axis=1)
    max_s2 = np.abs(est['S2']).max(axis=(1, 2))
    print('sum S1', sum_s1, 'sum S2', sum_s2, 'max |S2|', max_s2)
    half = 0.5e-4 * (1 + 1e-9)
    assert np.all(np.abs(sum_s1 - [0.9996, 0.9126, 0.9232]) <= half), sum_s1
    assert np.all(np.abs(sum_s2 - [0.0023, 0.0603, 0.1109]) <= half), sum_s2
    assert np.all(np.abs(max_s2 - [0.0003, 0.0398, 0.0275]) <= half), max_s2
    names = [d.names[v] for v in varied]
    i, j = np.unravel_index(np.argmax(np.abs(np.triu(est['S2'][1], 1))), est['S2'][1].shape)
    assert {names[i], names[j]} == {'c1', 'c3'}, (names[i], names[j])
    assert np.array_equal(est['S2'], est['S2'].transpose(0, 2, 1)) and np.all(est['S2'][:, np.arange(12), np.arange(12)] == 0)


# ---- 2. functions with known indices --------------------------------------------------------------------------------------------
WEIGHTS = np.array([3.0, 0.0, 1.0, 2.0, 0.5, 0.0, 1.5, 0.25, 4.0, 0.0, 1.0, 2.5, 0.75, 0.1, 1.25])


def _additive(x):
    f = (WEIGHTS[:, None] * x).sum(axis=0)
    return np.stack([f, 2.0 * f + 100.0, -0.5 * f - 3.0])                        # the indices do not see an affine map


def _blocks(n, design):
    if design == 'sobol':
        return qmc_np.sample(n, 0, SEED, 0, **U01), qmc_np.sample(n, 0, SEED, 0, swap_dim=-2, **U01)
    return snp.sample(n, 0, 7, 0, U01['kind'], U01['a'], U01['b']), snp.sample(n, 0, 7, 0, U01['kind'], U01['a'], U01['b'], swap_dim=-2)


@pytest.mark.parametrize('design', ['sobol', 'mc'])
def test_on_an_additive_function_every_second_order_index_is_within_twice_the_worst_first_order_error(design):
    """f = sum a_k x_k, x uniform: S1_k = a_k^2 / sum a^2 exactly and every S2 is 0.  The estimate of S2_ij is minus the sampling
    errors of S1_i and S1_j, so |S2_ij| <= 2 max |S1 - exact|."""
    n, varied = 4096, list(range(15))
    A, B = _blocks(n, design)
    centre = s2.pilot_centre(_additive, A, B)
    rows, _, _ = s2.sums(_additive, A, B, varied, centre, dtype=s2.LD)
    est = s2.indices(rows.astype(np.float64), n, 15)
    exact = WEIGHTS ** 2 / (WEIGHTS ** 2).sum()
    for q in range(3):
        worst = np.abs(est['S1'][:, q] - exact).max()
        print(design, q, 'max |S1 - exact|', worst, 'max |S2|', np.abs(est['S2'][q]).max())
        assert np.abs(est['S2'][q]).max() <= 2.0 * worst, (design, q)


def _product(x):
    f = x[0] * x[1] + x[2]
    # (an offset far above the spread would drown S1 -- whose products are not centred -- and with it S2, in noise)
    return np.stack([f, 2.0 * f + 1.0, -0.5 * f - 0.25])


@pytest.mark.parametrize('design', ['sobol', 'mc'])
def test_on_x0_x1_plus_x2_the_pair_index_converges_to_its_closed_form_and_the_others_to_zero(design):
    """x uniform on [0, 1]: Var = 7/144 + 1/12 = 19/144, V_0 = V_1 = 1/48, V_01 = 7/144 - 2/48 = 1/144, so S2_01 = 1/19 and every
    other pair is 0.  Held to 5 standard errors of the estimate, the standard error taken from the per-sample terms themselves
    (independent draws; the sequence does no worse), at two sizes, the second four times the first, where that bound is half as wide."""
    varied = [0, 1, 2, 5]
    want = np.zeros((4, 4))
    want[0, 1] = want[1, 0] = 1.0 / 19.0
    for n in (1 << 12, 1 << 14):
        A, B = _blocks(n, design)
        centre = s2.pilot_centre(_product, A[:, :min(n, 4096)], B[:, :min(n, 4096)])
        ev = s2.evaluate(_product, A, B, varied)
        t, _, _ = s2.terms(*ev, centre)
        est = s2.indices(t.sum(axis=2), n, 4)
        for q in range(3):
            var = est['var'][q]
            for p, (i, j) in enumerate(s2.pairs(4)):
                per_sample = (t[3 + 16 + p, q] - t[2 + 16, q] - t[2 + 2 * i, q] - t[2 + 2 * j, q]) / var
                se = per_sample.std(ddof=1) / np.sqrt(n)
                err = abs(est['S2'][q, i, j] - want[i, j])
                print(design, n, q, (i, j), 'S2', est['S2'][q, i, j], 'err', err, 'se', se)
                assert err <= 5.0 * se, (design, n, q, i, j)


# ---- 3. the centre --------------------------------------------------------------------------------------------------------------
def _poly(x):
    f = x[0] * x[1] + x[2] * x[2] * x[0] + 3 * x[1] - x[2]
    return np.stack([f, 2 * f + 100, -f * Fraction(1, 2) - 3])


def test_the_estimate_does_not_depend_on_the_centre_in_exact_arithmetic():
    """C_ij - D = sum (fBA_i fAB_j - fA fB) - c sum (fBA_i + fAB_j - fA - fB): the estimate moves with c by exactly that last sum,
    whose expectation is 0.  N = 8, integer inputs, fractions.Fraction throughout.
    (a) A = the 2^3 factorial of three inputs, B = M A over GF(2) with M unit upper triangular: every one of the 2 nv + 2 blocks is
        then the whole factorial in another order, every block has the same sum of f, and S2 is the same for every c -- exactly.
    (b) a design without that symmetry: S2(c) - S2(0) = -c sum (fBA_i + fAB_j - fA - fB) / (N Var), exactly."""
    varied, nv = [0, 1, 2], 3
    bits = np.array([[(n >> k) & 1 for n in range(8)] for k in range(3)])
    mixed = np.array([bits[0] ^ bits[1], bits[1] ^ bits[2], bits[2]])

    def design(cols):
        x = np.empty((15, 8), dtype=object)
        for d in range(15):
            x[d] = [Fraction(int(v)) for v in (1 + 2 * cols[d] if d < 3 else np.full(8, d))]
        return x
    centres = [(Fraction(0),) * 3, (Fraction(7, 3), Fraction(-100), Fraction(1, 7)), (Fraction(10 ** 6),) * 3]
    A, B = design(bits), design(mixed)
    ev = s2.evaluate(_poly, A, B, varied)
    ests = [s2.indices(s2.terms(*ev, c, dtype=object)[0].sum(axis=2), 8, nv)['S2'] for c in centres]
    assert all(isinstance(v, Fraction) for v in ests[0].ravel()[[1, 2, 5]]) and ests[0][0, 0, 1] != 0
    assert np.array_equal(ests[0], ests[1]) and np.array_equal(ests[0], ests[2])
    # (b)
    rng = np.random.default_rng(3)
    A, B = design(rng.integers(0, 5, size=(3, 8))), design(rng.integers(0, 5, size=(3, 8)))
    fA, fB, fAB, fBA = s2.evaluate(_poly, A, B, varied)
    base = s2.indices(s2.terms(fA, fB, fAB, fBA, centres[0], dtype=object)[0].sum(axis=2), 8, nv)
    moved = s2.indices(s2.terms(fA, fB, fAB, fBA, centres[1], dtype=object)[0].sum(axis=2), 8, nv)
    assert all(np.array_equal(base[k], moved[k]) for k in ('S1', 'ST', 'S1_mirror', 'ST_mirror', 'mean', 'var'))
    for q in range(3):
        for i, j in s2.pairs(nv):
            drift = (fBA[i, q] + fAB[j, q] - fA[q] - fB[q]).sum()
            assert drift != 0
            assert moved['S2'][q, i, j] - base['S2'][q, i, j] == -centres[1][q] * drift / (8 * base['var'][q])


# ---- 4. the entry points --------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    for name, n_args in ENTRY_POINTS.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header)
        assert m and len(m.group(1).split(',')) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_lib.load(), name)
        assert name in (ROOT / 'INTEGRATION.md').read_text(), name
    assert build.PKG / 'csrc' / 'pem_saltelli2.hip' in build.SRCS


def _host(values, dtype):
    return None if values is None else np.ascontiguousarray(values, dtype=dtype)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _launch(entry='f64', n_base=10, first=0, kind=(0,) * 15, a=(0.0,) * 15, b=(1.0,) * 15, n_varied=2, varied=(2, 8), centre=(0.0, 0.0, 0.0),
            partial=FAKE, flags=FAKE, n_blocks=4):
    from hallthrusterpem_amd import _lib
    kind, a, b, varied, centre = _host(kind, np.int32), _host(a, np.float64), _host(b, np.float64), _host(varied, np.int32), _host(centre, np.float64)
    fn = getattr(_lib.load(), f'pem_saltelli2_{entry}_dev')
    head = (n_base, first, SEED, 3) + ((1,) if entry.startswith('qmc') else ())
    return fn(*head, _ptr(kind), _ptr(a), _ptr(b), n_varied, _ptr(varied), _ptr(centre), 133.3, 1.0, partial, flags, n_blocks, None)


def _id(bad):
    return '-'.join(f'{k}={"tuple" if isinstance(v, tuple) and len(v) > 3 else v}' for k, v in bad.items())


BAD = [dict(kind=None), dict(a=None), dict(b=None), dict(varied=None), dict(centre=None), dict(partial=None), dict(flags=None), dict(n_varied=0),
       dict(n_varied=16), dict(n_blocks=0), dict(centre=None, n_base=0)]
BAD_QMC = [dict(first=2 ** 30 - 9), dict(first=2 ** 30 + 1), dict(n_base=0, first=2 ** 30 + 1), dict(first=2 ** 64 - 5)]


CASES = [(e, bad) for e in ('f32', 'f64', 'qmc_f32', 'qmc_f64') for bad in BAD + (BAD_QMC if e.startswith('qmc') else [])]


@pytest.mark.parametrize('entry, bad', CASES, ids=[f'{e}-{_id(bad)}' for e, bad in CASES])
def test_malformed_second_order_calls_are_refused_without_a_device(entry, bad):
    from hallthrusterpem_amd import _lib
    assert _launch(entry, **bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert f'pem_saltelli2_{entry}'.encode() in _lib.load().pem_last_error()


def test_bad_kinds_and_bad_varied_indices_are_refused_or_need_a_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    for entry in ENTRY_POINTS:
        e = entry[len('pem_saltelli2_'):-len('_dev')]
        assert _launch(e) == _lib.PEM_ERR_NO_DEVICE and _launch(e, n_varied=15, varied=tuple(range(15)), n_blocks=1) == _lib.PEM_ERR_NO_DEVICE
        assert _launch(e, n_varied=1, varied=(14,)) == _lib.PEM_ERR_NO_DEVICE


# ---- 5. the Python layer --------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    import torch
    from hallthrusterpem_amd import _lib
    for name in ('current_device', 'current_stream'):
        monkeypatch.setattr(torch.cuda, name, lambda *a, **k: pytest.fail('touched a device'))
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('loaded the library'))


@pytest.mark.parametrize('kw, match', [
    (dict(precision='fp32', fused=False), 'fused launch only'),
    (dict(design='lhs'), "'mc' or 'sobol'"),
    (dict(design='qmc'), "'mc' or 'sobol'"),
    (dict(design='sobol', n_base=2 ** 30 + 1), '2\\^30 points'),
])
def test_sobol_indices_refuses_what_it_cannot_run_before_touching_a_device(kw, match, monkeypatch):
    from hallthrusterpem_amd import drivers
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        drivers.sobol_indices(**dict(dict(n_base=100, second_order=True), **kw))


def test_saltelli2_sums_refuses_bad_designs_and_a_missing_centre_before_touching_a_device(monkeypatch):
    from hallthrusterpem_amd import fp32, sampling
    _no_device(monkeypatch)
    d = sampling.Design(seed=1)
    for method in ('lhs', 'qmc'):
        with pytest.raises(ValueError, match="'mc' or 'sobol'"):
            fp32.saltelli2_sums(d, [2, 8], 100, (0.0, 0.0, 0.0), method=method)
    with pytest.raises(ValueError, match='2\\^30 points'):
        fp32.saltelli2_sums(d, [2, 8], 2 ** 30 + 1, (0.0, 0.0, 0.0), method='sobol')
    with pytest.raises(ValueError, match='2\\^30 points'):
        fp32.saltelli2_sums(d, [2, 8], 100, (0.0, 0.0, 0.0), first_index=2 ** 30 - 99, method='sobol')
    for method in ('mc', 'sobol'):
        with pytest.raises(ValueError, match='centre'):
            fp32.saltelli2_sums(d, [2, 8], 100, None, method=method)
    with pytest.raises(ValueError, match='centre'):
        fp32.saltelli2_sums(d, [2, 8], 100, (0.0, 0.0))


def test_the_default_never_resolves_a_second_order_symbol(monkeypatch):
    """second_order=False with the launch itself replaced by a recording stand-in on the CPU device: the driver asks the first-order
    wrapper only, never `saltelli2_sums`, and never takes a `pem_saltelli2_*` attribute of the library."""
    import torch
    from hallthrusterpem_amd import _lib, drivers, fp32
    real = _lib.load()
    asked, calls = [], []

    class Spy:
        def __getattr__(self, name):
            asked.append(name)
            assert not name.startswith('pem_saltelli2'), name
            return getattr(real, name)

    def stand_in(design, varied, n_base, **kw):
        calls.append((len(varied), n_base, kw['method']))
        g = torch.Generator().manual_seed(1)
        sums = torch.rand((2 + 2 * len(varied), 3), dtype=torch.float64, generator=g) + 1.0
        sums[1] += 2.0 * n_base * 10.0
        return sums, torch.zeros(2, dtype=torch.int64)
    monkeypatch.setattr(_lib, 'load', lambda: Spy())
    monkeypatch.setattr(fp32, 'saltelli_sums', stand_in)
    monkeypatch.setattr(fp32, 'saltelli2_sums', lambda *a, **k: pytest.fail('the second-order launch was asked for'))
    for kw in (dict(), dict(second_order=False), dict(design='sobol', precision='fp32')):
        res = drivers.sobol_indices(1000, seed=3, fixed=FIXED, device='cpu', **kw)
        assert sorted(res) == sorted(['S1', 'ST', 'inputs', 'mean', 'var', 'evaluations', 'precision', 'fused', 'design', 'non_physical', 'invalid'])
        assert res['evaluations'] == 1000 * 14
    assert calls == [(12, 1000, 'mc'), (12, 1000, 'mc'), (12, 1000, 'sobol')]
    assert not [n for n in asked if 'saltelli2' in n]
