"""The model's Jacobian and the derivative-based measures without a GPU: the float64 restatement (tests/jacobian_np.py) is held to a
long-double reference by differences and to its branch rules exactly; `derivatives.measures` is held to closed forms on a linear
function; the entry points are declared, bound, built and exported and refuse malformed calls before they look for a device.

The reference is the Richardson extrapolation (4 D(h/2) - D(h)) / 3 of central differences of `hp_model.reference` (the model as the
exact function of its inputs, in long double) at the relative steps 2^-12 and 2^-13, over the doubles actually passed.  The error is
taken in the scaled units  err = |x_i| |J - J_ref| / max(|f_q|, max_j |x_j J_ref[q][j]|)  and held to parity_rules.TOL = 1e-10.
Measured on `hp_model.prior_set(3000, seed=2)`: V_cc 3.1e-15 (P_b), div_angle 1.2e-13 (c0), T_c 8.3e-15 (c3), with 17 of the 3000 samples
left out as near a clip -- the reference's own noise is 4e-13 (its step pairs (2^-12, 2^-13) and (2^-14, 2^-15) compared)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import hp_model as hp
import jacobian_np as jn
from parity_rules import TOL

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = {'pem_coupled_jacobian_f64_dev': 10, 'pem_gradient_sums_f64_dev': 16, 'pem_gradient_sums_qmc_f64_dev': 17}
FAKE = C.c_void_p(4096)                        # a device pointer that is never dereferenced: every check runs on the host
NAMES = jn.NAMES


def _k():
    from hallthrusterpem_amd import constants
    return constants.TORR_2_PA


# ---- the restatement against the reference ----------------------------------------------------------------------------------------
def test_the_restatement_equals_the_long_double_reference_on_the_prior_set():
    x = hp.prior_set(3000, seed=2)
    res = jn.jacobian(x, _k())
    near = jn.near_clip(res, x)
    print('near a clip:', int(near.sum()), 'of', near.size, '; smallest a1', float(res['a1_un'].min()))
    assert near.mean() <= 0.02
    J_ref, f_ref = jn.reference_jacobian(x, _k())
    keep = ~near
    err = jn.scaled_error(res['x'][:, keep], f_ref[:, keep], res['jac'][:, :, keep], J_ref[:, :, keep])
    for q, name in enumerate(jn.QOI):
        i, _ = np.unravel_index(np.argmax(err[q]), err[q].shape)
        print(f'{name}: worst scaled error {err[q].max():.3g} (with respect to {NAMES[i]})')
    assert np.all(err <= TOL), err.max()
    rel = np.abs(res['f'][:, keep] - f_ref[:, keep]) / np.abs(f_ref[:, keep])
    assert np.all(rel <= TOL), rel.max()
    assert not res['flags'].any()


# ---- the branch rules, exactly ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def branches():
    x, rows = jn.branch_cases()
    return jn.jacobian(x, _k()), rows


def _col(name):
    return NAMES.index(name)


def test_V_cc_clamped_to_zero_has_a_zero_row_and_T_c_sees_the_cathode_through_V_a_only(branches):
    res, rows = branches
    s = rows['V_zero']
    assert res['f'][0, s] == 0.0 and res['V_un'][s] < 0.0
    assert not res['jac'][0, :, s].any()
    for name in ('T_e', 'V_vac', 'Pstar', 'P_T'):
        assert res['jac'][2, _col(name), s] == 0.0, name
    assert res['jac'][2, _col('V_a'), s] > 0.0
    # P_b still reaches T_c through the plume, and only through it: T dcos / dP_b
    T = res['f'][2, s] / np.cos(res['f'][1, s])
    want = -np.sin(res['f'][1, s]) * res['jac'][1, _col('P_b'), s] * T
    assert abs(res['jac'][2, _col('P_b'), s] - want) <= 1e-12 * abs(want)


def test_V_cc_clamped_to_V_a_follows_V_a(branches):
    res, rows = branches
    s = rows['V_at_Va']
    assert res['f'][0, s] == 300.0
    assert res['jac'][0, :, s].tolist() == [1.0 if n == 'V_a' else 0.0 for n in NAMES]
    assert res['f'][2, s] == 0.0 and not res['jac'][2, :, s].any()             # T = 0 on the whole branch


def test_a1_clipped_has_no_derivative(branches):
    res, rows = branches
    s = rows['a1_clipped']
    assert res['a1_un'][s] > hp.HALF_PI
    for name in ('P_b', 'c2', 'c3'):
        assert res['jac'][1, _col(name), s] == 0.0, name
    assert res['jac'][1, _col('c0'), s] != 0.0 and res['jac'][1, _col('c1'), s] != 0.0


def test_the_structural_entries(branches):
    res, rows = branches
    x = hp.prior_set(500, seed=2)
    pri = jn.jacobian(x, _k())
    for r in (res, pri):
        assert not r['jac'][:, _col('a_1'), :].any()
        for name in ('mdot_a', 'c4', 'c5', 'sigma_cex'):
            assert not r['jac'][1, _col(name), :].any(), name
    free = (pri['V_un'] > 0) & (pri['V_un'] < x['V_a'])
    assert free.sum() > 400 and np.all(pri['jac'][0, _col('V_vac'), free] == 1.0)
    got, want = x['mdot_a'] * pri['jac'][2, _col('mdot_a')], pri['f'][2]
    assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want)))


def test_the_literal_branch_is_differentiated_too(branches):
    """a beam below the tables' range (a1 = 0.02): the same expressions, held to differences of the reference"""
    res, rows = branches
    x, _ = jn.branch_cases()
    s = [rows['literal'], rows['plain']]
    xs = hp.take(x, s)
    J_ref, f_ref = jn.reference_jacobian(xs, _k())
    err = jn.scaled_error(res['x'][:, s], f_ref, res['jac'][:, :, s], J_ref)
    print('literal / plain worst scaled error', err[:, :, 0].max(), err[:, :, 1].max())
    assert np.all(err <= TOL)


def test_the_selection_of_columns():
    x = hp.prior_set(10, seed=2)
    full = jn.jacobian(x, _k())['jac']
    pick = jn.jacobian(x, _k(), wrt=['c3', 'P_b'])['jac']
    assert pick.shape == (3, 2, 10) and np.array_equal(pick[:, 0], full[:, _col('c3')]) and np.array_equal(pick[:, 1], full[:, 0])
    assert jn.jacobian(x, _k(), wrt=[])['jac'].shape == (3, 0, 10)


# ---- the measures -----------------------------------------------------------------------------------------------------------------
def _linear_sums(coef, N):
    """sums of f = sum a_i z_i about its mean: every sample has the gradient a"""
    d = len(coef)
    rows = [np.zeros(3), None] + [np.full(3, N * c) for c in coef] + [np.full(3, N * c ** 4) for c in coef]
    rows += [np.full(3, N * coef[i] * coef[j]) for i in range(d) for j in range(i, d)]
    return rows


@pytest.mark.parametrize('kind', [jn.UNIFORM, jn.LOGUNIFORM, jn.NORMAL])
def test_measures_of_a_linear_function(kind):
    import torch
    from hallthrusterpem_amd import derivatives
    coef = np.array([2.0, -0.5, 0.0, 3.0])
    a, b = np.array([0.0, -1.0, 2.0, 1.0]), np.array([1.0, 3.0, 5.0, 1.5])
    var_z = b * b if kind == jn.NORMAL else (b - a) ** 2 / 12.0
    var = float((coef ** 2 * var_z).sum())
    N = 1000
    rows = _linear_sums(coef, N)
    rows[1] = np.full(3, N * var)
    sums = np.array(rows)
    assert sums.shape == (derivatives.n_rows(4), 3) == (jn.n_rows(4), 3)
    got = derivatives.measures(torch.from_numpy(sums), N, [kind] * 4, a, b)
    want = jn.measures(sums, N, [kind] * 4, a, b)
    for key, w in want.items():
        if key == 'eigenvectors':
            continue                                                    # (a degenerate eigenspace: any basis)
        assert np.allclose(got[key].numpy(), w, rtol=1e-12, atol=1e-12), key
    ST = coef ** 2 * var_z / var
    for q in range(3):
        assert np.allclose(got['nu'][q].numpy(), coef ** 2, rtol=1e-14) and not got['nu_se'][q].numpy().any()
        assert np.allclose(got['mean_gradient'][q].numpy(), coef, rtol=1e-14)
        ratio = got['bound_ST'][q].numpy()[ST > 0] / ST[ST > 0]
        assert np.allclose(ratio, 1.0 if kind == jn.NORMAL else 12.0 / np.pi ** 2, rtol=1e-13)
        s = b if kind == jn.NORMAL else (b - a) / 2.0
        lam = got['eigenvalues'][q].numpy()
        assert np.isclose(lam[0], ((s * coef) ** 2).sum(), rtol=1e-13) and np.all(np.abs(lam[1:]) <= 1e-13 * lam[0])
        w1 = got['eigenvectors'][q].numpy()[:, 0]
        assert np.allclose(np.abs(w1), np.abs(s * coef) / np.linalg.norm(s * coef), atol=1e-13)
        assert np.allclose(got['activity'][q].numpy(), (s * coef) ** 2, atol=1e-12)
    with pytest.raises(ValueError, match='take sums of shape'):
        derivatives.measures(torch.from_numpy(sums[:-1]), N, [kind] * 4, a, b)


def test_the_restated_sums_put_every_term_in_its_row():
    rng = np.random.default_rng(3)
    f, g, c = rng.normal(size=(3, 50)), rng.normal(size=(3, 3, 50)), np.array([0.1, -0.2, 0.3])
    g[1, 2, 7] = np.nan
    s, mag, form, skipped = jn.sums_of(f, g, c)
    ok = np.arange(50) != 7
    assert skipped == 1 and s.shape == (jn.n_rows(3), 3) and form.shape == (jn.n_rows(3),)
    assert np.allclose(s[0].astype(float), (f[:, ok] - c[:, None]).sum(axis=1)) and np.allclose(s[1].astype(float), ((f[:, ok] - c[:, None]) ** 2).sum(axis=1))
    assert np.allclose(s[2 + 1].astype(float), g[:, 1, ok].sum(axis=1)) and np.allclose(s[2 + 3 + 2].astype(float), (g[:, 2, ok] ** 4).sum(axis=1))
    assert np.allclose(s[2 + 6 + 4].astype(float), (g[:, 1, ok] * g[:, 2, ok]).sum(axis=1))          # pairs: 00 01 02 11 12 22
    assert np.all(mag >= np.abs(s))


# ---- the entry points -------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    for name, n_args in ENTRY_POINTS.items():
        mm = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header)
        assert mm and len(mm.group(1).split(',')) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(_lib.load(), name)
        assert name in (ROOT / 'INTEGRATION.md').read_text(), name
    assert build.PKG / 'csrc' / 'pem_jacobian.hip' in build.SRCS
    assert (build.PKG / 'csrc' / 'pem_jacobian.h').exists()


def _host(values, dtype):
    return None if values is None else np.ascontiguousarray(values, dtype=dtype)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def launch_sums(entry='f64', n=10, first=0, kind=(0,) * 15, a=(0.0,) * 15, b=(1.0,) * 15, n_varied=2, varied=(2, 8), centre=None, radius=1.0,
                partial=FAKE, flags=FAKE, n_blocks=4):
    from hallthrusterpem_amd import _lib
    kind, a, b, varied = _host(kind, np.int32), _host(a, np.float64), _host(b, np.float64), _host(varied, np.int32)
    fn = getattr(_lib.load(), f'pem_gradient_sums_{entry}_dev')
    head = (n, first, 12345, 3) + ((1,) if entry.startswith('qmc') else ())
    return fn(*head, _ptr(kind), _ptr(a), _ptr(b), n_varied, _ptr(varied), centre, 133.3, radius, partial, flags, n_blocks, None)


def launch_jacobian(n=10, x=FAKE, n_varied=2, varied=(2, 8), radius=1.0, qoi=FAKE, jac=FAKE, flags=FAKE):
    from hallthrusterpem_amd import _lib
    varied = _host(varied, np.int32)
    return _lib.load().pem_coupled_jacobian_f64_dev(n, x, n_varied, _ptr(varied), 133.3, radius, qoi, jac, flags, None)


BAD = [dict(n_varied=-1), dict(n_varied=16), dict(varied=(2, 15)), dict(varied=(-1, 3)), dict(n_blocks=0), dict(n_blocks=-3), dict(radius=0.0),
       dict(radius=-1.0), dict(radius=float('nan')), dict(partial=None), dict(flags=None), dict(kind=None), dict(a=None), dict(b=None),
       dict(varied=None), dict(partial=None, n=0), dict(kind=(3,) + (0,) * 14)]
BAD_QMC = [dict(first=2 ** 30 - 9), dict(first=2 ** 30 + 1), dict(n=0, first=2 ** 30 + 1), dict(n=2 ** 30 + 1)]
CASES = [(e, bad) for e in ('f64', 'qmc_f64') for bad in BAD + (BAD_QMC if e.startswith('qmc') else [])]
BAD_JAC = [dict(n_varied=-1), dict(n_varied=16), dict(varied=(2, 15)), dict(varied=None), dict(radius=0.0), dict(radius=float('nan')),
           dict(x=None), dict(qoi=None), dict(jac=None), dict(flags=None)]


@pytest.mark.parametrize('entry, bad', CASES, ids=[f'{e}-' + '-'.join(f'{k}={v}' for k, v in bad.items()) for e, bad in CASES])
def test_malformed_sums_calls_are_refused_without_a_device(entry, bad):
    from hallthrusterpem_amd import _lib
    assert launch_sums(entry, **bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert f'pem_gradient_sums_{entry}'.encode() in _lib.load().pem_last_error()


@pytest.mark.parametrize('bad', BAD_JAC, ids=['-'.join(f'{k}={v}' for k, v in bad.items()) for bad in BAD_JAC])
def test_malformed_jacobian_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert launch_jacobian(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_coupled_jacobian_f64' in _lib.load().pem_last_error()


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    import torch
    from hallthrusterpem_amd import _lib
    for name in ('current_device', 'current_stream'):
        monkeypatch.setattr(torch.cuda, name, lambda *a, **k: pytest.fail('touched a device'))
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('loaded the library'))


def test_jacobian_refuses_bad_arguments_before_touching_a_device(monkeypatch):
    from hallthrusterpem_amd import derivatives
    _no_device(monkeypatch)
    x = dict(hp.BASE)
    with pytest.raises(ValueError, match="'c9' is not an input"):
        derivatives.jacobian(x, wrt=['c0', 'c9'])
    with pytest.raises(ValueError, match='names an input twice'):
        derivatives.jacobian(x, wrt=['c0', 'P_b', 'c0'])
    with pytest.raises(ValueError, match='radius must be positive'):
        derivatives.jacobian(x, radius=0.0)
    with pytest.raises(ValueError, match='missing inputs'):
        derivatives.jacobian({k: v for k, v in x.items() if k != 'c4'})


def test_gradient_sums_refuses_bad_arguments_before_touching_a_device(monkeypatch):
    from hallthrusterpem_amd import derivatives, sampling
    _no_device(monkeypatch)
    d = sampling.Design(seed=1)
    for kw, match in ((dict(method='lhs'), "'mc' or 'sobol'"), (dict(radius=0.0), 'radius'), (dict(first_index=-1), 'negative'),
                      (dict(method='sobol', first_index=2 ** 30 - 99), '2\\^30 points')):
        with pytest.raises(ValueError, match=match):
            derivatives.gradient_sums(d, [2, 8], 100, **kw)
    with pytest.raises(ValueError, match='at most 15'):
        derivatives.gradient_sums(d, list(range(15)) + [0], 100)
    with pytest.raises(ValueError, match='indices 0..14'):
        derivatives.gradient_sums(d, [3, 15], 100)
    with pytest.raises(ValueError, match='negative'):
        derivatives.gradient_sums(d, [3], -1)


@pytest.mark.parametrize('kw, match', [(dict(design='lhs'), "'mc' or 'sobol'"), (dict(n=0), 'at least 1'), (dict(qois=('thrust',)), 'scalar QoIs'),
                                       (dict(design='sobol', n=2 ** 30 + 1), '2\\^30 points')])
def test_derivative_sensitivity_refuses_what_it_cannot_run_before_touching_a_device(kw, match, monkeypatch):
    from hallthrusterpem_amd import drivers
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        drivers.derivative_sensitivity(**dict(dict(n=100), **kw))
