"""The explicit Jacobian launch (`pem_coupled_jacobian_f64_dev` through `derivatives.jacobian`) on the GPU against the float64
restatement (tests/jacobian_np.py, itself held to a long-double reference by tests/test_jacobian_host.py).

Every entry is compared in the scaled units  err = |x_i| |J - J_want| / max(|f_q|, max_j |x_j J_want[q][j]|)  against
parity_rules.TOL = 1e-10 (where the scale is 0 -- V_cc clamped to 0, T_c with V_cc clamped to V_a -- the entry must be exactly 0),
the QoIs to TOL relative, the flags exactly.  Inputs: the prior set and the branch cases of jacobian_np.branch_cases (V_cc clamped
either way, a1 clipped, a beam below the tables).

Worst seen on an MI355X: scaled error 3.4e-12 and QoI 1.1e-12 relative, both div_angle of the branch case with a1 = 0.02, where
div_angle = 0.02 and acos turns one rounding of cos_div into 1 / div_angle^2 = 2500 of them; every other sample within 2.5e-14."""
import numpy as np
import pytest

import hp_model as hp
import jacobian_np as jn
from parity_rules import TOL

pytestmark = pytest.mark.gpu

NAMES = jn.NAMES
SHUFFLED = ['c1', 'V_vac', 'sigma_cex', 'P_b', 'a_1', 'c4', 'V_a', 'P_T', 'c2', 'T_e', 'c5', 'Pstar', 'c0', 'mdot_a', 'c3']
WRT = {'none': [], 'one': ['c3'], 'two': ['T_e', 'c2'], 'all-shuffled': SHUFFLED}
_cache = {}


def _k():
    from hallthrusterpem_amd import constants
    return constants.TORR_2_PA


def _inputs(n):
    """the first n - 5 samples of the prior set and the five branch cases (n = 1: one prior sample)"""
    if n not in _cache:
        pri = hp.prior_set(max(n, 6), seed=2)
        br, _ = jn.branch_cases()
        x = hp.take(pri, slice(0, 1)) if n < 6 else {q: np.concatenate([pri[q][:n - 5], br[q]]) for q in NAMES}
        _cache[n] = (x, jn.jacobian(x, _k()))
    return _cache[n]


def _hold(got, x, want, wrt):
    cols = [NAMES.index(w) for w in wrt]
    n = len(x['P_b'])
    J = got['jacobian']
    assert J.shape == (3, len(cols), n) and got['flags'].shape == (n,)
    f = np.stack([got[q] for q in jn.QOI])
    with np.errstate(all='ignore'):
        rel = np.abs(f - want['f']) / np.abs(want['f'])
    rel = np.where(f == want['f'], 0.0, rel)
    assert np.array_equal(np.isnan(f), np.isnan(want['f'])) and np.all(rel[~np.isnan(f)] <= TOL), np.nanmax(rel)
    assert np.array_equal(got['flags'].astype(np.int32), want['flags'])
    if not cols:
        return 0.0, float(np.nanmax(rel))
    # the scale takes every column of the restatement, the comparison the columns asked for
    with np.errstate(all='ignore'):
        scale = np.maximum(np.abs(want['f']), np.max(np.abs(want['x'][None] * want['jac']), axis=1))
        diff = np.abs(want['x'][None, cols, :]) * np.abs(J - want['jac'][:, cols, :])
        err = np.where(scale[:, None, :] == 0.0, np.where(J == 0.0, 0.0, np.inf), diff / scale[:, None, :])
    assert np.all(err <= TOL), (float(err.max()), np.argwhere(~(err <= TOL))[:5])
    return float(err.max()), float(np.nanmax(rel))


@pytest.mark.parametrize('wrt', list(WRT), ids=list(WRT))
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_the_launch_equals_the_restatement(n, wrt):
    from hallthrusterpem_amd import derivatives
    x, want = _inputs(n)
    err, rel = _hold(derivatives.jacobian(x, wrt=WRT[wrt]), x, want, WRT[wrt])
    print(f'n {n} wrt {wrt}: worst scaled error {err:.3g}, worst relative QoI error {rel:.3g}')


def test_the_default_is_every_input_in_order_and_tensors_stay_on_the_device():
    import torch
    from hallthrusterpem_amd import derivatives
    x, want = _inputs(65)
    host = derivatives.jacobian(x)
    assert isinstance(host['jacobian'], np.ndarray) and host['flags'].dtype == np.uint8
    _hold(host, x, want, list(NAMES))
    xt = {q: torch.from_numpy(v).cuda() for q, v in x.items()}
    dev = derivatives.jacobian(xt, wrt=SHUFFLED)
    assert all(v.is_cuda for v in dev.values()) and dev['jacobian'].dtype == torch.float64
    back = {q: v.cpu().numpy() for q, v in dev.items()}
    _hold(back, x, want, SHUFFLED)
    # the same numbers whichever way they came in, and whichever columns were asked for
    for j, name in enumerate(SHUFFLED):
        assert np.array_equal(back['jacobian'][:, j], host['jacobian'][:, NAMES.index(name)], equal_nan=True), name


def test_scalars_broadcast_and_the_loop_shape_is_kept():
    from hallthrusterpem_amd import derivatives
    x = dict(hp.BASE)
    x['c3'] = np.linspace(0.2, 1.5, 6).reshape(2, 3)
    got = derivatives.jacobian(x, wrt=['c3', 'c0'])
    assert got['V_cc'].shape == (2, 3) and got['jacobian'].shape == (3, 2, 2, 3) and got['flags'].shape == (2, 3)
    flat = {q: np.broadcast_to(np.asarray(v, dtype=np.float64), (2, 3)).reshape(-1) for q, v in x.items()}
    want = jn.jacobian(flat, _k())
    _hold({'V_cc': got['V_cc'].reshape(-1), 'div_angle': got['div_angle'].reshape(-1), 'T_c': got['T_c'].reshape(-1),
           'jacobian': got['jacobian'].reshape(3, 2, 6), 'flags': got['flags'].reshape(-1)}, flat, want, ['c3', 'c0'])


def test_the_branch_entries_are_exact_on_the_device():
    from hallthrusterpem_amd import derivatives
    x, rows = jn.branch_cases()
    J = derivatives.jacobian(x)['jacobian']
    col = NAMES.index
    assert not J[0, :, rows['V_zero']].any()
    assert all(J[2, col(k), rows['V_zero']] == 0.0 for k in ('T_e', 'V_vac', 'Pstar', 'P_T')) and J[2, col('V_a'), rows['V_zero']] > 0
    assert J[0, :, rows['V_at_Va']].tolist() == [1.0 if k == 'V_a' else 0.0 for k in NAMES] and not J[2, :, rows['V_at_Va']].any()
    assert all(J[1, col(k), rows['a1_clipped']] == 0.0 for k in ('P_b', 'c2', 'c3'))
    assert J[0, col('V_vac'), rows['plain']] == 1.0
    assert not J[:, col('a_1'), :].any() and not J[1][[col(k) for k in ('mdot_a', 'c4', 'c5', 'sigma_cex')]].any()


def test_refused_calls_launch_nothing():
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    from test_jacobian_host import BAD_JAC, launch_jacobian
    x = torch.ones((15, 10), dtype=torch.float64, device='cuda')
    out = {k: torch.full(s, -7.0, dtype=torch.float64, device='cuda') for k, s in (('qoi', (3, 10)), ('jac', (3, 2, 10)))}
    flags = torch.full((10,), 9, dtype=torch.uint8, device='cuda')
    ptrs = dict(x=C.c_void_p(x.data_ptr()), qoi=C.c_void_p(out['qoi'].data_ptr()), jac=C.c_void_p(out['jac'].data_ptr()),
                flags=C.c_void_p(flags.data_ptr()))
    for bad in BAD_JAC:
        assert launch_jacobian(**dict(ptrs, **bad)) == _lib.PEM_ERR_INVALID_ARG, bad
    torch.cuda.synchronize()
    assert bool((out['qoi'] == -7.0).all()) and bool((out['jac'] == -7.0).all()) and bool((flags == 9).all())
    assert launch_jacobian(**ptrs) == _lib.PEM_OK
    torch.cuda.synchronize()
    assert not bool((out['jac'] == -7.0).any()) and bool((flags < 4).all())
