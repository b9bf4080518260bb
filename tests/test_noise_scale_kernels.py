"""pem_loglik_marginal_scaled_f64_dev on the device, on synthetic per-sample sums: held to the long-double reference
(tests/hp_noise.py) under its bounds on the shapes and values of tests/noise_cases.py; at scale 1 it gives
pem_loglik_marginal_f64_dev's bits; two runs give the same bits."""
import ctypes as C

import numpy as np
import pytest

import noise_cases as nc

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _scaled(case, diagnostics=True, ld_chi=None):
    """(out, ess, chi) of a case on the device (ess, chi None without diagnostics); chi [K][G + 1] out of rows of ld_chi"""
    import torch
    from hallthrusterpem_amd import _lib
    K, M, E = case['ll'].shape
    G = len(case['group_end'])
    ll, md, a1, lp, theta = (_dev(case[k]) for k in ('ll', 'mdot_a', 'a_1', 'log_prior', 'theta'))
    out = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')
    ld_chi = G + 1 if ld_chi is None else ld_chi
    ess = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda') if diagnostics else None
    chi = torch.full((K, ld_chi), SENTINEL, dtype=torch.float64, device='cuda') if diagnostics else None
    ge, gc, sc = (np.ascontiguousarray(case[k], dtype=t) for k, t in (('group_end', np.int32), ('group_count', np.float64),
                                                                      ('scale_col', np.int32)))
    rc = _lib.load().pem_loglik_marginal_scaled_f64_dev(
        K, M, E, _p(ll), _p(md), _p(a1), *nc.DISCHARGE, _p(lp), G, C.c_void_p(ge.ctypes.data), C.c_void_p(gc.ctypes.data), _p(theta),
        case['d'], theta.stride(0) if theta is not None else 0, C.c_void_p(sc.ctypes.data), case['discharge_col'], _p(ess), _p(chi),
        ld_chi, _p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.load().pem_last_error()
    torch.cuda.synchronize()
    if not diagnostics:
        return out.cpu().numpy(), None, None
    chi = chi.cpu().numpy()
    assert np.all(chi[:, G + 1:] == SENTINEL), case['name']             # nothing written past the row's G + 1 entries
    return out.cpu().numpy(), ess.cpu().numpy(), chi[:, :G + 1]


def _unscaled(case):
    import torch
    from hallthrusterpem_amd import _lib
    K, M, E = case['ll'].shape
    ll, md, a1, lp = (_dev(case[k]) for k in ('ll', 'mdot_a', 'a_1', 'log_prior'))
    out = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')
    rc = _lib.load().pem_loglik_marginal_f64_dev(K, M, E, _p(ll), _p(md), _p(a1), *nc.DISCHARGE, _p(lp), _p(out),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('E, G', nc.COND_GROUPS)
def test_shapes_scales_and_discharge_against_the_long_double_reference(E, G):
    for i, case in enumerate(nc.shape_cases(E, G)):
        out, ess, chi = _scaled(case, ld_chi=G + 1 + 2 * (i % 2))
        nc.check(case, out, ess, chi)
        plain, _, _ = _scaled(case, diagnostics=False)
        assert plain.tobytes() == out.tobytes(), case['name']           # the diagnostics change nothing in out
        again, ess2, chi2 = _scaled(case, ld_chi=G + 1 + 2 * (i % 2))
        assert (again.tobytes(), ess2.tobytes(), chi2.tobytes()) == (out.tobytes(), ess.tobytes(), chi.tobytes()), case['name']


def test_non_finite_sums_and_bad_scales():
    for case, ninf, nan, void in nc.value_cases():
        out, ess, chi = _scaled(case)
        nc.check(case, out, ess, chi)
        assert np.all(out[ninf] == -np.inf) and np.all(np.isnan(out[nan])), case['name']
        assert np.all(np.isnan(ess[void])) and np.all(np.isnan(chi[void])), case['name']
        plain, _, _ = _scaled(case, diagnostics=False)
        assert np.array_equal(plain, out, equal_nan=True), case['name']


@pytest.mark.parametrize('E, G', nc.COND_GROUPS)
def test_at_scale_one_the_bits_are_the_unscaled_entry_points(E, G):
    """the contract: every column -1, or every column reading 1.0, gives pem_loglik_marginal_f64_dev's out bit for bit, with and
    without the diagnostics"""
    for case in nc.shape_cases(E, G):
        want = _unscaled(case)
        assert np.all(want != SENTINEL)
        for through_theta in (False, True):
            one = nc.at_scale_one(case, through_theta)
            for diagnostics in (False, True):
                got, _, _ = _scaled(one, diagnostics=diagnostics)
                assert got.tobytes() == want.tobytes(), (case['name'], through_theta, diagnostics, got, want)


def test_at_scale_one_non_finite_results_are_the_unscaled_entry_points():
    for case, _, _, _ in nc.value_cases():
        want = _unscaled(case)
        for through_theta in (False, True):
            got, _, _ = _scaled(nc.at_scale_one(case, through_theta), diagnostics=False)
            assert got.tobytes() == want.tobytes(), (case['name'], through_theta, got, want)
