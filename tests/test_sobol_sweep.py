"""drivers.sobol_sweep / pem_sobol_sweep_f64_dev on the GPU: held to the numpy restatement (sampler_np design with the rejection
streams, the CPU oracle as the model), to the already validated sobol_indices launch, to the structure of the model, and run at
full size (N = 1e6 per pressure, five pressures, all four QoIs)."""
import numpy as np
import pytest

import sobol_sweep_np as ref

pytestmark = pytest.mark.gpu

N, SEED = 20_000, 11


@pytest.fixture(scope='module')
def sweep():
    from hallthrusterpem_amd import drivers
    return drivers.sobol_sweep(N, seed=SEED)


@pytest.fixture(scope='module')
def restated():
    from hallthrusterpem_amd import constants
    from hallthrusterpem_amd import sobol as study
    from hallthrusterpem_amd.likelihood import UION_GRID
    c, _ = study.uion_node(study.L_CH, UION_GRID)
    pb = study.DEFAULT_PRESSURES
    return {g: ref.sweep(N, SEED, pb, g, constants.TORR_2_PA, uion=(*UION_GRID, c)) for g in study.GROUPS}


def _np(t):
    return t.cpu().numpy()


def _close(got, want, rec, atol, what):
    """|got - want| <= atol + 64 eps (1 + mean^2 / Var) |want|: Var = E f^2 - mean^2 is formed from sums that a QoI with little
    variance around a large mean (u_ion at the lowest pressures: mean^2 / Var ~ 1e8) cancels, and the kernel and numpy add those
    sums in different orders; every index and standard error divides by Var."""
    cond = 1.0 + rec['mean'] ** 2 / rec['var']
    tol = atol + 64 * np.finfo(np.float64).eps * cond * np.abs(want)
    assert np.all(np.abs(got - want) <= tol), (what, got, want, tol)


@pytest.mark.parametrize('qoi, group', [('V_cc', 'Cathode'), ('T', 'Thruster'), ('uion', 'Thruster'), ('jion', 'Plume')])
def test_against_the_restatement(sweep, restated, qoi, group):
    got = sweep[qoi]
    for p, rec in enumerate(restated[group]):
        want = rec[qoi]
        for k in ('S1', 'ST', 'S1_se', 'ST_se'):
            _close(_np(got[k][p]), want[k], want, 2e-9, f'{qoi} {k} p={p}')


def test_rejections_and_clip_against_the_restatement(sweep, restated):
    j = sweep['jion']
    want_rej = np.array([rec['rejected'] for rec in restated['Plume']])
    assert np.array_equal(j['rejected'], want_rej), (j['rejected'], want_rej)
    clip = _np(j['clip'])
    want = np.array([rec['clip'] for rec in restated['Plume']])
    np.testing.assert_allclose(clip, want, rtol=1e-13, atol=0)
    # bit-equal to numpy's percentile of the very values the pre-pass wrote
    j0 = _np(j['j0'])
    assert j0.shape == (5, 2 * N)
    assert np.array_equal(clip, np.percentile(j0, 99.0, axis=1))
    assert sweep['P_b'].shape == (5,) and sweep['evaluations'] == N * 5 * (7 + 6 + 10)
    assert sweep['non_physical'] == 0


def test_cathode_group_equals_sobol_indices(sweep):
    from hallthrusterpem_amd import drivers
    from hallthrusterpem_amd import sobol as study
    pri = study.sweep_priors(study.DEFAULT_PRESSURES[0], 'Cathode')
    fixed = {k: study.PEM_V0_NOMINAL[k] for k in study.PEM_V0_NOMINAL if k not in study.GROUP_INPUTS['Cathode']}
    old = drivers.sobol_indices(N, seed=SEED, priors=pri, fixed=fixed, qois=('V_cc',))
    assert old['inputs'] == list(study.GROUP_INPUTS['Cathode'])
    for k in ('S1', 'ST'):
        np.testing.assert_allclose(_np(sweep['V_cc'][k][0]), _np(old[k]['V_cc']), rtol=0, atol=1e-12)


def test_structure_of_the_model(sweep, restated):
    T, u = sweep['T'], sweep['uion']
    names = T['inputs']
    assert names == ('P_b', 'mdot_a', 'T_e', 'a_1')
    a1, md = names.index('a_1'), names.index('mdot_a')
    # the test double's thrust does not depend on a_1; u_ion = v_exh / const depends on neither mdot_a nor a_1
    assert np.all(_np(T['ST'][:, a1]) == 0.0)
    assert np.all(_np(u['ST'][:, md]) == 0.0) and np.all(_np(u['ST'][:, a1]) == 0.0)
    for p, rec in enumerate(restated['Thruster']):
        for k in ('S1', 'ST', 'S1_se', 'ST_se'):
            _close(_np(u[k][p]), rec['v_exh'][k], rec['v_exh'], 1e-12, f'uion / v_exh {k} p={p}')
    v = sweep['V_cc']
    st = _np(v['ST'])
    assert np.all(np.argmax(st, axis=1) == list(v['inputs']).index('V_vac'))


def test_full_size():
    import time

    import torch

    from hallthrusterpem_amd import drivers
    n = 1_000_000
    drivers.sobol_sweep(4096, seed=1)                      # warm-up: library, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = drivers.sobol_sweep(n, seed=1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert res['evaluations'] == n * 5 * 23 == 115_000_000
    assert res['non_physical'] == 0
    for q in ('V_cc', 'T', 'uion', 'jion'):
        r = {k: _np(res[q][k]) for k in ('S1', 'ST', 'S1_se', 'ST_se')}
        for k, v in r.items():
            assert np.all(np.isfinite(v)), (q, k)
        assert np.all(r['ST'] >= 0), q
        assert np.all(r['S1'] <= r['ST'] + 4 * np.maximum(r['S1_se'], r['ST_se'])), q
    print(f'sobol_sweep N = {n} x 5 pressures x 4 QoIs: {dt * 1e3:.2f} ms, {res["evaluations"] / dt:.3g} evaluations/s, '
          f'rejected {res["jion"]["rejected"].tolist()}, clip {_np(res["jion"]["clip"]).tolist()}')
