"""likelihood.SystemLikelihood on the host (no GPU): what it refuses, the order of its conditions (scripts/pem_v0/mcmc.py:36-45), its
record table, and the C ABI it binds (include/pem_hip.h)."""
import re
from pathlib import Path

import numpy as np
import pytest

from hallthrusterpem_amd import _lib
from hallthrusterpem_amd.likelihood import GRID_STEP, QOI_MAP, QOIS, UION_GRID, JionLikelihood, SystemLikelihood

ROOT = Path(__file__).resolve().parents[1]


def _x(rng, ne):
    return np.stack([10.0 ** rng.uniform(-6, -4.5, ne), rng.uniform(250, 350, ne), rng.uniform(4e-6, 6e-6, ne)], axis=1)


def _data(seed=0, na=12):
    rng = np.random.default_rng(seed)
    alpha = np.concatenate([[0.0, np.pi / 2, -0.3], rng.uniform(-np.pi / 2, np.pi / 2, na - 3)])
    return {
        'jion': {'x': _x(rng, 3), 'y': rng.lognormal(0, 1, (3, na)), 'var_y': rng.uniform(0.1, 2, (3, na)),
                 'loc': np.stack([np.ones(na), alpha], axis=1)},
        'T': {'x': _x(rng, 4), 'y': rng.uniform(0.05, 0.1, 4), 'var_y': rng.uniform(1e-5, 1e-4, 4)},
        'V_cc': {'x': _x(rng, 2), 'y': rng.uniform(15, 35, 2), 'var_y': rng.uniform(0.5, 4, 2)},
        'uion': {'x': _x(rng, 2), 'y': rng.uniform(1e3, 2e4, (2, 5)), 'var_y': np.ones((2, 5)),
                 'loc': np.array([0.0, 0.02, 0.04, 0.06, 0.08])},
    }


def test_conditions_follow_the_order_of_the_qois_and_the_records_restate_jion_likelihood():
    data = _data()
    del data['uion']                                   # (u_ion's interpolation pairs come from the device grid)
    lik = SystemLikelihood(data, device='cpu')
    assert lik.qois == ('V_cc', 'T', 'jion') and lik.component is None and lik.use_discharge
    assert np.array_equal(lik.operating, np.concatenate([data['V_cc']['x'], data['T']['x'], data['jion']['x']]))
    assert (lik.conditions['V_cc'], lik.conditions['T'], lik.conditions['jion']) == (slice(0, 2), slice(2, 6), slice(6, 9))
    span, rec = lik.span.numpy(), lik.rec.numpy()
    assert lik.n_cond == 9 and span.shape == (9, 4, 2)
    for c in range(9):
        kinds = np.nonzero(span[c, :, 1])[0]
        assert len(kinds) == 1                          # every condition measured one quantity
        kind = kinds[0]
        assert kind == (_lib.SYS_VCC if c < 2 else _lib.SYS_T if c < 6 else _lib.SYS_JION)
        first, count = span[c, kind]
        if c + 1 < 9:
            assert (span[c + 1].max(axis=0)[0] - first) % 2 == 1     # odd stride between conditions
    e = 1
    first, count = span[2 + e, _lib.SYS_T]
    assert count == 1 and rec[first, 1] == data['T']['y'][e] and rec[first, 2] == 1.0 / np.sqrt(data['T']['var_y'][e])
    # the j_ion records are JionLikelihood's (k, w, y, 1/std), bit for bit
    d = data['jion']
    ref = JionLikelihood(np.broadcast_to(d['loc'][:, 1], d['y'].shape), d['y'], np.sqrt(d['var_y']), device='cpu')
    for e in range(3):
        first, count = span[6 + e, _lib.SYS_JION]
        r = rec[first:first + count]
        assert count == 12
        assert np.array_equal(r[:, 0], ref.weight[e].numpy()) and np.array_equal(r[:, 1], ref.y[e].numpy())
        assert np.array_equal(r[:, 2], ref.inv_std[e].numpy())
        assert np.array_equal(r[:, 3].view(np.int64), ref.kidx[e].numpy().astype(np.int64))
    k0 = rec[span[6, _lib.SYS_JION, 0]: span[6, _lib.SYS_JION, 0] + 2, 3].view(np.int64)
    assert list(k0) == [0, 89] and rec[span[6, _lib.SYS_JION, 0] + 1, 0] == 1.0          # 0 and pi/2: first and last interval


def test_components_select_their_qois_and_cathode_drops_the_discharge_weight():
    data = _data()
    for comp, qois in QOI_MAP.items():
        if 'uion' in qois:
            continue
        lik = SystemLikelihood(data, qois=comp, device='cpu')
        assert lik.qois == tuple(qois) and lik.component == comp and lik.use_discharge == (comp != 'Cathode')
    lik = SystemLikelihood(data, qois=['jion', 'V_cc'], device='cpu')     # an explicit list keeps its order
    assert lik.qois == ('jion', 'V_cc') and lik.component is None
    assert np.array_equal(lik.operating[:3], data['jion']['x'])
    assert QOI_MAP['System'] == QOIS and UION_GRID == (0.0, 0.08, 200)


@pytest.mark.parametrize('case, match', [
    ('uion_outside', 'outside the u_ion grid'),
    ('uion_nan', 'outside the u_ion grid'),
    ('alpha_beyond', 'beyond 90 degrees'),
    ('radius', 'sweep_radius'),
    ('x_shape', "'x' must be"),
    ('y_shape', "'y' must have shape"),
    ('var_shape', "'var_y' must have shape"),
    ('unknown_qoi', 'unknown QoI'),
    ('unknown_component', 'unknown component'),
    ('missing', 'no dataset'),
    ('too_many_records', 'PEM_FUSED_SYSTEM_MAX_RECORDS = 1024'),
])
def test_host_refuses_what_the_kernel_cannot_compare(case, match):
    data = _data()
    kw = {}
    if case == 'uion_outside':
        data['uion']['loc'] = np.array([0.0, 0.02, 0.04, 0.06, 0.0800001])
    elif case == 'uion_nan':
        data['uion']['loc'] = np.array([0.0, np.nan, 0.04, 0.06, 0.08])
    elif case == 'alpha_beyond':
        data['jion']['loc'][4, 1] = np.pi / 2 + 1e-6
    elif case == 'radius':
        data['jion']['loc'][3, 0] = 1.5
    elif case == 'x_shape':
        data['T']['x'] = data['T']['x'][:, :2]
    elif case == 'y_shape':
        data['T']['y'] = data['T']['y'][:3]
    elif case == 'var_shape':
        data['jion']['var_y'] = data['jion']['var_y'][:, :5]
    elif case == 'unknown_qoi':
        data['I_D'] = data['T']
    elif case == 'unknown_component':
        kw['qois'] = 'Anode'
    elif case == 'missing':
        del data['V_cc']
        kw['qois'] = 'System'
    elif case == 'too_many_records':
        rng = np.random.default_rng(1)
        na = 341                                       # 3 x 341 + 2 + 4 + 2 x 5 (padded) > 1024
        data['jion'] = {'x': _x(rng, 3), 'y': np.ones((3, na)), 'var_y': np.ones((3, na)),
                        'loc': np.stack([np.ones(na), np.linspace(0, 1.5, na)], axis=1)}
    err = KeyError if case in ('unknown_qoi', 'unknown_component', 'missing') else ValueError
    with pytest.raises(err, match=match):
        SystemLikelihood(data, device='cpu', **kw)


def test_abi_constants_match_the_header():
    h = (ROOT / 'include' / 'pem_hip.h').read_text()
    define = lambda name: int(re.search(rf'#define {name} (\d+)', h).group(1))                          # noqa: E731
    assert define('PEM_FUSED_SYSTEM_MAX_RECORDS') == _lib.FUSED_SYSTEM_MAX_RECORDS
    assert [define(f'PEM_SYS_{k}') for k in ('JION', 'VCC', 'T', 'UION')] == [_lib.SYS_JION, _lib.SYS_VCC, _lib.SYS_T, _lib.SYS_UION]
    assert 'pem_coupled_system_loglik_f64_dev' in _lib.SIGNATURES
    assert GRID_STEP == (np.pi / 2) / 90.0
