"""The Sobol' study over a pressure sweep, host side (no GPU): the nominal table, the per-pressure prior tables, the estimators and
standard errors of the numpy restatement on a model with known indices, the kernel's resources and the driver's argument checks."""
import json
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import sobol_sweep_np as ref
from hallthrusterpem_amd import drivers, sampling
from hallthrusterpem_amd import sobol as study
from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS

ROOT = Path(__file__).resolve().parents[1]
TABLE = json.loads((ROOT / 'tests' / 'golden' / 'pem_v0_variables.json').read_text())


def test_nominal_values_are_the_yaml_ones():
    nominal = {v['name']: float(v['nominal']) for c in TABLE['components'] for v in c['inputs'] if 'nominal' in v}
    assert tuple(study.PEM_V0_NOMINAL) == COUPLED_INPUTS
    for k in COUPLED_INPUTS:
        assert study.PEM_V0_NOMINAL[k] == nominal[k], k


def test_groups_vary_the_components_exogenous_inputs():
    comps = {c['name']: [v['name'] for v in c['inputs']] for c in TABLE['components']}
    for g, names in study.GROUP_INPUTS.items():
        # every varied input is an input of that component in the YAML, none is a constant or a coupling variable
        assert set(names) <= set(comps[g]) and 'V_a' not in names and not set(names) & {'V_cc', 'I_B0'}
    # the YAML inputs of each component that the 15-input model has, V_a held constant
    for g in study.GROUPS:
        want = [k for k in comps[g] if k in COUPLED_INPUTS and k != 'V_a']
        assert list(study.GROUP_INPUTS[g]) == want, g


@pytest.mark.parametrize('group', study.GROUPS)
def test_prior_tables_of_the_default_sweep(group):
    pb = study.DEFAULT_PRESSURES
    assert np.array_equal(pb, 10 ** np.linspace(-6, -4, 5)) and pb[-1] == 1e-4
    kind, a, b = study.prior_tables(pb, group)
    assert kind.shape == a.shape == b.shape == (5, 15) and kind.dtype == np.int32
    varied = study.GROUP_INPUTS[group]
    for p, pres in enumerate(pb):
        for d, k in enumerate(COUPLED_INPUTS):
            if k not in varied:                               # pinned at the nominal value
                assert (kind[p, d], a[p, d], b[p, d]) == (sampling.UNIFORM, study.PEM_V0_NOMINAL[k], study.PEM_V0_NOMINAL[k]), k
            elif k == 'P_b':                                  # Relative(20) around the pressure, inside (1e-8, 1e-4)
                assert kind[p, d] == sampling.UNIFORM
                assert a[p, d] == pres * (1 - 20 / 100)
                assert b[p, d] == (1e-4 if p == 4 else pres * (1 + 20 / 100))
                assert 1e-8 <= a[p, d] < b[p, d] <= 1e-4
            elif k == 'mdot_a':                               # Relative(3) around 5e-6
                assert (kind[p, d], a[p, d], b[p, d]) == (sampling.UNIFORM, 5e-6 * (1 - 3 / 100), 5e-6 * (1 + 3 / 100))
            else:
                pr = sampling.PEM_V0_PRIORS[k]
                assert (kind[p, d], a[p, d], b[p, d]) == (pr.kind, pr.a, pr.b), k
    assert b[4, 0] == 1e-4 and b[3, 0] < 1e-4          # the 1e-4 Torr edge is clipped to the domain, the others are not


def test_stream_numbering():
    # the Cathode group at pressure 0 uses streams 0 and 1: the design of sobol_indices(seed) with the same table
    assert study.row_stream(0, 5, 0, 0, 0) == 0 and study.row_stream(0, 5, 0, 0, 1) == 1
    seen = {study.row_stream(g, 5, p, k, r) for g in range(3) for p in range(5) for k in range(64) for r in range(2)}
    assert len(seen) == 3 * 5 * 64 * 2 and min(seen) == 0 and max(seen) == 2 * 3 * 5 * 64 - 1


def test_uion_node_nearest_l_ch():
    c, z = study.uion_node(0.025, (0.0, 0.08, 200))
    grid = 0.0 + 0.08 * (np.arange(200) / 199.0)
    assert c == int(np.argmin(np.abs(grid - 0.025))) == 62 and z == grid[62]


def _additive(n, a, rng):
    x = rng.random((len(a), n))
    return x, a @ x


def _additive_estimates(n, a, seed):
    rng = np.random.default_rng(seed)
    xa, fa = _additive(n, a, rng)
    xb, fb = _additive(n, a, rng)
    fab = []
    for i in range(len(a)):
        x = xa.copy()
        x[i] = xb[i]
        fab.append(a @ x)
    return ref.estimates(fa, fb, np.stack(fab))


def test_restated_estimators_on_an_additive_model():
    # f = sum a_i x_i, x_i ~ U(0, 1): Var = sum a_i^2 / 12 and S1_i = ST_i = a_i^2 / sum a^2
    a = np.array([1.0, 2.0, 0.5, 3.0])
    exact = a ** 2 / np.sum(a ** 2)
    n = 40_000
    r = _additive_estimates(n, a, 7)
    for k in ('S1', 'ST'):
        se = r[k + '_se']
        assert np.all(se > 0)
        assert np.all(np.abs(r[k] - exact) <= 4 * se), (k, r[k], exact, se)
    r4 = _additive_estimates(4 * n, a, 8)
    for k in ('S1_se', 'ST_se'):
        ratio = r[k] / r4[k]
        assert np.all(np.abs(ratio - 2) <= 0.2), (k, ratio)


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_sweep_kernel_has_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_sobol_sweep.hip')],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    assert sorted(rows) == ['sobol_sweep_kernel<0>', 'sobol_sweep_kernel<1>', 'sobol_sweep_kernel<2>'], rows
    for name, r in rows.items():        # launched at two waves per SIMD: at most 256 registers
        assert r['vspill'] == 0 and r['scratch'] == 0 and r['vgpr'] <= 256, (name, r)


@pytest.mark.parametrize('kw, match', [
    (dict(qois=('V_cc', 'thrust')), 'unknown QoI'),
    (dict(qois=()), 'non-empty'),
    (dict(pressures=[]), 'non-empty'),
    (dict(pressures=[1e-5, 2e-4]), 'domain'),
    (dict(pressures=[1e-9]), 'domain'),
    (dict(pressures=[np.nan]), 'domain'),
    (dict(l_ch=0.09), 'outside the u_ion grid'),
    (dict(l_ch=-0.01), 'outside the u_ion grid'),
    (dict(clip_percentile=101.0), 'clip_percentile'),
])
def test_sobol_sweep_rejects_bad_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        drivers.sobol_sweep(100, **kw)


def test_sobol_sweep_rejects_an_empty_design():
    with pytest.raises(ValueError, match='n_base'):
        drivers.sobol_sweep(0)
