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


# ---- the restatement with explicit tables, and the conditions tests/test_sobol_sweep_kernel.py rests on (no GPU) --------------------
def test_restatement_with_explicit_tables_is_the_default_one():
    """design / sweep given the study's own tables, and the default max_attempts, return what they return without them, bit for bit"""
    pb = study.DEFAULT_PRESSURES[[0, 4]]
    for g in study.GROUPS:
        t = study.prior_tables(pb, g)
        for row in (0, 1):
            x0, r0, u0 = ref.design(g, 400, 11, pb, 1, row, 133.3)
            x1, r1, u1 = ref.design(g, 400, 11, pb, 1, row, 133.3, tables=t, max_attempts=64)
            assert np.array_equal(x0, x1) and (r0, u0) == (r1, u1) and u0 == 0
    a = ref.sweep(300, 11, pb, 'Plume', 133.3)
    b = ref.sweep(300, 11, pb, 'Plume', 133.3, tables=study.prior_tables(pb, 'Plume'), max_attempts=64)
    for ra, rb in zip(a, b):
        assert ra['clip'] == rb['clip'] and ra['rejected'] == rb['rejected'] and ra['unaccepted'] == rb['unaccepted'] == 0
        for k in ('S1', 'ST', 'S1_se', 'ST_se'):
            assert np.array_equal(ra['jion'][k], rb['jion'][k])


def test_restated_rejection_loop_at_its_end():
    """max_attempts draws at most: a row never accepted keeps draw max_attempts - 1 and is counted; a pinned input is the pin"""
    import sobol_sweep_cases as sc
    from oracle import sampler_np
    t = sc.rough_plume_tables()
    p, row, n = 0, 0, sc.ROUGH_N
    draws = [sampler_np.sample(n, 0, 5, study.row_stream(2, 3, p, k, row), *(v[p] for v in t)) for k in range(3)]
    hit = [(ref.model('Plume', d, sc.torr())['profile'] >= sc.SPIKE).any(axis=1) for d in draws]
    x1, rej1, un1 = ref.design_rows('Plume', n, 5, None, p, row, sc.torr(), sc.SPIKE, 1, t)
    assert np.array_equal(x1, draws[0]) and np.array_equal(rej1, hit[0]) and np.array_equal(un1, hit[0]) and hit[0].sum() > 10
    x3, rej3, un3 = ref.design_rows('Plume', n, 5, None, p, row, sc.torr(), sc.SPIKE, 3, t)
    want = np.where(hit[0], np.where(hit[1], draws[2], draws[1]), draws[0])
    assert np.array_equal(x3, want)
    h01, h012 = hit[0] & hit[1], hit[0] & hit[1] & hit[2]
    assert np.array_equal(rej3, hit[0].astype(int) + h01 + h012) and np.array_equal(un3, h012)
    kind, a, b = (v.copy() for v in sc.rough_stage_tables('Thruster'))
    b[:, 3] = 90.0                                               # V_vac is pinned in the Thruster group: b is never read
    x, _, _ = ref.design_rows('Thruster', 50, 5, None, 1, 0, sc.torr(), tables=(kind, a, b))
    assert np.all(x[3] == a[1, 3]) and np.ptp(x[6]) > 0 and np.ptp(x[2]) > 0 and np.ptp(x[7]) > 0


def test_point_masses_reach_every_branch():
    """part 1: the Plume points hold enough valid off-axis maxima, literal-branch and invalid points, and no profile value lies
    within 1e-8 relative of a spike threshold in use; the Thruster points hold non-physical results"""
    import sobol_sweep_cases as sc
    pts = sc.points('Plume')
    assert np.isfinite(pts).all() and len(pts) >= 400
    ev = sc.evaluate('Plume', sc.designed('Plume', pts))
    off = sc.off_axis(ev)
    levels, members = sc.spike_levels(ev)
    assert int(off.sum()) >= 20 and int(ev['literal'].sum()) >= 50 and int(ev['invalid'].sum()) >= 20
    assert int((off & ev['literal']).sum()) == int(off.sum())                       # only the literal branch sees them
    placed = np.concatenate(members)
    assert len(set(placed)) == len(placed) >= 20 and len(levels) <= 20
    for thr, mem in zip(levels, members):
        prof = ev['profile'][mem]
        assert np.all(prof[:, 0] < thr) and np.all(prof.max(axis=1) > thr)         # j(0) alone would accept, the grid rejects
    for thr in levels + [sc.SPIKE]:
        assert sc.near(ev['profile'], thr) == 0, thr
    assert 10 <= int(sc.expect_rejected(ev, sc.SPIKE).sum()) <= len(pts) - 10
    th = sc.evaluate('Thruster', sc.designed('Thruster', sc.points('Thruster')))
    assert int(th['nonphys'].sum()) >= 5 and int(np.isnan(th['f'][0]).sum()) >= 3


@pytest.fixture(scope='module')
def rough():
    import sobol_sweep_cases as sc
    return {ma: sc.restate('Plume', sc.rough_plume_tables(), sc.ROUGH_N, sc.ROUGH_SEED, max_attempts=ma) for ma in (64, 2)}


def test_rough_plume_design_reaches_every_branch(rough):
    """parts 2 and 3: per pressure no non-finite value, more than 1000 literal, 300 invalid and 20 rejected evaluations, a row
    never accepted in two draws; the clip threshold has no value within its own bound of it, the first-order bound of the sums
    holds (its second-order remainder is below the 1 % it is given)"""
    import sobol_sweep_cases as sc
    for p, rec in enumerate(rough[64]):
        assert np.isfinite(rec['f']).all() and np.isfinite(rec['e']).all()
        assert int(rec['literal'].sum()) > 1000 and int(rec['invalid'].sum()) > 300 and int(rec['rejected'].sum()) > 20, p
        assert int(rec['unaccepted'].sum()) == 0
        thr = sc.choose_clip(rec['f'][:2])
        assert sc.near(rec['f'], thr) == 0 and np.all(np.abs(rec['f'] - thr) > rec['e'])
        assert 5 <= int((rec['f'][:2] > thr).sum()) <= 30
        for nb in (1, 3):
            want, bound, exact = sc.partial_sums(*sc.clipped(rec, thr), nb)
            assert np.isfinite(np.asarray(want, dtype=np.float64)).all() and np.all(exact <= bound)
    assert sum(int(rec['unaccepted'].sum()) for rec in rough[2]) >= 1
    assert all(np.isfinite(rec['f']).all() for rec in rough[2])


def test_wild_plume_design_holds_nan_and_no_inf():
    """the wild table: NaN j_ion among the accepted rows (and no infinite one: a partial a non-finite value enters is NaN), every
    finite value with a finite bound"""
    import sobol_sweep_cases as sc
    recs = sc.restate('Plume', sc.wild_plume_tables(), sc.ROUGH_N, sc.ROUGH_SEED)
    n_nan = 0
    for rec in recs:
        f = rec['f']
        assert not np.isinf(f).any() and np.array_equal(np.isfinite(f), np.isfinite(rec['e']))
        n_nan += int(np.isnan(f[:2]).sum())
        thr = sc.choose_clip(f[:2])
        fin = np.isfinite(f)
        assert np.all(np.abs(f[fin] - thr) > rec['e'][fin])
    assert n_nan >= 5


@pytest.mark.parametrize('group', ['Cathode', 'Thruster'])
def test_rough_stage_designs(group):
    """part 4: more than 20 non-physical Thruster evaluations per pressure, the first-order bound of the sums holds"""
    import sobol_sweep_cases as sc
    for rec in sc.restate(group, sc.rough_stage_tables(group), sc.STAGE_N, sc.STAGE_SEED):
        assert int(rec['nonphys'].sum()) > (20 if group == 'Thruster' else -1)
        assert np.isfinite(rec['f']).all() and np.isfinite(rec['e']).all()
        for nb in (1, 2):
            want, bound, exact = sc.partial_sums(rec['f'], rec['e'], nb)
            # (a bound of 0: a QoI that does not depend on the input, u_ion on mdot_a and a_1, T on a_1 -- every term is an exact 0)
            assert np.all((exact <= bound) | (bound == 0))
            assert np.all(want[bound == 0] == 0) and ((bound == 0).sum() > 0) == (group == 'Thruster')
