"""The Sobol' study through the chained surrogate on the GPU: pem_chain_sobol_sweep_f64_dev against the chained predict (bit for bit
on linear slots), against the restatement of tests/chain_sobol_np.py (log10 slots), its sums against the estimators applied to its
own f, and `drivers.sobol_sweep(surrogate=)` on a chain trained on the test double."""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu

N_EXT, VCC, IB0 = 5, 5, 6                     # test_chained_surrogate's synthetic chain: 5 external slots, then V_cc, I_B0
NCELLS, CELL = 7, 4
GROUP_ROWS = {'Cathode': (3, 0, 5, 2, 4),      # the input row every external slot reads: the group's varied inputs, shuffled
              'Thruster': (7, 0, 1, 6, 2)}     # P_b mdot_a T_e a_1 and V_a, which the group pins


def _p(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _hp(x):
    return x.ctypes.data_as(C.c_void_p)


def _chain(rng, outers, u_rank, big):
    """test_chain_uion._case's tables and coupling domains (its own points are not used)"""
    import test_chain_uion as tcu
    return tcu._case(rng, 1000, 2, outers, 0, u_rank, NCELLS, (VCC, IB0), big, pad=0)


def _np_chain(cs):
    import chain_sobol_np as csn
    return dict(stages=[csn.as_dicts(s) for s in cs['stages']], vcc_slot=VCC, ib0_slot=IB0, vmap=cs['vmap'])


def _launch(cs, group, n, tabs, slot, first=0, seed=5, n_blocks=1, want_f=True, u_norm=2):
    """pem_chain_sobol_sweep_f64_dev on a synthetic chain: (f_out [n_p][nv + 2][nq][n + 2] padded with NaN, partial, flags)"""
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd import sobol as study
    import test_chain_uion as tcu
    kind, a, b = (torch.as_tensor(np.ascontiguousarray(t), device='cuda') for t in tabs)
    n_p = kind.shape[0]
    nv, nq = len(study.GROUP_INPUTS[group]), len(study.GROUP_QOIS[group])
    f = torch.full((n_p * (nv + 2) * nq * n + 2,), np.nan, dtype=torch.float64, device='cuda') if want_f else None
    partial = torch.full((n_p, n_blocks, 2 + 4 * nv, nq), np.nan, dtype=torch.float64, device='cuda')
    flags = torch.full((n_p, n_blocks, 2), -1, dtype=torch.int64, device='cuda')
    rows, is_log, sa, sw = (np.ascontiguousarray(v, dtype=t) for v, t in zip(slot, (np.int32, np.int32, np.float64, np.float64)))
    ur = cs['u_rank']
    _lib.check(_lib.load().pem_chain_sobol_sweep_f64_dev(
        study.GROUPS.index(group), n, first, seed, n_p, _p(kind), _p(a), _p(b), N_EXT + 2, VCC, IB0, cs['arr'], cs['vmap'][0], cs['vmap'][1],
        _hp(rows), _hp(is_log), _hp(sa), _hp(sw), ur, NCELLS, u_norm, tcu.U_SCALE[u_norm], _p(cs['ubasis']) if ur else None, CELL, _p(f),
        _p(partial), _p(flags), n_blocks, None))
    torch.cuda.synchronize()
    if want_f:
        assert torch.isnan(f[-2:]).all(), 'wrote past f_out'
        f = f[:-2].reshape(n_p, nv + 2, nq, n)
    return f, partial, flags


def _linear_tables(group, n_p):
    """uniform priors that differ per pressure, pins inside the box, and the all-linear slot map over the box [0, 10] of every input"""
    from hallthrusterpem_amd import sobol as study
    kind = np.zeros((n_p, 15), dtype=np.int32)
    a = np.array([[1.0 + 0.3 * c + 1.5 * p for c in range(15)] for p in range(n_p)])
    b = a + np.array([[2.0 + 0.1 * c for c in range(15)] for p in range(n_p)])
    pins = [c for c, k in enumerate(study.PEM_V0_NOMINAL) if k not in study.GROUP_INPUTS[group]]
    b[:, pins] = a[:, pins]
    slot = (np.array(GROUP_ROWS[group]), np.zeros(N_EXT, dtype=np.int32), np.zeros(N_EXT), np.full(N_EXT, 10.0))
    return (kind, a, b), slot


def _design_coords(group, n, first, seed, tabs, slot):
    """the external coordinates of every evaluation, formed in numpy from sampler_np rows: [n_ext][n_p (nv + 2) n], evaluation-major"""
    import chain_sobol_np as csn
    from hallthrusterpem_amd import sobol as study
    kind, a, b = tabs
    n_p = kind.shape[0]
    cols = [list(study.PEM_V0_NOMINAL).index(k) for k in study.GROUP_INPUTS[group]]
    blocks = []
    for p in range(n_p):
        xa, xb = csn.rows(group, n, first, seed, n_p, p, kind[p], a[p], b[p])
        blocks += [csn.coords(xa, *slot), csn.coords(xb, *slot)]
        for c in cols:
            x = xa.copy()
            x[c] = xb[c]
            blocks.append(csn.coords(x, *slot))
    return np.concatenate(blocks, axis=1)


CASES = [
    # group, u_rank, outers (cathode, thruster, plume), big
    ('Cathode', 1, (2, 1, 0), False),
    ('Cathode', 0, (4, 0, 1), False),
    ('Thruster', 0, (1, 2, 0), False),            # no latents: the u_ion column is NaN
    ('Thruster', 1, (0, 3, 1), False),            # thruster width 3 exact; a cathode table of few slots: V_cc of row A is reused
    ('Thruster', 3, (3, 1, 2), False),            # width 16 guarded
    ('Thruster', 3, (2, 3, 0), True),             # level-4 dimensions: 51 outer-basis words, 118 KB of LDS
    ('Cathode', 1, (2, 0, 0), True),              # 34 words: 86 KB
]


@pytest.mark.parametrize('group, u_rank, outers, big', CASES, ids=[f'{c[0]}-u{c[1]}-{"".join(map(str, c[2]))}{"-big" if c[3] else ""}' for c in CASES])
def test_f_bits_against_the_chained_predict(group, u_rank, outers, big):
    """linear slots and uniform priors: every f equals the row of pem_sparse_predict_chain_fields_f64_dev (and column CELL of its
    u_ion field) at coordinates formed in numpy from sampler_np rows; n_base = 300 is two grid-stride rounds of one workgroup with
    dead lanes in the second"""
    import torch
    import test_chain_uion as tcu
    from hallthrusterpem_amd import sobol as study
    n, n_p, seed = 300, 2, 5
    torch.manual_seed(u_rank)
    rng = np.random.default_rng(100 * u_rank + len(group) + 7 * big)
    cs = _chain(rng, outers, u_rank, big)
    words = max((na - 1 if na > 1 else 0) * ((1 << lv) + 1 if lv else 1) for *_, na, lv in cs['keep'][0][:2 if group == 'Thruster' else 1])
    lds = (words + N_EXT + 2) * 2048
    print(f'{group}: {words} outer-basis words, {lds} B of bases and coordinates')
    assert (lds > 64 * 1024) == big
    tabs, slot = _linear_tables(group, n_p)
    nv, nq = len(study.GROUP_INPUTS[group]), len(study.GROUP_QOIS[group])
    f, partial, flags = _launch(cs, group, n, tabs, slot, seed=seed, n_blocks=1)
    assert f.shape == (n_p, nv + 2, nq, n)
    # the reference: ONE chained predict over all n_p (nv + 2) n coordinates
    t = torch.from_numpy(_design_coords(group, n, 0, seed, tabs, slot)).cuda()
    ref = dict(cs, t=t, n=t.shape[1], ld=t.shape[1])
    out, _, ufield = tcu._predict(ref, 1, 2, want_field=False)
    rows = out[:, :t.shape[1]].reshape(out.shape[0], n_p, nv + 2, n)
    if group == 'Cathode':
        assert torch.equal(f[:, :, 0], rows[0]), 'V_cc'
    else:
        assert torch.equal(f[:, :, 0], rows[2]), 'T'
        if u_rank:
            assert torch.equal(f[:, :, 1], ufield[:t.shape[1], CELL].reshape(n_p, nv + 2, n)), 'u_ion: the field column'
        else:
            assert ufield is None and torch.isnan(f[:, :, 1]).all()
    # the counts, from the reference's rows
    tv = 2.0 * (rows[0].cpu().numpy() - cs['vmap'][0]) / cs['vmap'][1] - 1.0
    assert int(flags[:, :, 1].sum()) == int((~((tv >= -1.0) & (tv <= 1.0))).sum()), 'V_cc coordinates outside [-1, 1]'
    want_bad = int(((rows[2] < 0) | (rows[1] < 0)).sum()) if group == 'Thruster' else 0
    assert int(flags[:, :, 0].sum()) == want_bad, 'non-physical thruster values'
    # the launch shape changes no bit; nor does asking for f
    f3, partial3, flags3 = _launch(cs, group, n, tabs, slot, seed=seed, n_blocks=3)
    assert torch.equal(f3.nan_to_num(), f.nan_to_num()) and torch.equal(flags3.sum(dim=1), flags.sum(dim=1))
    _, partial_nf, flags_nf = _launch(cs, group, n, tabs, slot, seed=seed, n_blocks=3, want_f=False)
    assert torch.equal(partial_nf.nan_to_num(), partial3.nan_to_num()) and torch.equal(flags_nf, flags3)
    assert torch.isfinite(partial3[..., 0]).all()
    # first_index: the tail of the launch from 0
    ft, _, _ = _launch(cs, group, n - 37, tabs, slot, first=37, seed=seed, n_blocks=2)
    assert torch.equal(ft.nan_to_num(), f[..., 37:].nan_to_num()) and torch.equal(ft.isnan(), f[..., 37:].isnan())
    # another seed is another design
    assert not torch.equal(_launch(cs, group, n, tabs, slot, seed=seed + 1)[0][:, :, 0], f[:, :, 0])


def _log_tables(group, pressures):
    """the study's own prior tables (P_b Relative around the pressure, a_1 log-uniform) and a slot map with log10 slots for P_b and a_1
    over the PEM-v0 boxes"""
    from hallthrusterpem_amd import sampling
    from hallthrusterpem_amd import sobol as study
    names = list(study.PEM_V0_NOMINAL)
    tabs = study.prior_tables(pressures, group)
    pri = [sampling.PEM_V0_PRIORS[names[r]] for r in GROUP_ROWS[group]]
    slot = (np.array(GROUP_ROWS[group]), np.array([p.kind == sampling.LOGUNIFORM for p in pri], dtype=np.int32),
            np.array([p.a for p in pri]), np.array([np.float64(p.b) - np.float64(p.a) for p in pri]))
    return tabs, slot


def _restated(group, n, seed, tabs, slot, chain, u, first=0):
    """(f [n_p][nv + 2][nq][n], bound [n_p][nq]) of the restatement: the bound is 4 x the largest change of f when every log10 value
    moves by one ulp either way, plus chain_loglik_np.CHAIN_REL max |f| (how the project holds chain_np.compose to the chain), both
    from the reference side only"""
    import chain_loglik_np as cl
    import chain_sobol_np as csn
    kind, a, b = tabs
    n_p = kind.shape[0]
    up = lambda x: np.nextafter(np.log10(x), np.inf)                                          # noqa: E731
    down = lambda x: np.nextafter(np.log10(x), -np.inf)                                       # noqa: E731
    f, bound = [], []
    for p in range(n_p):
        f0, fu, fd = (csn.sweep_f(group, n, first, seed, n_p, p, kind[p], a[p], b[p], slot, chain, u, log10=lg) for lg in (np.log10, up, down))
        moved = np.maximum(np.abs(fu - f0), np.abs(fd - f0)).max(axis=(0, 2))
        f.append(f0)
        bound.append(4 * moved + cl.CHAIN_REL * np.abs(f0).max(axis=(0, 2)))
    return np.stack(f), np.stack(bound)


@pytest.mark.parametrize('group', ['Cathode', 'Thruster'])
def test_log10_slots_against_the_restatement_and_the_sums(group):
    """P_b and a_1 through log10 slots: the device log10 may differ from numpy's by an ulp, so |f - restatement| is held to the bound of
    `_restated`; and the indices and standard errors from `partial` against sobol_sweep_np.estimates applied to the launch's own f
    (only the summation order differs: test_sobol_sweep's rule and atol)"""
    import chain_sobol_np as csn
    from test_sobol_sweep import _close
    from hallthrusterpem_amd import sobol as study
    n, seed, pressures = 300, 9, (1e-6, 1e-4)
    rng = np.random.default_rng(31 + len(group))
    cs = _chain(rng, (2, 2, 1), 1, False)
    tabs, slot = _log_tables(group, pressures)
    assert slot[1].sum() == (2 if group == 'Thruster' else 1)
    u = dict(basis=cs['ubasis'].cpu().numpy(), cell=CELL, norm=2, scale=1e-3)
    f, partial, flags = _launch(cs, group, n, tabs, slot, seed=seed, n_blocks=3)
    got = f.cpu().numpy()
    want, bound = _restated(group, n, seed, tabs, slot, _np_chain(cs), u)
    err = np.abs(got - want).max(axis=(1, 3))
    print(f'{group}: largest |f - restatement| per pressure and QoI {err.tolist()}, bound {bound.tolist()}')
    assert np.isfinite(got).all() and np.all(err <= bound), (err, bound)
    # the sums
    nv = len(study.GROUP_INPUTS[group])
    for nb in (3, 1):
        if nb == 1:
            f1, partial, _ = _launch(cs, group, n, tabs, slot, seed=seed, n_blocks=1)
            assert np.array_equal(f1.cpu().numpy(), got)
        s = partial.sum(dim=1).cpu().numpy()                                                 # [P][rows][nq]
        mean = s[:, 0] / (2 * n)
        var = s[:, 1] / (2 * n) - mean * mean
        m1, m1sq, m2, m2sq = (s[:, 2 + w::4] / n for w in range(4))
        assert m1.shape == (2, nv, len(csn.GROUP_QOIS[group]))
        for p in range(2):
            for k, q in enumerate(csn.GROUP_QOIS[group]):
                rec = csn.estimates(got[p], group)[q]
                v = var[p, k]
                mine = {'S1': m1[p, :, k] / v, 'ST': m2[p, :, k] / (2 * v), 'S1_se': np.sqrt((m1sq[p, :, k] - m1[p, :, k] ** 2) / n) / v,
                        'ST_se': np.sqrt((m2sq[p, :, k] - m2[p, :, k] ** 2) / n) / (2 * v)}
                for key, val in mine.items():
                    _close(val, rec[key], rec, 2e-9, f'{group} {q} {key} p={p} n_blocks={nb}')
                _close(mean[p, k], rec['mean'], rec, 2e-9, 'mean')


# ---- the driver on a chain trained on the test double --------------------------------------------------------------------------
VARIED = ('P_b', 'T_e', 'V_vac', 'Pstar', 'P_T', 'mdot_a', 'a_1')
N_REFINE, N, SEED, PRESSURES = 48, 4096, 3, (1e-6, 1e-4)


def _fixed(**over):
    from hallthrusterpem_amd import sobol as study
    fx = {k: v for k, v in study.PEM_V0_NOMINAL.items() if k not in VARIED}
    fx.update(over)
    return fx


@pytest.fixture(scope='module')
def trained():
    import torch
    from hallthrusterpem_amd.chain import ChainedSurrogate
    t0 = time.perf_counter()
    s = ChainedSurrogate(VARIED, _fixed(), max_level=3, u_ion=True, field=False)
    for it in range(N_REFINE):
        s.refine_step(num_refine=500, seed=it)
    torch.cuda.synchronize()
    print(f'chain trained in {time.perf_counter() - t0:.2f} s, evaluations {s.model_evals}')
    return s


@pytest.fixture(scope='module')
def swept(trained):
    from hallthrusterpem_amd import drivers
    return drivers.sobol_sweep(N, pressures=PRESSURES, qois=('V_cc', 'T', 'uion'), seed=SEED, surrogate=trained)


def _trained_np(s):
    """the restatement's view of the trained chain, from the tables of `stage_tables`"""
    import chain_sobol_np as csn
    _, keep = s.stage_tables()
    stages = [csn.stage_from_tables(keep[3 * k].cpu().numpy(), keep[3 * k + 1].cpu().numpy(), keep[3 * k + 2].cpu().numpy(), s.n_dim)
              for k in range(3)]
    vlo, vhi = s.domains[0]
    cu = s.u_compression
    return (dict(stages=stages, vcc_slot=s.vcc_slot, ib0_slot=s.ib0_slot, vmap=(vlo, vhi - vlo)),
            dict(basis=cu.basis.cpu().numpy(), norm=cu.norm, scale=cu.scale))


def _own_f(s, group, n, sm, cell, n_blocks=2):
    """the entry point as the driver calls it for `group`, with f_out"""
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd import sobol as study
    kind, a, b = (torch.as_tensor(t, device='cuda') for t in study.prior_tables(np.asarray(PRESSURES), group))
    nv, nq = len(study.GROUP_INPUTS[group]), len(study.GROUP_QOIS[group])
    f = torch.full((2, nv + 2, nq, n), np.nan, dtype=torch.float64, device='cuda')
    partial = torch.empty((2, n_blocks, 2 + 4 * nv, nq), dtype=torch.float64, device='cuda')
    flags = torch.empty((2, n_blocks, 2), dtype=torch.int64, device='cuda')
    st, _keep = s.stage_tables()
    cu = s.u_compression
    ub = cu.basis.contiguous()
    vlo, vhi = s.domains[0]
    _lib.check(_lib.load().pem_chain_sobol_sweep_f64_dev(
        study.GROUPS.index(group), n, 0, SEED, 2, _p(kind), _p(a), _p(b), s.n_dim, s.vcc_slot, s.ib0_slot, st, vlo, vhi - vlo, _hp(sm.rows),
        _hp(sm.is_log), _hp(sm.a), _hp(sm.w), cu.rank, s.uion_grid[2], cu.norm, cu.scale, _p(ub), cell, _p(f), _p(partial), _p(flags), n_blocks,
        None))
    torch.cuda.synchronize()
    return f.cpu().numpy(), int(flags[:, :, 1].sum())


@pytest.mark.parametrize('group', ['Cathode', 'Thruster'])
def test_driver_against_the_restatement(trained, swept, group):
    """`sobol_sweep(surrogate=)` in two steps that together hold it to the restatement: its indices and standard errors equal
    sobol_sweep_np.estimates of the f the same launch writes (rule of the sums: only the summation order differs), and that f
    equals the restatement built from `stage_tables` within the bound of the log10 slots (on the first N_F base samples: an f
    depends on its sample's index, not on n_base)."""
    import chain_sobol_np as csn
    from test_sobol_sweep import _close
    from hallthrusterpem_amd import sobol as study
    s, res = trained, swept
    assert res['surrogate'] is True and res['non_physical'] == 0 and res['invalid'] == 0
    assert res['evaluations'] == N * 2 * (7 + 6)
    cell, _ = study.uion_node(study.L_CH, s.uion_grid)
    sm = study.surrogate_sweep_map(s.varied, s.fixed, s.priors, PRESSURES, group, True, study.GROUP_QOIS[group])
    f, outside = _own_f(s, group, N, sm, cell)
    assert np.isfinite(f).all()
    for p in range(2):
        est = csn.estimates(f[p], group)
        for q in study.GROUP_QOIS[group]:
            assert res[q]['inputs'] == study.GROUP_INPUTS[group]
            for key in ('S1', 'ST', 'S1_se', 'ST_se'):
                _close(res[q][key][p].cpu().numpy(), est[q][key], est[q], 2e-9, f'{q} {key} p={p}')
            _close(res[q]['mean'][p].cpu().numpy(), est[q]['mean'], est[q], 2e-9, f'{q} mean p={p}')
    N_F = 512
    chain, u = _trained_np(s)
    u['cell'] = cell
    t0 = time.perf_counter()
    want, bound = _restated(group, N_F, SEED, study.prior_tables(np.asarray(PRESSURES), group), (sm.rows, sm.is_log, sm.a, sm.w), chain, u)
    err = np.abs(f[..., :N_F] - want).max(axis=(1, 3))
    print(f'{group}: restated in {time.perf_counter() - t0:.2f} s; largest |f - restatement| {err.tolist()}, bound {bound.tolist()}; '
          f'V_cc coordinates outside [-1, 1]: {outside} of {f.shape[0] * f.shape[1] * N}')
    assert np.all(err <= bound), (err, bound)


def test_driver_structure_and_the_plume_group(trained, swept):
    import torch
    from hallthrusterpem_amd import drivers
    v = swept['V_cc']
    st = v['ST'].cpu().numpy()
    assert np.all(np.argmax(st, axis=1) == list(v['inputs']).index('V_vac'))
    assert swept['extrapolated'] >= 0 and set(swept) >= {'V_cc', 'T', 'uion', 'P_b', 'surrogate', 'extrapolated', 'evaluations'}
    for q in ('V_cc', 'T', 'uion'):
        for key in ('S1', 'ST', 'S1_se', 'ST_se'):
            assert swept[q][key].shape == (2, len(swept[q]['inputs'])) and torch.isfinite(swept[q][key]).all(), (q, key)
    # the Plume group stays on the model: the same bits with and without a surrogate
    plain = drivers.sobol_sweep(N, pressures=PRESSURES, qois=('jion',), seed=SEED)
    both = drivers.sobol_sweep(N, pressures=PRESSURES, qois=('T', 'jion'), seed=SEED, surrogate=trained)
    assert 'surrogate' not in plain and both['surrogate'] is True
    for key in ('S1', 'ST', 'S1_se', 'ST_se', 'mean', 'var', 'clip', 'j0'):
        assert torch.equal(both['jion'][key], plain['jion'][key]), key
    assert np.array_equal(both['jion']['rejected'], plain['jion']['rejected'])
    assert torch.equal(both['T']['S1'], swept['T']['S1'])
    # one seed, one design: the model's own sweep of V_cc is close to the surrogate's (a trained chain, no figure asserted)
    model = drivers.sobol_sweep(N, pressures=PRESSURES, qois=('V_cc',), seed=SEED)
    print('V_cc ST model', model['V_cc']['ST'].cpu().numpy().tolist(), 'surrogate', st.tolist())


def test_driver_refusals(trained):
    from hallthrusterpem_amd import drivers
    from hallthrusterpem_amd.chain import ChainedSurrogate
    off = ChainedSurrogate(tuple(k for k in VARIED if k != 'Pstar'), _fixed(Pstar=5e-5), max_level=3, field=False)
    with pytest.raises(ValueError, match='Pstar'):
        drivers.sobol_sweep(256, pressures=PRESSURES, qois=('V_cc',), surrogate=off)
    with pytest.raises(ValueError, match='uion'):                                         # `off` carries no latents
        drivers.sobol_sweep(256, pressures=PRESSURES, qois=('uion',), surrogate=off)
    with pytest.raises(ValueError, match='grid'):
        drivers.sobol_sweep(256, pressures=PRESSURES, qois=('uion',), surrogate=trained, uion_grid=(0.0, 0.08, 150))
    # T alone from a chain without latents: served (refined first: an untrained chain is one constant grid per stage, and the indices
    # of a constant are 0 / 0)
    ok = ChainedSurrogate(VARIED, _fixed(), max_level=3, field=False)
    for it in range(24):
        ok.refine_step(num_refine=500, seed=it)
    r = drivers.sobol_sweep(256, pressures=PRESSURES, qois=('T',), surrogate=ok)
    print('T of a chain without latents: var', r['T']['var'].cpu().numpy().tolist(), 'S1', r['T']['S1'].cpu().numpy().tolist())
    assert 'uion' not in r and (r['T']['var'] > 0).all() and np.isfinite(r['T']['S1'].cpu().numpy()).all()
    assert np.isfinite(r['T']['ST_se'].cpu().numpy()).all()
