"""The Sobol' study through the chained surrogate, without a GPU: pem_chain_sobol_sweep_f64_dev is declared, bound and refuses every
malformed call before it looks for a device; `sobol.surrogate_sweep_map` refuses what a chain cannot serve; the restatement
tests/chain_sobol_np.py reproduces the closed-form indices of a chain whose tables interpolate a quadratic exactly; the new unit's
kernels neither spill a vector register nor touch scratch."""
import ctypes as C
import re
import shutil
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT))
ENTRY = 'pem_chain_sobol_sweep_f64_dev'


def test_symbol_is_declared_and_bound():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    assert re.search(r'\bint\s+%s\s*\(' % ENTRY, header)
    assert ENTRY in _lib.SIGNATURES and len(_lib.SIGNATURES[ENTRY][1]) == 29
    assert hasattr(_lib.load(), ENTRY)
    assert any(s.name == 'pem_surrogate_sobol.hip' for s in build.SRCS)
    unit = (ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_surrogate_sobol.hip').read_text()
    assert '#include "pem_surrogate_fields.hip"' in unit


# ---- the entry point's refusals ---------------------------------------------------------------------------------------------------
def _call(group=1, n_base=1000, n_p=2, tables=True, n_dim=6, vcc_slot=4, ib0_slot=5, stages=True, outs=None, vcc=(20.0, 25.0),
          slot_row=(0, 6, 2, 7), slot_tab=True, slot_a=(0.0,) * 4, slot_w=(1.0,) * 4, u_rank=1, u_dof=200, u_norm=2, u_scale=1e-3,
          u_basis=True, u_cell=62, partial=True, flags=True, n_blocks=3, levels=(5, 4)):
    from hallthrusterpem_amd import _lib
    fake = C.c_void_p(4096)                       # never dereferenced: every check below runs on the host
    arr = (_lib.SurrStage * 3)()
    for k, no in enumerate(outs or (1, 2 + max(u_rank, 0), 3)):
        arr[k] = _lib.SurrStage(4096, 4096, 4096, 3, no, *levels)
    keep = [np.asarray(slot_row, dtype=np.int32), np.zeros(len(slot_row), dtype=np.int32), np.asarray(slot_a, dtype=np.float64),
            np.asarray(slot_w, dtype=np.float64)]
    ptrs = [k.ctypes.data_as(C.c_void_p) if slot_tab else None for k in keep]
    return _lib.load().pem_chain_sobol_sweep_f64_dev(
        group, n_base, 0, 7, n_p, fake if tables else None, fake, fake, n_dim, vcc_slot, ib0_slot, arr if stages else None, vcc[0], vcc[1],
        *ptrs, u_rank, u_dof, u_norm, u_scale, fake if u_basis else None, u_cell, None, fake if partial else None, fake if flags else None,
        n_blocks, None)


BAD = [
    dict(group=2), dict(group=3), dict(group=-1),                                        # the Plume group stays on the model
    dict(u_rank=15, outs=(1, 17, 3)), dict(u_rank=-1), dict(u_rank=2, outs=(1, 3, 3)),    # 0 .. 14, and 2 + u_rank thruster outputs
    dict(u_cell=200), dict(u_cell=-1), dict(u_cell=7, u_dof=7),                           # a cell outside the grid
    dict(tables=False), dict(partial=False), dict(flags=False), dict(slot_tab=False), dict(stages=False), dict(u_basis=False),
    dict(n_p=0), dict(n_p=65536), dict(n_base=0), dict(n_base=(1 << 40) + 1), dict(n_blocks=0),
    dict(slot_row=(0, 6, 2, 2)), dict(slot_row=(0, 6, 2, 15)), dict(slot_row=(0, 6, 2, -1)),       # distinct input rows 0 .. 14
    dict(slot_row=(0, 6, 2, 1)),                                                          # a_1 (row 7), which the group varies, has no slot
    dict(group=0, slot_row=(0, 6, 2, 7)),                                                 # nor have V_vac, Pstar, P_T for the Cathode group
    dict(slot_w=(1.0, 0.0, 1.0, 1.0)), dict(slot_w=(1.0, -2.0, 1.0, 1.0)), dict(slot_a=(0.0, float('nan'), 0.0, 0.0)),
    dict(vcc=(20.0, 0.0)), dict(vcc_slot=5), dict(u_scale=0.0), dict(u_norm=5), dict(u_dof=1),
    dict(n_dim=12, vcc_slot=10, ib0_slot=11, slot_row=tuple(range(10)), slot_a=(0.0,) * 10, slot_w=(1.0,) * 10),   # 4 x 17 + 12 slots: > 160 KB
]


@pytest.mark.parametrize('bad', BAD, ids=lambda b: ','.join(f'{k}={v}' for k, v in b.items())[:40])
def test_entry_point_refuses_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_chain_sobol_sweep' in _lib.load().pem_last_error()


def test_well_formed_calls_need_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    for kw in (dict(), dict(u_rank=0, u_basis=False, u_cell=-5), dict(u_rank=14), dict(group=0, slot_row=(0, 2, 3, 4, 5), n_dim=7, vcc_slot=5,
                                                                                      ib0_slot=6, slot_a=(0.0,) * 5, slot_w=(1.0,) * 5),
               dict(n_p=65535), dict(levels=(5, 3), n_dim=12, vcc_slot=10, ib0_slot=11, slot_row=tuple(range(10)), slot_a=(0.0,) * 10,
                                     slot_w=(1.0,) * 10)):
        assert _call(**kw) == _lib.PEM_ERR_NO_DEVICE, kw


# ---- the host map's refusals ------------------------------------------------------------------------------------------------------
VARIED = ('P_b', 'T_e', 'V_vac', 'Pstar', 'P_T', 'mdot_a', 'a_1')


def _fixed(**over):
    from hallthrusterpem_amd import sobol as study
    fx = {k: v for k, v in study.PEM_V0_NOMINAL.items() if k not in VARIED}
    fx.update(over)
    return fx


def _map(group='Thruster', varied=VARIED, fixed=None, priors=None, pressures=(1e-6, 1e-4), has_uion=True, qois=('T', 'uion')):
    from hallthrusterpem_amd import sampling
    from hallthrusterpem_amd import sobol as study
    pri = dict(sampling.PEM_V0_PRIORS)
    pri.update(priors or {})
    return study.surrogate_sweep_map(varied, _fixed() if fixed is None else fixed, pri, pressures, group, has_uion, qois)


def test_sweep_map_of_a_chain_that_serves_the_study():
    from hallthrusterpem_amd import sampling
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    for g, q in (('Cathode', ('V_cc',)), ('Thruster', ('T', 'uion'))):
        m = _map(g, qois=q)
        assert [COUPLED_INPUTS[r] for r in m.rows] == list(VARIED) and m.rows.dtype == np.int32 and m.is_log.dtype == np.int32
        for k, name in enumerate(VARIED):
            p = sampling.PEM_V0_PRIORS[name]
            assert m.is_log[k] == (p.kind == sampling.LOGUNIFORM) and m.a[k] == p.a and m.w[k] == np.float64(p.b) - np.float64(p.a)
        x = np.array([[2e-5], [300.0], [2.0], [30.0], [5e-5], [5e-5], [5e-6], [0.01]] + [[1.0]] * 7)
        t = m.coords(x)
        assert t.shape == (7, 1) and t[0, 0] == 2.0 * (np.log10(2e-5) - -8.0) / 4.0 - 1.0 and t[1, 0] == 2.0 * (2.0 - 1.0) / 4.0 - 1.0
    # plume-only inputs are not examined: a chain may fix them anywhere, or vary them under any prior
    weird = {'c0': sampling.Prior(sampling.NORMAL, 0.5, 0.1, 'normal')}
    m = _map(varied=VARIED + ('c0',), fixed={k: v for k, v in _fixed(c1=0.3, sigma_cex=51e-20).items() if k != 'c0'}, priors=weird)
    assert len(m.rows) == 8 and np.isfinite(m.a).all() and (m.w > 0).all()
    # a chain that varies V_a (the study pins it inside the box) serves it too
    assert len(_map(varied=VARIED + ('V_a',), fixed={k: v for k, v in _fixed().items() if k != 'V_a'}).rows) == 8


def _without(*names):
    return tuple(k for k in VARIED if k not in names)


def _refusals():
    from hallthrusterpem_amd import sampling
    P, U, LU = sampling.Prior, sampling.UNIFORM, sampling.LOGUNIFORM
    with_va = dict(varied=VARIED + ('V_a',), fixed={k: v for k, v in _fixed().items() if k != 'V_a'})
    return [
        # the chain does not vary one of the group's varied inputs
        ('fixes-mdot_a', dict(varied=_without('mdot_a'), fixed=_fixed(mdot_a=5e-6)), 'mdot_a'),
        ('fixes-Pstar-cathode', dict(group='Cathode', qois=('V_cc',), varied=_without('Pstar'), fixed=_fixed(Pstar=3.463406e-05)), 'Pstar'),
        # it fixes an input the group's stages read at another value than the study pins it at
        ('Pstar-5e-5', dict(qois=('T',), varied=_without('Pstar'), fixed=_fixed(Pstar=5e-5)), 'Pstar'),
        ('V_a-250', dict(fixed=_fixed(V_a=250.0)), 'V_a'),
        # a sweep range or a pin outside the chain's box
        ('T_e-box', dict(priors={'T_e': P(U, 1.5, 5.0, '')}), 'T_e'),                       # the study draws T_e on [1, 5]
        ('P_b-box', dict(priors={'P_b': P(LU, -8.0, -4.2, '')}), 'P_b'),                     # Relative(20) around 1e-4 reaches 1e-4 > 10^-4.2
        ('P_b-box-low', dict(priors={'P_b': P(LU, -6.05, -4.0, '')}), 'P_b'),                # 0.8e-6 < 10^-6.05
        ('mdot_a-box', dict(priors={'mdot_a': P(U, 4.9e-6, 7e-6, '')}), 'mdot_a'),           # Relative(3): from 4.85e-6
        ('V_a-pin', dict(priors={'V_a': P(U, 310.0, 400.0, '')}, **with_va), 'V_a'),         # pinned at 300
        ('Pstar-pin', dict(priors={'Pstar': P(U, 4e-5, 1e-4, '')}), 'Pstar'),                # pinned at 3.46e-5 in the Thruster group
        # a normal prior of a varied input
        ('V_vac-normal', dict(priors={'V_vac': P(sampling.NORMAL, 30.0, 5.0, '')}), 'V_vac'),
        ('uion', dict(has_uion=False), 'uion'),
        ('plume', dict(group='Plume', qois=('jion',)), 'Plume'),
    ]


@pytest.mark.parametrize('name, kw, match', _refusals(), ids=[r[0] for r in _refusals()])
def test_sweep_map_refuses_and_names_the_input(name, kw, match):
    with pytest.raises(ValueError, match=match):
        _map(**kw)
    if name == 'Pstar-5e-5':                                # the same chain serves neither group: the cathode stage reads Pstar in both
        with pytest.raises(ValueError, match='Pstar'):
            _map(**dict(kw, group='Cathode', qois=('V_cc',)))


def test_driver_refuses_before_any_device_work():
    from hallthrusterpem_amd import drivers, sampling

    class Chain:                                            # what the driver reads of a ChainedSurrogate before it launches
        varied, priors, uion_grid, u_compression = tuple(k for k in VARIED if k != 'Pstar'), sampling.PEM_V0_PRIORS, (0.0, 0.08, 200), None
        fixed = _fixed(Pstar=5e-5)
    with pytest.raises(ValueError, match='Pstar'):
        drivers.sobol_sweep(100, qois=('V_cc',), surrogate=Chain())
    with pytest.raises(ValueError, match='grid'):
        drivers.sobol_sweep(100, qois=('V_cc',), surrogate=Chain(), uion_grid=(0.0, 0.08, 150))
    Chain.fixed = _fixed(Pstar=3.463406e-05)
    with pytest.raises(ValueError, match='uion'):
        drivers.sobol_sweep(100, qois=('T', 'uion'), surrogate=Chain())


# ---- the restatement on tables that interpolate a quadratic exactly: closed-form indices ---------------------------------------------
N_DIM, VCC, IB0 = 10, 8, 9                                  # slots 0 .. 7: P_b V_a T_e V_vac Pstar P_T mdot_a a_1
VMAP, IMAP = (20.0, 25.0), (2.0, 3.0)
CAT = dict(lin=[4.0, 1.5, 2.5, 3.0, -2.0, 1.0], quad=[1.0, 0.5, -1.5, 0.8, 0.6, -0.4], cross=2.0)          # slots 0 .. 5; the cross term: t_0 t_2
T_TV, T_MD, T_A1 = 0.02, (0.01, 0.004), 0.003               # T = 0.08 + T_TV tv + T_MD . (t_6, t_6^2) + T_A1 t_7 + 0.001 t_1
L_TV, L_MD = 20.0, 5.0                                      # latent = 100 + L_TV tv + L_MD t_6
UB, USCALE, CELL = np.linspace(0.01, 0.1, 7)[:, None], 1e-3, 4


def _grids(terms, n_out):
    """a table as test_chained_surrogate._stage builds one -- (betas, coefficients, values per beta) -- whose grids are level 1 in their
    active slots (3 nodes: a quadratic is interpolated exactly); terms: [({slot: level}, f(t) -> [n_out][nodes])]; in the dict form
    oracle/surrogate_np.predict reads"""
    import itertools

    from oracle import surrogate_np as snp
    betas, coefs, values = [], {}, {}
    for levels, f in terms:
        beta = tuple(levels.get(d, 0) for d in range(N_DIM))
        pts = np.array(list(itertools.product(*[snp.nodes(l) for l in beta]))).T
        betas.append(beta)
        coefs[beta] = 1.0
        values[beta] = np.asarray(f(pts), dtype=np.float64).reshape(n_out, -1).T
    return betas, coefs, values


def _quadratic_chain():
    one = lambda t: np.ones(t.shape[1])                                                      # noqa: E731
    cat = [({}, lambda t: 30.0 * one(t))]
    cat += [({d: 1}, lambda t, d=d: CAT['lin'][d] * t[d] + CAT['quad'][d] * t[d] ** 2) for d in range(6)]
    cat.append(({0: 1, 2: 1}, lambda t: CAT['cross'] * t[0] * t[2]))
    z = lambda t: np.zeros(t.shape[1])                                                       # noqa: E731
    thr = [({}, lambda t: np.stack([3.0 * one(t), 0.08 * one(t), 100.0 * one(t)])),
           ({VCC: 1}, lambda t: np.stack([z(t), T_TV * t[VCC], L_TV * t[VCC]])),
           ({6: 1}, lambda t: np.stack([0.5 * t[6], T_MD[0] * t[6] + T_MD[1] * t[6] ** 2, L_MD * t[6]])),
           ({7: 1}, lambda t: np.stack([z(t), T_A1 * t[7], z(t)])),
           ({1: 1}, lambda t: np.stack([z(t), 0.001 * t[1], z(t)]))]
    plu = [({}, lambda t: 0.3 * one(t)), ({IB0: 1}, lambda t: 0.05 * t[IB0])]
    return dict(stages=[_grids(cat, 1), _grids(thr, 3), _grids(plu, 1)], vcc_slot=VCC, ib0_slot=IB0, vmap=VMAP, imap=IMAP)


def _uniform_tables(n_p):
    """kind, a, b [n_p][15], all uniform, and the all-linear slot map over the box [0, 10] of every input: t = x / 5 - 1.  Input c is
    drawn on [lo, hi] that depend on the pressure index (off-centre, narrower than the box) or pinned at lo."""
    from hallthrusterpem_amd import sobol as study
    kind = np.zeros((n_p, 15), dtype=np.int32)
    a, b = np.zeros((n_p, 15)), np.zeros((n_p, 15))
    for p in range(n_p):
        for c in range(15):
            a[p, c], b[p, c] = 1.0 + 0.5 * c / 15 + 2.0 * p, 6.0 + 0.2 * c + 1.5 * p
    tabs = {}
    for g in study.SURROGATE_GROUPS:
        pins = [list(study.PEM_V0_NOMINAL).index(k) for k in study.PEM_V0_NOMINAL if k not in study.GROUP_INPUTS[g]]
        bg = b.copy()
        bg[:, pins] = a[:, pins]
        tabs[g] = (kind, a, bg)
    slot = (np.arange(8), np.zeros(8, dtype=bool), np.zeros(8), np.full(8, 10.0))
    return tabs, slot


def test_restatement_reproduces_the_closed_form_indices_of_a_quadratic_chain():
    import chain_sobol_np as cs
    n, n_p, p = 4096, 2, 1
    chain = _quadratic_chain()
    tabs, slot = _uniform_tables(n_p)
    u = dict(basis=UB, cell=CELL, norm=2, scale=USCALE)
    tof = lambda x: 2.0 * (x - 0.0) / 10.0 - 1.0                                             # noqa: E731
    # the Cathode group: V_cc over slots P_b, T_e, V_vac, Pstar, P_T (the cross term couples the first two); V_a is a pin
    kind, a, b = tabs['Cathode']
    f = cs.sweep_f('Cathode', n, 0, 5, n_p, p, kind[p], a[p], b[p], slot, chain, u)
    assert f.shape == (7, 1, n)
    got = cs.estimates(f, 'Cathode')['V_cc']
    d = [0, 2, 3, 4, 5]
    s1, st = cs.quadratic_indices([CAT['lin'][k] for k in d], [CAT['quad'][k] for k in d], CAT['cross'], tof(a[p, d]), tof(b[p, d]))
    for k, want in (('S1', s1), ('ST', st)):
        assert np.all(got[k + '_se'] > 0) and np.all(np.abs(got[k] - want) <= 4 * got[k + '_se']), (k, got[k], want, got[k + '_se'])
    # the pin enters the value, not the indices: the restated V_cc IS the polynomial
    xa, _ = cs.rows('Cathode', n, 0, 5, n_p, p, kind[p], a[p], b[p])
    t = tof(xa[:6])
    want_v = 30.0 + sum(CAT['lin'][k] * t[k] + CAT['quad'][k] * t[k] ** 2 for k in range(6)) + CAT['cross'] * t[0] * t[2]
    assert np.all(np.abs(f[0, 0] - want_v) <= 1e-13 * np.abs(want_v).max())
    # the Thruster group (P_b, mdot_a, T_e, a_1): T and the latent are affine in the V_cc coordinate, V_cc is quadratic in P_b and T_e
    kind, a, b = tabs['Thruster']
    f = cs.sweep_f('Thruster', n, 0, 5, n_p, p, kind[p], a[p], b[p], slot, chain, u)
    assert f.shape == (6, 2, n)
    got = cs.estimates(f, 'Thruster')
    k = 2.0 / VMAP[1]                                                                         # d tv / d V_cc
    lo, hi = tof(a[p, [0, 2, 6, 7]]), tof(b[p, [0, 2, 6, 7]])                                 # the crossing pair first
    order = [0, 2, 1, 3]                                                                      # back to the group's P_b, mdot_a, T_e, a_1
    for q, c_tv, md, a1 in (('T', T_TV, T_MD, T_A1), ('uion', L_TV, (L_MD, 0.0), 0.0)):
        s1, st = cs.quadratic_indices([c_tv * k * CAT['lin'][0], c_tv * k * CAT['lin'][2], md[0], a1],
                                      [c_tv * k * CAT['quad'][0], c_tv * k * CAT['quad'][2], md[1], 0.0], c_tv * k * CAT['cross'], lo, hi)
        for key, want in (('S1', s1[order]), ('ST', st[order])):
            g, se = got[q][key], got[q][key + '_se']
            assert np.all(np.abs(g - want) <= 4 * se + 1e-12), (q, key, g, want, se)
        assert np.all(got[q]['ST_se'][:3] > 0)
    # u_ion is the latent times u_basis[cell] / scale: u_ion does not depend on a_1 at all
    assert got['uion']['ST'][3] == 0.0 and got['T']['ST'][3] > 0.0
    # without latents the u_ion row is NaN and T keeps its bits
    cut = dict(chain, stages=[chain['stages'][0], (chain['stages'][1][0], chain['stages'][1][1],
                                                   {bt: v[:, :2] for bt, v in chain['stages'][1][2].items()}), chain['stages'][2]])
    f0 = cs.sweep_f('Thruster', 64, 0, 5, n_p, p, kind[p], a[p], b[p], slot, cut, None)
    assert np.isnan(f0[:, 1]).all() and np.array_equal(f0[:, 0], f[:, 0, :64])


def test_restated_rows_are_the_model_sweeps():
    """one seed, one design: rows A and B of the restatement are sobol_sweep_np.design's for the Cathode and Thruster groups"""
    import chain_sobol_np as cs
    import sobol_sweep_np as ssn
    from hallthrusterpem_amd import sobol as study
    pb = study.DEFAULT_PRESSURES
    for g in study.SURROGATE_GROUPS:
        kind, a, b = study.prior_tables(pb, g)
        for p in (0, 4):
            xa, xb = cs.rows(g, 50, 0, 11, len(pb), p, kind[p], a[p], b[p])
            assert np.array_equal(xa, ssn.design(g, 50, 11, pb, p, 0, 133.3)[0]) and np.array_equal(xb, ssn.design(g, 50, 11, pb, p, 1, 133.3)[0])


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_sobol_chain_kernels_neither_spill_vgprs_nor_use_scratch():
    from test_kernel_resources import kernel_rows
    rows = kernel_rows('pem_surrogate_sobol.hip')
    assert sorted(rows) == ['chain_sobol_sweep_kernel<0, 2, true>', 'chain_sobol_sweep_kernel<1, 16, false>',
                            'chain_sobol_sweep_kernel<1, 2, true>', 'chain_sobol_sweep_kernel<1, 3, true>'], sorted(rows)
    for name, r in rows.items():          # 256 threads per workgroup: at most 256 registers keep two workgroups on a CU
        assert r['vspill'] == 0 and r['scratch'] == 0 and r['vgpr'] <= 256, (name, r)
