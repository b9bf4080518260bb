"""The surrogate posterior without a GPU: pem_chain_system_loglik_f64_dev is declared and bound and refuses every malformed call
before it looks for a device; tests/chain_loglik_np.py restates it in float64 and long double; the host input map of
calibration.SurrogatePosterior equals PemV0System._external_coords and refuses what the surrogate cannot serve; no instantiation of
the kernel spills a vector register."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
NAME = 'pem_chain_system_loglik_f64_dev'


def test_symbol_is_declared_and_bound():
    from hallthrusterpem_amd import _lib
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    assert re.search(r'\bint\s+%s\s*\(' % NAME, header)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 30
    assert hasattr(_lib.load(), NAME)


def _call(stages=True, n=1000, n_dim=4, vcc_slot=2, ib0_slot=3, vcc=(0.0, 1.0), ib0=(0.0, 1.0), t=True, ld=1000, lat0=1, rank=2, dof=91,
          norm=1, basis=True, n_cond=3, n_rec=9, rec=True, span=True, a_1=False, sigma=0.2, loglik=True, out=False, ld_out=1000,
          pred=False, ld_pred=9, outs=(1, 2, 3), active=(5, 5, 5), level=(4, 4, 4), null_table=None):
    from hallthrusterpem_amd import _lib
    fake = C.c_void_p(4096)                     # never dereferenced: every check below runs on the host
    arr = (_lib.SurrStage * 3)()
    for k in range(3):
        ptrs = [fake.value] * 3
        if null_table == k:
            ptrs[k % 3] = None
        arr[k] = _lib.SurrStage(ptrs[0], ptrs[1], ptrs[2], 3, outs[k], active[k], level[k])
    f = lambda on: fake if on else None                                                          # noqa: E731
    return _lib.load().pem_chain_system_loglik_f64_dev(
        n, n_dim, vcc_slot, ib0_slot, arr if stages else None, vcc[0], vcc[1], ib0[0], ib0[1], f(t), ld, lat0, rank, dof, norm, 1.0,
        f(basis), n_cond, n_rec, f(rec), f(span), f(a_1), 4.5, sigma, f(loglik), f(out), ld_out, f(pred), ld_pred, None)


@pytest.mark.parametrize('bad', [
    # the new rules
    dict(n_cond=0), dict(n_cond=1025), dict(n_rec=0), dict(n_rec=1025),
    dict(rec=False), dict(span=False), dict(loglik=False),
    dict(pred=True, ld_pred=8), dict(out=True, ld_out=999),
    dict(rank=0), dict(rank=17, outs=(1, 2, 16)), dict(lat0=1, rank=3), dict(lat0=2, rank=2), dict(lat0=-1), dict(dof=90), dict(dof=0),
    dict(norm=7), dict(norm=-1),
    dict(a_1=True, sigma=0.0), dict(a_1=True, sigma=-1.0), dict(a_1=True, sigma=float('nan')), dict(a_1=True, sigma=float('inf')),
    # a sample of the chain's own
    dict(stages=False), dict(null_table=0), dict(null_table=2), dict(outs=(2, 2, 3)), dict(outs=(1, 3, 3)), dict(outs=(1, 2, 17)),
    dict(active=(6, 5, 5)), dict(level=(4, 5, 4)), dict(vcc_slot=4), dict(vcc_slot=3), dict(n_dim=1), dict(n_dim=33),
    dict(vcc=(0.0, 0.0)), dict(ib0=(0.0, float('nan'))), dict(t=False), dict(ld=999),
    dict(n_dim=13),                              # 4 outer dimensions of 17 nodes and 13 coordinates: 162 KB of LDS
])
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_chain_system_loglik' in _lib.load().pem_last_error()


def test_a_well_formed_call_needs_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _call() == _lib.PEM_ERR_NO_DEVICE
    assert _call(n_dim=12, lat0=1, rank=2) == _lib.PEM_ERR_NO_DEVICE                        # 160 KB exactly: the tables go through the cache
    assert _call(basis=False, rank=0, dof=0, norm=9) == _lib.PEM_ERR_NO_DEVICE              # no j_ion map: its arguments are not looked at
    assert _call(a_1=True, out=True, pred=True, ld_pred=11, n_cond=1024, n_rec=1024, ld_out=1003) == _lib.PEM_ERR_INVALID_ARG   # ld_pred < n_rec
    assert _call(a_1=True, out=True, pred=True, ld_pred=1024, n_cond=1024, n_rec=1024, ld_out=1003) == _lib.PEM_ERR_NO_DEVICE
    assert _call(n_dim=2, vcc_slot=0, ib0_slot=1, t=False, ld=0) == _lib.PEM_ERR_NO_DEVICE
    assert _call(n=0, t=False, rec=False, span=False, loglik=False) == _lib.PEM_OK


# ---- the restatement on a hand-built chain whose stages interpolate low-degree polynomials exactly ---------------------------
def _table(rng, conds):
    """records {w, y, 1/std, bits} of conditions given as {kind: count}, each block padded to an odd count; span [n_cond][4][2]"""
    blocks, span, first = [], np.zeros((len(conds), 4, 2), dtype=np.int32), 0
    for c, kinds in enumerate(conds):
        cnt = sum(kinds.values())
        recs = np.zeros((cnt + (1 - cnt % 2), 4))
        at = 0
        for kd in (0, 1, 2, 3):                                   # blocks in any order would do: the spans say where each kind is
            m = kinds.get(kd, 0)
            if not m:
                continue
            span[c, kd] = (first + at, m)
            r = recs[at:at + m]
            r[:, 1] = {0: rng.uniform(0.0, 0.2, m), 1: rng.uniform(25, 40, m), 2: rng.uniform(0.07, 0.1, m), 3: rng.uniform(0, 1, m)}[kd]
            r[:, 2] = {0: rng.uniform(5, 50, m), 1: rng.uniform(0.5, 2, m), 2: rng.uniform(100, 300, m), 3: rng.uniform(1, 2, m)}[kd]
            if kd in (0, 3):
                r[:, 0] = rng.uniform(0, 1, m)
                r[:, 3] = np.sort(rng.integers(0, 90, m)).astype(np.int64).view(np.float64)
            at += m
        blocks.append(recs)
        first += recs.shape[0]
    return np.concatenate(blocks), span


def _hand_chain():
    from test_chained_surrogate_host import _tensor_stage
    n_dim, vs, ib = 4, 2, 3
    vcc_f = lambda t: 30.0 + 5.0 * t[0] + 2.0 * t[0] * t[1] + 3.0 * t[1] ** 2          # noqa: E731
    ib0_f = lambda t: 3.0 + 0.1 * t[2] + 0.05 * t[0] * t[2]                               # noqa: E731
    thr_f = lambda t: 0.08 + 0.01 * t[2] ** 2                                             # noqa: E731
    div_f = lambda t: 0.3 + 0.05 * t[3] - 0.02 * t[1] * t[3] ** 3                         # noqa: E731
    la_f = lambda t: -1.5 + 0.25 * t[3] ** 2 * t[1]                                       # noqa: E731
    lb_f = lambda t: 0.4 - 0.3 * t[3] + 0.1 * t[1]                                        # noqa: E731
    stages = [_tensor_stage(n_dim, {0: 1, 1: 2}, [vcc_f]), _tensor_stage(n_dim, {0: 1, 2: 2}, [ib0_f, thr_f]),
              _tensor_stage(n_dim, {1: 1, 3: 2}, [div_f, la_f, lb_f])]
    return stages, vs, ib, (20.0, 25.0), (2.5, 1.0)


def test_restatement_float64_against_long_double():
    import chain_loglik_np as cl
    import hp_likelihood as hl
    stages, vs, ib, vmap, imap = _hand_chain()
    rng = np.random.default_rng(11)
    rec, span = _table(rng, [{0: 6, 1: 1, 2: 1}, {1: 2, 2: 1}, {0: 4, 2: 2}])           # the second condition has no j_ion records
    basis = rng.uniform(-0.3, 0.3, (91, 2))
    n, first = 500, 7
    te = rng.uniform(-1, 1, (2, n))
    a_1 = 10.0 ** rng.uniform(-2.5, -1, n)
    idx = first + np.arange(n)
    for kw in (dict(), dict(a_1=a_1, discharge=(4.5, 0.2))):
        got, m, rows = cl.chain_loglik(stages, te, vs, ib, vmap, imap, rec, span, 3, first=first, basis=basis, **kw)
        want, m_ld, rows_ld = cl.chain_loglik(stages, te, vs, ib, vmap, imap, rec, span, 3, first=first, basis=basis, ld=True, **kw)
        kind, w, y, s, k = cl.sample_tables(rec, span, 3, idx)
        assert np.array_equal(np.isnan(m), kind < 0) and np.array_equal(np.isnan(m_ld), kind < 0)
        dm = cl.model_bound(rows_ld, idx, rec, span, 3, basis)
        hl.assert_within(np.where(kind >= 0, m, 0.0), np.where(kind >= 0, m_ld, hl.LD(0)), dm, 'model values')
        # the float64 sum against the long-double sum of ITS model values, then the model values' own share
        ref, bound = cl.sum_ref(m, kind, y, s, rows[1], kw.get('a_1'), kw.get('discharge'))
        hl.assert_within(got, ref, bound, 'sum of the float64 model values')
        z = (hl._ld(y) - np.where(kind >= 0, m_ld, hl.LD(0))) * hl._ld(s)
        share = 1.01 * np.where(kind >= 0, np.abs(z) * hl._ld(s) * dm, hl.LD(0)).sum(axis=1)
        if kw:
            i_d = np.abs(rows_ld[1] / (1 - 2 * hl._ld(a_1)))
            zd = np.abs((hl.LD(4.5) - i_d) * hl.LD(1 / 0.2))
            share = share + 1.01 * zd * hl.LD(1 / 0.2) * hl.LD(cl.CHAIN_REL) * np.abs(rows_ld[1]).max() / np.abs(1 - 2 * hl._ld(a_1))
        hl.assert_within(got, want, bound + share, 'float64 against long double')
        assert np.all(np.isfinite(got)) and np.all(got < 0)


def test_restatement_marks_what_the_chain_cannot_give():
    import chain_loglik_np as cl
    stages, vs, ib, vmap, imap = _hand_chain()
    rng = np.random.default_rng(12)
    rec, span = _table(rng, [{0: 3, 1: 1}, {1: 1, 3: 2}, {2: 1}])                          # u_ion records in the second condition
    basis = rng.uniform(-0.3, 0.3, (91, 2))
    te = rng.uniform(-1, 1, (2, 30))
    cond = np.arange(30) % 3
    for ld in (False, True):
        ll, _, _ = cl.chain_loglik(stages, te, vs, ib, vmap, imap, rec, span, 3, basis=basis, ld=ld)
        assert np.array_equal(np.isnan(ll), cond == 1)
        ll, m, _ = cl.chain_loglik(stages, te, vs, ib, vmap, imap, rec, span, 3, basis=None, ld=ld)     # j_ion records without a basis
        assert np.array_equal(np.isnan(ll), cond != 2) and np.all(np.isfinite(ll[cond == 2].astype(np.float64)))


# ---- the host input map ------------------------------------------------------------------------------------------------------
OPS = np.array([[1e-5, 300.0, 5e-6], [3e-6, 250.0, 4e-6]])
FIXED = {'Pstar': 3e-5, 'P_T': 2e-5, 'c4': 1e20, 'c5': 1e16, 'sigma_cex': 55e-20, 'c0': 0.5, 'c1': 0.5}
VARIED = ('P_b', 'V_a', 'T_e', 'V_vac', 'mdot_a', 'a_1', 'c2', 'c3')


def test_input_map_equals_external_coords():
    from hallthrusterpem_amd.calibration import surrogate_input_map
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    from hallthrusterpem_amd.sampling import PEM_V0_PRIORS
    from hallthrusterpem_amd.system import PemV0System
    m = surrogate_input_map(('T_e', 'c2'), OPS, VARIED, FIXED, PEM_V0_PRIORS, ('V_cc', 'T', 'jion'))
    assert [COUPLED_INPUTS[r] for r in m.rows] == list(VARIED)
    assert [COUPLED_INPUTS[r] for r in m.fixed_rows] == [k for k in COUPLED_INPUTS if k in FIXED]
    assert np.array_equal(m.fixed_vals, [FIXED[k] for k in COUPLED_INPUTS if k in FIXED])
    rng = np.random.default_rng(3)
    x = np.stack([10.0 ** rng.uniform(p.a, p.b, 257) if p.kind == 1 else rng.uniform(p.a, p.b, 257) for p in PEM_V0_PRIORS.values()])
    want, _ = PemV0System._external_coords(dict(zip(COUPLED_INPUTS, x)), VARIED, PEM_V0_PRIORS)
    assert np.array_equal(m.coords(x), want)
    assert np.abs(m.coords(x)).max() <= 1.0 + 1e-12


@pytest.mark.parametrize('kw, word', [
    (dict(theta=('Pstar',)), 'fixed'),                                         # held fixed by the surrogate
    (dict(theta=('c9',)), 'does not know'),
    (dict(fixed={**FIXED, 'V_a': 300.0}, varied=tuple(k for k in VARIED if k != 'V_a')), '250'),      # another value than a condition's
    (dict(ops=np.array([[1e-5, 300.0, 5e-6], [3e-6, 450.0, 4e-6]])), '450'),                             # outside the box, named
    (dict(ops=np.array([[1e-9, 300.0, 5e-6]])), '1.e-09'),
    (dict(qois=('V_cc', 'uion')), 'u_ion latents'),
    (dict(qois=('jion',), field=False), 'field=False'),
])
def test_input_map_refuses(kw, word):
    from hallthrusterpem_amd.calibration import surrogate_input_map
    from hallthrusterpem_amd.sampling import PEM_V0_PRIORS
    with pytest.raises(ValueError, match=re.escape(word)):
        surrogate_input_map(kw.get('theta', ('T_e',)), kw.get('ops', OPS), kw.get('varied', VARIED), kw.get('fixed', FIXED), PEM_V0_PRIORS,
                            kw.get('qois', ('V_cc',)), field=kw.get('field', True))


# ---- the kernel's resources ----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc is not available')
def test_chain_loglik_kernels_neither_spill_vgprs_nor_use_scratch():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_surrogate.hip'),
                          '--grep', 'chain_loglik_kernel'], capture_output=True, text=True, check=True).stdout
    rows = [line for line in out.splitlines() if line.startswith('chain_loglik_kernel')]
    assert len(rows) == 6, out                                  # plume widths 1, 2, 3, 4 exact; 8, 16 guarded
    for line in rows:
        g = lambda k: int(re.search(k + r'\s+(\d+)', line).group(1))              # noqa: E731
        assert g('v-spill') == 0 and g('scratch') == 0, line
        print(line[:40], 'VGPRs:', g('vgpr'), 'SGPR spills:', g('s-spill'))      # reported, not gated
