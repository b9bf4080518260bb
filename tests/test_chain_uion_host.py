"""u_ion through the chained surrogate, without a GPU: the two entry points of csrc/pem_surrogate_fields.hip are declared and bound
and refuse every malformed call before they look for a device; tests/chain_uion_np.py restates them in float64 and long double and IS
tests/chain_loglik_np.py at u_rank 0; `surrogate_input_map(..., uion=True)` accepts u_ion records; no instantiation of the new
kernels spills a vector register."""
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
PREDICT, LOGLIK = 'pem_sparse_predict_chain_fields_f64_dev', 'pem_chain_fields_loglik_f64_dev'


def test_symbols_are_declared_and_bound():
    from hallthrusterpem_amd import _lib
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    for name, n_args in ((PREDICT, 28), (LOGLIK, 39)):
        assert re.search(r'\bint\s+%s\s*\(' % name, header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(_lib.load(), name)


def _stages(outs, null_table=None):
    from hallthrusterpem_amd import _lib
    arr = (_lib.SurrStage * 3)()
    for k in range(3):
        ptrs = [4096] * 3                       # never dereferenced: every check below runs on the host
        if null_table == k:
            ptrs[k % 3] = None
        arr[k] = _lib.SurrStage(ptrs[0], ptrs[1], ptrs[2], 3, outs[k], 5, 4)
    return arr


def _u_args(kw):
    u_rank = kw.get('u_rank', 2)
    return dict(u_lat0=kw.get('u_lat0', 2), u_rank=u_rank, u_dof=kw.get('u_dof', 200), u_norm=kw.get('u_norm', 2), u_scale=kw.get('u_scale', 1e-3),
                u_basis=C.c_void_p(4096) if kw.get('u_basis', True) else None, outs=kw.get('outs', (1, 2 + max(u_rank, 0), 3)))


def _predict(n=1000, u_field=True, stages=True, **kw):
    from hallthrusterpem_amd import _lib
    fake = C.c_void_p(4096)
    u = _u_args(kw)
    return _lib.load().pem_sparse_predict_chain_fields_f64_dev(
        n, 4, 2, 3, _stages(u['outs']) if stages else None, 0.0, 1.0, 0.0, 1.0, fake, 1000, fake, 1000, 1, 2, 91, 1, 1.0, fake, fake,
        u['u_lat0'], u['u_rank'], u['u_dof'], u['u_norm'], u['u_scale'], u['u_basis'], fake if u_field else None, None)


def _loglik(n=1000, n_node=6, node=(0, 1, 7, 8, 198, 199), node_dev=True, node_host=True, stages=True, n_dim=4, **kw):
    from hallthrusterpem_amd import _lib
    fake = C.c_void_p(4096)
    u = _u_args(kw)
    host = np.asarray(node, dtype=np.int32)
    return _lib.load().pem_chain_fields_loglik_f64_dev(
        n, n_dim, 2, 3, _stages(u['outs']) if stages else None, 0.0, 1.0, 0.0, 1.0, fake, 1000, 1, 2, 91, 1, 1.0, fake, 3, 9, fake, fake, None,
        4.5, 0.2, fake, None, 0, None, 0, u['u_lat0'], u['u_rank'], u['u_dof'], u['u_norm'], u['u_scale'], u['u_basis'], n_node,
        fake if node_dev else None, host.ctypes.data_as(C.c_void_p) if node_host else None, None)


BOTH = [
    dict(u_basis=False),                                     # NULL basis with u_rank > 0
    dict(u_dof=1), dict(u_dof=0),
    dict(outs=(1, 2, 3)), dict(outs=(1, 5, 3)), dict(u_rank=14, outs=(1, 15, 3)),        # u_rank + 2 != stages[1].n_out
    dict(u_rank=15, outs=(1, 16, 3)), dict(u_rank=-1),
    dict(u_lat0=1), dict(u_norm=5),
    dict(u_scale=0.0), dict(u_scale=float('nan')), dict(u_scale=float('inf')),          # the linear norm divides every node value by it
    dict(stages=False), dict(u_rank=0, outs=(1, 3, 3)),       # u_rank 0: the parent's rule, a thruster stage of exactly two outputs
]
LOGLIK_ONLY = [
    dict(node=(0, 1, 7, 200, 198, 199)), dict(node=(0, 1, -1, 8, 198, 199)), dict(node=(0, 1, 2, 3, 4, 7), u_dof=7),   # outside [0, u_dof)
    dict(n_node=2049, node=tuple(range(200)) * 11), dict(n_node=-1),
    dict(n_node=1),                                          # a u_ion record reads two entries
    dict(node_dev=False), dict(node_host=False),
    dict(n_dim=13, outs=(1, 4, 3)),                          # the parent's LDS rule holds here too
]


@pytest.mark.parametrize('bad', BOTH)
def test_both_entry_points_refuse_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    for call in (_predict, _loglik):
        assert call(**bad) == _lib.PEM_ERR_INVALID_ARG, (call.__name__, bad)


@pytest.mark.parametrize('bad', LOGLIK_ONLY)
def test_the_likelihood_refuses_its_node_table_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _loglik(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_chain_fields_loglik' in _lib.load().pem_last_error()


def test_well_formed_calls_need_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    for kw in (dict(), dict(u_rank=1), dict(u_rank=14), dict(u_rank=0), dict(u_rank=0, u_basis=False, u_dof=0, u_norm=9, u_lat0=0)):
        assert _predict(**kw) == _lib.PEM_ERR_NO_DEVICE, kw
        assert _loglik(**kw) == _lib.PEM_ERR_NO_DEVICE, kw
    assert _predict(u_field=False) == _lib.PEM_ERR_NO_DEVICE                               # the latents' rows alone
    assert _predict(u_norm=0, u_scale=0.0) == _lib.PEM_ERR_NO_DEVICE and _loglik(u_norm=1, u_scale=0.0) == _lib.PEM_ERR_NO_DEVICE   # not read
    assert _predict(u_scale=-2.0) == _lib.PEM_ERR_NO_DEVICE
    assert _loglik(n_node=0, node_dev=False, node_host=False) == _lib.PEM_ERR_NO_DEVICE    # a table without u_ion records
    assert _loglik(n_node=2048, node=tuple(range(200)) * 11) == _lib.PEM_ERR_NO_DEVICE
    assert _predict(n=0) == _lib.PEM_OK and _loglik(n=0) == _lib.PEM_OK


# ---- the restatement on a hand-built chain whose stages interpolate low-degree polynomials exactly ---------------------------
def _hand_chain(u_rank):
    from test_chained_surrogate_host import _tensor_stage
    n_dim, vs, ib = 4, 2, 3
    vcc_f = lambda t: 30.0 + 5.0 * t[0] + 2.0 * t[0] * t[1] + 3.0 * t[1] ** 2          # noqa: E731
    ib0_f = lambda t: 3.0 + 0.1 * t[2] + 0.05 * t[0] * t[2]                               # noqa: E731
    thr_f = lambda t: 0.08 + 0.01 * t[2] ** 2                                             # noqa: E731
    lat_f = [lambda t, q=q: (150.0 - 40.0 * q) + (12.0 + q) * t[2] - 3.0 * t[0] * t[2] ** 2 for q in range(u_rank)]      # O(100), as v_exh 1e-3 sqrt(200)
    div_f = lambda t: 0.3 + 0.05 * t[3] - 0.02 * t[1] * t[3] ** 3                         # noqa: E731
    la_f = lambda t: -1.5 + 0.25 * t[3] ** 2 * t[1]                                       # noqa: E731
    lb_f = lambda t: 0.4 - 0.3 * t[3] + 0.1 * t[1]                                        # noqa: E731
    stages = [_tensor_stage(n_dim, {0: 1, 1: 2}, [vcc_f]), _tensor_stage(n_dim, {0: 1, 2: 2}, [ib0_f, thr_f] + lat_f),
              _tensor_stage(n_dim, {1: 1, 3: 2}, [div_f, la_f, lb_f])]
    return stages, vs, ib, (20.0, 25.0), (2.5, 1.0)


def uion_table(rng, conds, cells, ncells):
    """test_surrogate_posterior_host._table with real u_ion records: `cells` the left grid cell of every measured position (one list
    for the whole table, as likelihood.SystemLikelihood shares `loc` among a dataset's conditions); u_ion record j of a condition
    reads node[2 j], node[2 j + 1].  Returns (rec, span, node)."""
    from test_surrogate_posterior_host import _table
    rec, span = _table(rng, conds)
    node = np.array([v for k in cells for v in (k, k + 1)], dtype=np.int32)
    assert node.max() < ncells
    for c in range(len(conds)):
        f, m = span[c, 3]
        assert m <= len(cells)
        rec[f:f + m, 1] = rng.uniform(5e3, 2e4, m)                # m/s
        rec[f:f + m, 2] = rng.uniform(1e-3, 5e-3, m)              # 1 / std
        rec[f:f + m, 3] = (2 * np.arange(m, dtype=np.int64)).view(np.float64)
    return rec, span, node


@pytest.mark.parametrize('u_rank, norm, scale', [(1, 2, 1e-3), (3, 2, 1e-3), (2, 0, 1.0), (2, 1, 1.0)])
def test_restatement_float64_against_long_double(u_rank, norm, scale):
    import chain_loglik_np as cl
    import chain_uion_np as cu
    import hp_likelihood as hl
    stages, vs, ib, vmap, imap = _hand_chain(u_rank)
    rng = np.random.default_rng(20 + u_rank)
    ncells = 23
    conds = [{0: 6, 1: 1, 2: 1, 3: 4}, {1: 2, 2: 1}, {3: 5}, {0: 4, 2: 2}]            # conditions 1 and 3 have no u_ion records
    rec, span, node = uion_table(rng, conds, [0, 3, 4, 11, 21], ncells)
    basis = rng.uniform(-0.3, 0.3, (91, 2))
    ub = rng.uniform(0.0, 0.1, (ncells, u_rank)) * (0.02 if norm == 1 else 1.0)       # (10^v of an O(100) latent stays finite)
    u = dict(basis=ub, node=node, norm=norm, scale=scale)
    n, first, nc = 400, 8, len(conds)
    te = rng.uniform(-1, 1, (2, n))
    a_1 = 10.0 ** rng.uniform(-2.5, -1, n)
    idx = first + np.arange(n)
    for kw in (dict(), dict(a_1=a_1, discharge=(4.5, 0.2))):
        got, m, rows = cu.chain_loglik(stages, te, vs, ib, vmap, imap, rec, span, nc, first=first, basis=basis, u=u, **kw)
        want, m_ld, rows_ld = cu.chain_loglik(stages, te, vs, ib, vmap, imap, rec, span, nc, first=first, basis=basis, u=u, ld=True, **kw)
        assert rows.shape[0] == 4 + 3 + u_rank
        kind, w, y, s, k = cl.sample_tables(rec, span, nc, idx)
        assert np.array_equal(np.isnan(m), kind < 0) and np.array_equal(np.isnan(m_ld), kind < 0)
        assert (kind == cu.UION).any() and np.all(np.isfinite(got))
        dm = cu.model_bound(rows_ld, idx, rec, span, nc, 3, u, basis)
        hl.assert_within(np.where(kind >= 0, m, 0.0), np.where(kind >= 0, m_ld, hl.LD(0)), dm, 'model values')
        ref, bound = cu.sum_ref(m, kind, y, s, rows[1], kw.get('a_1'), kw.get('discharge'))
        hl.assert_within(got, ref, bound, 'sum of the float64 model values')
        z = (hl._ld(y) - np.where(kind >= 0, m_ld, hl.LD(0))) * hl._ld(s)
        share = 1.01 * np.where(kind >= 0, np.abs(z) * hl._ld(s) * dm, hl.LD(0)).sum(axis=1)
        if kw:
            i_d = np.abs(rows_ld[1] / (1 - 2 * hl._ld(a_1)))
            zd = np.abs((hl.LD(4.5) - i_d) * hl.LD(1 / 0.2))
            share = share + 1.01 * zd * hl.LD(1 / 0.2) * hl.LD(cl.CHAIN_REL) * np.abs(rows_ld[1]).max() / np.abs(1 - 2 * hl._ld(a_1))
        hl.assert_within(got, want, bound + share, 'float64 against long double')
        # bit contract 2 in the restatement: a condition without u_ion records sums as the parent does on the cut thruster table
        cut = [stages[0], (stages[1][0], stages[1][1], {b: v[:, :2] for b, v in stages[1][2].items()}), stages[2]]
        par, m_par, rows_par = cl.chain_loglik(cut, te, vs, ib, vmap, imap, rec, span, nc, first=first, basis=basis, **kw)
        no_u = ~(kind == cu.UION).any(axis=1)
        assert np.array_equal(rows[:7], rows_par) and np.array_equal(got[no_u], par[no_u]) and np.all(np.isnan(par[~no_u]))
        assert np.array_equal(m[no_u], m_par[no_u], equal_nan=True)


def test_restatement_is_the_parents_at_rank_zero():
    import chain_loglik_np as cl
    import chain_uion_np as cu
    from test_surrogate_posterior_host import _hand_chain as parent_chain, _table
    stages, vs, ib, vmap, imap = parent_chain()
    rng = np.random.default_rng(12)
    rec, span = _table(rng, [{0: 3, 1: 1}, {1: 1, 3: 2}, {2: 1}])                          # u_ion records in the second condition
    basis = rng.uniform(-0.3, 0.3, (91, 2))
    te = rng.uniform(-1, 1, (2, 60))
    a_1 = 10.0 ** rng.uniform(-2.5, -1, 60)
    for ld in (False, True):
        for kw in (dict(), dict(a_1=a_1, discharge=(4.5, 0.2))):
            got = cu.chain_loglik(stages, te, vs, ib, vmap, imap, rec, span, 3, first=4, basis=basis, ld=ld, u=None, **kw)
            want = cl.chain_loglik(stages, te, vs, ib, vmap, imap, rec, span, 3, first=4, basis=basis, ld=ld, **kw)
            for g, w in zip(got, want):
                assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True)
            assert np.array_equal(np.isnan(got[0].astype(np.float64)), (4 + np.arange(60)) % 3 == 1)


# ---- the host input map ------------------------------------------------------------------------------------------------------
def test_input_map_accepts_uion_records_when_the_chain_carries_them():
    from hallthrusterpem_amd.calibration import SurrogateInputMap, surrogate_input_map
    from hallthrusterpem_amd.sampling import PEM_V0_PRIORS
    from test_surrogate_posterior_host import FIXED, OPS, VARIED
    m = surrogate_input_map(('T_e',), OPS, VARIED, FIXED, PEM_V0_PRIORS, ('V_cc', 'uion'), uion=True)
    ref = surrogate_input_map(('T_e',), OPS, VARIED, FIXED, PEM_V0_PRIORS, ('V_cc',))
    assert isinstance(m, SurrogateInputMap) and np.array_equal(m.rows, ref.rows) and np.array_equal(m.fixed_vals, ref.fixed_vals)
    with pytest.raises(ValueError, match='u_ion latents'):
        surrogate_input_map(('T_e',), OPS, VARIED, FIXED, PEM_V0_PRIORS, ('V_cc', 'uion'), uion=False)
    with pytest.raises(ValueError, match='field=False'):                                  # the other refusals are untouched
        surrogate_input_map(('T_e',), OPS, VARIED, FIXED, PEM_V0_PRIORS, ('jion', 'uion'), field=False, uion=True)


# ---- the kernels' resources --------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc is not available')
def test_fields_kernels_neither_spill_vgprs_nor_use_scratch():
    src = ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_surrogate_fields.hip'
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(src)], capture_output=True, text=True, check=True).stdout
    rows = [line for line in out.splitlines() if line.startswith('fields_chain')]
    # thruster widths 3 exact, 16 guarded x plume widths 1 exact, 8, 16 guarded, for the predict and for the likelihood; nothing else
    assert len(rows) == 12 and sum(line.startswith('fields_chain_loglik_kernel') for line in rows) == 6, out
    assert not [line for line in out.splitlines() if re.match(r'(sparse_|chain_loglik)', line)], 'the included unit instantiated a kernel of its own'
    for line in rows:
        g = lambda k: int(re.search(k + r'\s+(\d+)', line).group(1))              # noqa: E731
        assert g('v-spill') == 0 and g('scratch') == 0, line
        print(line[:60], 'VGPRs:', g('vgpr'), 'SGPR spills:', g('s-spill'))      # reported, not gated
