"""u_ion through the chained surrogate on the GPU: pem_sparse_predict_chain_fields_f64_dev and pem_chain_fields_loglik_f64_dev against
their parents (bit for bit where include/pem_hip.h says so) and the restatement of tests/chain_uion_np.py over their dispatch space;
`ChainedSurrogate(u_ion=True)` on the thruster test double; `SurrogatePosterior` with all four measured quantities; the round trip
through `PemV0System`."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

NORMS = {1: 1.0, 2: 0.5, 0: 1.0}            # the j_ion map's PEM_NORM_*: its norm_scale (test_surrogate_posterior's)
U_SCALE = {2: 1e-3, 0: 1.0}                 # the u_ion map's: linear(1e-3) (yml:207-214), or none
DISCHARGE = (4.5, 0.2)


def _p(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _case(rng, n, n_plume, outers, rank, u_rank, ncells, slots, big, pad):
    """test_surrogate_posterior._chain_case with a thruster table of 2 + u_rank outputs (latents of O(100), as 1e-3 v_exh sqrt(cells))
    and the same table cut to its first two columns: `arr` / `arr_cut`.  thr: the full thruster table alone at the chain's own
    coordinates (one pem_sparse_predict_f64_dev launch)."""
    import torch
    import test_chained_surrogate as tc
    from hallthrusterpem_amd import _lib
    VCC, IB0 = slots
    ext = [d for d in range(tc.N_DIM) if d not in slots]
    thr = tc._stage(rng, 2 + u_rank, outers[1], ext[:4] + [VCC], big)
    for v in thr[2]:
        v[:, 2:] *= 100.0
    cut = (thr[0], thr[1], [np.ascontiguousarray(v[:, :2]) for v in thr[2]])
    stages = [tc._stage(rng, 1, outers[0], ext, big), thr, tc._stage(rng, n_plume, outers[2], ext[:4] + [IB0], big)]
    tabs = [tc._upload(*s) for s in stages]
    tab_cut = tc._upload(*cut)
    ld = n + pad
    tfull = torch.zeros((tc.N_DIM, ld), dtype=torch.float64, device='cuda')
    tfull[ext, :n] = torch.rand((tc.N_EXT, n), dtype=torch.float64, device='cuda') * 2 - 1
    vcc = tc._single(tabs[0], tfull, n)[0]
    vmap = tc._domain(vcc)
    tfull[VCC, :n] = 2.0 * (vcc - vmap[0]) / torch.tensor(vmap[1], dtype=torch.float64, device='cuda') - 1.0
    thr_rows = tc._single(tabs[1], tfull, n)
    imap = tc._domain(tc._single(tab_cut, tfull, n)[0])
    t = tfull[ext].contiguous()
    mk = lambda tt: (_lib.SurrStage * 3)(*[_lib.SurrStage(a.data_ptr(), b.data_ptr(), c.data_ptr(), nb, no, na, lv)     # noqa: E731
                                           for a, b, c, nb, no, na, lv in tt])
    basis = torch.from_numpy(rng.uniform(-0.3, 0.3, (91, max(rank, 1))) * min(1.0, 4.0 / max(rank, 1))).cuda() if rank else None
    ubasis = torch.from_numpy(rng.uniform(0.0, 0.1, (ncells, u_rank))).cuda()
    return dict(n=n, ld=ld, t=t, arr=mk(tabs), arr_cut=mk([tabs[0], tab_cut, tabs[2]]), keep=(tabs, tab_cut), vmap=vmap, imap=imap,
                slots=slots, n_plume=n_plume, rank=rank, basis=basis, u_rank=u_rank, ncells=ncells, ubasis=ubasis, thr=thr_rows,
                stages=stages)


def _predict(cs, norm, u_norm, u_rank=None, first=0, count=None, want_field=True, want_ufield=True):
    """pem_sparse_predict_chain_fields_f64_dev: (rows padded with NaN columns, j_ion field or None, u_ion field or None)"""
    import torch
    from hallthrusterpem_amd import _lib
    ur = cs['u_rank'] if u_rank is None else u_rank
    n = cs['n'] - first if count is None else count
    out = torch.full((4 + cs['n_plume'] + ur, n + 3), np.nan, dtype=torch.float64, device='cuda')
    f = torch.full((n + 1, 91), np.nan, dtype=torch.float64, device='cuda') if cs['rank'] and want_field else None
    uf = torch.full((n + 1, cs['ncells']), np.nan, dtype=torch.float64, device='cuda') if ur and want_ufield else None
    _lib.check(_lib.load().pem_sparse_predict_chain_fields_f64_dev(
        n, 7, cs['slots'][0], cs['slots'][1], cs['arr'] if ur else cs['arr_cut'], *cs['vmap'], *cs['imap'],
        C.c_void_p(cs['t'].data_ptr() + 8 * first), cs['ld'], _p(out), n + 3, 1, cs['rank'], 91, norm, NORMS[norm], _p(cs['basis']), _p(f),
        2, ur, cs['ncells'], u_norm, U_SCALE[u_norm], _p(cs['ubasis']), _p(uf), None))
    torch.cuda.synchronize()
    return out, f, uf


def _loglik(cs, norm, u_norm, rec, span, n_cond, node, u_rank=None, a_1=None, want_out=True, want_pred=True, first=0, count=None):
    """pem_chain_fields_loglik_f64_dev: (loglik, rows, pred), every array padded with NaN"""
    import torch
    from hallthrusterpem_amd import _lib
    ur = cs['u_rank'] if u_rank is None else u_rank
    n = cs['n'] - first if count is None else count
    n_rec = rec.shape[0]
    rows = -(-n // n_cond)
    ll = torch.full((n + 2,), np.nan, dtype=torch.float64, device='cuda')
    out = torch.full((4 + cs['n_plume'] + ur, n + 3), np.nan, dtype=torch.float64, device='cuda') if want_out else None
    pred = torch.full((rows + 1, n_rec + 5), np.nan, dtype=torch.float64, device='cuda') if want_pred else None
    node_d = torch.from_numpy(node).cuda()
    _lib.check(_lib.load().pem_chain_fields_loglik_f64_dev(
        n, 7, cs['slots'][0], cs['slots'][1], cs['arr'] if ur else cs['arr_cut'], *cs['vmap'], *cs['imap'],
        C.c_void_p(cs['t'].data_ptr() + 8 * first), cs['ld'], 1, cs['rank'], 91, norm, NORMS[norm], _p(cs['basis']), n_cond, n_rec, _p(rec),
        _p(span), C.c_void_p(a_1.data_ptr() + 8 * first) if a_1 is not None else None, DISCHARGE[0], DISCHARGE[1], _p(ll), _p(out), n + 3,
        _p(pred), n_rec + 5, 2, ur, cs['ncells'], u_norm, U_SCALE[u_norm], _p(cs['ubasis']), node.size, _p(node_d),
        node.ctypes.data_as(C.c_void_p), None))
    torch.cuda.synchronize()
    return ll, out, pred


def _staged(cs, n_rec, n_cond, n_node):
    """whether pem_chain_fields_loglik_f64_dev stages its tables beside the coordinates for this case, by the launch's own rule
    (csrc/pem_surrogate_fields.hip chain_fields_loglik): (staged, base bytes, extra bytes)"""
    words = max((na - 1 if na > 1 else 0) * ((1 << lv) + 1 if lv else 1) for *_, na, lv in cs['keep'][0])
    words = max(words, cs['u_rank'], cs['rank'])              # a latent slot per thread for either field
    base = (words + 7) * 256 * 8
    extra = n_rec * 32 + n_cond * 32 + 91 * cs['rank'] * 8 + n_node * cs['u_rank'] * 8
    return base + extra <= (80 if base <= 80 * 1024 else 160) * 1024, base, extra


MIXES = {                                                # {kind: count} per condition, cycled over n_cond; kind 3: u_ion
    'four': [{0: 9, 1: 1, 2: 1, 3: 4}, {1: 1, 2: 2}, {3: 5}, {0: 5}, {0: 3, 2: 1, 3: 2}],
    'scalars': [{1: 1, 3: 3}, {2: 1}, {3: 5, 2: 1}],
    'heavy': [{0: 40, 3: 5}, {0: 7}, {3: 5, 1: 1}],
}
CELLS = {200: [0, 17, 18, 101, 198], 7: [0, 2, 3, 5, 5]}

CASES = [
    # u_rank, n_plume, rank, n_cond, n, mix, outers, slots, big, ncells, j norm, u norm
    (1, 1, 0, 3, 1003, 'scalars', (1, 2, 0), (5, 6), False, 200, 1, 2),        # plume width 1 exact, thruster 3 exact
    (1, 7, 6, 5, 1009, 'four', (2, 3, 1), (5, 6), False, 200, 1, 2),           # the shipped shape: thruster 3 exact, plume 8 guarded
    (2, 3, 2, 5, 1012, 'four', (3, 1, 2), (1, 4), False, 7, 2, 0),             # thruster 4 in the guarded width, 7 cells, no u norm
    (6, 16, 15, 16, 1013, 'heavy', (4, 2, 3), (1, 4), True, 200, 1, 2),        # 150 KB of bases, 22 KB of tables: through the cache
    (14, 8, 3, 4, 777, 'four', (0, 4, 2), (4, 2), False, 7, 0, 2),             # thruster 16, plume 8 exactly full
    (1, 5, 0, 3, 2048 * 256 + 80, 'scalars', (2, 1, 2), (4, 2), False, 7, 1, 2),   # a second grid-stride round
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=lambda c: f'u{c[0]}w{c[1]}r{c[2]}c{c[3]}n{c[4]}{c[5]}z{c[9]}')
def test_kernels_against_parents_and_restatement(case):
    import torch
    import chain_loglik_np as cl
    import chain_uion_np as cu
    import hp_likelihood as hl
    import test_surrogate_posterior as tsp
    from test_chain_uion_host import uion_table
    u_rank, n_plume, rank, n_cond, n, mix, outers, slots, big, ncells, norm, u_norm = case
    assert n % n_cond and n % 256
    torch.manual_seed(n)
    rng = np.random.default_rng(n + u_rank)
    cs = _case(rng, n, n_plume, outers, rank, u_rank, ncells, slots, big, pad=11)
    cut = dict(cs, arr=cs['arr_cut'])
    rec_h, span_h, node = uion_table(rng, [MIXES[mix][c % len(MIXES[mix])] for c in range(n_cond)], CELLS[ncells], ncells)
    rec, span = torch.from_numpy(rec_h).cuda(), torch.from_numpy(span_h).cuda()
    n_rec = rec_h.shape[0]
    # which path the likelihood launch takes, from the case's own numbers: the `big` case alone reads its tables through the cache
    staged, base, extra = _staged(cs, n_rec, n_cond, node.size)
    print(f'LDS: {base} B of bases and coordinates, {extra} B of tables: {"staged" if staged else "through the cache"}')
    assert staged == (not big) and (not big or (base == 75 * 2048 and base + extra > 160 * 1024))
    a_1 = torch.from_numpy(10.0 ** rng.uniform(-2.5, -1.0, n)).cuda()
    sub = np.arange(n) if n < 5000 else np.unique(np.concatenate([np.arange(600), np.linspace(0, n - 1, 600).astype(int), np.arange(n - 600, n)]))
    sub_t = torch.from_numpy(sub).cuda()

    # ---- the predict: contract 2 (the parent on the cut table), the latents' rows, the profile ----
    rows_par, field_par = tsp._chain(cut, norm)
    out, field, ufield = _predict(cs, norm, u_norm)
    assert torch.isnan(out[:, n:]).all() and torch.isfinite(out[:, :n]).all(), 'wrote past n'
    assert torch.equal(out[:4 + n_plume, :n], rows_par[:, :n]), 'the parent rows'
    assert torch.equal(out[1:3, :n], cs['thr'][:2]) and torch.equal(out[4 + n_plume:, :n], cs['thr'][2:]), 'the thruster table alone'
    if rank:
        assert torch.equal(field[:n], field_par) and torch.isnan(field[n:]).all(), 'j_ion field'
    assert torch.isnan(ufield[n:]).all() and torch.isfinite(ufield[:n]).all()
    lat_h = out[4 + n_plume:, sub_t].cpu().numpy()
    ub_h = cs['ubasis'].cpu().numpy()
    want_u = cu.uion_cells(lat_h, ub_h, np.arange(ncells), u_norm, U_SCALE[u_norm])
    uf_h = ufield[sub_t].cpu().numpy()
    assert np.array_equal(uf_h, want_u), 'u_field: fma chain over the latents, then the denormalisation'
    # contract 3: without the fields, and a shifted truncated batch
    assert torch.equal(_predict(cs, norm, u_norm, want_field=False, want_ufield=False)[0][:, :n], out[:, :n])
    first, count = 5 * n_cond, n - 5 * n_cond - 301
    out_s, field_s, ufield_s = _predict(cs, norm, u_norm, first=first, count=count)
    assert torch.equal(out_s[:, :count], out[:, first:first + count]) and torch.equal(ufield_s[:count], ufield[first:first + count])
    assert torch.isnan(ufield_s[count:]).all() and (not rank or torch.equal(field_s[:count], field[first:first + count]))
    # contract 1: u_rank 0 through the new entry point is the parent
    out0, field0, _ = _predict(cs, norm, u_norm, u_rank=0)
    assert torch.equal(out0[:, :n], rows_par[:, :n]) and torch.isnan(out0[:, n:]).all() and (not rank or torch.equal(field0[:n], field_par))

    # ---- the likelihood ----
    ll_par, out_par, pred_par = tsp._loglik(cut, norm, rec, span, n_cond, a_1=a_1)
    ll, out_l, pred = _loglik(cs, norm, u_norm, rec, span, n_cond, node, a_1=a_1)
    assert torch.equal(out_l.isnan(), out.isnan()) and torch.equal(out_l[:, :n], out[:, :n]), 'rows'
    assert torch.isnan(ll[n:]).all() and torch.isfinite(ll[:n]).all()
    kind_c = cl.sample_tables(rec_h, span_h, n_cond, np.arange(n_cond))[0]                  # [n_cond][n_rec]
    has_u = torch.from_numpy((kind_c == cu.UION).any(axis=1)).cuda()[torch.arange(n, device='cuda') % n_cond]
    assert has_u.any() and (~has_u).any()
    assert torch.equal(ll[:n][~has_u], ll_par[:n][~has_u]) and torch.isnan(ll_par[:n][has_u]).all(), 'contract 2: conditions without u_ion'
    # the model values: the parent's bits for its kinds, the interpolated profile for u_ion; nothing else is written
    u_col = torch.from_numpy((kind_c == cu.UION).any(axis=0)).cuda()
    assert torch.equal(pred[:, :n_rec][:, ~u_col].nan_to_num(), pred_par[:, :n_rec][:, ~u_col].nan_to_num())
    assert torch.equal(pred[:, :n_rec][:, ~u_col].isnan(), pred_par[:, :n_rec][:, ~u_col].isnan()) and torch.isnan(pred[:, n_rec:]).all()
    kind, w, y, s, _ = cl.sample_tables(rec_h, span_h, n_cond, sub)
    a, b = cu.uion_nodes(rec_h, node)
    got = pred[torch.from_numpy(sub // n_cond).cuda()][:, :n_rec].cpu().numpy()
    is_u = kind == cu.UION
    assert np.array_equal(got[is_u], hl.interp_model(w, uf_h[:, a], uf_h[:, b])[is_u]), 'u_ion pred'
    assert np.isfinite(got[kind >= 0]).all()
    # the sum: the restated order, bit for bit, and within record_sum's bound of the long-double sum of these model values
    r_h = out[:, sub_t].cpu().numpy()
    a_h = a_1.cpu().numpy()[sub]
    ll_h = cu.ordered_sum(got, kind, y, s, (cu.UION, cu.JION, cu.VCC, cu.T))
    z = (DISCHARGE[0] - r_h[1] / (1.0 - 2.0 * a_h)) * (1.0 / DISCHARGE[1])
    assert np.array_equal(ll[:n].cpu().numpy()[sub], hl.fma(-0.5 * z, z, ll_h)), 'loglik: u_ion, j_ion, V_cc, T, discharge, one fma each'
    ref, bound = cu.sum_ref(got, kind, y, s, r_h[1], a_h, DISCHARGE)
    hl.assert_within(ll[:n].cpu().numpy()[sub], ref, bound, 'loglik')
    ll_nd = _loglik(cs, norm, u_norm, rec, span, n_cond, node)[0]
    assert np.array_equal(ll_nd[:n].cpu().numpy()[sub], ll_h), 'without the discharge term'
    # contract 3: whatever is asked for, and a shifted truncated batch that keeps i mod n_cond
    for wo, wp in ((False, False), (True, False), (False, True)):
        assert torch.equal(_loglik(cs, norm, u_norm, rec, span, n_cond, node, a_1=a_1, want_out=wo, want_pred=wp)[0][:n], ll[:n]), (wo, wp)
    ll_s, out_s, pred_s = _loglik(cs, norm, u_norm, rec, span, n_cond, node, a_1=a_1, first=first, count=count)
    assert torch.equal(ll_s[:count], ll[first:first + count]) and torch.equal(out_s[:, :count], out[:, first:first + count])
    whole = count // n_cond
    assert torch.equal(pred_s[:whole].nan_to_num(), pred[5:5 + whole].nan_to_num())
    # contract 1: u_rank 0 is the parent, NaN exactly where a condition has u_ion records
    ll0, out0, pred0 = _loglik(cs, norm, u_norm, rec, span, n_cond, node, u_rank=0, a_1=a_1)
    assert torch.equal(ll0[:n].isnan(), has_u) and torch.equal(ll0.nan_to_num(), ll_par.nan_to_num()) and torch.equal(ll0.isnan(), ll_par.isnan())
    assert torch.equal(out0.nan_to_num(), out_par.nan_to_num()) and torch.equal(pred0.nan_to_num(), pred_par.nan_to_num())
    assert torch.equal(pred0.isnan(), pred_par.isnan())
    # u_ion records without a node table (n_node 0; the spans are device memory, the host cannot refuse them): NaN exactly on their
    # conditions, the parent's bits on the others
    ll_n = _loglik(cs, norm, u_norm, rec, span, n_cond, node[:0], a_1=a_1)[0]
    assert torch.equal(ll_n[:n].isnan(), has_u) and torch.equal(ll_n[:n][~has_u], ll_par[:n][~has_u]) and torch.isnan(ll_n[n:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('u_rank, n_plume, rank, big', [(1, 7, 6, False), (5, 16, 15, True)], ids=['u1w7', 'u5w16cache'])
def test_a_table_without_uion_records_sums_as_the_parent(u_rank, n_plume, rank, big):
    """chain_fields_epilogue is a hand-kept twin of the parent's chain_loglik_epilogue: on a table that holds no u_ion record the new
    kernels (u_rank > 0) and the parent on the cut thruster table agree in every bit of loglik, pred and the rows"""
    import torch
    import test_surrogate_posterior as tsp
    from test_surrogate_posterior_host import _table
    n, n_cond = 1003, 16 if big else 5
    torch.manual_seed(7)
    rng = np.random.default_rng(7 + u_rank)
    cs = _case(rng, n, n_plume, (4, 1, 3) if big else (2, 3, 1), rank, u_rank, 200, (5, 6), big, pad=3)
    mix = MIXES['heavy'] if big else tsp.MIXES['all']
    rec_h, span_h = _table(rng, [{k: v for k, v in mix[c % len(mix)].items() if k != 3} for c in range(n_cond)])
    assert not span_h[:, 3].any()
    rec, span = torch.from_numpy(rec_h).cuda(), torch.from_numpy(span_h).cuda()
    assert _staged(cs, rec_h.shape[0], n_cond, 0)[0] == (not big)
    a_1 = torch.from_numpy(10.0 ** rng.uniform(-2.5, -1.0, n)).cuda()
    none = np.zeros(0, dtype=np.int32)
    for a in (None, a_1):
        ll_par, out_par, pred_par = tsp._loglik(dict(cs, arr=cs['arr_cut']), 1, rec, span, n_cond, a_1=a)
        ll, out, pred = _loglik(cs, 1, 2, rec, span, n_cond, none, a_1=a)
        assert torch.isfinite(ll[:n]).all() and torch.equal(ll.nan_to_num(), ll_par.nan_to_num()) and torch.equal(ll.isnan(), ll_par.isnan())
        assert torch.equal(pred.nan_to_num(), pred_par.nan_to_num()) and torch.equal(pred.isnan(), pred_par.isnan())
        assert torch.equal(out[:4 + n_plume].nan_to_num(), out_par.nan_to_num()) and torch.isfinite(out[4 + n_plume:, :n]).all()


@pytest.mark.gpu
def test_kernel_against_the_long_double_restatement():
    """the whole launch from the tables in long double (tests/chain_uion_np.py), on a subset: 1e-11 of the rows as
    test_chained_surrogate holds them, and the sums within the bound the host test derives"""
    import torch
    import chain_loglik_np as cl
    import chain_uion_np as cu
    import hp_likelihood as hl
    from test_chain_uion_host import uion_table
    n, n_cond, ncells, u_rank, n_plume = 1001, 5, 200, 2, 4
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    cs = _case(rng, n, n_plume, (1, 2, 2), 3, u_rank, ncells, (5, 6), False, pad=0)
    basis_h, ub_h = cs['basis'].cpu().numpy(), cs['ubasis'].cpu().numpy()
    rec_h, span_h, node = uion_table(rng, [MIXES['four'][c] for c in range(n_cond)], CELLS[ncells], ncells)
    rec, span = torch.from_numpy(rec_h).cuda(), torch.from_numpy(span_h).cuda()
    ll, out, pred = _loglik(cs, 1, 2, rec, span, n_cond, node)
    sub = np.linspace(0, n - 1, 64).astype(int)
    u = dict(basis=ub_h, node=node, norm=2, scale=1e-3)
    rows_ld = cu.compose(cs['stages'], cs['t'][:, sub].cpu().numpy(), 5, 6, cs['vmap'], cs['imap'], ld=True)
    # (sample i of the subset has global index sub[i]: its condition is sub[i] mod n_cond)
    want, m_ld = cu.loglik_from_rows(rows_ld, sub, rec_h, span_h, n_cond, n_plume, u=u, basis=basis_h, ld=True)
    g = out[:, sub].cpu().numpy()
    assert np.all(np.abs(g - rows_ld.astype(np.float64)) <= 1e-11 * np.maximum(np.abs(rows_ld).max(axis=1, keepdims=True), 1.0).astype(np.float64))
    kind, w, y, s, _ = cl.sample_tables(rec_h, span_h, n_cond, sub)
    got_m = pred[torch.from_numpy(sub // n_cond).cuda()][:, :rec_h.shape[0]].cpu().numpy()
    dm = cu.model_bound(rows_ld, sub, rec_h, span_h, n_cond, n_plume, u, basis_h)
    # the kernel's rows are within 1e-11 of the long-double rows where the float64 restatement is within CHAIN_REL = 1e-13: scale the bound
    hl.assert_within(np.where(kind >= 0, got_m, 0.0), np.where(kind >= 0, m_ld, hl.LD(0)), dm * 100, 'model values')
    z = (hl._ld(y) - np.where(kind >= 0, m_ld, hl.LD(0))) * hl._ld(s)
    share = 1.01 * np.where(kind >= 0, np.abs(z) * hl._ld(s) * dm * 100, hl.LD(0)).sum(axis=1)
    ref, bound = cu.sum_ref(got_m, kind, y, s)
    hl.assert_within(ll[:n].cpu().numpy()[sub], want, bound + share, 'loglik against long double')


# ---- a real fit on the thruster test double ----------------------------------------------------------------------------------
VARIED = ('P_b', 'V_a', 'T_e', 'V_vac', 'mdot_a', 'a_1', 'c0', 'c3')
FIXED = {'Pstar': 5e-5, 'P_T': 5e-5, 'c1': 0.3, 'c2': 5.0, 'c4': 1e20, 'c5': 1e16, 'sigma_cex': 55e-20}
NAMES = ('T_e', 'V_vac', 'c0', 'c3')
TRUTH = {'T_e': 3.0, 'V_vac': 30.0, 'c0': 0.35, 'c3': 0.6}
N_REFINE = 48             # where T, whose error is the cathode's V_cc error until then, meets the 1e-3 the project holds it to


@pytest.fixture(scope='module')
def fit():
    import torch
    from hallthrusterpem_amd.calibration import OPERATING
    from hallthrusterpem_amd.chain import ChainedSurrogate
    from hallthrusterpem_amd.likelihood import UION_GRID, SystemLikelihood
    from hallthrusterpem_amd.models.coupled import pem_v0_coupled
    from hallthrusterpem_amd.models.thruster import thruster_analytic
    s = ChainedSurrogate(VARIED, FIXED, max_level=3, u_ion=True)
    for it in range(N_REFINE):
        s.refine_step(num_refine=500, seed=it)
    rng = np.random.default_rng(8)
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)   # noqa: E731
    alpha = np.linspace(-1.5, 1.5, 14)
    zloc = np.array([0.0, 0.0123, 0.031, 0.0402, 0.0555, 0.08])
    grid = np.linspace(0, np.pi / 2, 91)

    def model(o):
        x = {k: np.full(o.shape[0], v) for k, v in {**FIXED, **TRUTH, 'a_1': 0.02}.items()}
        x.update({k: o[:, j] for j, k in enumerate(OPERATING)})
        out = pem_v0_coupled(x)
        th = thruster_analytic({'V_a': x['V_a'], 'V_cc': out['V_cc'], 'mdot_a': x['mdot_a'], 'a_1': x['a_1']}, num_cells=UION_GRID[2],
                               domain=UION_GRID[:2])
        return out, th
    ops = {'V_cc': op(3), 'T': op(2), 'uion': op(2), 'jion': op(3)}
    data = {}
    out, _ = model(ops['V_cc'])
    data['V_cc'] = {'x': ops['V_cc'], 'y': np.asarray(out['V_cc']), 'var_y': np.full(3, 0.5 ** 2)}
    _, th = model(ops['T'])
    data['T'] = {'x': ops['T'], 'y': np.asarray(th['T']), 'var_y': (0.05 * np.asarray(th['T'])) ** 2}
    _, th = model(ops['uion'])
    u = np.stack([np.interp(zloc, np.asarray(th['u_ion_coords']), np.asarray(th['u_ion'])[e]) for e in range(2)])
    data['uion'] = {'x': ops['uion'], 'y': u, 'var_y': (0.05 * u + 100.0) ** 2, 'loc': zloc}
    out, _ = model(ops['jion'])
    j = np.stack([np.interp(np.abs(alpha), grid, np.asarray(out['j_ion'])[e]) for e in range(3)])
    data['jion'] = {'x': ops['jion'], 'y': j, 'var_y': (0.2 * j + 1e-3) ** 2, 'loc': np.stack([np.ones(alpha.size), alpha], 1)}
    torch.cuda.synchronize()
    return s, SystemLikelihood(data)


@pytest.mark.gpu
def test_fitted_uion_meets_the_reconstruction_tolerance(fit):
    """500 held-out seeded points of the chain's box: the predicted profile against the thruster test double at the TRUE cathode
    coupling voltage, relative L2 <= 0.01 (yml:207-214 reconstruction_tol; DESIGN.md section 4.7.2 records the value)."""
    import torch
    from hallthrusterpem_amd.chain import COMPONENT_INPUTS, box_points
    from hallthrusterpem_amd.models.cathode import cathode_coupling
    from hallthrusterpem_amd.models.thruster import thruster_analytic
    from hallthrusterpem_amd.system import PemV0System
    s, _ = fit
    assert s.u_compression.rank == 1 and s.stages[1].n_out == 3                            # u_ion(z) = v_exh s(z): exactly rank 1
    assert s.u_compression.norm == 2 and s.u_compression.scale == 1e-3 and s.uion_grid == (0.0, 0.08, 200)
    x = box_points(s.varied, s.fixed, s.priors, {}, 500, seed=123)
    t, _ = PemV0System._external_coords(x, s.varied, s.priors)
    y = s.predict_fields(torch.from_numpy(t))
    dev = lambda keys: {k: torch.as_tensor(x[k], device='cuda') for k in keys}             # noqa: E731
    vcc = cathode_coupling(dev(COMPONENT_INPUTS[0]))['V_cc']
    xin = dev(('V_a', 'mdot_a', 'a_1'))
    xin['V_cc'] = vcc
    true = thruster_analytic(xin, num_cells=200)
    err = {k: float(torch.linalg.norm(y[k] - true[k]) / torch.linalg.norm(true[k])) for k in ('u_ion', 'T', 'I_B0')}
    print('relative L2 after', N_REFINE, 'refinements:', err, 'evaluations', s.model_evals)
    assert y['u_ion'].shape == (500, 200) and y['u_ion_latent'].shape == (500, 1)
    assert torch.equal(y['u_ion_coords'], true['u_ion_coords'])
    assert err['u_ion'] <= 0.01
    # the latents (O(100)) do not starve the scalars of the same stage: T meets the 1e-3 the project holds it to (the issue's figure);
    # I_B0 is linear in mdot_a and free of V_cc, its interpolant is exact: rounding only
    assert err['T'] <= 1e-3 and err['I_B0'] <= 1e-12
    # the profile is the reconstruction of the latents' row (pem_svd_reconstruct_f64_dev), to the last few ulp
    again = s.u_compression.reconstruct(y['u_ion_latent'].contiguous())
    assert torch.all((again - y['u_ion']).abs() <= 4 * 2.0 ** -52 * y['u_ion'].abs())
    # the same chain without the option keeps the parent's launch, and its state round-trips
    from hallthrusterpem_amd.chain import ChainedSurrogate
    s2 = ChainedSurrogate.from_state(s.state(), priors=s.priors)
    y2 = s2.predict_fields(torch.from_numpy(t))
    assert all(torch.equal(y2[k], y[k]) for k in y) and s2.u_compression.norm == 2 and s2.compression.norm == 1
    assert s2.model_evals == s.model_evals and s.model_evals[1] >= 1000                   # the 500 domain + 500 compression evaluations count


def _thetas(K, seed):
    import torch
    from hallthrusterpem_amd.sampling import PEM_V0_PRIORS
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([rng.uniform(PEM_V0_PRIORS[k].a, PEM_V0_PRIORS[k].b, K) for k in NAMES], axis=1)).cuda()


@pytest.mark.gpu
def test_surrogate_posterior_with_all_four_quantities(fit):
    import torch
    import hp_likelihood as hl
    from hallthrusterpem_amd.calibration import DRAM, Metropolis, SurrogatePosterior
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    s, lik = fit
    assert lik.qois == ('V_cc', 'T', 'uion', 'jion') and lik.component == 'System' and lik.n_node == 12
    K, M = 4, 5
    post = SurrogatePosterior(NAMES, lik, s, n_chains=K, n_nuisance=M, seed=2, fresh_nuisance=False)
    theta = _thetas(K, 6)
    got = post.record_predictions(theta)
    # the u_ion records: linear interpolation of predict_fields' profile between the kernel's grid doubles
    y = s.predict_fields(post.coords)
    uf = y['u_ion'].cpu().numpy().reshape(K * M, lik.n_cond, -1)
    rec, span, node = lik.rec.cpu().numpy(), lik.span.cpu().numpy(), lik.node_host
    n_u = 0
    for c in range(lik.n_cond):
        f, cnt = span[c, 3]
        for r in range(f, f + cnt):
            p = int(np.ascontiguousarray(rec[r, 3:4]).view(np.int64)[0])
            lo, hi = uf[:, c, node[p]], uf[:, c, node[p + 1]]
            want = hl._ld(lo) + hl._ld(rec[r, 0]) * (hl._ld(hi) - hl._ld(lo))
            hl.assert_within(got[:, r].cpu().numpy(), want, hl.model_error(np.full(K * M, rec[r, 0]), lo, hi), f'u_ion record {r}')
            n_u += 1
    assert n_u == 12
    valid = ~torch.isnan(lik.rec[:, 1]) & (lik.rec[:, 2] != 0)
    assert torch.isfinite(got[:, valid]).all() and torch.isnan(got[:, ~valid]).all()
    # the data came from the model the surrogate stands for: at the truth its u_ion predictions are within the fit's error of them
    truth = torch.tensor([[TRUTH[k] for k in NAMES]] * K, dtype=torch.float64, device='cuda')
    at = post.record_predictions(truth)
    ucol = np.concatenate([np.arange(span[c, 3, 0], span[c, 3, 0] + span[c, 3, 1]) for c in range(lik.n_cond)]).astype(np.int64)
    yu = lik.rec[:, 1][torch.from_numpy(ucol).cuda()]
    assert torch.all((at[:, torch.from_numpy(ucol).cuda()] - yu).abs() <= 0.05 * yu.abs().max())
    # finite, and one graph replay equals the eager evaluation
    post = SurrogatePosterior(NAMES, lik, s, n_chains=K, n_nuisance=M, seed=1)
    replay = post.capture()
    val = replay(theta).clone()
    fresh, post.fresh = post.fresh, False
    eager = post.log_posterior(theta)
    post.fresh = fresh
    assert torch.isfinite(val).all() and torch.equal(val, eager)
    # the same launch on the data without the ion velocities, one point of the box under every condition: the conditions both tables
    # hold sum to the same bits, and the u_ion conditions' sums are their records' alone (finite, below zero)
    few = SystemLikelihood({k: v for k, v in lik.data.items() if k != 'uion'})
    assert few.qois == ('V_cc', 'T', 'jion') and few.n_cond == lik.n_cond - 2
    point = post.coords[:, :1].clone()
    ll_all = s.run_system_loglik(point.expand(-1, lik.n_cond).contiguous(), lik)
    ll_few = s.run_system_loglik(point.expand(-1, few.n_cond).contiguous(), few)
    is_u = torch.from_numpy(span[:, 3, 1] > 0).cuda()
    assert int(is_u.sum()) == 2 and torch.equal(ll_all[~is_u], ll_few)
    assert torch.isfinite(ll_all[is_u]).all() and (ll_all[is_u] < 0).all()
    # the samplers take it unchanged
    post = SurrogatePosterior(NAMES, lik, s, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False, shared_nuisance=True)
    mh = Metropolis(post, [TRUTH[k] for k in NAMES], scale=[0.02, 0.3, 0.01, 0.01], seed=3, use_graph=True)
    trace = mh.run(20)
    assert torch.isfinite(trace).all() and torch.isfinite(mh.logp).all()
    dram = DRAM(post.log_posterior, [TRUTH[k] for k in NAMES], cov0=np.diag([0.02, 0.3, 0.01, 0.01]) ** 2, n_chains=K, seed=2, adapt_after=10,
                adapt_interval=5, device=post.device, use_graph=True)
    trace = dram.run(20)
    torch.cuda.synchronize()
    assert torch.isfinite(trace).all() and torch.isfinite(dram.logp).all()


@pytest.mark.gpu
def test_likelihood_on_another_grid_is_refused(fit):
    import torch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    s, lik = fit
    other = SystemLikelihood({'uion': lik.data['uion']}, uion_grid=(0.0, 0.08, 150))
    t = torch.zeros((s.n_ext, other.n_cond), dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match='grid'):
        s.run_system_loglik(t, other)
    same = SystemLikelihood({'uion': lik.data['uion']})
    assert torch.isfinite(s.run_system_loglik(t, same)).all()


@pytest.mark.gpu
def test_system_round_trip(tmp_path):
    import torch
    from hallthrusterpem_amd.chain import ChainedSurrogate
    from hallthrusterpem_amd.system import PemV0System
    system = PemV0System(seed=2)
    hist = system.fit(targets=['V_cc', 'T_c', 'u_ion'], fixed=FIXED, max_iter=6, max_tol=0.0, num_refine=300, components=True)
    s = system.surrogate
    assert isinstance(s, ChainedSurrogate) and s.u_compression is not None and s.field is None and len(hist) == 6
    xt = system.sample_inputs(300, normalize=False)
    xt.update({k: np.full(300, v) for k, v in FIXED.items()})
    pred = system.predict(xt, normalized_inputs=False)
    assert pred['u_ion'].shape == (300, 200) and pred['u_ion_coords'].shape == (300,) and pred['u_ion_coords'][7].shape == (200,)
    assert np.isfinite(pred['u_ion']).all() and 'j_ion' not in pred
    assert set(system.predict(xt, normalized_inputs=False, targets=['u_ion'])) == {'u_ion', 'u_ion_coords'}
    again = PemV0System.load_from_file(system.save_to_file('uion.pkl', save_dir=tmp_path))
    p2 = again.predict(xt, normalized_inputs=False)
    assert set(p2) == set(pred) and all(np.array_equal(p2[k], pred[k]) for k in pred if not k.endswith('_coords'))
    assert np.array_equal(p2['u_ion_coords'][0], pred['u_ion_coords'][0])
    assert again.surrogate.u_compression.scale == 1e-3 and again.surrogate.u_compression.norm == 2
    # default targets: no u_ion, the parent's launch
    system.fit(fixed=FIXED, max_iter=1, max_tol=0.0, num_refine=200, components=True)
    assert system.surrogate.u_compression is None and 'u_ion' not in system.predict(xt, normalized_inputs=False)
    torch.cuda.synchronize()
