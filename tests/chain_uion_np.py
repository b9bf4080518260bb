"""numpy / long-double restatements of pem_sparse_predict_chain_fields_f64_dev and pem_chain_fields_loglik_f64_dev
(csrc/pem_surrogate_fields.hip): tests/chain_np.py's component chain with a thruster stage of 2 + u_rank outputs, then the sums of
tests/chain_loglik_np.py with the u_ion records served.  TEST INFRASTRUCTURE.

Rows of the launch: V_cc, I_B0, T, div_angle, T_c, p_1 .. p_{n_plume-1}, then the thruster's latents l_0 .. l_{u_rank-1} (rows
4 + n_plume + q).  Per sample i (condition c = i mod n_cond):
    u[c]   = denorm(v), v = 0; v = fma(l_q, u_basis[c][q], v) for q = 0 .. u_rank - 1; denorm: 10^v | v / scale | v
    m_r    = fma(w, u[b] - u[a], u[a]), a = node[p], b = node[p + 1], p = min(bits, n_node - 2)     (PEM_SYS_UION)
    loglik = the terms in the order u_ion, j_ion, V_cc, T (each kind in record order), every one added by one fma(-0.5 z, z, sum)
             from 0, then the discharge term -- chain_loglik_np's sum with the u_ion terms in front.
With u_rank = 0 everything here IS chain_loglik_np (the functions are called, nothing is restated).

Bounds (u = 2^-53, as tests/chain_loglik_np.py and tests/hp_likelihood.py):
  * the record sum given the model values: one fma per record and lane; with n records of all four kinds a term passes through at
    most n additions and z^2 carries 4 roundings: hp_likelihood.record_sum's n + 6 as it is, n + 7 with the discharge term.
  * the u_ion model values of the float64 restatement against the long-double one: chain_loglik_np.model_bound's j_ion derivation
    with the other norm -- a latent error d moves v by at most sum_q |u_basis[c][q]| d, plus gamma_rank sum_q |l_q u_basis[c][q]| of the
    fma chain; the linear denormalisation v / scale is ONE more division: |du| <= |dv| / |scale| + u |u|; the interpolation adds
    u (|w| |hi - lo| + |m|) and at most |du_lo| + 2 |w| max |du|.
"""
import numpy as np

import chain_loglik_np as cl
import chain_np
import hp_likelihood as hl

LD, U = hl.LD, hl.U
JION, VCC, T, UION = cl.JION, cl.VCC, cl.T, cl.UION
NORM_NONE, NORM_LOG10, NORM_LINEAR = cl.NORM_NONE, cl.NORM_LOG10, cl.NORM_LINEAR


def compose(stages, t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map, ld=False):
    """chain_np.compose / compose_ld for a thruster stage of 2 + u_rank outputs: its rows, then the latents' rows"""
    from oracle import surrogate_np as snp
    import hp_reference as hp
    ft = LD if ld else np.float64
    pred = (lambda s, t: hp.predict_ref(*s, t)[0]) if ld else (lambda s, t: snp.predict(*s, t))
    n_dim = t_ext.shape[0] + 2
    t = np.zeros((n_dim, t_ext.shape[1]), dtype=ft)
    t[[d for d in range(n_dim) if d not in (vcc_slot, ib0_slot)]] = np.asarray(t_ext, dtype=np.float64).astype(ft)
    vcc = pred(stages[0], t)[0]
    t[vcc_slot] = chain_np.coupling_coord(vcc, ft(vcc_map[0]), ft(vcc_map[1]))
    thr = pred(stages[1], t)
    t[ib0_slot] = chain_np.coupling_coord(thr[0], ft(ib0_map[0]), ft(ib0_map[1]))
    plu = pred(stages[2], t)
    return np.concatenate([np.stack([vcc, thr[0], thr[1], plu[0], thr[1] * np.cos(plu[0])]), plu[1:], thr[2:]])


def uion_cells(lat, ubasis, cells, norm=NORM_LINEAR, scale=1e-3, ld=False):
    """u[c] of every sample: lat [u_rank][n] the latents' rows, ubasis [dof][u_rank], cells [n][m] or [m] cell indices -> [n][m]"""
    cells = np.asarray(cells, dtype=np.int64)
    n = np.asarray(lat[0]).shape[0]
    cells = np.broadcast_to(cells, (n,) + cells.shape[-1:])
    if ld:
        v = np.zeros(cells.shape, dtype=LD)
        for q in range(ubasis.shape[1]):
            v = v + np.asarray(lat[q], dtype=LD)[:, None] * ubasis[cells, q].astype(LD)
        return LD(10) ** v if norm == NORM_LOG10 else (v / LD(scale) if norm == NORM_LINEAR else v)
    v = np.zeros(cells.shape)
    for q in range(ubasis.shape[1]):
        v = hl.fma(np.broadcast_to(np.asarray(lat[q], dtype=np.float64)[:, None], cells.shape), ubasis[cells, q], v)
    return 10.0 ** v if norm == NORM_LOG10 else (v / scale if norm == NORM_LINEAR else v)


def uion_nodes(rec, node):
    """(a, b) [n_rec]: the grid cells every record would read as a u_ion record, p clamped as the kernel clamps it"""
    node = np.asarray(node, dtype=np.int64)
    bits = np.ascontiguousarray(np.asarray(rec, dtype=np.float64)[:, 3]).view(np.int64).astype(np.uint64)
    p = np.minimum(bits.astype(np.uint32), max(node.size - 2, 0)).astype(np.int64)      # (the kernel compares the low 32 bits, unsigned)
    return node[p], node[p + 1]


def ordered_sum(m, kind, y, s, order, ld=False, start=None):
    """sum over the records of -0.5 ((y - m) s)^2, kinds in `order`, each in record order; float64: one fma per term"""
    ft = LD if ld else np.float64
    ll = np.zeros(kind.shape[0], dtype=ft) if start is None else start
    with np.errstate(invalid='ignore'):
        for kd in order:
            for r in range(kind.shape[1]):
                on = kind[:, r] == kd
                if not on.any():
                    continue
                z = (y[:, r].astype(ft) - m[:, r]) * s[:, r].astype(ft)
                ll = np.where(on, ll + ft(-0.5) * z * z if ld else hl.fma(-0.5 * z, z, ll), ll)
    return ll


def loglik_from_rows(rows, idx, rec, span, n_cond, n_plume, u=None, basis=None, lat0=1, norm=NORM_LOG10, scale=1.0, a_1=None,
                     discharge=None, ld=False):
    """(loglik [n], pred [n][n_rec]) of the launch from its rows; u: None (u_rank 0: chain_loglik_np.loglik_from_rows itself) or
    dict(basis [dof][u_rank], node [n_node], norm, scale)"""
    if u is None:
        return cl.loglik_from_rows(rows, idx, rec, span, n_cond, basis=basis, lat0=lat0, norm=norm, scale=scale, a_1=a_1,
                                   discharge=discharge, ld=ld)
    kind, w, y, s, k = cl.sample_tables(rec, span, n_cond, idx)
    ft = LD if ld else np.float64
    rows = [np.asarray(r, dtype=ft) for r in rows]
    # the parent's model values: with every u_ion record hidden from it (it would mark the condition)
    hidden = np.asarray(span).reshape(-1, 4, 2).copy()
    hidden[:, UION] = 0
    _, m = cl.loglik_from_rows(rows, idx, rec, hidden, n_cond, basis=basis, lat0=lat0, norm=norm, scale=scale, ld=ld)
    a, b = uion_nodes(rec, u['node'])
    lat = rows[4 + n_plume:]
    ua, ub = (uion_cells(lat, u['basis'], c, u['norm'], u['scale'], ld) for c in (a, b))
    mu = ua + w.astype(LD) * (ub - ua) if ld else hl.interp_model(w, ua, ub)
    m = np.where(kind == UION, mu, m)
    ll = ordered_sum(m, kind, y, s, (UION,) + ((JION,) if basis is not None else ()) + (VCC, T), ld)
    with np.errstate(invalid='ignore'):
        if basis is None:
            ll = np.where((kind == JION).any(axis=1), ft(np.nan), ll)
        if a_1 is not None:
            i_d = rows[1] / (ft(1) - ft(2) * np.asarray(a_1, dtype=ft))
            z = (ft(discharge[0]) - i_d) * ft(1.0 / discharge[1])
            ll = ll + ft(-0.5) * z * z if ld else hl.fma(-0.5 * z, z, ll)
    return ll, m


def chain_loglik(stages, t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map, rec, span, n_cond, first=0, ld=False, u=None, **kw):
    """the whole launch from the tables; sample i has global index first + i.  u = None: chain_loglik_np.chain_loglik itself."""
    if u is None:
        return cl.chain_loglik(stages, t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map, rec, span, n_cond, first=first, ld=ld, **kw)
    st = stages
    if ld:
        st = [(b, [c[x] for x in b], [v[x] for x in b]) if isinstance(c, dict) else (b, c, v) for b, c, v in stages]
    rows = compose(st, t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map, ld=ld)
    n_plume = rows.shape[0] - 4 - u['basis'].shape[1]
    return loglik_from_rows(rows, first + np.arange(t_ext.shape[1]), rec, span, n_cond, n_plume, u=u, ld=ld, **kw) + (rows,)


def sum_ref(pred, kind, y, inv_std, i_b0=None, a_1=None, discharge=None):
    """chain_loglik_np.sum_ref with the u_ion records counted: (sum, bound) of the launch's loglik given ITS model values"""
    valid = kind >= 0
    tot, bound = hl.record_sum(np.where(valid, pred, 0.0), y, inv_std, valid)
    if a_1 is not None:
        t, tb = cl.discharge_term(i_b0, a_1, discharge[0], 1.0 / discharge[1])
        nv = valid.sum(axis=-1)
        sabs = bound / (1.01 * (nv + 6) * U)
        tot = tot + t
        bound = 1.01 * (nv + 7) * U * (sabs + np.abs(t)) + tb
    return tot, bound


def model_bound(rows, idx, rec, span, n_cond, n_plume, u, basis, lat0=1, norm=NORM_LOG10, scale=1.0):
    """chain_loglik_np.model_bound plus the u_ion records' (module docstring); rows: the long-double rows"""
    kind, w, _, _, _ = cl.sample_tables(rec, span, n_cond, idx)
    dm = cl.model_bound(rows, idx, rec, span, n_cond, basis, lat0, norm, scale)
    rows = [np.asarray(r, dtype=LD) for r in rows]
    lat = rows[4 + n_plume:]
    rank = u['basis'].shape[1]
    d_lat = [LD(cl.CHAIN_REL) * np.abs(r).max() for r in lat]
    a, b = uion_nodes(rec, u['node'])

    def du(cells):
        ab = np.abs(u['basis'][cells]).astype(LD)                                        # [n_rec][rank]
        dv = sum(ab[None, :, q] * (d_lat[q] + LD(1.01 * rank * U) * np.abs(lat[q])[:, None]) for q in range(rank))
        val = uion_cells(lat, u['basis'], cells, u['norm'], u['scale'], ld=True)
        if u['norm'] == NORM_LOG10:
            return np.abs(val) * (LD(np.log(10.0)) * dv + 2 * U) * LD(1.01), val
        return (dv / LD(abs(u['scale'])) if u['norm'] == NORM_LINEAR else dv) + U * np.abs(val), val
    dlo, lo = du(a)
    dhi, hi = du(b)
    wl = np.abs(w).astype(LD)
    mu = lo + w.astype(LD) * (hi - lo)
    dmu = dlo + 2 * wl * np.maximum(dlo, dhi) + LD(1.01 * U) * (wl * np.abs(hi - lo) + np.abs(mu))
    return np.where(kind == UION, dmu, dm)
