"""numpy / long-double restatements of pem_chain_system_loglik_f64_dev (csrc/pem_surrogate.hip): the component chain of
tests/chain_np.py followed by the multi-QoI Gaussian sums of tests/hp_likelihood.py.  TEST INFRASTRUCTURE.

Per sample i (condition c = i mod n_cond), from the chain's rows V_cc, I_B0, T, div_angle, T_c, p_1 .. (plume output o at row 3 for
o = 0, else 4 + o):
    j[k]   = denorm(v), v = 0; v = fma(p_{lat0+q}, basis[k][q], v) for q = 0 .. rank - 1; denorm: 10^v | v / scale | v
    m_r    = fma(w, j[k+1] - j[k], j[k]) (j_ion) | V_cc | T
    loglik = sum_r -0.5 z^2, z = (y - m) * inv_std, in the order j_ion, V_cc, T, each term added by one fma(-0.5 z, z, sum);
             then, with a_1, one more term z = (D - I_d) * inv_sigma, I_d = I_B0 / (1 - 2 a_1)
    a condition with u_ion records, or with j_ion records and no basis, gives NaN.

Bounds (u = 2^-53, gamma_k <= 1.01 k u, as tests/hp_likelihood.py):
  * the record sum given the model values: the kernel adds a term by ONE fma per record and lane (no shuffle adds), so a term passes
    through at most n additions and z^2 carries 4 roundings: n + 4 <= hp_likelihood.record_sum's n + 6, which is used as it is.
  * the discharge term: 1 - 2 a_1 is one rounding (2 a_1 is exact) and the division a second: |dI_d| <= 2.02 u |I_d|; z = (D - I_d)
    inv_sigma two more, so t = -0.5 z^2 moves by |z| inv_sigma 2.02 u |I_d| + 4.04 u |t|; it is added by one more fma, so every term
    now passes through at most n + 1 additions: the sum's constant becomes n + 7 (4 of z^2 + n + 1 additions + the 2 spare of
    record_sum's count), over sum |t_r| + |t_d|.
  * the model values of the float64 restatement against the long-double one (`model_bound`): the chain's rows differ by at most
    CHAIN_REL max|row| (the figure tests/test_chained_surrogate_host.py holds chain_np.compose to on exact polynomial stages); a
    latent error d moves v by at most sum_q |basis[k][q]| d, plus gamma_rank sum_q |p_q basis[k][q]| of the fma chain; 10^v moves by
    10^v (ln 10 |dv| + 2 u) (pow within 1 ulp); the interpolation adds u (|w| |hi - lo| + |m|) and at most |dj_lo| + 2 |w| max |dj|.
"""
import numpy as np

import chain_np
import hp_likelihood as hl

LD, U = hl.LD, hl.U
JION, VCC, T, UION = 0, 1, 2, 3
NORM_NONE, NORM_LOG10, NORM_LINEAR = 0, 1, 2
CHAIN_REL = 1e-13


def _plume_row(o):
    return 3 if o == 0 else 4 + o


def node_values(rows, basis, lat0, k, norm=NORM_LOG10, scale=1.0, ld=False):
    """j[k] of every sample: rows [4 + n_plume][n], basis [91][rank], k [n][m] node indices -> [n][m]"""
    rank = basis.shape[1]
    k = np.asarray(k, dtype=np.int64)
    if ld:
        v = np.zeros(k.shape, dtype=LD)
        for q in range(rank):
            v = v + np.asarray(rows[_plume_row(lat0 + q)], dtype=LD)[:, None] * basis[k, q].astype(LD)
        return LD(10) ** v if norm == NORM_LOG10 else (v / LD(scale) if norm == NORM_LINEAR else v)
    v = np.zeros(k.shape)
    for q in range(rank):
        v = hl.fma(np.broadcast_to(np.asarray(rows[_plume_row(lat0 + q)], dtype=np.float64)[:, None], k.shape), basis[k, q], v)
    return 10.0 ** v if norm == NORM_LOG10 else (v / scale if norm == NORM_LINEAR else v)


def sample_tables(rec, span, n_cond, idx):
    """per sample of global index idx [n]: (kind [n][n_rec] with -1 where the record is not the sample's, w, y, inv_std, k [n][n_rec])"""
    rec, span = np.asarray(rec, dtype=np.float64), np.asarray(span).reshape(-1, 4, 2)
    n_rec = rec.shape[0]
    kind_c = np.full((n_cond, n_rec), -1, dtype=np.int64)
    for c in range(n_cond):
        for kd in range(4):
            f, cnt = span[c, kd]
            kind_c[c, f:f + cnt] = kd
    kind = kind_c[np.asarray(idx) % n_cond]
    k = np.minimum(np.ascontiguousarray(rec[:, 3]).view(np.int64).astype(np.uint64), 89).astype(np.int64)
    bc = lambda a: np.broadcast_to(a, kind.shape)                                                # noqa: E731
    return kind, bc(rec[:, 0]), bc(rec[:, 1]), bc(rec[:, 2]), bc(k)


def loglik_from_rows(rows, idx, rec, span, n_cond, basis=None, lat0=1, norm=NORM_LOG10, scale=1.0, a_1=None, discharge=None, ld=False):
    """(loglik [n], pred [n][n_rec] with NaN where a record is not the sample's) from the chain's rows of the samples whose global
    indices are idx; float64 in the kernel's order, or long double (ld)"""
    kind, w, y, s, k = sample_tables(rec, span, n_cond, idx)
    n, n_rec = kind.shape
    ft = LD if ld else np.float64
    rows = [np.asarray(r, dtype=ft) for r in rows]
    m = np.full((n, n_rec), np.nan, dtype=ft)
    if basis is not None:
        kj = np.where(kind == JION, k, 0)
        lo, hi = (node_values(rows, basis, lat0, kk, norm, scale, ld) for kk in (kj, kj + 1))
        mj = lo + w.astype(LD) * (hi - lo) if ld else hl.interp_model(w, lo, hi)
        m = np.where(kind == JION, mj, m)
    m = np.where(kind == VCC, rows[0][:, None], m)
    m = np.where(kind == T, rows[2][:, None], m)
    bad = (kind == UION).any(axis=1) | ((kind == JION).any(axis=1) if basis is None else False)
    ll = np.zeros(n, dtype=ft)
    with np.errstate(invalid='ignore'):
        for kd in (JION, VCC, T):                                   # the kernel's order: kinds in turn, each in record order
            if kd == JION and basis is None:
                continue
            for r in range(n_rec):
                on = kind[:, r] == kd
                if not on.any():
                    continue
                z = (y[:, r].astype(ft) - m[:, r]) * s[:, r].astype(ft)
                ll = np.where(on, ll + ft(-0.5) * z * z if ld else hl.fma(-0.5 * z, z, ll), ll)
        ll = np.where(bad, ft(np.nan), ll)
        if a_1 is not None:
            i_d = rows[1] / (ft(1) - ft(2) * np.asarray(a_1, dtype=ft))
            z = (ft(discharge[0]) - i_d) * ft(1.0 / discharge[1])
            ll = ll + ft(-0.5) * z * z if ld else hl.fma(-0.5 * z, z, ll)
    return ll, m


def chain_loglik(stages, t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map, rec, span, n_cond, first=0, ld=False, **kw):
    """the whole launch from the tables: chain_np.compose / compose_ld, then loglik_from_rows; sample i has global index first + i"""
    if ld:
        rows = chain_np.compose_ld([(b, [c[x] for x in b], [v[x] for x in b]) if isinstance(c, dict) else (b, c, v) for b, c, v in stages],
                                   t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map)
    else:
        rows = chain_np.compose(stages, t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map)
    return loglik_from_rows(rows, first + np.arange(t_ext.shape[1]), rec, span, n_cond, ld=ld, **kw) + (rows,)


def discharge_term(i_b0, a_1, discharge, inv_sigma):
    """(t, bound) of the launch's discharge term from ITS I_B0 (float64), long double"""
    i_d = hl._ld(i_b0) / (LD(1) - LD(2) * hl._ld(a_1))
    z = (LD(discharge) - i_d) * LD(inv_sigma)
    t = LD(-0.5) * z * z
    return t, np.abs(z) * LD(inv_sigma) * LD(2.02 * U) * np.abs(i_d) + LD(4.04 * U) * np.abs(t)


def sum_ref(pred, kind, y, inv_std, i_b0=None, a_1=None, discharge=None):
    """(sum, bound) of the launch's loglik given ITS model values `pred` [n][n_rec] (float64): hp_likelihood.record_sum over the
    sample's own records, plus the discharge term with the constant n + 7 (module docstring)"""
    valid = (kind == JION) | (kind == VCC) | (kind == T)
    tot, bound = hl.record_sum(np.where(valid, pred, 0.0), y, inv_std, valid)
    if a_1 is not None:
        t, tb = discharge_term(i_b0, a_1, discharge[0], 1.0 / discharge[1])
        nv = valid.sum(axis=-1)
        sabs = bound / (1.01 * (nv + 6) * U)                        # record_sum's sum |t|
        tot = tot + t
        bound = 1.01 * (nv + 7) * U * (sabs + np.abs(t)) + tb
    return tot, bound


def model_bound(rows, idx, rec, span, n_cond, basis, lat0=1, norm=NORM_LOG10, scale=1.0):
    """bound on |m (float64 restatement) - m (long double)| per sample and record (module docstring); rows: the long-double rows"""
    kind, w, _, _, k = sample_tables(rec, span, n_cond, idx)
    rows = [np.asarray(r, dtype=LD) for r in rows]
    d_row = [LD(CHAIN_REL) * np.abs(r).max() for r in rows]
    dm = np.zeros(kind.shape, dtype=LD)
    if basis is not None:
        rank = basis.shape[1]
        kj = np.where(kind == JION, k, 0)

        def dj(kk):
            ab = np.abs(basis[kk]).astype(LD)                                            # [n][n_rec][rank]
            dv = sum(ab[..., q] * (d_row[_plume_row(lat0 + q)] + LD(1.01 * rank * U) * np.abs(rows[_plume_row(lat0 + q)])[:, None])
                     for q in range(rank))
            j = node_values(rows, basis, lat0, kk, norm, scale, ld=True)
            if norm == NORM_LOG10:
                return np.abs(j) * (LD(np.log(10.0)) * dv + 2 * U) * LD(1.01), j
            return (dv / LD(abs(scale)) if norm == NORM_LINEAR else dv) + U * np.abs(j), j
        dlo, lo = dj(kj)
        dhi, hi = dj(kj + 1)
        wl = np.abs(w).astype(LD)
        mj = lo + w.astype(LD) * (hi - lo)
        dmj = dlo + 2 * wl * np.maximum(dlo, dhi) + LD(1.01 * U) * (wl * np.abs(hi - lo) + np.abs(mj))
        dm = np.where(kind == JION, dmj, dm)
    dm = np.where(kind == VCC, d_row[0], dm)
    dm = np.where(kind == T, d_row[2], dm)
    return dm


def composition_ref(field, rows, idx, rec, span, n_cond, a_1=None, discharge=None):
    """(loglik, bound) of the launch against the COMPOSITION it replaces: `field` [n][91] and `rows` of
    pem_sparse_predict_chain_f64_dev for the same samples (float64), each j_ion record interpolated exactly in long double
    (hl.model_error bounds the kernel's own fma), V_cc and T taken from the rows, every term summed in long double.  A term passes
    through at most n + 1 additions of the kernel and z^2 carries 4 roundings: the constant n + 7 of the module docstring."""
    kind, w, y, s, k = sample_tables(rec, span, n_cond, idx)
    valid = (kind == JION) | (kind == VCC) | (kind == T)
    m = np.zeros(kind.shape, dtype=LD)
    dm = np.zeros(kind.shape, dtype=LD)
    if field is not None:
        field = np.asarray(field, dtype=np.float64)
        kj = np.where(kind == JION, k, 0)
        lo, hi = np.take_along_axis(field, kj, axis=1), np.take_along_axis(field, kj + 1, axis=1)
        m = np.where(kind == JION, hl._ld(lo) + hl._ld(w) * (hl._ld(hi) - hl._ld(lo)), m)
        dm = np.where(kind == JION, hl.model_error(w, lo, hi), dm)
    m = np.where(kind == VCC, hl._ld(rows[0])[:, None], m)
    m = np.where(kind == T, hl._ld(rows[2])[:, None], m)
    z = (hl._ld(y) - m) * hl._ld(s)
    t = np.where(valid, LD(-0.5) * z * z, LD(0))
    tot, sabs = t.sum(axis=1), np.abs(t).sum(axis=1)
    extra = 1.01 * np.where(valid, np.abs(z) * hl._ld(s) * dm, LD(0)).sum(axis=1)
    if a_1 is not None:
        td, tb = discharge_term(rows[1], a_1, discharge[0], 1.0 / discharge[1])
        tot, sabs, extra = tot + td, sabs + np.abs(td), extra + tb
    bound = 1.01 * (valid.sum(axis=1) + 7) * U * sabs + extra
    bad = (kind == UION).any(axis=1) | ((kind == JION).any(axis=1) if field is None else False)
    return np.where(bad, LD(np.nan), tot), np.where(bad, LD(0), bound)
