"""numpy restatement of pem_chain_sobol_sweep_f64_dev (csrc/pem_surrogate_sobol.hip): the Sobol' study over a pressure sweep through
the chained surrogate.  TEST INFRASTRUCTURE, composed from existing pieces: the design rows are oracle/sampler_np.sample on the
streams of sobol.row_stream; the coordinates are u = log10(x) or x, t = 2.0 * (u - a) / w - 1.0; the chain is
chain_uion_np.compose, the u_ion cell chain_uion_np.uion_cells; the estimators are sobol_sweep_np.estimates.

    f[e][q][i]   e = 0: row A, 1: row B, 2 + j: row A with the group's varied input j from B;  q: V_cc | T, u_ion(cell)
"""
import numpy as np

import chain_uion_np as cu
import sobol_sweep_np as ssn

GROUP_QOIS = {'Cathode': ('V_cc',), 'Thruster': ('T', 'uion')}


def as_dicts(stage):
    """a (betas, coefs, values) stage given as lists (test_chained_surrogate._stage) in the form oracle/surrogate_np.predict reads"""
    betas, coefs, values = stage
    if isinstance(coefs, dict):
        return stage
    return betas, dict(zip(betas, coefs)), dict(zip(betas, values))


def stage_from_tables(idx, coef, vals, n_dim):
    """a device table of the chained launch -- index rows {n_active, first value row, dims[5], levels[5]}, coefficients, value rows
    [rows][n_out] -- in the form oracle/surrogate_np.predict reads: the kernel keeps a grid's nodes in the order of the row's dims
    (the last one innermost), surrogate_np in the order of the slots"""
    idx, coef, vals = np.asarray(idx), np.asarray(coef, dtype=np.float64), np.asarray(vals, dtype=np.float64)
    betas, coefs, values = [], {}, {}
    for row, c in zip(idx, coef):
        na, off = int(row[0]), int(row[1])
        dims, lv = [int(d) for d in row[2:2 + na]], [int(l) for l in row[7:7 + na]]
        beta = [0] * n_dim
        for d, l in zip(dims, lv):
            beta[d] = l
        beta = tuple(beta)
        ms = [2 ** l + 1 for l in lv]
        k = int(np.prod(ms)) if ms else 1
        y = vals[off:off + k].reshape(*ms, vals.shape[1])
        y = y.transpose(*np.argsort(dims), na).reshape(k, vals.shape[1])
        assert beta not in coefs
        betas.append(beta)
        coefs[beta], values[beta] = float(c), y
    return betas, coefs, values


def rows(group, n, first, seed, n_p, p, kind, a, b):
    """(xa, xb) [15][n]: rows A and B of `group` at pressure index p for the prior table kind, a, b ([15] each)"""
    from oracle import sampler_np
    from hallthrusterpem_amd import sobol as study
    g = study.GROUPS.index(group)
    return tuple(sampler_np.sample(n, first, seed, study.row_stream(g, n_p, p, 0, r), kind, a, b) for r in (0, 1))


def coords(x, slot_rows, is_log, a, w, log10=np.log10):
    """x: [15][n] -> [n_ext][n], left to right; `log10`: the logarithm (the tests move it by an ulp either way)"""
    t = np.empty((len(slot_rows), x.shape[1]))
    for k, r in enumerate(slot_rows):
        u = log10(x[r]) if is_log[k] else x[r]
        t[k] = 2.0 * (u - a[k]) / w[k] - 1.0
    return t


def evaluate(group, t_ext, chain, u=None):
    """the group's QoIs [nq][n] at external coordinates t_ext.  chain: dict(stages (dict form; the cathode's and the thruster's are
    read), vcc_slot, ib0_slot, vmap); u: None (no latents: the u_ion row is NaN) or dict(basis [dof][rank], cell, norm, scale)"""
    # no QoI of these groups reads the plume stage (the launch never runs it): a constant table stands in for it
    zero = (0,) * (t_ext.shape[0] + 2)
    stages = [chain['stages'][0], chain['stages'][1], ([zero], {zero: 1.0}, {zero: np.zeros((1, 1))})]
    out = cu.compose(stages, t_ext, chain['vcc_slot'], chain['ib0_slot'], chain['vmap'], (0.0, 1.0))
    if group == 'Cathode':
        return out[:1]
    n_plume = 1
    if u is None:
        return np.stack([out[2], np.full(t_ext.shape[1], np.nan)])
    lat = out[4 + n_plume:]
    return np.stack([out[2], cu.uion_cells(lat, u['basis'], [u['cell']], u['norm'], u['scale'])[:, 0]])


def sweep_f(group, n, first, seed, n_p, p, kind, a, b, slot, chain, u=None, log10=np.log10):
    """f [nv + 2][nq][n] of pressure index p; slot = (rows, is_log, a, w) of the external coordinates"""
    from hallthrusterpem_amd import sobol as study
    xa, xb = rows(group, n, first, seed, n_p, p, kind, a, b)
    cols = [list(study.PEM_V0_NOMINAL).index(k) for k in study.GROUP_INPUTS[group]]
    f = [evaluate(group, coords(x, *slot, log10=log10), chain, u) for x in (xa, xb)]
    for c in cols:
        x = xa.copy()
        x[c] = xb[c]
        f.append(evaluate(group, coords(x, *slot, log10=log10), chain, u))
    return np.stack(f)


def estimates(f, group):
    """{qoi: sobol_sweep_np.estimates} of one pressure's f [nv + 2][nq][n]"""
    return {q: ssn.estimates(f[0, k], f[1, k], f[2:, k]) for k, q in enumerate(GROUP_QOIS[group])}


# ---- closed-form indices of  f = c0 + sum_i (a_i t_i + b_i t_i^2) + c t_0 t_1,  t_i ~ U(lo_i, hi_i) independent --------------------
def _moments(lo, hi):
    return [(hi ** (k + 1) - lo ** (k + 1)) / ((k + 1) * (hi - lo)) for k in range(1, 5)]


def quadratic_indices(lin, quad, cross, lo, hi):
    """(S1, ST) of the polynomial above.  The first-order part of input 0 is (a_0 + c E t_1) t_0 + b_0 t_0^2 (and likewise for 1);
    Var(alpha t + beta t^2) = alpha^2 Var t + beta^2 Var t^2 + 2 alpha beta Cov(t, t^2); the one interaction has variance
    c^2 Var t_0 Var t_1 and belongs to the total index of both."""
    lin, quad = np.asarray(lin, dtype=np.float64), np.asarray(quad, dtype=np.float64)
    m = np.array([_moments(l, h) for l, h in zip(lo, hi)])            # [d][E t, E t^2, E t^3, E t^4]
    var_t, var_t2, cov = m[:, 1] - m[:, 0] ** 2, m[:, 3] - m[:, 1] ** 2, m[:, 2] - m[:, 0] * m[:, 1]
    alpha = lin.copy()
    alpha[0] += cross * m[1, 0]
    alpha[1] += cross * m[0, 0]
    v1 = alpha ** 2 * var_t + quad ** 2 * var_t2 + 2 * alpha * quad * cov
    v01 = cross ** 2 * var_t[0] * var_t[1]
    total = v1.sum() + v01
    vt = v1.copy()
    vt[:2] += v01
    return v1 / total, vt / total
