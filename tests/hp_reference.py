"""Long-double restatements of the configs[3] pipeline's kernels, with per-entry error bounds.  TEST INFRASTRUCTURE.

The SVD compression (csrc/pem_svd.hip) and the sparse-grid predict (csrc/pem_surrogate.hip) are held here to their own
formulas evaluated in np.longdouble (64-bit mantissa: its own error is 2^-11 of the double rounding unit, absorbed by the
factor 1.01 below), entry by entry, under a bound of the form  C * u * S  where u = 2^-53 and S is the same formula run on
absolute values.  C is derived from the number of roundings a term of the kernel's sum goes through (the classical
|fl(sum x_i) - sum x_i| <= gamma_k sum |x_i|, gamma_k = k u / (1 - k u) <= 1.01 k u for k u < 0.01), whatever the order
the kernel sums in: a kernel that drops a term, reads a wrong row or applies a wrong norm misses it by orders of magnitude.

Transcendentals add their own error, E ulp being at most 2 E u of the magnitude.  The constants are tests/hp_math.py's, derived
or measured there on the host and on the device (profiles/pem_math_r01.txt): log10 in the compress kernels is the table version
(csrc/pem_math.h), within LOG10_TAB_ULPS = 1.4 ulp of the exact value, i.e. 2.8 u of its magnitude; 10^x is held to EXP10_REL =
2 EXP10_ULPS u = 3.33e-16 of its value for pem_exp10 (the reconstruct kernel) and to LIB_EXP10_REL = 2 LIB_EXP10_ULPS u for the
library exp10 (the fused field path), plus the argument's bound scaled by ln 10 (d 10^v = ln 10 * 10^v dv).
"""
import ctypes as C
import itertools

import numpy as np

from hp_math import EXP10_ULPS, LIB_EXP10_ULPS, LOG10_TAB_ULPS

LD = np.longdouble
U = 2.0 ** -53
EXP10_REL = 2.0 * EXP10_ULPS * U            # pem_exp10
LIB_EXP10_REL = 2.0 * LIB_EXP10_ULPS * U    # the library exp10
LOG10_TAB_REL = 2.0 * LOG10_TAB_ULPS        # in units of u
LN10 = 2.302585092994045684
NORMS = {'none': 0, 'log10': 1, 'linear': 2}
assert np.finfo(LD).nmant >= 63, 'the reference needs an 80-bit long double'


# ---- SVD compression ------------------------------------------------------------------------------------------------
def norm_ld(y, norm, scale=1.0):
    y = np.asarray(y, dtype=np.float64).astype(LD)
    if norm == 'log10':
        return np.log10(y)
    return y * LD(scale) if norm == 'linear' else y


def compress_ref(y, basis, norm, scale=1.0):
    """(latent, bound) for latent = norm(y) @ basis, y [n][dof], basis [dof][r] (float64 arrays).

    C: each latent is a sum of dof products.  The direct kernel sums them on the matrix pipe (24 MFMA steps of four products
    in two chains, then one add), the tiled kernels in an fma chain of ceil(dof / KG) steps per k-group and log2(KG) shuffle
    adds: no term goes through more than dof + 1 roundings, so the product costs 1.01 (dof + 1) <= dof + 4 for dof <= 208.
    The norm: linear is one multiplication (1 u of |norm(y)|), log10 the table version (LOG10_TAB_REL = 2.8 u of |norm(y)|); each enters
    the sum weighted by |basis|, hence the same S."""
    yn = norm_ld(y, norm, scale)
    b = np.asarray(basis, dtype=np.float64).astype(LD)
    z = yn @ b
    s = np.abs(yn) @ np.abs(b)
    dof = b.shape[0]
    c = dof + 4 + {'none': 0.0, 'linear': 1.0, 'log10': LOG10_TAB_REL}[norm]
    return z, c * U * s


def denorm_bound(v, s_v, c_v, norm, scale=1.0, exp10_rel=EXP10_REL):
    """(field, bound) for field = denorm(v) where v (long double) was formed with at most c_v roundings per term of S = s_v;
    exp10_rel: the relative error of the 10^x the kernel calls."""
    dv = 1.01 * c_v * U * s_v
    if norm == 'log10':
        f = LD(10.0) ** v
        return f, np.abs(f) * (1.01 * LN10 * dv + exp10_rel)
    if norm == 'linear':
        f = v / LD(scale)
        return f, dv / abs(scale) + U * np.abs(f)
    return v, dv


def reconstruct_ref(latent, basis, norm, scale=1.0, exp10_rel=EXP10_REL):
    """(field, bound) for field = denorm(latent @ basis^T), latent [n][r], basis [dof][r].

    C: each value is a sum of r products on the matrix pipe (ceil(r / 4) MFMA steps of four; the zero-padded columns add
    exact zeros): at most r roundings, plus the denorm (one division for linear; 10^x see the module docstring)."""
    lat = np.asarray(latent, dtype=np.float64).astype(LD)
    b = np.asarray(basis, dtype=np.float64).astype(LD)
    v = lat @ b.T
    return denorm_bound(v, np.abs(lat) @ np.abs(b).T, b.shape[1], norm, scale, exp10_rel)


def field_ref(latent, basis, norm, scale=1.0):
    """the fused reconstruction of pem_sparse_predict_field_f64_dev: an fma chain over the rank (r roundings), then the
    denorm -- the same bound as reconstruct_ref, with the library exp10 in the place of pem_exp10"""
    return reconstruct_ref(latent, basis, norm, scale, LIB_EXP10_REL)


def assert_within(got, want, bound, what=''):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f'{what}: non-finite output'
    err = np.abs(got.astype(LD) - want)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err / np.maximum(bound, LD(1e-300))), err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} entries outside the bound; worst at {i}: got {got[i]!r} want '
                             f'{float(want[i])!r} err {float(err[i]):.3e} bound {float(bound[i]):.3e}')


# ---- sparse-grid predict ----------------------------------------------------------------------------------------------
def node_count(level):
    return 1 if level == 0 else 2 ** level + 1


def lagrange_ld(level, t):
    """[m][n] Lagrange cardinal polynomials of the level's node doubles (surrogate.nodes, the kernel's LOBATTO_NODES) at t"""
    from hallthrusterpem_amd.surrogate import nodes
    x = nodes(level).astype(LD)
    tl = np.asarray(t, dtype=np.float64).astype(LD)
    out = np.ones((x.size, tl.size), dtype=LD)
    for j in range(x.size):
        for k in range(x.size):
            if k != j:
                out[j] *= (tl - x[k]) / (x[j] - x[k])
    return out


def grid_roundings(levels, n_beta):
    """C of one grid (levels of its active dimensions, in dimension order) in a sum over n_beta grids.

    A basis value l_j of m nodes is c_j * prod_{i<j} d_i * prod_{i>j} d_i, d_i = t - t_i: m - 1 subtractions, m - 3
    multiplications in the prefix / suffix chains, two more to join them and the rounded c_j: 2m - 1 roundings (0 for m = 1).
    The outer dimensions' weights are multiplied together (n_outer - 1 roundings), the innermost row is an fma chain of m_I
    terms, the rows an fma chain of R = prod(outer m) terms, the grids an fma chain of n_beta terms."""
    ms = [node_count(l) for l in levels]
    basis = sum(2 * m - 1 for m in ms if m > 1)
    outer = ms[:-1]
    return basis + max(len(outer) - 1, 0) + (ms[-1] if ms else 1) + int(np.prod(outer)) + n_beta


def grid_ref(beta, values, t):
    """(f [n_out][n], S [n_out][n]) of one grid: sum over its nodes of Y[node] prod_d l_{j_d}(t_d) (long double)"""
    active = [d for d in range(len(beta)) if beta[d] > 0]
    n = t.shape[1]
    w = np.ones((1, n), dtype=LD)
    for d in active:
        b = lagrange_ld(beta[d], t[d])
        w = (w[:, None, :] * b[None, :, :]).reshape(-1, n)
    y = np.asarray(values, dtype=np.float64).astype(LD)
    assert y.shape[0] == w.shape[0]
    return y.T @ w, np.abs(y).T @ np.abs(w)


def predict_ref(betas, coefs, values, t, per_grid=False):
    """(f, bound) of pem_sparse_predict_f64_dev (f [n_out][n]) or, per_grid, of pem_sparse_grid_values_f64_dev ([n_beta][n_out][n],
    every grid times its coefficient).  betas: level tuples; coefs: one per beta; values: [rows][n_out] per beta."""
    nb = len(betas)
    parts, bounds = [], []
    for beta, c, y in zip(betas, coefs, values):
        f, s = grid_ref(beta, y, t)
        k = grid_roundings([l for l in beta if l > 0], 1 if per_grid else nb)
        parts.append(LD(c) * f)
        bounds.append(1.01 * k * U * abs(c) * s)
    if per_grid:
        return np.stack(parts), np.stack(bounds)
    return sum(parts), sum(bounds)


def index_table(betas, values):
    """the kernel's index rows {n_active, first value row, dims[5], levels[5]} and the concatenated value table"""
    idx = np.zeros((len(betas), 12), dtype=np.int32)
    off = 0
    for i, b in enumerate(betas):
        active = [d for d in range(len(b)) if b[d] > 0]
        assert len(active) <= 5 and max(b) <= 4
        idx[i, 0], idx[i, 1] = len(active), off
        for a, d in enumerate(active):
            idx[i, 2 + a], idx[i, 7 + a] = d, b[d]
        assert values[i].shape[0] == int(np.prod([node_count(l) for l in b]))
        off += values[i].shape[0]
    return idx, np.ascontiguousarray(np.concatenate(values))


def beta_of(D, levels_at):
    """level tuple of D dimensions from {dimension: level}"""
    b = [0] * D
    for d, l in levels_at.items():
        b[d] = l
    return tuple(b)


def ptr(x):
    return C.c_void_p(x.data_ptr())
