"""numpy restatement of hallthrusterpem_amd/marginals.py (the definitions its docstring states), for the tests.

  draws         drop b = int(burnin * n) rows; pool the remaining n' rows of all K chains into m = n' K draws of d parameters.
  edges         edges[i] = np.linspace(lo_i, hi_i, bins + 1); (lo_i, hi_i) = (min, max) over the finite pooled draws unless
                `ranges` gives them; lo_i == hi_i widened to (lo - 0.5, hi + 0.5); no finite draw: (0, 1).
  bin rule      k = np.searchsorted(edges, v, side='right') - 1; v == edges[bins] goes to bin bins - 1; k outside 0 ... bins-1
                or v not finite: no bin.
  counts        hist1d[i] = np.bincount of the bins of parameter i; hist2d[i][j] = np.bincount of ki * bins + kj over the
                draws with both values in a bin; dropped[i], nonfinite[i] = draws of parameter i in no bin / not finite.
  density       kde[i][q] = 1 / (m h sqrt(2 pi)) sum_t exp(-((g_q - x_t) / h)^2 / 2), h = f s, s = std(ddof 1) of the pooled
                draws, f = m^(-1/5) ('scott'), (3 m / 4)^(-1/5) ('silverman') or the given factor; s == 0 or a non-finite
                draw: NaN.  `kde_direct` sums in np.longdouble and returns the sums the error bound needs.
  levels        counts sorted descending, accumulated; level(p) = the count of the first cell with cumulative >= p * total.
"""
import numpy as np


def pool(samples, burnin=0.1):
    s = np.asarray(samples, dtype=np.float64)
    if s.ndim == 2:
        s = s[:, None, :]
    s = s[int(burnin * s.shape[0]):]
    return s.reshape(-1, s.shape[2])


def make_edges(x, bins, ranges=None):
    d = x.shape[1]
    out = np.empty((d, bins + 1))
    for i in range(d):
        if ranges is None:
            f = x[np.isfinite(x[:, i]), i]
            lo, hi = (f.min(), f.max()) if f.size else (0.0, 1.0)
        else:
            lo, hi = ranges[i]
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        out[i] = np.linspace(lo, hi, bins + 1)
    return out


def bin_index(v, edges):
    """bins of the values v under the table `edges` (bins + 1,); -1 = no bin"""
    bins = edges.size - 1
    k = np.searchsorted(edges, v, side='right') - 1
    k[v == edges[-1]] = bins - 1
    k[(k < 0) | (k >= bins) | ~np.isfinite(v)] = -1
    return k


def histograms(x, edges, pairs=True):
    """x (m, d) pooled draws, edges (d, bins + 1) -> hist1d (d, bins), hist2d (d, d, bins, bins) or None, dropped, nonfinite"""
    m, d = x.shape
    bins = edges.shape[1] - 1
    k = np.stack([bin_index(x[:, i], edges[i]) for i in range(d)], axis=1)
    h1 = np.stack([np.bincount(k[k[:, i] >= 0, i], minlength=bins) for i in range(d)]).astype(np.int64)
    dropped = (k < 0).sum(axis=0).astype(np.int64)
    nonfinite = (~np.isfinite(x)).sum(axis=0).astype(np.int64)
    h2 = None
    if pairs:
        h2 = np.zeros((d, d, bins, bins), np.int64)
        for i in range(d):
            h2[i, i] = np.diag(h1[i])
            for j in range(i + 1, d):
                ok = (k[:, i] >= 0) & (k[:, j] >= 0)
                t = np.bincount(k[ok, i] * bins + k[ok, j], minlength=bins * bins).reshape(bins, bins)
                h2[i, j], h2[j, i] = t, t.T
    return h1, h2, dropped, nonfinite


def bandwidth(x, bw='scott', dtype=np.longdouble):
    """h (d,) in `dtype`; NaN where s == 0 or a draw is not finite"""
    m = x.shape[0]
    xl = x.astype(dtype)
    with np.errstate(invalid='ignore'):
        mean = xl.sum(axis=0) / dtype(m)
        s = np.sqrt(((xl - mean) ** 2).sum(axis=0) / dtype(m - 1))
    f = dtype(m) ** dtype(-0.2) if bw == 'scott' else (dtype(0.75) * m) ** dtype(-0.2) if bw == 'silverman' else dtype(bw)
    h = f * s
    h[~np.isfinite(s) | (s == 0)] = np.nan
    return h


def kde_direct(x, grid, inv_h, scale, dtype=np.longdouble):
    """x (m,), grid (G,), inv_h and scale as the kernel gets them (float64) -> kde (G,), sw = sum_t w_t, saw = sum_t a_t w_t,
    amax = max_t a_t per grid point, with a_t = ((g - x_t) inv_h)^2 / 2 and w_t = exp(-a_t), all in `dtype`; the difference
    g - x_t is formed first"""
    xl, ih = x.astype(dtype), dtype(inv_h)
    out, sw, saw, amax = (np.empty(grid.size, dtype) for _ in range(4))
    for q, g in enumerate(grid.astype(dtype)):
        z = (g - xl) * ih
        a = z * z / 2
        w = np.exp(-a)
        sw[q], saw[q], amax[q] = w.sum(), (a * w).sum(), a.max()
        out[q] = dtype(scale) * sw[q]
    return out, sw, saw, amax


def kde(x, grid, bw='scott', dtype=np.float64):
    """the formula in plain numpy: x (m,) finite draws, grid (G,) -> density (G,)"""
    m = x.size
    h = bandwidth(x[:, None], bw, dtype)[0]
    z = (grid[:, None].astype(dtype) - x[None, :].astype(dtype)) / h
    return np.exp(-z * z / 2).sum(axis=1) / (m * h * np.sqrt(2 * dtype(np.pi)))


def credible_levels(table, mass=(0.5, 0.9)):
    c = np.sort(np.asarray(table, dtype=np.int64).ravel())[::-1]
    cs = np.cumsum(c)
    if cs[-1] == 0:
        return np.zeros(len(mass), np.int64)
    return np.array([c[min(np.searchsorted(cs, p * cs[-1]), c.size - 1)] for p in mass], dtype=np.int64)


def corner(samples, select=None, burnin=0.1, bins=15, cmin=0, points=256, bw='scott', mass=(0.5, 0.9)):
    """the assembly of marginals.corner from the pieces above (float64 edges and grids; mean and cov in long double)"""
    x = pool(samples, burnin)
    if select is not None:
        x = x[:, list(select)]
    m, d = x.shape
    edges = make_edges(x, bins)
    h1, h2, dropped, nonfinite = histograms(x, edges)
    lo, hi = edges[:, 0], edges[:, -1]
    grid = np.stack([np.linspace(np.min(x[np.isfinite(x[:, i]), i]), np.max(x[np.isfinite(x[:, i]), i]), points) for i in range(d)])
    xl = x.astype(np.longdouble)
    mean = xl.sum(axis=0) / m
    y = xl - mean
    cov = y.T @ y / (m - 1)
    sd = np.sqrt(np.diag(cov))
    levels = np.stack([np.stack([credible_levels(h2[i, j], mass) for j in range(d)]) for i in range(d)])
    return dict(edges=edges, hist1d=h1, hist2d=h2, dropped=dropped, nonfinite=nonfinite, n_draws=m, grid=grid,
                bandwidth=bandwidth(x, bw), mask=h2 < cmin, mean=mean, cov=cov, corr=cov / np.outer(sd, sd), levels=levels,
                abs_cov=np.abs(y).T @ np.abs(y), abs_x=np.abs(xl).sum(axis=0), lo=lo, hi=hi)
