"""Corner-plot marginals of an MCMC trace: 1-D histograms, pair counts in square or hexagonal bins, Gaussian kernel density
estimates, credible levels.

What the reference's calibration publishes: `show_mcmc` ends in `uq.ndscatter(samples, plot2d='hist', cov_overlay=cov)`
(scripts/pem_v0/mcmc.py:339-340) and `journal_plots` is three calls of `uq.ndscatter(samples[:, idx_use], plot1d='kde',
plot2d='hex', bins=15, cmin=int(0.0015 * n))` (mcmc.py:351-385).  `uqtils` is third-party and absent: parity with ndscatter is
UNPINNED.  This module returns the arrays such a figure is drawn from (plotting itself is out of scope), under definitions
that make numpy, scipy and matplotlib exact yardsticks, stated once here and once in tests/marginals_np.py (the hexagons:
tests/hexbin_np.py):

  draws         drop b = int(burnin * n) rows; the remaining n' rows of all K chains are pooled into m = n' K draws of d
                parameters.
  edges         edges[i] = np.linspace(lo_i, hi_i, bins + 1), computed on the host and handed to the kernel as a table.
                (lo_i, hi_i) = (min, max) over the finite pooled draws of parameter i (numpy's range=None) unless `ranges`
                gives them; lo_i == hi_i is widened to (lo - 0.5, hi + 0.5) as numpy does; a parameter without a finite draw
                gets (0, 1).
  bin rule      v is in bin k iff edges[k] <= v < edges[k+1], the last bin also taking v == edges[bins]; anything else
                (outside the range, NaN, +-inf) is in no bin: np.histogram's and np.histogramdd's rule.  The kernel decides
                by comparing against the edge table (pem_chain_hist_f64_dev, csrc/pem_marginals.hip).
  counts        hist1d[i][k] = draws with parameter i in bin k.  hist2d[i][j][ki][kj], i < j = draws with parameter i in bin
                ki AND parameter j in bin kj (np.histogram2d with range= given): a draw with either value in no bin is dropped
                from that pair only.  dropped[i] = draws of parameter i in no bin, nonfinite[i] = how many of those were NaN
                or inf.  64-bit integers, exact.
  density       with the finite draws x_t, grid points g_q (default np.linspace(min, max, points)), bandwidth h = f s, s the
                sample standard deviation (ddof 1) of the pooled draws, f = m^(-1/5) for bw='scott', (3 m / 4)^(-1/5) for
                'silverman', or a given float factor:
                    kde[i][q] = 1 / (m h sqrt(2 pi)) * sum_t exp(-((g_q - x_t) / h)^2 / 2)
                which is scipy.stats.gaussian_kde(x, bw_method=...)(g) in one dimension; the sum is direct and untruncated
                (pem_chain_kde_f64_dev).  s == 0 or any non-finite draw makes that parameter's kde and bandwidth NaN.
  levels        for a 2-D count table and a mass p: the cell counts sorted descending and accumulated; the level is the count
                of the first cell at which the cumulative count is >= p * total (0 for an empty table).  Host, numpy.
  hexagons      matplotlib's `Axes.hexbin(x_i, x_j, C=None, gridsize=(nx, ny), extent=(lo_i, hi_i, lo_j, hi_j))`, linear scales,
                for the pairs (i, j), i < j, in the order (0,1), (0,2) ... (d-2,d-1): parameter i is the x and j the y
                coordinate (the panel in row j, column i of a corner plot; the table is not symmetric in its axes, so only
                i < j exists).  An int gridsize nx gives ny = int(nx / sqrt(3)); 1 <= nx, ny <= 64.  The extent (lo, hi) of a
                parameter is the finite (min, max) of the pooled draws unless `extent` gives it; lo == hi is widened to
                (lo - 0.5, hi + 0.5) (matplotlib's own default uses `nonsingular` here, which differs for degenerate data
                only).  Lattice constants per parameter, in numpy on the host, in exactly this order:
                    pad = 1e-9 * (hi - lo);  x0 = lo - pad;  sx = ((hi + pad) - x0) / nx;  y0 = lo;  sy = (hi - lo) / ny
                (matplotlib pads x only).  A draw (x, y) of a pair, every operation rounded once, none contracted:
                    ix = (x - x0_i) / sx_i             iy = (y - y0_j) / sy_j
                    r1 = rint(ix)  (half to even)      s1 = rint(iy)
                    r2 = floor(ix)                     s2 = floor(iy)
                    d1 = (ix - r1)^2 + 3.0 * (iy - s1)^2
                    d2 = (ix - r2 - 0.5)^2 + 3.0 * (iy - s2 - 0.5)^2
                    d1 <  d2: counted in cell r1 * (ny + 1) + s1            iff 0 <= r1 <= nx and 0 <= s1 <= ny
                    else    : counted in cell (nx+1)(ny+1) + r2 * ny + s2   iff 0 <= r2 <  nx and 0 <= s2 <  ny
                n_cells = (nx+1)(ny+1) + nx ny.  A draw whose chosen cell is out of range, or with a NaN or infinite value in
                either coordinate (matplotlib casts those to int, which is undefined), is dropped from that pair only; the
                range tests are made on the floating-point r, s; ties d1 == d2 go to the second lattice.  64-bit integers,
                exact (pem_chain_hex_f64_dev, csrc/pem_hexbin.hip).  Geometry, host, numpy, with matplotlib's operations so
                that it equals get_offsets(): centres (x0 + a sx, y0 + b sy), a in 0..nx, b in 0..ny, then
                (x0 + (a + 0.5) sx, y0 + (b + 0.5) sy), a < nx, b < ny; the polygon [sx, sy / 3] * [[.5, -.5], [.5, .5],
                [0, 1], [-.5, .5], [-.5, -.5], [0, -1]].  hexbin's `mincnt=k` blanks exactly the cells with counts < k.
                The 2-D Gaussian KDE of a pair stays out: scipy's definition is a direct sum over every draw per grid point.

Inputs as in `diagnostics`: `samples` is (n, K, d) or (n, d).  A CUDA fp64 tensor whose rows after burn-in form one (m, d)
matrix with unit column stride (a contiguous (n, K, d) trace; an (n, d) trace with any row stride) is read in place and the
results stay on its device; another CUDA tensor is copied once on its device.  Anything else is copied once to the current
device and the results come back as numpy.  There is no CPU path.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .diagnostics import _check, _device_view, _out, autocovariance

# what `import *` gives is pinned by tests/test_marginals_host.py; `hexbins` and `hex_lattice` are public too, taken by name
__all__ = ['histograms', 'kde', 'credible_levels', 'corner']

_COV_ROWS = 4096            # rows per product of corner()'s covariance


# ---------------------------------------------------------------------------------------------------------------- checks

def _check_bins(bins, d):
    if int(bins) != bins or not 1 <= bins <= _lib.MARGINALS_MAX_BINS:
        raise ValueError(f'bins must be an integer in 1 ... {_lib.MARGINALS_MAX_BINS}, got {bins}')
    if d > _lib.MARGINALS_MAX_PAR:
        raise ValueError(f'{d} parameters: at most {_lib.MARGINALS_MAX_PAR} per call (select a subset)')
    return int(bins)


def _check_ranges(ranges, d):
    if ranges is None:
        return None
    r = np.asarray(ranges, dtype=np.float64)
    if r.shape != (d, 2) or not np.all(np.isfinite(r)) or np.any(r[:, 0] > r[:, 1]):
        raise ValueError(f'ranges must be ({d}, 2) finite (lo, hi) with lo <= hi')
    return r


def _check_gridsize(gridsize, d):
    """(nx, ny) of an int or a pair, as matplotlib's hexbin reads it"""
    if d < 2:
        raise ValueError('hexagonal pair bins need at least 2 parameters')
    if d > _lib.MARGINALS_MAX_PAR:
        raise ValueError(f'{d} parameters: at most {_lib.MARGINALS_MAX_PAR} per call (select a subset)')
    try:
        if np.iterable(gridsize):
            nx, ny = gridsize
            if int(nx) != nx or int(ny) != ny:
                raise TypeError
            nx, ny = int(nx), int(ny)
        else:
            if isinstance(gridsize, bool) or int(gridsize) != gridsize:
                raise TypeError
            nx = int(gridsize)
            ny = int(nx / math.sqrt(3))
    except (TypeError, ValueError):
        raise ValueError(f'gridsize must be an integer nx or a pair (nx, ny) of integers, got {gridsize!r}') from None
    if not (1 <= nx <= _lib.HEX_MAX_GRID and 1 <= ny <= _lib.HEX_MAX_GRID):
        raise ValueError(f'gridsize {gridsize!r} gives nx = {nx}, ny = {ny}: both must lie in 1 ... {_lib.HEX_MAX_GRID}')
    return nx, ny


def _check_extent(extent, d):
    if extent is None:
        return None
    try:
        r = np.asarray(extent, dtype=np.float64)
    except (TypeError, ValueError):
        r = np.empty(0)
    if r.shape != (d, 2) or not np.all(np.isfinite(r)) or np.any(r[:, 0] > r[:, 1]):
        raise ValueError(f'extent must be ({d}, 2) finite (lo, hi) with lo <= hi')
    return r


def _check_kde(points, grid, bw, d):
    if d > _lib.MARGINALS_MAX_PAR:
        raise ValueError(f'{d} parameters: at most {_lib.MARGINALS_MAX_PAR} per call (select a subset)')
    if isinstance(bw, str):
        if bw not in ('scott', 'silverman'):
            raise ValueError(f"bw must be 'scott', 'silverman' or a positive factor, got {bw!r}")
    elif not (isinstance(bw, (int, float, np.floating, np.integer)) and math.isfinite(bw) and bw > 0):
        raise ValueError(f"bw must be 'scott', 'silverman' or a positive factor, got {bw!r}")
    if grid is None:
        if int(points) != points or not 1 <= points <= _lib.KDE_MAX_GRID:
            raise ValueError(f'points must be an integer in 1 ... {_lib.KDE_MAX_GRID}, got {points}')
        return None
    g = grid.detach().cpu().numpy() if hasattr(grid, 'detach') else np.asarray(grid)
    g = np.asarray(g, dtype=np.float64)
    if g.ndim == 1:
        g = np.broadcast_to(g, (d, g.size))
    if g.ndim != 2 or g.shape[0] != d or not 1 <= g.shape[1] <= _lib.KDE_MAX_GRID:
        raise ValueError(f'grid must be (G,) or ({d}, G) with 1 <= G <= {_lib.KDE_MAX_GRID}, got shape {g.shape}')
    return np.ascontiguousarray(g)


def _select(select, names, d):
    if select is None:
        return None
    idx = []
    for s in select:
        if isinstance(s, str):
            if names is None or s not in list(names):
                raise ValueError(f'select: no parameter named {s!r}')
            idx.append(list(names).index(s))
        else:
            if int(s) != s or not -d <= s < d:
                raise ValueError(f'select: index {s} outside {d} parameters')
            idx.append(int(s) % d)
    if not idx:
        raise ValueError('select: empty selection')
    return idx


# ---------------------------------------------------------------------------------------------------------- device layer

def _pooled(flat, K, d):
    """(n', K*d) view -> the pooled (m, d) draws, in place when the rows form one matrix of row stride d (or K == 1)"""
    if K == 1:
        return flat
    if flat.stride(0) != K * d:
        flat = flat.contiguous()
    return flat.view(-1, d)


def _finite_minmax(pooled):
    """(lo, hi) numpy (d,) over the finite draws; a parameter without one gets (0, 1).  A masked copy of the trace is made
    only when some draw is not finite."""
    import torch
    lo, hi = pooled.amin(dim=0), pooled.amax(dim=0)
    if not (torch.isfinite(lo).all() and torch.isfinite(hi).all()):
        ok = torch.isfinite(pooled)
        lo = torch.where(ok, pooled, torch.full_like(pooled, math.inf)).amin(dim=0)
        hi = torch.where(ok, pooled, torch.full_like(pooled, -math.inf)).amax(dim=0)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    none = lo > hi
    return np.where(none, 0.0, lo), np.where(none, 1.0, hi)


def _edges(pooled, bins, ranges, minmax=None):
    if ranges is None:
        lo, hi = _finite_minmax(pooled) if minmax is None else minmax
    else:
        lo, hi = ranges[:, 0].copy(), ranges[:, 1].copy()
    same = lo == hi
    lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
    return np.stack([np.linspace(a, b, bins + 1) for a, b in zip(lo, hi)])


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _hist_dev(pooled, edges, pairs):
    """pem_chain_hist_f64_dev on the pooled (m, d) CUDA view -> hist1d (d, bins), hist2d (d (d-1)/2, bins, bins) or None,
    dropped (d,), nonfinite (d,): int64 CUDA tensors"""
    import torch
    m, d = pooled.shape
    bins = edges.shape[1] - 1
    dev = pooled.device
    e = torch.as_tensor(edges, device=dev)
    h1 = torch.empty((d, bins), dtype=torch.int64, device=dev)
    h2 = torch.empty((d * (d - 1) // 2, bins, bins), dtype=torch.int64, device=dev) if pairs else None
    drop = torch.empty(d, dtype=torch.int64, device=dev)
    nonf = torch.empty(d, dtype=torch.int64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.pem_chain_hist_f64_dev(m, d, int(pooled.stride(0)), _ptr(pooled), bins, _ptr(e), _ptr(h1),
                                              _ptr(h2) if pairs and h2.numel() else None, _ptr(drop), _ptr(nonf), stream))
    return h1, h2, drop, nonf


def _full_hist2d(h1, h2):
    """(d, d, bins, bins): [i, j] for i < j from the pair tables, [j, i] its transpose, hist1d on the diagonal of [i, i]"""
    import torch
    d, bins = h1.shape
    full = torch.zeros((d, d, bins, bins), dtype=torch.int64, device=h1.device)
    iu = torch.triu_indices(d, d, 1, device=h1.device)
    if iu.shape[1]:
        full[iu[0], iu[1]] = h2
        full[iu[1], iu[0]] = h2.transpose(1, 2)
    ar = torch.arange(d, device=h1.device)
    full[ar, ar] = torch.diag_embed(h1)
    return full


def _histograms(pooled, bins, ranges, pairs, minmax=None):
    edges = _edges(pooled, bins, ranges, minmax)
    h1, h2, drop, nonf = _hist_dev(pooled, edges, pairs)
    return {'edges': edges, 'hist1d': h1, 'hist2d': _full_hist2d(h1, h2) if pairs else None, 'dropped': drop, 'nonfinite': nonf,
            'n_draws': int(pooled.shape[0])}


def _hex_extent(pooled, extent, minmax=None):
    """(d, 2) numpy: the given extent or the finite (min, max); lo == hi widened by 0.5 either side, as _edges does"""
    if extent is None:
        lo, hi = _finite_minmax(pooled) if minmax is None else minmax
    else:
        lo, hi = extent[:, 0], extent[:, 1]
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    same = lo == hi
    return np.stack([np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)], axis=1)


def _hex_table(extent, nx, ny):
    """(d, 4) numpy {x0, sx, y0, sy} per parameter, formed as matplotlib's hexbin forms them (the x axis padded, y not)"""
    lo, hi = extent[:, 0], extent[:, 1]
    pad = 1e-9 * (hi - lo)
    x0 = lo - pad
    sx = ((hi + pad) - x0) / nx
    y0 = lo
    sy = (hi - lo) / ny
    return np.ascontiguousarray(np.stack([x0, sx, y0, sy], axis=1), dtype=np.float64)


def hex_lattice(nx, ny, xlim, ylim):
    """Geometry of one hexbin table, numpy: (centers (n_cells, 2), polygon (6, 2)) for x in xlim = (lo, hi) and y in ylim,
    equal to matplotlib's get_offsets() and to the hexagon it draws around each offset: the (nx+1)(ny+1) centres of the first
    lattice (x0 + a sx, y0 + b sy), a outer, then the nx ny of the second (x0 + (a + 0.5) sx, y0 + (b + 0.5) sy)."""
    nx, ny = int(nx), int(ny)
    if nx < 1 or ny < 1:
        raise ValueError(f'need nx, ny >= 1, got {nx}, {ny}')
    (x0, sx, _, _), (_, _, y0, sy) = _hex_table(np.array([xlim, ylim], dtype=np.float64), nx, ny)
    n1 = (nx + 1) * (ny + 1)
    c = np.zeros((n1 + nx * ny, 2))
    c[:n1, 0] = np.repeat(np.arange(nx + 1), ny + 1)
    c[:n1, 1] = np.tile(np.arange(ny + 1), nx + 1)
    c[n1:, 0] = np.repeat(np.arange(nx) + 0.5, ny)
    c[n1:, 1] = np.tile(np.arange(ny), nx) + 0.5
    c[:, 0] *= sx
    c[:, 1] *= sy
    c[:, 0] += x0
    c[:, 1] += y0
    polygon = [sx, sy / 3] * np.array([[.5, -.5], [.5, .5], [0., 1.], [-.5, .5], [-.5, -.5], [0., -1.]])
    return c, polygon


def _hex_dev(pooled, nx, ny, table):
    """pem_chain_hex_f64_dev on the pooled (m, d) CUDA view; table (d, 4) numpy -> counts (d (d-1)/2, n_cells) int64 CUDA"""
    import torch
    m, d = pooled.shape
    table = np.ascontiguousarray(table, dtype=np.float64)
    counts = torch.empty((d * (d - 1) // 2, (nx + 1) * (ny + 1) + nx * ny), dtype=torch.int64, device=pooled.device)
    lib = _lib.load()
    with torch.cuda.device(pooled.device):
        stream = C.c_void_p(torch.cuda.current_stream(pooled.device).cuda_stream)
        _lib.check(lib.pem_chain_hex_f64_dev(m, d, int(pooled.stride(0)), _ptr(pooled), nx, ny, C.c_void_p(table.ctypes.data),
                                             _ptr(counts), stream))
    return counts


def _hexbins(pooled, nx, ny, extent, minmax=None):
    d = pooled.shape[1]
    extent = _hex_extent(pooled, extent, minmax)
    counts = _hex_dev(pooled, nx, ny, _hex_table(extent, nx, ny))
    pairs = np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int64)
    geom = [hex_lattice(nx, ny, extent[i], extent[j]) for i, j in pairs]
    return {'nx': nx, 'ny': ny, 'extent': extent, 'pairs': pairs, 'counts': counts, 'n_draws': int(pooled.shape[0]),
            'centers': np.stack([g[0] for g in geom]), 'polygon': np.stack([g[1] for g in geom])}


_HEX_PLAIN = ('nx', 'ny', 'n_draws')            # python ints of a hexbins result; everything else is an array


def _bandwidth(pooled, bw):
    """(h, inv_h, scale) numpy (d,): s from the pooled mean and gamma(0) of pem_chain_autocov_f64_dev, the rest on the host"""
    m = int(pooled.shape[0])
    _, acov = autocovariance(pooled, 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = np.sqrt(acov[0, 0].cpu().numpy() * (m / (m - 1)))
        f = m ** -0.2 if bw == 'scott' else (0.75 * m) ** -0.2 if bw == 'silverman' else float(bw)
        h = f * s
        bad = ~np.isfinite(s) | (s == 0)
        h[bad] = np.nan
        inv_h = 1.0 / h
        scale = inv_h / (m * math.sqrt(2.0 * math.pi))
    return h, inv_h, scale


def _kde_dev(pooled, grid, inv_h, scale):
    """pem_chain_kde_f64_dev on the pooled (m, d) CUDA view; grid (d, G), inv_h, scale (d,) numpy -> kde (d, G) CUDA"""
    import torch
    m, d = pooled.shape
    G = grid.shape[1]
    dev = pooled.device
    g, ih, sc = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev) for a in (grid, inv_h, scale))
    out = torch.empty((d, G), dtype=torch.float64, device=dev)
    work = torch.empty(-(-m // _lib.KDE_ROW_BLOCK) * d * G, dtype=torch.float64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.pem_chain_kde_f64_dev(m, d, int(pooled.stride(0)), _ptr(pooled), G, _ptr(g), _ptr(ih), _ptr(sc), _ptr(out),
                                             _ptr(work), work.numel(), stream))
    return out


def _kde(pooled, points, grid, bw, minmax=None):
    if grid is None:
        lo, hi = _finite_minmax(pooled) if minmax is None else minmax
        grid = np.stack([np.linspace(a, b, int(points)) for a, b in zip(lo, hi)])
    h, inv_h, scale = _bandwidth(pooled, bw)
    return grid, _kde_dev(pooled, grid, inv_h, scale), h


# ---------------------------------------------------------------------------------------------------------------- public

def histograms(samples, bins: int = 15, ranges=None, burnin: float = 0.1, pairs: bool = True):
    """1-D and pair counts of the pooled draws after burn-in: dict with `edges` (d, bins+1), `hist1d` (d, bins), `hist2d`
    (d, d, bins, bins) (filled for i < j; [j, i] is the transpose of [i, j]; [i, i] holds hist1d[i] on its diagonal; None
    when `pairs` is false), `dropped` (d,), `nonfinite` (d,), `n_draws`.  `ranges`: (d, 2) of (lo, hi) instead of the
    finite (min, max).  At most 32 parameters and 64 bins."""
    n, K, d, b = _check(samples, burnin)
    bins = _check_bins(bins, d)
    ranges = _check_ranges(ranges, d)
    flat, K, d, host = _device_view(samples, b)
    r = _histograms(_pooled(flat, K, d), bins, ranges, bool(pairs))
    return {k: (v if v is None or k == 'n_draws' else _out(v, host, flat)) for k, v in r.items()}


def hexbins(samples, gridsize=15, extent=None, burnin: float = 0.1):
    """Hexagonal pair counts of the pooled draws after burn-in, matplotlib's `hexbin` for every pair (i, j), i < j, with
    parameter i on x and j on y: dict with `nx`, `ny`, `extent` (d, 2), `pairs` (P, 2), `counts` (P, n_cells) int64 in the
    order of hexbin's get_array(), `n_draws`, and the geometry `centers` (P, n_cells, 2) (get_offsets()) and `polygon`
    (P, 6, 2).  `gridsize`: nx (then ny = int(nx / sqrt(3))) or (nx, ny), each in 1 ... 64; `extent`: (d, 2) of (lo, hi)
    instead of the finite (min, max).  2 to 32 parameters."""
    n, K, d, b = _check(samples, burnin)
    nx, ny = _check_gridsize(gridsize, d)
    extent = _check_extent(extent, d)
    flat, K, d, host = _device_view(samples, b)
    r = _hexbins(_pooled(flat, K, d), nx, ny, extent)
    return {k: (v if k in _HEX_PLAIN else _out(v, host, flat)) for k, v in r.items()}


def kde(samples, points: int = 256, grid=None, bw='scott', burnin: float = 0.1):
    """Gaussian kernel density estimate of every parameter from the pooled draws after burn-in: (grid (d, G), density (d, G),
    bandwidth (d,)).  `grid`: (G,) for every parameter or (d, G), instead of np.linspace(min, max, points); `bw`: 'scott',
    'silverman' or a factor f (h = f * std).  A direct sum over every draw."""
    n, K, d, b = _check(samples, burnin)
    grid = _check_kde(points, grid, bw, d)
    flat, K, d, host = _device_view(samples, b)
    g, dens, h = _kde(_pooled(flat, K, d), points, grid, bw)
    return _out(g, host, flat), _out(dens, host, flat), _out(h, host, flat)


def credible_levels(hist2d, mass=(0.5, 0.9)):
    """Count levels enclosing the given posterior masses: for a table (bins, bins) -> (len(mass),) int64; for a stack
    (..., bins, bins) -> (..., len(mass)).  Host, numpy: the cell counts sorted descending and accumulated; the level of
    mass p is the count of the first cell at which the cumulative count is >= p * total; 0 for an empty table."""
    h = np.asarray(hist2d.cpu() if hasattr(hist2d, 'cpu') else hist2d)
    if h.ndim < 2:
        raise ValueError(f'hist2d must be (..., bins, bins), got shape {h.shape}')
    mass = tuple(float(p) for p in mass)
    if not all(0.0 < p <= 1.0 for p in mass):
        raise ValueError(f'mass must lie in (0, 1], got {mass}')
    lead = h.shape[:-2]
    flat = h.reshape((-1, h.shape[-2] * h.shape[-1])).astype(np.int64)
    out = np.zeros((flat.shape[0], len(mass)), dtype=np.int64)
    for t, cells in enumerate(flat):
        c = np.sort(cells)[::-1]
        cs = np.cumsum(c)
        if cs[-1] == 0:
            continue
        for k, p in enumerate(mass):
            out[t, k] = c[min(int(np.searchsorted(cs, p * cs[-1])), c.size - 1)]
    return out.reshape(lead + (len(mass),))


def corner(samples, names=None, select=None, burnin: float = 0.1, bins: int = 15, cmin: int = 0, points: int = 256, bw='scott',
           mass=(0.5, 0.9), plot2d: str = 'hist', gridsize=None):
    """Everything one `uq.ndscatter` call draws, for the selected parameters (`select`: names or indices, as journal_plots'
    str_use; the columns are gathered once on the device): the results of `histograms` and `kde` (`grid`, `density`,
    `bandwidth`), `mask` = hist2d < cmin (matplotlib's cmin / hexbin's mincnt: cells with fewer draws are blanked;
    journal_plots uses int(0.0015 * n_draws)), the pooled `mean` (d,), `cov` (d, d) (ddof 1) and `corr` for the covariance
    overlay, and `levels` (d, d, len(mass)) (numpy; credible_levels of every table), with `names` and `mass`.
    `plot2d='hex'` (journal_plots' choice) adds `hex`: the `hexbins` result for the selected parameters over the same finite
    (min, max), with `mask` = counts < cmin (P, n_cells) and `levels` (P, len(mass)); `gridsize` None means `bins`, as
    ndscatter hands `bins` to both.  With the default 'hist' nothing else changes."""
    import torch
    if plot2d not in ('hist', 'hex'):
        raise ValueError(f"plot2d must be 'hist' or 'hex', got {plot2d!r}")
    n, K, d, b = _check(samples, burnin)
    if names is not None and len(names) != d:
        raise ValueError(f'{len(names)} names for {d} parameters')
    idx = _select(select, names, d)
    dsel = d if idx is None else len(idx)
    bins = _check_bins(bins, dsel)
    _check_kde(points, None, bw, dsel)
    if plot2d == 'hex':
        nx, ny = _check_gridsize(bins if gridsize is None else gridsize, dsel)
    if int(cmin) != cmin or cmin < 0:
        raise ValueError(f'cmin must be a non-negative integer, got {cmin}')
    mass = tuple(float(p) for p in mass)
    if not all(0.0 < p <= 1.0 for p in mass):
        raise ValueError(f'mass must lie in (0, 1], got {mass}')
    flat, K, d, host = _device_view(samples, b)
    pooled = _pooled(flat, K, d)
    if idx is not None:
        pooled = pooled[:, torch.as_tensor(idx, device=pooled.device)]
    minmax = _finite_minmax(pooled)                          # one pass for the edges and the grids
    out = _histograms(pooled, bins, None, True, minmax)
    out['grid'], out['density'], out['bandwidth'] = _kde(pooled, points, None, bw, minmax)
    m = pooled.shape[0]
    mean = pooled.mean(dim=0)
    y = pooled - mean
    nb = m // _COV_ROWS                                  # a (d, m) x (m, d) product as a batch of short ones, then their sum
    head = y[:nb * _COV_ROWS].view(nb, _COV_ROWS, y.shape[1])
    cov = (torch.bmm(head.transpose(1, 2), head).sum(dim=0) + y[nb * _COV_ROWS:].T @ y[nb * _COV_ROWS:]) / (m - 1)
    sd = torch.sqrt(torch.diagonal(cov))
    out['mean'], out['cov'], out['corr'] = mean, cov, cov / torch.outer(sd, sd)
    out['mask'] = out['hist2d'] < int(cmin)
    levels = credible_levels(out['hist2d'], mass)
    for k, v in out.items():
        if k != 'n_draws':
            out[k] = _out(v, host, flat)
    all_names = list(names) if names is not None else [f'x{i}' for i in range(d)]
    out['names'] = all_names if idx is None else [all_names[i] for i in idx]
    out['levels'], out['mass'] = levels, mass
    if plot2d == 'hex':
        hx = _hexbins(pooled, nx, ny, None, minmax)
        hx['mask'] = hx['counts'] < int(cmin)
        hx_levels = credible_levels(hx['counts'][:, None, :], mass)        # the rule does not look at the shape of a cell
        out['hex'] = {k: (v if k in _HEX_PLAIN else _out(v, host, flat)) for k, v in hx.items()}
        out['hex']['levels'] = hx_levels
    return out
