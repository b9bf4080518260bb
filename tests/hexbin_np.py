"""numpy restatement of the hexagonal pair bins of hallthrusterpem_amd/marginals.py (matplotlib's `Axes.hexbin` with C=None, linear
scales, gridsize=(nx, ny) and extent= given), for the tests.  Read matplotlib/axes/_axes.py (`hexbin`) beside it.

  grid size     an int nx gives ny = int(nx / math.sqrt(3)); a pair is (nx, ny).
  extent        (lo, hi) per parameter: the finite (min, max) of the draws unless given; lo == hi widened to (lo - 0.5, hi + 0.5);
                no finite draw: (0, 1).
  lattice       per parameter, in this order: pad = 1e-9 * (hi - lo); x0 = lo - pad; sx = ((hi + pad) - x0) / nx; y0 = lo;
                sy = (hi - lo) / ny.  (matplotlib pads x only.)
  a draw        ix = (x - x0_i) / sx_i, iy = (y - y0_j) / sy_j; r1 = np.round(ix), s1 = np.round(iy), r2 = np.floor(ix),
                s2 = np.floor(iy); d1 = (ix - r1)**2 + 3.0 * (iy - s1)**2; d2 = (ix - r2 - 0.5)**2 + 3.0 * (iy - s2 - 0.5)**2.
                d1 < d2: cell r1 * (ny + 1) + s1 iff 0 <= r1 <= nx and 0 <= s1 <= ny; else cell (nx+1)(ny+1) + r2 * ny + s2 iff
                0 <= r2 < nx and 0 <= s2 < ny.  The range tests are made on the floating-point r, s, so NaN, +-inf and values
                beyond the integers are in no cell (matplotlib casts them, which is undefined); ties go to the second lattice.
  pairs         (i, j), i < j, in the order (0,1), (0,2) ... (d-2,d-1); parameter i is x, parameter j is y.
  geometry      matplotlib's own operations: centres (a * sx + x0, b * sy + y0) over a in 0..nx (outer), b in 0..ny, then
                ((a + 0.5) * sx + x0, (b + 0.5) * sy + y0) over a < nx (outer), b < ny; polygon [sx, sy / 3] * the six corners.
"""
import math

import numpy as np

CORNERS = np.array([[.5, -.5], [.5, .5], [0., 1.], [-.5, .5], [-.5, -.5], [0., -1.]])


def grid_size(gridsize):
    if np.iterable(gridsize):
        nx, ny = gridsize
        return int(nx), int(ny)
    return int(gridsize), int(gridsize / math.sqrt(3))


def n_cells(nx, ny):
    return (nx + 1) * (ny + 1) + nx * ny


def make_extent(x, extent=None):
    d = x.shape[1]
    out = np.empty((d, 2))
    for i in range(d):
        if extent is None:
            f = x[np.isfinite(x[:, i]), i]
            lo, hi = (f.min(), f.max()) if f.size else (0.0, 1.0)
        else:
            lo, hi = extent[i]
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        out[i] = lo, hi
    return out


def lattice_table(extent, nx, ny):
    """(d, 4): {x0, sx, y0, sy} per parameter"""
    extent = np.asarray(extent, dtype=np.float64)
    out = np.empty((extent.shape[0], 4))
    for i, (lo, hi) in enumerate(extent):
        pad = 1e-9 * (hi - lo)
        x0 = lo - pad
        out[i] = x0, ((hi + pad) - x0) / nx, lo, (hi - lo) / ny
    return out


def lattice_coordinates(v, origin, step):
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.asarray(v, dtype=np.float64) - origin) / step


def distances(ix, iy):
    """(d1, d2, r1, s1, r2, s2) of lattice coordinates, as written above"""
    with np.errstate(invalid='ignore', over='ignore'):
        r1, s1, r2, s2 = np.round(ix), np.round(iy), np.floor(ix), np.floor(iy)
        d1 = (ix - r1) ** 2 + 3.0 * (iy - s1) ** 2
        d2 = (ix - r2 - 0.5) ** 2 + 3.0 * (iy - s2 - 0.5) ** 2
    return d1, d2, r1, s1, r2, s2


def cells(x, y, nx, ny, xrow, yrow):
    """cell of every draw (x, y) under the lattice rows of its two parameters; -1 = no cell"""
    ix = lattice_coordinates(x, xrow[0], xrow[1])
    iy = lattice_coordinates(y, yrow[2], yrow[3])
    d1, d2, r1, s1, r2, s2 = distances(ix, iy)
    first = d1 < d2
    in1 = first & (0 <= r1) & (r1 <= nx) & (0 <= s1) & (s1 <= ny)
    in2 = ~first & (0 <= r2) & (r2 < nx) & (0 <= s2) & (s2 < ny)
    out = np.full(ix.shape, -1, dtype=np.int64)
    out[in1] = r1[in1].astype(np.int64) * (ny + 1) + s1[in1].astype(np.int64)
    out[in2] = (nx + 1) * (ny + 1) + r2[in2].astype(np.int64) * ny + s2[in2].astype(np.int64)
    return out


def counts_of_pair(x, y, nx, ny, xrow, yrow):
    c = cells(x, y, nx, ny, xrow, yrow)
    return np.bincount(c[c >= 0], minlength=n_cells(nx, ny)).astype(np.int64)


def pair_list(d):
    return np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int64).reshape(-1, 2)


def hexbins(x, nx, ny, extent=None, table=None):
    """x (m, d) pooled draws, extent (d, 2) or a ready lattice table (d, 4) -> counts (d (d-1)/2, n_cells) int64"""
    if table is None:
        table = lattice_table(extent, nx, ny)
    return np.stack([counts_of_pair(x[:, i], x[:, j], nx, ny, table[i], table[j]) for i, j in pair_list(x.shape[1])])


def geometry(nx, ny, xlim, ylim):
    """(centers (n_cells, 2), polygon (6, 2)) of the table of x in xlim, y in ylim"""
    (x0, sx, _, _), (_, _, y0, sy) = lattice_table([xlim, ylim], nx, ny)
    n1 = (nx + 1) * (ny + 1)
    c = np.zeros((n_cells(nx, ny), 2))
    c[:n1, 0] = np.repeat(np.arange(nx + 1), ny + 1)
    c[:n1, 1] = np.tile(np.arange(ny + 1), nx + 1)
    c[n1:, 0] = np.repeat(np.arange(nx) + 0.5, ny)
    c[n1:, 1] = np.tile(np.arange(ny), nx) + 0.5
    c[:, 0] *= sx
    c[:, 1] *= sy
    c[:, 0] += x0
    c[:, 1] += y0
    return c, [sx, sy / 3] * CORNERS


def dropped_of_pair(x, y, nx, ny, xrow, yrow):
    return int((cells(x, y, nx, ny, xrow, yrow) < 0).sum())


def adversarial_draws(nx, ny, xlim, ylim, rng, n_random=3000, cap=120_000):
    """(x, y) finite draws for the table of x in xlim, y in ylim: random draws inside and around the extent; every lattice
    coordinate q = 0, 0.25, 0.5 ... (lattice points, the rint ties at half-integers, the quarter points where the two
    lattices are equally far) and its two neighbours in fp64, in both axes, paired in full when that is at most `cap` draws
    and by `cap` random pairs otherwise; each side and corner of the extent, of the padded extent, and their neighbours."""
    (x0, sx, _, _), (_, _, y0, sy) = lattice_table([xlim, ylim], nx, ny)

    def around(v):
        v = np.asarray(v, dtype=np.float64)
        return np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])
    qx = around(x0 + np.arange(-0.5, nx + 0.75, 0.25) * sx)
    qy = around(y0 + np.arange(-0.5, ny + 0.75, 0.25) * sy)
    if qx.size * qy.size <= cap:
        gx, gy = np.repeat(qx, qy.size), np.tile(qy, qx.size)
    else:
        gx, gy = qx[rng.integers(0, qx.size, cap)], qy[rng.integers(0, qy.size, cap)]
    (xl, xh), (yl, yh) = xlim, ylim
    ex = around([xl, xh, x0, x0 + nx * sx, xl - 0.3 * sx, xh + 0.3 * sx, xl - sx, xh + sx])
    ey = around([yl, yh, yl - 0.3 * sy, yh + 0.3 * sy, yl - 0.5 * sy, yh + 0.5 * sy, yl - sy, yh + sy])
    rx = rng.uniform(xl - 0.2 * (xh - xl), xh + 0.2 * (xh - xl), n_random)
    ry = rng.uniform(yl - 0.2 * (yh - yl), yh + 0.2 * (yh - yl), n_random)
    x = np.concatenate([rx, gx, np.repeat(ex, ey.size), rng.choice(qx, 2000), rx[:2000]])
    y = np.concatenate([ry, gy, np.tile(ey, ex.size), ry[:2000], rng.choice(qy, 2000)])
    order = rng.permutation(x.size)
    return x[order], y[order]
