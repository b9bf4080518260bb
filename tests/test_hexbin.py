"""Hexagonal pair bins on the MI355X: pem_chain_hex_f64_dev equal to tests/hexbin_np.py (which test_hexbin_host.py holds to
matplotlib's `Axes.hexbin` bit for bit) count for count over its dispatch space, on adversarial values, in place, run after
run, and marginals.corner(plot2d='hex') on a DeviceDRAM trace end to end.

Counts have no tolerance: np.array_equal on int64.
"""
import ctypes as C

import numpy as np
import pytest

import hexbin_np as ref
import marginals_np as mref
from hallthrusterpem_amd import _lib

pytestmark = pytest.mark.gpu

TILE = _lib.HEX_ROW_TILE
WGS = 1024                      # workgroups a launch aims at: floor(WGS / task blocks) row blocks
GRIDSIZES = [(1, 1), 2, 15, 64, (64, 64), (1, 64)]          # an int 1 would give ny = 0: ny is forced to 1


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _check(xh, x, gridsize, extent=None, table=None):
    """the entry point on the device view x against the restatement on the host copy xh"""
    from hallthrusterpem_amd import marginals
    nx, ny = ref.grid_size(gridsize)
    if table is None:
        table = ref.lattice_table(ref.make_extent(xh, extent), nx, ny)
    got = marginals._hex_dev(x, nx, ny, table).cpu().numpy()
    want = ref.hexbins(xh, nx, ny, table=table)
    assert got.dtype == np.int64 and got.shape == want.shape == (xh.shape[1] * (xh.shape[1] - 1) // 2, ref.n_cells(nx, ny))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad[:5], int(np.abs(got - want).sum()))
    return got


# ---- counts over the dispatch space

@pytest.mark.parametrize('n_par', [2, 3, 17, 32])
@pytest.mark.parametrize('gridsize', GRIDSIZES)
def test_counts_over_parameters_and_grid_sizes(n_par, gridsize):
    rng = np.random.default_rng(100 * n_par + sum(ref.grid_size(gridsize)))
    n = 700 if n_par > 2 else 3000
    xh = rng.standard_normal((n, n_par)) * rng.uniform(0.1, 10, n_par) + rng.uniform(-5, 5, n_par)
    got = _check(xh, _dev(xh), gridsize)
    assert np.all(got.sum(axis=1) > 0.9 * n)                    # the default extent holds every draw but those on its rim
    _check(xh, _dev(xh), gridsize, extent=[(-1.0 - i % 3, 2.0 + i % 5) for i in range(n_par)])


@pytest.mark.parametrize('n_rows', [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE, TILE * WGS - 1, TILE * WGS, TILE * WGS + 1,
                                    2 * TILE * WGS + TILE + 5])
def test_counts_around_the_row_tiles(n_rows):
    """TILE rows per stage; 3 pairs are one task block, so the launch has up to 1024 row blocks and past TILE * 1024 rows a
    workgroup walks more than one tile"""
    rng = np.random.default_rng(n_rows)
    xh = rng.standard_normal((n_rows, 3))
    _check(xh, _dev(xh), 15, extent=[(-1, 1), (-4, 4), (0, 0.5)])
    _check(xh, _dev(xh), (7, 5))


@pytest.mark.parametrize('n_rows', [TILE * (WGS // 4) - 1, TILE * (WGS // 4), TILE * (WGS // 4) + 1])
def test_counts_around_the_row_blocks_of_four_task_blocks(n_rows):
    """17 parameters at gridsize 15 are 136 tables of 264 cells in 4 task blocks of 34: 256 row blocks"""
    rng = np.random.default_rng(n_rows)
    xh = rng.standard_normal((n_rows, 17))
    _check(xh, _dev(xh), 15)


@pytest.mark.parametrize('n,S,pad,off', [(1000, 5, 0, 0), (1000, 5, 7, 1), (333, 17, 2, 3), (129, 2, 4, 1)])
def test_counts_of_a_strided_view(n, S, pad, off):
    rng = np.random.default_rng(n + S + off)
    wide = rng.standard_normal((n, S + pad + off))
    wide[:, :off], wide[:, off + S:] = np.nan, 1e300            # the padding must not be read
    xh = wide[:, off:off + S]
    x = _dev(wide)[:, off:off + S]
    assert x.stride(0) == S + pad + off and (x.data_ptr() % 16 == 8) == (off % 2 == 1)
    got = _check(xh, x, 15)
    assert np.all(got.sum(axis=1) > 0.9 * n)
    _check(xh, x, (3, 11), extent=[(-2.0, 1.5)] * S)


# ---- adversarial values

@pytest.mark.parametrize('gridsize', [(1, 1), (2, 1), (15, 8), (64, 36), (64, 64), (1, 64)])
def test_counts_on_lattice_points_rint_ties_and_the_rim_of_the_extent(gridsize):
    """the draws test_hexbin_host.py holds to matplotlib, as three parameters: (x, y), (x, y reversed), (y, y reversed)"""
    nx, ny = gridsize
    rng = np.random.default_rng(100 * nx + ny)
    xlim, ylim = (-1.3, 2.9), (1e-3, 1.7e-3)
    x, y = ref.adversarial_draws(nx, ny, xlim, ylim, rng)
    xh = np.stack([x, y, y[::-1]], axis=1)
    _check(xh, _dev(xh), gridsize, extent=[xlim, ylim, ylim])


def _tie_draws(nx, ny, sx, sy, x0, y0):
    """every (ix, iy) = (a + q, b + p) with q, p in {0.25, 0.75}: both lattices equally far, exactly, when the lattice steps
    are powers of two"""
    a = np.arange(-1, nx + 1)[:, None] + np.array([0.25, 0.75])
    b = np.arange(-1, ny + 1)[:, None] + np.array([0.25, 0.75])
    ix, iy = np.meshgrid(a.ravel(), b.ravel(), indexing='ij')
    return x0 + ix.ravel() * sx, y0 + iy.ravel() * sy


@pytest.mark.parametrize('nx,ny', [(1, 1), (15, 8), (64, 64)])
def test_exact_ties_go_to_the_second_lattice(nx, ny):
    sx, sy, x0, y0 = 0.5, 4.0, -3.0, 16.0
    x, y = _tie_draws(nx, ny, sx, sy, x0, y0)
    table = np.array([[x0, sx, x0, sx], [y0, sy, y0, sy]])
    d1, d2, _, _, r2, s2 = ref.distances(ref.lattice_coordinates(x, x0, sx), ref.lattice_coordinates(y, y0, sy))
    assert np.array_equal(d1, d2) and np.all(d1 == 0.25)                    # the restatement sees nothing but ties
    xh = np.stack([x, y], axis=1)
    got = _check(xh, _dev(xh), (nx, ny), table=table)
    n1 = (nx + 1) * (ny + 1)
    inside = (r2 >= 0) & (r2 < nx) & (s2 >= 0) & (s2 < ny)
    assert not got[0, :n1].any() and np.all(got[0, n1:] == 4) and got.sum() == inside.sum() == 4 * nx * ny


def test_values_beyond_the_integers_and_non_finite_values():
    """|ix| >= 2^31, 2^63 and near the largest double: in no cell, whatever a cast would have made of them"""
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(3)
    xh = rng.uniform(0, 1, (4000, 3))
    table = ref.lattice_table([(0.0, 1.0)] * 3, 15, 8)
    clean = ref.hexbins(xh, 15, 8, table=table)
    big = np.array([3e9, -3e9, 2.0 ** 31, -2.0 ** 31, 2.0 ** 62, 1e19, -1e19, 1e300, -1e300, 1.7e308, -1.7e308, np.inf, -np.inf, np.nan,
                    2.0 ** 31 / 16, 1e-320, -1e-320])
    assert abs(ref.lattice_coordinates(3e9, table[0, 0], table[0, 1])) >= 2.0 ** 31
    rows = rng.choice(4000, big.size, replace=False)
    xh[rows, 1] = big
    got = _check(xh, _dev(xh), (15, 8), table=table)
    assert np.array_equal(got[1], clean[1])                                 # pair (0, 2) does not hold parameter 1
    assert got[0].sum() == 4000 - (big.size - 2) and got[2].sum() == 4000 - (big.size - 2)     # the two denormals are at the origin
    assert marginals._hex_dev(_dev(np.full((5, 2), np.nan)), 3, 2, table[:2]).sum() == 0


def test_non_finite_values_poison_only_their_pairs():
    rng = np.random.default_rng(9)
    xh = rng.standard_normal((5000, 6))
    ext = [(-5, 5)] * 6
    clean = _check(xh, _dev(xh), 15, extent=ext)
    xh[rng.integers(0, 5000, 40), 1] = np.nan
    xh[rng.integers(0, 5000, 30), 4] = np.inf
    xh[rng.integers(0, 5000, 30), 4] = -np.inf
    got = _check(xh, _dev(xh), 15, extent=ext)
    for p, (i, j) in enumerate(ref.pair_list(6)):
        assert np.array_equal(got[p], clean[p]) == (1 not in (i, j) and 4 not in (i, j)), (i, j)
    n_bad = (~np.isfinite(xh[:, [1, 4]])).any(axis=1).sum()
    assert got[ref.pair_list(6).tolist().index([1, 4])].sum() == 5000 - n_bad
    _check(xh, _dev(xh), 15)                                    # default extent: the finite min and max


@pytest.mark.parametrize('n_par,gridsize', [(2, 15), (32, 15), (2, (64, 64)), (32, (1, 1))])
def test_counts_when_every_row_is_identical(n_par, gridsize):
    """every add of a table lands on one word"""
    row = np.random.default_rng(n_par).uniform(-3, 3, n_par)
    xh = np.tile(row, (20_000, 1))
    got = _check(xh, _dev(xh), gridsize, extent=[(-4, 4)] * n_par)
    assert np.all(got.max(axis=1) == 20_000) and np.all(got.sum(axis=1) == 20_000)
    _check(xh, _dev(xh), gridsize)                              # constant parameters: extents widened by 0.5 either side


def test_counts_of_a_rejecting_samplers_trace():
    rng = np.random.default_rng(8)
    xh = np.repeat(rng.standard_normal((3000, 17)), rng.integers(1, 60, 3000), axis=0)
    _check(xh, _dev(xh), 15)


def test_single_cells_beyond_16_and_24_bits():
    """2^24 + 3 identical rows of two parameters, and 70 000 rows of another value: cells above 65 535 and above 2^24"""
    import torch
    from hallthrusterpem_amd import marginals
    n_big, n_small = 2 ** 24 + 3, 70_000
    x = torch.empty((n_big + n_small, 2), dtype=torch.float64, device='cuda')
    x[:n_big] = torch.tensor([0.25, -1.5], dtype=torch.float64, device='cuda')
    x[n_big:] = torch.tensor([2.75, 1.5], dtype=torch.float64, device='cuda')
    table = ref.lattice_table([(0.0, 4.0), (-2.0, 2.0)], 4, 3)
    two = np.array([[0.25, -1.5], [2.75, 1.5]])
    ca, cb = ref.cells(two[:, 0], two[:, 1], 4, 3, table[0], table[1])
    assert ca >= 0 and cb >= 0 and ca != cb
    want = np.zeros((1, ref.n_cells(4, 3)), np.int64)
    want[0, ca], want[0, cb] = n_big, n_small
    assert np.array_equal(marginals._hex_dev(x, 4, 3, table).cpu().numpy(), want)


# ---- determinism, independence of the other parameters, in place

def test_repeat_runs_give_the_same_bits():
    import torch
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(18)
    x = _dev(np.repeat(rng.standard_normal((3000, 9)), rng.integers(1, 9, 3000), axis=0))
    table = ref.lattice_table(ref.make_extent(x.cpu().numpy()), 15, 8)
    a = marginals._hex_dev(x, 15, 8, table)
    for _ in range(3):
        assert torch.equal(a, marginals._hex_dev(x, 15, 8, table))


def test_a_pairs_table_does_not_depend_on_the_other_parameters():
    import torch
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(19)
    xh = rng.standard_normal((9000, 17)) * rng.uniform(0.1, 10, 17)
    xh[rng.integers(0, 9000, 50), 5] = np.nan
    table = ref.lattice_table(ref.make_extent(xh), 15, 8)
    whole = marginals._hex_dev(_dev(xh), 15, 8, table)
    pairs = ref.pair_list(17).tolist()
    for sel in ([0, 1], [3, 16], [2, 5, 11], [11, 2, 5], list(range(1, 17, 2))):
        part = marginals._hex_dev(_dev(xh[:, sel]), 15, 8, table[sel])
        for p, (i, j) in enumerate(ref.pair_list(len(sel))):
            if sel[i] < sel[j]:
                assert torch.equal(part[p], whole[pairs.index([sel[i], sel[j]])]), (sel, i, j)
    # 34 tables per workgroup at 17 parameters, 3 at 3: the same table from another task block and another lane mapping
    assert torch.equal(marginals._hex_dev(_dev(xh[:, [14, 15, 16]]), 15, 8, table[14:])[2], whole[-1])


def test_a_contiguous_trace_is_read_in_place(monkeypatch):
    import torch
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(20)
    n, K, d = 500, 6, 5
    trace = _dev(rng.standard_normal((n, K, d)))
    b = int(0.1 * n)
    lib = _lib.load()
    seen = {}
    real = lib.pem_chain_hex_f64_dev

    def spy(*args):
        seen['hex'] = (args[0], args[2], args[3].value)
        return real(*args)
    monkeypatch.setattr(lib, 'pem_chain_hex_f64_dev', spy, raising=False)
    r = marginals.hexbins(trace)
    assert seen['hex'] == ((n - b) * K, d, trace.data_ptr() + b * K * d * 8)
    assert all(isinstance(r[k], torch.Tensor) and r[k].is_cuda for k in ('extent', 'pairs', 'counts', 'centers', 'polygon'))
    assert r['counts'].dtype == torch.int64 and r['n_draws'] == (n - b) * K and (r['nx'], r['ny']) == (15, 8)
    pooled = mref.pool(trace.cpu().numpy())
    ext = ref.make_extent(pooled)
    assert np.array_equal(r['extent'].cpu().numpy(), ext) and np.array_equal(r['pairs'].cpu().numpy(), ref.pair_list(d))
    assert np.array_equal(r['counts'].cpu().numpy(), ref.hexbins(pooled, 15, 8, ext))
    for p, (i, j) in enumerate(ref.pair_list(d)):
        c, poly = ref.geometry(15, 8, ext[i], ext[j])
        assert np.array_equal(r['centers'][p].cpu().numpy(), c) and np.array_equal(r['polygon'][p].cpu().numpy(), poly)
    # the same draws as one chain of (n' K) rows in a wider buffer, starting at an odd column: a strided view, in place too
    wide = torch.zeros(((n - b) * K, d + 4), dtype=torch.float64, device='cuda')
    wide[:, 1:1 + d] = trace[b:].reshape(-1, d)
    view = wide[:, 1:1 + d]
    r2 = marginals.hexbins(view, burnin=0.0)
    assert seen['hex'] == ((n - b) * K, d + 4, view.data_ptr())
    assert all(torch.equal(r[k], r2[k]) for k in ('extent', 'pairs', 'counts', 'centers', 'polygon'))
    # numpy in -> numpy out, the same numbers; a given extent and a pair gridsize
    rh = marginals.hexbins(trace.cpu().numpy())
    assert all(isinstance(rh[k], np.ndarray) for k in ('extent', 'pairs', 'counts', 'centers', 'polygon'))
    assert np.array_equal(rh['counts'], r['counts'].cpu().numpy())
    given = [(-1.0, 1.0), (-2.0, 0.5), (0.0, 0.0), (-3.0, 3.0), (0.1, 0.2)]
    r3 = marginals.hexbins(trace, gridsize=(7, 9), extent=given)
    assert r3['extent'][2].tolist() == [-0.5, 0.5] and (r3['nx'], r3['ny']) == (7, 9)
    assert np.array_equal(r3['counts'].cpu().numpy(), ref.hexbins(pooled, 7, 9, ref.make_extent(pooled, given)))


# ---- the ABI

def test_abi_refusals_with_device_buffers():
    import torch
    x = torch.zeros((100, 3), dtype=torch.float64, device='cuda')
    out = torch.full((4000,), -1, dtype=torch.int64, device='cuda')
    table = ref.lattice_table([(-1.0, 1.0)] * 3, 15, 8)
    lib = _lib.load()

    def call(n_rows=100, n_par=3, ld=3, xp=x, nx=15, ny=8, t=table, cp=out):
        p = lambda a: None if a is None else C.c_void_p(a.data_ptr() if hasattr(a, 'data_ptr') else a.ctypes.data)    # noqa: E731
        return lib.pem_chain_hex_f64_dev(n_rows, n_par, ld, p(xp), nx, ny, p(t), p(cp), None)

    def edited(i, k, v):
        t = table.copy()
        t[i, k] = v
        return t
    for bad in (dict(ld=2), dict(n_par=1), dict(n_par=33, ld=40), dict(nx=0), dict(nx=65), dict(ny=0), dict(ny=65), dict(n_rows=0),
                dict(xp=None), dict(t=None), dict(cp=None), dict(t=edited(0, 0, np.nan)), dict(t=edited(1, 2, np.inf)),
                dict(t=edited(2, 1, 0.0)), dict(t=edited(1, 3, -1.0)), dict(t=edited(0, 3, np.nan))):
        assert call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    torch.cuda.synchronize()
    assert torch.all(out == -1)                                 # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    n = 3 * ref.n_cells(15, 8)
    assert np.array_equal(o[:n].reshape(3, -1), ref.hexbins(np.zeros((100, 3)), 15, 8, table=table)) and np.all(o[n:] == -1)


# ---- end to end

def test_corner_with_hexagons_on_a_device_dram_trace_end_to_end():
    import torch
    from hallthrusterpem_amd import marginals
    from hallthrusterpem_amd.calibration import DeviceDRAM
    mu = torch.tensor([1.0, -2.0, 0.5, 30.0], dtype=torch.float64, device='cuda')
    sd = np.array([1.0, 0.3, 2.0, 0.05])
    corr = np.array([[1.0, 0.6, -0.3, 0.0], [0.6, 1.0, 0.2, 0.1], [-0.3, 0.2, 1.0, 0.0], [0.0, 0.1, 0.0, 1.0]])
    cov = corr * np.outer(sd, sd)
    prec = torch.as_tensor(np.linalg.inv(cov), device='cuda')

    def logp(t):
        z = t - mu
        return -0.5 * ((z @ prec) * z).sum(dim=1)
    K = 32
    theta0 = np.random.default_rng(7).multivariate_normal(mu.cpu().numpy(), cov, size=K)
    trace = DeviceDRAM(logp, theta0, cov0=cov, n_chains=K, seed=11, adapt_after=200, adapt_interval=100).run(1000)
    names = ['a', 'b', 'c', 'e']
    sel = [3, 0, 2]
    xh = trace.cpu().numpy()
    pooled = mref.pool(xh)[:, sel]
    m = pooled.shape[0]
    cmin = int(0.0015 * m)
    hist = marginals.corner(trace, names=names, select=['e', 'a', 2], bins=15, cmin=cmin, points=48)
    got = marginals.corner(trace, names=names, select=['e', 'a', 2], bins=15, cmin=cmin, points=48, plot2d='hex')
    assert 'hex' not in hist and sorted(got) == sorted(list(hist) + ['hex'])
    for k, v in hist.items():                                   # the 'hist' keys, bit for bit
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, got[k]), k
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, got[k]), k
        else:
            assert v == got[k], k
    hx = got['hex']
    assert (hx['nx'], hx['ny'], hx['n_draws']) == (15, 8, m)    # gridsize None means bins
    ext = ref.make_extent(pooled)
    table = ref.lattice_table(ext, 15, 8)
    want = ref.hexbins(pooled, 15, 8, table=table)
    counts = hx['counts'].cpu().numpy()
    assert np.array_equal(hx['extent'].cpu().numpy(), ext) and np.array_equal(counts, want)
    dropped = np.array([ref.dropped_of_pair(pooled[:, i], pooled[:, j], 15, 8, table[i], table[j]) for i, j in ref.pair_list(3)])
    assert np.array_equal(counts.sum(axis=1), m - dropped)
    assert isinstance(hx['mask'], torch.Tensor) and hx['mask'].is_cuda and np.array_equal(hx['mask'].cpu().numpy(), want < cmin)
    assert hx['mask'].any() and not hx['mask'].all()
    levels = np.stack([mref.credible_levels(t, (0.5, 0.9)) for t in want])
    assert hx['levels'].shape == (3, 2) and np.array_equal(hx['levels'], levels) and np.all(levels[:, 0] >= levels[:, 1]) and levels.min() > 0
    for p, (i, j) in enumerate(ref.pair_list(3)):
        c, poly = ref.geometry(15, 8, ext[i], ext[j])
        assert np.array_equal(hx['centers'][p].cpu().numpy(), c) and np.array_equal(hx['polygon'][p].cpu().numpy(), poly)
    wide = marginals.corner(xh, select=sel, cmin=cmin, points=48, plot2d='hex', gridsize=(20, 20))['hex']
    assert isinstance(wide['counts'], np.ndarray) and np.array_equal(wide['counts'], ref.hexbins(pooled, 20, 20, ext))
