"""Corner-plot marginals on the MI355X: pem_chain_hist_f64_dev equal to tests/marginals_np.py count for count over its dispatch
space, pem_chain_kde_f64_dev against the long-double restatement within a derived bound, determinism, in-place reading, and
marginals.corner on a DRAM trace end to end.

Counts have no tolerance: np.array_equal on int64.

Error bound of the density (u = 2^-53, gamma_k = k u / (1 - k u)).  With a_t = ((g - x_t) inv_h)^2 / 2 and w_t = exp(-a_t):
the kernel forms z = fl(fl(g - x_t) inv_h) (two roundings), fl(z z) (one more; squaring doubles the two before it) and halves
it exactly, so a^_t = a_t (1 + delta), |delta| <= gamma_5: C_A = 5.  exp is OCML's exp f64, documented to 1 ulp of the result,
i.e. a relative 2 u: E = 2.  So exp^(-a^_t) = w_t (1 + theta), |theta| <= (C_A a_t + E) u up to second order; the second
order is e^y - 1 <= y (1 + y) with y = C_A a_t u <= 5 * 745.2 * u < 5e-13 for every term that is not below 2^-1075, covered by
the factor (1 + 1e-9) on the first term.  A term passes through at most K_S additions: 1024 in its wave's chain over a
4096-row block (64 of every 256 rows), 3 to add the four wave sums, n_rb = ceil(n_rows / 4096) to add the block partials:
K_S = 1027 + n_rb.  Hence
    |S^ - S| <= u (C_A sum a_t w_t + E sum w_t) (1 + 1e-9) + gamma_{K_S} (1 + (C_A a_max + E) u) sum w_t + n_rows 2^-1022
(the last term covers terms that underflow or come out denormal), and the multiplication by scale adds u |kde^|.  sum w_t,
sum a_t w_t, a_max and the reference density come from marginals_np.kde_direct in np.longdouble, given the same float64 inv_h
and scale as the kernel.

Bandwidth.  s^2 = gamma^(0) m / (m - 1) with gamma^(0) from pem_chain_autocov_f64_dev over the pooled draws, whose bound is
derived in tests/test_chain_diagnostics.py (lag 0: S = sum y^2, A = 2 sum |y|, n_l = m, K = m + ceil(m / 4096)); call its
relative size r.  m / (m - 1), the product, the square root (which halves r), the factor f (a correctly rounded constant or
pow to 1 ulp: 2 u) and f s add at most 0.5 + 1 + 1 + 2 + 1 < 6 roundings: |h^ - h| <= h (r / (2 (1 - r)) + 6 u).

Correlation of corner(): formed from the device's covariance by two square roots, a product and a division (4 roundings;
gamma_5 is asserted), compared with the same expression in long double on that covariance; the covariance itself carries
the bound below.

Mean and covariance of corner().  mean^ is a sum of m terms in an unknown order and a division: |mean^_i - mean_i| <= D_i =
gamma_{m+1} sum_t |x_ti| / m.  y^_ti = (y_ti - delta_i)(1 + e), |delta_i| <= D_i; a product of two carries gamma_3; the m
products are added in an unknown order (gamma_{m-1}) and divided by m - 1.  With S_ij = sum_t |y_ti y_tj|, A_i = sum_t |y_ti|
and Q_ij = S_ij + D_j A_i + D_i A_j + m D_i D_j:
    (m - 1) |cov^_ij - cov_ij| <= D_j A_i + D_i A_j + m D_i D_j + (gamma_3 + gamma_m (1 + gamma_3)) Q_ij,  plus u |cov^_ij|.
"""
import ctypes as C

import numpy as np
import pytest

import chain_diag_np as chain_ref
import marginals_np as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
C_A, E_EXP = 5, 2
TILE, HIST_WGS = 128, 1024
KDE_BLOCK = 4096


def _g(k):
    return k * U / (1 - k * U)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _counts(x, edges, pairs=True):
    from hallthrusterpem_amd import marginals
    h1, h2, drop, nonf = marginals._hist_dev(x, edges, pairs)
    full = marginals._full_hist2d(h1, h2).cpu().numpy() if pairs else None
    return h1.cpu().numpy(), full, drop.cpu().numpy(), nonf.cpu().numpy()


def _check_counts(xh, x, bins, ranges=None, pairs=True):
    edges = ref.make_edges(xh, bins, ranges)
    got = _counts(x, edges, pairs)
    want = ref.histograms(xh, edges, pairs)
    for g, w, name in zip(got, want, ('hist1d', 'hist2d', 'dropped', 'nonfinite')):
        if w is None:
            assert g is None
            continue
        assert g.dtype == np.int64 and np.array_equal(g, w), name
    h1, h2, dropped, _ = got
    n = xh.shape[0]
    assert np.array_equal(h1.sum(axis=1) + dropped, np.full(xh.shape[1], n))
    if pairs:
        d = xh.shape[1]
        for i in range(d):
            for j in range(d):
                if i != j:
                    assert np.all(h2[i, j].sum(axis=1) <= h1[i])
                    if dropped[j] == 0:
                        assert np.array_equal(h2[i, j].sum(axis=1), h1[i])
    return got


# ---- counts over the dispatch space

@pytest.mark.parametrize('n_par', [1, 2, 17, 32])
@pytest.mark.parametrize('bins', [1, 2, 15, 64])
def test_counts_over_parameters_and_bins(n_par, bins):
    rng = np.random.default_rng(100 * n_par + bins)
    n = 700 if n_par > 2 else 3000
    xh = rng.standard_normal((n, n_par)) * rng.uniform(0.1, 10, n_par) + rng.uniform(-5, 5, n_par)
    _check_counts(xh, _dev(xh), bins)
    _check_counts(xh, _dev(xh), bins, ranges=[(-1.0 - i % 3, 2.0 + i % 5) for i in range(n_par)])


@pytest.mark.parametrize('n_rows', [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE, TILE * HIST_WGS - 1, TILE * HIST_WGS, TILE * HIST_WGS + 1,
                                    2 * TILE * HIST_WGS + TILE + 5])
def test_counts_around_the_row_tiles(n_rows):
    """128 rows per stage; with one task block the launch has up to 1024 row blocks, so past 128 * 1024 rows a workgroup
    walks more than one tile"""
    rng = np.random.default_rng(n_rows)
    xh = rng.standard_normal((n_rows, 3))
    _check_counts(xh, _dev(xh), 15)
    _check_counts(xh, _dev(xh), 15, ranges=[(-1, 1), (-4, 4), (0, 0.5)])


@pytest.mark.parametrize('n_rows', [TILE * (HIST_WGS // 4) - 1, TILE * (HIST_WGS // 4) + 1])
def test_counts_around_the_row_blocks_of_four_task_blocks(n_rows):
    """17 parameters at 15 bins are 153 tables in 4 task blocks: 256 row blocks"""
    rng = np.random.default_rng(n_rows)
    xh = rng.standard_normal((n_rows, 17))
    _check_counts(xh, _dev(xh), 15)


@pytest.mark.parametrize('n,S,pad,off', [(1000, 5, 0, 0), (1000, 5, 7, 1), (333, 17, 2, 3), (129, 1, 4, 1)])
def test_counts_of_a_strided_view(n, S, pad, off):
    rng = np.random.default_rng(n + S + off)
    wide = rng.standard_normal((n, S + pad + off))
    xh = wide[:, off:off + S]
    x = _dev(wide)[:, off:off + S]
    assert x.stride(0) == S + pad + off and (x.data_ptr() % 16 == 8) == (off % 2 == 1)
    _check_counts(xh, x, 15)
    _check_counts(xh, x, 7, pairs=False)


@pytest.mark.parametrize('bins', [1, 3, 15, 64])
def test_counts_on_and_around_every_edge(bins):
    rng = np.random.default_rng(bins)
    e0, e1 = np.linspace(-1.3, 2.9, bins + 1), np.linspace(1e-3, 1.7e-3, bins + 1)
    v0 = np.concatenate([e0, np.nextafter(e0, -np.inf), np.nextafter(e0, np.inf)])
    v1 = np.concatenate([e1, np.nextafter(e1, -np.inf), np.nextafter(e1, np.inf)])
    xh = np.stack([np.tile(v0, v1.size), np.repeat(v1, v0.size)], axis=1)
    xh = xh[rng.permutation(xh.shape[0])]
    _check_counts(xh, _dev(xh), bins, ranges=[(-1.3, 2.9), (1e-3, 1.7e-3)])
    _check_counts(xh, _dev(xh), bins)


@pytest.mark.parametrize('n_par,bins', [(1, 15), (2, 1), (17, 15), (32, 64), (5, 64)])
def test_counts_when_every_row_is_identical(n_par, bins):
    """every increment of every table lands on one cell: the worst contention"""
    row = np.random.default_rng(n_par).standard_normal(n_par)
    xh = np.tile(row, (20_000, 1))
    h1, h2, _, _ = _check_counts(xh, _dev(xh), bins, ranges=[(-4, 4)] * n_par)
    assert np.all(h1.max(axis=1) == 20_000)
    _check_counts(xh, _dev(xh), bins)                           # constant parameters: ranges widened by 0.5 either side


def test_counts_of_a_rejecting_samplers_trace():
    rng = np.random.default_rng(8)
    xh = np.repeat(rng.standard_normal((3000, 17)), rng.integers(1, 60, 3000), axis=0)
    _check_counts(xh, _dev(xh), 15)


def test_non_finite_values_poison_only_their_pairs():
    rng = np.random.default_rng(9)
    xh = rng.standard_normal((5000, 6))
    clean = _check_counts(xh, _dev(xh), 15, ranges=[(-5, 5)] * 6)
    xh[rng.integers(0, 5000, 40), 1] = np.nan
    xh[rng.integers(0, 5000, 30), 4] = np.inf
    xh[rng.integers(0, 5000, 30), 4] = -np.inf
    h1, h2, dropped, nonfinite = _check_counts(xh, _dev(xh), 15, ranges=[(-5, 5)] * 6)
    assert nonfinite[1] > 0 and nonfinite[4] > 0 and not nonfinite[[0, 2, 3, 5]].any()
    for i in (0, 2, 3, 5):
        assert np.array_equal(h1[i], clean[0][i])
        for j in (0, 2, 3, 5):
            assert np.array_equal(h2[i, j], clean[1][i, j])
    assert h2[0, 1].sum() == 5000 - dropped[1] and h2[1, 4].sum() < min(h1[1].sum(), h1[4].sum())
    _check_counts(xh, _dev(xh), 15)                             # default ranges: the finite min and max


def test_counts_at_production_size():
    """case (b) of profiles/chain_diagnostics_r01.txt: 64 chains x 17 parameters x 20 000 rows, a random walk per chain"""
    rng = np.random.default_rng(10)
    xh = (rng.standard_normal((20_000, 64 * 17)).cumsum(axis=0) * 1e-2 + 5.0).reshape(-1, 17)
    _check_counts(xh, _dev(xh), 15)


def test_single_cells_beyond_16_and_24_bits():
    """2^24 + 3 identical rows of two parameters, and 70 000 rows of another value: cells above 65 535 and above 2^24"""
    import torch
    from hallthrusterpem_amd import marginals
    n_big, n_small = 2 ** 24 + 3, 70_000
    x = torch.empty((n_big + n_small, 2), dtype=torch.float64, device='cuda')
    x[:n_big] = torch.tensor([0.25, -1.5], dtype=torch.float64, device='cuda')
    x[n_big:] = torch.tensor([2.75, 1.5], dtype=torch.float64, device='cuda')
    edges = ref.make_edges(np.zeros((1, 2)), 4, ranges=[(0.0, 4.0), (-2.0, 2.0)])
    two = np.array([[0.25, -1.5], [2.75, 1.5]])
    one1, one2, _, _ = ref.histograms(two, edges)
    (k0a, k0b), (k1a, k1b) = (ref.bin_index(two[:, i], edges[i]) for i in range(2))
    want1 = np.zeros((2, 4), np.int64)
    want1[0, k0a], want1[0, k0b], want1[1, k1a], want1[1, k1b] = n_big, n_small, n_big, n_small
    want2 = np.zeros((4, 4), np.int64)
    want2[k0a, k1a], want2[k0b, k1b] = n_big, n_small
    h1, h2, drop, nonf = marginals._hist_dev(x, edges, True)
    assert np.array_equal(h1.cpu().numpy(), want1) and np.array_equal(h2[0].cpu().numpy(), want2)
    assert not drop.any() and not nonf.any()
    assert np.array_equal(one2[0, 1] > 0, want2 > 0)


def test_histogram_abi_refusals_with_device_buffers_and_one_dimension_only():
    import torch
    from hallthrusterpem_amd import _lib
    x = torch.zeros((100, 3), dtype=torch.float64, device='cuda')
    e = torch.as_tensor(np.tile(np.linspace(-1, 1, 16), (3, 1)), device='cuda')
    out = torch.full((4000,), -1, dtype=torch.int64, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731
    lib = _lib.load()
    ok = dict(n_rows=100, n_par=3, ld=3, bins=15)
    for bad in (dict(ld=2), dict(n_par=0), dict(n_par=33, ld=40), dict(bins=0), dict(bins=65), dict(n_rows=0)):
        a = {**ok, **bad}
        rc = lib.pem_chain_hist_f64_dev(a['n_rows'], a['n_par'], a['ld'], p(x), a['bins'], p(e), p(out), p(out[100:]), p(out[3000:]),
                                        p(out[3100:]), None)
        assert rc == _lib.PEM_ERR_INVALID_ARG, bad
    assert lib.pem_chain_hist_f64_dev(100, 3, 3, p(x), 15, p(e), p(out), None, p(out[3000:]), p(out[3100:]), None) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[:45].sum() == 300 and np.all(o[45:3000] == -1) and not o[3000:3003].any() and not o[3100:3103].any()


# ---- density

def _kde_bound(x, grid, inv_h, scale, got):
    want, sw, saw, amax = ref.kde_direct(x, grid, inv_h, scale)
    n = x.size
    k_s = 1027 + -(-n // KDE_BLOCK)
    ld = np.longdouble
    s_err = ld(U) * (C_A * saw + E_EXP * sw) * (1 + ld(1e-9)) + ld(_g(k_s)) * (1 + (C_A * amax + E_EXP) * ld(U)) * sw + n * ld(2.0) ** -1022
    bound = ld(scale) * s_err + ld(U) * np.abs(got.astype(ld))
    err = np.abs(got.astype(ld) - want)
    return err, bound, want


def _check_density(xh, grid, h):
    """xh (m, d), grid (d, G), h (d,) -> the device's density, every value inside its bound"""
    from hallthrusterpem_amd import marginals
    m, d = xh.shape
    inv_h = 1.0 / np.asarray(h, dtype=np.float64)
    scale = inv_h / (m * np.sqrt(2 * np.pi))
    got = marginals._kde_dev(_dev(xh), grid, inv_h, scale).cpu().numpy()
    worst = 0.0
    for i in range(d):
        err, bound, want = _kde_bound(xh[:, i], grid[i], inv_h[i], scale[i], got[i])
        ratio = float(np.max(err / np.maximum(bound, np.finfo(np.longdouble).tiny)))
        print(f'density parameter {i}: largest error / bound = {ratio:.3g}')
        assert np.all(np.isfinite(got[i])) and np.all(err <= bound), (i, ratio)
        worst = max(worst, ratio)
    return got, worst


@pytest.mark.parametrize('n_rows', [1, 63, 64, 65, 255, 256, 257, KDE_BLOCK - 1, KDE_BLOCK, KDE_BLOCK + 1, 2 * KDE_BLOCK + 1])
def test_density_around_the_row_tiles(n_rows):
    rng = np.random.default_rng(n_rows)
    xh = rng.standard_normal((n_rows, 2)) * [1.0, 0.02] + [0.5, 40.0]
    grid = np.stack([np.linspace(-4, 5, 100), np.linspace(39.9, 40.1, 100)])
    _check_density(xh, grid, [0.2, 0.004])


@pytest.mark.parametrize('n_grid', [1, 2, 255, 256, 257])
def test_density_around_the_grid_blocks(n_grid):
    rng = np.random.default_rng(n_grid)
    xh = rng.standard_normal((3000, 3)) * [1.0, 3.0, 0.1] + [0.0, -2.0, 7.0]
    grid = np.stack([np.linspace(xh[:, i].min(), xh[:, i].max(), n_grid) for i in range(3)])
    _check_density(xh, grid, [0.3, 0.8, 0.02])


def test_density_far_outside_the_data():
    """grid points 30 to 40 bandwidths from the nearest draw: densities near 1e-300, and far enough for an exact 0"""
    rng = np.random.default_rng(12)
    xh = rng.uniform(-1, 1, (2000, 1))
    h = 0.05
    grid = np.array([[1 + 30 * h, 1 + 36 * h, 1 + 37.1 * h, 1 + 38.5 * h, 1 + 39.5 * h, -1 - 37 * h, 1 + 60 * h, -1 - 1e6, 1e300]])
    got, _ = _check_density(xh, grid, [h])
    assert 0 < got[0, 1] < 1e-270 and got[0, 6] == 0.0 and got[0, 7] == 0.0 and got[0, 8] == 0.0


@pytest.mark.parametrize('factor', [1e-6, 1e-3, 1.0, 1e3, 1e6])
def test_density_over_twelve_decades_of_bandwidth(factor):
    rng = np.random.default_rng(13)
    xh = rng.standard_normal((4000, 2)) * [2.0, 1e-4] + [1.0, 3e-3]
    grid = np.stack([np.linspace(xh[:, i].min(), xh[:, i].max(), 64) for i in range(2)])
    _check_density(xh, grid, [2.0 * factor, 1e-4 * factor])


def test_density_of_draws_far_from_zero():
    """mean / sd = 1e4: the subtraction g - x_t comes first, so the bound needs no conditioning term"""
    rng = np.random.default_rng(14)
    xh = 1000.0 + 0.1 * rng.standard_normal((5000, 2)) * [1.0, 10.0]
    grid = np.stack([np.linspace(xh[:, i].min(), xh[:, i].max(), 128) for i in range(2)])
    _check_density(xh, grid, [0.02, 0.2])


def test_degenerate_parameters_give_nan_and_leave_their_neighbours_alone():
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(15)
    xh = rng.standard_normal((1000, 4, 4))
    g0, d0, h0 = marginals.kde(xh, points=50, burnin=0.0)
    xh[:, :, 1] = 2.5
    xh[300, 2, 3] = np.nan
    g1, d1, h1 = marginals.kde(xh, points=50, burnin=0.0)
    assert np.all(np.isnan(d1[1])) and np.isnan(h1[1]) and np.all(np.isnan(d1[3])) and np.isnan(h1[3])
    for i in (0, 2):
        assert np.array_equal(d0[i], d1[i]) and h0[i] == h1[i] and np.array_equal(g0[i], g1[i])
    r = marginals.histograms(xh, burnin=0.0)
    assert r['nonfinite'].tolist() == [0, 0, 0, 1] and r['dropped'].tolist() == [0, 0, 0, 1]
    assert r['edges'][1, 0] == 2.0 and r['edges'][1, -1] == 3.0 and r['hist1d'][1].sum() == 4000


def _check_bandwidth(pooled, bw, h):
    """h (d,) float64 from the device path against marginals_np.bandwidth in long double, within the bound of the docstring"""
    m = pooled.shape[0]
    mean, gam, sabs, aabs, xabs = chain_ref.gamma_direct(pooled, [0])
    D = _g(m + 33) * xabs[0] / m + U * np.abs(mean[0])
    Q = sabs[0, 0] + D * aabs[0, 0] + m * D * D
    r = ((D * aabs[0, 0] + m * D * D + (_g(2) + _g(m + -(-m // 4096)) * (1 + _g(2))) * Q) / m) / gam[0, 0] + U * (1 + 1e-9)
    want = ref.bandwidth(pooled, bw)
    err = np.abs(np.asarray(h).astype(np.longdouble) - want)
    assert np.all(err <= want * (r / (2 * (1 - r)) + 6 * U)), (err / want, r)


@pytest.mark.parametrize('bw', ['scott', 'silverman', 0.25])
def test_bandwidth_against_long_double(bw):
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(16)
    xh = rng.standard_normal((2500, 4, 3)) * [1.0, 1e-3, 50.0] + [0.0, 7.0, -1e4]
    _, _, h = marginals.kde(xh, points=4, bw=bw, burnin=0.0)
    _check_bandwidth(xh.reshape(-1, 3), bw, h)


def test_python_density_matches_the_restatement_and_scipy():
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(17)
    xh = rng.standard_normal((800, 4, 2)) * [1.0, 0.3] + [0.0, 2.0]
    grid, dens, h = marginals.kde(xh, points=64, bw='silverman', burnin=0.25)
    pooled = ref.pool(xh, 0.25)
    assert grid.shape == (2, 64) and dens.shape == (2, 64) and h.shape == (2,)
    for i in range(2):
        assert np.array_equal(grid[i], np.linspace(pooled[:, i].min(), pooled[:, i].max(), 64))
        m = pooled.shape[0]
        inv_h = 1.0 / h[i]
        err, bound, _ = _kde_bound(pooled[:, i], grid[i], inv_h, inv_h / (m * np.sqrt(2 * np.pi)), dens[i])
        assert np.all(err <= bound)
    stats = pytest.importorskip('scipy.stats')
    for i in range(2):
        want = stats.gaussian_kde(pooled[:, i], bw_method='silverman')(grid[i])
        assert np.max(np.abs(dens[i] - want) / want) <= 1e-11
    g2, d2, _ = marginals.kde(xh, grid=np.linspace(-1, 1, 9), burnin=0.25)
    assert g2.shape == (2, 9) and np.array_equal(g2[0], g2[1])


# ---- determinism, independence of the other grid points, in place

def test_repeat_runs_give_the_same_bits():
    import torch
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(18)
    x = _dev(np.repeat(rng.standard_normal((3000, 9)), rng.integers(1, 9, 3000), axis=0))
    edges = ref.make_edges(x.cpu().numpy(), 15)
    grid = np.tile(np.linspace(-3, 3, 300), (9, 1))
    inv_h, scale = np.full(9, 4.0), np.full(9, 4.0 / (x.shape[0] * np.sqrt(2 * np.pi)))
    a = marginals._hist_dev(x, edges, True)
    k = marginals._kde_dev(x, grid, inv_h, scale)
    for _ in range(3):
        b = marginals._hist_dev(x, edges, True)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        assert torch.equal(k, marginals._kde_dev(x, grid, inv_h, scale))


def test_a_density_value_does_not_depend_on_the_other_grid_points():
    import torch
    from hallthrusterpem_amd import marginals
    x = _dev(np.random.default_rng(19).standard_normal((9000, 3)))
    grid = np.tile(np.linspace(-3, 3, 600), (3, 1))
    inv_h, scale = np.full(3, 5.0), np.full(3, 1e-4)
    whole = marginals._kde_dev(x, grid, inv_h, scale)
    for sl in (slice(0, 1), slice(17, 18), slice(100, 357), slice(300, 600), slice(5, 600, 7)):
        part = marginals._kde_dev(x, np.ascontiguousarray(grid[:, sl]), inv_h, scale)
        assert torch.equal(part, whole[:, sl])


def test_a_contiguous_trace_is_read_in_place(monkeypatch):
    import torch
    from hallthrusterpem_amd import _lib, marginals
    rng = np.random.default_rng(20)
    n, K, d = 500, 6, 5
    trace = _dev(rng.standard_normal((n, K, d)))
    b = int(0.1 * n)
    lib = _lib.load()
    seen = {}
    for name in ('pem_chain_hist_f64_dev', 'pem_chain_kde_f64_dev'):
        real = getattr(lib, name)

        def spy(*args, _real=real, _name=name):
            seen[_name] = (args[0], args[2], args[3].value)
            return _real(*args)
        monkeypatch.setattr(lib, name, spy, raising=False)
    r = marginals.histograms(trace)
    g, dens, h = marginals.kde(trace, points=32)
    want_ptr = trace.data_ptr() + b * K * d * 8
    assert seen['pem_chain_hist_f64_dev'] == ((n - b) * K, d, want_ptr) and seen['pem_chain_kde_f64_dev'] == ((n - b) * K, d, want_ptr)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in (r['edges'], r['hist1d'], r['hist2d'], r['dropped'], r['nonfinite'], g, dens, h))
    assert r['hist1d'].dtype == torch.int64 and r['hist2d'].dtype == torch.int64 and r['n_draws'] == (n - b) * K
    # the same draws as one chain of (n' K) rows in a wider buffer, starting at an odd column: a strided view, in place too
    wide = torch.zeros(((n - b) * K, d + 4), dtype=torch.float64, device='cuda')
    wide[:, 1:1 + d] = trace[b:].reshape(-1, d)
    view = wide[:, 1:1 + d]
    r2 = marginals.histograms(view, burnin=0.0)
    g2, dens2, h2 = marginals.kde(view, points=32, burnin=0.0)
    assert seen['pem_chain_hist_f64_dev'] == ((n - b) * K, d + 4, view.data_ptr()) and seen['pem_chain_kde_f64_dev'][2] == view.data_ptr()
    for k in ('edges', 'hist1d', 'hist2d', 'dropped', 'nonfinite'):
        assert torch.equal(r[k], r2[k]), k
    assert torch.equal(g, g2) and torch.equal(dens, dens2) and torch.equal(h, h2)
    # numpy in -> numpy out, the same numbers
    rh = marginals.histograms(trace.cpu().numpy())
    gh, dh, hh = marginals.kde(trace.cpu().numpy(), points=32)
    assert all(isinstance(v, np.ndarray) for v in (rh['edges'], rh['hist1d'], rh['hist2d'], rh['dropped'], rh['nonfinite'], gh, dh, hh))
    assert np.array_equal(rh['hist2d'], r['hist2d'].cpu().numpy()) and np.array_equal(dh, dens.cpu().numpy())
    assert marginals.histograms(trace, pairs=False)['hist2d'] is None


# ---- end to end

def _dram_trace(K=32, n_steps=2000):
    import torch
    from hallthrusterpem_amd.calibration import DRAM
    mu = np.array([1.0, -2.0, 0.5, 30.0])
    sd = np.array([1.0, 0.3, 2.0, 0.05])
    corr = np.array([[1.0, 0.6, -0.3, 0.0], [0.6, 1.0, 0.2, 0.1], [-0.3, 0.2, 1.0, 0.0], [0.0, 0.1, 0.0, 1.0]])
    cov = corr * np.outer(sd, sd)
    prec = torch.as_tensor(np.linalg.inv(cov), device='cuda')
    mu_d = torch.as_tensor(mu, device='cuda')

    def logp(theta):
        z = theta - mu_d
        return -0.5 * ((z @ prec) * z).sum(dim=1)
    theta0 = np.random.default_rng(7).multivariate_normal(mu, cov, size=K)
    s = DRAM(logp, theta0, cov0=cov, n_chains=K, seed=11, adapt_after=500, adapt_interval=100, device='cuda')
    return s.run(n_steps), mu, cov


def test_corner_of_a_dram_trace_end_to_end():
    import torch
    from hallthrusterpem_amd import marginals
    trace, mu, cov = _dram_trace()
    names = ['a', 'b', 'c', 'e']
    xh = trace.cpu().numpy()
    m = ref.pool(xh).shape[0]
    cmin = int(0.0015 * m)
    got = marginals.corner(trace, names=names, select=['e', 'a', 2], bins=15, cmin=cmin, points=48)
    want = ref.corner(xh, select=[3, 0, 2], bins=15, cmin=cmin, points=48)
    assert got['names'] == ['e', 'a', 'c'] and got['n_draws'] == m == want['n_draws']
    for k in ('edges', 'hist1d', 'hist2d', 'dropped', 'nonfinite', 'grid', 'mask'):
        assert isinstance(got[k], torch.Tensor) and got[k].is_cuda
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert np.array_equal(got['levels'], want['levels']) and got['levels'].shape == (3, 3, 2)
    assert got['mask'].any() and not got['mask'].all()
    pooled = ref.pool(xh)[:, [3, 0, 2]]
    h = got['bandwidth'].cpu().numpy()
    dens = got['density'].cpu().numpy()
    _check_bandwidth(pooled, 'scott', h)
    for i in range(3):
        inv_h = 1.0 / h[i]
        err, bound, _ = _kde_bound(pooled[:, i], want['grid'][i], inv_h, inv_h / (m * np.sqrt(2 * np.pi)), dens[i])
        assert np.all(err <= bound), i
    ld = np.longdouble
    mean, c = got['mean'].cpu().numpy().astype(ld), got['cov'].cpu().numpy().astype(ld)
    D = ld(_g(m + 1)) * want['abs_x'] / m
    assert np.all(np.abs(mean - want['mean']) <= D)
    A = np.abs(pooled.astype(ld) - want['mean']).sum(axis=0)
    DA = np.outer(A, D)                                         # [i, j] = A_i D_j
    DD = m * np.outer(D, D)
    Q = want['abs_cov'] + DA + DA.T + DD
    bound = (DA + DA.T + DD + (_g(3) + _g(m) * (1 + _g(3))) * Q) / (m - 1) + U * np.abs(c)
    assert np.all(np.abs(c - want['cov']) <= bound), float(np.max(np.abs(c - want['cov']) / bound))
    # corr^ = cov^_ij / (sqrt(cov^_ii) sqrt(cov^_jj)) from the device's own cov: two square roots, a product and a division
    sd = np.sqrt(np.diag(c))
    corr_of_cov = c / np.outer(sd, sd)
    assert np.all(np.abs(got['corr'].cpu().numpy().astype(ld) - corr_of_cov) <= _g(5) * np.abs(corr_of_cov))
    # and the marginals are the Gaussian's: the KDE peaks near the mean, the pooled moments are the posterior's
    sel = [3, 0, 2]
    assert np.all(np.abs(mean.astype(np.float64) - mu[sel]) < 0.1 * np.sqrt(np.diag(cov)[sel]))
    peak = want['grid'][np.arange(3), dens.argmax(axis=1)]
    assert np.all(np.abs(peak - mu[sel]) < 0.5 * np.sqrt(np.diag(cov)[sel]))
    host = marginals.corner(xh, names=names, select=['e', 'a', 2], bins=15, cmin=cmin, points=48)
    assert isinstance(host['hist2d'], np.ndarray) and np.array_equal(host['hist2d'], want['hist2d'])
