"""Corner-plot marginals without a GPU: pem_chain_hist_f64_dev and pem_chain_kde_f64_dev are declared, bound, built and
exported, refuse every malformed call before they look for a device and compile without scratch or spills; marginals.py
refuses bad arguments before it touches a device; tests/marginals_np.py equals np.histogram, np.histogram2d and
scipy.stats.gaussian_kde, and gives the known answers of a hand-worked example."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import marginals_np as ref

ROOT = Path(__file__).resolve().parents[1]
HIST, KDE = 'pem_chain_hist_f64_dev', 'pem_chain_kde_f64_dev'


def test_symbols_are_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    for name, n_args in ((HIST, 11), (KDE, 12)):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header)
        assert m and len(m.group(1).split(',')) == n_args
        assert len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(_lib.load(), name)
    for macro, value in (('PEM_MARGINALS_MAX_PAR', _lib.MARGINALS_MAX_PAR), ('PEM_MARGINALS_MAX_BINS', _lib.MARGINALS_MAX_BINS),
                         ('PEM_HIST_ROW_TILE', _lib.HIST_ROW_TILE), ('PEM_KDE_MAX_GRID', _lib.KDE_MAX_GRID),
                         ('PEM_KDE_ROW_BLOCK', _lib.KDE_ROW_BLOCK)):
        assert re.search(r'#define %s (\d+)' % macro, header).group(1) == str(value)
    assert _lib.MARGINALS_MAX_PAR >= 32 and _lib.MARGINALS_MAX_BINS >= 64
    assert build.PKG / 'csrc' / 'pem_marginals.hip' in build.SRCS


FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host


def _hist(n_rows=100, n_par=3, ld=3, x=True, bins=15, edges=True, hist1d=True, hist2d=True, dropped=True, nonfinite=True):
    from hallthrusterpem_amd import _lib
    p = lambda on: FAKE if on else None        # noqa: E731
    return _lib.load().pem_chain_hist_f64_dev(n_rows, n_par, ld, p(x), bins, p(edges), p(hist1d), p(hist2d), p(dropped), p(nonfinite), None)


def _kde(n_rows=10_000, n_par=3, ld=3, x=True, n_grid=64, grid=True, inv_h=True, scale=True, kde=True, work=True, work_len=None):
    from hallthrusterpem_amd import _lib
    p = lambda on: FAKE if on else None        # noqa: E731
    if work_len is None:
        work_len = -(-n_rows // _lib.KDE_ROW_BLOCK) * n_par * n_grid
    return _lib.load().pem_chain_kde_f64_dev(n_rows, n_par, ld, p(x), n_grid, p(grid), p(inv_h), p(scale), p(kde), p(work), work_len, None)


@pytest.mark.parametrize('bad', [
    dict(n_rows=0), dict(n_par=0), dict(n_par=-1), dict(n_par=33, ld=33), dict(bins=0), dict(bins=-3), dict(bins=65), dict(ld=2),
    dict(x=False), dict(edges=False), dict(hist1d=False), dict(dropped=False), dict(nonfinite=False), dict(n_rows=1 << 48),
])
def test_malformed_histogram_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _hist(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_chain_hist' in _lib.load().pem_last_error()


@pytest.mark.parametrize('bad', [
    dict(n_rows=0, work_len=10), dict(n_par=0, work_len=10), dict(n_par=33, ld=33), dict(n_grid=0, work_len=10), dict(n_grid=4097),
    dict(ld=2), dict(x=False), dict(grid=False), dict(inv_h=False), dict(scale=False), dict(kde=False), dict(work=False),
    dict(work_len=3 * 3 * 64 - 1), dict(work_len=0), dict(n_rows=65536 * 4096, work_len=1 << 60),
])
def test_malformed_density_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _kde(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_chain_kde' in _lib.load().pem_last_error()


def test_the_row_limit_of_the_counts_is_the_documented_one():
    """n_rows >= 2^32 * floor(1024 / task blocks) is refused: 2^42 with one task block, 2^40 at n_par = 17, bins = 15 (4 task
    blocks); just below it the call gets as far as looking for a device"""
    from hallthrusterpem_amd import _lib
    assert _hist(n_rows=1 << 42) == _lib.PEM_ERR_INVALID_ARG
    assert _hist(n_rows=1 << 40, n_par=17, ld=17) == _lib.PEM_ERR_INVALID_ARG
    assert _hist(n_rows=1 << 42, n_par=17, ld=17, hist2d=False) == _lib.PEM_ERR_INVALID_ARG     # 17 tables: one block, 2^42
    if _lib.device_count() == 0:
        assert _hist(n_rows=(1 << 42) - (1 << 17)) == _lib.PEM_ERR_NO_DEVICE
        assert _hist(n_rows=(1 << 40) - (1 << 15), n_par=17, ld=17) == _lib.PEM_ERR_NO_DEVICE
        assert _hist(n_rows=1 << 41, n_par=17, ld=17, hist2d=False) == _lib.PEM_ERR_NO_DEVICE


def test_a_null_pair_table_is_not_a_refusal():
    """hist2d NULL means 1-D only: without a device the call gets as far as looking for one"""
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _hist(hist2d=False) == _lib.PEM_ERR_NO_DEVICE


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_marginal_kernels_have_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_marginals.hip')],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    assert sorted(rows) == ['chain_hist_kernel', 'chain_kde_partial_kernel', 'chain_kde_reduce_kernel'], rows
    for name, r in rows.items():
        assert r['vspill'] == 0 and r['sspill'] == 0 and r['scratch'] == 0, (name, r)
    assert rows['chain_kde_partial_kernel']['vgpr'] <= 128           # four waves per SIMD
    assert rows['chain_hist_kernel']['vgpr'] <= 256                  # two waves per SIMD: two workgroups per CU


# ---- Python refusals: raised from shapes and arguments alone, before any device is looked for

@pytest.mark.parametrize('call', [
    lambda m, x: m.histograms(x, burnin=1.0), lambda m, x: m.histograms(x, burnin=-0.1), lambda m, x: m.histograms(x[:3], burnin=0.0),
    lambda m, x: m.histograms(x, bins=0), lambda m, x: m.histograms(x, bins=65), lambda m, x: m.histograms(x, bins=2.5),
    lambda m, x: m.histograms(x[..., None]), lambda m, x: m.histograms(x[:, 0, 0]),
    lambda m, x: m.histograms(x, ranges=[(0, 1)]), lambda m, x: m.histograms(x, ranges=[(0, 1), (2, 1), (0, 1)]),
    lambda m, x: m.histograms(x, ranges=[(0, 1), (0, np.inf), (0, 1)]), lambda m, x: m.histograms(np.zeros((20, 2, 33))),
    lambda m, x: m.kde(x, burnin=1.5), lambda m, x: m.kde(x, points=0), lambda m, x: m.kde(x, points=4097), lambda m, x: m.kde(x, bw='botev'),
    lambda m, x: m.kde(x, bw=0.0), lambda m, x: m.kde(x, bw=-1.0), lambda m, x: m.kde(x, bw=np.nan), lambda m, x: m.kde(x, grid=np.zeros((2, 8))),
    lambda m, x: m.kde(x, grid=np.zeros((3, 0))), lambda m, x: m.kde(np.zeros((20, 2, 33))),
    lambda m, x: m.corner(x, names=['a', 'b']), lambda m, x: m.corner(x, select=['a']), lambda m, x: m.corner(x, names=['a', 'b', 'c'], select=['q']),
    lambda m, x: m.corner(x, select=[3]), lambda m, x: m.corner(x, select=[]), lambda m, x: m.corner(x, cmin=-1), lambda m, x: m.corner(x, bins=100),
    lambda m, x: m.corner(x, bw='x'), lambda m, x: m.corner(x, burnin=1.0), lambda m, x: m.corner(x, mass=(0.0,)),
])
def test_python_refusals_come_before_the_device(call, monkeypatch):
    from hallthrusterpem_amd import _lib, marginals
    monkeypatch.setattr(_lib, 'require_device', lambda: pytest.fail('a device was looked for'))
    with pytest.raises(ValueError):
        call(marginals, np.zeros((20, 4, 3)))


def test_module_surface():
    from hallthrusterpem_amd import marginals
    assert sorted(marginals.__all__) == ['corner', 'credible_levels', 'histograms', 'kde']


# ---- the restatement against numpy

def _edge_values(edges):
    """every edge, one ulp below and one ulp above it"""
    return np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])


def _against_numpy(x, bins, ranges=None):
    """hist1d against np.histogram, hist2d against np.histogram2d given the finite rows of the pair"""
    edges = ref.make_edges(x, bins, ranges)
    h1, h2, dropped, nonfinite = ref.histograms(x, edges)
    d = x.shape[1]
    for i in range(d):
        fin = np.isfinite(x[:, i])
        want, e = np.histogram(x[fin, i], bins=bins, range=(edges[i, 0], edges[i, -1]))
        assert np.array_equal(e, edges[i]) and np.array_equal(h1[i], want), i
        assert dropped[i] == x.shape[0] - want.sum() and nonfinite[i] == (~fin).sum()
        for j in range(i + 1, d):
            both = fin & np.isfinite(x[:, j])
            want2, _, _ = np.histogram2d(x[both, i], x[both, j], bins=bins, range=[(edges[i, 0], edges[i, -1]), (edges[j, 0], edges[j, -1])])
            assert np.array_equal(h2[i, j], want2.astype(np.int64)) and np.array_equal(h2[j, i], h2[i, j].T), (i, j)
        assert np.array_equal(h2[i, i], np.diag(h1[i]))
    return h1, h2, dropped, nonfinite


@pytest.mark.parametrize('bins', [1, 2, 15, 64])
def test_restatement_equals_numpy_on_random_draws_with_default_ranges(bins):
    rng = np.random.default_rng(bins)
    x = rng.standard_normal((5000, 4)) * [1.0, 1e-6, 3e4, 0.1] + [0.0, 5.0, -1e5, 1000.0]
    h1, _, dropped, _ = _against_numpy(x, bins)
    assert not dropped.any() and np.all(h1.sum(axis=1) == 5000)         # min and max sit on the outer edges


@pytest.mark.parametrize('bins', [1, 3, 15, 64])
def test_restatement_equals_numpy_on_and_around_every_edge(bins):
    rng = np.random.default_rng(7)
    e0 = np.linspace(-1.3, 2.9, bins + 1)
    e1 = np.linspace(1e-3, 1.7e-3, bins + 1)
    v0, v1 = _edge_values(e0), _edge_values(e1)
    x = np.stack([np.tile(v0, v1.size), np.repeat(v1, v0.size)], axis=1)
    x = x[rng.permutation(x.shape[0])]
    _against_numpy(x, bins, ranges=[(-1.3, 2.9), (1e-3, 1.7e-3)])


def test_restatement_equals_numpy_on_repeated_rows_ranges_constants_and_non_finite_values():
    rng = np.random.default_rng(3)
    x = np.repeat(rng.standard_normal((400, 3)), rng.integers(1, 40, 400), axis=0)        # a rejecting sampler's trace
    _against_numpy(x, 15)
    _, _, dropped, _ = _against_numpy(x, 15, ranges=[(-0.5, 0.5), (-10, 10), (0.0, 0.1)])   # draws left outside
    assert dropped[0] > 0 and dropped[1] == 0 and dropped[2] > 0
    x[:, 1] = 2.5                                                                           # a constant parameter
    h1, _, dropped, _ = _against_numpy(x, 15)
    e = ref.make_edges(x, 15)
    assert e[1, 0] == 2.0 and e[1, -1] == 3.0 and h1[1].sum() == x.shape[0] and dropped[1] == 0
    x[5, 0], x[17, 2], x[40, 2], x[41, 0] = np.nan, np.inf, -np.inf, np.nan
    _, h2, dropped, nonfinite = _against_numpy(x, 15)
    assert list(nonfinite) == [2, 0, 2] and list(dropped) == [2, 0, 2]
    assert h2[0, 2].sum() == x.shape[0] - 4 and h2[0, 1].sum() == x.shape[0] - 2


# ---- the restatement against scipy

@pytest.mark.parametrize('mean,sd', [(0.0, 1.0), (3.0, 0.1), (-5e-6, 2e-6), (1e20, 3e19)])
@pytest.mark.parametrize('bw', ['scott', 'silverman', 0.37])
@pytest.mark.parametrize('n', [50, 2000, 20_000])
def test_density_formula_equals_scipy(mean, sd, bw, n):
    stats = pytest.importorskip('scipy.stats')
    rng = np.random.default_rng(n)
    x = mean + sd * rng.standard_normal(n)
    grid = np.linspace(x.min() - sd, x.max() + sd, 64)
    want = stats.gaussian_kde(x, bw_method=bw)(grid)
    got = ref.kde(x, grid, bw, dtype=np.longdouble).astype(np.float64)
    assert np.max(np.abs(got - want) / want) <= 1e-12
    assert np.max(np.abs(ref.kde(x, grid, bw) - want) / want) <= 1e-12
    h = float(ref.bandwidth(x[:, None], bw)[0])
    direct, _, _, _ = ref.kde_direct(x, grid, 1.0 / h, 1.0 / h / (n * np.sqrt(2 * np.pi)))
    assert np.max(np.abs(direct.astype(np.float64) - want) / want) <= 1e-12


def test_density_integrates_to_one():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(3000), 4.0 + 0.5 * rng.standard_normal(1000)])
    h = float(ref.bandwidth(x[:, None], 'scott')[0])
    grid = np.linspace(x.min() - 8 * h, x.max() + 8 * h, 4001)
    dens = ref.kde(x, grid, 'scott')
    step = grid[1] - grid[0]
    area = step * (dens.sum() - 0.5 * (dens[0] + dens[-1]))
    # trapezoid error <= step^2 (b - a) / 12 max|f''|, |f''| <= max|phi''| / h^3 = 1 / (h^3 sqrt(2 pi)); tails past 8 h: < 1e-14
    assert abs(area - 1.0) <= step ** 2 * (grid[-1] - grid[0]) / 12 / (h ** 3 * np.sqrt(2 * np.pi)) + 1e-13


def test_degenerate_bandwidths():
    x = np.random.default_rng(2).standard_normal((100, 3))
    x[:, 0] = 1.5
    x[7, 2] = np.nan
    h = ref.bandwidth(x, 'scott')
    assert np.isnan(h[0]) and np.isfinite(h[1]) and np.isnan(h[2])
    assert np.isclose(float(h[1]), x[:, 1].std(ddof=1) * 100 ** -0.2, rtol=1e-14)


# ---- a hand-worked example

def test_hand_worked_dozen_draws():
    from hallthrusterpem_amd import marginals
    a = np.array([0.0, 0.5, 1.0, 1.0, 1.5, 2.9, 3.0, 3.0, 2.0, 1.9, 0.1, 2.0])
    b = np.array([10., 10., 10., 11., 11., 13., 13., 12., 12., 14., -1., 11.])
    x = np.stack([a, b], axis=1)
    ranges = [(0.0, 3.0), (10.0, 13.0)]                   # edges 0 1 2 3 and 10 11 12 13; b = 14 and b = -1 fall outside
    edges = ref.make_edges(x, 3, ranges)
    assert np.array_equal(edges, [[0, 1, 2, 3], [10, 11, 12, 13]])
    h1, h2, dropped, nonfinite = ref.histograms(x, edges)
    # a: [0, 1): 0, .5, .1 -> 3;  [1, 2): 1, 1, 1.5, 1.9 -> 4;  [2, 3]: 2.9, 3, 3, 2, 2 -> 5
    # b: [10, 11): 3;  [11, 12): 11, 11, 11 -> 3;  [12, 13]: 13, 13, 12, 12 -> 4;  14 and -1 dropped
    assert np.array_equal(h1, [[3, 4, 5], [3, 3, 4]]) and list(dropped) == [0, 2] and list(nonfinite) == [0, 0]
    # pairs (bin a, bin b): (0,0) (0,0) (1,0) (1,1) (1,1) (2,2) (2,2) (2,2) (2,2) [1.9, 14: dropped] [0.1, -1: dropped] (2,1)
    want = np.array([[2, 0, 0], [1, 2, 0], [0, 1, 4]])
    assert np.array_equal(h2[0, 1], want) and np.array_equal(h2[1, 0], want.T)
    assert np.array_equal(h2[0, 0], np.diag([3, 4, 5])) and np.array_equal(h2[1, 1], np.diag([3, 3, 4]))
    # levels: sorted 4 2 2 1 1 0..., cumulative 4 6 8 9 10; total 10: mass 0.5 -> 5 reached at the second cell (2), 0.9 -> 9 at the fourth (1)
    assert list(ref.credible_levels(want)) == [2, 1] and list(marginals.credible_levels(want)) == [2, 1]
    # corner's assembly at cmin = 2, on the ten draws inside the ranges (their min and max ARE the ranges, so the edges and
    # the pair table are the ones above); cells with fewer than 2 draws are blanked
    inside = x[(b >= 10) & (b <= 13)]
    c = ref.corner(inside[:, None, :], burnin=0.0, bins=3, cmin=2, points=4)
    assert c['n_draws'] == 10 and np.array_equal(c['edges'], edges) and np.array_equal(c['hist2d'][0, 1], want)
    assert np.array_equal(c['hist1d'], [[2, 3, 5], [3, 3, 4]])
    assert np.array_equal(c['mask'][0, 1], [[False, True, True], [True, False, True], [True, True, False]])
    assert np.array_equal(c['mask'][1, 0], c['mask'][0, 1].T) and np.array_equal(c['mask'][0, 0], np.diag([2, 3, 5]) < 2)
    assert c['levels'][0, 1].tolist() == [2, 1] and c['levels'][0, 0].tolist() == [5, 2]
    table = [[5, 1, 0], [2, 9, 1], [0, 1, 1]]
    assert list(marginals.credible_levels(table)) == [5, 1] and list(ref.credible_levels(table)) == [5, 1]
    assert list(marginals.credible_levels(np.zeros((3, 3), int))) == [0, 0]
    assert marginals.credible_levels(np.stack([table, want]), mass=(0.5,)).tolist() == [[5], [2]]
