"""Hexagonal pair bins without a GPU: tests/hexbin_np.py equals matplotlib's `Axes.hexbin` bit for bit (counts, centres, polygon,
mincnt); pem_chain_hex_f64_dev is declared, bound, built and exported, refuses every malformed call before it looks for a device
and compiles without scratch or spills; marginals.hexbins and corner(plot2d='hex') refuse bad arguments before they touch a
device, and the lattice table and geometry marginals builds are the restatement's."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hexbin_np as ref

ROOT = Path(__file__).resolve().parents[1]
HEX = 'pem_chain_hex_f64_dev'
GRIDS = [(1, 1), (2, 1), (15, 8), (64, 36), (64, 64), (1, 64)]
LIMITS = [((-1.3, 2.9), (1e-3, 1.7e-3)), ((0.0, 1.0), (-5e4, 3e4))]


# ---- the restatement against matplotlib

@pytest.fixture(scope='module')
def axes():
    matplotlib = pytest.importorskip('matplotlib')
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots()
    yield ax
    plt.close(fig)


@pytest.mark.parametrize('nx,ny', GRIDS)
@pytest.mark.parametrize('xlim,ylim', LIMITS)
def test_restatement_equals_matplotlib_bit_for_bit(axes, nx, ny, xlim, ylim):
    """random draws, lattice points, half-integer and quarter lattice coordinates with their fp64 neighbours, both sides of
    every side of the extent and its corners; finite draws only (NaN and inf are this project's definition)"""
    rng = np.random.default_rng(100 * nx + ny)
    x, y = ref.adversarial_draws(nx, ny, xlim, ylim, rng)
    table = ref.lattice_table([xlim, ylim], nx, ny)
    ix, iy = ref.lattice_coordinates(x, table[0, 0], table[0, 1]), ref.lattice_coordinates(y, table[1, 2], table[1, 3])
    d1, d2, r1, _, _, _ = ref.distances(ix, iy)
    assert (d1 == d2).any() and (np.abs(ix - np.floor(ix)) == 0.5).any() and (ix == r1).any()      # the cases are in the draws
    want = axes.hexbin(x, y, gridsize=(nx, ny), extent=(*xlim, *ylim), mincnt=None)
    counts = ref.counts_of_pair(x, y, nx, ny, table[0], table[1])
    centers, polygon = ref.geometry(nx, ny, xlim, ylim)
    assert counts.dtype == np.int64 and counts.shape == (ref.n_cells(nx, ny),)
    assert np.array_equal(np.asarray(want.get_array()), counts)
    assert np.array_equal(np.asarray(want.get_offsets()), centers)
    assert np.array_equal(want.get_paths()[0].vertices[:6], polygon)
    assert 0 < ref.dropped_of_pair(x, y, nx, ny, table[0], table[1]) == x.size - counts.sum()
    for k in (1, 2, int(np.median(counts[counts > 0])) + 1):
        cut = axes.hexbin(x, y, gridsize=(nx, ny), extent=(*xlim, *ylim), mincnt=k)
        mask = counts < k
        assert np.array_equal(np.asarray(cut.get_array()), counts[~mask]) and np.array_equal(np.asarray(cut.get_offsets()), centers[~mask])


@pytest.mark.parametrize('gridsize', [2, 15, 64, 100])
def test_an_integer_gridsize_is_read_as_matplotlib_reads_it(axes, gridsize):
    rng = np.random.default_rng(gridsize)
    x, y = rng.standard_normal(4000), 3.0 + 0.1 * rng.standard_normal(4000)
    nx, ny = ref.grid_size(gridsize)
    want = axes.hexbin(x, y, gridsize=gridsize, extent=(-2.0, 2.0, 2.8, 3.2))
    table = ref.lattice_table([(-2.0, 2.0), (2.8, 3.2)], nx, ny)
    assert np.array_equal(np.asarray(want.get_array()), ref.counts_of_pair(x, y, nx, ny, table[0], table[1]))


def test_non_finite_values_and_huge_values_are_in_no_cell_of_the_restatement():
    table = ref.lattice_table([(0.0, 1.0), (0.0, 1.0)], 4, 3)
    x = np.array([0.5, np.nan, np.inf, -np.inf, 0.5, 0.5, 0.5, 1e300, -1e300, 3e9, 0.5, 1.7e308])
    y = np.array([0.5, 0.5, 0.5, 0.5, np.nan, np.inf, -np.inf, 0.5, 0.5, 0.5, -4e9, -1.7e308])
    c = ref.cells(x, y, 4, 3, table[0], table[1])
    assert c[0] >= 0 and np.all(c[1:] == -1)
    assert abs(ref.lattice_coordinates(3e9, table[0, 0], table[0, 1])) >= 2.0 ** 31
    assert ref.counts_of_pair(x, y, 4, 3, table[0], table[1]).sum() == 1


def test_pair_order_and_poisoning_of_the_restatement():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2000, 4))
    ext = [(-3.0, 3.0)] * 4
    clean = ref.hexbins(x, 6, 3, ext)
    assert ref.pair_list(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and clean.shape == (6, ref.n_cells(6, 3))
    t = ref.lattice_table(ext, 6, 3)
    assert np.array_equal(clean[4], ref.counts_of_pair(x[:, 1], x[:, 3], 6, 3, t[1], t[3]))
    assert not np.array_equal(clean[4], ref.counts_of_pair(x[:, 3], x[:, 1], 6, 3, t[3], t[1]))     # not symmetric in its axes
    x[rng.integers(0, 2000, 25), 2] = np.nan
    dirty = ref.hexbins(x, 6, 3, ext)
    for p, (i, j) in enumerate(ref.pair_list(4)):
        assert np.array_equal(dirty[p], clean[p]) == (2 not in (i, j)), (i, j)


# ---- the entry point without a device

def test_symbol_is_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % HEX, header)
    assert m and len(m.group(1).split(',')) == 9 and len(_lib.SIGNATURES[HEX][1]) == 9
    assert hasattr(_lib.load(), HEX)
    for macro, value in (('PEM_HEX_MAX_GRID', _lib.HEX_MAX_GRID), ('PEM_HEX_ROW_TILE', _lib.HEX_ROW_TILE)):
        assert re.search(r'#define %s (\d+)' % macro, header).group(1) == str(value)
    assert _lib.HEX_MAX_GRID == 64 and ref.n_cells(64, 64) == 8321
    assert build.PKG / 'csrc' / 'pem_hexbin.hip' in build.SRCS
    assert HEX in (ROOT / 'INTEGRATION.md').read_text()


FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host


def _hex(n_rows=100, n_par=3, ld=3, x=True, nx=15, ny=8, lattice=True, counts=True, edit=None):
    from hallthrusterpem_amd import _lib
    table = ref.lattice_table([(-1.0, 1.0)] * max(n_par, 1), 15, 8)
    if edit:
        table[edit[0], edit[1]] = edit[2]
    return _lib.load().pem_chain_hex_f64_dev(n_rows, n_par, ld, FAKE if x else None, nx, ny, C.c_void_p(table.ctypes.data) if lattice else None,
                                             FAKE if counts else None, None)


@pytest.mark.parametrize('bad', [
    dict(n_rows=0), dict(n_par=1), dict(n_par=0), dict(n_par=-2), dict(n_par=33, ld=33), dict(nx=0), dict(nx=65), dict(nx=-1), dict(ny=0),
    dict(ny=65), dict(ld=2), dict(x=False), dict(lattice=False), dict(counts=False), dict(n_rows=1 << 48),
    dict(edit=(0, 0, np.nan)), dict(edit=(1, 0, np.inf)), dict(edit=(2, 2, -np.inf)), dict(edit=(1, 2, np.nan)), dict(edit=(0, 1, 0.0)),
    dict(edit=(2, 1, -0.25)), dict(edit=(1, 1, np.nan)), dict(edit=(1, 1, np.inf)), dict(edit=(0, 3, 0.0)), dict(edit=(2, 3, -1e-300)),
    dict(edit=(2, 3, np.nan)),
])
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _hex(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_chain_hex' in _lib.load().pem_last_error()


def test_a_well_formed_call_gets_as_far_as_looking_for_a_device():
    """so the refusals above are the arguments', and the row limit is the documented one: 136 pairs at 15 x 8 are 4 task
    blocks of 34 tables, 256 row blocks, so 2^40 rows are refused and just below that the call goes on"""
    from hallthrusterpem_amd import _lib
    assert _hex(n_rows=1 << 40, n_par=17, ld=17) == _lib.PEM_ERR_INVALID_ARG
    assert _hex(n_rows=1 << 42, n_par=2, ld=2) == _lib.PEM_ERR_INVALID_ARG
    if _lib.device_count() == 0:
        assert _hex() == _lib.PEM_ERR_NO_DEVICE
        assert _hex(n_par=32, ld=40, nx=64, ny=64) == _lib.PEM_ERR_NO_DEVICE and _hex(n_par=2, ld=2, nx=1, ny=1) == _lib.PEM_ERR_NO_DEVICE
        assert _hex(n_rows=(1 << 40) - (1 << 15), n_par=17, ld=17) == _lib.PEM_ERR_NO_DEVICE


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_hex_kernel_has_no_scratch_and_no_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_hexbin.hip')],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), sspill=int(m.group(4)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    assert sorted(rows) == ['chain_hex_kernel'], rows
    r = rows['chain_hex_kernel']
    assert r['vspill'] == 0 and r['sspill'] == 0 and r['scratch'] == 0, r
    assert r['vgpr'] <= 168                                            # three waves per SIMD


# ---- Python refusals: raised from shapes and arguments alone, before any device is looked for

@pytest.mark.parametrize('call', [
    lambda m, x: m.hexbins(x, gridsize=0), lambda m, x: m.hexbins(x, gridsize=65), lambda m, x: m.hexbins(x, gridsize=1),
    lambda m, x: m.hexbins(x, gridsize=2.5), lambda m, x: m.hexbins(x, gridsize=(15,)), lambda m, x: m.hexbins(x, gridsize=(15, 0)),
    lambda m, x: m.hexbins(x, gridsize=(65, 8)), lambda m, x: m.hexbins(x, gridsize=(15, 8, 3)), lambda m, x: m.hexbins(x, gridsize=(15, 2.5)),
    lambda m, x: m.hexbins(x, gridsize='15'), lambda m, x: m.hexbins(x, gridsize=None), lambda m, x: m.hexbins(x, gridsize=(-3, 4)),
    lambda m, x: m.hexbins(x, extent=[(0, 1)]), lambda m, x: m.hexbins(x, extent=[(0, 1), (2, 1), (0, 1)]),
    lambda m, x: m.hexbins(x, extent=[(0, 1), (0, np.inf), (0, 1)]), lambda m, x: m.hexbins(x, extent=[(0, 1), (np.nan, 1), (0, 1)]),
    lambda m, x: m.hexbins(x, extent=(0, 1, 0, 1)), lambda m, x: m.hexbins(np.zeros((20, 2, 33))), lambda m, x: m.hexbins(x[:, :, :1]),
    lambda m, x: m.hexbins(x, burnin=1.0), lambda m, x: m.hexbins(x[:3], burnin=0.0), lambda m, x: m.hexbins(x[:, 0, 0]),
    lambda m, x: m.corner(x, plot2d='kde'), lambda m, x: m.corner(x, plot2d='hexagon'), lambda m, x: m.corner(x, plot2d=None),
    lambda m, x: m.corner(x, plot2d='hex', bins=1), lambda m, x: m.corner(x, plot2d='hex', gridsize=(15, 0)),
    lambda m, x: m.corner(x, plot2d='hex', gridsize=65), lambda m, x: m.corner(x, plot2d='hex', gridsize=(3, 4, 5)),
    lambda m, x: m.corner(x, plot2d='hex', select=[1]), lambda m, x: m.corner(x, plot2d='hex', cmin=-1),
    lambda m, x: m.corner(np.zeros((20, 2, 33)), plot2d='hex'),
])
def test_python_refusals_come_before_the_device(call, monkeypatch):
    from hallthrusterpem_amd import _lib, marginals
    monkeypatch.setattr(_lib, 'require_device', lambda: pytest.fail('a device was looked for'))
    with pytest.raises(ValueError):
        call(marginals, np.zeros((20, 4, 3)))


@pytest.mark.parametrize('gridsize,want', [(15, (15, 8)), (2, (2, 1)), (64, (64, 36)), ((64, 64), (64, 64)), ((1, 64), (1, 64)), ([7, 3], (7, 3)),
                                           (np.int64(15), (15, 8)), (15.0, (15, 8))])
def test_gridsize_is_read_as_the_restatement_reads_it(gridsize, want):
    from hallthrusterpem_amd import marginals
    assert marginals._check_gridsize(gridsize, 3) == want == ref.grid_size(gridsize)


@pytest.mark.parametrize('nx,ny', GRIDS)
def test_lattice_table_and_geometry_of_marginals_equal_the_restatement(nx, ny):
    from hallthrusterpem_amd import marginals
    rng = np.random.default_rng(nx + ny)
    lo = rng.standard_normal(6) * [1.0, 1e-6, 3e4, 0.1, 1e3, 1.0]
    ext = np.stack([lo, lo + rng.uniform(0.1, 2.0, 6) * [1.0, 1e-6, 3e4, 0.1, 1e-9, 1e12]], axis=1)
    ext[5] = 2.5, 2.5                                                  # a constant parameter: widened by 0.5 either side
    want_ext = ref.make_extent(np.zeros((1, 6)), ext)
    got_ext = marginals._hex_extent(None, marginals._check_extent(ext, 6))
    assert np.array_equal(got_ext, want_ext) and got_ext[5].tolist() == [2.0, 3.0]
    table = marginals._hex_table(got_ext, nx, ny)
    assert table.dtype == np.float64 and table.flags.c_contiguous and np.array_equal(table, ref.lattice_table(want_ext, nx, ny))
    for i, j in ((0, 1), (2, 4), (3, 5)):
        c, p = marginals.hex_lattice(nx, ny, got_ext[i], got_ext[j])
        wc, wp = ref.geometry(nx, ny, want_ext[i], want_ext[j])
        assert np.array_equal(c, wc) and np.array_equal(p, wp) and c.shape == (ref.n_cells(nx, ny), 2) and p.shape == (6, 2)
    with pytest.raises(ValueError):
        marginals.hex_lattice(0, 3, (0, 1), (0, 1))


def test_default_extent_is_the_finite_minimum_and_maximum():
    from hallthrusterpem_amd import marginals
    x = np.array([[1.0, 5.0, np.nan], [np.nan, 5.0, np.nan], [3.0, 5.0, np.inf], [-2.0, 5.0, np.nan]])
    want = ref.make_extent(x)
    assert want.tolist() == [[-2.0, 3.0], [4.5, 5.5], [0.0, 1.0]]
    assert np.array_equal(marginals._hex_extent(None, None, (np.array([-2.0, 5.0, 0.0]), np.array([3.0, 5.0, 1.0]))), want)
