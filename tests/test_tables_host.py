"""csrc/pem_tables.h, the committed generated header of the fp64 model kernels, against the truth.  No GPU.

normaliser() and simpson_functionals() of csrc/pem_model.h are restated bit-faithfully (tests/hp_model.py: an exact fma) on the tables
PARSED from the header and compared with mpmath; the Simpson weights with scipy's, bit for bit; rows of the header with what
tools/gen_tables.py's functions produce today, hex literal for hex literal.  Four mutants of the header must each turn this file red.
The measured worst errors are module constants of tests/hp_model.py (TABLE_D_ERR, TABLE_QD_ERR, TABLE_QN_ERR, EXPNP_ULPS) and are
asserted here; DESIGN section 4.1 and the comments of pem_model.h quote them."""
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
sys.path.insert(0, str(ROOT / 'tools'))

import hp_model as hp  # noqa: E402

mp = pytest.importorskip('mpmath')
U = hp.U
HEADER = hp.CSRC / 'pem_tables.h'


def _rel(got, want):
    """|got - want| / |want| for a double and an mpmath number, as a float"""
    return float(abs(mp.mpf(float(got)) - want) / abs(want))


_truth = {}


def _d_truth(x):
    if ('d', x) not in _truth:
        _truth[('d', x)] = hp.D_mp(x)
    return _truth[('d', x)]


def _q_truth(x, tab):
    """(the weights define Q: the truth is cached for the committed weights only)"""
    key = ('q', x, tab['SIMPSON_CDEN'].tobytes(), tab['SIMPSON_CNUM'].tobytes())
    if key not in _truth:
        _truth[key] = hp.Q_mp(x, tab)
    return _truth[key]


def _d_errors(tab):
    """per point of hp.table_points() (and eight random points per interval): the error of the restated normaliser against the closed
    form at 50 digits, in units of U"""
    a, _ = hp.table_points()
    rng = np.random.default_rng(11)
    a = np.unique(np.concatenate([a, 1.0 / np.sqrt(np.repeat(np.arange(tab['NDI']) / 2.0, 8) + rng.uniform(1e-3, 0.5, 8 * tab['NDI']))]))
    got = hp.normaliser64(a, tab)
    return a, np.array([_rel(g, _d_truth(x)) for g, x in zip(got, a)]) / U


def _q_errors(tab):
    _, a = hp.table_points()
    rng = np.random.default_rng(12)
    a = np.unique(np.concatenate([a, tab['QA_MIN'] + rng.uniform(0.0, tab['NQB'], 4 * tab['NQB']) / tab['QB_SCALE'],
                                  1.0 / np.sqrt(rng.uniform(1e-3, 16.0, 4 * tab['NDI']))]))
    qd, qn = hp.functionals64(a, tab)
    ed, en = [], []
    for g1, g2, x in zip(qd, qn, a):
        td, tn = _q_truth(x, tab)
        ed.append(_rel(g1, td))
        en.append(_rel(g2, tn))
    return a, np.array(ed) / U, np.array(en) / U


def _half_ulp_up(v):
    """a worst error in units of U rounded up to the next half ulp (an ulp is 2 U)"""
    return math.ceil(v) * U


# the checks of a header, each raising AssertionError: the tests below run them on the committed header, the mutant tests on edited copies
def check_d(path=None):
    a, e = _d_errors(hp.tables(path))
    worst = float(e.max())
    assert worst * U <= hp.TABLE_D_ERR, f'D(a) is off by {worst:.3f} u at a = {a[e.argmax()]!r}'
    assert hp.TABLE_D_ERR == _half_ulp_up(worst), f'TABLE_D_ERR = {hp.TABLE_D_ERR / U} u, measured {worst:.3f} u'
    return a, e


def check_q(path=None):
    a, ed, en = _q_errors(hp.tables(path))
    for name, e, const in (('Qd', ed, hp.TABLE_QD_ERR), ('Qn', en, hp.TABLE_QN_ERR)):
        worst = float(e.max())
        assert worst * U <= const, f'{name}(a) is off by {worst:.3f} u at a = {a[e.argmax()]!r}'
        assert const == _half_ulp_up(worst), f'{name}: the constant is {const / U} u, measured {worst:.3f} u'
    return a, ed, en


def check_simpson(path=None):
    """CDEN[k] = w_m cos(x_m), CNUM[k] = CDEN[k] sin(x_m), m = 90 - k, w the weights scipy.integrate.simpson gives the grid"""
    from scipy.integrate import simpson
    tab = hp.tables(path)
    x = np.linspace(0, np.pi / 2, 91)
    w = np.array([simpson(np.eye(91)[m], x=x) for m in range(91)])
    cden = (w * np.cos(x))[::-1]
    cnum = cden * np.sin(x)[::-1]
    assert np.array_equal(tab['SIMPSON_CDEN'], cden)
    assert np.array_equal(tab['SIMPSON_CNUM'], cnum)


def _hex_rows(name, path=None):
    body = re.search(r'%s\[\d+\] = \{(.*?)\};' % name, Path(path or HEADER).read_text(), re.S).group(1)
    return [re.findall(r'-?0x[0-9a-fA-F.]+p[-+]?\d+', re.sub(r'//[^\n]*', '', line)) for line in body.strip().split('\n')]


def check_regeneration(path=None, polys=True):
    """first, a middle and the last row of DPOLY and of each QPOLY region, the Dawson row, the Simpson rows and the #defines: the hex
    literals of the header, exactly (the whole regeneration takes 40 s and is not run)"""
    import gen_tables as gt
    text = Path(path or HEADER).read_text()
    for k, v in gt.defines().items():
        assert re.search(r'#define %s %s\n' % (k, re.escape(v)), text), k
    cden, cnum = gt.simpson_tables()
    assert [r[0] for r in _hex_rows('PEM_SIMPSON_CDEN', path)] == [gt.hexd(v) for v in cden]
    assert [r[0] for r in _hex_rows('PEM_SIMPSON_CNUM', path)] == [gt.hexd(v) for v in cnum]
    assert [r[0] for r in _hex_rows('PEM_DAWSON', path)] == [gt.hexd(v) for v in gt.dawson_table()]
    if not polys:
        return
    rows = (0, gt.NDI // 2, gt.NDI - 1)
    committed = _hex_rows('PEM_DPOLY', path)
    assert len(committed) == gt.NDI
    for i, row in zip(rows, gt.dpoly_tables(rows)):
        assert committed[i] == [gt.hexd(v) for v in row], f'DPOLY row {i}'
    qrows = rows + (gt.NDI, gt.NDI + gt.NQB // 2, gt.NDI + gt.NQB - 1)
    committed = _hex_rows('PEM_QPOLY', path)
    assert len(committed) == gt.NDI + gt.NQB
    for i, (qd, qn) in zip(qrows, gt.qpoly_tables(cden, cnum, qrows)):
        assert committed[i] == [h for a, b in zip(qd, qn) for h in (gt.hexd(a), gt.hexd(b))], f'QPOLY row {i}'


def test_exact_fma_is_exact():
    """the emulated fma against rational arithmetic, cancelling cases included; and against math.fma where Python has it"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a, b, c = rng.standard_normal((3, 4000)) * 10.0 ** rng.integers(-8, 8, (3, 4000))
    c[:2000] = -(a * b)[:2000] * (1.0 + rng.standard_normal(2000) * 1e-16)          # a b + c cancels to the last bits of the product
    c[2000:2200] = -(a * b)[2000:2200]
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(hp.fma_eft(a, b, c), want)
    assert np.array_equal(hp.fma(a, b, c), want)
    assert ((a * b + c) != want).sum() > 100                        # the twice-rounded stand-in is NOT the same thing


def test_closed_form_of_the_normaliser_is_the_integral():
    for a in (1e-3, 0.0044, 0.03, 0.2, 0.25, 1.0, 1.63299, 10.0, 53.28):
        assert abs(hp.D_mp(a) / hp.D_quad_mp(a) - 1) < mp.mpf(10) ** -35, a


def test_dpoly_and_dawson_against_mpmath():
    """both sides of every one of the 32 interval edges, the index clamp at u = 16, both sides of |a| = 0.25, interior points of every
    interval (a = 1.63299 among them), a down to 1e-3 and up to 53.28"""
    a, e = check_d()
    tab = hp.tables()
    assert a.min() <= 1e-3 and a.max() >= 53.28 and np.any(np.abs(a - 1.63299) < 1e-6)
    for i in range(1, tab['NDI'] + 1):                              # the doubles on both sides of every edge are among the points
        edge = 1.0 / math.sqrt(i / 2.0)
        assert np.any((a > edge) & (a < edge * (1 + 1e-15))) and np.any((a < edge) & (a > edge * (1 - 1e-15)))
    series = a < 0.25
    print(f'D(a): worst {e.max():.3f} u = {e.max() * U:.3e} at a = {a[e.argmax()]!r}; table {e[~series].max():.3f} u, series {e[series].max():.3f} u, '
          f'at a = 1.63299: {e[np.argmin(np.abs(a - 1.63299))] * U:.3e}')


def test_normaliser_symmetry_and_nan_rule():
    a = np.array([1e-3, 0.1, 0.25, 1.0, 1.63299, 53.28, hp.ALPHA_OVERFLOW])
    assert np.array_equal(hp.normaliser64(-a), hp.normaliser64(a)) and np.all(np.isfinite(hp.normaliser64(a)))
    bad = np.array([0.0, -0.0, np.nextafter(hp.ALPHA_OVERFLOW, np.inf), -np.nextafter(hp.ALPHA_OVERFLOW, np.inf), 54.0, 1e300, np.inf, -np.inf, np.nan])
    assert np.all(np.isnan(hp.normaliser64(bad)))
    # the index clamp: u = 16 and above it use the last row (the series takes over below |a| = 0.25; the row is still evaluated)
    tab = hp.tables()
    assert np.array_equal(hp._to_int(np.array([2.0 * 16.0, 2.0 * 17.0, np.inf, np.nan])), [32, 34, 2 ** 31 - 1, 0])
    assert hp.normaliser64(np.array([0.25]))[0] == hp._horner(tab['DPOLY'][[31]], np.array([1.0]))[0]


def test_qpoly_against_the_91_term_sums():
    """both regions in every interval, both sides of QA_MIN and of 0.25, a = 0.184687"""
    a, ed, en = check_q()
    tab = hp.tables()
    assert np.any(np.abs(a - 0.184687) < 1e-9) and a.min() == tab['QA_MIN']
    for lo, hi in [(tab['QA_MIN'] + j / tab['QB_SCALE'], tab['QA_MIN'] + (j + 1) / tab['QB_SCALE']) for j in range(tab['NQB'])] + \
                  [(1.0 / math.sqrt((i + 1) / 2.0), 1.0 / math.sqrt(max(i, 1e-7) / 2.0)) for i in range(tab['NDI'])]:
        assert ((a > lo) & (a < hi)).sum() >= 4, (lo, hi)
    assert np.any(a == np.nextafter(0.25, 0)) and np.any(a == 0.25) and np.any(a == np.nextafter(tab['QA_MIN'], 1))
    # below QA_MIN the kernel does not use the table (the sample is not `plain`)
    for name, e in (('Qd', ed), ('Qn', en)):
        print(f'{name}(a): worst {e.max():.3f} u = {e.max() * U:.3e} at a = {a[e.argmax()]!r}; region A {e[a >= 0.25].max():.3f} u, region B {e[a < 0.25].max():.3f} u, '
              f'at a = 0.184687: {e[np.argmin(np.abs(a - 0.184687))] * U:.3e}')


def test_exp_nonpos_against_mpmath():
    """exp_nonpos restated with the exact fma over [-708, 0]: random arguments, small ones, and the multiples of ln 2 / 2 where the
    reduced argument is largest"""
    rng = np.random.default_rng(3)
    x = np.concatenate([-rng.uniform(0, 708, 6000), -10.0 ** rng.uniform(-8, 0, 1500), -np.arange(1, 2043) * (math.log(2) * 0.5), [0.0, -0.0]])
    x = x[x >= -708.0]
    g = hp.exp_nonpos64(x)
    with mp.workdps(30):
        e = np.array([float(abs(mp.mpf(float(gg)) - mp.exp(mp.mpf(float(xx)))) / mp.mpf(float(np.spacing(gg)))) for gg, xx in zip(g, x)])
    print(f'exp_nonpos: worst {e.max():.4f} ulp at x = {x[e.argmax()]!r}')
    assert e.max() <= hp.EXPNP_ULPS and hp.EXPNP_ULPS == math.ceil(2.0 * e.max()) / 2.0


def test_exp_nonpos_truncation():
    """the degree-13 polynomial of exp_nonpos with its double coefficients, evaluated exactly, against e^r on |r| <= ln 2 / 2 (a little
    beyond: the reduced argument carries the rounding of n ln 2): the 1.3e-17 of pem_model.h's comment"""
    with mp.workdps(40):
        worst = mp.mpf(0)
        for r in np.linspace(-1.0, 1.0, 401) * (math.log(2) * 0.5 * (1 + 1e-9)):
            p = mp.mpf(hp._EXPNP[0])
            for c in hp._EXPNP[1:]:
                p = p * mp.mpf(float(r)) + mp.mpf(c)
            worst = max(worst, abs(p / mp.exp(mp.mpf(float(r))) - 1))
    print(f'exp_nonpos: truncation and coefficient rounding {float(worst):.2e}')
    assert worst <= 1.3e-17


def test_simpson_weights_are_scipys_bit_for_bit():
    check_simpson()


def test_generator_reproduces_the_committed_literals():
    check_regeneration()


# ---------------------------------------------------------------------------------------------------------------------------------
# the mutants: an edited copy of the header, and the check that must turn red on it
# ---------------------------------------------------------------------------------------------------------------------------------
def _edit_literal(tmp_path, name, row, col, new):
    """a copy of the header with literal `col` of line `row` of table `name` replaced by new(value) (None: the literal removed)"""
    text = HEADER.read_text()
    m = re.search(r'%s\[\d+\] = \{\n(.*?)\};' % name, text, re.S)
    lines = m.group(1).split('\n')
    toks = list(re.finditer(r'-?0x[0-9a-fA-F.]+p[-+]?\d+,?', lines[row]))
    t = toks[col]
    repl = '' if new is None else float(new(float.fromhex(t.group(0).rstrip(',')))).hex() + ','
    lines[row] = lines[row][:t.start()] + repl + lines[row][t.end():]
    out = tmp_path / 'pem_tables.h'
    out.write_text(text[:m.start(1)] + '\n'.join(lines) + text[m.end(1):])
    return out


def test_mutant_dpoly_coefficient_scaled_by_1e_13(tmp_path):
    """(it passes every other test of the suite: the kernels are held to 1e-10 there)"""
    path = _edit_literal(tmp_path, 'PEM_DPOLY', 7, 0, lambda v: v * (1.0 + 1e-13))
    assert hp.tables(path)['DPOLY'][7, 0] != hp.tables()['DPOLY'][7, 0]
    with pytest.raises(AssertionError, match='D\\(a\\) is off'):
        check_d(path)


def test_mutant_qpoly_row_swapped_with_its_neighbour(tmp_path):
    text = HEADER.read_text()
    m = re.search(r'PEM_QPOLY\[\d+\] = \{\n(.*?)\};', text, re.S)
    lines = m.group(1).split('\n')
    lines[40], lines[41] = lines[41], lines[40]
    path = tmp_path / 'pem_tables.h'
    path.write_text(text[:m.start(1)] + '\n'.join(lines) + text[m.end(1):])
    with pytest.raises(AssertionError, match='is off'):
        check_q(path)


def test_mutant_simpson_weight_off_by_one_ulp(tmp_path):
    for name, row in (('PEM_SIMPSON_CDEN', 17), ('PEM_SIMPSON_CNUM', 60)):
        path = _edit_literal(tmp_path, name, row, 0, lambda v: np.nextafter(v, np.inf))
        with pytest.raises(AssertionError):
            check_simpson(path)
        with pytest.raises(AssertionError):
            check_regeneration(path, polys=False)


def test_mutant_last_dawson_coefficient_dropped(tmp_path):
    """the tenth term is 4e-23 of the sum at |a| = 0.25, so no error measurement can see it: the header no longer parses to NDAW
    coefficients, or -- zeroed instead of removed -- is no longer what the generator writes"""
    with pytest.raises(AssertionError):
        hp.tables(_edit_literal(tmp_path, 'PEM_DAWSON', 9, 0, None))
    with pytest.raises(AssertionError):
        check_regeneration(_edit_literal(tmp_path, 'PEM_DAWSON', 9, 0, lambda v: 0.0), polys=False)
