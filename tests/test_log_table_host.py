"""csrc/pem_log_table.h held to mpmath entry by entry, and csrc/pem_math.h's log10 / 10^x -- restated in tests/hp_math.py -- held to a
long-double and mpmath reference over the argument sets the device tests (tests/test_math_kernels.py) and the device measurement
(tools/microbench/pem_math_ulps.hip, profiles/pem_math_r01.txt) use.  No GPU.  Every test prints the figure it asserts."""
import re

import numpy as np
import pytest

import hp_math as M

HEADER = (M.CSRC / 'pem_log_table.h').read_text()


def _entry(text, k):
    """(start, end, token) of the k-th hex double of the table"""
    body = re.search(r'PEM_LOG10_TAB\[\d+\] = \{', text).end()
    m = list(re.finditer(r'-?0x[0-9a-fA-F.]+p[-+]?\d+', text[body:]))[k]
    return body + m.start(), body + m.end(), m.group(0)


def _flip(tok):
    """the hex double with the last bit of its significand flipped"""
    v = np.array([float.fromhex(tok)])
    v.view(np.int64)[0] ^= 1
    return float(v[0]).hex()


def _replace(text, k, new):
    a, b, _ = _entry(text, k)
    return text[:a] + new + text[b:]


def _mutants():
    out = {}
    out['the last bit of c[500] flipped'] = _replace(HEADER, 2 * 500, _flip(_entry(HEADER, 2 * 500)[2]))
    out['the last bit of T[700] flipped'] = _replace(HEADER, 2 * 700 + 1, _flip(_entry(HEADER, 2 * 700 + 1)[2]))
    c300, t300, c301, t301 = (_entry(HEADER, k)[2] for k in (600, 601, 602, 603))
    swapped = HEADER
    for k, tok in ((600, c301), (601, t301), (602, c300), (603, t300)):
        swapped = _replace(swapped, k, tok)
    out['entries 300 and 301 swapped'] = swapped
    low = M.header()['LOW_BELOW']
    out['LOW_BELOW + 1'] = HEADER.replace(f'#define PEM_LOG_LOW_BELOW {low}', f'#define PEM_LOG_LOW_BELOW {low + 1}')
    out['LOW_BELOW - 1'] = HEADER.replace(f'#define PEM_LOG_LOW_BELOW {low}', f'#define PEM_LOG_LOW_BELOW {low - 1}')
    a3 = re.search(r'#define PEM_LOG_A3 (\S+)', HEADER).group(1)
    out['the last bit of A3 flipped'] = HEADER.replace(f'#define PEM_LOG_A3 {a3}', f'#define PEM_LOG_A3 {_flip(a3)}')
    return out


def test_the_committed_header_is_what_the_method_says():
    """counts and defines; c_0 = 2, c_1023 = 1, both T = 0; every other T_i the correctly rounded -log10(c_i) + [i < LOW_BELOW] log10 2
    from the rounded c_i; c_i within 600 ulp of 1 / centre; |r| <= 2^-11 over every interior interval (2^-10 / 2^-11 at the ends);
    LOW_BELOW the first interval that reaches sqrt(1/2); signs and monotonicity of T; A_k correctly rounded"""
    h = M.header()
    assert (h['NBITS'], h['N'], h['LOW_BELOW']) == (10, 1024, 424) and h['tab'].size == 2048
    assert M.header_failures(HEADER) == []


@pytest.mark.parametrize('name', list(_mutants()))
def test_every_mutant_of_the_header_is_caught(name):
    """a copy of the header's text with one defect, through the same checks: at least one must turn red"""
    text = _mutants()[name]
    assert text != HEADER
    bad = M.header_failures(text)
    print(name, '->', bad[:3])
    assert bad, f'{name}: not noticed'


def test_gal_miss_is_what_the_generator_documents():
    """T_i is a double to within 0.06 ulp (the generator's search over the 1201 candidates reaches that, not the 1e-3 it aims at)"""
    import mpmath as mp
    h = M.header()
    worst = 0.0
    with mp.workdps(40):
        for i in range(1, h['N'] - 1):
            Tm = -mp.log10(mp.mpf(float(h['c'][i]))) + (mp.log10(2) if i < h['LOW_BELOW'] else 0)
            worst = max(worst, float(abs(Tm - mp.mpf(float(h['T'][i]))) / mp.mpf(float(np.spacing(abs(h['T'][i]))))))
    print(f'worst Gal miss {worst:.4f} ulp')
    assert worst <= 0.06


def test_table_log10_over_its_argument_set():
    x, got = M.log10_args(), M.restated('log10_tab')
    bound, cases = M.near_one_bound()
    w = M.worst_error(x, got, 'log10', bound)               # (mpmath for every argument within 0.01 ulp of the bound)
    near = (x >= 1.0 - 2.0 ** -11) & (x < 1.0 + 2.0 ** -10)
    w_far = M.worst_error(x[~near], got[~near], 'log10', bound)
    print(f'{w["rechecked"]} arguments scored against mpmath')
    print(f'log10_tab: {x.size} arguments, worst {w["normal"][0]:.4f} ulp at {w["normal"][1].hex()}; outside entries 0 and 1023 '
          f'{w_far["normal"][0]:.4f} ulp at {w_far["normal"][1].hex()}; derived bound in entries 0 and 1023 {bound:.4f} ulp {cases}')
    assert w['denormal'][1] is None
    # the sampled worst lies under the derived bound, the bound under the constant, and the constant is the bound rounded up to a tenth
    assert w['normal'][0] <= bound <= M.LOG10_TAB_ULPS
    assert np.ceil(10.0 * bound) / 10.0 == M.LOG10_TAB_ULPS
    assert w_far['normal'][0] <= bound
    # the documented 1.3 ulp was wrong: the bound and one argument exceed it (mpmath)
    import mpmath as mp
    xw = float.fromhex('0x1.0024d25b66d4cp+0')
    with mp.workdps(50):
        t = mp.log10(mp.mpf(xw))
        e = float(abs(mp.mpf(float(M.log10_tab(np.array([xw]))[0])) - t) * mp.mpf(2) ** (52 - int(mp.floor(mp.log(t, 2)))))
    print(f'log10_tab({xw.hex()}): {e:.5f} ulp against mpmath')
    assert 1.3 < e <= bound


def test_table_log10_special_and_exact_values():
    got = M.log10_tab(np.array(M.LOG10_SPECIALS))
    assert np.array_equal(got, np.array(M.LOG10_SPECIALS_WANT), equal_nan=True), got
    assert np.array_equal(M.bits(M.log10_tab(np.array([1.0, 1e-20]))), M.bits(np.array([0.0, -20.0])))
    got = M.log10_series(np.array(M.LOG10_SPECIALS))
    assert np.array_equal(got, np.array(M.LOG10_SPECIALS_WANT), equal_nan=True), got


def test_series_log10_over_its_argument_set():
    """with the IEEE quotient (PEM_LOG10_IEEE_DIV); the device's own quotient is measured by tools/microbench/pem_math_ulps.hip"""
    x = M.log10_args()
    w = M.worst_error(x, M.restated('log10_series'), 'log10', M.LOG10_SERIES_ULPS)
    print(f'log10_series (IEEE quotient): {x.size} arguments, worst {w["normal"][0]:.4f} ulp at {w["normal"][1].hex()}')
    assert w['normal'][0] <= M.LOG10_SERIES_ULPS
    one = M.log10_series(np.array([1.0, 1e-20]))
    assert one[0] == 0.0 and abs(one[1] + 20.0) <= M.LOG10_SERIES_ULPS * np.spacing(20.0)


def test_exp10_over_its_argument_set():
    y, got = M.exp10_args(), M.restated('exp10')
    w = M.worst_error(y, got, 'exp10', M.EXP10_ULPS, M.EXP10_DENORMAL_UNITS)
    print(f'exp10: {y.size} arguments, normal results worst {w["normal"][0]:.4f} ulp at {w["normal"][1]!r}; below 2^-1022 worst '
          f'{w["denormal"][0]:.4f} units of 2^-1074 at {w["denormal"][1]!r}')
    assert w['normal'][0] <= M.EXP10_ULPS and w['denormal'][0] <= M.EXP10_DENORMAL_UNITS
    # beyond the doubles: 0 and inf exactly where the long double value rounds there
    ref = M.exp10_ld(y)
    with np.errstate(over='ignore'):
        over, under = ref > M.LD(1.7976931348623157e308) * M.LD(1.0000001), ref < M.LD(2.0 ** -1074) * M.LD(0.4999)
        assert over.any() and under.any() and (got[over] == np.inf).all() and (got[under] == 0.0).all()
    sp = M.exp10(np.array(M.EXP10_SPECIALS))
    assert np.array_equal(sp, np.array(M.EXP10_SPECIALS_WANT), equal_nan=True), sp
    assert np.array_equal(M.exp10(np.array([0.0, 1.0, 2.0, 22.0])), [1.0, 10.0, 100.0, 1e22])


def test_constants_are_the_recorded_figures_rounded_up():
    """each constant is the larger of the host's worst and the device's (profiles/pem_math_r01.txt) rounded up to the next half ulp;
    the table log10's is the derived bound rounded up to a tenth, and the record lies under it"""
    rec = M.recorded()
    print(rec)
    assert rec['clean'] and rec['differs'] == 0
    x, y = M.log10_args(), M.exp10_args()
    host_series = M.worst_error(x, M.restated('log10_series'), 'log10', None)['normal'][0]
    host_exp = M.worst_error(y, M.restated('exp10'), 'exp10', None)
    assert M.half_up(max(rec['pem_log10']['normal'], host_series)) == M.LOG10_SERIES_ULPS
    assert M.half_up(max(rec['pem_exp10']['normal'], host_exp['normal'][0])) == M.EXP10_ULPS
    assert M.half_up(max(rec['pem_exp10']['denormal'], host_exp['denormal'][0])) == M.EXP10_DENORMAL_UNITS
    assert M.half_up(max(rec['exp10']['normal'], rec['exp10']['denormal'])) == M.LIB_EXP10_ULPS
    bound, _ = M.near_one_bound()
    assert rec['pem_log10_tab']['normal'] == rec['pem_log10_tab_pos']['normal'] <= bound
    import hp_model
    import hp_reference
    assert hp_model.LOG10_TAB_ULPS is M.LOG10_TAB_ULPS and hp_model.LOG10_SERIES_ULPS is M.LOG10_SERIES_ULPS
    assert hp_reference.EXP10_REL == 2.0 * M.EXP10_ULPS * M.U < 4.5e-16 and hp_reference.LIB_EXP10_REL == 2.0 * M.LIB_EXP10_ULPS * M.U < 4.5e-16
