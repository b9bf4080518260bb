"""The single-precision model (csrc/pem_model_f32.h) restated in numpy, and the per-sample bound that holds it to the fp64 CPU
oracle.  TEST INFRASTRUCTURE, no GPU needed.

(a) `restate(x, k, radius)` -- coupled_f32 operation by operation in the order of pem_model_f32.h, vectorised over samples, with the
    tables PARSED from csrc/pem_tables_f32.h (so the committed header is what is tested).  Conventions:
      * fmaf(a, b, c) = float32(float64(a) * float64(b) + float64(c)).  The product of two floats is exact in double; the sum is
        rounded to double and then to float, i.e. TWICE.  Where the exact sum lies within 2^-53 relative of the midpoint of two
        floats the double rounding can land on the other neighbour: half an ulp of float32, in rare ties (about one fma in 2^29).
      * v_rcp_f32, v_sqrt_f32, __expf, __logf and acosf are restated as the correctly rounded float32 of the fp64 function.  The raw
        instructions v_rcp_f32 / v_sqrt_f32 read a denormal argument as zero and write a denormal result as zero, and __expf writes a
        result below 2^-126 as zero (profiles/fp32_intrinsics_r01.txt); that is restated too.
      * (int)t is the conversion of v_cvt_i32_f32: truncation, NaN -> 0, saturating.
    It returns V_cc, div_angle, T_c, the `invalid` flag, the `plain` predicate and the intermediates a1, a2, X1, X2, den, num (and more).
    It is NOT the reference.  It says which path a sample took, it is what the kernel is compared with bit-closely, and it lets the
    bound below be checked without a GPU.

(b) The reference is oracle_ctypes.coupled / plume_terms on the FLOAT-ROUNDED INPUTS WIDENED TO DOUBLE, with torr2pa the float the
    entry point takes (it is a `float` argument of pem_coupled_f32_dev), also widened.  The oracle's own error (4e-14) is 1e-6 of a
    float ulp.  `reference(x32, k, radius)` adds what the bound needs from fp64 restatements of the oracle's formulas (the unclamped
    V_cc, the 91 terms of the two Simpson sums with the fp64 weights of csrc/pem_tables.h).

    `bounds(ref)` gives, per sample, the largest error a correct evaluation in float arithmetic can make.  u = U32 = 2^-24 is the
    relative rounding error of one float operation; an intrinsic with a worst error of E ulp has relative error <= 2 E u (an ulp
    is at most 2^-23 of the value).  R, S, L, A = 2 x the measured ulps of rcp, sqrt, __logf, acosf; X(t) = 2 x the measured ulps of
    __expf in the binade of |t| (the figures: *_ULPS below, measured exhaustively by tools/microbench/f32_intrinsics.hip, each rounded
    UP to the next half ulp and to nothing more).  Every bound is first order in u and multiplied by SECOND = 1.01 for the products of
    errors; the one place where a first-order error can be large, the quotient num / den of cancelling sums, is handled explicitly.

    V_cc = clamp(V, 0, V_a),  V = V_vac + T_e log(w) - t3,  w = 1 + z,  z = PB / PT,  t3 = T_e PB / (PT + PS):
      PB, PT, PS = P k: one rounding each.  z = PB * rcp(PT): (3 + R) u.  w = fl(1 + z): u |w| + (3 + R) u |z| absolute, which the
      logarithm turns into the ABSOLUTE error u (1 + (3 + R) |z / w|) whatever the size of log(w); __logf adds L u |log w|.
      fmaf(T_e, lg, V_vac) rounds once: u (|V_vac| + |T_e log w|).  q = T_e * rcp(PT + PS): the sum (1 + cs) u with
      cs = (|PT| + |PS|) / |PT + PS|, rcp R u, product u; fmaf(-q, PB, V): PB u, result u |V| <= u (|V_vac| + |T_e log w| + |t3|):
        bound_V = u [ 2 |V_vac| + (2 + L) |T_e log w| + |T_e| (1 + (3 + R) |z / w|) + (cs + R + 4) |t3| ]
      (coefficients of |V_vac|, |T_e log w|, |T_e|, |t3|: 2, 2 + L, 1 [+ (3 + R) |z / w| <= 4 + R], cs + R + 4).  clamp() is 1-Lipschitz, so the clamped value is
      held to [clamp(V - bound_V), clamp(V + bound_V)] with V the UNCLAMPED fp64 value: a sample whose reference lies within the bound
      of 0 or V_a may land on the clamp or off it, and is compared against that interval -- never skipped.

    cos_div = num / den.  Errors of the beam widths: a1 = fmaf(c2, PB, c3): e1 = u (1 + |c2 PB| / |a1|) (also covers the clip at
      float(pi/2), 0.47 u from pi/2); a2 = a1 * rcp(c1): e2 = e1 + (R + 1) u.
      TABLE PATH (`plain`):  num, den = X1 Q(a1) + X2 Q(a2),  X = base A,  A1 = (1 - c0) / D(a1),  A2 = c0 / D(a2).
        D and Q evaluated AS THE KERNEL DOES from a float a (a * a, rcp, the interval index, the Horner scheme; intrinsics correctly
        rounded) differ from the truth by at most TABLE_D_ERR, TABLE_QD_ERR, TABLE_QN_ERR relative: module constants MEASURED against
        the oracle's normaliser and the literal 91-term sums over every interval by tests/test_fp32_host.py, which asserts them.  On top:
        the hardware rcp behind u = 1 / a^2 (R u, times |dlog f / dlog u| = kappa / 2) and the error of a itself times kappa:
          e_D(a) = TABLE_D_ERR + 2 e_a + R u            (kappa_D = dlog D / dlog a lies in [0, 2]: D -> pi a^2 for small a, 2 pi for large a)
          e_Q(a) = TABLE_Q_ERR + kappa_Q (e_a + R u / 2), kappa_Q(a) = sum_k c_k g_k 2 t_k^2 / sum_k c_k g_k  (t_k = alpha_k / a,
                   g_k = exp(-t_k^2); from the fp64 weights, not from the kernel)
        `base` is common to X1 and X2 and cancels in the ratio, so e_X1 = e_D(a1) + (R + 3) u  (1 - c0, rcp, two products) and
        e_X2 = e_D(a2) + (R + 2) u.  den = fmaf(X1, Qd1, X2 * Qd2):
          e_den = [ |X1 Qd1| (e_X1 + e_Qd1) + |X2 Qd2| (e_X2 + e_Qd2 + u) ] / |den| + u      (cancellation, and nothing else, widens it)
        e_num alike, and cos_div = num * rcp(den):   e_cos = e_den + e_num + (R + 1) u, all over (1 - e_den) for the
        quotient; e_den >= 1/2 means den is within twice its bound of 0: the threshold rule `den against 0` below, and an infinite bound.
      LITERAL PATH (not `plain`): f_k = fmaf(X1, E1k, X2 * E2k), E = __expf(-(t * t)), t = alpha_k * rcp(a); den = sum_k w_k f_k as 91 fmaf.
        t: grid angle 2.5 u (float(pi/2) / 90 rounded, times k rounded) + e_a + (R + 1) u = e_t;  t^2: 2 e_t + u, which is an ABSOLUTE
        error of the exponent: the term moves by t^2 (2 e_t + u) relative, plus X(t^2) u of __expf itself, plus FLT_MIN absolute where
        it underflows.  Then the weight's rounding u, the inner product's u and gamma_91 = 91 u on the absolute sum:
          |den - den_ref| <= sum_k |w_k| [ |X1| g1k (e_X1 + eps1k) + |X2| g2k (e_X2 + eps2k + u) + (|X1| + |X2|) FLT_MIN ] + 93 u sum_k |w_k f_k|
      A sample within a few floats of a term of the `plain` predicate may take either path: it gets the larger of the two bounds.

    T = mdot sqrt(2 q/m (V_a - V)): with x = V_a - V_cc >= 0 and d = bound_V + u x, the square root is monotone, so
        bound_T = |mdot| sqrt(2 q/m) (sqrt(x + d) - sqrt(max(x - d, 0))) + (S + 4) u |T|
      -- near the clamp V_cc = V_a this GROWS to sqrt(d) instead of dividing by zero; the sample is compared, not dropped.
    T_c = T cos_div:  bound_Tc = |cos_div| bound_T + (|T| + bound_T) |cos_div| e_cos + u |T_c|.
    div_angle = arccos(cos_div) is judged through cos_div as parity_rules.divergence_error does: |cos(got) - cos(want)|, evaluated as
      2 |sin((g + w) / 2) sin((g - w) / 2)|, must be <= |cos_div| e_cos + |sin w| da + da^2 / 2 with da = A u |w| + 2^-149 (acosf's own
      error), so the pole needs no tolerance of its own.

    FLAGS AND NaN PATTERN are the oracle's, except where the reference value of the deciding quantity lies within its own bound of the
    threshold (`excused`): a1 against 0 (invalid; fmaf(c2, PB, c3) keeps the sign of the exact sum, so only PB's rounding u |c2 PB| counts),
    the profile against 0 (invalid), decided TERM BY TERM: with j_k = X1 g1k + X2 g2k + j_cex and b_k the literal path's term bound with
    the FULL error of X (base included) and of j_cex, a sample is certainly invalid if some j_k + b_k < 0 or some j_k is exactly 0 from
    exact zeros, certainly valid if every j_k - b_k > 0, and excused only otherwise; |a1|, |a2| against 53.28349511409265,
    den against 0, |cos_div| against 1 (arccos: NaN or not), and -- the fp32 counterpart of parity_rules' denormal rule -- a beam
    amplitude whose reference is below RANGE_FLOOR = 2^-120 (64 FLT_MIN) in magnitude without being zero or above 2^120, or a decay
    exponent above +80 (float's exp ends at 88.7): there the float amplitudes are denormal, flushed or infinite and num / den is noise or 0 / 0.
    Above that floor the literal path's bound carries FLT_MIN per term for the products and exponentials that underflow.
    NOT excused: a decay exponent below -88.5.  Float's exp has then underflowed for certain (it flushes below 2^-126, at -87.34), both
    amplitudes are zeros or NaN, and the float model's answer is defined: cos_div = 0 / 0, so div_angle and T_c are NaN, and the flag is
    a1 <= 0 or mdot_a <= 0 (a1 <= 0 alone where a2 is beyond the overflow bound).  `check` holds such samples to that answer.
    Where something is excused, `check(..., res=restatement)` still requires the restatement's NaN pattern and flag.
    Over the wild set every excuse together stays under 2 % of the finite reference values (of the samples, for the flag):
    tests/test_fp32_host.py and tests/test_fp32_kernels.py assert it.
    A reference value that is finite while its bound is not finite FAILS the check.
"""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / 'hallthrusterpem_amd' / 'csrc'
f32, f64 = np.float32, np.float64
U32 = 2.0 ** -24
SECOND = 1.01
FLT_MIN = 2.0 ** -126
RANGE_FLOOR = 2.0 ** -120
ALPHA_OVERFLOW = 53.28349511409265
COUPLED_INPUTS = ('P_b', 'V_a', 'T_e', 'V_vac', 'Pstar', 'P_T', 'mdot_a', 'a_1', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')

# Worst errors in float ulps over EVERY finite float of the domain, normal arguments and results, each rounded up to the next half ulp:
# profiles/fp32_intrinsics_r01.txt (tools/microbench/f32_intrinsics.hip on an MI355X).
RCP_ULPS = 1.0            # measured 0.8818 (v_rcp_f32)
SQRT_ULPS = 1.0           # measured 0.9236 (v_sqrt_f32)
LOG_ULPS = 2.5            # measured 2.3315 (__logf)
ACOS_ULPS = 1.5           # measured 1.4636 (acosf; 1.3153 for negative arguments)
# __expf(x) per binade of |x|: < 1, [1, 2), [2, 4), [4, 8), [8, 16), [16, 32), [32, 64), >= 64; the larger of the two signs
# (measured 1.4654 2.3460 4.0822 7.7459 15.1288 29.7212 58.7188 64.2151)
EXP_ULPS = np.array([1.5, 2.5, 4.5, 8.0, 15.5, 30.0, 59.0, 64.5])

# Worst relative error of the tables evaluated as the kernel does from a float a (restated intrinsics), against the oracle's normaliser
# and the literal 91-term Simpson sums in fp64, over every interval: measured and asserted by tests/test_fp32_host.py, in units of U32
# rounded up to the next ulp (2 U32).
TABLE_D_ERR = 4.0 * U32           # measured 3.17 (the series; the table 2.72)
TABLE_QD_ERR = 4.0 * U32          # measured 3.61 (narrow interval 17; wide 2.86)
TABLE_QN_ERR = 4.0 * U32          # measured 3.26 (narrow interval 10; wide 2.69)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------------------
def _parse(name, text, strip_f=False):
    body = re.search(r'%s\[\d+\] = \{(.*?)\};' % name, text, re.S).group(1)
    body = re.sub(r'//[^\n]*', '', body)
    return np.array([float.fromhex(tok) for tok in re.findall(r'-?0x[0-9a-fA-F.]+p[-+]?\d+', body)])


_tables32 = None
_tables64 = None


def tables32(path=None):
    """csrc/pem_tables_f32.h as float32 arrays (every literal must be a float exactly)."""
    global _tables32
    if _tables32 is not None and path is None:
        return _tables32
    text = Path(path or CSRC / 'pem_tables_f32.h').read_text()
    d = {k: int(re.search(r'#define PEM32_%s (\d+)' % k, text).group(1)) for k in ('NDC', 'NDI', 'NQB', 'NDAW')}
    out = dict(d)
    for k in ('QA_MIN', 'QB_SCALE'):
        v = float.fromhex(re.search(r'#define PEM32_%s (\S+?)f\s' % k, text).group(1))
        assert float(f32(v)) == v
        out[k] = f32(v)
    for name, shape in (('SIMPSON', (91, 2)), ('DAWSON', (d['NDAW'],)), ('DPOLY', (d['NDI'], d['NDC'])), ('QPOLY', (d['NDI'] + d['NQB'], d['NDC'], 2))):
        v = _parse('PEM32_' + name, text)
        assert v.size == int(np.prod(shape)), (name, v.size)
        assert np.array_equal(v.astype(f32).astype(f64), v), f'{name}: a literal is not a float'
        out[name] = v.astype(f32).reshape(shape)
    if path is None:
        _tables32 = out
    return out


def tables64():
    """The fp64 Simpson weights of csrc/pem_tables.h (pinned through the oracle by the fp64 kernels' tests)."""
    global _tables64
    if _tables64 is None:
        text = (CSRC / 'pem_tables.h').read_text()
        _tables64 = {'CDEN': _parse('PEM_SIMPSON_CDEN', text), 'CNUM': _parse('PEM_SIMPSON_CNUM', text)}
        assert _tables64['CDEN'].size == 91 and _tables64['CNUM'].size == 91
    return _tables64


def angle_grid64():
    a = np.arange(91) * ((np.pi / 2) / 90.0)
    a[-1] = np.pi / 2
    return a


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def _flush(x):
    x = np.asarray(x, f32)
    return np.where(np.abs(x) < f32(FLT_MIN), np.copysign(f32(0), x), x).astype(f32)


def rcp(x):
    with np.errstate(all='ignore'):
        return _flush((1.0 / _flush(x).astype(f64)).astype(f32))


def sqrt32(x):
    with np.errstate(all='ignore'):
        return np.sqrt(_flush(x).astype(f64)).astype(f32)


def exp32(x):
    with np.errstate(all='ignore'):
        return _flush(np.exp(np.asarray(x, f32).astype(f64)).astype(f32))


def log32(x):
    with np.errstate(all='ignore'):
        return np.log(np.asarray(x, f32).astype(f64)).astype(f32)


def acos32(x):
    with np.errstate(all='ignore'):
        return np.arccos(np.asarray(x, f32).astype(f64)).astype(f32)


def to_int(t):
    """(int)t as v_cvt_i32_f32 does it: truncation, NaN -> 0, saturating"""
    t = np.asarray(t, f32).astype(f64)
    return np.trunc(np.clip(np.nan_to_num(t, nan=0.0, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


F_PI = f32(3.14159265358979323846)
F_HALF_PI = f32(1.57079632679489661923)
F_GRID_H = f32(F_HALF_PI / f32(90.0))
F_ALPHA_OVERFLOW = f32(ALPHA_OVERFLOW)
Q_OVER_M = f32(1.6e-19 / 2.18e-25)


def _horner(rows, x):
    """rows (n, ncoef) float32, x (n,): fmaf Horner from the highest coefficient down"""
    acc = rows[:, -1]
    for j in range(rows.shape[1] - 2, -1, -1):
        acc = fma(acc, x, rows[:, j])
    return acc


def normaliser32(a, u, tab=None):
    tab = tab or tables32()
    a, u = np.asarray(a, f32), np.asarray(u, f32)
    with np.errstate(all='ignore'):
        i = np.clip(to_int(f32(2.0) * u), 0, tab['NDI'] - 1)
        x = fma(f32(4.0), u, -(2 * i + 1).astype(f32))
        d = _horner(tab['DPOLY'][i], x)
        a2 = a * a
        y = f32(0.5) * a2
        s = np.full(a.shape, tab['DAWSON'][-1], f32)
        for j in range(tab['NDAW'] - 2, -1, -1):
            s = fma(s, y, tab['DAWSON'][j])
        D = np.where(np.abs(a) < f32(0.25), (F_PI * a2) * s, d).astype(f32)
        bad = ~(np.abs(a) < F_ALPHA_OVERFLOW) | (a == 0)
    return np.where(bad, f32(np.nan), D).astype(f32)


def functionals32(aa, u, tab=None):
    """(Qd, Qn) float32 for aa = |a|, u = rcp(a * a)"""
    tab = tab or tables32()
    aa, u = np.asarray(aa, f32), np.asarray(u, f32)
    with np.errstate(all='ignore'):
        wide = aa >= f32(0.25)
        t = np.where(wide, f32(2.0) * u, (aa - tab['QA_MIN']) * tab['QB_SCALE']).astype(f32)
        last = np.where(wide, tab['NDI'] - 1, tab['NQB'] - 1)
        i = np.maximum(np.minimum(to_int(t), last), 0)
        x = (f32(2.0) * (t - i.astype(f32)) - f32(1.0)).astype(f32)
        rows = tab['QPOLY'][np.where(wide, 0, tab['NDI']) + i]            # (n, NDC, 2)
        return _horner(rows[:, :, 0], x), _horner(rows[:, :, 1], x)


def as_f32_inputs(x):
    """dict or (15, n) array -> (15, n) float32, rounded to nearest"""
    if isinstance(x, dict):
        x = np.stack([np.asarray(x[k], f64) for k in COUPLED_INPUTS])
    with np.errstate(over='ignore'):
        return np.ascontiguousarray(np.asarray(x).astype(f32))


def restate(x32, k, radius=1.0, tab=None):
    """coupled_f32 on (15, n) float32 inputs; k = torr2pa, radius: the entry point's float arguments."""
    tab = tab or tables32()
    x32 = np.asarray(x32, f32)
    P_b, V_a, T_e, V_vac, Pstar, P_T, mdot, a_1, c0, c1, c2, c3, c4, c5, sigma = x32
    k, rad = f32(k), f32(radius)
    with np.errstate(all='ignore'):
        inv_r2 = f32(1.0) / (rad * rad)
        inv_2pi_r2 = f32(1.0) / ((f32(2.0) * F_PI) * (rad * rad))
        PB, PS, PT = P_b * k, Pstar * k, P_T * k
        V = fma(T_e, log32(f32(1.0) + PB * rcp(PT)), V_vac)
        V = fma(-(T_e * rcp(PT + PS)), PB, V)
        V = np.where(V < 0, f32(0), V)
        V = np.where(V > V_a, V_a, V).astype(f32)
        I_B0 = Q_OVER_M * mdot
        T = mdot * sqrt32((f32(2.0) * Q_OVER_M) * (V_a - V))
        n_neutral = fma(c4, PB, c5)
        a1 = fma(c2, PB, c3)
        a1 = np.where(a1 > F_HALF_PI, F_HALF_PI, a1).astype(f32)
        a2 = a1 * rcp(c1)
        u1, u2 = rcp(a1 * a1), rcp(a2 * a2)
        A1 = (f32(1.0) - c0) * rcp(normaliser32(a1, u1, tab))
        A2 = c0 * rcp(normaliser32(a2, u2, tab))
        decay = exp32(-rad * n_neutral * sigma)
        j_cex = I_B0 * (f32(1.0) - decay) * inv_2pi_r2
        base = I_B0 * decay * inv_r2
        X1, X2 = base * A1, base * A2
        aa1, aa2 = np.abs(a1), np.abs(a2)
        plain = ((aa1 >= tab['QA_MIN']) & (aa2 >= tab['QA_MIN']) & (X1 >= 0) & (X2 >= 0) & (j_cex > 0)
                 & ((np.fmax(X1, X2) >= f32(1e-30)) | ((X1 == 0) & (X2 == 0))))
        invalid = a1 <= 0
        q1d, q1n = functionals32(aa1, u1, tab)
        q2d, q2n = functionals32(aa2, u2, tab)
        den = fma(X1, q1d, X2 * q2d)
        num = fma(X1, q1n, X2 * q2n)
        lit = np.flatnonzero(~plain)
        if lit.size:
            d = np.zeros(lit.size, f32)
            nn = np.zeros(lit.size, f32)
            lo = np.full(lit.size, np.inf, f32)
            r1, r2 = rcp(a1[lit]), rcp(a2[lit])
            for kk in range(91):
                alpha = F_HALF_PI if kk == 90 else f32(kk) * F_GRID_H
                t1, t2 = alpha * r1, alpha * r2
                f = fma(X1[lit], exp32(-(t1 * t1)), X2[lit] * exp32(-(t2 * t2)))
                lo = np.fmin(lo, f + j_cex[lit])
                d = fma(tab['SIMPSON'][kk, 0], f, d)
                nn = fma(tab['SIMPSON'][kk, 1], f, nn)
            den, num = den.copy(), num.copy()
            den[lit], num[lit] = d, nn
            invalid = invalid.copy()
            invalid[lit] |= lo <= 0
        cos_div = num * rcp(den)
        cos_div = np.where(cos_div == np.inf, f32(np.nan), cos_div).astype(f32)
        div = acos32(cos_div)
        T_c = T * cos_div
    return {'V_cc': V, 'div_angle': div, 'T_c': T_c, 'invalid': invalid, 'plain': plain, 'a1': a1, 'a2': a2, 'X1': X1, 'X2': X2, 'den': den,
            'num': num, 'cos_div': cos_div, 'T': T, 'I_B0': I_B0, 'j_cex': j_cex, 'decay': decay, 'u1': u1, 'u2': u2}


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the reference and the bound
# ---------------------------------------------------------------------------------------------------------------------------------
def reference(x32, k, radius=1.0, threads=16):
    """The oracle on the float inputs widened to double (k: the float torr2pa widened), plus the fp64 term sizes the bound needs."""
    from oracle import oracle_ctypes as oc
    oc.set_threads(threads)
    xd = {n: np.ascontiguousarray(np.asarray(x32[i], f32).astype(f64)) for i, n in enumerate(COUPLED_INPUTS)}
    kd, rad = float(f32(k)), float(f32(radius))
    with np.errstate(all='ignore'):
        want = oc.coupled(xd, kd, rad)
        terms = oc.plume_terms(*[xd[q] for q in ('P_b', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')], want['I_B0'], kd, radii=(rad,))
        ref = {'x': xd, 'k': kd, 'radius': rad, 'V_cc': want['V_cc'], 'div_angle': want['div_angle'], 'T_c': want['T_c'], 'T': want['T'],
               'I_B0': want['I_B0'], 'invalid': want['invalid']}
        for q in ('X1', 'X2', 'j_cex', 'decay', 'den', 'num'):
            ref[q] = terms[q][:, 0]
        ref['a1'], ref['a2'] = terms['a1'], terms['a2']
        ref['cos_div'] = ref['num'] / np.where(ref['den'] == 0, np.nan, ref['den'])
        PB, PT, PS = xd['P_b'] * kd, xd['P_T'] * kd, xd['Pstar'] * kd
        z = PB / PT
        w = 1.0 + z
        lg = np.log(w)
        t3 = (xd['T_e'] / (PT + PS)) * PB
        ref.update(V_un=(xd['V_vac'] + xd['T_e'] * lg) - t3, z=z, w=w, Tlg=xd['T_e'] * lg, t3=t3, cs=np.where(np.isinf(PT + PS), 1.0, (np.abs(PT) + np.abs(PS)) / np.abs(PT + PS)),
                   c2PB=xd['c2'] * PB, arg=-rad * (xd['c4'] * PB + xd['c5']) * xd['sigma_cex'])
    return ref


def _exp_ulps(t):
    """the measured __expf figure for the binade of |t| (a margin of 1e-3 of |t| decides the binade upwards)"""
    with np.errstate(all='ignore'):
        e = np.floor(np.log2(np.maximum(np.abs(t) * 1.001, 0.5))).astype(np.int64) + 1
    return EXP_ULPS[np.clip(e, 0, len(EXP_ULPS) - 1)]


def _term_sums(ref, idx, e_a1, e_a2, e_X1, e_X2, b_jcex=None):
    """Literal-path bounds for the samples idx: absolute bounds of den and num; and, with b_jcex given (then the X errors e_X* include
    base), whether the sign of the profile minimum is UNDECIDED: term by term, j_k = X1 g1k + X2 g2k + j_cex with its own bound b_k; the
    sample is certainly invalid if some j_k + b_k < 0, certainly valid if every j_k - b_k > 0, undecided otherwise."""
    R = 2.0 * RCP_ULPS
    t64 = tables64()
    al = angle_grid64()[None, :]
    with np.errstate(all='ignore'):
        a1, a2 = ref['a1'][idx, None], ref['a2'][idx, None]
        X1, X2 = np.abs(ref['X1'][idx, None]), np.abs(ref['X2'][idx, None])
        out = []
        per = []
        for name, a, X, e_a, e_X, extra in (('X1', a1, X1, e_a1[idx, None], e_X1[idx, None], 0.0), ('X2', a2, X2, e_a2[idx, None], e_X2[idx, None], U32)):
            tt = (al / a) ** 2
            g = np.exp(-tt)
            e_t = 2.5 * U32 + e_a + (R + 1.0) * U32
            eps = tt * (2.0 * e_t + U32) + 2.0 * _exp_ulps(tt) * U32
            eps = np.where(g == 0.0, 0.0, eps)                      # a term that is zero in fp64 is zero (or below FLT_MIN) in float
            per.append((X * g, X * g * (e_X + eps + extra) + (X + 1.0) * FLT_MIN, np.where(X == 0.0, 0.0, ref[name][idx, None] * g)))
        absf = per[0][0] + per[1][0]
        errf = per[0][1] + per[1][1]
        jk = per[0][2] + per[1][2] + ref['j_cex'][idx, None]
        jmin = np.min(jk, axis=1)
        undecided = None
        if b_jcex is not None:
            bk = SECOND * (errf + U32 * absf) + b_jcex[idx, None]
            # a term that is exactly 0 in fp64 (an amplitude that is exactly 0, or a tail that underflows there) with j_cex exactly 0 is
            # exactly 0 in float as well, where tails underflow sooner and the zero sources (c0, 1 - c0, mdot, sigma, decay = 1) are exact
            exact_zero = np.any((per[0][2] == 0.0) & (per[1][2] == 0.0), axis=1) & (ref['j_cex'][idx] == 0.0)
            sure_invalid = np.any(jk + bk < 0.0, axis=1) | exact_zero
            sure_valid = np.all((jk - bk > 0.0) | np.isnan(jk), axis=1)
            undecided = ~(sure_invalid | sure_valid)
        for c in (t64['CDEN'], t64['CNUM']):
            out.append(np.sum(np.abs(c)[None, :] * (errf + 93.0 * U32 * absf), axis=1))
    return out[0], out[1], undecided, jmin


def kappa_q(a):
    """(kappa_Qd, kappa_Qn, Qd, Qn): d log Q / d log a and Q itself from the literal sums with the fp64 weights"""
    t64 = tables64()
    with np.errstate(all='ignore'):
        tt = (angle_grid64()[None, :] / np.asarray(a, f64)[:, None]) ** 2
        g = np.exp(-tt)
        qd, qn = g @ t64['CDEN'], g @ t64['CNUM']
        kd, kn = (g * 2.0 * tt) @ t64['CDEN'] / qd, (g * 2.0 * tt) @ t64['CNUM'] / qn
    return kd, kn, qd, qn


def bounds(ref, res, chunk=50_000, table_err=True):
    """Per-sample bounds from the reference `ref`; `res` (the restatement) only says which path a sample took.  Returns dict of
    V_lo, V_hi (the clamped interval), bound_V, e_cos (relative), bound_Tc, bound_T, and the `excused` masks."""
    R, S, L = 2.0 * RCP_ULPS, 2.0 * SQRT_ULPS, 2.0 * LOG_ULPS
    tD, tQd, tQn = (TABLE_D_ERR, TABLE_QD_ERR, TABLE_QN_ERR) if table_err else (0.0, 0.0, 0.0)    # (False: kernel against restatement, same tables)
    x = ref['x']
    n = len(ref['V_cc'])
    u = U32
    tab = tables32()
    with np.errstate(all='ignore'):
        zw = np.where(ref['z'] == 0.0, 0.0, np.abs(ref['z'] / ref['w']))          # (an infinite pressure makes a term exactly zero, in any arithmetic)
        bV = SECOND * u * (2.0 * np.abs(x['V_vac']) + (2.0 + L) * np.abs(ref['Tlg']) + np.abs(x['T_e']) * (1.0 + (3.0 + R) * zw)
                           + np.where(ref['t3'] == 0.0, 0.0, (ref['cs'] + R + 4.0) * np.abs(ref['t3'])))
        Vun = ref['V_un']
        bV = np.where(np.isinf(Vun), 0.0, bV)          # an infinite V is clamped to 0 or V_a exactly, in any arithmetic

        def clamp(v):
            v = np.where(v < 0.0, 0.0, v)
            return np.where(v > x['V_a'], x['V_a'], v)
        V_lo, V_hi = clamp(Vun - bV), clamp(Vun + bV)
        # thrust
        xx = x['V_a'] - ref['V_cc']
        d = bV + u * np.abs(xx)
        c = 2.0 * (1.6e-19 / 2.18e-25)
        bT = SECOND * (np.abs(x['mdot_a']) * np.sqrt(c) * (np.sqrt(xx + d) - np.sqrt(np.maximum(xx - d, 0.0))) + (S + 4.0) * u * np.abs(ref['T']))
        # beam widths
        a1, a2 = ref['a1'], ref['a2']
        e_a1 = u * (1.0 + np.abs(ref['c2PB']) / np.abs(a1))
        e_a2 = e_a1 + (R + 1.0) * u
        e_D1 = tD + 2.0 * e_a1 + R * u
        e_D2 = tD + 2.0 * e_a2 + R * u
        e_X1 = e_D1 + (R + 3.0) * u
        e_X2 = e_D2 + (R + 2.0) * u
        # full error of X = base A (for the profile minimum): I_B0 u, decay = __expf(arg): arg's three roundings (PB, fma, two products: 4 u) as an
        # absolute error of the exponent, __expf's own, two more products
        arg = ref['arg']
        e_base = u * (1.0 + 4.0 * np.abs(arg) + 2.0 * _exp_ulps(arg) + 2.0)
        unit = np.abs(ref['I_B0']) / (2.0 * np.pi * ref['radius'] ** 2)
        # j_cex = I_B0 (1 - decay) / (2 pi r^2): decay's absolute error is the exponent's (4 u |arg|) plus __expf's measured ulps of decay's
        # own binade (half as large just below 1 as above it); 1 - decay is then exact or rounded once, and five roundings follow
        dec = np.abs(ref['decay'])
        ulp_dec = 2.0 ** (np.floor(np.log2(np.where(dec > 0.0, dec, 1.0))) - 23.0)
        b_jcex = SECOND * (unit * (dec * 4.0 * u * np.abs(arg) + _exp_ulps(arg) * ulp_dec) + 5.0 * u * np.abs(ref['j_cex']))
        # which path
        near = np.zeros(n, bool)
        qa = float(tab['QA_MIN'])
        for a, e in ((a1, e_a1), (a2, e_a2)):
            near |= np.abs(np.abs(a) - qa) <= 4.0 * e * qa
        near |= (np.abs(ref['X1']) <= 2e-30) | (np.abs(ref['X2']) <= 2e-30) | (np.abs(ref['j_cex']) <= b_jcex)
        plain = np.asarray(res['plain'], bool)
        # table path
        e_tab = np.full(n, np.inf)
        for s in range(0, n, chunk):
            sl = slice(s, min(n, s + chunk))
            k1d, k1n, q1d, q1n = kappa_q(a1[sl])
            k2d, k2n, q2d, q2n = kappa_q(a2[sl])
            X1, X2 = ref['X1'][sl], ref['X2'][sl]
            parts = []
            for kq1, kq2, Q1, Q2, E, tot in ((k1d, k2d, q1d, q2d, tQd, ref['den'][sl]), (k1n, k2n, q1n, q2n, tQn, ref['num'][sl])):
                eq1 = E + kq1 * (e_a1[sl] + 0.5 * R * u)
                eq2 = E + kq2 * (e_a2[sl] + 0.5 * R * u)
                parts.append((np.abs(X1 * Q1) * (e_X1[sl] + eq1) + np.abs(X2 * Q2) * (e_X2[sl] + eq2 + u)) / np.abs(tot) + u)
            e_tab[sl] = np.where(parts[0] < 0.5, SECOND * (parts[0] + parts[1] + (R + 1.0) * u) / (1.0 - parts[0]), np.inf)
        e_tab = np.where(np.isfinite(e_tab), e_tab, np.inf)
        # literal path (and the profile minimum of every sample that is not plain)
        e_lit = np.full(n, np.nan)
        j_und = np.zeros(n, bool)
        j_min = np.full(n, np.inf)
        for idx in np.array_split(np.flatnonzero(~plain | near), max(1, int((~plain | near).sum()) // 20_000 + 1)):
            if not idx.size:
                continue
            bd, bn, _, jmin = _term_sums(ref, idx, e_a1, e_a2, e_X1, e_X2)
            e_den = bd / np.abs(ref['den'][idx])
            e = SECOND * (e_den + bn / np.abs(ref['num'][idx]) + (R + 1.0) * u) / (1.0 - e_den)
            e_lit[idx] = np.where(np.isfinite(e) & (e_den < 0.5), e, np.inf)
            _, _, und, _ = _term_sums(ref, idx, e_a1, e_a2, e_X1 + e_base, e_X2 + e_base, b_jcex)
            j_und[idx] = und
            j_min[idx] = jmin
        e_cos = np.where(plain & ~near, e_tab, np.where(~plain & ~near, e_lit, np.fmax(e_tab, e_lit)))
        cosr = ref['cos_div']
        bTc = SECOND * (np.abs(cosr) * bT + (np.abs(ref['T']) + bT) * np.abs(cosr) * e_cos + u * np.abs(ref['T_c']))
        # thresholds
        amp = np.fmax(np.abs(ref['X1']), np.abs(ref['X2']))
        # fmaf(c2, PB, c3) is the exact c2 PB + c3 rounded once, which keeps its sign: only PB's own rounding can move a1 across 0
        b_a1 = SECOND * u * np.abs(ref['c2PB'])
        exc = {
            'range': ((amp < RANGE_FLOOR) & (amp > 0.0)) | (arg > 80.0) | (amp > 1.0 / RANGE_FLOOR),
            'a1_zero': (np.abs(ref['c2PB'] + x['c3']) <= b_a1) & (b_a1 > 0.0) & np.isfinite(b_a1),      # (a1 before the clip at pi/2)
            'overflow': (np.isfinite(e_a1) & (np.abs(np.abs(a1) - ALPHA_OVERFLOW) <= 4.0 * e_a1 * ALPHA_OVERFLOW))
                        | (np.isfinite(e_a2) & (np.abs(np.abs(a2) - ALPHA_OVERFLOW) <= 4.0 * e_a2 * ALPHA_OVERFLOW)),
            'den_zero': np.isfinite(ref['den']) & np.isfinite(ref['num']) & ~np.isfinite(e_cos),
            'j_min': j_und,
            'pole': np.abs(np.abs(cosr) - 1.0) <= np.abs(cosr) * e_cos,
        }
    return {'V_lo': V_lo, 'V_hi': V_hi, 'bound_V': bV, 'bound_T': bT, 'e_cos': e_cos, 'bound_Tc': bTc, 'near': near, 'excused': exc, 'jcex_border': np.abs(ref['j_cex']) <= b_jcex}


QOI = ('V_cc', 'T_c', 'cos_div')


def check(got, ref, bnd, res=None):
    """Hold `got` (V_cc, div_angle, T_c as float arrays, invalid) to the reference under the bound.  Returns a report:
    per QoI `compared`, `excused`, `finite` (reference values that are finite), `ratio` (largest error / bound) and `worst` (its sample),
    `failures`: list of (what, sample indices) -- empty when everything holds; and `rel_bound` (per-sample bound / |value|, for the medians)."""
    exc = bnd['excused']
    n = len(ref['V_cc'])
    fails = []
    rep = {'n': n, 'failures': fails, 'rel_bound': {}}

    def fail(what, mask):
        if np.any(mask):
            fails.append((what, np.flatnonzero(mask)[:8].tolist()))

    def stats(name, fin, excused, err, bound):
        cmp_ = fin & ~excused
        fail(f'{name}: reference finite, bound not finite', cmp_ & ~np.isfinite(bound))
        with np.errstate(all='ignore'):
            ratio = np.where(cmp_, np.where(err == 0.0, 0.0, err / bound), 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        fail(f'{name}: outside the bound', ratio > 1.0)
        rep[name] = {'compared': int(cmp_.sum()), 'excused': int((fin & excused).sum()), 'finite': int(fin.sum()),
                     'ratio': float(np.max(ratio, initial=0.0)), 'worst': int(np.argmax(ratio)) if n else -1}

    with np.errstate(all='ignore'):
        # V_cc: the clamped interval; nothing is excused except values past float's range
        g, w = np.asarray(got['V_cc'], f64), ref['V_cc']
        big = bnd['bound_V'] / U32 > 2.0 ** 100
        fin = np.isfinite(w)
        stats('V_cc', fin, big, np.abs(g - w), bnd['bound_V'])
        inside = (g >= bnd['V_lo']) & (g <= bnd['V_hi'])
        fail('V_cc: outside the clamped interval', fin & ~big & ~inside)
        fail('V_cc: NaN pattern', ~big & (np.isnan(g) != np.isnan(w)))
        rep['rel_bound']['V_cc'] = bnd['bound_V'] / np.abs(w)
        # cos_div through T_c and div_angle
        # Where the decay exponent is below -88.5 float's exp has underflowed for certain (it flushes below 2^-126, at -87.34): both
        # amplitudes are +-0 or NaN and the float model's answer is DEFINED -- cos_div = 0 / 0, so div_angle and T_c are NaN.  Such a
        # sample is held to that answer and is not excused.  With both beam widths finite, non-zero and inside the overflow bound the
        # amplitudes are exact zeros, the profile is j_cex = I_B0 / (2 pi r^2) at every angle, and the flag is a1 <= 0 or mdot_a <= 0.
        a1r, a2r = ref['a1'], ref['a2']
        flush = exc['range'] & (ref['arg'] < -88.5)
        clean = (np.isfinite(a1r) & np.isfinite(a2r) & (a2r != 0.0) & ~exc['a1_zero'] & (a1r != 0.0) & (np.abs(a1r) < 53.0) & (np.abs(a2r) < 53.0)
                 & np.isfinite(ref['x']['c0']))
        # ... and with a2 beyond the overflow bound (or infinite, or NaN) X2 is NaN at every angle, fminf ignores it: the flag is a1 <= 0
        beyond = (np.isfinite(a1r) & (a1r != 0.0) & ~exc['a1_zero'] & ~exc['overflow'] & np.isfinite(ref['x']['c0'])
                  & ((np.abs(a2r) > 54.0) | np.isnan(a2r)))
        flush_flag = flush & (clean | beyond)
        ex_cos = (exc['range'] & ~flush) | exc['overflow'] | exc['den_zero'] | exc['a1_zero']
        gt, wt = np.asarray(got['T_c'], f64), ref['T_c']
        fin_t = np.isfinite(wt)
        stats('T_c', fin_t & ~flush, ex_cos, np.abs(gt - wt), bnd['bound_Tc'])
        rep['T_c']['finite'] += int((fin_t & flush).sum())
        rep['T_c']['compared'] += int((fin_t & flush).sum())
        fail('T_c: NaN pattern', ~ex_cos & ~flush & (np.isnan(gt) != np.isnan(wt)))
        fail('T_c: not NaN where the decay has underflowed', flush & ~np.isnan(gt))
        rep['rel_bound']['T_c'] = bnd['bound_Tc'] / np.abs(wt)
        gd, wd = np.asarray(got['div_angle'], f64), ref['div_angle']
        cosr = ref['cos_div']
        da = 2.0 * ACOS_ULPS * U32 * np.abs(wd) + 2.0 ** -149
        allowed = SECOND * (np.abs(cosr) * bnd['e_cos'] + np.abs(np.sin(wd)) * da + 0.5 * da * da)
        err_cos = 2.0 * np.abs(np.sin(0.5 * (gd + wd)) * np.sin(0.5 * (gd - wd)))
        fin_d = np.isfinite(wd)
        # at the pole arccos is 0-or-NaN on either side: a NaN there is inside the bound when |cos_ref| is within it of 1
        at_pole = exc['pole']
        nan_ok = at_pole & np.isnan(gd)
        stats('cos_div', fin_d & ~flush, ex_cos | nan_ok, np.where(np.isnan(gd), np.inf, err_cos), allowed)
        rep['cos_div']['finite'] += int((fin_d & flush).sum())
        rep['cos_div']['compared'] += int((fin_d & flush).sum())
        fail('div_angle: NaN pattern', ~ex_cos & ~flush & ~at_pole & (np.isnan(gd) != np.isnan(wd)))
        fail('div_angle: not NaN where the decay has underflowed', flush & ~np.isnan(gd))
        rep['rel_bound']['cos_div'] = bnd['e_cos']
        rep['cos_div']['excused'] = int((fin_d & ~flush & (ex_cos | at_pole)).sum())
        # flags
        ex_flag = (exc['range'] & ~flush_flag) | exc['a1_zero'] | exc['j_min'] | exc['overflow']
        gi = np.asarray(got['invalid'], bool)
        fail('invalid flag', ~ex_flag & ~flush_flag & (gi != ref['invalid']))
        fail('invalid flag where the decay has underflowed', flush_flag & (gi != ((a1r <= 0.0) | (clean & (ref['x']['mdot_a'] <= 0.0)))))
        rep['flags'] = {'compared': int((~ex_flag).sum()), 'excused': int(ex_flag.sum())}
        rep['ex_cos'], rep['ex_flag'] = ex_cos, ex_flag
        if res is not None:
            # what the oracle cannot decide the restatement does: same NaN pattern and the same flag there
            fail('T_c: NaN pattern against the restatement where excused', ex_cos & (np.isnan(gt) != np.isnan(res['T_c'])))
            fail('div_angle: NaN pattern against the restatement where excused', ex_cos & ~at_pole & (np.isnan(gd) != np.isnan(res['div_angle'])))
            # (except where j_cex = I_B0 (1 - decay) / (2 pi r^2) is within its own bound of 0: there 1 - decay is a few ulps of __expf's
            # result, which the restatement rounds correctly and the hardware does not)
            fail('invalid flag against the restatement where excused', ex_flag & ~bnd['jcex_border'] & (gi != np.asarray(res['invalid'], bool)))
    return rep


def summary(rep, what, inside_priors=False):
    lines = [f'{what}: {rep["n"]} samples']
    for q in QOI:
        r = rep[q]
        rb = rep['rel_bound'][q]
        with np.errstate(all='ignore'):
            med = float(np.nanmedian(np.where(np.isfinite(rb), rb, np.nan))) if np.isfinite(rb).any() else float('nan')
        lines.append(f'  {q:8s} compared {r["compared"]:8d}  excused {r["excused"]:6d} of {r["finite"]:8d} finite ({100.0 * r["excused"] / max(r["finite"], 1):.2f} %)'
                     f'  worst error/bound {r["ratio"]:.3f} (sample {r["worst"]})  median bound/|value| {med:.2e}')
        r['median_rel_bound'] = med
    lines.append(f'  flags    compared {rep["flags"]["compared"]:8d}  excused {rep["flags"]["excused"]:6d}')
    return '\n'.join(lines)


# ---------------------------------------------------------------------------------------------------------------------------------
# the input sets of tests/test_fp32_host.py and tests/test_fp32_kernels.py
# ---------------------------------------------------------------------------------------------------------------------------------
PRIOR_SEEDS = (2, 11, 29)
WILD_SEEDS = (0, 1, 2, 3, 65, 867, 940, 1100, 5160)          # the seeds tests/test_saltelli_model.py lists


def prior_set(seed, n):
    """n samples of the PEM-v0 prior design (oracle/sampler_np: the numbers the device design holds), rounded to float: (15, n)"""
    from hallthrusterpem_amd import sampling
    from oracle import sampler_np
    d = sampling.Design(seed=seed)
    return as_f32_inputs(sampler_np.sample(n, 0, d.seed, d.stream, d.kind, d.a, d.b))


def wild_set(seed, n=20_000):
    import sys
    tools = str(ROOT / 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from fuzz_parity import wild
    return as_f32_inputs(wild(np.random.default_rng(1000 + seed), n))


SEMANTICS_BASE = {'P_b': 1e-5, 'V_a': 300.0, 'T_e': 3.0, 'V_vac': 30.0, 'Pstar': 2e-5, 'P_T': 5e-5, 'mdot_a': 5e-6, 'a_1': 0.01,
                  'c0': 0.5, 'c1': 0.5, 'c2': -8.0, 'c3': 0.3, 'c4': 1e20, 'c5': 1e16, 'sigma_cex': 55e-20}
# the eleven points of tests/test_fp32.py::test_fp32_semantics_outside_the_plain_path
SEMANTICS_EDITS = [{}, {'c2': 0.0, 'c3': -0.3}, {'c0': 1.2}, {'c0': -0.1}, {'c2': 0.0, 'c3': 0.02}, {'c2': 0.0, 'c3': 0.1}, {'c3': float('nan')},
                   {'c2': 0.0, 'c3': 0.0}, {'mdot_a': -5e-6}, {'c2': 0.0, 'c3': 1.5, 'c1': 0.02}, {'V_vac': 0.0, 'T_e': 1.0}]


def neighbours(v, m=8):
    """the 2 m + 1 floats around v"""
    out = [np.float32(v)]
    lo = hi = np.float32(v)
    for _ in range(m):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.array(out, dtype=np.float32)


def table_points(n_random=300):
    """float widths a > 0 covering every interval of the three layouts: per interval both ends (the floats around each knot, where
    (int)t flips), the midpoint and 300 random points; the switches 0.25, QA_MIN, pi/2, the last interval's clamp, the series."""
    tab = tables32()
    rng = np.random.default_rng(5)
    pts = []
    for i in range(tab['NDI']):                                     # u = 1 / a^2 in [i / 2, (i + 1) / 2]
        ulo, uhi = max(i / 2.0, 1.0 / ALPHA_OVERFLOW ** 2), (i + 1) / 2.0
        uu = np.concatenate([rng.uniform(ulo, uhi, n_random), [0.5 * (ulo + uhi)]])
        pts.append((1.0 / np.sqrt(uu)).astype(np.float32))
        pts.append(neighbours(1.0 / np.sqrt(uhi)))
    pts.append(neighbours(ALPHA_OVERFLOW))                      # both sides of the bound: NaN above it, as the oracle has it
    pts.append(np.array([1.0, 2.0, 10.0, 50.0, 53.0], dtype=np.float32))
    qa, sc = float(tab['QA_MIN']), float(tab['QB_SCALE'])
    for j in range(tab['NQB']):                                     # |a| in QA_MIN + [j, j + 1] / QB_SCALE
        lo, hi = qa + j / sc, qa + (j + 1) / sc
        pts.append(np.concatenate([rng.uniform(lo, hi, n_random), [0.5 * (lo + hi)]]).astype(np.float32))
        pts.append(neighbours(lo))
    pts += [neighbours(0.25), neighbours(qa), neighbours(float(F_HALF_PI))]
    pts.append(10.0 ** rng.uniform(-3, np.log10(0.25), 400).astype(np.float32))      # the series of D
    a = np.unique(np.concatenate(pts))
    return a[a > 0]



def sweep_set(n_random=6):
    """(15, m) float32: beam widths over every table interval (c2 = 0: a1 = c3 <= pi/2; c1 = 1 and 0.029: a2 = a1 and a1 / 0.029 up to 53.28)"""
    a = table_points(n_random)
    a1 = a[a <= F_HALF_PI]
    cols = []
    for c1, aa in ((1.0, a1), (0.029, a1[a1 > f32(0.03)])):
        x = np.repeat(np.array([[SEMANTICS_BASE[q]] for q in COUPLED_INPUTS], dtype=f64), aa.size, axis=1)
        x[COUPLED_INPUTS.index('c2')], x[COUPLED_INPUTS.index('c1')], x[COUPLED_INPUTS.index('c3')] = 0.0, c1, aa
        cols.append(x)
    return as_f32_inputs(np.concatenate(cols, axis=1))


def edge_set(k):
    """(15, m) float32: the eleven points above; every term of the `plain` predicate one float either side of its threshold; V_cc at and
    next to both clamps; a1 at and above pi/2; c1 -> 0; a1 = 0; |a| at 53.28; NaN, +inf, -inf in each of the 15 inputs in turn."""
    pts = []

    def add(**kw):
        p = dict(SEMANTICS_BASE, **kw)
        pts.append([p[q] for q in COUPLED_INPUTS])
        return len(pts) - 1

    def around(v, steps=(-2, -1, 0, 1, 2)):
        out = []
        for s_ in steps:
            w = f32(v)
            for _ in range(abs(s_)):
                w = np.nextafter(w, f32(np.inf if s_ > 0 else -np.inf))
            out.append(float(w))
        return out
    for e in SEMANTICS_EDITS:
        add(**e)
    qa = float(tables32()['QA_MIN'])
    for c3 in around(qa) + around(-qa) + around(0.25) + around(0.015):
        add(c2=0.0, c1=1.0, c3=c3)                   # a1 = a2 = c3
        add(c2=0.0, c1=0.5, c3=c3)                   # a2 = 2 c3
    for c0 in (0.0, -0.0, 1.0, float(np.nextafter(f32(1), f32(2))), float(np.nextafter(f32(1), f32(0))), float(np.nextafter(f32(0), f32(-1))),
               float(np.nextafter(f32(0), f32(1))), -1e-3, 1.001):
        add(c0=c0)
        add(c0=c0, c2=0.0, c1=1.0, c3=0.05)
    # amplitudes around the 1e-30 term of the predicate: X is proportional to mdot_a
    r0 = restate(as_f32_inputs(np.array([pts[0]]).T), k)
    for c0 in (0.5, 1.0, 0.0):
        for target in (1e-30,):
            scale = target / float(max(r0['X1'][0], r0['X2'][0])) * (0.5 / max(c0, 1 - c0) if c0 in (0.0, 1.0) else 1.0)
            for fct in (0.25, 0.999999, 1.0, 1.000001, 4.0, 1e-4, 1e-7, 1e-9):
                add(c0=c0, mdot_a=5e-6 * scale * fct)
    for c3 in (0.5, 0.05, 0.02):
        add(sigma_cex=0.0, c2=0.0, c1=1.0, c3=c3)    # j_cex = 0 through sigma = 0
        add(c4=0.0, c5=0.0, c2=0.0, c1=1.0, c3=c3)   # ... through n_neutral = 0
        add(sigma_cex=0.0, c0=0.0, c2=0.0, c1=0.2, c3=c3)
    add(sigma_cex=1e-30)                              # 1 - decay rounds to 0 in float, not in double
    # the clamps of V_cc
    add(V_vac=0.0, T_e=1.0, Pstar=1e-6)               # V < 0
    add(V_a=10.0)                                     # V > V_a
    v0 = float(r0['V_cc'][0])
    for va in around(v0, (-3, -2, -1, 0, 1, 2, 3)):
        add(V_a=va)                                   # V_a next to V: the thrust's cancellation
    add(V_a=v0 * (1 + 1e-6))
    add(V_a=v0 * (1 + 1e-4))
    add(V_vac=-28.1)                                  # V next to 0
    add(V_vac=-28.130)
    add(V_vac=-28.2)
    # the clip of a1, a2 = inf, a1 = 0, the overflow bound
    for c3 in around(float(F_HALF_PI)) + [2.0]:
        add(c2=0.0, c3=c3)
    add(c2=1e4, c3=0.5)
    for c1 in (0.0, -0.0, 1e-3, 1e-30, 1e-39, 1e-45, -0.5):
        add(c1=c1)
    add(c2=0.0, c3=0.0)
    add(c2=0.0, c3=0.0, c0=1.0)
    add(c2=0.0, c3=1e-45)
    add(c2=-225.0, c3=0.3)                            # a1 = c2 PB + c3 cancels to about 0
    for c1 in around(1.5 / ALPHA_OVERFLOW, (-3, -2, -1, 0, 1, 2, 3)) + [1.5 / 53.0, 1.5 / 54.0]:
        add(c2=0.0, c3=1.5, c1=c1)
    for q in COUPLED_INPUTS:
        for v in (float('nan'), float('inf'), float('-inf')):
            add(**{q: v})
    return as_f32_inputs(np.array(pts, dtype=f64).T)
