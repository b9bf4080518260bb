"""The fp64 model kernels' high-precision reference, the per-entry bound that holds them to it, and the committed tables restated
bit-faithfully.  TEST INFRASTRUCTURE, no GPU needed.

(a) THE TABLES.  `tables()` parses csrc/pem_tables.h; `normaliser64`, `functionals64` and `exp_nonpos64` restate pem_model.h's
    normaliser(), simpson_functionals() and exp_nonpos() operation by operation with an EXACT fma (`fma`: math.fma where Python has
    it, otherwise Boldo and Melquiond's emulation -- exact product by Dekker, two TwoSums, one addition rounded to odd, one to
    nearest -- which is correctly rounded, not a twice-rounded stand-in).  `D_mp`, `Q_mp` are the truth at 50 digits (the closed erf
    form of the normaliser, cross-checked against quadrature by tests/test_tables_host.py; the literal 91-term sums).  The worst
    errors of the restated tables against them are the TABLE_* constants below, asserted by tests/test_tables_host.py.

(b) THE REFERENCE.  `reference(x, k, radii)` is the coupled PEM-v0 model as the exact real function of its fp64 inputs, evaluated in
    np.longdouble (64-bit significand: 2^-11 of a double's rounding per operation, absorbed in SECOND = 1.01 together with the
    products of errors):
      V = V_vac + T_e log(1 + PB / PT) - T_e PB / (PT + PS), PB = P_b k ..., V_cc = clamp(V, 0, V_a)
      I_B0 = (q/m) mdot, eta_c = 1 - 2 a_1, I_d = I_B0 / eta_c, v_exh = sqrt(2 q (V_a - V_cc) / m), T = mdot v_exh,
      eta_m = 1 - 5 a_1, eta_v = eta_c, eta_a = T^2 / (2 mdot V_a I_d)                   (q, m: the doubles 1.6e-19, 2.18e-25)
      n = c4 PB + c5, a1 = min(c2 PB + c3, fl(pi/2)), a2 = a1 / c1, A1 = (1 - c0) / D(a1), A2 = c0 / D(a2)
      decay_r = exp(-r n sigma), base_r = I_B0 decay_r / r^2, j_cex_r = I_B0 (1 - decay_r) / (2 pi r^2)   (1 - decay by expm1)
      j_ion[k][r] = base_r (A1 g1k + A2 g2k) + j_cex_r, g_ik = exp(-(alpha_k / a_i)^2), alpha_k = k pi / 180
      den_r, num_r = sum_k CDEN_k f_kr, sum_k CNUM_k f_kr (f = j_ion - j_cex), cos_div = num / den, div_angle = arccos, T_c = T cos_div
    The Simpson weights CDEN, CNUM are the 91 doubles of the header taken as exact constants: they DEFINE the model (tests/
    test_tables_host.py holds them to scipy bit for bit).  D(a) = 2 pi Int_0^T exp(-(t/a)^2) sin t dt, T = min(pi/2, 12 |a|) (beyond
    12 |a| the integrand is below e^-144 of its peak), by 16-point Gauss-Legendre on 24 panels of width T / 24 <= |a| / 2 -- the
    panels scale with a, a = 0.0044 is resolved as a = 53 is; nodes from mpmath at 40 digits; never the tables under test.  The
    flags and the NaN rules are the reference implementation's: D is NaN at a = 0 and for |a| > 53.28349511409265, invalid = a1 <= 0
    or some j_ion <= 0, an invalid sample's profile is 1e-20.
    Side products for the bound: every sum again on absolute values, and the per-term exponents t = (alpha_k / a)^2.

(c) THE BOUND.  `bounds(ref, path)`: per entry, the largest error a correct fp64 evaluation can make ON THE PATH THE KERNEL TOOK.
    u = U = 2^-53 is the relative error of one rounded operation (+, -, *, /, sqrt and fma are correctly rounded on the device, which
    tools/microbench/f64_intrinsics.hip confirms for / and sqrt); a library function with a worst error of E ulp has relative error
    <= 2 E u.  Every bound is first order in u and multiplied by SECOND.  The derivation follows tests/hp_fp32.py's, with the
    roundings of the fp64 sources counted anew:

    cathode_vcc (contract off):  PB, PT, PS: u each.  z = PB / PT: 3 u.  w = fl(1 + z): |w| u + 3 u |z| absolute, which log turns into
      the ABSOLUTE error u (1 + 3 |z / w|); log adds LOG u |log w| (LOG = 2 LOG_ULPS).  T_e * lg: u.  V_vac + .: u of the sum.
      q = T_e / (PT + PS): the sum (1 + cs) u, cs = (|PT| + |PS|) / |PT + PS|; the quotient u; q * PB: PB's u and the product's u; the
      difference u |V|, |V| <= |V_vac| + |T_e log w| + |t3|:
        bound_V = u [ 2 |V_vac| + (3 + LOG) |T_e log w| + |T_e| (1 + 3 |z / w|) + (cs + 5) |t3| ]
      The clamp is 1-Lipschitz: the clamped value is held to [clamp(V - bound_V), clamp(V + bound_V)], never skipped.
    thruster_stage (contract off):  I_B0: 2 u (the constant q / m is rounded, the product is).  eta_c = fl(1 - fl(2 a_1)): 2 a_1 is exact,
      one rounding: u |eta_c|.  I_d = I_B0 / eta_c: (2 + 1 + 1) u -- relative to I_d; eta_c's rounding is relative to eta_c itself, so
      near eta_c = 0 the bound does not blow up unless eta_c is exactly where 1 - 2 a_1 cancels: the subtraction of two doubles within
      a factor 2 is EXACT (Sterbenz), the error is 0 there; the bound keeps u and is simply safe.
      v_exh = sqrt(2 q x / m), x = V_a - V_cc: bound_x = bound_V + u |x| absolute; 2 q: exact; the product, the quotient: 2 u; sqrt
      halves what is under it (u) and adds its own u (correctly rounded); monotone: bound_v = c (sqrt(x + d) - sqrt(max(x - d, 0))) + 3 u v with
      c = sqrt(2 q / m), d = bound_x -- near the clamp V_cc = V_a this GROWS to c sqrt(d), the sample is compared, not dropped.
      T = mdot v_exh: + u.  eta_m: 5 a_1 rounds: u |5 a_1| + u |eta_m| absolute.  eta_v = eta_c.
      eta_a = 0.5 (T T) / ((mdot V_a) I_d): relative 2 e_T + u + (u + e_Id + u) + u.
    plume_setup (contract off):  PB: u.  n = fl(fl(c4 PB) + c5): 2 u |c4 PB| + u |n| absolute.  a1 = fl(fl(c2 PB) + c3): 2 u |c2 PB| + u |a1|
      absolute -- e_a1 = u (1 + 2 |c2 PB| / |a1|) relative, the conditioning of the beam width that every Gaussian then carries as the
      ABSOLUTE error 2 e_a t of its exponent t = (alpha_k / a)^2 (the clip at fl(pi/2) is exact: e_a1 = 0 where the reference is
      clipped and not within e_a1 of the clip).  a2 = a1 / c1: e_a2 = e_a1 + u.
    amplitudes:  u_i = 1 / (a a): 2 u.  D(a) AS THE KERNEL EVALUATES IT from the double a (a * a, 1 / ., the index, the Horner scheme)
      is within TABLE_D_ERR of the truth (measured, (a)); so A1 = (1 - c0) / D(a1): e_A1 = TABLE_D_ERR + 2 e_a1 + 2 u (kappa_D =
      dlog D / dlog a lies in [0, 2]), A2 = c0 / D(a2): e_A2 = TABLE_D_ERR + 2 e_a2 + u.
      decay = exp(arg), arg = -r n sigma: two products, n's own error: the exponent is off by |arg| (2 u + e_n) ABSOLUTE, exp adds EXP u:
      e_decay = |arg| (2 u + e_n) + EXP u.  base = I_B0 decay / r^2 (R = 1: * fl(1 / fl(r r))): e_base = 2 u + e_decay + 4 u.
      j_cex = I_B0 (1 - decay) / (2 pi r^2): |decay| e_decay absolute on 1 - decay, which then rounds; 2 + 5 roundings around it:
        b_jcex = unit (|decay| e_decay + 8 u |1 - decay|), unit = |I_B0| / (2 pi r^2).
      X_i = base A_i: e_X = e_base + e_A + u.
    Gaussians, per path, as relative error of g_k = exp(-t_k):  e_g(k) = t_k (2 e_a + C_path u) + N_path(k) u
      the first part is the conditioning of the exponent: the beam width's error, the rounding of the grid angle or of the step
      (GRID_H = fl(fl(pi/2) / 90): 1.5 u, squared: 3 u; u_i: 2 u; the product s = GRID_H^2 u_i: u; the integer multiple m s handed to
      exp_nonpos: u -- C_rec = 3 + 2 + 1 + 1 = 7;  literal: alpha_k = fl(k GRID_H): 2.5 u, t = alpha / a: u, t t: u -- C_lit = 2 (2.5 + 1) + 1 = 8);
      N counts the roundings of values:
      LITERAL (exact_chunk, literal_sample, plume_radii_kernel, the literal passes of the others): N = EXP (library exp: 2 EXP_ULPS).
      RECURRENCE in chunks of CH angles over L chunk lanes (plume_r1_kernel: CH = 23; coupled_latent_kernel the same; plume_rfew_kernel:
        CH = 12): seeds r0 = e^-s, G = e^-2CHs, E = e^-CH^2 s by exp_nonpos, each off by XNP u in value (XNP = 2 EXPNP_ULPS).  The chunk
        start c: X_c = X prod_{i<c} rho_i, rho_i = E (E E)^i: c products, c E's, i (E E)'s with 2 XNP + 1 each and i products:
          N_X(c) = c + c XNP + c (c - 1) / 2 (2 XNP + 2);   rr_c = r0 G^c: N_rr(c) = XNP + c (XNP + 1);   q = r0 r0: N_q = 2 XNP + 1.
        Inside the chunk X_{j} = X_c prod_{i<j} rr_i, rr_i = rr_c q^i with i products:
          N(c, j) = N_X(c) + j + j N_rr(c) + j (j - 1) / 2 (N_q + 1)
        -- the growth is quadratic in the position inside the chunk and in the chunk index: 1539 u = 1.7e-13 at the end of the last
        chunk of CH = 23 with XNP = 2 (EXPNP_ULPS = 1), a function of k; with the exponent's part, of k and t.
      DIRECT START (plume_rmid_kernel: chunks of ceil(91 / R) angles, e_k0, r_k0, q = e^-2s each by one exp_nonpos):
          N(j) = XNP + j + j XNP + j (j - 1) / 2 (XNP + 1)
      WHOLE SWEEP (plume_generic_kernel: e = 1, r = exp(-s), q = exp(-2 s) by the library exp, k steps): N(k) = k + k EXP + k (k - 1) / 2 (EXP + 1).
    profile:  f_k = X1 g1k + X2 g2k (products rounded on the literal paths and where amplitudes multiply Gaussians: u each; the sum: u),
      j_k = f_k + j_cex (u):
        b_j(k) = |X1| g1k (e_X1 + e_g1(k) + 2 u) + |X2| g2k (e_X2 + e_g2(k) + 2 u) + b_jcex + u |j_k|
      -- on the sum of MAGNITUDES: where the amplitudes have opposite signs or j_cex is negative, cancellation, and nothing else, widens
      the bound relative to the result.  Mixed mode: the rounded fp64 profile, + 2^-24 |j_k| (checked bit for bit against the fp64 run).
      A chunk whose smallest value is below 1e-290 takes the literal path; a sample whose smallest j_ion is within a factor 2 of that
      switch or below it takes the larger of the two bounds.  Results in the denormal range round ABSOLUTELY: every bound carries a few
      units of 2^-1074 times the amplitudes (a Gaussian there is within EXP_ULPS units of 2^-1074).
    Simpson sums (fma fold, CH or 91 terms; partial sums added):  with W the weights and N_SUM = 100 (91 additions in any order, the product of
      a term where it is not fused, up to 8 partial sums),
        b_sum = sum_k |W_k| (b_f(k)) + N_SUM u sum_k |W_k f_k|,   b_f(k) = b_j(k) without j_cex and its rounding
      `base` is common to every term of num and den and cancels in the quotient: e_X excludes e_base for cos_div.
      Table path (reduced mode, `plain`): Q AS THE KERNEL EVALUATES IT is within TABLE_Q_ERR of the truth; den = fma(X1, Qd1, X2 Qd2):
        e = [ |X1 Qd1| (e_A1 + u + TABLE_Q_ERR + kappa_Q(a1) e_a1) + |X2 Qd2| (e_A2 + u + TABLE_Q_ERR + kappa_Q(a2) e_a2 + u) ] / |den| + u.
      cos_div = num / den takes the SAME f_k in both sums: an error d_k of f_k moves the quotient by (CNUM_k - cos_div CDEN_k) d_k / den,
      not by the sum of what it does to num and to den; what the sums do not share is their own rounding:
        |cos_div| e_cos = [ sum_k |CNUM_k - cos_div CDEN_k| b_f(k) / |den| + N_SUM u (den_abs / |den| + num_abs / |num|) |cos_div| + u |cos_div| ] / (1 - e_den)
      e_den >= 1/2: den is within twice its bound of 0, `den against 0`.  (The table path's Qd and Qn come from two polynomials and share nothing.)
      div_angle through the cosine, as parity_rules.divergence_error does: |cos(got) - cos(want)| <= |cos_div| e_cos + |sin w| da + da^2 / 2,
      da = ACOS u |w| + 2^-1074 (acos's own error).  T_c = T cos_div: |cos| b_T + (|T| + b_T) |cos| e_cos + u |T_c|.
    latents (coupled_latent_kernel): lat_r = sum_k norm(j_k) B_kr by 91 fma: (91 u + e_norm(k)) sum_k |norm(j_k) B_kr| with
      e_norm = b_j / |j_k| for norm none; for log10 the ABSOLUTE error b_j / (|j_k| ln 10) + LOG10 u |log10 j_k| per term.

    EXCUSES.  Where the reference of a deciding quantity lies within its own bound of a threshold the flag or NaN pattern may differ:
      a1 against 0; the profile against 0, term by term; |a| against 53.28349511409265; den against 0; |cos_div| against 1; the
      smallest j_ion against 1e-290 (path, hence bound: the larger applies).  Caps, asserted on the reference alone by
      tests/test_hp_model_host.py: none on the prior and width sets, at most 2 % on the tail and cancellation sets.
      A finite reference with a bound that is not finite FAILS.
"""
import math
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / 'hallthrusterpem_amd' / 'csrc'
f64 = np.float64
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, 'np.longdouble must carry a 64-bit significand'
U = 2.0 ** -53
SECOND = 1.01
ALPHA_OVERFLOW = 53.28349511409265
HALF_PI = 1.5707963267948966
GRID_H = HALF_PI / 90.0
NANG = 91
Q_E, M_ION = 1.6e-19, 2.18e-25
COUPLED_INPUTS = ('P_b', 'V_a', 'T_e', 'V_vac', 'Pstar', 'P_T', 'mdot_a', 'a_1', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')
SWITCH = 1e-290            # below it a chunk is evaluated literally

# Worst errors of the device's fp64 library functions in ulps of the result, each rounded UP to the next half ulp and to nothing more:
# profiles/f64_intrinsics_r01.txt (tools/microbench/f64_intrinsics.hip on an MI355X; random arguments and binade edges over the
# ranges the model uses, against long double).
EXP_ULPS = 1.0            # measured 0.8730 (exp(x), -745.2 <= x <= 88; 0.84 units of 2^-1074 where the result is denormal)
LOG_ULPS = 1.0            # measured 0.6313 (log(x), x = 1 + 10^[-16, 9]: the model takes log(1 + PB / PT))
ACOS_ULPS = 1.0           # measured 0.7534 (acos(x), |x| <= 1)
LOG10_ULPS = 1.0          # measured 0.6030 (log10(x); pem_math.h's own log10 functions: LOG10_TAB_ULPS, LOG10_SERIES_ULPS below)
DIV_ULPS = 0.5            # measured 0.5000: a / b is correctly rounded
SQRT_ULPS = 0.5           # measured 0.5000: sqrt(x) is correctly rounded
# exp_nonpos (pem_model.h; pure fp64 and fma) restated with an exact fma and measured against mpmath on the host over [-708, 0]:
# tests/test_tables_host.py asserts it (the device's own: 0.8579 in the same file of profiles/)
EXPNP_ULPS = 1.0          # measured 0.8367

# Worst relative errors of the tables evaluated AS THE KERNEL DOES from a double a (a * a, 1 / (a a), index, Horner by fma), against the
# truth at 50 digits, over every interval with both sides of every edge: measured and asserted by tests/test_tables_host.py, in
# units of U, rounded up to the next half ulp (= U).
TABLE_D_ERR = 4.0 * U             # measured 3.075 = 3.41e-16 (a = 1.63299..., u = 3/8, interval 0; the series below 0.25: 1.885)
TABLE_QD_ERR = 4.0 * U            # measured 3.718 = 4.13e-16 (a = 0.15289, region B; region A 2.658)
TABLE_QN_ERR = 5.0 * U            # measured 4.118 = 4.57e-16 (a = 0.18598, region B; region A 2.218)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) exact fma, the tables, the restatements
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a          # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_eft(a, b, c):
    """round-to-nearest(a b + c), one rounding: Boldo and Melquiond's emulation (finite arguments away from over- and underflow)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, f64), np.asarray(b, f64), np.asarray(c, f64))
    with np.errstate(all='ignore'):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, ul)
        vh, vl = _two_sum(uh, th)
        s, e = _two_sum(tl, vl)
        # s = tl + vl rounded to ODD: if inexact and the significand of s is even, the neighbour on the side of the remainder
        even = (s.view(np.int64) & 1) == 0
        s = np.where((e != 0.0) & even, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
        return vh + s


if hasattr(math, 'fma'):
    _vfma = np.frompyfunc(math.fma, 3, 1)

    def fma(a, b, c):
        return np.asarray(_vfma(np.asarray(a, f64), np.asarray(b, f64), np.asarray(c, f64)), dtype=f64)
else:
    fma = fma_eft


def _parse(name, text):
    from hp_fp32 import _parse as parse
    return parse(name, text)


_tables = None


def tables(path=None):
    """csrc/pem_tables.h: the five tables and the #defines"""
    global _tables
    if _tables is not None and path is None:
        return _tables
    text = Path(path or CSRC / 'pem_tables.h').read_text()
    out = {k: int(re.search(r'#define PEM_%s (\d+)\s' % k, text).group(1)) for k in ('NDAW', 'NDI', 'NDC', 'NQB')}
    for k in ('QA_MIN', 'QB_SCALE'):
        out[k] = float(re.search(r'#define PEM_%s (\S+)\s' % k, text).group(1))
    for name, shape in (('SIMPSON_CDEN', (NANG,)), ('SIMPSON_CNUM', (NANG,)), ('DAWSON', (out['NDAW'],)), ('DPOLY', (out['NDI'], out['NDC'])),
                        ('QPOLY', (out['NDI'] + out['NQB'], out['NDC'], 2))):
        v = _parse('PEM_' + name, text)
        assert v.size == int(np.prod(shape)), (name, v.size)
        out[name] = v.reshape(shape)
    if path is None:
        _tables = out
    return out


def _to_int(t):
    """(int)t of a double: truncation, NaN -> 0, saturating"""
    t = np.asarray(t, f64)
    return np.trunc(np.clip(np.nan_to_num(t, nan=0.0, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def _horner(rows, x):
    acc = rows[:, -1]
    for j in range(rows.shape[1] - 2, -1, -1):
        acc = fma(acc, x, rows[:, j])
    return acc


def normaliser64(a, tab=None):
    """pem_model.h normaliser(a, 1 / (a * a), PEM_DPOLY), operation by operation"""
    tab = tab or tables()
    a = np.atleast_1d(np.asarray(a, f64))
    with np.errstate(all='ignore'):
        a2 = a * a
        u = 1.0 / a2
        i = np.clip(_to_int(2.0 * u), 0, tab['NDI'] - 1)
        x = fma(4.0, u, -(2 * i + 1).astype(f64))
        d = _horner(tab['DPOLY'][i], np.where(np.isfinite(x), x, 0.0))
        y = 0.5 * a2
        s = np.full(a.shape, tab['DAWSON'][-1])
        for j in range(tab['NDAW'] - 2, -1, -1):
            s = fma(s, np.where(np.isfinite(y), y, 0.0), tab['DAWSON'][j])
        D = np.where(np.abs(a) < 0.25, math.pi * a2 * s, d)
        bad = ~(np.abs(a) <= ALPHA_OVERFLOW) | (a == 0.0)
    return np.where(bad, np.nan, D)


def functionals64(aa, tab=None):
    """pem_model.h simpson_functionals(qpoly, |a|, 1 / (a * a)): (Qd, Qn)"""
    tab = tab or tables()
    aa = np.atleast_1d(np.asarray(aa, f64))
    with np.errstate(all='ignore'):
        u = 1.0 / (aa * aa)
        wide = aa >= 0.25
        t = np.where(wide, 2.0 * u, (aa - tab['QA_MIN']) * tab['QB_SCALE'])
        last = np.where(wide, tab['NDI'] - 1, tab['NQB'] - 1)
        i = np.maximum(np.minimum(_to_int(t), last), 0)
        x = 2.0 * (t - i.astype(f64)) - 1.0
        rows = tab['QPOLY'][np.where(wide, 0, tab['NDI']) + i]
        return _horner(rows[:, :, 0], x), _horner(rows[:, :, 1], x)


_EXPNP = [float(s) for s in ('1.6059043836821614599e-10', '2.0876756987868098979e-09', '2.5052108385441718775e-08', '2.7557319223985890653e-07',
                             '2.7557319223985890653e-06', '2.4801587301587301587e-05', '1.9841269841269841270e-04', '1.3888888888888888889e-03',
                             '8.3333333333333333333e-03', '4.1666666666666666667e-02', '1.6666666666666666667e-01', '0.5', '1.0', '1.0')]


def exp_nonpos64(x):
    """pem_model.h exp_nonpos(x), operation by operation (results in the normal range)"""
    x = np.fmax(np.asarray(x, f64), -800.0)
    n = np.rint(x * 1.4426950408889634074)
    r = fma(n, -6.93147180369123816490e-01, x)
    r = fma(n, -1.90821492927058770002e-10, r)
    p = np.full(r.shape, _EXPNP[0])
    for c in _EXPNP[1:]:
        p = fma(p, r, c)
    return np.ldexp(p, n.astype(np.int64))


def D_mp(a, dps=50):
    """D(a) = 2 pi Int_0^{pi/2} exp(-(t/a)^2) sin t dt in closed form: completing the square in -t^2/a^2 + i t,
    D(a) = 2 pi Im Int_0^{pi/2} exp(-t^2/a^2 + i t) dt = pi^(3/2) a e^(-a^2/4) Im[ erf(pi/(2a) - i a/2) + erf(i a/2) ]"""
    import mpmath as mp
    with mp.workdps(dps + int(abs(float(a)) ** 2 / 4 / 2.3) + 10):      # e^(a^2/4) cancels between the two erf: carry its digits
        a = mp.mpf(float(a))
        z = mp.erf(mp.mpc(mp.pi / (2 * a), -a / 2)) + mp.erf(mp.mpc(0, a / 2))
        return +(mp.pi ** mp.mpf(1.5) * a * mp.exp(-a * a / 4) * z.imag)


def D_quad_mp(a, dps=40):
    """the same by quadrature (the cross-check of the closed form)"""
    import mpmath as mp
    with mp.workdps(dps):
        a = mp.mpf(float(a))
        T = min(mp.pi / 2, 14 * abs(a))
        return +(2 * mp.pi * mp.quad(lambda t: mp.exp(-(t / a) ** 2) * mp.sin(t), mp.linspace(0, T, 29)))


def Q_mp(a, tab=None, dps=40):
    """(Qd, Qn) = sum_k C_k exp(-(k pi / (180 a))^2) with the header's double weights taken exactly"""
    import mpmath as mp
    tab = tab or tables()
    with mp.workdps(dps):
        s = (mp.pi / 180 / mp.mpf(float(a))) ** 2
        e = [mp.exp(-(k * k) * s) for k in range(NANG)]
        return (mp.fsum(mp.mpf(float(c)) * g for c, g in zip(tab['SIMPSON_CDEN'], e)),
                mp.fsum(mp.mpf(float(c)) * g for c, g in zip(tab['SIMPSON_CNUM'], e)))


def neighbours(v, m=2):
    out = [f64(v)]
    lo = hi = f64(v)
    for _ in range(m):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.array(out)


def table_points():
    """(points of D, points of Q): doubles a > 0 -- both sides of every interval edge (the doubles around each knot, where (int)t
    flips), the clamp at u = 16, both sides of 0.25 and QA_MIN, seven interior points per interval (u = i/2 + j/16: a = 1.63299 is
    u = 3/8), the series down to 1e-3, up to the overflow bound"""
    tab = tables()
    d, q = [], []
    for i in range(tab['NDI']):
        uu = i / 2.0 + np.arange(1, 8) / 16.0
        d.append(1.0 / np.sqrt(uu))
        d.append(neighbours(1.0 / math.sqrt((i + 1) / 2.0)))
    d.append(1.0 / np.sqrt(np.array([1e-3, 3.5e-4 + 1.0 / ALPHA_OVERFLOW ** 2, 0.01, 0.03, 0.0625])))     # interval 0 towards u = 0
    d += [neighbours(ALPHA_OVERFLOW)[[0, 1, 3]], np.array([1.63299, 53.28, 53.0, 50.0, 30.0, 10.0, HALF_PI])]
    q = [np.concatenate(d)]
    d.append(10.0 ** np.linspace(-3, math.log10(0.25), 40)[:-1])
    d.append(neighbours(0.25))
    qa, sc = tab['QA_MIN'], tab['QB_SCALE']
    for j in range(tab['NQB']):
        q.append(qa + (j + np.arange(1, 8) / 8.0) / sc)
        q.append(neighbours(qa + j / sc))
    q += [neighbours(0.25), np.array([0.184687]), np.array([1e6, 1e3])]
    dd, qq = np.unique(np.concatenate(d)), np.unique(np.concatenate(q))
    return dd[dd <= ALPHA_OVERFLOW], qq[qq >= qa]


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _ld(v):
    """an mpmath number as a long double (two doubles added exactly)"""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


_consts = None


def _constants():
    """pi, the 16-point Gauss-Legendre rule (Newton on P_16 at 40 digits) and the grid angles k pi / 180 as long doubles"""
    global _consts
    if _consts is None:
        import mpmath as mp
        with mp.workdps(40):
            npts = 16
            xs, ws = [], []
            for z0 in np.polynomial.legendre.leggauss(npts)[0]:
                z = mp.mpf(float(z0))
                for _ in range(8):
                    p1, p2 = mp.mpf(1), mp.mpf(0)
                    for j in range(1, npts + 1):
                        p1, p2 = ((2 * j - 1) * z * p1 - (j - 1) * p2) / j, p1
                    pp = npts * (z * p1 - p2) / (z * z - 1)
                    dz = p1 / pp
                    z -= dz
                assert abs(dz) < mp.mpf(10) ** -35
                xs.append(_ld(z))
                ws.append(_ld(2 / ((1 - z * z) * pp * pp)))
            _consts = {'pi': _ld(mp.pi), 'glx': np.array(xs, dtype=LD), 'glw': np.array(ws, dtype=LD),
                       'alpha': np.array([_ld(k * mp.pi / 180) for k in range(NANG)], dtype=LD)}
    return _consts


def D_ld(a, panels=24):
    """the normaliser by panel Gauss-Legendre quadrature in long double; NaN at 0, beyond the overflow bound, for inf and NaN"""
    c = _constants()
    a = np.atleast_1d(np.asarray(a, LD))
    with np.errstate(all='ignore'):
        aa = np.abs(a)
        ok = (aa > 0) & (aa <= LD(ALPHA_OVERFLOW))
        aa = np.where(ok, aa, LD(1))
        T = np.minimum(c['pi'] / 2, 12 * aa)
        hw = T / (2 * panels)
        t = ((2 * np.arange(panels) + 1)[None, :, None] + c['glx'][None, None, :]) * hw[:, None, None]
        f = np.exp(-(t / aa[:, None, None]) ** 2) * np.sin(t)
        D = 2 * c['pi'] * hw * np.sum(f * c['glw'][None, None, :], axis=(1, 2))
    return np.where(ok, D, LD(np.nan))


def as_inputs(x, names=COUPLED_INPUTS):
    """dict or (len(names), n) array -> dict of contiguous fp64 arrays (n,)"""
    if not isinstance(x, dict):
        x = {q: np.asarray(x)[i] for i, q in enumerate(names)}
    n = np.broadcast(*[x[q] for q in names]).size
    return {q: np.ascontiguousarray(np.broadcast_to(np.asarray(x[q], f64), (n,))) for q in names}


def cathode_reference(X, k):
    """V_cc of cathode_vcc and its bound; X: long double inputs"""
    k = LD(float(k))
    with np.errstate(all='ignore'):
        PB, PT, PS = X['P_b'] * k, X['P_T'] * k, X['Pstar'] * k
        z = PB / PT
        w = 1 + z
        Tlg = X['T_e'] * np.log1p(z)
        t3 = X['T_e'] * PB / (PT + PS)
        V_un = X['V_vac'] + Tlg - t3
        V_a = X['V_a']
        clamp = lambda v: np.where(v > V_a, V_a, np.where(v < 0, LD(0), v))                     # noqa: E731
        cs = ((np.abs(PT) + np.abs(PS)) / np.abs(PT + PS)).astype(f64)
        zw = np.abs(z / w).astype(f64)
        L = 2.0 * LOG_ULPS
        bV = SECOND * U * (2.0 * np.abs(X['V_vac']) + (3.0 + L) * np.abs(Tlg) + np.abs(X['T_e']) * (1.0 + 3.0 * zw) + (cs + 5.0) * np.abs(t3)).astype(f64)
        return {'V_un': V_un, 'V_cc': clamp(V_un), 'bound_V': bV, 'V_lo': clamp(V_un - bV), 'V_hi': clamp(V_un + bV)}


THRUSTER_OUT = ('I_B0', 'I_d', 'T', 'eta_c', 'eta_m', 'eta_v', 'eta_a', 'v_exh')


def thruster_reference(V_a, V_cc, mdot, a_1, V_lo=None, V_hi=None):
    """thruster_stage: values (long double) and absolute bounds 'b_<name>'.  V_lo, V_hi: the interval a computed V_cc may lie in
    (the coupled kernels; None: V_cc is an input)."""
    V_a, V_cc, mdot, a_1 = (np.asarray(v, LD) for v in (V_a, V_cc, mdot, a_1))
    out = {}
    with np.errstate(all='ignore'):
        I_B0 = (LD(Q_E) / LD(M_ION)) * mdot
        eta_c = 1 - 2 * a_1
        I_d = I_B0 / eta_c
        x = V_a - V_cc
        c = np.sqrt(2 * LD(Q_E) / LD(M_ION))
        v = c * np.sqrt(x)
        T = mdot * v
        eta_m = 1 - 5 * a_1
        eta_a = T * T / (2 * mdot * V_a * I_d)
        d = U * np.abs(x) if V_lo is None else np.maximum(V_hi - V_cc, V_cc - V_lo) + U * np.abs(x)
        b_v = c * (np.sqrt(x + d) - np.sqrt(np.maximum(x - d, 0))) + 3.0 * U * np.abs(v)
        b_T = np.abs(mdot) * b_v + U * np.abs(T)
        e_T = np.where(T == 0, 0.0, b_T / np.abs(T))
        vals = {'I_B0': (I_B0, 2.0 * U * np.abs(I_B0)), 'I_d': (I_d, 4.0 * U * np.abs(I_d)), 'T': (T, b_T), 'eta_c': (eta_c, U * np.abs(eta_c)),
                'eta_m': (eta_m, U * (np.abs(5 * a_1) + np.abs(eta_m))), 'eta_v': (eta_c, U * np.abs(eta_c)),
                'eta_a': (eta_a, (2.0 * e_T + 8.0 * U) * np.abs(eta_a)), 'v_exh': (v, b_v)}
        for q, (val, b) in vals.items():
            out[q] = val
            out['b_' + q] = (SECOND * b).astype(f64) + 2.0 * TINY          # (a result in the denormal range rounds absolutely)
    return out


def uion_reference(v_exh, z0, z1, ncells):
    """thruster_uion_kernel: u_ion (n, ncells) long double, its absolute bound, and the nodes z"""
    v = np.asarray(v_exh, LD)[:, None]
    z0, z1 = LD(float(z0)), LD(float(z1))
    with np.errstate(all='ignore'):
        frac = np.arange(ncells).astype(LD) / LD(ncells - 1)
        z = z0 + (z1 - z0) * frac
        b_z = U * (3.0 * np.abs((z1 - z0) * frac) + np.abs(z))
        e = -100 * (z - LD(0.04))
        b_e = 100.0 * (b_z + U * np.abs(z - LD(0.04))) + U * np.abs(e)
        E = np.exp(e)
        den = 1 + E
        rel = E * (b_e + 2.0 * EXP_ULPS * U) / den + 3.0 * U
        u = v / den[None, :]
    return u, (SECOND * rel[None, :] * np.abs(u)).astype(f64), z.astype(f64)


def reference(x, k, radii=(1.0,), I_B0=None, T=None):
    """the coupled model; with I_B0 (and T) given, the plume stage alone on those doubles as exact inputs (current_density)"""
    x = as_inputs(x)
    n = len(x['P_b'])
    X = {q: v.astype(LD) for q, v in x.items()}
    c = _constants()
    tab = tables()
    rad = np.atleast_1d(np.asarray(radii, f64)).astype(LD)
    kk = LD(float(k))
    ref = {'x': x, 'n': n, 'k': float(k), 'radii': rad}
    with np.errstate(all='ignore'):
        ref.update(cathode_reference(X, k))
        ref.update(thruster_reference(X['V_a'], ref['V_cc'], X['mdot_a'], X['a_1'], ref['V_lo'], ref['V_hi']))
        if I_B0 is not None:
            ref['I_B0'] = np.asarray(I_B0, f64).astype(LD)
            ref['T'] = np.full(n, np.nan, LD) if T is None else np.asarray(T, f64).astype(LD)
            ref['b_T'] = np.zeros(n)
        ref.update(plume_reference(X, ref['I_B0'], kk, rad, c, tab))
        ref['T_c'] = ref['T'][:, None] * ref['cos_div']
    return ref


def plume_reference(X, I_B0, kk, rad, c=None, tab=None):
    """the plume stage from long double inputs X (P_b, c0 .. c5, sigma_cex) and I_B0: the factors of the profile
    j_ion[k][r] = base_r (A1 g1k + A2 g2k) + j_cex_r, the Simpson sums with their sums of magnitudes, the flags"""
    c = c or _constants()
    tab = tab or tables()
    out = {}
    with np.errstate(all='ignore'):
        PB = X['P_b'] * kk
        c2PB, c4PB = X['c2'] * PB, X['c4'] * PB
        a1_un = c2PB + X['c3']
        clipped = a1_un > LD(HALF_PI)
        a1 = np.where(clipped, LD(HALF_PI), a1_un)
        a2 = a1 / X['c1']
        nn = c4PB + X['c5']
        A1, A2 = (1 - X['c0']) / D_ld(a1), X['c0'] / D_ld(a2)
        t1, t2 = (c['alpha'][None, :] / a1[:, None]) ** 2, (c['alpha'][None, :] / a2[:, None]) ** 2
        g1, g2 = np.exp(-t1), np.exp(-t2)
        arg = -rad[None, :] * (nn * X['sigma_cex'])[:, None]
        decay = np.exp(arg)
        unit = I_B0[:, None] / (2 * c['pi'] * rad[None, :] ** 2)
        base = I_B0[:, None] * decay / rad[None, :] ** 2
        j_cex = -unit * np.expm1(arg)
        shape = A1[:, None] * g1 + A2[:, None] * g2                              # (n, 91)
        # a term whose amplitude is exactly zero is exactly zero whatever its Gaussian (0 * NaN aside: the kernels and the
        # reference implementation give NaN there, and so does this)
        out.update(a1=a1, a2=a2, a1_un=a1_un, clipped=clipped, c2PB=c2PB, c4PB=c4PB, n_neutral=nn, A1=A1, A2=A2, t1=t1, t2=t2, g1=g1, g2=g2,
                   arg=arg, decay=decay, unit=unit, base=base, j_cex=j_cex, shape=shape)
        for name, C in (('den', tab['SIMPSON_CDEN']), ('num', tab['SIMPSON_CNUM'])):
            C = C.astype(LD)
            s = shape @ C
            out['s_' + name] = s
            out[name] = base * s[:, None]
            out[name + '_abs'] = np.abs(base) * ((np.abs(A1)[:, None] * g1 + np.abs(A2)[:, None] * g2) @ np.abs(C))[:, None]
        cos = out['num'] / np.where(out['den'] == 0, LD(np.nan), out['den'])
        out['cos_div'] = cos
        out['div_angle'] = np.arccos(cos)
        # plume.py:105: a1 <= 0 or some j_ion <= 0; the extremes of the shape decide per radius (base_r shape_k + j_cex_r is monotone in shape_k)
        smin, smax = np.nanmin(shape, axis=1), np.nanmax(shape, axis=1)
        jmin = np.minimum(base * smin[:, None], base * smax[:, None]) + j_cex
        out['j_min'] = jmin
        out['invalid'] = (a1 <= 0) | np.any(jmin <= 0, axis=1)
    return out


def j_ion(ref, r=None):
    """the profile (n, 91, R) -- or (n, 91) at radius index r -- in long double, the 1e-20 fill of invalid samples included"""
    with np.errstate(all='ignore'):
        if r is None:
            j = ref['base'][:, None, :] * ref['shape'][:, :, None] + ref['j_cex'][:, None, :]
            return np.where(ref['invalid'][:, None, None], LD(1e-20), j)
        j = ref['base'][:, None, r] * ref['shape'] + ref['j_cex'][:, None, r]
        return np.where(ref['invalid'][:, None], LD(1e-20), j)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the bound
# ---------------------------------------------------------------------------------------------------------------------------------
TINY = 2.0 ** -1074
# the paths: which Gaussians, in chunks of how many angles; which Simpson sums
PATH_R1 = {'gauss': 'chunk', 'CH': 23, 'sums': 'fold'}                # plume_r1_kernel<4, ...> with a profile; coupled_latent_kernel
PATH_R1_REDUCED = {'gauss': 'chunk', 'CH': 23, 'sums': 'table'}       # ... reduced mode: `plain` samples take the tables, the others the loop
PATH_RFEW = {'gauss': 'chunk', 'CH': 12, 'sums': 'fold'}              # plume_rfew_kernel (2 .. 8 radii)
PATH_RADII = {'gauss': 'literal', 'sums': 'fold'}                     # plume_radii_kernel (9 .. 12, 65 .. 256 radii)
PATH_GENERIC = {'gauss': 'sweep', 'sums': 'fold'}                     # plume_generic_kernel (more than 256 radii)
PATH_ORACLE = {'gauss': 'literal', 'sums': 'fold', 'oracle': True}    # oracle/pem_oracle.c: literal exponentials, Gauss-Legendre normaliser
N_SUM = 100.0        # 91 additions in any order, the product of a term where it is not fused, up to 8 partial sums added
# the oracle's normaliser: 32-point Gauss-Legendre on [0, min(pi/2, 6.5 |a|)] -- the truncation (< 5e-19 of the peak), 32 products and
# additions of positive terms, exp and sin of each node with the conditioning of the exponent (up to 42 u at the last node, where the
# integrand is e^-42 of its peak: a weighted mean below 4 u): 64 u = 7e-15 covers it (tests/test_hp_model_host.py measures 4.8 u and asserts the figure)
ORACLE_D_ERR = 64.0 * U


def path_rmid(R):
    return {'gauss': 'direct', 'CH': (NANG + R - 1) // R, 'sums': 'fold'}      # plume_rmid_kernel (13 .. 64 radii)


def path_for_radii(R):
    """DESIGN section 4.2's dispatch"""
    if R == 1:
        return PATH_R1
    if R <= 8:
        return PATH_RFEW
    if R <= 12 or 65 <= R <= 256:
        return PATH_RADII
    return path_rmid(R) if R <= 64 else PATH_GENERIC


def gauss_counts(path):
    """(N(k) for k = 0 .. 90, C): the roundings of VALUES behind the Gaussian of angle k, and the roundings of its EXPONENT"""
    XNP, EXP = 2.0 * EXPNP_ULPS, 2.0 * EXP_ULPS
    k = np.arange(NANG, dtype=f64)
    kind = path['gauss']
    if kind == 'literal':
        return np.full(NANG, EXP), 8.0
    if kind == 'chunk':
        c, j = np.floor(k / path['CH']), k % path['CH']
        n_x = c + c * XNP + c * (c - 1) / 2 * (2 * XNP + 2)
        n_rr = XNP + c * (XNP + 1)
        return n_x + j + j * n_rr + j * (j - 1) / 2 * (2 * XNP + 2), 7.0
    if kind == 'direct':
        j = k % path['CH']
        return XNP + j + j * XNP + j * (j - 1) / 2 * (XNP + 1), 7.0
    assert kind == 'sweep'
    return k + k * EXP + k * (k - 1) / 2 * (EXP + 1), 7.0


def kappa_q(ref, which):
    """(kappa_Qd, kappa_Qn, Qd, Qn) of beam `which` (1 or 2): dlog Q / dlog a = sum C g 2 t / sum C g, from the reference's Gaussians"""
    tab = tables()
    g, t = ref['g%d' % which], ref['t%d' % which]
    with np.errstate(all='ignore'):
        out = []
        for C in (tab['SIMPSON_CDEN'], tab['SIMPSON_CNUM']):
            q = g @ C.astype(LD)
            out.append(((g * 2 * t) @ C.astype(LD) / q).astype(f64))
            out.append(q)
    return out[0], out[2], out[1], out[3]


def bounds(ref, path, plain=None):
    """Everything but the profile's per-entry bound (`j_bound`): bound_V and the clamped interval, the thruster bounds (already in ref),
    e_cos (n, R) relative, bound_Tc, the path masks and the `excused` masks.  plain: reduced mode only -- which samples took the tables
    (from the reference where None)."""
    x = ref['x']
    n, R = ref['n'], len(ref['radii'])
    u = U
    EXP = 2.0 * EXP_ULPS
    oracle = bool(path.get('oracle'))
    tD = ORACLE_D_ERR if oracle else TABLE_D_ERR
    with np.errstate(all='ignore'):
        a1, a2 = ref['a1'].astype(f64), ref['a2'].astype(f64)
        c2PB = np.abs(ref['c2PB']).astype(f64)
        a1_un = ref['a1_un'].astype(f64)
        e_a1_un = u * (1.0 + 2.0 * c2PB / np.abs(a1_un))
        near_clip = np.abs(a1_un - HALF_PI) <= 2.0 * e_a1_un * HALF_PI
        e_a1 = np.where(ref['clipped'] & ~near_clip, 0.0, e_a1_un)
        e_a2 = e_a1 + u
        e_A1 = tD + 2.0 * e_a1 + 2.0 * u
        e_A2 = tD + 2.0 * e_a2 + u
        nn = ref['n_neutral']
        e_n = np.where(nn == 0, 0.0, (u * (2.0 * np.abs(ref['c4PB']) + np.abs(nn)) / np.abs(nn)).astype(f64))
        arg = ref['arg'].astype(f64)
        e_decay = np.abs(arg) * (2.0 * u + e_n[:, None]) + EXP * u
        e_base = 6.0 * u + e_decay + (2.0 * u if oracle else 0.0)
        dec = np.abs(ref['decay']).astype(f64)
        unit = np.abs(ref['unit']).astype(f64)
        b_jcex = SECOND * (unit * (dec * e_decay + 8.0 * u * np.abs(1.0 - dec)) + 4.0 * TINY)
        b_jcex = np.where(ref['j_cex'] == 0, np.where(arg == 0.0, 0.0, b_jcex), b_jcex)           # sigma = 0 or n = 0: 1 - exp(0) is exactly 0
        N, C = gauss_counts(path)
        t1, t2 = ref['t1'].astype(f64), ref['t2'].astype(f64)
        e_g1 = t1 * (2.0 * e_a1[:, None] + C * u) + N[None, :] * u
        e_g2 = t2 * (2.0 * e_a2[:, None] + C * u) + N[None, :] * u
        # a sample whose smallest value may be below the switch takes the literal evaluation in some chunk: the larger bound
        NL, CL = gauss_counts(PATH_RADII)
        lit = np.nanmin(np.where(np.isfinite(ref['j_min']), ref['j_min'], -1), axis=1).astype(f64) < 2.0 * SWITCH
        if path['gauss'] != 'literal':
            e_g1 = np.where(lit[:, None], np.maximum(e_g1, t1 * (2.0 * e_a1[:, None] + CL * u) + NL[None, :] * u), e_g1)
            e_g2 = np.where(lit[:, None], np.maximum(e_g2, t2 * (2.0 * e_a2[:, None] + CL * u) + NL[None, :] * u), e_g2)
        g1, g2 = ref['g1'].astype(f64), ref['g2'].astype(f64)
        A1, A2 = np.abs(ref['A1']).astype(f64), np.abs(ref['A2']).astype(f64)
        # the two terms of the shape with their relative errors, amplitudes without `base` (which cancels in cos_div)
        m1, m2 = A1[:, None] * g1, A2[:, None] * g2
        m1, m2 = np.where(A1[:, None] == 0, 0.0, m1), np.where(A2[:, None] == 0, 0.0, m2)
        extra = 4.0 * u if oracle else 2.0 * u          # (the oracle rounds base * A * g as two products, and the sum of the two beams)
        f_err = m1 * (e_A1[:, None] + u + e_g1 + extra) + m2 * (e_A2[:, None] + u + e_g2 + extra)          # (n, 91), per unit of base
        f_abs = m1 + m2
        tab = tables()
        base = np.abs(ref['base']).astype(f64)
        e_sum = {}
        for name, W in (('den', tab['SIMPSON_CDEN']), ('num', tab['SIMPSON_CNUM'])):
            # (the oracle forms w cos [sin] f with a product each instead of the folded weight: 4 u more per term)
            b = base * ((f_err + (N_SUM + (4.0 if oracle else 0.0)) * u * f_abs) @ np.abs(W))[:, None] + TINY * N_SUM * (base + 1.0 + 4.0 * (A1 + A2)[:, None])
            e_sum[name] = b / np.abs(ref[name]).astype(f64)
        # cos_div = sum_k CNUM_k f_k / sum_k CDEN_k f_k takes the SAME f_k in both sums: an error d_k of f_k moves the quotient by
        # (CNUM_k - cos_div CDEN_k) d_k / den, not by the sum of what it does to num and to den -- for a narrow beam, where every term
        # that matters has CNUM_k / CDEN_k next to cos_div, that is much less.  What the two sums do not share is their own rounding.
        cosr = ref['cos_div'].astype(f64)
        s_den, s_num = np.abs(ref['s_den']).astype(f64)[:, None], np.abs(ref['s_num']).astype(f64)[:, None]
        CD, CN = tab['SIMPSON_CDEN'], tab['SIMPSON_CNUM']
        shared = np.stack([(np.abs(CN[None, :] - cosr[:, r, None] * CD[None, :]) * f_err).sum(axis=1) for r in range(R)], axis=1) / s_den
        n_sum = (N_SUM + (4.0 if oracle else 0.0)) * u
        own = n_sum * ((f_abs @ np.abs(CD))[:, None] / s_den + (f_abs @ np.abs(CN))[:, None] / s_num) * np.abs(cosr)
        t_abs = TINY * N_SUM * (base + 1.0 + 4.0 * (A1 + A2)[:, None])          # (divided term by term: 1 / den overflows for a denormal den)
        tiny = (t_abs / np.abs(ref['den']).astype(f64) + t_abs / np.abs(ref['num']).astype(f64)) * np.abs(cosr)
        e_cos = np.where(e_sum['den'] < 0.5, SECOND * ((shared + own + tiny) / np.abs(cosr) + u) / (1.0 - e_sum['den']), np.inf)
        e_cos = np.where(np.isfinite(e_cos), e_cos, np.inf)
        near = np.zeros(n, bool)
        is_plain = np.zeros(n, bool)
        den_near_zero = e_sum['den'] >= 0.5
        if path['sums'] == 'table':
            qa = tables()['QA_MIN']
            X1, X2 = (ref['base'][:, 0] * ref['A1']).astype(f64), (ref['base'][:, 0] * ref['A2']).astype(f64)
            jc = ref['j_cex'][:, 0].astype(f64)
            ref_plain = ((np.abs(a1) >= qa) & (np.abs(a2) >= qa) & (X1 >= 0) & (X2 >= 0) & (jc > 0)
                         & ((np.fmax(X1, X2) >= 1e-280) | ((X1 == 0) & (X2 == 0))))
            for a, e in ((a1, e_a1), (a2, e_a2)):
                near |= np.abs(np.abs(a) - qa) <= SECOND * np.maximum(e, u) * qa          # (the width within its own error of the switch)
            near |= (np.abs(np.fmax(X1, X2) - 1e-280) <= 1e-282) | (np.abs(jc) <= b_jcex[:, 0])
            is_plain = ref_plain if plain is None else np.asarray(plain, bool)
            k1d, k1n, q1d, q1n = kappa_q(ref, 1)
            k2d, k2n, q2d, q2n = kappa_q(ref, 2)
            parts = []
            for kq1, kq2, Q1, Q2, E, tot in ((k1d, k2d, q1d, q2d, TABLE_QD_ERR, ref['s_den']), (k1n, k2n, q1n, q2n, TABLE_QN_ERR, ref['s_num'])):
                p1 = np.abs(ref['A1'] * Q1).astype(f64) * (e_A1 + u + E + kq1 * e_a1)
                p2 = np.abs(ref['A2'] * Q2).astype(f64) * (e_A2 + u + E + kq2 * e_a2 + u)
                parts.append(((p1 + p2) / np.abs(tot).astype(f64) + u))
            e_tab = np.where(parts[0] < 0.5, SECOND * (parts[0] + parts[1] + u) / (1.0 - parts[0]), np.inf)[:, None]
            e_tab = np.where(np.isfinite(e_tab), e_tab, np.inf)
            den_near_zero = np.where((is_plain & ~near)[:, None], (parts[0] >= 0.5)[:, None], np.where((~is_plain & ~near)[:, None], den_near_zero,
                                                                                                  den_near_zero | (parts[0] >= 0.5)[:, None]))
            e_cos = np.where((is_plain & ~near)[:, None], e_tab, np.where((~is_plain & ~near)[:, None], e_cos, np.fmax(e_tab, e_cos)))
        T = np.abs(ref['T']).astype(f64)[:, None]
        bT = ref['b_T'][:, None]
        bTc = SECOND * (np.abs(cosr) * bT + (T + bT) * np.abs(cosr) * e_cos + u * np.abs(ref['T_c']).astype(f64))
        # thresholds
        b_a1 = SECOND * 2.0 * u * c2PB           # the sum c2 PB + c3 keeps its sign when it rounds: only fl(c2 PB) can move a1 across 0
        e_ov1, e_ov2 = np.maximum(e_a1, u), np.maximum(e_a2, u)
        exc = {
            'a1_zero': (np.abs(a1_un) <= b_a1) & (b_a1 > 0.0),
            'overflow': (np.abs(np.abs(a1) - ALPHA_OVERFLOW) <= SECOND * e_ov1 * ALPHA_OVERFLOW) | (np.abs(np.abs(a2) - ALPHA_OVERFLOW) <= SECOND * e_ov2 * ALPHA_OVERFLOW),
            # (den within twice its bound of 0, and nothing else: a bound that is not finite for another reason is reported, not excused)
            'den_zero': np.isfinite(ref['den']) & np.isfinite(ref['num']) & den_near_zero,
            'pole': np.abs(np.abs(cosr) - 1.0) <= np.abs(cosr) * e_cos,
        }
        # double overflow: the real function exceeds the doubles (an amplitude from exp(+x) of a negative density): the answer is the
        # reference implementation's inf / NaN arithmetic, which the oracle defines; such a sample is held to the oracle's pattern
        big = np.fmax(np.abs(ref['base']) * np.fmax(A1, A2)[:, None], np.abs(ref['j_cex'])).astype(f64)
        overflowed = np.any(~(big < 1e300) & ~np.isnan(big), axis=1) | np.any(arg > 700.0, axis=1)
    return {'path': path, 'bound_V': ref['bound_V'], 'V_lo': ref['V_lo'], 'V_hi': ref['V_hi'], 'e_cos': e_cos, 'bound_Tc': bTc, 'excused': exc,
            'lit': lit, 'near': near, 'plain': is_plain, 'overflowed': overflowed, 'b_jcex': b_jcex, 'e_base': e_base, 'f_err': f_err, 'f_abs': f_abs,
            'e_a1': e_a1, 'e_a2': e_a2, 'e_sum': e_sum, 'e_g1': e_g1, 'e_g2': e_g2}


def j_bound(ref, bnd, r):
    """(j (n, 91) long double, its absolute bound (n, 91), sure_invalid, sure_valid) at radius index r: the bound on the sum of
    magnitudes; the sign of the profile decided term by term"""
    with np.errstate(all='ignore'):
        base = np.abs(ref['base'][:, r]).astype(f64)[:, None]
        j = ref['base'][:, None, r] * ref['shape'] + ref['j_cex'][:, None, r]
        # (absolute: a Gaussian in the denormal range is within EXP_ULPS units of 2^-1074, times its amplitude; a `base` in the denormal range
        # has rounded absolutely three times before the amplitudes A multiply it; the roundings of denormal products)
        amp = base[:, 0] * (np.abs(ref['A1']) + np.abs(ref['A2'])).astype(f64)
        b = (SECOND * (base * (bnd['f_err'] + bnd['e_base'][:, r, None] * bnd['f_abs']) + TINY * (2.0 * EXP_ULPS * amp + 4.0 * (np.abs(ref['A1']) + np.abs(ref['A2'])).astype(f64) + 8.0)[:, None]) + bnd['b_jcex'][:, r, None]
             + U * np.abs(j).astype(f64))
        # exact zeros stay exact zeros; and a Gaussian whose true value is below an eighth of the smallest denormal is exactly zero in
        # fp64 (the library exp is within 0.84 units of 2^-1074 there, profiles/f64_intrinsics_r01.txt; every chunk that deep is literal):
        # with j_cex exactly zero the profile then holds an exact zero, which plume.py:105 flags
        gone = lambda A, g, e: (A == 0)[:, None] | (8.0 * g.astype(f64) * (1.0 + e) < TINY)                 # noqa: E731
        zero = gone(ref['A1'], ref['g1'], bnd['e_g1']) & gone(ref['A2'], ref['g2'], bnd['e_g2']) & ((ref['j_cex'][:, r] == 0) & (ref['base'][:, r] != 0))[:, None]
        zero |= ((ref['base'][:, r] == 0) & (ref['j_cex'][:, r] == 0))[:, None] & np.isfinite(ref['shape'])
        sure_invalid = np.any((j + b < 0) | zero, axis=1)
        # ... and a Gaussian whose true value is above two denormals is a positive double; times an amplitude of at least 1, with no term
        # of the other sign, the entry is positive
        alive = lambda A, g, e: ((A * ref['base'][:, r]) >= 1)[:, None] & (g.astype(f64) * (1.0 - e) > 2.0 * TINY)            # noqa: E731
        same = ((ref['A1'] * ref['base'][:, r] >= 0) & (ref['A2'] * ref['base'][:, r] >= 0) & (ref['j_cex'][:, r] >= 0) & (bnd['b_jcex'][:, r] <= ref['j_cex'][:, r]))[:, None]
        positive = same & (alive(ref['A1'], ref['g1'], bnd['e_g1']) | alive(ref['A2'], ref['g2'], bnd['e_g2']))
        sure_valid = np.all((j - b > 0) | positive | np.isnan(j), axis=1)
    return j, b, sure_invalid, sure_valid


def flags(ref, bnd):
    """(certainly invalid, certainly valid) per sample over every radius; neither: the profile is within its bound of 0, excused"""
    inv = np.zeros(ref['n'], bool)
    val = np.ones(ref['n'], bool)
    for r in range(len(ref['radii'])):
        _, _, si, sv = j_bound(ref, bnd, r)
        inv |= si
        val &= sv
    a1 = ref['a1']
    ex = bnd['excused']['a1_zero'] | bnd['excused']['overflow']
    return (inv | (a1 <= 0)) & ~ex, val & (a1 > 0) & ~ex & ~inv


def check(got, ref, bnd, what='', mixed=False, oracle=None):
    """Hold `got` to the reference under the bound.  got: any of V_cc, I_B0, T, the other thruster outputs, j_ion (n, 91[, R]),
    div_angle, T_c (n[, R]), invalid.  Returns a report: per quantity `compared`, `excused`, `finite`, `ratio` (largest error / bound),
    `worst`; `failures`: (what, indices) -- empty when everything holds.  oracle: the oracle's results for the same inputs, which
    decide the inf / NaN pattern of the samples whose real value exceeds the doubles."""
    n, R = ref['n'], len(ref['radii'])
    exc = bnd['excused']
    fails = []
    rep = {'n': n, 'what': what, 'failures': fails}

    def fail(msg, mask):
        if np.any(mask):
            fails.append((msg, np.argwhere(mask)[:6].tolist()))

    def stats(name, fin, excused, err, bound):
        cmp_ = fin & ~excused
        fail(f'{name}: reference finite, bound not finite', cmp_ & ~np.isfinite(bound))
        with np.errstate(all='ignore'):
            ratio = np.where(cmp_, np.where(err == 0, 0.0, (err / bound).astype(f64)), 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        fail(f'{name}: outside the bound', ratio > 1.0)
        rep[name] = {'compared': int(cmp_.sum()), 'excused': int((fin & excused).sum()), 'finite': int(fin.sum()),
                     'ratio': float(np.max(ratio, initial=0.0)), 'worst': int(np.argmax(ratio)) if ratio.size else -1}

    ovf = bnd['overflowed']
    none = np.zeros(n, bool)
    with np.errstate(all='ignore'):
        if 'V_cc' in got:
            g = np.asarray(got['V_cc'], f64).astype(LD)
            w = ref['V_cc']
            fin = np.isfinite(w)
            stats('V_cc', fin, none, np.abs(g - w), bnd['bound_V'] + 0.0 * np.abs(w).astype(f64))
            fail('V_cc: outside the clamped interval', fin & ~((g >= bnd['V_lo']) & (g <= bnd['V_hi'])))
            fail('V_cc: NaN pattern', np.isnan(g) != np.isnan(w))
        for q in THRUSTER_OUT:
            if q in got:
                g, w = np.asarray(got[q], f64).astype(LD), ref[q]
                fin = np.isfinite(w)
                stats(q, fin, none, np.abs(g - w), ref['b_' + q])
                fail(f'{q}: inf / NaN pattern', (np.isnan(g) != np.isnan(w)) | (np.isinf(g) != np.isinf(w)))
        ex_s = exc['overflow'] | exc['a1_zero'] | ovf                      # per sample
        sure_inv, sure_val = flags(ref, bnd)
        ex_flag = ~(sure_inv | sure_val) | ovf
        if 'invalid' in got:
            gi = np.asarray(got['invalid'], bool)
            fail('invalid flag', ~ex_flag & (gi != sure_inv))
            rep['flags'] = {'compared': int((~ex_flag).sum()), 'excused': int(ex_flag.sum()), 'finite': n}
            if oracle is not None:
                fail('invalid flag against the oracle where the doubles overflow', ovf & (gi != np.asarray(oracle['invalid'], bool)))
        if 'j_ion' in got:
            gj = np.asarray(got['j_ion']).reshape(n, NANG, R)
            worst, nc, ne, nf, wi = 0.0, 0, 0, 0, -1
            for r in range(R):
                j, b, _, _ = j_bound(ref, bnd, r)
                g = gj[:, :, r].astype(LD)
                filled = np.all(gj[:, :, r] == (np.float32(1e-20) if mixed else 1e-20), axis=1)
                fail('j_ion: the 1e-20 fill of an invalid sample', ~ex_flag & (filled != sure_inv))
                if mixed:
                    b = b + 2.0 ** -24 * np.abs(j).astype(f64)
                fin = np.isfinite(j) & ~filled[:, None] & ~sure_inv[:, None]
                ex = (ex_s | (ex_flag & filled))[:, None] & fin
                cmp_ = fin & ~ex
                fail('j_ion: reference finite, bound not finite', cmp_ & ~np.isfinite(b))
                ratio = np.where(cmp_, np.where(g == j, 0.0, (np.abs(g - j) / b).astype(f64)), 0.0)
                ratio = np.where(np.isnan(ratio), np.inf, ratio)
                fail(f'j_ion: outside the bound (radius {r})', ratio > 1.0)
                fail(f'j_ion: NaN pattern (radius {r})', ~ex_s[:, None] & ~filled[:, None] & (np.isnan(g) != np.isnan(j)))
                if ratio.max(initial=0.0) > worst:
                    worst, wi = float(ratio.max()), int(np.argmax(ratio)) * R + r
                nc, ne, nf = nc + int(cmp_.sum()), ne + int(ex.sum()), nf + int(fin.sum())
                if oracle is not None and ovf.any():
                    oj = np.asarray(oracle['j_ion']).reshape(n, NANG, R)[:, :, r]
                    fail('j_ion: inf / NaN pattern against the oracle where the doubles overflow',
                         ovf[:, None] & ((np.isnan(gj[:, :, r]) != np.isnan(oj)) | (np.isinf(gj[:, :, r]) != np.isinf(oj))))
            rep['j_ion'] = {'compared': nc, 'excused': ne, 'finite': nf, 'ratio': worst, 'worst': wi}
        ex_cos = ex_s[:, None] | exc['den_zero']
        if 'T_c' in got:
            gt, wt = np.asarray(got['T_c'], f64).reshape(n, R).astype(LD), ref['T_c']
            fin = np.isfinite(wt)
            stats('T_c', fin, ex_cos, np.abs(gt - wt), bnd['bound_Tc'])
            fail('T_c: NaN pattern', ~ex_cos & (np.isnan(gt) != np.isnan(wt)))
        if 'div_angle' in got:
            gd, wd = np.asarray(got['div_angle'], f64).reshape(n, R), ref['div_angle'].astype(f64)
            cosr = ref['cos_div'].astype(f64)
            da = 2.0 * ACOS_ULPS * U * np.abs(wd) + TINY
            allowed = SECOND * (np.abs(cosr) * bnd['e_cos'] + np.abs(np.sin(wd)) * da + 0.5 * da * da)
            # |cos(got) - cos(want)| without cancellation; `want` to long double, so that the metric itself is exact to 2^-64
            wl, gl = ref['div_angle'], gd.astype(LD)
            err_cos = 2 * np.abs(np.sin((gl + wl) / 2) * np.sin((gl - wl) / 2))
            fin = np.isfinite(wd)
            at_pole = exc['pole']
            nan_ok = at_pole & np.isnan(gd)
            stats('cos_div', fin, ex_cos | nan_ok, np.where(np.isnan(gd), LD(np.inf), err_cos), allowed)
            rep['cos_div']['excused'] = int((fin & (ex_cos | at_pole)).sum())
            fail('div_angle: NaN pattern', ~ex_cos & ~at_pole & (np.isnan(gd) != np.isnan(wd)))
            if oracle is not None and ovf.any():
                od = np.asarray(oracle['div_angle'], f64).reshape(n, R)
                fail('div_angle: NaN pattern against the oracle where the doubles overflow', ovf[:, None] & (np.isnan(gd) != np.isnan(od)))
    rep['overflowed'] = int(ovf.sum())
    return rep


# pem_math.h's own log10 functions.  LOG10_TAB_ULPS = 1.4: the table log10 (csrc/pem_log_table.h), derived in tests/hp_math.py and held on
# the host by tests/test_log_table_host.py.  LOG10_SERIES_ULPS = 2.0: the series log10, which literal_sample takes; measured on the device
# with its v_rcp_f64 quotient by tools/microbench/pem_math_ulps.hip (profiles/pem_math_r01.txt) and held elementwise through the fused
# latent kernel by tests/test_math_kernels.py::test_series_log10_on_the_literal_path.
from hp_math import LOG10_SERIES_ULPS, LOG10_TAB_ULPS  # noqa: E402


def latent_reference(ref, bnd, basis, log10):
    """coupled_latent_kernel: lat_r = sum_k norm(j_k) B_kr by 91 fma.  Returns (lat (n, rank) long double, its absolute bound):
    the rounding count of the fma chain, 91 u, on sum_k |norm(j_k) B_kr|, plus what the error of each norm(j_k) contributes: b_j(k)
    for norm none; for log10 the ABSOLUTE error b_j / (|j_k| ln 10) + 2 LOG10 u max(|log10 j_k|, log10 2) -- the table log10 assembles
    its result from e log10(2) + T_i + r P(r), parts that are at least log10(2) in size unless e = 0, so near j = 1 its error is
    absolute; the series log10 of literal_sample has 2 ulp instead of the table's 1.4.  An invalid sample's row is fill * sum_k B_kr."""
    B = np.asarray(basis, f64)
    with np.errstate(all='ignore'):
        j, b, _, _ = j_bound(ref, bnd, 0)
        ulps = np.where(bnd['lit'], LOG10_SERIES_ULPS, LOG10_TAB_ULPS)[:, None]
        if log10:
            v = np.log10(j)
            bv = b / (np.abs(j).astype(f64) * math.log(10.0)) + 2.0 * ulps * U * np.maximum(np.abs(v).astype(f64), math.log10(2.0))
        else:
            v, bv = j, b
        lat = v @ B.astype(LD)
        bl = SECOND * (bv @ np.abs(B) + (NANG + 1.0) * U * (np.abs(v).astype(f64) @ np.abs(B)))
        fill = LD(-20.0) if log10 else LD(1e-20)
        col = np.abs(B).sum(axis=0)
        lat_fill = np.broadcast_to((fill * B.astype(LD).sum(axis=0))[None, :], lat.shape)
        b_fill = np.broadcast_to(((NANG + 2.0) * U * float(abs(fill)) * col)[None, :], lat.shape)
    return lat, bl, lat_fill, b_fill


def excused_share(rep):
    """the largest excused share among the quantities of a report"""
    return max((r['excused'] / max(r['finite'], 1) for q, r in rep.items() if isinstance(r, dict) and 'excused' in r), default=0.0)


def summary(rep):
    lines = [f'{rep["what"]}: {rep["n"]} samples, {rep["overflowed"]} past the doubles']
    for q, r in rep.items():
        if isinstance(r, dict) and 'compared' in r:
            lines.append(f'  {q:9s} compared {r["compared"]:9d}  excused {r["excused"]:6d} of {r["finite"]:9d}'
                         + (f'  worst error/bound {r["ratio"]:.3f} (entry {r["worst"]})' if 'ratio' in r else ''))
    for msg, idx in rep['failures']:
        lines.append(f'  FAIL {msg}: {idx}')
    return '\n'.join(lines)


# ---------------------------------------------------------------------------------------------------------------------------------
# the input sets of tests/test_hp_model_host.py and tests/test_model_kernels.py
# ---------------------------------------------------------------------------------------------------------------------------------
BASE = {'P_b': 1e-5, 'V_a': 300.0, 'T_e': 3.0, 'V_vac': 30.0, 'Pstar': 2e-5, 'P_T': 5e-5, 'mdot_a': 5e-6, 'a_1': 0.01,
        'c0': 0.5, 'c1': 0.5, 'c2': -8.0, 'c3': 0.3, 'c4': 1e20, 'c5': 1e16, 'sigma_cex': 55e-20}
SIZES = (1, 63, 64, 65, 64 * 4 + 37)          # one sample, around a tile, one workgroup of four tiles plus a ragged wave


def _columns(cols):
    """list of dicts of edits to BASE -> dict of arrays"""
    return {q: np.array([c.get(q, BASE[q]) for c in cols], dtype=f64) for q in COUPLED_INPUTS}


def take(x, idx):
    return {q: np.ascontiguousarray(v[idx]) for q, v in x.items()}


def prior_set(n=3000, seed=2):
    import sys
    if str(ROOT / 'tests') not in sys.path:
        sys.path.insert(0, str(ROOT / 'tests'))
    from _inputs import coupled_inputs
    return coupled_inputs(n, seed=seed)


def width_values():
    """beam widths on both sides of every table edge, one interior point per interval, the switches"""
    tab = tables()
    pts = [neighbours(0.25, 1), neighbours(tab['QA_MIN'], 1), np.array([1.63299, 0.184687])]
    for i in range(tab['NDI']):
        pts += [neighbours(1.0 / math.sqrt((i + 1) / 2.0), 1), np.array([1.0 / math.sqrt(i / 2.0 + 5.0 / 16.0)])]
    for j in range(tab['NQB']):
        pts += [neighbours(tab['QA_MIN'] + j / tab['QB_SCALE'], 1), np.array([tab['QA_MIN'] + (j + 3.0 / 8.0) / tab['QB_SCALE']])]
    return np.unique(np.concatenate(pts))


def widths_set():
    """c2 = 0: a1 = c3 exactly.  a1 = a2 (c1 = 1) over every table edge up to the clip at pi/2, with c0 in {0, 1, 0.5} and sigma_cex = 0
    or the prior's; a2 = a1 / c1 beyond pi/2 up to 53.28 from a1 = 1.5.  With c0 = 0 and sigma_cex = 0, j_ion[0] = I_B0 / (r^2 D(a1)):
    the device's normaliser seen through three roundings."""
    a = width_values()
    a = a[a <= HALF_PI]
    cols = []
    for c0, sigmas in ((0.0, (0.0, 55e-20)), (1.0, (0.0,)), (0.5, (55e-20,))):
        for s in sigmas:
            # (without j_cex a beam below 0.0575 underflows to an exact zero at 90 degrees, an invalid sample: the tail set's business)
            cols += [dict(c2=0.0, c1=1.0, c3=float(v), c0=c0, sigma_cex=s if v >= 0.07 else 55e-20) for v in a]
            cols += [dict(c2=0.0, c1=1.0, c3=float(v), c0=c0, sigma_cex=s) for v in list(neighbours(HALF_PI, 1)) + [2.0]]        # the clip
    wide = np.concatenate([1.0 / np.sqrt(np.array([0.49, 0.45, 0.3, 0.2, 0.1, 0.05, 0.01, 1e-3])), [2.0, 5.0, 20.0, 50.0, 53.0, 53.28]])
    for c0, s in ((1.0, 0.0), (0.5, 55e-20)):
        cols += [dict(c2=0.0, c3=1.5, c1=1.5 / float(v), c0=c0, sigma_cex=s) for v in wide]
    return _columns(cols)


def tail_set():
    """narrow beams with j_cex exactly zero (sigma_cex = 0): the smallest j_ion on both sides of the 1e-290 switch (a = 0.0607), deep
    in the recurrence's tail above it and on the literal path below it; widths around QA_MIN and below it down to 1e-3 (the tail
    underflows to an exact zero: invalid); amplitudes that leave the doubles at either end"""
    cols = [dict(c2=0.0, c1=1.0, c3=float(v), sigma_cex=0.0) for v in np.linspace(0.0578, 0.0660, 300)]
    cols += [dict(c2=0.0, c1=1.0, c3=float(v), sigma_cex=0.0, c0=c0) for v in np.linspace(0.0585, 0.075, 60) for c0 in (0.0, 1.0)]
    cols += [dict(c2=0.0, c1=0.5, c3=float(v), sigma_cex=0.0) for v in np.linspace(0.0291, 0.0340, 120)]                  # a2 = 2 a1 around the switch, a1 around QA_MIN
    cols += [dict(c2=0.0, c1=1.0, c3=float(v), c4=0.0, c5=0.0) for v in np.linspace(0.0580, 0.0640, 60)]                  # j_cex = 0 through n = 0
    cols += [dict(c2=0.0, c1=1.0, c3=float(v), sigma_cex=0.0) for v in (0.05, 0.04, 0.031, 0.0300001, 0.03, 0.0299999, 0.02, 0.01, 0.0044, 0.003, 0.001)]
    cols += [dict(c2=0.0, c1=0.25, c3=float(v), sigma_cex=0.0) for v in (0.0299, 0.02, 0.01, 0.0044, 0.002)]
    cols += [dict(c2=0.0, c1=1.0, c3=float(v)) for v in (0.0299, 0.02, 0.0044, 0.003)]                                     # ... with the prior's j_cex: valid, reduced mode takes the loop
    cols += [dict(c5=1.3e21), dict(c5=1.29e21, c3=0.2), dict(mdot_a=1e-318), dict(mdot_a=3e-320, sigma_cex=0.0), dict(mdot_a=5e-324, c3=0.1)]     # denormal amplitudes
    cols += [dict(c5=-1.4e21), dict(c5=-1.3e21, c3=0.06, c2=0.0, c1=1.0), dict(c4=-1.5e23, c5=0.0)]                      # exp(+x) past the doubles
    return _columns(cols)


def cancellation_set(n=1500, seed=7):
    """c0 in [-0.2, 1.2] (amplitudes of opposite sign) and negative c4 (j_cex < 0, decay > 1), finite results"""
    x = prior_set(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    x['c0'] = rng.uniform(-0.2, 1.2, n)
    x['c4'] = -(10.0 ** rng.uniform(18.0, 21.0, n))
    return x


SETS = {'priors': prior_set, 'widths': widths_set, 'tail': tail_set, 'cancellation': cancellation_set}
CAPS = {'priors': 0.0, 'widths': 0.0, 'tail': 0.02, 'cancellation': 0.02}
