"""The single-precision kernels held to the fp64 CPU oracle SAMPLE BY SAMPLE under the derived bound of tests/hp_fp32.py:
`pem_coupled_f32_dev` (csrc/pem_fp32.hip) on the prior design, the fuzz tool's wild inputs, an edge list and a sweep over every table
interval; its dispatch space; and `Model32` inside the fused Saltelli launch (`pem_saltelli_f32_dev`), read back sample by sample
through point-mass designs and required BIT-EQUAL to the explicit-input kernel.  tests/test_fp32_host.py checks the same reference,
bound and sets on the numpy restatement without a GPU.

Against the restatement: the same NaN pattern and flag wherever the oracle comparison excuses a sample, and values within TWICE the
bound WITHOUT its table term (both read the same header).  The count: the two evaluate the same operations and differ at first by the
intrinsics' roundings only (rcp, sqrt, __expf, __logf, acosf), but once an intermediate differs by an ulp every later operation rounds
two different numbers, so each operation of the bound's count contributes its u once per side.  In general that is no tighter than the
bound against the oracle, which is already a count of a few dozen roundings with measured errors at a tenth of it.  Where it IS tight
it is asserted: narrow beams with c2 = 0, c1 = 1, c0 = 0 use no intrinsic inside functionals32, and cos_div of kernel and restatement
agree within 9 u there (test_coupled_f32_narrow_beams_against_the_restatement).  What is observed elsewhere is printed.

Figures measured on an MI355X (this file prints them; run with -s):
  inside the priors (3 seeds): compared 100 %, excused 0; worst error / bound V_cc 0.95, T_c 0.12, cos_div 0.11; median bound / |value|
    V_cc 1.3e-7, T_c 3.6e-6, cos_div 3.0e-6 (required: <= 1e-5)
  wild (9 seeds x 20 000): worst error / bound V_cc 0.99, T_c 0.30, cos_div 0.10; excused by a threshold rule, every rule counted: T_c 0.29 %,
    cos_div 1.74 % of the finite reference values, the flag 1.81 % of the samples (required: <= 2 %); the 4 % of the samples whose decay has
    underflowed in float are held to the model's defined answer there (hp_fp32.check)
  edges 189 points, table sweep 5146 points: worst error / bound 0.14 / 0.08
  against the restatement: V_cc 98 % bit-equal, T_c 66 %, div_angle 55 % inside the priors; T_c within 11 ulp there

Mutations of csrc (each built apart, this file and tests/test_fp32.py run against it); "old" = tests/test_fp32.py caught it:
   5 functionals32 `last` = NQB - 2 ............ NOT CAUGHT, old no.  Row 62 extrapolated over the last narrow interval moves Qd by 1 ulp on
     6 % of that interval's floats and Qn by 1 ulp on 62 %, staying 1.7 - 2.1 u32 from the truth: below the table's own 3.6 u32, so no
     reference can see it; only bit-equality with a restatement of the SAME intrinsics could, and the hardware's rcp / exp bits are not
     restated
   6 normaliser32 x off-centre ................. priors, wild, edges, radius, dispatch, Model32; old yes
   7 V > V_a clamp removed ..................... wild, edges, radius, dispatch, Model32; old no
   8 j_cex > 0 dropped from `plain` ............ wild, edges (invalid flag of the sigma = 0 points), radius, dispatch, Model32; old no
   9 u2 = rcp(a2 * a1) ......................... priors, wild, edges, radius, dispatch, Model32; old yes
  10 loop bound n - 1 .......................... every test that launches (a sentinel is left); old yes.   stride x 2: dispatch; old yes
  11 Model32 k: double multiply then rounding .. NOT CAUGHT, and cannot be: pem_saltelli_f32_dev takes torr2pa as a float, the product of
     two floats is exact in double, so rounding it once gives the float product bit for bit -- the mutant is equivalent
  12 ld < n check removed ...................... test_coupled_f32_argument_errors; old no
Mutations 1 - 4 of csrc/pem_tables_f32.h fail tests/test_fp32_host.py (1 and 3 through test_header_is_what_the_generator_writes only: a
DPOLY coefficient off by 1e-4 and the last Dawson coefficient are below the tables' rounding error; 2 and 4 through the tables against
the oracle and the bound as well)."""
import ctypes as C

import numpy as np
import pytest

import hp_fp32 as hp

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
N_PRIOR = 100_000
N_STRIDE = 2048 * 256          # the grid of coupled_f32_kernel is capped at 2048 workgroups of 256: 524 288 samples per trip


def _k():
    from hallthrusterpem_amd import constants
    return np.float32(constants.TORR_2_PA)


def _launch(x32, radius=1.0, ld=None, ldq=None, with_invalid=True, n=None):
    """pem_coupled_f32_dev on (15, n) float32 inputs.  Buffers of leading dimension ld / ldq, pre-filled with a sentinel.  Returns
    (rc, qoi (3, ldq) float32, invalid (ldq,) uint8 or None) as numpy arrays."""
    import torch
    from hallthrusterpem_amd import _lib
    lib = _lib.load()
    _lib.require_device()
    m = x32.shape[1]
    n = m if n is None else n
    ld = m if ld is None else ld
    ldq = m if ldq is None else ldq
    xin = torch.full((15, max(ld, 1)), SENTINEL, dtype=torch.float32, device='cuda')
    xin[:, :m] = torch.from_numpy(np.ascontiguousarray(x32))
    qoi = torch.full((3, max(ldq, 1)), SENTINEL, dtype=torch.float32, device='cuda')
    inv = torch.full((max(ldq, 1),), 0xAB, dtype=torch.uint8, device='cuda')
    s = torch.cuda.current_stream()
    rc = lib.pem_coupled_f32_dev(n, float(_k()), float(radius), C.c_void_p(xin.data_ptr()), ld, C.c_void_p(qoi.data_ptr()), ldq,
                                 C.c_void_p(inv.data_ptr()) if with_invalid else None, C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    return rc, qoi.cpu().numpy(), inv.cpu().numpy()


def _got(qoi, inv, n):
    return {'V_cc': qoi[0, :n], 'div_angle': qoi[1, :n], 'T_c': qoi[2, :n], 'invalid': inv[:n].astype(bool)}


def _ulps(g, w):
    """difference in float ulps of w; 0 where both are NaN or equal"""
    g, w = np.asarray(g, np.float32), np.asarray(w, np.float32)
    with np.errstate(all='ignore'):
        d = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
    same = (g == w) | (np.isnan(g) & np.isnan(w))
    return np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))


def _against_restatement(got, res, ref, what):
    """The kernel against the numpy restatement: same flags and NaN pattern away from the thresholds, values within twice the bound
    without its table term, centred on the restatement."""
    bnd = hp.bounds(ref, res, table_err=False)
    bnd = dict(bnd, **{q: 2.0 * bnd[q] for q in ('bound_V', 'bound_T', 'bound_Tc', 'e_cos')})
    with np.errstate(all='ignore'):
        pseudo = dict(ref, V_cc=res['V_cc'].astype(np.float64), T_c=res['T_c'].astype(np.float64), div_angle=res['div_angle'].astype(np.float64),
                      cos_div=res['cos_div'].astype(np.float64), invalid=res['invalid'])
        bnd = dict(bnd, V_lo=pseudo['V_cc'] - bnd['bound_V'], V_hi=pseudo['V_cc'] + bnd['bound_V'])
    rep = hp.check(got, pseudo, bnd)
    line = f'  against the restatement ({what}):'
    for q, key in (('V_cc', 'V_cc'), ('div_angle', 'div_angle'), ('T_c', 'T_c')):
        ul = _ulps(got[key], res[key])
        fin = np.isfinite(ul)
        line += f'  {q}: {100.0 * np.mean(ul == 0):.1f} % bit-equal, worst {np.max(ul[fin], initial=0.0):.0f} ulp;'
    print(line)
    assert rep['failures'] == [], (what, rep['failures'])
    return rep


def _hold(x32, what, radius=1.0, restatement=True):
    k = _k()
    rc, qoi, inv = _launch(x32, radius=radius)
    assert rc == 0
    got = _got(qoi, inv, x32.shape[1])
    ref = hp.reference(x32, k, radius)
    res = hp.restate(x32, k, radius)
    bnd = hp.bounds(ref, res)
    rep = hp.check(got, ref, bnd, res)
    print('\n' + hp.summary(rep, what))
    assert rep['failures'] == [], (what, rep['failures'])
    for q in hp.QOI:
        assert rep[q]['ratio'] <= 1.0
    if restatement:
        _against_restatement(got, res, ref, what)
    return got, ref, res, bnd, rep


def test_coupled_f32_against_the_oracle_inside_the_priors():
    """1e5 samples of the prior design from each of three seeds (2e5 in the host test: fewer here, so that this file runs within twice the
    time of tests/test_fp32.py + tests/test_saltelli_model.py), uploaded as floats: every sample compared, none excused, each inside its
    bound; median bound / |value| <= 1e-5.  Measured: worst error / bound V_cc 0.95, T_c 0.12, cos_div 0.11."""
    for seed in hp.PRIOR_SEEDS:
        got, ref, res, bnd, rep = _hold(hp.prior_set(seed, N_PRIOR), f'priors, seed {seed}')
        for q in hp.QOI:
            assert rep[q]['compared'] == N_PRIOR and rep[q]['excused'] == 0, (seed, q, rep[q])
            assert rep[q]['median_rel_bound'] <= 1e-5
        assert rep['flags']['excused'] == 0


def test_coupled_f32_against_the_oracle_on_wild_inputs():
    """The fuzz tool's wild inputs, 20 000 per seed: inside the bound wherever compared; of the finite reference values of T_c and div_angle
    and of the flags of all samples at most 2 % excused, every rule counted; where excused, the restatement's NaN pattern and flag."""
    tot = {q: [0, 0] for q in ('T_c', 'cos_div', 'flags')}
    for seed in hp.WILD_SEEDS:
        got, ref, res, bnd, rep = _hold(hp.wild_set(seed), f'wild, seed {seed}')
        for q in ('T_c', 'cos_div'):
            tot[q][0] += rep[q]['finite']
            tot[q][1] += rep[q]['excused']
        tot['flags'][0] += rep['n']
        tot['flags'][1] += rep['flags']['excused']
        assert rep['V_cc']['excused'] == 0
    for q, (fin, exc) in tot.items():
        print(f'{q}: {exc} of {fin} excused by a threshold rule ({100.0 * exc / fin:.2f} %)')
        assert exc <= 0.02 * fin, (q, exc, fin)


def test_coupled_f32_at_the_edges_and_over_every_table_interval():
    """The edge list (every term of `plain` either side of its threshold, both clamps of V_cc, the clip of a1, a2 = inf, a1 = 0, the overflow
    bound, NaN / inf in each input) and beam widths over each of the 32 + 64 table intervals with the floats around every knot."""
    _hold(hp.edge_set(_k()), 'edges')
    x = hp.sweep_set()
    got, ref, res, bnd, rep = _hold(x, 'every table interval')
    assert rep['T_c']['excused'] == 0


def test_coupled_f32_at_the_overflow_bound_itself():
    """|a2| exactly the float above 53.28349511409265 (c2 = 0, c3 = that float / 64, c1 = 2^-6: the reciprocal of a power of two and the
    product by 64 are exact): the oracle's bracket is NaN there and so are div_angle and T_c, with no excuse; one float below they are finite."""
    hi = hp.F_ALPHA_OVERFLOW
    lo = np.nextafter(hi, np.float32(0))
    assert float(hi) > hp.ALPHA_OVERFLOW >= float(lo)
    x = np.repeat(hp.edge_set(_k())[:, :1], 4, axis=1)
    x[10], x[9] = 0.0, np.float32(2.0 ** -6)
    x[11] = np.array([hi, lo, -hi, -lo], np.float32) / np.float32(64.0)
    rc, qoi, inv = _launch(x)
    assert rc == 0
    ref = hp.reference(x, _k())
    assert np.array_equal(ref['a2'], np.array([hi, lo, -hi, -lo], np.float64) ) and np.array_equal(np.isnan(ref['T_c']), [True, False, True, False])
    assert np.array_equal(np.isnan(qoi[1, :4]), [True, False, True, False]) and np.array_equal(np.isnan(qoi[2, :4]), [True, False, True, False])
    assert np.array_equal(inv[:4].astype(bool), ref['invalid'])


def test_coupled_f32_narrow_beams_against_the_restatement():
    """Narrow beams with c2 = 0, c1 = 1, c0 = 0: a1 = a2 = c3 exactly, X2 = 0, and functionals32 reads |a| alone (no rcp, no exp), so kernel and
    restatement compute the same Qd, Qn bit for bit.  cos_div = fl(X1 Qn) rcp(fl(X1 Qd)): X1 differs between the two by its intrinsics'
    roundings but is common to both products, each of which is then rounded once per side (2 u each), rcp is 1 ulp against half an ulp
    (3 u), the last product 2 u: 9 u in all.  Judged through div_angle = acosf(cos_div) with acosf's 1.5 + 0.5 ulp on top."""
    tab = hp.tables32()
    a = hp.table_points(40)
    a = a[(a >= tab['QA_MIN']) & (a < np.float32(0.25))]
    x = np.repeat(hp.edge_set(_k())[:, :1], a.size, axis=1)
    x[10], x[9], x[8], x[11] = 0.0, 1.0, 0.0, a
    rc, qoi, inv = _launch(x)
    assert rc == 0
    res = hp.restate(x, _k())
    assert res['plain'].all() and not res['invalid'].any() and not inv[:a.size].any() and a.size > 64 * 40
    g, w = qoi[1, :a.size].astype(np.float64), res['div_angle'].astype(np.float64)
    cosw = res['cos_div'].astype(np.float64)
    da = 2.0 * (hp.ACOS_ULPS + 0.5) * hp.U32 * np.abs(w)
    allowed = hp.SECOND * (9.0 * hp.U32 * np.abs(cosw) + np.abs(np.sin(w)) * da + 0.5 * da * da)
    err = 2.0 * np.abs(np.sin(0.5 * (g + w)) * np.sin(0.5 * (g - w)))
    print(f'\n{a.size} narrow beams: worst |cos(div) - cos(div of the restatement)| / allowed = {np.max(err / allowed):.3f}, '
          f'{100.0 * np.mean(qoi[1, :a.size] == res["div_angle"]):.1f} % of div_angle bit-equal')
    assert np.all(err <= allowed), np.flatnonzero(err > allowed)[:10]


def test_coupled_f32_radius():
    """radius 0.5 and 2: the amplitudes scale by 1 / r^2 and the decay exponent by r; cos_div, T_c, V_cc stay inside the same bound."""
    x = hp.prior_set(5, 20_000)
    xe = hp.edge_set(_k())
    for radius in (0.5, 2.0):
        got, ref, res, bnd, rep = _hold(x, f'priors, radius {radius}', radius=radius)
        # (at r = 2 the decay exponent r n sigma of the prior box reaches 154: 0.2 % of the samples underflow in float, the flags may change)
        assert rep['T_c']['excused'] <= (0 if radius < 1.0 else int((bnd['excused']['range'] & (ref['arg'] >= -88.5)).sum()))
        _hold(xe, f'edges, radius {radius}', radius=radius)


def test_coupled_f32_dispatch_space():
    """n = 1, 63, 255, 256, 257, 524 288, 524 289 and 3 * 524 288 + 17 (three trips of the grid-stride loop and a ragged tail): EVERY sample
    written and checked (the outputs are pre-filled with a sentinel), the same bits for the same sample wherever it sits in whatever batch;
    ld, ldq > n with the padding left alone; invalid = NULL; n = 0 touches nothing.  The values are checked where the samples are first
    evaluated (against the oracle and the restatement); the large batches are compared with those bits."""
    n_big = 3 * N_STRIDE + 17
    # 100 003 samples (not a multiple of the workgroup, so a sample meets every lane), a fifth of them from outside the priors so that flags
    # and the literal path occur in every stretch of the stride loop: held to the oracle and the restatement in a launch of their own,
    # then tiled over the large batch, where every sample must give the bits it gave there
    m = 100_003
    xs = hp.prior_set(3, m)
    w = hp.wild_set(7, 40_000)
    w = w[:, np.isfinite(w).all(axis=0)]
    pos = np.arange(0, m, 5)
    xs[:, pos] = w[:, np.arange(pos.size) % w.shape[1]]
    small, _, _, _, rep = _hold(xs, f'the {m} samples of the dispatch test')
    assert rep['flags']['compared'] > 0.9 * m and small['invalid'].sum() > 100
    x = np.ascontiguousarray(xs[:, np.arange(n_big) % m])
    rc, qoi, inv = _launch(x)
    assert rc == 0
    assert not np.any(qoi == np.float32(SENTINEL)) and not np.any(inv == 0xAB), 'a sample was never written'
    tile = np.arange(n_big) % m
    for i, key in enumerate(('V_cc', 'div_angle', 'T_c')):
        assert np.array_equal(qoi[i].view(np.uint32), np.ascontiguousarray(small[key][tile]).view(np.uint32)), key
    assert np.array_equal(inv.astype(bool), small['invalid'][tile])
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)                       # noqa: E731
    for n in (1, 63, 255, 256, 257, N_STRIDE, N_STRIDE + 1):
        for off in (0, n_big - n):                                                 # the first n samples and the last n
            xs = np.ascontiguousarray(x[:, off:off + n])
            rc, q, iv = _launch(xs, ld=n + 37, ldq=n + 101)
            assert rc == 0
            assert np.array_equal(bits(q[:, :n]), bits(qoi[:, off:off + n])), (n, off)
            assert np.array_equal(iv[:n], inv[off:off + n]), (n, off)
            assert np.all(q[:, n:] == np.float32(SENTINEL)) and np.all(iv[n:] == 0xAB), (n, off, 'padding written')
        rc, q2, iv2 = _launch(xs, with_invalid=False)
        assert rc == 0 and np.array_equal(bits(q2), bits(q[:, :n])) and np.all(iv2 == 0xAB), (n, 'invalid = NULL')
    rc, q, iv = _launch(x[:, :64], n=0)
    assert rc == 0 and np.all(q == np.float32(SENTINEL)) and np.all(iv == 0xAB)


def test_coupled_f32_argument_errors():
    """NULL arrays and leading dimensions smaller than n are refused with PEM_ERR_INVALID_ARG before anything is launched (n = 8 with
    buffers of 1024 floats per row: nothing here could reach past a buffer even if a check were missing); n = 0 is PEM_OK."""
    import torch
    from hallthrusterpem_amd import _lib
    lib = _lib.load()
    _lib.require_device()
    xin = torch.zeros((15, 1024), dtype=torch.float32, device='cuda')
    qoi = torch.full((3, 1024), SENTINEL, dtype=torch.float32, device='cuda')
    inv = torch.zeros(1024, dtype=torch.uint8, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                          # noqa: E731
    call = lambda n, x, ld, q, ldq: lib.pem_coupled_f32_dev(n, float(_k()), 1.0, x, ld, q, ldq, p(inv), s)      # noqa: E731
    assert call(8, None, 1024, p(qoi), 1024) == _lib.PEM_ERR_INVALID_ARG
    assert call(8, p(xin), 1024, None, 1024) == _lib.PEM_ERR_INVALID_ARG
    assert call(8, p(xin), 7, p(qoi), 1024) == _lib.PEM_ERR_INVALID_ARG
    assert call(8, p(xin), 1024, p(qoi), 7) == _lib.PEM_ERR_INVALID_ARG
    assert call(8, p(xin), 0, p(qoi), 0) == _lib.PEM_ERR_INVALID_ARG
    assert b'pem_coupled_f32' in lib.pem_last_error()
    assert call(0, None, 0, None, 0) == _lib.PEM_OK
    torch.cuda.synchronize()
    assert bool((qoi == SENTINEL).all())
    assert call(8, p(xin), 8, p(qoi), 8) == _lib.PEM_OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# Model32 inside the fused Saltelli launch, sample by sample (the point-mass method of tests/test_saltelli_model.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _point_sums32(points):
    import torch
    from hallthrusterpem_amd import sampling
    from hallthrusterpem_amd.fp32 import saltelli_sums
    from test_saltelli_model import VARIED, _names
    design = sampling.Design(priors={q: sampling.Prior(sampling.UNIFORM, 0.0, 0.0, 'point') for q in _names()}, seed=7, stream=3)
    sums, flags = [], []
    for v in points:
        design.a[:] = v
        design.b[:] = v
        s, f = saltelli_sums(design, VARIED, n_base=1, n_blocks=1, precision='fp32')
        sums.append(s)
        flags.append(f)
    torch.cuda.synchronize()
    return torch.stack(sums).cpu().numpy(), torch.stack(flags).cpu().numpy()


def _saltelli_points(points, what):
    import torch
    from test_saltelli_model import VARIED, _designed_values
    k = _k()
    nev = len(VARIED) + 2
    sums, flags = _point_sums32(points)
    xv = _designed_values(points)                                         # what the design holds, in double
    with np.errstate(over='ignore'):
        x32 = np.ascontiguousarray(torch.from_numpy(xv).to(torch.float32).numpy().T)      # the device rounds to nearest, as torch does
    assert np.array_equal(x32.view(np.uint32), hp.as_f32_inputs(xv.T).view(np.uint32))
    rc, qoi, inv = _launch(x32)
    assert rc == 0
    want = qoi[:, :len(points)].T.astype(np.float64)                      # (m, 3) V_cc, div_angle, T_c of the explicit-input kernel
    f = sums[:, 0, :] / 2.0                                               # row 0 = fA + fB = 2 f, exact
    assert np.array_equal(f, want, equal_nan=True), (what, np.flatnonzero(~np.all((f == want) | (np.isnan(f) & np.isnan(want)), axis=1))[:10])
    # (the sign of a zero cannot be read from a sum that starts at +0)
    fin = np.isfinite(f)
    with np.errstate(over='ignore', invalid='ignore'):
        sq = 2.0 * (f * f)                                                # floats squared and added in double: exact
    assert np.array_equal(sums[:, 1, :][fin], sq[fin]), what
    assert np.array_equal(np.isnan(sums[:, 1, :]), np.isnan(f)), what
    for r in (2, 3):
        assert np.all(sums[:, r, :][fin] == 0.0) and np.all(np.isnan(sums[:, r, :][~fin])), (what, r)
    assert np.all(np.isin(flags, (0, nev))), what
    # the two counters: the explicit kernel's flag, and both against the oracle's predicates away from their thresholds
    assert np.array_equal(flags[:, 1] == nev, inv[:len(points)].astype(bool)), what
    ref = hp.reference(x32, k)
    res = hp.restate(x32, k)
    bnd = hp.bounds(ref, res)
    # (the invalid counter is the explicit kernel's flag, which check() holds to the oracle, the defined answers and the restatement)
    rep = hp.check(_got(qoi, inv, len(points)), ref, bnd, res)
    assert rep['failures'] == [], (what, rep['failures'])
    ex_flag = rep['ex_flag']
    with np.errstate(invalid='ignore'):
        nonphys = (ref['T'] < 0.0) | (ref['I_B0'] < 0.0)
        near = np.abs(ref['T']) <= bnd['bound_T']                          # T = -0 in float, a tiny negative number in double
    assert np.array_equal((flags[:, 0] == nev)[~near], nonphys[~near]), what
    return int((~res['plain']).sum()), int(ex_flag.sum())


def test_model32_in_the_fused_saltelli_launch_is_the_explicit_kernel_bit_for_bit():
    """About 2 000 finite wild points and the edge list, one fused fp32 launch each: f read back from row 0 equals pem_coupled_f32_dev on
    the float-rounded point bit for bit (the header of coupled_f32 says "the same bits"); rows 1-3 have the structure of a point mass;
    the two flag counters are the oracle's predicates; the design's double -> float conversion rounds to nearest."""
    from test_saltelli_model import _wild_points
    pts = _wild_points()
    n_lit, n_ex = _saltelli_points(pts, 'wild')
    print(f'\nModel32 on {len(pts)} wild points: {n_lit} took the literal sums, {n_ex} flags near a threshold')
    assert 200 <= n_lit <= len(pts) - 200
    edges = hp.edge_set(_k()).astype(np.float64).T
    n_lit, n_ex = _saltelli_points(np.ascontiguousarray(edges), 'edges')
    assert n_lit >= 40
