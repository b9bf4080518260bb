"""`pem_sobol_sweep_f64_dev` (csrc/pem_sobol_sweep.hip) called directly, with tables of its own, and held to the CPU oracle SAMPLE BY
SAMPLE: the branches the PEM-v0 priors never take (the whole-grid spike and positivity test `literal_j`, invalid plume samples,
the rejection loop at its end, non-physical thruster results), the launch itself (dead lanes, workgroups without a live sample, the
per-workgroup partial layout, first_index, one pressure or many, the clip) and the values behind the sums.  The inputs, the oracle
values and the bounds are tests/sobol_sweep_cases.py's; tests/test_sobol_sweep_host.py checks without a GPU that they reach
every branch and keep clear of every threshold.

Part 1, point masses.  A table of point masses U(v, v) makes rows A, B and every AB row the point v, so with n_base = 1 a launch of
m "pressures" evaluates m points: row 0 = 2 f, row 1 = 2 f^2, every other row 0 (NaN where f is not finite), every flag 0 or nv + 2,
and with max_attempts = 1 the Plume group reports rejected = unaccepted = 2 exactly when the point's profile reaches the spike.

Parts 2 - 4, designs on rough priors.  Per value the kernel is held to e = TOL |f| + slack (tests/parity_rules.py: slack = the j_ion
slack of the oracle's term decomposition; TAU times the three terms of V_cc; nothing for T and u_ion).  A clipped value is the
threshold itself, e = 0: the threshold lies between two order statistics of the oracle that are further apart than any e.  The
sums are compared per workgroup -- sample i belongs to workgroup (i mod (256 n_blocks)) // 256 -- with long-double sums:

  rows 0, 1 (sum of fA + fB, fA^2 + fB^2) against the device's own pre-pass values min(j0, clip): only rounding separates them,
      |got - want| <= gamma_k sum |terms|,  gamma_k = k u / (1 - k u),  u = 2^-53,  k = addends + 16
      (k - 1 additions in any order and the few roundings of a term itself);
  rows 2 + 4 j + w against the oracle's clipped values.  With |dfA| <= eA, |dfB| <= eB, |dfAB| <= eAB and D = fAB - fA, to first order
      t1 = fB D        |dt1|   <= eB |D| + |fB| (eAB + eA)
      t1^2             |dt1^2| <= 2 |t1| |dt1|
      t2 = D^2         |dt2|   <= 2 |D| (eAB + eA)
      t2^2             |dt2^2| <= 2 t2 |dt2|
      and a sum is held to 1.01 (sum of these + gamma_k sum |terms|).  The dropped terms are of second order in e: e / |f| <= 1e-10
      makes them 1e-10 of the bound; where cancellation makes e / |f| larger the host test checks that they stay below the 1 %.
      Where every term of a row is an exact zero (u_ion does not depend on mdot_a) the bound is zero and so must the sum be.
The non-Plume groups have no pre-pass: their rows 0 and 1 are held to the oracle like the others (|d(fA + fB)| <= eA + eB,
|d(fA^2 + fB^2)| <= 2 |fA| eA + 2 |fB| eB)."""
import ctypes as C

import numpy as np
import pytest

import sobol_sweep_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = 1.2345e300            # what the output buffers hold before a launch: no result can be this
L = np.longdouble


def _nv(group):
    return len(sc.varied_cols(group))


def _launch(group, tables, n_base, *, first=0, seed=sc.ROUGH_SEED, spike=np.inf, max_attempts=1, clip=None, prepass=False, n_blocks=1):
    """One call of pem_sobol_sweep_f64_dev on buffers filled with SENTINEL (flags: -1).  Returns dict(partial
    (n_p, n_blocks, rows, nq), flags (n_p, n_blocks, 4), j0 (n_p, 2, n_base) or None) as numpy arrays."""
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd import sobol as study
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    kind, a, b = (torch.as_tensor(np.ascontiguousarray(t), device=dev) for t in tables)
    assert kind.dtype == torch.int32 and a.dtype == b.dtype == torch.float64 and kind.shape == a.shape == b.shape and kind.shape[1] == 15
    n_p = kind.shape[0]
    rows = 2 + 4 * _nv(group)
    partial = torch.full((n_p, n_blocks, rows, sc.NQ[group]), SENTINEL, dtype=torch.float64, device=dev)
    flags = torch.full((n_p, n_blocks, 4), -1, dtype=torch.int64, device=dev)
    j0 = torch.full((n_p, 2, n_base), SENTINEL, dtype=torch.float64, device=dev) if prepass else None
    clip_t = torch.as_tensor(np.asarray(clip, dtype=np.float64), device=dev) if clip is not None else None
    assert clip_t is None or clip_t.shape == (n_p,)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                        # noqa: E731
    rc = lib.pem_sobol_sweep_f64_dev(study.GROUPS.index(group), n_base, first, seed, n_p, ptr(kind), ptr(a), ptr(b), sc.torr(),
                                     study.PLUME_RADIUS, study.PLUME_I_B0, sc.uion()[1], float(spike), int(max_attempts), ptr(clip_t),
                                     ptr(j0), ptr(partial), ptr(flags), n_blocks, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.PEM_OK, (rc, lib.pem_last_error().decode(errors='replace'))
    out = {'partial': partial.cpu().numpy(), 'flags': flags.cpu().numpy(), 'j0': j0.cpu().numpy() if prepass else None}
    if prepass:                                         # the pre-pass forms no sums and leaves the partial alone
        assert np.all(out['partial'] == SENTINEL) and not np.any(out['j0'] == SENTINEL)
    else:
        assert not np.any(out['partial'] == SENTINEL)
    assert np.all(out['flags'] >= 0)
    return out


def _held(got, want, e, what):
    """The per-entry rule: NaN and inf patterns identical, |got - want| <= e where e is finite (e = 0: equal; e = inf: the oracle's
    own terms are not finite, nothing to hold).  Returns the largest |got - want| / e."""
    got, want, e = np.broadcast_arrays(np.asarray(got, dtype=np.float64), want, e)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f'NaN pattern differs: {what}: {np.argwhere(np.isnan(got) != np.isnan(want))[:10]}'
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.sign(got[np.isinf(got)]), np.sign(want[np.isinf(want)])), \
        f'inf pattern differs: {what}'
    fin = np.isfinite(want) & np.isfinite(e)
    d = np.abs(got[fin] - want[fin])
    bad = d > e[fin]
    assert not bad.any(), f'{what}: {int(bad.sum())} values outside their bound, worst {np.max(d[bad] / e[fin][bad])} x at ' \
                          f'{np.argwhere(fin)[bad][:5].tolist()}: got {got[fin][bad][:5]}, want {want[fin][bad][:5]}'
    pos = e[fin] > 0
    return float(np.max(d[pos] / e[fin][pos], initial=0.0))


def _sums_held(got, want, bound, what):
    """long-double sums: NaN pattern identical, |got - want| <= bound elsewhere.  Returns the largest |got - want| / bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'NaN pattern differs: {what}: got {np.argwhere(np.isnan(got)).tolist()[:12]}, ' \
                                               f'want {np.argwhere(nan).tolist()[:12]}'
    assert np.isfinite(np.asarray(want, dtype=np.float64)[~nan]).all() and np.isfinite(got[~nan]).all(), what
    d = np.abs(got.astype(L) - want)
    bad = ~nan & ~(d <= bound)
    assert not bad.any(), f'{what}: {int(bad.sum())} sums outside their bound at {np.argwhere(bad)[:8].tolist()}: ' \
                          f'error / bound {np.asarray(d[bad] / bound[bad], dtype=np.float64)[:8]}'
    pos = ~nan & (bound > 0)
    return float(np.max(d[pos] / bound[pos], initial=0.0))


# ---- part 1: every group, point by point ----------------------------------------------------------------------------------------------
def _points_launch(group, pts, **kw):
    """m point masses as the pressures of launches of one base sample: (f (nq, m), flags (m, 4)), the structure of the sums checked"""
    nv = _nv(group)
    parts, flags = [], []
    for s in range(0, len(pts), 256):
        out = _launch(group, sc.point_tables(pts[s:s + 256]), 1, n_blocks=1, max_attempts=1, **kw)
        parts.append(out['partial'][:, 0])
        flags.append(out['flags'][:, 0])
    part, flags = np.concatenate(parts), np.concatenate(flags)
    f = part[:, 0, :] / 2.0
    fin = np.isfinite(f)
    with np.errstate(over='ignore', invalid='ignore'):
        sq = 2.0 * (f * f)
    normal = fin & ((np.abs(f) > 1e-150) | (f == 0.0))              # (2 f^2 in the denormal range is not exact)
    assert np.array_equal(part[:, 1, :][normal], sq[normal]), group
    assert np.array_equal(np.isnan(part[:, 1, :]), np.isnan(f)), group
    rest = part[:, 2:, :]
    finr = np.broadcast_to(fin[:, None, :], rest.shape)
    assert np.all(rest[finr] == 0.0) and np.all(np.isnan(rest[~finr])), group
    assert np.all(np.isin(flags[:, :2], (0, nv + 2))) and np.all(np.isin(flags[:, 2:], (0, 2))), group
    return f.T, flags


@pytest.fixture(scope='module')
def plume_points():
    pts = sc.points('Plume')
    ev = sc.evaluate('Plume', sc.designed('Plume', pts))
    f, flags = _points_launch('Plume', pts, spike=np.inf)
    return pts, ev, f, flags


def test_plume_points_against_the_oracle(plume_points):
    """j_ion(0) of every point under the fuzz tool's per-entry rule, 1e-20 exactly and flag 1 = nv + 2 exactly where the oracle calls
    the sample invalid; nothing is rejected under an infinite threshold"""
    pts, ev, f, flags = plume_points
    assert int(sc.off_axis(ev).sum()) >= 20 and int(ev['literal'].sum()) >= 50 and int(ev['invalid'].sum()) >= 20
    assert np.array_equal(flags[:, 1] == 10, ev['invalid']), np.flatnonzero((flags[:, 1] == 10) != ev['invalid'])
    assert np.all(f[0][ev['invalid']] == 1e-20) and not np.any(f[0][~ev['invalid']] == 1e-20)
    assert np.all(flags[:, [0, 2, 3]] == 0)
    r = _held(f, ev['f'], ev['e'], 'Plume points')
    print(f'\nSWEEP-KERNEL part 1 Plume: {len(pts)} points, {int(ev["literal"].sum())} literal branch, {int(ev["invalid"].sum())} invalid, '
          f'{int(sc.off_axis(ev).sum())} off-axis maximum, {int((~np.isfinite(ev["f"])).sum())} non-finite; worst error / bound {r:.3g}')


def test_plume_points_spike_decisions(plume_points):
    """the study's threshold, and thresholds between j(0) and the maximum of the profiles whose maximum is off the axis: rejected =
    unaccepted = 2 (rows A and B, one draw each) exactly where the oracle's profile reaches the threshold; the last draw is kept"""
    pts, ev, f_inf, _ = plume_points
    levels, members = sc.spike_levels(ev)
    assert sum(len(m) for m in members) >= 20
    seen = np.zeros(len(pts), dtype=bool)
    n_rej = 0
    for thr, mem in [(sc.SPIKE, [])] + list(zip(levels, members)):
        assert sc.near(ev['profile'], thr) == 0
        f, flags = _points_launch('Plume', pts, spike=thr)
        want = sc.expect_rejected(ev, thr)
        assert np.array_equal(flags[:, 2] == 2, want), (thr, np.flatnonzero((flags[:, 2] == 2) != want))
        assert np.array_equal(flags[:, 3], flags[:, 2])
        assert np.array_equal(f, f_inf, equal_nan=True)
        assert np.all(want[mem]) and np.all(ev['profile'][mem, 0] < thr)           # j(0) alone would have accepted these
        seen[mem] = True
        n_rej += int(want.sum()) if thr == sc.SPIKE else 0
    print(f'\nSWEEP-KERNEL part 1 spike: {n_rej} points rejected at {sc.SPIKE}; {len(levels)} further thresholds, {int(seen.sum())} off-axis '
          f'points rejected by the grid alone')


@pytest.mark.parametrize('group', ['Cathode', 'Thruster'])
def test_stage_points_against_the_oracle(group):
    """V_cc under the rule of wild_parity.check_against_oracle, T and u_ion at the node to TOL relative, flag 0 = nv + 2 exactly where
    the oracle's thrust or beam current is negative"""
    pts = sc.points(group)
    ev = sc.evaluate(group, sc.designed(group, pts))
    f, flags = _points_launch(group, pts)
    r = _held(f, ev['f'], ev['e'], f'{group} points')
    assert np.array_equal(flags[:, 0] == _nv(group) + 2, ev['nonphys']), np.flatnonzero((flags[:, 0] != 0) != ev['nonphys'])
    assert np.all(flags[:, 1:] == 0)
    if group == 'Thruster':
        assert int(ev['nonphys'].sum()) >= 5
    print(f'\nSWEEP-KERNEL part 1 {group}: {len(pts)} points, {int(ev["nonphys"].sum())} non-physical, '
          f'{int((~np.isfinite(ev["f"])).any(axis=0).sum())} non-finite; worst error / bound {r:.3g}')


# ---- part 2: the Plume pre-pass on rough priors -----------------------------------------------------------------------------------------
def _prepass(tables, max_attempts, n_blocks=3, n_base=sc.ROUGH_N, first=0):
    return _launch('Plume', tables, n_base, first=first, spike=sc.SPIKE, max_attempts=max_attempts, prepass=True, n_blocks=n_blocks)


def _check_prepass(out, recs, n_blocks, what):
    """j0 entry by entry against the oracle at the restated rows; every workgroup's flags against the restatement"""
    worst = 0.0
    for p, rec in enumerate(recs):
        worst = max(worst, _held(out['j0'][p], rec['f'][:2, 0], rec['e'][:2, 0], f'{what} j0 p={p}'))
        ab = {k: rec[k][:2] for k in ('nonphys', 'invalid', 'rejected', 'unaccepted')}        # the pre-pass evaluates A and B alone
        want = sc.flag_counts(ab, n_blocks)
        assert np.array_equal(out['flags'][p], want), (what, p, out['flags'][p].tolist(), want.tolist())
    return worst


@pytest.fixture(scope='module')
def rough():
    t = sc.rough_plume_tables()
    recs = {ma: sc.restate('Plume', t, sc.ROUGH_N, sc.ROUGH_SEED, max_attempts=ma) for ma in (64, 2)}
    return t, recs, {ma: _prepass(t, ma) for ma in (64, 2)}


@pytest.mark.parametrize('max_attempts', [64, 2])
def test_prepass_on_rough_priors(rough, max_attempts):
    """accepted (or last) rows, rejected, unaccepted and invalid counts of 700 samples at three pressures in three workgroups"""
    t, recs, outs = rough
    rec = recs[max_attempts]
    for r in rec:                                       # the conditions, from the restatement alone
        assert np.isfinite(r['f']).all() and int(r['literal'].sum()) > 1000 and int(r['invalid'].sum()) > 300 and int(r['rejected'].sum()) > 20
    n_un = sum(int(r['unaccepted'].sum()) for r in rec)
    assert (n_un >= 1) if max_attempts == 2 else (n_un == 0)
    worst = _check_prepass(outs[max_attempts], rec, 3, f'rough pre-pass, {max_attempts} attempts')
    print(f'\nSWEEP-KERNEL part 2 max_attempts={max_attempts}: per pressure literal {[int(r["literal"].sum()) for r in rec]}, invalid '
          f'{[int(r["invalid"].sum()) for r in rec]} of {10 * sc.ROUGH_N} evaluations, rejected {[int(r["rejected"].sum()) for r in rec]}, '
          f'never accepted {[int(r["unaccepted"].sum()) for r in rec]}; worst error / bound {worst:.3g}')


def test_prepass_does_not_depend_on_the_launch_shape(rough):
    """one, three or seven workgroups (seven: whole workgroups and most of another without a live sample) and one launch or two with
    first_index: the same bits, the same counts"""
    t, recs, outs = rough
    base = outs[2]
    total = base['flags'].sum(axis=1)
    for nb in (1, 7):
        out = _prepass(t, 2, n_blocks=nb)
        assert np.array_equal(out['j0'], base['j0']) and np.array_equal(out['flags'].sum(axis=1), total), nb
        for p, rec in enumerate(recs[2]):
            want = sc.flag_counts({k: rec[k][:2] for k in ('nonphys', 'invalid', 'rejected', 'unaccepted')}, nb)
            assert np.array_equal(out['flags'][p], want), (nb, p)
        if nb == 7:
            assert np.all(out['flags'][:, 3:] == 0)                        # 700 samples: workgroups 3 .. 6 have no live sample
    lo, hi = _prepass(t, 2, n_base=257, first=0), _prepass(t, 2, n_base=443, first=257)
    assert np.array_equal(np.concatenate([lo['j0'], hi['j0']], axis=2), base['j0'])
    assert np.array_equal(lo['flags'].sum(axis=1) + hi['flags'].sum(axis=1), total)


def test_prepass_of_one_pressure_has_its_own_streams(rough):
    """n_p = 1: the stream numbering of one pressure, not the row p = 0 of three"""
    t, recs, outs = rough
    one = tuple(v[:1] for v in t)
    rec = sc.restate('Plume', one, sc.ROUGH_N, sc.ROUGH_SEED, max_attempts=2, only_ab=True)
    assert not np.array_equal(rec[0]['xa'], recs[2][0]['xa'])
    out = _prepass(one, 2)
    worst = _check_prepass(out, rec, 3, 'one pressure')
    assert not np.array_equal(out['j0'][0], outs[2]['j0'][0])
    print(f'\nSWEEP-KERNEL part 2 one pressure: rejected {int(rec[0]["rejected"].sum())}, never accepted {int(rec[0]["unaccepted"].sum())}; '
          f'worst error / bound {worst:.3g}')


@pytest.fixture(scope='module')
def wild():
    t = sc.wild_plume_tables()
    return t, sc.restate('Plume', t, sc.ROUGH_N, sc.ROUGH_SEED)


def test_prepass_on_wild_priors(wild):
    """densities below zero: NaN j0 where the oracle has them, the values under the same rule"""
    t, recs = wild
    n_nan = sum(int(np.isnan(r['f'][:2]).sum()) for r in recs)
    assert n_nan >= 5 and not any(np.isinf(r['f']).any() for r in recs)
    worst = _check_prepass(_prepass(t, 64), recs, 3, 'wild pre-pass')
    print(f'\nSWEEP-KERNEL part 2 wild: {n_nan} NaN j0 in {6 * sc.ROUGH_N} rows; worst error / bound {worst:.3g}')


# ---- part 3: the estimator sums per workgroup ---------------------------------------------------------------------------------------------
def _check_main(group, out, recs, clip, n_blocks, what, j0=None):
    """every workgroup's partial and flags of one launch against the oracle (and rows 0, 1 against the device's own j0)"""
    worst = {'sums': 0.0, 'ab': 0.0}
    for p, rec in enumerate(recs):
        f, e = sc.clipped(rec, clip[p]) if clip is not None else (rec['f'], rec['e'])
        want, bound, _ = sc.partial_sums(f, e, n_blocks)
        got = out['partial'][p]
        assert np.all(got[want == 0] == 0.0), (what, p)                     # (also the workgroups without a live sample)
        worst['sums'] = max(worst['sums'], _sums_held(got, want, bound, f'{what} p={p} n_blocks={n_blocks}'))
        assert np.array_equal(out['flags'][p], sc.flag_counts(rec, n_blocks)), (what, p, out['flags'][p].tolist())
        if j0 is not None:
            with np.errstate(invalid='ignore'):
                v = np.where(j0[p] > clip[p], clip[p], j0[p]) if clip is not None else j0[p]
            w2, b2 = sc.ab_sums(v[0][None], v[1][None], n_blocks)
            worst['ab'] = max(worst['ab'], _sums_held(got[:, :2], w2, b2, f'{what} rows 0, 1 of the pre-pass values p={p}'))
    return worst


@pytest.mark.parametrize('n_blocks', [1, 3, 7])
def test_plume_sums_per_workgroup(rough, n_blocks):
    t, recs, outs = rough
    rec = recs[64]
    clip = np.array([sc.choose_clip(r['f'][:2]) for r in rec])
    for r, thr in zip(rec, clip):
        assert sc.near(r['f'], thr) == 0 and np.all(np.abs(r['f'] - thr) > r['e']) and int((r['f'] > thr).sum()) >= 5
    out = _launch('Plume', t, sc.ROUGH_N, spike=sc.SPIKE, max_attempts=64, clip=clip, n_blocks=n_blocks)
    worst = _check_main('Plume', out, rec, clip, n_blocks, 'rough Plume', j0=outs[64]['j0'])
    print(f'\nSWEEP-KERNEL part 3 n_blocks={n_blocks}: clip {clip.tolist()}, worst error / bound: sums against the oracle '
          f'{worst["sums"]:.3g}, rows 0 and 1 against the pre-pass values {worst["ab"]:.3g}')


def test_plume_sums_without_a_clip(rough):
    """clip = NULL: nothing is clipped (rows 0 and 1 are the sums of the pre-pass values themselves, which the clipped ones are not)"""
    t, recs, outs = rough
    out = _launch('Plume', t, sc.ROUGH_N, spike=sc.SPIKE, max_attempts=64, clip=None, n_blocks=3)
    _check_main('Plume', out, recs[64], None, 3, 'rough Plume, no clip', j0=outs[64]['j0'])
    clip = np.array([sc.choose_clip(r['f'][:2]) for r in recs[64]])
    there = _launch('Plume', t, sc.ROUGH_N, spike=sc.SPIKE, max_attempts=64, clip=clip, n_blocks=3)
    assert np.all(there['partial'][:, :, 0].sum(axis=1) < out['partial'][:, :, 0].sum(axis=1))


def test_nan_stays_in_the_partials_it_enters(wild):
    """the wild table in three workgroups: exactly the partial entries (workgroup, pressure, row) a NaN value enters are NaN, every
    other entry is held as before"""
    t, recs = wild
    clip = np.array([sc.choose_clip(r['f'][:2]) for r in recs])
    for r, thr in zip(recs, clip):
        fin = np.isfinite(r['f'])
        assert np.all(np.abs(r['f'][fin] - thr) > r['e'][fin])
    pre = _prepass(t, 64)
    out = _launch('Plume', t, sc.ROUGH_N, spike=sc.SPIKE, max_attempts=64, clip=clip, n_blocks=3)
    nan = np.isnan(out['partial'])
    assert int(nan.sum()) >= 10 and int((~nan).sum()) >= 10               # (a NaN fA takes its whole workgroup: most entries are NaN)
    worst = _check_main('Plume', out, recs, clip, 3, 'wild Plume', j0=pre['j0'])
    print(f'\nSWEEP-KERNEL part 3 wild: {int(nan.sum())} of {nan.size} partial entries NaN, as the oracle says; worst error / bound of the '
          f'others {worst["sums"]:.3g}')


# ---- part 4: the Thruster and Cathode launches on rough priors ------------------------------------------------------------------------------
@pytest.mark.parametrize('n_blocks', [1, 2])
@pytest.mark.parametrize('group', ['Cathode', 'Thruster'])
def test_stage_sums_per_workgroup(group, n_blocks):
    """negative flow rates, a normal T_e, vacuum potentials below zero: the non-physical count per workgroup exactly, the
    [row][q] layout of both QoIs"""
    t = sc.rough_stage_tables(group)
    recs = sc.restate(group, t, sc.STAGE_N, sc.STAGE_SEED)
    nonphys = [int(r['nonphys'].sum()) for r in recs]
    assert all(np.isfinite(r['f']).all() for r in recs) and (group != 'Thruster' or min(nonphys) > 20)
    out = _launch(group, t, sc.STAGE_N, seed=sc.STAGE_SEED, n_blocks=n_blocks)
    worst = _check_main(group, out, recs, None, n_blocks, f'rough {group}')
    print(f'\nSWEEP-KERNEL part 4 {group} n_blocks={n_blocks}: non-physical evaluations per pressure {nonphys} of '
          f'{(_nv(group) + 2) * sc.STAGE_N}; worst error / bound {worst["sums"]:.3g}')


# ---- the refusals of the entry point, and the driver's ---------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """each refused call returns PEM_ERR_INVALID_ARG and leaves the device buffers as they were"""
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd import sobol as study
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device())
    n_p_max = 65536
    kind = torch.zeros((n_p_max, 15), dtype=torch.int32, device=dev)
    a = torch.as_tensor(np.tile(np.array(list(study.PEM_V0_NOMINAL.values())), (n_p_max, 1)), device=dev)     # the nominal point
    partial = torch.full((n_p_max, 34, 2), SENTINEL, dtype=torch.float64, device=dev)
    flags = torch.full((n_p_max, 4), -1, dtype=torch.int64, device=dev)
    j0 = torch.full((n_p_max, 2), SENTINEL, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                        # noqa: E731
    ok = dict(group=2, n_base=1, n_p=1, max_attempts=1, j0=None, partial=partial, n_blocks=1)
    cases = {'an unknown group': dict(group=3), 'a negative group': dict(group=-1), 'n_p = 0': dict(n_p=0), 'n_p = 65536': dict(n_p=65536),
             'n_blocks = 0': dict(n_blocks=0), 'n_base = 0': dict(n_base=0), 'j0_out for the Cathode group': dict(group=0, j0=j0),
             'j0_out for the Thruster group': dict(group=1, j0=j0), 'j0_out and partial NULL': dict(partial=None),
             'max_attempts = 0': dict(max_attempts=0), '6 n_p max_attempts = 2^32 + 2': dict(max_attempts=715827883),
             '6 n_p max_attempts = 6 2^30': dict(n_p=4, max_attempts=1 << 28)}
    for what, change in cases.items():
        kw = dict(ok, **change)
        rc = lib.pem_sobol_sweep_f64_dev(kw['group'], kw['n_base'], 0, 1, kw['n_p'], ptr(kind), ptr(a), ptr(a), sc.torr(), study.PLUME_RADIUS,
                                         study.PLUME_I_B0, sc.uion()[1], np.inf, kw['max_attempts'], None, ptr(kw['j0']), ptr(kw['partial']),
                                         ptr(flags), kw['n_blocks'], C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == _lib.PEM_ERR_INVALID_ARG, (what, rc)
        assert 'pem_sobol_sweep_f64' in lib.pem_last_error().decode(errors='replace'), what
    torch.cuda.synchronize()
    assert bool((partial == SENTINEL).all()) and bool((flags == -1).all()) and bool((j0 == SENTINEL).all())
    # the largest product that is accepted: 6 n_p max_attempts = 2^32 - 4 (nothing is rejected under an infinite threshold)
    rc = lib.pem_sobol_sweep_f64_dev(2, 1, 0, 1, 1, ptr(kind), ptr(a), ptr(a), sc.torr(), study.PLUME_RADIUS, study.PLUME_I_B0, sc.uion()[1], np.inf,
                                     715827882, None, None, ptr(partial), ptr(flags), 1, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.PEM_OK and bool((flags[0] >= 0).all())


def test_driver_raises_on_a_row_never_accepted():
    """drivers.sobol_sweep(max_attempts=1): the first base sample of the default study at seed 11 whose draw is rejected makes the
    call raise; one sample fewer and it returns"""
    import sobol_sweep_np as ref
    from hallthrusterpem_amd import drivers
    from hallthrusterpem_amd import sobol as study
    pb = study.DEFAULT_PRESSURES
    first = min(int(np.flatnonzero(rej)[0]) for p in range(len(pb)) for row in (0, 1)
                for rej in [ref.design_rows('Plume', 2000, 11, pb, p, row, sc.torr(), sc.SPIKE, 1)[1]] if rej.any())
    with pytest.raises(RuntimeError, match=r'plume rows still reach 200(\.0)? A/m\^2 after 1 draws'):
        drivers.sobol_sweep(first + 1, seed=11, max_attempts=1, qois=('jion',))
    res = drivers.sobol_sweep(first, seed=11, max_attempts=1, qois=('jion',))
    assert np.all(res['jion']['rejected'] == 0)
    print(f'\nSWEEP-KERNEL driver: N = {first + 1} raises, N = {first} returns')
