"""The fused likelihood against j_ion measured at several sweep radii (`pem_coupled_system_{loglik,predict}_radii_f64_dev`,
JMODE 8 / 9 of plume_r1_kernel) over its dispatch space -- the net tests/test_likelihood_kernels.py holds its one-radius parent in.

Every launch is checked three ways (`_system_radii`): JMODE 9's j_ion predictions sample by sample against the long-double
restatement from the oracle's terms (hp_likelihood.radii_record_ref, under the project's own j_ion slack), its other columns and
everything it must not write bit for bit; JMODE 8's sums against the long-double sum over JMODE 9's own values; the flags and
scalars against the oracle.  Sample counts reach past two rounds of the persistent loop; the tables are small enough for two
workgroups per CU, large enough for one, and of the size at which the radii area behind the table decides between the two; every
radius count 2 .. 8 runs, with conditions whose records all sit at the first or at the last radius; the table limits are run with
8 radii (160 000 bytes of LDS); radius indices past the table clamp; non-physical samples leave nothing behind for the samples
that follow them in the same slot of the per-wave `pairs` area."""
from types import SimpleNamespace

import numpy as np
import pytest

import hp_likelihood as hl
import parity_rules as pr
from test_likelihood_kernels import SENTINEL, _assert_refused, _batch, _predict_ref, _rounds_n, _table

PLUME_ROWS = ('P_b', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')
FAST_LDS = 69696           # fast_lds_doubles<4, 8>() * 8: Simpson and normaliser tables (576 doubles) + 4 waves x (9 x 64 + 16 x 91 + 2)
CU_LDS = 160 * 1024
assert FAST_LDS == 8 * (2 * 96 + 32 * 12 + 4 * (9 * 64 + 16 * 91 + 2))


def _table_bytes(tab):
    """system_lds_bytes, padded to 16 as radii_lds_bytes pads it: records | spans | u_ion denominators"""
    return (32 * tab.n_rec + 32 * tab.n_cond + 8 * max(tab.n_node, 2) + 15) & ~15


def _radii_bytes(R):
    """what radii_lds_bytes adds behind the table: {r, 1 / r^2, 1 / (2 pi r^2)} [R] padded to 16 bytes | pairs [4 waves][16][R] double2"""
    return 8 * ((3 * R + 1) & ~1) + 4 * 16 * R * 16


def _radii(R):
    return tuple(float(r) for r in np.linspace(0.4, 1.6, R))


def _table_radii(rng, n_cond, R, counts=None, big=False):
    """`_table` with sweep_radii = linspace(0.4, 1.6, R): the fourth word of every j_ion record becomes k | (ridx << 8).  The two
    conditions with the most j_ion records have all of them at radius 0 and all at radius R - 1; the radius of every other
    record is drawn, every radius at least once (where the table has R such records)."""
    import torch
    tab = _table(rng, n_cond, counts=counts, big=big)
    rec, span = tab.np_rec.copy(), tab.np_span
    k = np.zeros(tab.n_rec, np.int64)
    ridx = np.full(tab.n_rec, -1, np.int64)
    by_count = sorted((c for c in range(n_cond) if span[c, 0, 1] > 0), key=lambda c: -span[c, 0, 1])
    pinned = dict(zip(by_count[:2], (0, R - 1))) if len(by_count) >= 3 else {}
    free = []
    for c in by_count:
        f, cnt = span[c, 0]
        k[f:f + cnt] = np.ascontiguousarray(rec[f:f + cnt, 3]).view(np.int64)
        if c in pinned:
            ridx[f:f + cnt] = pinned[c]
        else:
            free += list(range(f, f + cnt))
    free = np.asarray(free, np.int64)
    ridx[free] = rng.integers(0, R, free.size)
    if free.size >= R:
        ridx[rng.choice(free, R, replace=False)] = np.arange(R)
        assert set(ridx[free]) == set(range(R))
    j = ridx >= 0
    rec[j, 3] = (k[j] | (ridx[j] << 8)).view(np.float64)
    tab.sweep_radii = _radii(R)
    tab.sweep_radius = tab.sweep_radii[-1]
    tab.np_rec, tab.rec, tab.np_k, tab.np_ridx = rec, torch.as_tensor(rec, device='cuda'), k, ridx
    return tab


def _with_ridx(tab, ridx):
    """tab with the radius index of its j_ion records replaced (the clamp test writes indices past the table)"""
    import torch
    new = SimpleNamespace(**vars(tab))
    rec = tab.np_rec.copy()
    j = tab.np_ridx >= 0
    rec[j, 3] = (tab.np_k[j] | (ridx[j] << 8)).view(np.float64)
    new.np_rec, new.rec, new.np_ridx = rec, torch.as_tensor(rec, device='cuda'), ridx
    return new


def _batch_of(x):
    """`_batch` for given [15][n] inputs (numpy)"""
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    b = CoupledBatch(x.shape[1], profile=True, thruster_qoi=True)
    b.inputs.copy_(torch.as_tensor(x, device='cuda'))
    b.run()
    return b


def _rows(x, idx=None):
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    return {k: np.ascontiguousarray(x[i] if idx is None else x[i, idx]) for i, k in enumerate(COUPLED_INPUTS)}


def _qoi_ref(x, radii, chunk=16384):
    """the oracle's per-sample results for [15][n] inputs: the all-radii invalid flag, and div_angle and T_c at the last radius with
    the bounds parity_rules.divergence_error holds them to -- in chunks, (n, 91, R) profiles are not small at a quarter of a
    million samples"""
    from hallthrusterpem_amd import constants
    from oracle import oracle_ctypes as oc
    n = x.shape[1]
    out = SimpleNamespace(invalid=np.zeros(n, bool), div=np.zeros(n), tc=np.zeros(n), bounds=[])
    keep = ('cos_rel', 'cond_cos', 'comparable', 'cos_div')
    with np.errstate(all='ignore'):
        for f in range(0, n, chunk):
            d = _rows(x, slice(f, f + chunk))
            last = oc.coupled(d, constants.TORR_2_PA, radius=radii[-1])
            args = [d[q] for q in PLUME_ROWS] + [last['I_B0'], constants.TORR_2_PA]
            out.invalid[f:f + chunk] = oc.plume(*args, radii=radii)['invalid']
            out.div[f:f + chunk], out.tc[f:f + chunk] = last['div_angle'], last['T_c']
            bd = pr.plume_bounds(oc.plume_terms(*args, radii=radii[-1:]), last['I_B0'])
            out.bounds.append({q: bd[q] for q in keep})
    out.bounds = {q: np.concatenate([bd[q] for bd in out.bounds]) for q in keep}
    return out


def _records_of(tab, c):
    span = tab.np_span
    return np.concatenate([np.arange(span[c, kd, 0], span[c, kd, 0] + span[c, kd, 1]) for kd in range(4)]).astype(np.int64)


def _system_radii(b, tab, subset=None, extra_ld=0, ref=None):
    """One launch of each mode on batch b and table tab; mirrors test_likelihood_kernels._system.
    1. JMODE 9: the j_ion columns of the samples in `subset` (default: all) against hl.radii_record_ref under its slack; every
       other entry -- V_cc, T and u_ion columns, which do not depend on the radii, padding records and columns, rows of absent
       samples (the sentinel) -- bit for bit `_predict_ref`'s, for all samples.
    2. JMODE 8 against hl.record_sum over JMODE 9's OWN values, all samples: both modes take a record's model value from the same
       `jion_model`, so the sum carries the roundings of the one-radius sum and nothing else -- the one-radius bound, unchanged.
    3. all samples: `invalid` the oracle's all-radii flag, V_cc the bits of pem_coupled_f64_dev, div_angle and T_c those of the
       last radius under parity_rules.divergence_error (`comparable` is all true under the priors: tests/test_hp_likelihood.py).
    Returns (predictions, per-sample sums, the largest |j_ion error| / slack)."""
    import torch
    from hallthrusterpem_amd import constants
    from oracle import oracle_ctypes as oc
    n, n_cond, radii = b.n, tab.n_cond, tab.sweep_radii
    R = len(radii)
    rows, ld = -(-n // n_cond), tab.n_rec + extra_ld
    what = f'n={n} n_cond={n_cond} n_rec={tab.n_rec} R={R}'
    b.run()                                            # (an earlier check on this batch left the fused launch's V_cc behind)
    vcc = b.qoi[0].cpu().numpy().copy()
    x = b.inputs.cpu().numpy()
    rec, span = tab.np_rec, tab.np_span

    # ---- 1. JMODE 9
    pred = torch.full((rows, ld), SENTINEL, dtype=torch.float64, device='cuda')
    b.run_system_predict(tab, pred)
    got = pred.cpu().numpy()
    no_jion = SimpleNamespace(**vars(tab))
    no_jion.np_span = span.copy()
    no_jion.np_span[:, 0, 1] = 0
    want = _predict_ref(b, no_jion, ld)
    jion = np.zeros(got.shape, bool)
    for c in range(n_cond):
        f, cnt = span[c, 0]
        jion[: len(range(c, n, n_cond)), f:f + cnt] = True
    bad = (got.view(np.int64) != want.view(np.int64)) & ~jion
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f'JMODE 9 {what}: {int(bad.sum())} entries beside the j_ion records differ; first at {i}: got {got[i]!r} '
                             f'want {want[i]!r}')
    sub = np.arange(n) if subset is None else np.unique(np.asarray(subset, np.int64))
    with np.errstate(all='ignore'):
        d = _rows(x, sub)
        args = [d[q] for q in PLUME_ROWS] + [oc.coupled(d, constants.TORR_2_PA)['I_B0'], constants.TORR_2_PA]
        terms = oc.plume_terms(*args, radii=radii)
        invalid_sub = oc.plume(*args, radii=radii)['invalid']
    worst = 0.0
    for c in range(n_cond):
        f, cnt = span[c, 0]
        at = np.flatnonzero(sub % n_cond == c)
        if cnt == 0 or at.size == 0:
            continue
        tc = {q: (v if q == 'radii' else v[at]) for q, v in terms.items()}
        r = rec[f:f + cnt]
        model, slack = hl.radii_record_ref(tc, invalid_sub[at], tab.np_k[None, f:f + cnt], r[None, :, 0],
                                           np.minimum(tab.np_ridx[None, f:f + cnt], R - 1), I_B0=args[-2][at])
        worst = max(worst, hl.assert_model_within(got[sub[at] // n_cond, f:f + cnt], model, slack, f'JMODE 9 j_ion {what} condition {c}'))
    print(f'\n{what}: JMODE 9 j_ion over {sub.size} samples, worst |error| / slack = {worst:.3e}')

    # ---- 2. JMODE 8
    ll = torch.full((n,), np.nan, dtype=torch.float64, device='cuda')
    b.run_system_loglik(tab, out=ll)
    ll = ll.cpu().numpy()
    want, bound = np.zeros(n, dtype=hl.LD), np.zeros(n, dtype=hl.LD)
    with np.errstate(all='ignore'):
        for c in range(n_cond):
            idx = np.arange(c, n, n_cond)
            r = _records_of(tab, c)
            if idx.size == 0 or r.size == 0:
                continue
            want[idx], bound[idx] = hl.record_sum(got[(idx // n_cond)[:, None], r[None, :]], rec[r, 1], rec[r, 2])
        w64 = want.astype(np.float64)
        want = np.where(np.isinf(w64), w64.astype(hl.LD), want)      # past the double range every fp64 sum is infinite
    hl.assert_within(ll, want, bound, f'JMODE 8 {what}')

    # ---- 3. flags and scalars
    ref = _qoi_ref(x, radii) if ref is None else ref
    flag = b.invalid.cpu().numpy().astype(bool)
    assert np.array_equal(flag, ref.invalid), f'{what}: invalid differs from the oracle at {np.flatnonzero(flag != ref.invalid)[:8]}'
    assert np.array_equal(flag[sub], invalid_sub)
    assert np.array_equal(b.qoi[0].cpu().numpy().view(np.int64), vcc.view(np.int64)), f'{what}: V_cc is not pem_coupled_f64_dev\'s'
    e = pr.divergence_error(b.qoi[1].cpu().numpy(), ref.div, b.qoi[2].cpu().numpy(), ref.tc, ref.bounds, what)
    assert e['err_div'] <= pr.TOL and e['err_tc'] <= pr.TOL, (what, e)
    return got, ll, worst


# ---- 1. sample counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 64 * 6 + 17])
def test_sample_counts(n):
    rng = np.random.default_rng(n)
    # (`_table`'s counts, turned so that condition 0 -- all there is at n = 1 -- has j_ion records)
    tab = _table_radii(rng, 36, 3, counts=lambda c: ((c + 7) % 18, c % 4, (c // 4) % 4, (c // 2) % 5))
    assert tab.np_span[0, 0, 1] == 7
    _system_radii(_batch(n, seed=n), tab)


# ---- 2. every radius count ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('R', range(2, 9))
def test_every_radius_count(R):
    """lane (s, c) forms the pairs of radii c and c + 4: R = 4 gives every lane one, R = 5 lane 0 alone two, R = 8 every lane two.
    Record counts 0 .. 17 per condition, one condition all at the first radius, one all at the last; three padding columns."""
    rng = np.random.default_rng(100 + R)
    tab = _table_radii(rng, 36, R)
    j = tab.np_ridx >= 0
    assert set(tab.np_ridx[j]) == set(range(R)) and sorted(set(tab.np_span[:, 0, 1])) == list(range(18))
    first, last = (np.flatnonzero([np.all(tab.np_ridx[f:f + cnt] == r) and cnt > 1 for f, cnt in tab.np_span[:, 0]]) for r in (0, R - 1))
    assert first.size and last.size
    got, _, _ = _system_radii(_batch(64 * 3 + 5, seed=R), tab, extra_ld=3)
    assert np.all(got[:, -3:] == SENTINEL)


# ---- 3. two rounds and a ragged tail ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('R', [3, 8])
def test_two_rounds_small_large_and_straddling_table(R):
    """past two rounds of the persistent loop plus a ragged tail, with a table that leaves two workgroups per CU, one that leaves
    one, and one for which the radii area behind the table decides: FAST + table <= 80 KiB < FAST + table + radii area.  Every
    round of every tile rewrites the wave's `pairs`; two non-physical samples in round 0 of tile 0 overwrite theirs with
    {0, 1e-20}, and the samples in the same slots of the next round and of the same wave's next tile (at two workgroups per CU
    and at one) are held to the oracle.  The oracle check of the predictions runs on the first tile, the ragged last tile, every
    61st sample between and those; the sums, flags and scalars on every sample."""
    import torch
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    rng = np.random.default_rng(200 + R)
    n = _rounds_n(tail=45)
    b = _batch(n, seed=21 + R)
    plant = np.array([3, 9])
    b.inputs[COUPLED_INPUTS.index('mdot_a'), torch.as_tensor(plant, device='cuda')] = 0.0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    after = np.concatenate([plant + 16] + [plant + 64 * 4 * cus * per_cu for per_cu in (1, 2)])
    assert after.max() < n
    subset = np.concatenate([np.arange(64), np.arange(n - n % 64, n), np.arange(64, n, 61), after])
    half = CU_LDS // 2
    small = _table_radii(rng, 7, R, counts=lambda c: (c + 3, c % 2, 1, c % 3))
    assert FAST_LDS + _table_bytes(small) + _radii_bytes(R) <= half
    large = _table_radii(rng, 127, R, counts=lambda c: (c % 18 // 3, 1, c % 2, 1 if c % 5 == 0 else 0))
    assert FAST_LDS + _table_bytes(large) > half
    straddle = _table_radii(rng, 24, R, counts=lambda c: (c % 12 + 3, c % 2, 1, c % 3))
    assert FAST_LDS + _table_bytes(straddle) <= half < FAST_LDS + _table_bytes(straddle) + _radii_bytes(R)
    print(f'\nR = {R}: straddling table {_table_bytes(straddle)} B + radii area {_radii_bytes(R)} B behind {FAST_LDS} B')
    ref = _qoi_ref(b.inputs.cpu().numpy(), _radii(R))
    assert ref.invalid[plant].all() and not ref.invalid[after].any()
    for tab in (small, straddle, large):
        got, _, _ = _system_radii(b, tab, subset=subset, ref=ref)
        for s in plant:
            f, cnt = tab.np_span[s % tab.n_cond, 0]
            assert cnt > 0 and np.all(got[s // tab.n_cond, f:f + cnt] == 1e-20)


# ---- 4. at the limits ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_at_and_past_the_table_limits_with_eight_radii():
    """PEM_FUSED_SYSTEM_MAX_RECORDS conditions and records, 2048 u_ion nodes, PEM_FUSED_SYSTEM_MAX_RADII radii: 160 000 of the
    CU's 163 840 bytes of LDS; one more of each refused"""
    import torch
    rng = np.random.default_rng(2)
    R = 8
    b = _batch(64 * 33 + 5, seed=9)
    tab = _table_radii(rng, 1024, R, counts=lambda c: [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)][c % 4], big=True)
    assert tab.n_rec == 1024
    node = np.concatenate([tab.np_node, np.tile([5, 6], (2048 - tab.np_node.size) // 2)]).astype(np.int32)
    tab.np_node, tab.node, tab.n_node = node, torch.as_tensor(node, device='cuda'), node.size
    assert tab.n_node == 2048
    assert _table_bytes(tab) == 81920 and _radii_bytes(R) == 8384
    assert FAST_LDS + _table_bytes(tab) + _radii_bytes(R) == 160000 <= CU_LDS
    _system_radii(b, tab)
    out = torch.empty(b.n, dtype=torch.float64, device='cuda')
    wide = torch.empty((b.n, 1025), dtype=torch.float64, device='cuda')
    for field, v in (('n_cond', 1025), ('n_rec', 1025), ('n_node', 2049), ('sweep_radii', tuple(np.linspace(0.4, 1.6, 9)))):
        bad = SimpleNamespace(**vars(tab))
        setattr(bad, field, v)
        bad.rec = torch.zeros((1025, 4), dtype=torch.float64, device='cuda')
        bad.span = torch.zeros((1025, 4, 2), dtype=torch.int32, device='cuda')
        bad.node = torch.zeros(2049, dtype=torch.int32, device='cuda')
        _assert_refused(lambda: b.run_system_loglik(bad, out=out))
        _assert_refused(lambda: b.run_system_predict(bad, wide))


# ---- 5. radius indices past the table -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('R', [3, 8])
def test_radius_index_past_the_table_is_the_last_radius(R):
    """records with ridx = R, 200 and 255 predict and sum bit for bit as with ridx = R - 1"""
    import torch
    rng = np.random.default_rng(300 + R)
    tab = _table_radii(rng, 9, R, counts=lambda c: (2 * c + 1, c % 2, 1, c % 3))
    at_last = np.flatnonzero(tab.np_ridx == R - 1)
    assert at_last.size >= 6
    ridx = tab.np_ridx.copy()
    ridx[at_last] = np.resize([R, 200, 255], at_last.size)
    past = _with_ridx(tab, ridx)
    assert not np.array_equal(past.np_rec.view(np.int64), tab.np_rec.view(np.int64))
    b = _batch(64 * 2 + 31, seed=5)
    res = []
    for t in (tab, past):
        pred = torch.full((-(-b.n // t.n_cond), t.n_rec), SENTINEL, dtype=torch.float64, device='cuda')
        b.run_system_predict(t, pred)
        ll = torch.full((b.n,), np.nan, dtype=torch.float64, device='cuda')
        b.run_system_loglik(t, out=ll)
        res.append((pred.cpu().numpy(), ll.cpu().numpy()))
    assert np.isfinite(res[0][1]).all()
    assert np.array_equal(res[0][0].view(np.int64), res[1][0].view(np.int64))
    assert np.array_equal(res[0][1].view(np.int64), res[1][1].view(np.int64))
    # and the last radius is not any radius: the same records one radius in give other values
    ridx[at_last] = R - 2
    other = _with_ridx(tab, ridx)
    pred = torch.full(res[0][0].shape, SENTINEL, dtype=torch.float64, device='cuda')
    b.run_system_predict(other, pred)
    assert not np.array_equal(pred.cpu().numpy().view(np.int64), res[0][0].view(np.int64))


# ---- 6. non-physical pairs ----------------------------------------------------------------------------------------------------
def _scan_c5(I_B0, radii, scan, pick):
    """the middle one of the c5 of `scan` (no pressure dependence: c2 = c4 = 0, so the neutral density is c5 itself) at which the
    oracle's terms and flags satisfy `pick(terms, invalid over all radii, invalid at the first radius alone)`"""
    from hallthrusterpem_amd import constants
    from oracle import oracle_ctypes as oc
    kw = dict(P_b=np.full(scan.size, 1e-5), c0=0.3, c1=0.5, c2=0.0, c3=0.6, c4=0.0, c5=scan, sigma_cex=55e-20, I_B0=I_B0,
              torr2pa=constants.TORR_2_PA)
    with np.errstate(all='ignore'):
        hit = np.flatnonzero(pick(oc.plume_terms(**kw, radii=radii), oc.plume(**kw, radii=radii)['invalid'],
                                  oc.plume(**kw, radii=radii[:1])['invalid']))
    assert hit.size >= 3
    return scan[hit[hit.size // 2]]


@pytest.mark.gpu
def test_non_physical_pairs_beside_prior_draws():
    """mdot_a = 0 (base = j_cex = 0 at every radius: every record 1e-20, div_angle NaN); a negative neutral density whose j_ion
    goes non-positive at the far radii only, and one whose exp(+x) overflows at the far radius only (both found by scanning the
    oracle) -- each in round 0 of a tile with valid samples in the same slot of the next round and of the next tile, whose pairs
    step 1 of `_system_radii` holds to the oracle; NaN, inf and invalid patterns identical to the oracle's"""
    from _inputs import coupled_inputs
    from hallthrusterpem_amd import constants
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    from oracle import oracle_ctypes as oc
    R = 3
    radii = _radii(R)
    n = 2 * 64 + 12
    rng = np.random.default_rng(6)
    tab = _table_radii(rng, 12, R)
    d = coupled_inputs(n, seed=61)
    x = np.stack([d[k] for k in COUPLED_INPUTS])
    row = COUPLED_INPUTS.index
    zero, far, over = np.array([5, 64 + 3]), np.array([9, 64 + 10]), np.array([13, 64 + 2])
    assert all(tab.np_span[s % 12, 0, 1] > 0 for s in np.concatenate([zero, far, over]))
    x[row('mdot_a'), zero] = 0.0
    both = np.concatenate([far, over])
    I_B0 = oc.coupled(_rows(x, both), constants.TORR_2_PA)['I_B0']
    for k, v in dict(P_b=1e-5, c0=0.3, c1=0.5, c2=0.0, c3=0.6, c4=0.0, sigma_cex=55e-20).items():
        x[row(k), both] = v
    for j, s in enumerate(both):
        if s in far:      # valid at the first radius alone: decay > 1 and j_cex < 0, which grows against base with r
            x[row('c5'), s] = _scan_c5(I_B0[j], radii, np.linspace(-6e17, -0.2e17, 59), lambda t, inv, inv0: inv & ~inv0)
        else:             # exp(+r n sigma) finite at the first two radii, infinite at the last
            x[row('c5'), s] = _scan_c5(I_B0[j], radii, -np.linspace(6e20, 1.4e21, 81),
                                       lambda t, inv, inv0: np.isfinite(t['decay'][:, :-1]).all(axis=1) & np.isinf(t['decay'][:, -1]))
    # (the thruster does not see the plume's inputs)
    assert np.array_equal(oc.coupled(_rows(x, both), constants.TORR_2_PA)['I_B0'], I_B0)
    b = _batch_of(x)
    ref = _qoi_ref(x, radii)
    planted = np.concatenate([zero, far, over])
    valid_after = np.concatenate([planted + 16, planted[::2] + 64])       # the same slot one round on, and one tile on
    assert valid_after.max() < n and not np.isin(valid_after, planted).any()
    assert ref.invalid[zero].all() and ref.invalid[far].all() and not ref.invalid[valid_after].any()
    got, ll, _ = _system_radii(b, tab, ref=ref)
    assert np.isnan(ref.div[zero]).all() and np.isnan(b.qoi[1].cpu().numpy()[zero]).all()
    flag = b.invalid.cpu().numpy().astype(bool)
    for s in np.flatnonzero(flag):
        f, cnt = tab.np_span[s % 12, 0]
        assert np.all(got[s // 12, f:f + cnt] == 1e-20)
    assert flag[zero].all() and flag[far].all()
    # what the overflow does is the oracle's to say (`_system_radii` held the kinds): it is not nothing
    args = [x[row(k), over] for k in PLUME_ROWS] + [I_B0[2:], constants.TORR_2_PA]
    with np.errstate(all='ignore'):
        pl = oc.plume(*args, radii=radii)
    assert pl['invalid'].all() or not np.isfinite(pl['j_ion'][:, :, -1]).all()
    assert np.isfinite(ll[~flag & ~np.isin(np.arange(n), over)]).all()


# ---- 7. the posterior ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_system_posterior_log_likelihood_with_sweep_radii_past_two_rounds():
    """SystemPosterior.log_likelihood on the reference-shaped 16-condition table with its 40 angles spread over three sweep radii,
    K M n_cond past two rounds, against the long-double marginal of the JMODE 9 records of the same inputs -- the radii twin of
    test_likelihood_kernels.test_system_posterior_log_likelihood_past_two_rounds"""
    import torch
    from test_predictive import _reference_shaped
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    radii = _radii(3)
    data = _reference_shaped(0)
    loc = data['jion']['loc']
    loc[:, 0] = np.resize(radii, loc.shape[0])
    lik = SystemLikelihood(data, sweep_radii=radii)
    assert lik.n_cond == 16 and lik.sweep_radii == radii
    bits = np.ascontiguousarray(lik.rec.cpu().numpy()[:, 3]).view(np.int64)
    assert {0, 1, 2} <= set(bits >> 8)
    K = 4
    M = -(-_rounds_n() // (K * 16))
    names = ('T_e', 'c0', 'c1', 'c4')
    post = SystemPosterior(names, lik, n_chains=K, n_nuisance=M, fresh_nuisance=False, seed=3)
    theta = torch.tensor([[2.0, 0.3, 0.5, 1e20], [3.0, 0.6, 0.4, 3e19], [1.5, 0.1, 0.8, 2e21], [4.0, 0.9, 0.2, 5e18]],
                         dtype=torch.float64, device=post.device)
    got = post.log_likelihood(theta).cpu().numpy()
    pred = torch.full((K * M, lik.n_rec), SENTINEL, dtype=torch.float64, device=post.device)
    post.batch.run_system_predict(lik, pred)
    pred = pred.cpu().numpy()
    rec, span = lik.rec.cpu().numpy(), lik.span.cpu().numpy()
    n = K * M * 16
    ll, llb = np.zeros(n, dtype=hl.LD), np.zeros(n, dtype=hl.LD)
    for c in range(16):
        idx = np.arange(c, n, 16)
        r = np.concatenate([np.arange(span[c, kd, 0], span[c, kd, 0] + span[c, kd, 1]) for kd in range(4)])
        assert not np.any(pred[idx // 16][:, r] == SENTINEL)
        ll[idx], llb[idx] = hl.record_sum(pred[idx // 16][:, r], rec[r, 1], rec[r, 2])
    x = post.batch.inputs.cpu().numpy()
    md, a1 = (x[COUPLED_INPUTS.index(k)].reshape(K, M, 16) for k in ('mdot_a', 'a_1'))
    want, bound = hl.marginal_ref(ll.reshape(K, M, 16), llb.reshape(K, M, 16), md, a1, *post.discharge)
    assert np.isfinite(got).all()
    hl.assert_within(got, want, bound, 'SystemPosterior.log_likelihood with sweep_radii')
