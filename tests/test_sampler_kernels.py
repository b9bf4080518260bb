"""csrc/pem_sampler.hip and the thruster filter at their edges, against plain references: the three design kernels (Monte-Carlo,
Latin hypercube, tile-interleaved) against the numpy restatement oracle/sampler_np.py, the Saltelli partial sums against long
double (tests/hp_sampler.py), the predictive inputs and noise against the Philox restatement, the wave argmax of
pem_thruster_filter_f64_dev against np.argmax.

The shapes are the smallest that reach a path: past the grid caps (4096 workgroups of 256 threads, 16 384 waves) so that the
grid-stride loops make a second pass, across a multiple of 2^32 of the sample index, a seed and a stream whose every word
counts, Latin-hypercube domains at, below and above 4^h filled in shards, both members of a Saltelli pair, every `ndim` class,
leading dimensions wider than the data with the padding watched.

Tolerances of the designs are the project's: uniform dimensions bit-equal, log-uniform within 4e-15 relative, normal within
1e-12 b absolute (tests/test_sampler.py, tests/test_device_dram.py)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import hp_sampler as hs
from oracle import sampler_np as snp

SEED = (0x9E3779B9 << 32) | 0x7F4A7C15
SEED_OTHER_HIGH = (0x85EBCA6B << 32) | 0x7F4A7C15      # the same low word
STREAM = 0xFFFFFFFE
SENTINEL = -12345.5
FIRST = 2 ** 32 - 70                                    # a batch of more than 70 samples crosses a multiple of 2^32
LOG_REL, NORMAL_ABS = 4e-15, 1e-12
M32 = np.uint64(0xFFFFFFFF)
pytestmark = pytest.mark.gpu


def _lib():
    from hallthrusterpem_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _h(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _ok(rc):
    assert rc == 0, _lib().load().pem_last_error()


def _design(ndim, seed=SEED, stream=STREAM, kinds=(snp.UNIFORM, snp.LOGUNIFORM, snp.NORMAL)):
    """a design of ndim dimensions whose kinds cycle through `kinds`, every dimension with a table row of its own"""
    from hallthrusterpem_amd.sampling import Design, Prior
    rows = {snp.UNIFORM: lambda d: (-0.25 - 1.5 * d, 2.0 + d), snp.LOGUNIFORM: lambda d: (-8.0 + 0.125 * d, -4.0 + 0.25 * d),
            snp.NORMAL: lambda d: (30.0 - d, 2.0 + 0.5 * (d % 4))}
    names = tuple(f'x{d}' for d in range(ndim))
    priors = {k: Prior(kinds[d % len(kinds)], *rows[kinds[d % len(kinds)]](d), 'test') for d, k in enumerate(names)}
    return Design(priors=priors, names=names, seed=seed, stream=stream)


def _want(ds, n, first, **kw):
    return snp.sample(n, first, ds.seed, ds.stream, ds.kind, ds.a, ds.b, **kw)


def _errors(got, want, kind, b):
    """the largest error of each kind present: 'uniform' counts unequal entries, 'log' is relative, 'normal' in units of b"""
    err = {}
    for d in range(len(kind)):
        if kind[d] == snp.UNIFORM:
            err['uniform'] = err.get('uniform', 0) + int(np.sum(got[d] != want[d]))
        elif kind[d] == snp.LOGUNIFORM:
            err['log'] = max(err.get('log', 0.0), float(np.max(np.abs(got[d] / want[d] - 1))))
        else:
            err['normal'] = max(err.get('normal', 0.0), float(np.max(np.abs(got[d] - want[d])) / b[d]))
    return err


def _assert_design(got, want, ds, what):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = _errors(got, want, ds.kind, ds.b)
    print(f'{what}: {err}')
    assert err.get('uniform', 0) == 0 and err.get('log', 0.0) < LOG_REL and err.get('normal', 0.0) < NORMAL_ABS, (what, err)
    return err


def _fill_slice(ds, n, pad=(5, 6), **kw):
    """the design written into columns pad[0] .. pad[0] + n of a wider sentinel tensor; everything else must stay"""
    import torch
    big = torch.full((ds.ndim, pad[0] + n + pad[1]), SENTINEL, dtype=torch.float64, device='cuda')
    ds.fill(big[:, pad[0]:pad[0] + n], **kw)
    big = big.cpu().numpy()
    assert np.all(big[:, :pad[0]] == SENTINEL) and np.all(big[:, pad[0] + n:] == SENTINEL), 'the padding was written'
    return big[:, pad[0]:pad[0] + n]


# ---- the Monte-Carlo design -----------------------------------------------------------------------------------------------------
def test_mc_second_pass_of_the_grid_and_the_index_wrap_and_the_normal_tail():
    """n = 2^20 + 300 samples from first = 2^32 - 70: past sample_kernel's grid cap (4096 x 256 threads: 300 threads make a
    second pass) and across a multiple of 2^32 of the index, dimensions (uniform, log-uniform, normal).  The normal row at this
    size reaches |z| = 4.9: its 64 smallest, 64 largest and 64 random u are also held to the quantile at 40 digits (mpmath)
    under the same 1e-12 b.

    Largest errors measured on an MI355X: uniform 0 unequal entries (held to 0); log-uniform 2.2e-16 relative (held to
    4e-15); normal 2.4e-15 b against scipy's ndtri over the whole row and 2.7e-15 b against mpmath over the 192 picked values,
    |z| <= 4.87 (both held to 1e-12 b)."""
    n = 2 ** 20 + 300
    ds = _design(3)
    got = _fill_slice(ds, n, first_index=FIRST)
    _assert_design(got, _want(ds, n, FIRST), ds, 'mc n = 2^20 + 300')
    g = np.arange(FIRST, FIRST + n, dtype=np.uint64)
    r = snp.philox4x32_10(g & M32, g >> np.uint64(32), 1, ds.stream, ds.seed & 0xFFFFFFFF, ds.seed >> 32)
    u = snp.u53(r[0], r[1])                                          # dimension 2 is the even member of pair 1
    order = np.argsort(u, kind='stable')
    pick = np.concatenate([order[:64], order[-64:], np.random.default_rng(5).choice(n, 64, replace=False)])
    assert u[pick].min() > 0.0 and u[order[0]] < 1e-5 and u[order[-1]] > 1 - 1e-5
    want = hs.LD(ds.a[2]) + hs.LD(ds.b[2]) * hs.ndtri_mp(u[pick])
    err = float(np.max(np.abs(got[2][pick].astype(hs.LD) - want)) / ds.b[2])
    print(f'normal tail against mpmath: {err:.3g} b over |z| <= {float(np.max(np.abs((want - ds.a[2]) / ds.b[2]))):.2f}')
    assert err < NORMAL_ABS


@pytest.mark.parametrize('ndim', [32, 31, 2, 1])
def test_mc_every_dimension_count_into_a_slice_of_a_wider_tensor(ndim):
    ds = _design(ndim)
    got = _fill_slice(ds, 257, first_index=FIRST)
    _assert_design(got, _want(ds, 257, FIRST), ds, f'mc ndim = {ndim}')


@pytest.mark.parametrize('ndim', [15, 8])
def test_mc_saltelli_blocks_of_both_members_of_a_pair_and_the_lone_last_dimension(ndim):
    ds, n = _design(ndim), 130
    blocks = {sd: _fill_slice(ds, n, first_index=FIRST, swap_dim=sd) for sd in (-1, -2, 0, 1, 6, 7, ndim - 1)}
    for sd, got in blocks.items():
        _assert_design(got, _want(ds, n, FIRST, swap_dim=sd), ds, f'mc ndim = {ndim} swap_dim = {sd}')
    A, B = blocks[-1], blocks[-2]
    for d in range(ndim):
        assert not np.array_equal(A[d], B[d])
    for sd, AB in blocks.items():
        if sd >= 0:
            assert np.array_equal(AB[sd], B[sd]), sd
            for e in range(ndim):
                assert e == sd or np.array_equal(AB[e], A[e]), (sd, e)


def test_mc_stream_plus_one_wraps():
    n = 130
    last, zero = _design(15, stream=0xFFFFFFFF), _design(15, stream=0)
    B = _fill_slice(last, n, first_index=FIRST, swap_dim=-2)
    assert np.array_equal(B, _fill_slice(zero, n, first_index=FIRST))
    assert not np.array_equal(B, _fill_slice(last, n, first_index=FIRST))
    _assert_design(B, _want(last, n, FIRST, swap_dim=-2), last, 'stream 0xFFFFFFFF, matrix B')
    assert np.array_equal(_want(last, n, FIRST, swap_dim=-2), _want(zero, n, FIRST))


@pytest.mark.parametrize('ndim', [15, 4, 31])
def test_tiled_layout_equals_the_soa_design_and_leaves_the_ragged_tile_alone(ndim):
    import torch
    ds = _design(ndim)
    for n, sd in itertools.product((1, 64, 65, 200), (-1, 3)):
        soa = _fill_slice(ds, n, first_index=FIRST, swap_dim=sd)
        _assert_design(soa, _want(ds, n, FIRST, swap_dim=sd), ds, f'soa ndim = {ndim} n = {n} swap_dim = {sd}')
        tiles = -(-n // 64)
        tiled = torch.full((tiles + 1, ndim, 64), SENTINEL, dtype=torch.float64, device='cuda')   # one tile more than written
        ds.fill_tiled(tiled[:tiles], n, first_index=FIRST, swap_dim=sd)
        flat = tiled.permute(1, 0, 2).reshape(ndim, -1).cpu().numpy()
        assert np.array_equal(flat[:, :n], soa), (n, sd)
        assert np.all(flat[:, n:] == SENTINEL), (n, sd)


# ---- the Latin hypercube ----------------------------------------------------------------------------------------------------------
LHS_KINDS = (snp.UNIFORM, snp.LOGUNIFORM)      # five dimensions: U, logU, U, logU and a lone last U


@functools.lru_cache(maxsize=None)
def _lhs_reference(n_total, seed):
    ds = _design(5, seed=seed, kinds=LHS_KINDS)
    want = _want(ds, n_total, 0, mode='lhs', n_total=n_total)
    want.setflags(write=False)
    return want


def _strata(x, ds, n_total):
    """the stratum of every value, recovered from the value: floor(n_total u)"""
    u = np.empty_like(x)
    for d in range(ds.ndim):
        v = np.log10(x[d]) if ds.kind[d] == snp.LOGUNIFORM else x[d]
        u[d] = (v - ds.a[d]) / (ds.b[d] - ds.a[d])
    return np.floor(u * n_total).astype(np.int64)


@pytest.mark.parametrize('seed', [SEED, SEED_OTHER_HIGH], ids=['seed', 'other_high_word'])
@pytest.mark.parametrize('n_total', [1, 2, 3, 4, 5, 16, 17, 64, 65, 256, 257, 4096])
def test_lhs_in_three_shards_at_and_around_the_feistel_domains(n_total, seed):
    """n_total = 4^h is the boundary of the half_bits loop (no cycle walking), 1, 2, 3 the tiny domains; the design is filled
    by one call per shard [0, n/3), [n/3, 2n/3), [2n/3, n) with first_index > 0, the last ending exactly at n_total."""
    import torch
    ds = _design(5, seed=seed, kinds=LHS_KINDS)
    out = torch.full((5, n_total + 3), SENTINEL, dtype=torch.float64, device='cuda')
    cuts = [0, n_total // 3, 2 * n_total // 3, n_total]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:                                               # an empty shard is no call
            ds.fill(out[:, lo:hi], first_index=lo, method='lhs', n_total=n_total)
    out = out.cpu().numpy()
    assert np.all(out[:, n_total:] == SENTINEL)
    got, want = out[:, :n_total], _lhs_reference(n_total, seed)
    _assert_design(got, want, ds, f'lhs n_total = {n_total}')
    cells = _strata(got, ds, n_total)
    for d in range(5):
        assert np.array_equal(np.sort(cells[d]), np.arange(n_total)), d       # every stratum once
    if n_total >= 16:
        for d, e in itertools.combinations(range(5), 2):
            assert not np.array_equal(cells[d], cells[e]), (d, e)             # no two dimensions share a permutation
        if seed != SEED:                                                       # the high word of the seed keys the permutation
            other = _strata(_lhs_reference(n_total, SEED), ds, n_total)
            for d in range(5):
                assert not np.array_equal(cells[d], other[d]), d


# ---- the Saltelli partial sums --------------------------------------------------------------------------------------------------
def _sobol_data(nq, m, seed, cancel=True):
    """fA, fB, fAB [nq][m]: magnitudes 1e-3 .. 1e3 of either sign; in every fifth column fAB - fA cancels to 1e-12 of fA"""
    rng = np.random.default_rng(seed)
    draw = lambda: rng.choice([-1.0, 1.0], (nq, m)) * 10.0 ** rng.uniform(-3, 3, (nq, m))      # noqa: E731
    fA, fB, fAB = draw(), draw(), draw()
    if cancel:
        col = np.arange(m) % 5 == 0
        fAB[:, col] = fA[:, col] * (1.0 + 1e-12 * rng.uniform(-1, 1, (nq, int(col.sum()))))
    return fA, fB, fAB


def _padded(x, ld):
    """x [nq][m] as the first rows and columns of an [8][ld] NaN table on the device: a read past m or nq shows"""
    import torch
    t = torch.full((8, ld), np.nan, dtype=torch.float64, device='cuda')
    t[:x.shape[0], :x.shape[1]] = torch.from_numpy(x)
    return t


def _sobol_partial(fA, fB, fAB, m, nq, ld, n_blocks):
    import torch
    partial = torch.full((n_blocks, nq, 2), np.nan, dtype=torch.float64, device='cuda')
    _ok(_lib().load().pem_sobol_partial_f64_dev(m, nq, ld, _p(fA), _p(fB), _p(fAB), _p(partial), n_blocks, _stream()))
    return partial.cpu().numpy()


@pytest.mark.parametrize('with_ab', [False, True], ids=['mean_variance', 'first_total'])
@pytest.mark.parametrize('m, n_blocks', [(1, 4), (255, 1), (256 * 3 + 5, 2), (256 * 3 + 5, 7)])
@pytest.mark.parametrize('nq', [1, 3, 8])
def test_sobol_partial_against_long_double(nq, m, n_blocks, with_ab):
    """The bound is 1.01 C u S, S the sum of |a| + |b|, a^2 + b^2, |b| |ab - a|, (a - ab)^2; C = L + 6 + 4 + (the roundings that
    form a term), L = ceil(m / (256 n_blocks)) -- derived in hp_sampler.sobol_roundings.  (773, 2) makes a second pass of the
    stride loop, (1, 4) and (773, 7) have workgroups without a sample, which must write zeros.  Measured on an MI355X: the
    largest error over the 24 cases is 0.12 of its bound."""
    ld = m + 3
    fA, fB, fAB = _sobol_data(nq, m, seed=100 * nq + m + n_blocks)
    dA, dB, dAB = _padded(fA, ld), _padded(fB, ld), (_padded(fAB, ld) if with_ab else None)
    got = _sobol_partial(dA, dB, dAB, m, nq, ld, n_blocks)
    assert not np.isnan(got).any(), 'a partial was not written, or a pad column was read'
    empty = np.arange(n_blocks) * hs.SOBOL_BLOCK >= m
    assert np.all(got[empty] == 0.0)
    want, bound = hs.sobol_partial_ref(fA, fB, fAB if with_ab else None, n_blocks)
    total = got.astype(hs.LD).sum(axis=0)
    worst = float(np.max(np.abs(total - want) / bound))
    print(f'nq = {nq} m = {m} n_blocks = {n_blocks} fAB = {with_ab}: worst error / bound {worst:.3g}')
    assert np.all(np.abs(total - want) <= bound), worst
    again = _sobol_partial(dA, dB, dAB, m, nq, ld, n_blocks)
    assert np.array_equal(got, again)


def test_sobol_partial_of_an_input_the_qoi_does_not_see_is_exactly_zero():
    m, nq, n_blocks = 256 * 3 + 5, 3, 2
    fA, fB, _ = _sobol_data(nq, m, seed=9, cancel=False)
    got = _sobol_partial(_padded(fA, m + 3), _padded(fB, m + 3), _padded(fA.copy(), m + 3), m, nq, m + 3, n_blocks)
    assert np.all(got == 0.0)


def test_sobol_partial_refuses_malformed_calls():
    import torch
    lib = _lib()
    t = torch.zeros((8, 16), dtype=torch.float64, device='cuda')
    partial = torch.full((4, 8, 2), SENTINEL, dtype=torch.float64, device='cuda')
    for m, nq, ld, n_blocks in [(10, 0, 16, 4), (10, 9, 16, 4), (10, 3, 16, 0), (10, 3, 9, 4)]:
        rc = lib.load().pem_sobol_partial_f64_dev(m, nq, ld, _p(t), _p(t), _p(t), _p(partial), n_blocks, _stream())
        assert rc == lib.PEM_ERR_INVALID_ARG, (m, nq, ld, n_blocks)
    torch.cuda.synchronize()
    assert torch.all(partial == SENTINEL)


# ---- the predictive noise and inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_rows, m', [(30_001, 37), (257, 5), (257, 1)])
def test_predictive_noise_restates_counter_based_normals(n_rows, m):
    """30 001 x 37 elements are more than predictive_noise_kernel's 2^20 threads; rows start at 2^32 - 100, both leading
    dimensions are wider than m (pred's padding NaN, out's a sentinel that must stay), the seed has a high word.  Measured on
    an MI355X: the largest difference is 4.4e-15, under rtol 1e-9 and atol 1e-12 max(sigma) = 2e-12."""
    import torch
    from scipy.special import ndtri
    rng = np.random.default_rng(m)
    first, stream, ld_pred, ld_out = 2 ** 32 - 100, 5, m + 2, m + 5
    pred, sigma = rng.normal(size=(n_rows, m)), rng.uniform(0.1, 2.0, m)
    dpred = torch.full((n_rows, ld_pred), np.nan, dtype=torch.float64, device='cuda')
    dpred[:, :m] = torch.from_numpy(pred)
    out = torch.full((n_rows, ld_out), SENTINEL, dtype=torch.float64, device='cuda')
    _ok(_lib().load().pem_predictive_noise_f64_dev(n_rows, m, _p(dpred), ld_pred, _p(_dev(sigma)), first, SEED, stream, _p(out),
                                                   ld_out, _stream()))
    out = out.cpu().numpy()
    assert np.all(out[:, m:] == SENTINEL)
    g = np.arange(first, first + n_rows, dtype=np.uint64)[:, None]
    j = np.arange(m, dtype=np.uint64)[None, :]
    w = snp.philox4x32_10(g & M32, g >> np.uint64(32), j, stream, SEED & 0xFFFFFFFF, SEED >> 32)
    want = sigma * ndtri(snp.u53(w[0], w[1]))
    got = out[:, :m] - pred
    print(f'noise {n_rows} x {m}: largest difference {float(np.max(np.abs(got - want))):.3g}')
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * float(sigma.max()))      # test_noise_restates_counter_based_normals


OP_ROWS = (0, 1, 6)                                # P_b, V_a, mdot_a
FREE_ROWS = tuple(d for d in range(15) if d not in OP_ROWS)
THETA_STREAM = 0x80000003


@pytest.mark.parametrize('n, n_cond, theta', [(300, 1, 'table'), (300, 7, 'table'), (300, 1, 'prior'), (300, 7, 'prior'),
                                              (300, 7, 'table of four'), (2 ** 20 + 11, 7, 'table')])
def test_predictive_inputs_restate_the_design_the_operating_rows_and_the_theta_index(n, n_cond, theta):
    """Operating rows, table rows and drawn rows as tests/test_predictive.py compares them, by direct calls: a table of
    S = 100 003 rows over every free input (reversed, so that column j is not row j), the same rows drawn from the prior when
    there is no table, four of them from a table and the rest drawn; indices from 2^32 - 70; n = 2^20 + 11 makes a second pass
    of the stride loop."""
    import torch
    from hallthrusterpem_amd.sampling import NORMAL, PEM_V0_PRIORS, Design, Prior
    ds = Design(priors=dict(PEM_V0_PRIORS, V_vac=Prior(NORMAL, 30.0, 2.0, 'test')), seed=SEED, stream=STREAM)
    rng = np.random.default_rng(n_cond)
    S = 100_003
    rows = np.ascontiguousarray((FREE_ROWS[::-1] if theta != 'table of four' else (2, 8, 7, 14)), dtype=np.int32)
    table = None if theta == 'prior' else rng.uniform(size=(S, rows.size))
    operating = np.stack([10.0 ** rng.uniform(-6, -4.5, n_cond), rng.uniform(250, 350, n_cond), rng.uniform(4e-6, 6e-6, n_cond)], axis=1)
    dtable, dop = (None if table is None else _dev(table)), _dev(operating)
    out = torch.full((15, n + 3), SENTINEL, dtype=torch.float64, device='cuda')
    _ok(_lib().load().pem_predictive_inputs_f64_dev(n, n_cond, FIRST, SEED, STREAM, _h(ds.kind), _h(ds.a), _h(ds.b), _p(dop), _p(dtable),
                                                    0 if table is None else S, rows.size, _h(rows), THETA_STREAM, _p(out), n + 3, _stream()))
    out = out.cpu().numpy()
    assert np.all(out[:, n:] == SENTINEL)
    x = out[:, :n]
    g = np.arange(FIRST, FIRST + n, dtype=np.uint64)
    drawn = [d for d in range(15) if d not in OP_ROWS and (table is None or d not in rows)]
    if drawn:
        want = _want(ds, n, FIRST)
        sub = lambda v: np.asarray(v)[drawn]                                                # noqa: E731
        err = _errors(x[drawn], want[drawn], sub(ds.kind), sub(ds.b))
        print(f'drawn rows: {err}')
        assert err.get('uniform', 0) == 0 and err.get('log', 0.0) < LOG_REL and err.get('normal', 0.0) < NORMAL_ABS, err
    for k, d in enumerate(OP_ROWS):
        assert np.array_equal(x[d], operating[np.arange(n) % n_cond, k]), d
    if table is not None:
        w = snp.philox4x32_10(g & M32, g >> np.uint64(32), 0, THETA_STREAM, SEED & 0xFFFFFFFF, SEED >> 32)[0]
        idx = ((w * np.uint64(S)) >> np.uint64(32)).astype(np.int64)
        assert idx.min() < S // 50 and idx.max() > S - S // 50
        for j, d in enumerate(rows):
            assert np.array_equal(x[d], table[idx, j]), d


# ---- the thruster filter ----------------------------------------------------------------------------------------------------------
def _filter_rows(ncells, n, seed):
    """(u_ion, z, k): random rows with the edges of the wave argmax doctored in; z rises, so z[arg] < z[k] iff arg < k"""
    rng = np.random.default_rng(seed)
    u = 1e4 * rng.normal(size=(n, ncells))
    z = np.linspace(0.0, 0.08, ncells) if ncells > 1 else np.array([0.04])
    k = ncells // 2
    row = iter(range(3, n, 2))                       # doctored rows, random ones between them

    def put(*cells):
        r = next(row)
        top = u[r].max() + 1.0
        for c, v in cells:
            u[r, c] = top if v == 'max' else v
        return r

    nan, inf = np.nan, np.inf
    lo, hi = max(k - 30, 0), min(k + 30, ncells - 1)
    if ncells >= 33:                                 # the maximum twice, in two lanes: an odd lane first, an even lane second
        assert 5 < k <= k + k % 2 < ncells and (k + k % 2 - 5) % 64
        put((5, 'max'), (k + k % 2, 'max'))
    if ncells >= 65:                                 # the maximum twice in one lane: c and c + 64
        c = min(k - 1, ncells - 65)
        assert 0 <= c < k <= c + 64 < ncells
        put((c, 'max'), (c + 64, 'max'))
    if ncells >= 2:
        assert lo < k <= hi
        put((lo, nan), (hi, 'max'))                  # a NaN before the maximum
        put((lo, 'max'), (hi, nan))                  # a NaN after the maximum
        put((lo, nan), (hi, nan))                    # two NaNs: the first wins
        put((lo, inf))
        put((hi, 'max'), (lo, -inf))
    if ncells >= 71:                                 # two NaNs, the first of them in the higher lane
        put((k - 41, nan), (k + 19, nan))
    put((hi, inf))
    put((k, 'max'))                                  # z[arg] == threshold: not flagged
    put((0, nan))
    u[next(row)] = -inf                              # argmax 0
    T, Ib = rng.normal(size=n), rng.normal(size=n)
    T[:3], Ib[:3] = [nan, -0.0, 1.0], [1.0, 1.0, -0.0]   # not flagged
    T[4], Ib[4] = 1.0, nan
    return u, z, k, T, Ib


def _filter_reference(u, z, threshold, T, Ib, use_shock=True):
    with np.errstate(invalid='ignore'):
        flag = ((T < 0) | (Ib < 0)).astype(np.uint8)
        if use_shock:
            flag |= 2 * (z[np.argmax(u, axis=1)] < threshold).astype(np.uint8)
    return flag


def _filter(u, z, threshold, T, Ib, use_shock=1, profile=True):
    import torch
    n, ncells = u.shape
    flags = torch.full((n + 8,), 0xEE, dtype=torch.uint8, device='cuda')
    args = [None if a is None else _dev(a) for a in ((u, z) if profile else (None, None)) + (T, Ib)]
    _ok(_lib().load().pem_thruster_filter_f64_dev(n, ncells, _p(args[0]), _p(args[1]), threshold, use_shock, _p(args[2]), _p(args[3]),
                                                  _p(flags), _stream()))
    flags = flags.cpu().numpy()
    assert np.all(flags[n:] == 0xEE)
    return flags[:n]


@pytest.mark.parametrize('ncells', [1, 63, 64, 65, 102, 200])
def test_thruster_filter_equals_numpy_at_the_edges_of_the_wave_argmax(ncells):
    n = 300
    u, z, k, T, Ib = _filter_rows(ncells, n, seed=ncells)
    zero = np.zeros(n)
    for threshold in (z[k], np.nextafter(z[k], 1.0)):               # a maximum at cell k: equal to the threshold, then below it
        want = _filter_reference(u, z, threshold, T, Ib)
        assert len(np.unique(want)) == (4 if ncells > 1 else 2), 'every flag value must occur'
        assert np.array_equal(_filter(u, z, threshold, T, Ib), want)
        assert np.array_equal(_filter(u, z, threshold, None, Ib), _filter_reference(u, z, threshold, zero, Ib))
        assert np.array_equal(_filter(u, z, threshold, T, None), _filter_reference(u, z, threshold, T, zero))
    assert np.array_equal(_filter(u, z, z[k], T, Ib, use_shock=0), _filter_reference(u, z, z[k], T, Ib, use_shock=False))
    assert np.array_equal(_filter(u, z, z[k], T, Ib, use_shock=0, profile=False), _filter_reference(u, z, z[k], T, Ib, use_shock=False))


def test_thruster_filter_second_pass_of_the_wave_stride_loop():
    """20 000 rows are more than the launch's 16 384 waves"""
    n, ncells = 20_000, 64
    u, z, k, T, Ib = _filter_rows(ncells, n, seed=7)
    u[16_384 + 5, :] = np.arange(ncells)[::-1]                      # second pass: argmax 0, flagged
    u[16_384 + 6, :] = np.arange(ncells)                            # argmax 63, not flagged
    want = _filter_reference(u, z, z[k], T, Ib)
    assert want[16_384 + 5] & 2 and not want[16_384 + 6] & 2
    assert np.array_equal(_filter(u, z, z[k], T, Ib), want)
