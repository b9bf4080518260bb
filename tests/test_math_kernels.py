"""csrc/pem_math.h on the device, element by element, through the existing C ABI: with unit vectors as the basis a latent IS the log10 of
one field value and a reconstructed field value IS 10^(one latent), so
  pem_log10_tab      (pem_svd_compress_f64_dev, every compress kernel that instantiates the log10 norm),
  pem_exp10          (pem_svd_reconstruct_f64_dev, both reconstruct kernels),
  pem_log10_tab_pos  (pem_coupled_latent_f64_dev, the tile path of all six rank instantiations)
must equal tests/hp_math.py's restatements BIT FOR BIT over the argument sets of that module -- every operation of the source is a
correctly rounded IEEE operation written as an explicit fma, product or sum -- and the series pem_log10 (the literal path of
pem_coupled_latent_f64_dev, whose v_rcp_f64 quotient cannot be restated) must lie within LOG10_SERIES_ULPS of mpmath's log10 of the
same bits.  The restatements themselves are held to mpmath by tests/test_log_table_host.py."""
import numpy as np
import pytest

import hp_math as M
import hp_model as hp
import test_svd_kernel as tsk

pytestmark = pytest.mark.gpu
SWITCHES = ('PEM_SVD_TILED', 'PEM_SVD_NO_MFMA', 'PEM_SVD_GRID_MULT')
LATENT_RANKS = (1, 2, 3, 5, 7, 8)


@pytest.fixture(scope='module', autouse=True)
def _device():
    import torch
    from hallthrusterpem_amd import _lib
    _lib.load()
    _lib.require_device()
    torch.zeros(1, device='cuda').sum().item()


def _env(monkeypatch, env):
    for k in SWITCHES:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def _unit_basis(dof, rank):
    b = np.zeros((dof, rank))
    b[np.arange(rank), np.arange(rank)] = 1.0
    return b


def _log10_through_compress(x, dof, rank):
    """pem_log10_tab of every x: `rank` arguments per row in the first columns, the other columns 1.0 (log10 = +0 exactly)"""
    n = -(-x.size // rank)
    args = np.ones(n * rank)
    args[:x.size] = x
    y = np.ones((n, dof))
    y[:, :rank] = args.reshape(n, rank)
    return tsk._compress(y, _unit_basis(dof, rank), 'log10').reshape(-1)[:x.size]


def _same_bits(got, want, x, what):
    diff = np.flatnonzero(M.bits(got) != M.bits(want))
    assert diff.size == 0, f'{what}: {diff.size} of {got.size} results differ in their bits, first at argument {float(x[diff[0]]).hex()}: ' \
        f'got {float(got[diff[0]]).hex()} want {float(want[diff[0]]).hex()}'


def test_table_log10_in_the_default_compress_kernel(monkeypatch):
    """the whole log10 set (6.6 M arguments) through the direct kernel at the production shape, 91 angles"""
    _env(monkeypatch, {})
    x = M.log10_args()
    _same_bits(_log10_through_compress(x, 91, 16), M.restated('log10_tab'), x, 'svd_compress_direct_kernel')


# every other compress kernel that instantiates the log10 norm: dof and switches of tests/test_svd_kernel.py's regime table for the
# MFMA form, and beside it what that module's dof test reaches by PEM_SVD_NO_MFMA (ROWS = 16) and by dof > 96 (ROWS = 8), one per RT
_MFMA = tsk.KERNELS['mfma']
assert _MFMA[4] == 'log10' and tsk.KERNELS['direct'][4] == 'log10' and tsk.KERNELS['direct'][5] == {}
VARIANTS = [('mfma', _MFMA[2], 16, _MFMA[5]), ('mfma rank 5', _MFMA[2], 5, _MFMA[5])]
VARIANTS += [(f'tiled16 RT {rt}', 91, rt, dict(_MFMA[5], PEM_SVD_NO_MFMA='1')) for rt in (4, 8, 16)]
VARIANTS += [(f'tiled8 RT {rt}', tsk.KERNELS['tiled8'][2], rt, {}) for rt in (4, 8, 16)]
VARIANTS += [('direct dof 17 rank 3', 17, 3, {})]


@pytest.mark.parametrize('name,dof,rank,env', VARIANTS, ids=[v[0] for v in VARIANTS])
def test_table_log10_in_every_other_compress_kernel(name, dof, rank, env, monkeypatch):
    """the edge subset: every table entry and both sides of each of its edges in twelve binades, denormal ones included"""
    _env(monkeypatch, env)
    x = M.log10_edge_args()
    _same_bits(_log10_through_compress(x, dof, rank), M.log10_tab(x), x, name)


@pytest.mark.parametrize('name,dof,rank,env', [('direct', 91, 16, {})] + VARIANTS[:1] + VARIANTS[2:3] + VARIANTS[5:6], ids=['direct', 'mfma', 'tiled16', 'tiled8'])
def test_table_log10_special_values(name, dof, rank, env, monkeypatch):
    """one per row (a special value poisons the other columns of its row): +-0 -> -inf, negative -> NaN, +inf -> +inf, NaN -> NaN"""
    _env(monkeypatch, env)
    y = np.ones((len(M.LOG10_SPECIALS) + 2, dof))
    y[1:-1, 0] = M.LOG10_SPECIALS
    y[0, :rank] = y[-1, :rank] = 1e-20
    got = tsk._compress(y, _unit_basis(dof, rank), 'log10')
    assert np.array_equal(got[1:-1, 0], np.array(M.LOG10_SPECIALS_WANT), equal_nan=True), got[1:-1, 0]
    assert (got[0] == -20.0).all() and (got[-1] == -20.0).all()


def _exp10_through_reconstruct(z, dof, rank):
    n = -(-z.size // rank)
    lat = np.zeros((n, rank))
    lat.reshape(-1)[:z.size] = z
    got = tsk._reconstruct(lat, _unit_basis(dof, rank), 'log10')
    assert (got[:, rank:] == 1.0).all()
    return np.ascontiguousarray(got[:, :rank]).reshape(-1)[:z.size]


def test_exp10_in_the_reconstruct_kernel():
    """the whole 10^x set through svd_reconstruct_kernel<LOG10, true> at 91 angles: every result, the denormal ones and the ones past
    the clamps included, as ONE rounding of the polynomial's value gives it"""
    z = M.exp10_args()
    want = M.restated('exp10')
    assert ((want > 0) & (want < 2.2250738585072014e-308)).sum() > 1000 and (want == 0).any() and np.isinf(want).any()
    _same_bits(_exp10_through_reconstruct(z, 91, 16), want, z, 'svd_reconstruct_kernel<LOG10, true>')


def test_exp10_in_the_lds_reconstruct_kernel():
    """dof > 96: svd_reconstruct_kernel<LOG10, false>; the structured part of the set and 50 000 of the random ones"""
    z = M.exp10_args()[:M.exp10_args().size - 1_150_000]
    _same_bits(_exp10_through_reconstruct(z, 97, 8), M.restated('exp10')[:z.size], z, 'svd_reconstruct_kernel<LOG10, false>')


@pytest.mark.parametrize('dof,rank', [(91, 16), (97, 8)])
def test_exp10_special_values(dof, rank):
    """NaN -> NaN, +inf -> inf, -inf -> 0, at and beyond the clamps 0 / inf; one per row"""
    lat = np.zeros((len(M.EXP10_SPECIALS), rank))
    lat[:, 0] = M.EXP10_SPECIALS
    got = tsk._reconstruct(lat, _unit_basis(dof, rank), 'log10')
    assert np.array_equal(got[:, 0], np.array(M.EXP10_SPECIALS_WANT), equal_nan=True), got[:, 0]
    finite = np.isfinite(lat[:, 0])
    assert (got[finite, 1:] == 1.0).all()


# ---- the fused latent kernel: pem_log10_tab_pos on the tile path, the series pem_log10 on the literal path ----------------------------
def _angle_groups(rank):
    """groups of `rank` angles that together visit all 91"""
    starts = list(range(0, hp.NANG - rank + 1, rank))
    if starts[-1] + rank < hp.NANG:
        starts.append(hp.NANG - rank)
    return [np.arange(s, s + rank) for s in starts]


def _profile_and_its_log10(x, rank):
    """(j_ion (n, 91) as the `none` launch returns it through unit vectors, its log10 as the `log10` launch does, invalid flags)"""
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    from hallthrusterpem_amd.compression import SVDCompression
    n = len(x['P_b'])
    batch = CoupledBatch(n, profile=False)
    batch.set_inputs({q: torch.from_numpy(v) for q, v in x.items()})
    J, L = np.full((n, hp.NANG), np.nan), np.full((n, hp.NANG), np.nan)
    for angles in _angle_groups(rank):
        basis = np.zeros((hp.NANG, rank))
        basis[angles, np.arange(rank)] = 1.0
        for norm, out in (('none', J), ('log10', L)):
            comp = SVDCompression(norm=norm, rank=rank)
            comp.basis = torch.from_numpy(basis).cuda()
            out[:, angles] = batch.run_latent(comp).cpu().numpy()
    return J, L, batch.outputs()['invalid'].cpu().numpy().astype(bool)


def _classify(J, invalid):
    """tile: certainly the recurrence loop (every value finite, the smallest at least twice the switch); literal: certainly
    literal_sample (the smallest below half the switch).  In between either: the switch is decided on the recurrence's values,
    which the literal path's output does not show."""
    with np.errstate(all='ignore'):
        positive = np.isfinite(J).all(axis=1) & (J > 0).all(axis=1) & ~invalid
        tile = positive & (J.min(axis=1) >= 2.0 * hp.SWITCH) & (J.max(axis=1) < 1e290)
        literal = positive & (J.min(axis=1) < 0.5 * hp.SWITCH)
    return positive, tile, literal


@pytest.mark.parametrize('rank', LATENT_RANKS)
def test_table_log10_on_the_tile_path_of_the_fused_latent_kernel(rank):
    """2 000 samples under the PEM-v0 priors: the `none` launch returns j_ion[k] itself (the other 90 terms are fma(finite, 0, acc)),
    the `log10` launch pem_log10_tab_pos of the same bits"""
    J, L, invalid = _profile_and_its_log10(hp.prior_set(2000, seed=11), rank)
    positive, tile, literal = _classify(J, invalid)
    assert tile.sum() >= 1900 and not literal.any()
    _same_bits(L[tile], M.log10_tab(J[tile]), J[tile], f'coupled_latent_kernel<{rank}, true>')
    assert (L[invalid] == -20.0).all() and (J[invalid] == 1e-20).all()


@pytest.mark.parametrize('rank', LATENT_RANKS)
def test_series_log10_on_the_literal_path(rank):
    """hp_model's deep-tail inputs (the smallest j_ion below 1e-290): some samples take literal_sample, and there the series log10 --
    with the device's own quotient -- lies within LOG10_SERIES_ULPS of mpmath's log10 of the same bits; it is NOT the table version
    (bits differ); the samples that stay on the tile path equal the table version bit for bit; an invalid sample's latents are
    exactly -20 per column of a unit basis"""
    J, L, invalid = _profile_and_its_log10(hp.tail_set(), rank)
    positive, tile, literal = _classify(J, invalid)
    print(f'rank {rank}: {tile.sum()} tile, {literal.sum()} literal, {(positive & ~tile & ~literal).sum()} either, {invalid.sum()} invalid of {len(J)}')
    assert literal.sum() >= 50 and tile.sum() >= 50 and invalid.sum() >= 5
    _same_bits(L[tile], M.log10_tab(J[tile]), J[tile], f'coupled_latent_kernel<{rank}, true>, tile path')
    w = M.worst_error(J[literal], L[literal], 'log10', M.LOG10_SERIES_ULPS)
    differ = (M.bits(L[literal]) != M.bits(M.log10_tab(J[literal]))).sum()
    print(f'rank {rank}: series log10 on {literal.sum() * hp.NANG} values, worst {w["normal"][0]:.4f} ulp at {w["normal"][1].hex()}; {differ} differ from the table version')
    assert np.isfinite(L[literal]).all() and w['normal'][0] <= M.LOG10_SERIES_ULPS
    assert differ > 0, 'the literal path gave the table version bit for bit: the series did not run'
    either = positive & ~tile & ~literal
    if either.any():
        assert M.worst_error(J[either], L[either], 'log10', M.LOG10_SERIES_ULPS)['normal'][0] <= M.LOG10_SERIES_ULPS
    assert (L[invalid] == -20.0).all() and (J[invalid] == 1e-20).all()
