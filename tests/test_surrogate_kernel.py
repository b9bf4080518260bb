"""pem_surrogate.hip over its whole dispatch space, entry by entry against the long-double restatement of tests/hp_reference.py:
every register width (exact 1..4, guarded 8 at 5..8, guarded 16 at 9..16), every innermost node count, 0..4 outer dimensions with
a level-4 dimension in each outer slot, declared table maxima equal to and larger than the true ones, padded leading dimensions,
the largest LDS the launch check admits, the fused field path, and every entry point past the first round of its grid-stride loop
(2048 workgroups of 256 points)."""
import ctypes as C

import numpy as np
import pytest

import hp_reference as hr

pytestmark = pytest.mark.gpu

ROUND = 2048 * 256          # points per round of the grid-stride loop (launch_predict caps the grid at 2048 workgroups)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(D, betas, n_out, seed):
    rng = np.random.default_rng(seed)
    values = [rng.standard_normal((int(np.prod([hr.node_count(l) for l in b])), n_out)) * rng.uniform(0.5, 4.0, n_out) for b in betas]
    coefs = [float(c) for c in rng.integers(-3, 4, len(betas))]
    coefs = [c if c else 1.0 for c in coefs]
    return values, coefs


def _coords(D, n, ld, seed, hit_nodes=True):
    """[D][ld] coordinates in [-1, 1], columns past n NaN (a read past n would poison a point); some exact node hits"""
    from hallthrusterpem_amd.surrogate import nodes
    rng = np.random.default_rng(seed)
    t = np.full((D, ld), np.nan)
    t[:, :n] = rng.uniform(-1, 1, (D, n))
    if hit_nodes and n > 40:
        t[:, 0] = 0.0
        for d in range(D):
            x = nodes(1 + d % 4)
            t[d, 1:1 + x.size] = x
    return t


def _launch(fn, n, D, betas, coefs, values, n_out, t, ld, ld_out, max_active, max_level, per_grid=False):
    """run one of the two plain entry points; returns (out [n_out][ld_out] or [n_beta][n_out][ld_out], return code)"""
    import torch
    from hallthrusterpem_amd import _lib
    idx, vals = hr.index_table(betas, values)
    d_idx, d_val = torch.from_numpy(idx).cuda(), torch.from_numpy(vals).cuda()
    d_coef = torch.tensor(coefs, dtype=torch.float64, device='cuda')
    d_t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)).cuda()
    shape = (len(betas), n_out, ld_out) if per_grid else (n_out, ld_out)
    out = torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')
    rc = getattr(_lib.load(), fn)(n, D, len(betas), hr.ptr(d_idx), hr.ptr(d_coef), hr.ptr(d_val), n_out, hr.ptr(d_t), ld, hr.ptr(out),
                                  ld_out, max_active, max_level, _stream())
    torch.cuda.synchronize()
    return out, rc


# ---- the standard table: 12 coordinates, five active dimensions of level 4 -> (4 * 17 + 12) * 2048 B = 160 KiB of LDS ------------
D12 = 12
SLOT_BETAS = [hr.beta_of(D12, {})] + [hr.beta_of(D12, {3: l}) for l in (1, 2, 3, 4)] + [      # innermost 1 (constant), 3, 5, 9, 17
    hr.beta_of(D12, {0: 2, 11: 3}),                                    # one outer dimension
    hr.beta_of(D12, {1: 1, 5: 2, 9: 1}),                               # two
    hr.beta_of(D12, {2: 1, 4: 1, 6: 2, 10: 1}),                        # three
    hr.beta_of(D12, {0: 4, 1: 1, 2: 1, 3: 1, 4: 1}),                   # four, the level-4 one in outer slot 0 ..
    hr.beta_of(D12, {2: 1, 5: 4, 7: 1, 8: 1, 11: 1}),                  # .. slot 1
    hr.beta_of(D12, {1: 1, 3: 1, 6: 4, 9: 1, 10: 1}),                  # .. slot 2
    hr.beta_of(D12, {0: 1, 4: 1, 5: 1, 8: 4, 11: 1}),                  # .. slot 3
    hr.beta_of(D12, {7: 1, 8: 1, 9: 1, 10: 1, 11: 4}),                 # .. and innermost
    hr.beta_of(D12, {0: 4, 3: 4, 6: 1, 7: 1, 9: 1}),                   # two level-4 outer dimensions
]
N_STD, LD_STD, LDO_STD = 700, 709, 703


@pytest.fixture(scope='module')
def standard():
    """the standard table with 16 output columns and its long-double prediction (the n_out tests take the first columns)"""
    values, coefs = _table(D12, SLOT_BETAS, 16, seed=11)
    t = _coords(D12, N_STD, LD_STD, seed=12)
    want, bound = hr.predict_ref(SLOT_BETAS, coefs, values, t[:, :N_STD])
    return values, coefs, t, want, bound


@pytest.mark.parametrize('n_out', list(range(1, 17)))
def test_predict_every_output_width_on_the_largest_lds_table(standard, n_out):
    values, coefs, t, want, bound = standard
    vals = [np.ascontiguousarray(v[:, :n_out]) for v in values]
    out, rc = _launch('pem_sparse_predict_f64_dev', N_STD, D12, SLOT_BETAS, coefs, vals, n_out, t, LD_STD, LDO_STD, 5, 4)
    assert rc == 0
    got = out.cpu().numpy()
    assert np.isnan(got[:, N_STD:]).all()                                # nothing past n in a row of ld_out
    hr.assert_within(got[:, :N_STD], want[:n_out], bound[:n_out], f'n_out {n_out}')
    if n_out == 16:                                                      # one more coordinate does not fit the 160 KiB
        t13 = np.concatenate([t, t[:1]])
        _, rc = _launch('pem_sparse_predict_f64_dev', N_STD, D12 + 1, SLOT_BETAS, coefs, vals, n_out, t13, LD_STD, LDO_STD, 5, 4)
        assert rc == 1


@pytest.mark.parametrize('case', ['exact', 'larger', 'single', 'single_larger', 'wide32'])
def test_predict_declared_maxima_and_wide_tables(case):
    """The LDS of the outer bases is sized by the declared (max_active, max_level): equal to the table's maxima and larger;
    max_active = 1 (no outer slots at all); 32 coordinates."""
    D = 32 if case == 'wide32' else 6
    if case.startswith('single'):
        betas = [hr.beta_of(D, {})] + [hr.beta_of(D, {d: l}) for d, l in ((0, 1), (2, 4), (5, 3), (1, 2))]
        decl = (1, 4) if case == 'single' else (3, 4)
    elif case == 'wide32':
        betas = [hr.beta_of(D, {}), hr.beta_of(D, {31: 4}), hr.beta_of(D, {0: 1, 31: 2}), hr.beta_of(D, {17: 4, 30: 1, 31: 1}),
                 hr.beta_of(D, {5: 2, 16: 1})]
        decl = (3, 4)                                                    # (2 * 17 + 32) * 2048 B
    else:
        betas = [hr.beta_of(D, {}), hr.beta_of(D, {0: 2}), hr.beta_of(D, {1: 1, 4: 2}), hr.beta_of(D, {0: 1, 2: 1, 5: 2})]
        decl = (3, 2) if case == 'exact' else (5, 3)
    n_out, n = 5, 1000 + 17
    values, coefs = _table(D, betas, n_out, seed=len(case))
    t = _coords(D, n, n + 3, seed=D)
    out, rc = _launch('pem_sparse_predict_f64_dev', n, D, betas, coefs, values, n_out, t, n + 3, n + 1, *decl)
    assert rc == 0
    got = out.cpu().numpy()
    assert np.isnan(got[:, n:]).all()
    want, bound = hr.predict_ref(betas, coefs, values, t[:, :n])
    hr.assert_within(got[:, :n], want, bound, case)


# ---- past the first round: periodic coordinates, bit-equal period mates --------------------------------------------------
N_BIG = 2 * ROUND + 51_213           # > two rounds, ragged tail
PERIOD = 1000                        # not a multiple of 256: a point and its mates sit in different lanes, workgroups and rounds
D_BIG = 5
BIG_BETAS = [hr.beta_of(D_BIG, {}), hr.beta_of(D_BIG, {0: 4}), hr.beta_of(D_BIG, {1: 2, 3: 3}), hr.beta_of(D_BIG, {0: 4, 2: 1, 4: 2}),
             hr.beta_of(D_BIG, {0: 1, 1: 1, 2: 1, 3: 1, 4: 1})]


def _periodic_coords(ld):
    import torch
    base = _coords(D_BIG, PERIOD, PERIOD, seed=77)
    t = torch.full((D_BIG, ld), float('nan'), dtype=torch.float64, device='cuda')
    t[:, :N_BIG] = torch.from_numpy(base).cuda()[:, torch.arange(N_BIG, device='cuda') % PERIOD]
    return base, t


def _check_periodic(got, what):
    """every point equals its mate in the first period bit for bit: each point's arithmetic does not depend on its lane,
    workgroup or round"""
    import torch
    mate = torch.arange(N_BIG, device=got.device) % PERIOD
    same = got[..., :N_BIG] == got[..., mate]
    assert bool(same.all()), f'{what}: {int((~same).sum())} outputs differ from their period mate, first at point ' \
        f'{int(torch.nonzero(~same)[0][-1])}'


def _check_points():
    """one period, and the points around each round boundary (as positions within the period)"""
    pts = set(range(PERIOD))
    for k in (1, 2):
        pts.update(range(k * ROUND - 300, k * ROUND + 300))
    pts.update(range(N_BIG - 300, N_BIG))
    return np.array(sorted(pts))


@pytest.mark.parametrize('fn', ['pem_sparse_predict_f64_dev', 'pem_sparse_grid_values_f64_dev'])
def test_predict_past_the_first_round(fn):
    per_grid = fn == 'pem_sparse_grid_values_f64_dev'
    n_out = 2 if per_grid else 6                                         # grid values: n_beta * n_out * ld_out doubles
    values, coefs = _table(D_BIG, BIG_BETAS, n_out, seed=5)
    base, t = _periodic_coords(N_BIG + 9)
    out, rc = _launch(fn, N_BIG, D_BIG, BIG_BETAS, coefs, values, n_out, t, N_BIG + 9, N_BIG + 5, 5, 4, per_grid=per_grid)
    assert rc == 0
    assert bool(out[..., N_BIG:].isnan().all())                          # nothing past n or ld_out
    _check_periodic(out, fn)
    pts = _check_points()
    got = out[..., pts].cpu().numpy()
    want, bound = hr.predict_ref(BIG_BETAS, coefs, values, base[:, pts % PERIOD], per_grid=per_grid)
    hr.assert_within(got, want, bound, fn)


# ---- the fused field path ----------------------------------------------------------------------------------------------
DOFS = (1, 63, 64, 65, 91, 130)


def _field_case(rank):
    """rank 1..16 -> (norm, scale, lat0, n_out, dof, declared maxima): every norm, latents with scalars before and after them,
    dof values around the 64-lane loop, and LDS sized by the rank where rank > max_outer * max_m"""
    norm = ('none', 'log10', 'linear')[rank % 3]
    scale = {'none': 1.0, 'log10': 1.0, 'linear': (1e-3, 250.0)[rank % 2]}[norm]
    lat0 = min(rank % 4, 16 - rank)
    n_out = min(16, lat0 + rank + (rank % 2))
    decl = ((5, 4), (2, 1), (3, 2), (1, 4))[rank % 4]                   # max_outer * max_m = 68, 3, 10, 0
    return norm, scale, lat0, n_out, DOFS[rank % len(DOFS)], decl


def _field_run(n, D, betas, coefs, values, n_out, t, ld, ld_out, decl, lat0, rank, dof, norm, scale, basis):
    import torch
    from hallthrusterpem_amd import _lib
    idx, vals = hr.index_table(betas, values)
    d_idx, d_val = torch.from_numpy(idx).cuda(), torch.from_numpy(vals).cuda()
    d_coef = torch.tensor(coefs, dtype=torch.float64, device='cuda')
    d_t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)).cuda()
    d_b = torch.from_numpy(np.ascontiguousarray(basis)).cuda()
    out = torch.full((n_out, ld_out), float('nan'), dtype=torch.float64, device='cuda')
    field = torch.full((n + 1, dof), float('nan'), dtype=torch.float64, device='cuda')
    _lib.check(_lib.load().pem_sparse_predict_field_f64_dev(n, D, len(betas), hr.ptr(d_idx), hr.ptr(d_coef), hr.ptr(d_val), n_out,
                                                            hr.ptr(d_t), ld, hr.ptr(out), ld_out, *decl, lat0, rank, dof,
                                                            hr.NORMS[norm], scale, hr.ptr(d_b), hr.ptr(field), _stream()))
    plain = torch.full((n_out, ld_out), float('nan'), dtype=torch.float64, device='cuda')
    _lib.check(_lib.load().pem_sparse_predict_f64_dev(n, D, len(betas), hr.ptr(d_idx), hr.ptr(d_coef), hr.ptr(d_val), n_out,
                                                      hr.ptr(d_t), ld, hr.ptr(plain), ld_out, *decl, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[:, :n], plain[:, :n]), 'the field launch predicts other outputs than pem_sparse_predict'
    assert bool(out[:, n:].isnan().all()) and bool(field[n].isnan().all())
    return out, field


def _latent_scale(values, lat0, rank, norm):
    """latent columns of a size that keeps 10^(latent @ basis^T) in range"""
    for v in values:
        v[:, lat0:lat0 + rank] *= 0.3 if norm == 'log10' else 1.0


@pytest.mark.parametrize('rank', list(range(1, 17)))
def test_predict_field_every_rank_norm_and_dof(rank):
    norm, scale, lat0, n_out, dof, decl = _field_case(rank)
    D = 6
    if decl[0] == 1:
        betas = [hr.beta_of(D, {})] + [hr.beta_of(D, {d: l}) for d, l in ((0, 4), (3, 2), (5, 1))]
    elif decl == (2, 1):
        betas = [hr.beta_of(D, {}), hr.beta_of(D, {0: 1}), hr.beta_of(D, {1: 1, 4: 1})]
    elif decl == (3, 2):
        betas = [hr.beta_of(D, {}), hr.beta_of(D, {2: 2}), hr.beta_of(D, {0: 1, 1: 2, 5: 1})]
    else:
        betas = [hr.beta_of(D, {}), hr.beta_of(D, {1: 4, 2: 1}), hr.beta_of(D, {0: 1, 1: 1, 2: 1, 3: 1, 5: 4})]
    n = 700 + rank
    values, coefs = _table(D, betas, n_out, seed=100 + rank)
    _latent_scale(values, lat0, rank, norm)
    basis = np.linalg.qr(np.random.default_rng(rank).standard_normal((max(dof, rank), rank)))[0][:dof]
    t = _coords(D, n, n + 2, seed=rank)
    out, field = _field_run(n, D, betas, coefs, values, n_out, t, n + 2, n + 4, decl, lat0, rank, dof, norm, scale, basis)
    lat = out[lat0:lat0 + rank, :n].T.cpu().numpy()
    want, bound = hr.field_ref(lat, basis, norm, scale)
    hr.assert_within(field[:n].cpu().numpy(), want, bound, f'rank {rank} {norm} dof {dof}')
    pw, pb = hr.predict_ref(betas, coefs, values, t[:, :n])
    hr.assert_within(out[:, :n].cpu().numpy(), pw, pb, f'rank {rank} outputs')


def test_predict_field_past_the_first_round():
    import torch
    rank, lat0, n_out, dof, norm = 4, 2, 7, 65, 'log10'
    values, coefs = _table(D_BIG, BIG_BETAS, n_out, seed=9)
    _latent_scale(values, lat0, rank, norm)
    basis = np.linalg.qr(np.random.default_rng(1).standard_normal((dof, rank)))[0]
    base, t = _periodic_coords(N_BIG)
    out, field = _field_run(N_BIG, D_BIG, BIG_BETAS, coefs, values, n_out, t, N_BIG, N_BIG + 3, (5, 4), lat0, rank, dof, norm, 1.0, basis)
    _check_periodic(out, 'outputs')
    _check_periodic(field[:N_BIG].T, 'field')
    pts = _check_points()
    lat = out[lat0:lat0 + rank][:, torch.from_numpy(pts).cuda()].T.cpu().numpy()
    want, bound = hr.field_ref(lat, basis, norm)
    hr.assert_within(field[torch.from_numpy(pts).cuda()].cpu().numpy(), want, bound, 'field past the first round')
    pw, pb = hr.predict_ref(BIG_BETAS, coefs, values, base[:, pts % PERIOD])
    hr.assert_within(out[:, pts].cpu().numpy(), pw, pb, 'outputs past the first round')
