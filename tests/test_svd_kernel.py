"""pem_svd.hip over its whole dispatch space, entry by entry against the long-double restatement of tests/hp_reference.py:
every dof the kernels split on, every norm and rank class (RT 4 / 8 / 16), the per-call A/B switches PEM_SVD_TILED and
PEM_SVD_NO_MFMA (the only way to the ROWS = 16 tiled kernels and to svd_compress_kernel<16,12,16,LOG10,true>), pointers 8 bytes
off 16-byte alignment, and each kernel in each grid regime of balanced_blocks with periodic rows whose latents / fields must
equal their period mates bit for bit."""
import re
from pathlib import Path

import numpy as np
import pytest

import hp_reference as hr

SRC = Path(__file__).resolve().parents[1] / 'hallthrusterpem_amd' / 'csrc' / 'pem_svd.hip'
DOFS = (1, 2, 15, 16, 17, 63, 64, 91, 95, 96, 97, 128, 202, 207, 208)
RANKS = (1, 3, 4, 5, 8, 9, 16)
SCALE = {'none': 1.0, 'log10': 1.0, 'linear': 7.5e-3}


# ---- the grid regimes, restated ---------------------------------------------------------------------------------------
def balanced_blocks(need, cap):
    """(blocks, regime) of pem_svd.hip balanced_blocks (PEM_SVD_GRID_MULT unset)"""
    if need <= cap:
        return need, 'one'
    if need > 3 * cap:
        return (need if need < 4 * cap else 4 * cap), 'many'
    rounds = -(-need // cap)
    g = -(-need // rounds)
    return (g, 'balanced') if 10 * g >= 9 * cap else (cap, 'capped')


# kernel -> (rows per tile, resident workgroups of the cap, dof, rank, norm, environment)
KERNELS = {
    'direct': (16, 3 * 256, 91, 5, 'log10', {}),
    'tiled16': (16, 2 * 256, 91, 16, 'linear', {'PEM_SVD_TILED': '1'}),
    'mfma': (16, 2 * 256, 95, 7, 'log10', {'PEM_SVD_TILED': '1'}),
    'tiled8': (8, 2 * 256, 202, 7, 'linear', {}),
    'recon_breg': (16, 3 * 256, 91, 9, 'log10', {}),
    'recon_lds': (16, 2 * 256, 202, 7, 'linear', {}),
}
NEED = {'one': lambda cap: cap - 3, 'balanced': lambda cap: 2 * cap - 10, 'capped': lambda cap: cap + 1,
        'many': lambda cap: 8 * cap + cap // 2}


def test_balanced_blocks_restatement_matches_the_source():
    """The regime tests size their batches from the restatement above: a change of the dispatch must change this test too."""
    src = SRC.read_text()
    body = re.search(r'size_t balanced_blocks\(size_t need, size_t cap\) \{(.*?)\n\}', src, re.S).group(1)
    code = [ln.split('//')[0].strip() for ln in body.splitlines()]
    code = [ln for ln in code if ln]
    assert code == ['if (need <= cap) return need;', 'if (const char* e = getenv("PEM_SVD_GRID_MULT")) {', 'const long long m = atoll(e);',
                    'return (m <= 0 || (size_t)m * cap > need) ? need : (size_t)m * cap;', '}',
                    'if (need > 3 * cap) return need < 4 * cap ? need : 4 * cap;', 'const size_t rounds = (need + cap - 1) / cap;',
                    'const size_t g = (need + rounds - 1) / rounds;', 'return 10 * g >= 9 * cap ? g : cap;'], code
    assert 'size_t blocks = balanced_blocks((tiles + WAVES - 1) / WAVES, 256 * 2);' in src                  # tiled compress
    assert 'const size_t per_cu = 3;' in src and 'dblocks = balanced_blocks(dblocks, 256 * per_cu);' in src    # direct compress
    assert 'const unsigned rgrid = grid_for(n, rbreg ? 3 : 2);' in src                                      # reconstruct
    assert 'const int rows = dof <= 96 ? 16 : 8' in src and 'if (dof <= 4 * DIRECT_STEPS && !getenv("PEM_SVD_TILED"))' in src
    for kernel, (rows, cap, *_rest) in KERNELS.items():
        for regime, need in NEED.items():
            n = 4 * rows * need(cap) - 7
            assert balanced_blocks(-(-(-(-n // rows)) // 4), cap)[1] == regime, (kernel, regime)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def _call(fn, n, dof, rank, norm, src, basis, dst):
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    rc = getattr(_lib.load(), fn)(n, dof, rank, hr.NORMS[norm], SCALE[norm], hr.ptr(src), hr.ptr(basis), hr.ptr(dst),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc)


def _field(n, dof, norm, seed):
    rng = np.random.default_rng(seed)
    if norm == 'log10':
        return 10.0 ** rng.uniform(-3.0, 3.0, (n, dof))
    return rng.standard_normal((n, dof)) * 10.0 ** rng.uniform(-2, 2, (n, 1))


def _basis(dof, rank, seed):
    return np.random.default_rng(seed).standard_normal((dof, rank)) / np.sqrt(dof)


def _compress(y, basis, norm, offset=1):
    """latents through the C ABI into rows offset .. offset + n - 1 of a NaN-filled buffer: nothing may land outside them"""
    import torch
    n, dof = y.shape
    rank = basis.shape[1]
    d_y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    d_b = torch.from_numpy(np.ascontiguousarray(basis)).cuda()
    buf = torch.full((n + offset + 1, rank), float('nan'), dtype=torch.float64, device='cuda')
    _call('pem_svd_compress_f64_dev', n, dof, rank, norm, d_y, d_b, buf[offset:offset + n])
    got = buf.cpu().numpy()
    assert np.isnan(got[:offset]).all() and np.isnan(got[offset + n:]).all(), 'written outside the latents'
    return got[offset:offset + n]


def _reconstruct(z, basis, norm, offset=1):
    import torch
    n, rank = z.shape
    dof = basis.shape[0]
    d_z = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    d_b = torch.from_numpy(np.ascontiguousarray(basis)).cuda()
    buf = torch.full((n + offset + 1, dof), float('nan'), dtype=torch.float64, device='cuda')
    _call('pem_svd_reconstruct_f64_dev', n, dof, rank, norm, d_z, d_b, buf[offset:offset + n])
    got = buf.cpu().numpy()
    assert np.isnan(got[:offset]).all() and np.isnan(got[offset + n:]).all(), 'written outside the field'
    return got[offset:offset + n]


def _latents(n, rank, norm, seed):
    z = np.random.default_rng(seed).standard_normal((n, rank))
    return z * (0.5 if norm == 'log10' else 1.0)


# ---- every dof, norm and rank class -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dof', DOFS)
def test_compress_and_reconstruct_every_dof_norm_and_rank(dof, monkeypatch):
    """n = 37 (a ragged tile for 16 and 8 rows); the latent / field buffers are offset by one row, so that with an odd rank /
    dof the output pointer is 8 bytes off 16-byte alignment.  dof <= 96 also through the tiled kernels (PEM_SVD_TILED), with
    and without the MFMA form of the log10 one (PEM_SVD_NO_MFMA)."""
    n = 37
    switches = [{}] + ([{'PEM_SVD_TILED': '1'}, {'PEM_SVD_TILED': '1', 'PEM_SVD_NO_MFMA': '1'}] if dof <= 96 else [])
    for norm in ('none', 'log10', 'linear'):
        y = _field(n, dof, norm, seed=dof)
        for rank in RANKS:
            basis = _basis(dof, rank, seed=rank)
            want, bound = hr.compress_ref(y, basis, norm, SCALE[norm])
            for env in switches:
                for k in ('PEM_SVD_TILED', 'PEM_SVD_NO_MFMA'):
                    if k in env:
                        monkeypatch.setenv(k, env[k])
                    else:
                        monkeypatch.delenv(k, raising=False)
                hr.assert_within(_compress(y, basis, norm), want, bound, f'compress dof {dof} rank {rank} {norm} {env}')
            monkeypatch.delenv('PEM_SVD_TILED', raising=False)
            monkeypatch.delenv('PEM_SVD_NO_MFMA', raising=False)
            z = _latents(n, rank, norm, seed=dof + rank)
            want, bound = hr.reconstruct_ref(z, basis, norm, SCALE[norm])
            hr.assert_within(_reconstruct(z, basis, norm), want, bound, f'reconstruct dof {dof} rank {rank} {norm}')


@pytest.mark.gpu
@pytest.mark.parametrize('dof', [91, 95, 97, 203])
def test_eight_byte_offset_views(dof):
    """field, latent and output pointers 8 bytes off 16-byte alignment: the [1:] row slice of an odd-dof (or odd-rank) array"""
    import torch
    rank, n = 5, 1001
    for norm in ('log10', 'linear'):
        y = _field(n + 1, dof, norm, seed=3)
        basis = _basis(dof, rank, seed=4)
        d_b = torch.from_numpy(basis).cuda()
        d_y = torch.from_numpy(y).cuda()[1:]
        assert d_y.data_ptr() % 16 == 8
        lat = torch.full((n + 2, rank), float('nan'), dtype=torch.float64, device='cuda')
        _call('pem_svd_compress_f64_dev', n, dof, rank, norm, d_y, d_b, lat[1:n + 1])
        assert lat[1:].data_ptr() % 16 == 8
        got = lat.cpu().numpy()
        assert np.isnan(got[0]).all() and np.isnan(got[n + 1]).all()
        want, bound = hr.compress_ref(y[1:], basis, norm, SCALE[norm])
        hr.assert_within(got[1:n + 1], want, bound, f'compress from an offset view, dof {dof} {norm}')
        z = _latents(n + 1, rank, norm, seed=5)
        d_z = torch.from_numpy(z).cuda()[1:]
        assert d_z.data_ptr() % 16 == 8
        out = torch.full((n + 2, dof), float('nan'), dtype=torch.float64, device='cuda')
        _call('pem_svd_reconstruct_f64_dev', n, dof, rank, norm, d_z, d_b, out[1:n + 1])
        assert out[1:].data_ptr() % 16 == 8
        got = out.cpu().numpy()
        assert np.isnan(got[0]).all() and np.isnan(got[n + 1]).all()
        want, bound = hr.reconstruct_ref(z[1:], basis, norm, SCALE[norm])
        hr.assert_within(got[1:n + 1], want, bound, f'reconstruct into an offset view, dof {dof} {norm}')


# ---- every grid regime, periodic rows -------------------------------------------------------------------------------------
PERIOD = 997                 # rows; prime: a row and its mates sit in every position of a tile, in every wave and round


@pytest.mark.gpu
@pytest.mark.parametrize('regime', list(NEED))
@pytest.mark.parametrize('kernel', list(KERNELS))
def test_every_grid_regime_with_periodic_rows(kernel, regime, monkeypatch):
    import torch
    rows, cap, dof, rank, norm, env = KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if 'PEM_SVD_TILED' not in env:
        monkeypatch.delenv('PEM_SVD_TILED', raising=False)
    monkeypatch.delenv('PEM_SVD_NO_MFMA', raising=False)
    monkeypatch.delenv('PEM_SVD_GRID_MULT', raising=False)
    n = 4 * rows * NEED[regime](cap) - 7                             # ragged: the last tile is not full
    assert balanced_blocks(-(-(-(-n // rows)) // 4), cap)[1] == regime
    basis = _basis(dof, rank, seed=8)
    d_b = torch.from_numpy(basis).cuda()
    mate = torch.arange(n, device='cuda') % PERIOD
    # the rows held to the reference: one period and the rows around every round boundary of the grid
    blocks, _ = balanced_blocks(-(-(-(-n // rows)) // 4), cap)
    per_round = blocks * 4 * rows
    check = set(range(PERIOD)) | set(range(max(0, n - 100), n))
    for k in range(1, -(-n // per_round)):
        check |= set(range(k * per_round - 100, min(n, k * per_round + 100)))
    check = np.array(sorted(check))
    if kernel.startswith('recon'):
        base = _latents(PERIOD, rank, norm, seed=9)
        src = torch.from_numpy(base).cuda()[mate]
        out = torch.full((n + 1, dof), float('nan'), dtype=torch.float64, device='cuda')
        _call('pem_svd_reconstruct_f64_dev', n, dof, rank, norm, src, d_b, out)
        want, bound = hr.reconstruct_ref(base[check % PERIOD], basis, norm, SCALE[norm])
    else:
        base = _field(PERIOD, dof, norm, seed=10)
        src = torch.from_numpy(base).cuda()[mate]
        out = torch.full((n + 1, rank), float('nan'), dtype=torch.float64, device='cuda')
        _call('pem_svd_compress_f64_dev', n, dof, rank, norm, src, d_b, out)
        want, bound = hr.compress_ref(base[check % PERIOD], basis, norm, SCALE[norm])
    torch.cuda.synchronize()
    del src
    assert bool(out[n].isnan().all()), 'written past the batch'
    same = (out[:n] == out[:n][mate]).all(dim=1)
    assert bool(same.all()), f'{kernel} {regime}: {int((~same).sum())} rows differ from their period mate, first ' \
        f'{int(torch.nonzero(~same)[0][0])} of {n} ({per_round} rows per round)'
    hr.assert_within(out[torch.from_numpy(check).cuda()].cpu().numpy(), want, bound, f'{kernel} {regime}')
