"""The shifted Sobol' design on the GPU: pem_sample_sobol_f64_dev and the fused pem_saltelli_qmc_* launches against the numpy
restatement (tests/qmc_np.py, itself pinned to torch and scipy in tests/test_qmc_host.py), under the rules tests/test_sampler.py holds
the Philox sampler to: uniform dimensions equal bit for bit (the same IEEE operations), log-uniform ones within 4e-15 relative
(exp() differs by an ulp at most), normal ones within 1e-12 absolute at sigma <= 1."""
import numpy as np
import pytest

import qmc_np

pytestmark = pytest.mark.gpu

SEED = (0x9E3779B9 << 32) | 0x7F4A7C15
GRID_LANES = 256 * 16 * 256                  # what sobol_sample_kernel's grid covers in one pass (csrc/pem_qmc.hip)


def _design(ndim, seed=SEED, stream=3):
    """kinds cycle uniform / log-uniform / normal (sigma <= 1)"""
    from hallthrusterpem_amd.sampling import Design, Prior
    table = [Prior(0, 2.0, 5.0, 't'), Prior(1, -8.0, -4.0, 't'), Prior(2, 30.0, 0.75, 't')]
    names = tuple(f'x{i}' for i in range(ndim))
    return Design(priors={k: table[i % 3] for i, k in enumerate(names)}, names=names, seed=seed, stream=stream)


def _hold(got, d, n, first, **kw):
    """device rows `got` against the restatement, kind by kind"""
    want = qmc_np.sample(n, first, d.seed, d.stream, d.kind, d.a, d.b, **kw)
    assert got.shape == want.shape
    uni, logu, nrm = d.kind == 0, d.kind == 1, d.kind == 2
    assert np.array_equal(got[uni], want[uni])
    if logu.any():
        assert np.max(np.abs(got[logu] / want[logu] - 1)) < 4e-15
    if nrm.any():
        assert np.max(np.abs(got[nrm] - want[nrm])) < 1e-12
    return want


def test_a_second_grid_pass_across_the_top_gray_code_bit_and_the_last_points_of_the_sequence():
    d = _design(3)
    first = 2 ** 29 - 70                         # 58 lanes of lead; bit 29 of the Gray code switches on 70 samples in
    n = GRID_LANES + 1 + 37                      # one sample more than a pass covers, and a ragged tail
    for scramble in (True, False):
        _hold(d.sample(n, first_index=first, method='sobol', scramble=scramble).cpu().numpy(), d, n, first, scramble=scramble)
    _hold(d.sample(64, first_index=2 ** 30 - 64, method='sobol').cpu().numpy(), d, 64, 2 ** 30 - 64)
    _hold(d.sample(1, first_index=2 ** 30 - 1, method='sobol').cpu().numpy(), d, 1, 2 ** 30 - 1)
    from hallthrusterpem_amd._lib import PemHipError
    with pytest.raises((ValueError, PemHipError)):
        d.sample(65, first_index=2 ** 30 - 64, method='sobol')


@pytest.mark.parametrize('ndim', [1, 15, 16, 17, 32])
def test_every_dimension_count_into_a_slice_whose_neighbours_stay_untouched(ndim):
    import torch
    d = _design(ndim)
    n, first = 777, 1_000_003
    for scramble in (True, False):
        wide = torch.full((ndim + 2, n + 13), -777.0, dtype=torch.float64, device='cuda')
        d.fill(wide[1:1 + ndim, 5:5 + n], first_index=first, method='sobol', scramble=scramble)
        host = wide.cpu().numpy()
        _hold(host[1:1 + ndim, 5:5 + n], d, n, first, scramble=scramble)
        host[1:1 + ndim, 5:5 + n] = -777.0
        assert np.all(host == -777.0)
    # the shift is keyed by seed and stream
    a = d.sample(100, method='sobol')
    assert not torch.equal(a, _design(ndim, seed=SEED + 1).sample(100, method='sobol'))
    assert not torch.equal(a, _design(ndim, stream=4).sample(100, method='sobol'))
    assert torch.equal(a, d.sample(100, method='sobol', n_total=5))              # n_total is ignored


@pytest.mark.parametrize('ndim', [16, 15])
def test_every_saltelli_block(ndim):
    d = _design(ndim)
    n, first = 300, 4000
    A = _hold(d.sample(n, first_index=first, method='sobol').cpu().numpy(), d, n, first)
    B = _hold(d.sample(n, first_index=first, method='sobol', swap_dim=-2).cpu().numpy(), d, n, first, swap_dim=-2)
    for sd in range(ndim):
        got = d.sample(n, first_index=first, method='sobol', swap_dim=sd).cpu().numpy()
        want = _hold(got, d, n, first, swap_dim=sd)
        assert all(np.array_equal(want[c], (B if c == sd else A)[c]) for c in range(ndim)) and not np.array_equal(A[sd], B[sd])
    _hold(d.sample(n, first_index=first, method='sobol', swap_dim=ndim - 1, scramble=False).cpu().numpy(), d, n, first,
          swap_dim=ndim - 1, scramble=False)


def test_three_ragged_shards_equal_one_fill():
    import torch
    d = _design(15)
    first, cuts = 12_345, [0, 1, 1000, 3000 + 77]
    whole = d.sample(cuts[-1], first_index=first, method='sobol')
    parts = torch.cat([d.sample(hi - lo, first_index=first + lo, method='sobol') for lo, hi in zip(cuts[:-1], cuts[1:])], dim=1)
    assert torch.equal(whole, parts)
    AB = torch.cat([d.sample(hi - lo, first_index=first + lo, method='sobol', swap_dim=7) for lo, hi in zip(cuts[:-1], cuts[1:])], dim=1)
    assert torch.equal(AB, d.sample(cuts[-1], first_index=first, method='sobol', swap_dim=7))


def test_forward_uq_on_the_sobol_design_is_the_restatement_and_its_qois_the_oracles():
    import torch
    from conftest import div_err, rel_err
    from hallthrusterpem_amd import constants, drivers, sampling
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    from oracle import oracle_ctypes as oc
    n = 4096
    res = drivers.forward_uq(n, seed=11, method='sobol')
    d = sampling.Design(seed=11)
    x = res['x'].cpu().numpy()
    _hold(x, d, n, 0)
    want = oc.coupled(dict(zip(COUPLED_INPUTS, x)), constants.TORR_2_PA)
    assert rel_err(res['V_cc'].cpu().numpy(), want['V_cc']) <= 1e-10
    assert div_err(res['div_angle'].cpu().numpy(), want['div_angle']) <= 1e-10
    assert rel_err(res['T_c'].cpu().numpy(), want['T_c']) <= 1e-10
    assert np.array_equal(res['invalid'].cpu().numpy(), want['invalid'])
    # batches and shards are ranges of the same design
    other = drivers.forward_uq(n, seed=11, method='sobol', batch_size=1000)
    parts = [drivers.forward_uq(n, seed=11, method='sobol', rank=r, world=3) for r in range(3)]
    assert torch.equal(other['x'], res['x']) and torch.equal(torch.cat([p['x'] for p in parts], dim=1), res['x'])
    assert torch.equal(torch.cat([p['T_c'] for p in parts]), res['T_c'])


FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6}


@pytest.mark.parametrize('N, bs', [(777, 256), (20_000, 1 << 13)])
def test_fused_fp64_qmc_launch_equals_the_block_by_block_driver(N, bs):
    """the shapes and tolerances of tests/test_fp32.py::test_fused_fp64_launch_equals_the_block_by_block_fp64_driver"""
    from hallthrusterpem_amd import drivers
    for scramble in ((True, False) if N < 1000 else (True,)):
        a = drivers.sobol_indices(N, seed=21, fixed=FIXED, batch_size=bs, fused=False, design='sobol', scramble=scramble)
        b = drivers.sobol_indices(N, seed=21, fixed=FIXED, design='sobol', scramble=scramble)
        assert b['fused'] and not a['fused'] and b['non_physical'] == 0 and b['invalid'] == 0
        assert a['design'] == b['design'] == 'sobol' and a['inputs'] == b['inputs'] and b['evaluations'] == N * 14
        for q in ('V_cc', 'div_angle', 'T_c'):
            assert float(b['mean'][q]) == pytest.approx(float(a['mean'][q]), rel=1e-13)
            assert float(b['var'][q]) == pytest.approx(float(a['var'][q]), rel=1e-11)
            for key in ('S1', 'ST'):
                assert float((a[key][q] - b[key][q]).abs().max()) < 1e-11, (N, q, key)
    mc = drivers.sobol_indices(N, seed=21, fixed=FIXED)
    assert mc['design'] == 'mc' and float(mc['mean']['T_c']) != float(b['mean']['T_c'])


def _varied_design(seed=11):
    from hallthrusterpem_amd import sampling
    pri = dict(sampling.PEM_V0_PRIORS)
    for k, v in FIXED.items():
        pri[k] = sampling.Prior(sampling.UNIFORM, v, v, 'fixed')
    design = sampling.Design(priors=pri, seed=seed)
    return design, [i for i, k in enumerate(design.names) if k not in FIXED]


def _scale(want):
    return np.maximum(np.abs(want), np.abs(want[1])[None, :] * 1e-6)             # rows that are exactly 0 (V_cc against plume inputs)


def test_two_shards_of_the_fused_qmc_launch_sum_to_the_whole_and_an_empty_shard_is_zero():
    """the partial sums of two shards against one launch: the same terms added in another order, N eps = 2e-12 of the sum of their
    magnitudes at most; held to 1e-11 of the scale tests/test_fp32.py uses for these rows"""
    from hallthrusterpem_amd.fp32 import saltelli_sums
    design, varied = _varied_design()
    for precision in ('fp32', 'fp64'):
        sums, flags = saltelli_sums(design, varied, 0, precision=precision, method='sobol')
        assert float(sums.abs().sum()) == 0.0 and int(flags.sum()) == 0
        sums, flags = saltelli_sums(design, varied, 0, first_index=2 ** 30, precision=precision, method='sobol')
        assert float(sums.abs().sum()) == 0.0 and int(flags.sum()) == 0
        N, first, cut = 20_000, 777, 6_001
        whole, _ = saltelli_sums(design, varied, N, first_index=first, precision=precision, method='sobol')
        p0, _ = saltelli_sums(design, varied, cut, first_index=first, precision=precision, method='sobol')
        p1, _ = saltelli_sums(design, varied, N - cut, first_index=first + cut, precision=precision, method='sobol')
        want = whole.cpu().numpy()
        assert np.max(np.abs((p0 + p1).cpu().numpy() - want) / _scale(want)) < 1e-11, precision


def test_fused_fp32_qmc_launch_equals_the_block_by_block_fp32_pipeline():
    """as tests/test_fp32.py::test_fused_saltelli_launch_equals_the_block_by_block_fp32_pipeline, on the Sobol' rows"""
    import torch
    from hallthrusterpem_amd.fp32 import CoupledBatchF32, saltelli_sums
    design, varied = _varied_design()
    for N, first, scramble in ((20_000, 0, True), (1000, 12345, False), (63, 7, True)):
        sums, flags = saltelli_sums(design, varied, N, first_index=first, method='sobol', scramble=scramble)
        x64 = torch.empty((15, N), dtype=torch.float64, device='cuda')
        b = CoupledBatchF32(N)

        def block(swap):
            design.fill(x64, first_index=first, swap_dim=swap, method='sobol', scramble=scramble)
            b.inputs.copy_(x64)
            b.run()
            torch.cuda.synchronize()
            return b.qoi.double().cpu().numpy().T.copy()           # (N, 3)
        fA, fB = block(-1), block(-2)
        want = np.zeros((2 + 2 * len(varied), 3))
        want[0], want[1] = (fA + fB).sum(0), (fA * fA + fB * fB).sum(0)
        for j, d in enumerate(varied):
            fAB = block(d)
            want[2 + 2 * j], want[3 + 2 * j] = (fB * (fAB - fA)).sum(0), ((fA - fAB) ** 2).sum(0)
        assert np.max(np.abs(sums.cpu().numpy() - want) / _scale(want)) < 1e-11, (N, first)
        assert flags.tolist() == [0, 0]


def test_fused_fp64_qmc_indices_equal_the_restatement_through_the_oracle():
    from hallthrusterpem_amd import drivers, sampling
    n, seed = 4096, 5
    d = sampling.Design(seed=seed)
    got = drivers.sobol_indices(n, seed=seed, design='sobol')
    S1, ST, mean, var = qmc_np.saltelli(qmc_np.oracle_qois, n, 0, seed, 0, d.kind, d.a, d.b, list(range(15)))
    assert got['inputs'] == list(d.names) and got['non_physical'] == 0 and got['invalid'] == 0
    for i, q in enumerate(('V_cc', 'div_angle', 'T_c')):
        assert np.max(np.abs(got['S1'][q].cpu().numpy() - S1[:, i])) < 1e-9, q
        assert np.max(np.abs(got['ST'][q].cpu().numpy() - ST[:, i])) < 1e-9, q
        assert float(got['mean'][q]) == pytest.approx(mean[i], rel=1e-9)
