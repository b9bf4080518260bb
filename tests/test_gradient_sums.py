"""The fused gradient-sums launch (csrc/pem_jacobian.hip, `derivatives.gradient_sums`, `drivers.derivative_sensitivity`) on the GPU
against the composed path: the design's rows written out by `Design.sample(swap_dim=-1)`, the explicit launch
(`derivatives.jacobian`) on them, the gradient taken in the prior's coordinates and every term summed in long double on the host
(tests/jacobian_np.py).

The bound on a value of the partial is derived, not tuned:

    |got - want| <= 1.01 k 2^-53 S + ulp(want)

S the sum of the magnitudes of the row's terms for that QoI, k the roundings a term can pass through in the kernel and after it:
    forming the term            1 .. 15 (jacobian_np.terms: v = f - c: 1; v^2: 3; g = (x ln 10) df/dx: 3; g^4: 15; g_i g_j: 7)
    the lane's running sum      L      the lane that owns a row adds one term per sample of the tiles of its wave, 64 a tile:
                                       L = 64 ceil(groups / n_blocks), groups = ceil(tiles / 4), tiles = ceil((n + lead) / 64),
                                       lead = first_index % 64 on the Sobol' design (the grid walks 64-aligned tiles), 0 otherwise
    the four waves              3
    the sum over workgroups     B - 1  B = min(n_blocks, groups), the workgroups that hold a live sample (the others add exact zeros)
The factor 1.01 covers the products of roundings and the long-double sum.

There is NO model term: the two launches share bits.  Both inline the one device function of csrc/pem_jacobian.h, which is compiled
without contraction, on the same doubles (the fused launch's design rows are bit-identical to `Design.sample`), so f and df/dx of
the composed path are the very numbers the fused launch sums; the bound would not hold otherwise.  Each case prints its worst
error / bound.

Worst seen on an MI355X: |got - want| / bound 0.091 over the shapes, 0.037 with skipped rows, 0.013 for two shards against the whole;
the driver within 1.4e-13 of the restatement's measures, where 1e-8 is asked."""
import numpy as np
import pytest

import jacobian_np as jn

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DEFAULT_BLOCKS = 512
SHAPES = [(1, 0, 1), (63, 7, 1), (64, 0, 1), (65, 5, 1), (257, 0, 1), (1000, 12345, None)]
SHUFFLED = [9, 3, 14, 0, 7, 12, 1, 5, 10, 2, 13, 4, 8, 6, 11]
VARIED = {0: [], 1: [11], 2: [0, 10], 15: SHUFFLED}
CENTRE = np.array([31.0, 0.4, 0.09])                      # (any constants will do)
FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6}


def _k():
    from hallthrusterpem_amd import constants
    return constants.TORR_2_PA


def _design(priors=None, seed=11, fixed=None):
    from hallthrusterpem_amd import sampling
    pri = dict(sampling.PEM_V0_PRIORS)
    for k, v in (fixed or {}).items():
        pri[k] = sampling.Prior(sampling.UNIFORM, v, v, 'fixed')
    pri.update(priors or {})
    return sampling.Design(priors=pri, seed=seed)


class Composed:
    """the rows of a design, the explicit launch on them, and the gradient in the prior's coordinates (long double)"""

    def __init__(self, design, varied, n, first, method, scramble=True):
        from hallthrusterpem_amd import derivatives
        x = design.sample(n, first_index=first, method=method, swap_dim=-1, scramble=scramble)
        res = derivatives.jacobian(design.as_dict(x), wrt=[design.names[i] for i in varied])
        self.x = x.cpu().numpy()
        self.f = np.stack([res[q].cpu().numpy() for q in jn.QOI])
        flags = res['flags'].cpu().numpy()
        self.non_physical, self.invalid = int((flags & 1).sum()), int((flags >> 1 & 1).sum())
        self.g = jn.gradients({'jac': res['jacobian'].cpu().numpy(), 'x': self.x}, varied, design.kind)
        self.n, self.first, self.method = n, first, method


def _roundings(form, n, first, n_blocks, method):
    lead = first % 64 if method == 'sobol' else 0
    tiles = -(-(n + lead) // 64)
    groups = -(-tiles // 4)
    return form + 64 * -(-groups // n_blocks) + 3 + (min(n_blocks, groups) - 1)


def _bound(comp, c, n_blocks):
    want, mag, form, skipped = jn.sums_of(comp.f, comp.g, c)
    k = _roundings(form, comp.n, comp.first, n_blocks, comp.method)[:, None]
    return want, 1.01 * k * U * mag.astype(np.float64) + np.spacing(np.abs(want.astype(np.float64))), skipped


def _hold(design, varied, comp, centre, n_blocks, scramble=True):
    from hallthrusterpem_amd.derivatives import gradient_sums
    got, flags = gradient_sums(design, varied, comp.n, centre, first_index=comp.first, n_blocks=n_blocks, method=comp.method, scramble=scramble)
    got = got.cpu().numpy()
    want, bound, skipped = _bound(comp, np.zeros(3) if centre is None else centre, n_blocks or DEFAULT_BLOCKS)
    assert got.shape == want.shape == (jn.n_rows(len(varied)), 3)
    err = np.abs(got - want).astype(np.float64)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f'n {comp.n} first {comp.first} blocks {n_blocks or DEFAULT_BLOCKS} nv {len(varied)} {comp.method}: worst |got - want| / bound = {worst:.3g}')
    assert np.all(err <= bound), (comp.method, np.argwhere(err > bound)[:5], worst)
    assert flags.tolist() == [comp.non_physical, comp.invalid, skipped], (flags, comp.non_physical, comp.invalid, skipped)
    return got, flags, worst


@pytest.mark.parametrize('nv', [0, 1, 2, 15])
@pytest.mark.parametrize('n, first, n_blocks', SHAPES, ids=[f'n{n}-first{f}-blocks{b}' for n, f, b in SHAPES])
def test_every_row_of_the_partial_against_the_composed_path_in_long_double(n, first, n_blocks, nv):
    design, varied = _design(), VARIED[nv]
    for method in ('mc', 'sobol'):
        _, flags, _ = _hold(design, varied, Composed(design, varied, n, first, method), None if nv == 2 else CENTRE, n_blocks)
        assert flags.tolist() == [0, 0, 0]
    if (n, nv) == (65, 1):
        _hold(design, varied, Composed(design, varied, n, first, 'sobol', scramble=False), CENTRE, n_blocks, scramble=False)


def test_inert_inputs_have_exact_zero_sums():
    """a_1 reaches none of the three QoIs; mdot_a, c4, c5 and sigma_cex do not reach div_angle: bit-zeros in every sum of theirs"""
    from hallthrusterpem_amd.derivatives import gradient_sums
    design = _design()
    names = list(design.names)
    varied = list(range(15))
    got, flags = gradient_sums(design, varied, 1000, CENTRE, method='sobol')
    got = got.cpu().numpy()
    d = 15
    for name, qs in (('a_1', (0, 1, 2)), ('mdot_a', (0, 1)), ('c4', (0, 1)), ('c5', (0, 1)), ('sigma_cex', (0, 1))):
        j = names.index(name)
        for q in qs:
            assert got[2 + j, q] == 0.0 and got[2 + d + j, q] == 0.0, (name, q)
    M = np.zeros((d, d, 3))
    M[np.triu_indices(d)] = got[2 + 2 * d:]
    assert not M[names.index('a_1')].any() and not M[:, names.index('a_1')].any()
    assert M[names.index('c3'), names.index('c3'), 0] == 0.0 and np.all(M[names.index('c3'), names.index('c3'), 1:] > 0)      # (V_cc sees no c3)
    assert flags.tolist() == [0, 0, 0]


def test_rows_that_are_not_finite_are_skipped_and_counted():
    """(a) c2 P_B = -c3 exactly: a1 = 0, the normaliser and with it div_angle and T_c are NaN in every sample: all skipped, every sum an
    exact zero, all counted invalid as well.  (b) c1 ~ U(0.001, 0.1) with a1 = c3 = 0.3: |a2| = 0.3 / c1 passes 53.28, where the
    normaliser is NaN, in about one sample of twenty: those are left out of every sum, V_cc's too, and the rest is within the bound"""
    from hallthrusterpem_amd import sampling
    from hallthrusterpem_amd.derivatives import gradient_sums
    fix = lambda v: sampling.Prior(sampling.UNIFORM, v, v, 'fixed')                            # noqa: E731
    c2PB = -8.0 * (1e-5 * _k())
    design = _design({'P_b': fix(1e-5), 'c2': fix(-8.0), 'c3': fix(-c2PB)})
    varied = [2, 8, 9]
    n = 300
    for method in ('mc', 'sobol'):
        got, flags = gradient_sums(design, varied, n, CENTRE, method=method)
        assert not got.cpu().numpy().any() and flags.tolist() == [0, n, n], (method, flags)
        comp = Composed(design, varied, n, 0, method)
        assert np.isnan(comp.f[1]).all() and np.isfinite(comp.f[0]).all()
    design = _design({'c2': fix(0.0), 'c3': fix(0.3), 'c1': sampling.Prior(sampling.UNIFORM, 0.001, 0.1, 'test')})
    varied = [9, 3, 8, 0]
    for method in ('mc', 'sobol'):
        comp = Composed(design, varied, 1000, 0, method)
        _, flags, _ = _hold(design, varied, comp, CENTRE, None)
        print(method, 'skipped', int(flags[2]))
        assert 20 <= int(flags[2]) <= 90


def test_an_empty_shard_is_zero():
    from hallthrusterpem_amd.derivatives import gradient_sums
    design = _design()
    for method, first in (('mc', 0), ('mc', 12345), ('sobol', 0), ('sobol', 2 ** 30)):
        for nv in (0, 12):
            s, flags = gradient_sums(design, list(range(nv)), 0, CENTRE, first_index=first, method=method)
            assert s.shape == (jn.n_rows(nv), 3) and not s.cpu().numpy().any() and flags.tolist() == [0, 0, 0]


@pytest.mark.parametrize('method', ['mc', 'sobol'])
def test_two_shards_sum_to_the_whole(method):
    """the same terms in another order: each of the three launches is within its derived bound of the exact sum of its terms, so
    the parts together are within the sum of the three bounds of the whole"""
    from hallthrusterpem_amd.derivatives import gradient_sums
    design = _design(fixed=FIXED)
    varied = [i for i, k in enumerate(design.names) if k not in FIXED]
    N, cut = 1000, 700
    run = lambda n, lo: gradient_sums(design, varied, n, CENTRE, first_index=lo, method=method)[0].cpu().numpy()    # noqa: E731
    whole, p0, p1 = run(N, 0), run(cut, 0), run(N - cut, cut)
    bound = np.zeros_like(whole)
    for n, lo in ((N, 0), (cut, 0), (N - cut, cut)):
        bound += _bound(Composed(design, varied, n, lo, method), CENTRE, DEFAULT_BLOCKS)[1]
    err = np.abs(p0 + p1 - whole)
    print(method, 'worst |parts - whole| / bound', np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound + np.spacing(np.abs(whole)))                      # (one more rounding: p0 + p1)


def test_the_result_does_not_depend_on_scheduling():
    from hallthrusterpem_amd.derivatives import gradient_sums
    design = _design()
    a = gradient_sums(design, SHUFFLED, 5000, CENTRE, n_blocks=7)[0]
    b = gradient_sums(design, SHUFFLED, 5000, CENTRE, n_blocks=7)[0]
    assert bool((a == b).all())


@pytest.mark.parametrize('method', ['mc', 'sobol'])
def test_the_driver_end_to_end(method):
    """drivers.derivative_sensitivity(4096): every measure within 1e-8 of `jacobian_np.measures` applied to the float64 restatement's
    sums over the same design rows about the same centre, and the centre is the pilot's mean.  "Within 1e-8" is |got - want| <=
    1e-8 max(1, |want|): in physical units nu reaches 6e8 (V_cc with respect to P_T, a uniform prior over 1e-5 .. 1e-4 Torr), where
    one ulp is 1.2e-7 and an absolute 1e-8 is below what a double resolves; for every value up to 1 it is the absolute figure."""
    from hallthrusterpem_amd import drivers
    from hallthrusterpem_amd.derivatives import gradient_sums
    n, seed = 4096, 5
    res = drivers.derivative_sensitivity(n, seed=seed, design=method)
    design = _design(seed=seed)
    assert res['inputs'] == list(design.names) and res['evaluations'] == n and res['pilot_evaluations'] == n
    assert (res['non_physical'], res['invalid'], res['skipped'], res['design']) == (0, 0, 0, method)
    pilot, _ = gradient_sums(design, [], n, None, method=method)
    centre = np.array([res['centre'][q] for q in jn.QOI])
    assert np.array_equal(centre, (pilot[0] / n).cpu().numpy())
    x = design.sample(n, method=method).cpu().numpy()
    rest = jn.jacobian(x, _k())
    varied = list(range(15))
    sums, _, _, skipped = jn.sums_of(rest['f'], jn.gradients(rest, varied, design.kind), centre)
    want = jn.measures(sums.astype(np.float64), n, design.kind, design.a, design.b, centre)
    assert skipped == 0
    worst = {}
    for key, w in want.items():
        if key == 'eigenvectors':
            continue
        g = np.stack([np.asarray(res[key][q].cpu().numpy() if hasattr(res[key][q], 'cpu') else res[key][q]) for q in jn.QOI])
        assert g.shape == np.asarray(w).shape, key
        worst[key] = float(np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w))))
    # the leading direction up to its sign
    for qi, q in enumerate(jn.QOI):
        w1, g1 = want['eigenvectors'][qi][:, 0], res['eigenvectors'][q].cpu().numpy()[:, 0]
        worst['direction ' + q] = float(min(np.max(np.abs(g1 - w1)), np.max(np.abs(g1 + w1))))
    print(method, 'max |driver - restatement|', worst)
    assert all(v < 1e-8 for v in worst.values()), worst
    for q in jn.QOI:
        assert float(res['var'][q]) > 0 and bool((res['nu'][q] >= 0).all()) and bool((res['eigenvalues'][q][:-1] >= res['eigenvalues'][q][1:]).all())
    assert float(res['bound_ST']['V_cc'][design.names.index('a_1')]) == 0.0


def test_refused_calls_launch_nothing():
    """every argument error returns its status and leaves the outputs as they were"""
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    from test_jacobian_host import BAD, BAD_QMC, launch_sums
    partial = torch.full((4, jn.n_rows(2), 3), -7.0, dtype=torch.float64, device='cuda')
    flags = torch.full((4, 3), -7, dtype=torch.int64, device='cuda')
    for entry in ('f64', 'qmc_f64'):
        for bad in BAD + (BAD_QMC if entry == 'qmc_f64' else []):
            kw = dict(dict(partial=C.c_void_p(partial.data_ptr()), flags=C.c_void_p(flags.data_ptr())), **bad)
            assert launch_sums(entry, **kw) == _lib.PEM_ERR_INVALID_ARG, (entry, bad)
    torch.cuda.synchronize()
    assert bool((partial == -7.0).all()) and bool((flags == -7).all())
    assert launch_sums('f64', partial=C.c_void_p(partial.data_ptr()), flags=C.c_void_p(flags.data_ptr())) == _lib.PEM_OK
    torch.cuda.synchronize()
    assert not bool((partial == -7.0).any()) and bool((flags >= 0).all())
