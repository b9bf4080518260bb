"""The fp64 model kernels -- plume_r1_kernel in its profile, reduced and mixed modes, plume_rfew / radii / rmid / generic, the fused
coupled_latent_kernel, cathode, thruster and thruster_uion -- against the long double reference of tests/hp_model.py, under the
per-entry bound derived there for the path each kernel takes.  The input sets are hp_model's (priors, widths, tail, cancellation: the
ones tests/test_hp_model_host.py puts the oracle through without a GPU); launches have n = 1, 63, 64, 65 and 64 * 4 + 37 samples.
Every test prints the worst error / bound per quantity; one run is recorded in profiles/model_hp_r01.txt."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import hp_model as hp  # noqa: E402

pytestmark = pytest.mark.gpu
PLUME_KEYS = ('P_b', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')
SWEEP_COUNTS = (2, 8, 9, 12, 13, 64, 65, 256, 257)          # both sides of every kernel switch of DESIGN section 4.2, and the generic kernel


@pytest.fixture(scope='module')
def K():
    from hallthrusterpem_amd import constants
    return constants.TORR_2_PA


@pytest.fixture(scope='module')
def oracle():
    from oracle import oracle_ctypes as oc
    oc.set_threads(8)
    return oc


@pytest.fixture(scope='module', autouse=True)
def _device():
    """torch's device context and the library are brought up once, here: that takes about ten seconds and is no part of any test"""
    import torch
    from hallthrusterpem_amd import _lib
    _lib.load()
    _lib.require_device()
    torch.zeros(1, device='cuda').sum().item()


_cache = {}


def _set(name):
    if name not in _cache:
        _cache[name] = hp.SETS[name]()
    return _cache[name]


def _ref(name, K):
    """the one-radius reference of a set, computed once and shared (never modified)"""
    if ('ref', name) not in _cache:
        _cache[('ref', name)] = hp.reference(_set(name), K)
    return _cache[('ref', name)]


def _chunks(n):
    """launch sizes 1, 63, 64, 65, 293, 293, ... over n samples"""
    out, first = [], 0
    for size in hp.SIZES:
        if first < n:
            out.append((first, min(first + size, n)))
            first = out[-1][1]
    while first < n:
        out.append((first, min(first + hp.SIZES[-1], n)))
        first = out[-1][1]
    return out


def _launches(fn, x, **kw):
    """fn on consecutive pieces of the inputs, the results joined along the sample axis"""
    n = len(next(iter(x.values())))
    parts = [fn(hp.take(x, slice(a, b)), **kw) for a, b in _chunks(n)]
    return {q: np.concatenate([np.asarray(p[q]) for p in parts]) for q in parts[0] if q != 'j_ion_coords'}


def _hold(rep, cap):
    print(hp.summary(rep))
    assert not rep['failures'], rep['failures']
    share = hp.excused_share(rep)
    assert share <= cap, f'{share:.4f} of the finite reference values excused, cap {cap}'


@pytest.mark.parametrize('name', list(hp.SETS))
@pytest.mark.parametrize('profile', (True, False), ids=('profile', 'reduced'))
def test_coupled_r1_against_the_reference(K, oracle, name, profile):
    from hallthrusterpem_amd.models import pem_v0_coupled
    x, ref = _set(name), _ref(name, K)
    with np.errstate(all='ignore'):
        got = _launches(pem_v0_coupled, x, profile=profile)
        want = oracle.coupled(x, K)
    bnd = hp.bounds(ref, hp.PATH_R1 if profile else hp.PATH_R1_REDUCED)
    _hold(hp.check(got, ref, bnd, f'pem_v0_coupled, {name}, {"profile" if profile else "reduced"}', oracle=want), hp.CAPS[name])


@pytest.mark.parametrize('name', list(hp.SETS))
def test_mixed_mode_is_the_rounded_fp64_profile_and_tile_layout_is_the_array_layout(name):
    """one batch per launch size: the fp32 profile of the mixed mode is the fp64 profile rounded once, its scalars the fp64 run's bits;
    the tile-interleaved layout gives the array layout's bits, with and without the profile"""
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    x = _set(name)
    n_all = len(x['P_b'])
    for a, b in _chunks(min(n_all, 800)):
        xs = hp.take(x, slice(a, b))
        runs = {}
        for key, kw in (('f64', {}), ('mixed', {'mixed': True}), ('tile', {'layout': 'tile'}), ('reduced', {'profile': False}),
                        ('tile_reduced', {'layout': 'tile', 'profile': False})):
            batch = CoupledBatch(b - a, **kw)
            batch.set_inputs({q: torch.from_numpy(v) for q, v in xs.items()})
            batch.run()
            torch.cuda.synchronize()
            runs[key] = {q: v.cpu().numpy() for q, v in batch.outputs().items()}

        def same(u, v, keys):
            bits = {np.dtype(bool): np.uint8, np.dtype(np.float32): np.int32, np.dtype(np.float64): np.int64}
            for q in keys:
                assert u[q].dtype == v[q].dtype and np.array_equal(u[q].view(bits[u[q].dtype]), v[q].view(bits[v[q].dtype])), (name, a, b, q)
        scalars = ('V_cc', 'div_angle', 'T_c', 'invalid', 'I_B0', 'T')
        same(runs['mixed'], runs['f64'], scalars)
        with np.errstate(all='ignore'):
            assert np.array_equal(runs['mixed']['j_ion'], runs['f64']['j_ion'].astype(np.float32), equal_nan=True), (name, a, b)
        same(runs['tile'], runs['f64'], scalars + ('j_ion',))
        same(runs['tile_reduced'], runs['reduced'], scalars)


@pytest.mark.parametrize('name', list(hp.SETS))
def test_plume_alone_r1(K, oracle, name):
    """current_density at one radius: I_B0 and T are inputs (the oracle's doubles), the plume stage alone"""
    from hallthrusterpem_amd.models import current_density
    x = _set(name)
    with np.errstate(all='ignore'):
        first = oracle.coupled(x, K)
        xp = dict({q: x[q] for q in PLUME_KEYS}, I_B0=first['I_B0'], T=first['T'])
        got = _launches(current_density, xp, sweep_radius=1.0)
        want = oracle.plume(*[x[q] for q in PLUME_KEYS], first['I_B0'], K, T=first['T'])
    ref = hp.reference(x, K, I_B0=first['I_B0'], T=first['T'])
    bnd = hp.bounds(ref, hp.PATH_R1)
    got['invalid'] = np.all(got['j_ion'] == 1e-20, axis=1)              # (the callable returns no flag: the fill is it)
    _hold(hp.check(got, ref, bnd, f'current_density, {name}, one radius', oracle=want), hp.CAPS[name])


@pytest.mark.parametrize('R', SWEEP_COUNTS)
def test_sweep_radii_against_the_reference(K, oracle, R):
    from hallthrusterpem_amd.models import current_density
    radii = np.linspace(0.5, 2.0, R)
    per_set = max(65, min(hp.SIZES[-1] + 193, 1_200_000 // (hp.NANG * R)))
    for name in hp.SETS:
        x = _set(name)
        n_all = len(x['P_b'])
        idx = np.unique(np.linspace(0, n_all - 1, per_set).astype(int))
        xs = hp.take(x, idx)
        with np.errstate(all='ignore'):
            first = oracle.coupled(xs, K)
            xp = dict({q: xs[q] for q in PLUME_KEYS}, I_B0=first['I_B0'], T=first['T'])
            got = _launches(current_density, xp, sweep_radius=radii)
            want = oracle.plume(*[xs[q] for q in PLUME_KEYS], first['I_B0'], K, T=first['T'], radii=radii)
        ref = hp.reference(xs, K, radii, I_B0=first['I_B0'], T=first['T'])
        bnd = hp.bounds(ref, hp.path_for_radii(R))
        got['invalid'] = np.all(got['j_ion'].reshape(len(idx), -1) == 1e-20, axis=1)
        _hold(hp.check(got, ref, bnd, f'current_density, {name}, {R} radii ({hp.path_for_radii(R)["gauss"]})', oracle=want), max(hp.CAPS[name], 0.0))


@pytest.mark.parametrize('rank', (1, 5, 6, 8))
@pytest.mark.parametrize('norm', ('none', 'log10'))
def test_fused_latent_kernel(K, oracle, rank, norm):
    """CoupledBatch.run_latent: the latents under the fma chain's bound, V_cc / div_angle / T_c / invalid under the R = 1 bound; an `out`
    view that starts on an odd double takes the per-lane store path and must give the same bits"""
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    from hallthrusterpem_amd.compression import SVDCompression
    rng = np.random.default_rng(100 + rank)
    basis = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((hp.NANG, rank)))[0])
    comp = SVDCompression(norm=norm, rank=rank)
    comp.basis = torch.from_numpy(basis).cuda()
    for name in hp.SETS:
        x, ref = _set(name), _ref(name, K)
        n_all = len(x['P_b'])
        outs = []
        for a, b in _chunks(n_all):
            batch = CoupledBatch(b - a, profile=False)
            batch.set_inputs({q: torch.from_numpy(v[a:b]) for q, v in x.items()})
            lat = batch.run_latent(comp)
            buf = torch.empty((b - a) * rank + 1, dtype=torch.float64, device='cuda')
            odd = batch.run_latent(comp, out=buf[1:].view(b - a, rank))
            torch.cuda.synchronize()
            assert np.array_equal(lat.cpu().numpy(), odd.cpu().numpy(), equal_nan=True), (name, a, b)
            o = {q: v.cpu().numpy() for q, v in batch.outputs().items() if q in ('V_cc', 'div_angle', 'T_c', 'invalid')}
            o['latent'] = lat.cpu().numpy()
            outs.append(o)
        got = {q: np.concatenate([o[q] for o in outs]) for q in outs[0]}
        with np.errstate(all='ignore'):
            want = oracle.coupled(x, K)
        bnd = hp.bounds(ref, hp.PATH_R1)
        rep = hp.check(got, ref, bnd, f'run_latent, {name}, rank {rank}, norm {norm}', oracle=want)
        # the latents
        lat_ref, b_lat, lat_fill, b_fill = hp.latent_reference(ref, bnd, basis, norm == 'log10')
        sure_inv, sure_val = hp.flags(ref, bnd)
        with np.errstate(all='ignore'):
            g = got['latent'].astype(hp.LD)
            inv = got['invalid'].astype(bool)
            ratio = np.where(inv[:, None], np.abs(g - lat_fill) / b_fill, np.abs(g - lat_ref) / b_lat).astype(np.float64)
            decided = (sure_inv | sure_val) & ~bnd['overflowed'] & ~bnd['excused']['overflow'] & ~bnd['excused']['a1_zero']
            fin = np.isfinite(np.where(inv[:, None], lat_fill, lat_ref)) & decided[:, None]
            ratio = np.where(fin, np.where(np.isnan(ratio), np.inf, ratio), 0.0)
        rep['latent'] = {'compared': int(fin.sum()), 'excused': int((~decided).sum() * rank), 'finite': int(fin.sum() + (~decided).sum() * rank),
                         'ratio': float(ratio.max(initial=0.0)), 'worst': int(np.argmax(ratio))}
        if ratio.max(initial=0.0) > 1.0:
            rep['failures'].append(('latent: outside the bound', np.argwhere(ratio > 1.0)[:6].tolist()))
        _hold(rep, hp.CAPS[name])


def _thruster_inputs(n=3000):
    """the priors' thruster inputs, V_cc from the cathode stage in fp64; and eta_c = 1 - 2 a_1 at and next to zero"""
    x = hp.prior_set(n, seed=5)
    from hallthrusterpem_amd import constants
    ref = hp.reference(x, constants.TORR_2_PA)
    t = {'V_a': x['V_a'].copy(), 'V_cc': ref['V_cc'].astype(np.float64), 'mdot_a': x['mdot_a'].copy(), 'a_1': x['a_1'].copy()}
    edge = hp.neighbours(0.5, 8)
    t['a_1'][:len(edge)] = edge
    t['a_1'][len(edge):len(edge) + 6] = (0.2, np.nextafter(0.2, 1), np.nextafter(0.2, 0), 0.4999, 0.5001, 0.25)          # eta_m = 0
    t['V_cc'][40:50] = t['V_a'][40:50]                                                                             # v_exh = 0
    t['V_cc'][50:60] = np.nextafter(t['V_a'][50:60], 0)                                                            # ... and next to it
    return t


def test_cathode_kernel(K):
    from hallthrusterpem_amd.models import cathode_coupling
    x = hp.prior_set(3000, seed=4)
    x['V_vac'][:200] = 0.0                    # V_cc a difference of nearly equal terms ...
    x['P_b'][:100], x['P_T'][:100], x['Pstar'][:100] = 1e-4, 1e-5, 1e-5          # ... and below zero: the lower clamp
    x['V_a'][200:300] = 5.0                   # the upper clamp
    got = _launches(cathode_coupling, {q: x[q] for q in ('P_b', 'V_a', 'T_e', 'V_vac', 'Pstar', 'P_T')})
    ref = hp.cathode_reference({q: v.astype(hp.LD) for q, v in x.items()}, K)
    with np.errstate(all='ignore'):
        g = got['V_cc'].astype(hp.LD)
        ratio = (np.abs(g - ref['V_cc']) / ref['bound_V']).astype(np.float64)
        ratio = np.where(g == ref['V_cc'], 0.0, ratio)
    print(f'cathode_kernel: 3000 samples, worst error/bound {ratio.max():.3f}; on the lower clamp {int((ref["V_cc"] == 0).sum())}, on the upper {int((ref["V_cc"] == x["V_a"]).sum())}')
    assert np.all((g >= ref['V_lo']) & (g <= ref['V_hi'])) and ratio.max() <= 1.0
    assert (ref['V_cc'] == 0).sum() > 10 and (ref['V_cc'] == x['V_a']).sum() > 10


def test_thruster_kernel_all_eight_outputs():
    from hallthrusterpem_amd.models.thruster import thruster_analytic
    t = _thruster_inputs()
    got = _launches(thruster_analytic, t)
    ref = hp.thruster_reference(t['V_a'], t['V_cc'], t['mdot_a'], t['a_1'])
    lines = []
    with np.errstate(all='ignore'):
        for q in hp.THRUSTER_OUT:
            g, w, b = got[q].astype(hp.LD), ref[q], ref['b_' + q]
            assert np.array_equal(np.isnan(got[q]), np.isnan(w.astype(np.float64))) and np.array_equal(np.isinf(got[q]), np.isinf(w.astype(np.float64))), q
            fin = np.isfinite(w)
            ratio = np.where(fin & (g != w), (np.abs(g - w) / b).astype(np.float64), 0.0)
            lines.append(f'{q} {ratio.max():.3f}')
            assert ratio.max() <= 1.0, (q, int(np.argmax(ratio)), float(ratio.max()))
    print('thruster_kernel: worst error/bound ' + ', '.join(lines))
    assert np.isinf(ref['I_d'].astype(np.float64)).sum() >= 1          # eta_c = 0 exactly is among the samples


@pytest.mark.parametrize('ncells', (1, 7, 200))
def test_thruster_uion_kernel(ncells):
    from hallthrusterpem_amd.models.thruster import thruster_analytic
    t = hp.take(_thruster_inputs(), slice(0, 400))
    if ncells == 1:
        # z = range(z0, z1, length = 1) has no step: the entry point refuses a grid of fewer than two nodes, it does not divide by zero
        from hallthrusterpem_amd._lib import PemHipError
        with pytest.raises(PemHipError, match='at least 2 grid points'):
            thruster_analytic(hp.take(t, slice(0, 5)), num_cells=1)
        return
    got = _launches(lambda xs: {q: v for q, v in thruster_analytic(xs, num_cells=ncells).items() if q in ('v_exh', 'u_ion')}, t)
    u, b, z = hp.uion_reference(got['v_exh'], 0.0, 0.08, ncells)
    with np.errstate(all='ignore'):
        g = got['u_ion'].astype(hp.LD)
        assert np.array_equal(np.isnan(got['u_ion']), np.isnan(u.astype(np.float64)))
        ratio = np.where(np.isfinite(u) & (g != u), (np.abs(g - u) / b).astype(np.float64), 0.0)
    print(f'thruster_uion_kernel, {ncells} cells: worst error/bound {ratio.max(initial=0.0):.3f}')
    assert ratio.max(initial=0.0) <= 1.0
    zs = thruster_analytic(hp.take(t, slice(0, 2)), num_cells=ncells)['u_ion_coords']
    assert np.allclose(zs, z, rtol=4 * hp.U, atol=0, equal_nan=True)


def test_grid_independence_of_the_coupled_kernel():
    """The small launches above run on the persistent grid.  A batch with more than three rounds of work takes the one-shot grid
    (the size comes from pem_persistent_grid): every copy of a sample in it must carry the bits of the small run, in
    all three modes -- the bound checked on the small run then holds in both grid modes."""
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd.batch import CoupledBatch
    n0 = hp.SIZES[-1]
    x = hp.take(_set('priors'), slice(0, n0))
    rows = torch.stack([torch.from_numpy(x[q]) for q in hp.COUPLED_INPUTS]).cuda()
    for key, kw, mode in (('profile', {}, 1), ('reduced', {'profile': False}, 0), ('mixed', {'mixed': True}, 2)):
        cus, per_cu = _lib.coupled_occupancy(mode)
        reps = (3 * cus * per_cu * 4 * 64) // n0 + 2
        n_big = reps * n0
        wg_big, _ = _lib.persistent_grid(n_big, cus, per_cu, True)
        wg_small, _ = _lib.persistent_grid(n0, cus, per_cu, True)
        if key != 'reduced':          # (the reduced mode is not memory bound and keeps the persistent grid: it is run at that size all the same)
            assert wg_big == -(-((n_big + 63) // 64) // 4) and wg_big > 3 * cus * per_cu, (wg_big, cus, per_cu)
        assert wg_small <= cus * per_cu
        small, big = CoupledBatch(n0, **kw), CoupledBatch(n_big, **kw)
        small.inputs.copy_(rows)
        big.inputs.copy_(rows.repeat(1, reps))
        small.run()
        big.run()
        torch.cuda.synchronize()
        so, bo = small.outputs(), big.outputs()
        for q in so:
            s, b = so[q], bo[q]
            if s.dtype.is_floating_point:
                s, b = s.view(torch.int32 if s.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64)
            assert bool((b.reshape((reps,) + tuple(s.shape)) == s[None]).all()), (key, q)
        print(f'{key}: {n_big} samples in {wg_big} workgroups against {n0} in {wg_small}: bit-identical')
        del small, big
