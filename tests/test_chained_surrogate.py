"""The component chain on the GPU: pem_sparse_predict_chain_f64_dev against three single-table launches (bit for bit) and the
long-double composition over its dispatch space, and PemV0System.fit(components=True) end to end."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

N_EXT = 5
N_DIM = N_EXT + 2          # the coupling slots: the last two as the host numbers them, or interior ones (the kernel takes any two)


def _stage(rng, n_out, outer, slots, big=False):
    """a table of three grids over `slots`: the constant grid, one with 1 active slot and one with outer + 1 (levels 1..2, one
    level-4 dimension when `big`), coefficients 1, -0.5, 1"""
    import hp_reference as hp
    betas = [(0,) * N_DIM]
    one = [0] * N_DIM
    one[slots[-1]] = 2
    betas.append(tuple(one))
    act = sorted(rng.choice(slots, outer + 1, replace=False))
    lv = [int(rng.integers(1, 3)) for _ in act]
    if big:
        lv[0] = 4
    betas.append(hp.beta_of(N_DIM, dict(zip(act, lv))))
    values = [rng.uniform(-1, 1, (int(np.prod([hp.node_count(l) for l in b])), n_out)) for b in betas]
    return betas, [1.0, -0.5, 1.0], values


def _upload(betas, coefs, values):
    import torch
    import hp_reference as hp
    idx, vals = hp.index_table(betas, values)
    return (torch.from_numpy(idx).cuda(), torch.tensor(coefs, dtype=torch.float64, device='cuda'), torch.from_numpy(vals).cuda(),
            len(betas), values[0].shape[1], max(sum(1 for l in b if l > 0) for b in betas), max(max(b) for b in betas))


def _single(tab, t, n, field=None):
    """one existing launch: pem_sparse_predict_f64_dev, or _field_f64_dev with field = (lat0, rank, basis, out_field)"""
    import torch
    from hallthrusterpem_amd import _lib
    idx, coef, vals, nb, n_out, na, lv = tab
    out = torch.empty((n_out, n), dtype=torch.float64, device='cuda')
    p = lambda x: C.c_void_p(x.data_ptr())                                                   # noqa: E731
    lib = _lib.load()
    if field is None:
        _lib.check(lib.pem_sparse_predict_f64_dev(n, N_DIM, nb, p(idx), p(coef), p(vals), n_out, p(t), t.stride(0), p(out), n, na, lv, None))
    else:
        lat0, rank, basis, f = field
        _lib.check(lib.pem_sparse_predict_field_f64_dev(n, N_DIM, nb, p(idx), p(coef), p(vals), n_out, p(t), t.stride(0), p(out), n, na, lv,
                                                        lat0, rank, 91, 1, 1.0, p(basis), p(f), None))
    return out


def _domain(y):
    lo, hi = float(y.min()), float(y.max())
    w = max(hi - lo, 1e-3)
    return lo - 0.05 * w, 1.1 * w


def _run_case(rng, n, n_plume, outers, lat0=0, rank=0, pad=0, big=False, ld_check=64, slots=(N_EXT, N_EXT + 1)):
    """rank 0: no field; else the field rebuilt from plume outputs lat0 .. lat0 + rank - 1"""
    import torch
    import chain_np
    import hp_reference as hp
    from hallthrusterpem_amd import _lib
    VCC, IB0 = slots
    field = rank > 0
    ext = [d for d in range(N_DIM) if d not in slots]
    stages = [_stage(rng, 1, outers[0], ext, big), _stage(rng, 2, outers[1], ext[:4] + [VCC], big),
              _stage(rng, n_plume, outers[2], ext[:4] + [IB0], big)]
    tabs = [_upload(*s) for s in stages]
    ld = n + pad
    tfull = torch.zeros((N_DIM, ld), dtype=torch.float64, device='cuda')
    tfull[ext, :n] = torch.rand((N_EXT, n), dtype=torch.float64, device='cuda') * 2 - 1
    # the reference: three single-table launches and the coupling map in torch, left to right
    # (the widths as device tensors: torch divides by a host scalar as a multiplication by its reciprocal, not a division)
    vcc = _single(tabs[0], tfull, n)[0]
    vmap = _domain(vcc)
    tfull[VCC, :n] = 2.0 * (vcc - vmap[0]) / torch.tensor(vmap[1], dtype=torch.float64, device='cuda') - 1.0
    thr = _single(tabs[1], tfull, n)
    imap = _domain(thr[0])
    tfull[IB0, :n] = 2.0 * (thr[0] - imap[0]) / torch.tensor(imap[1], dtype=torch.float64, device='cuda') - 1.0
    basis = torch.from_numpy(rng.uniform(-0.3, 0.3, (91, max(rank, 1))) * min(1.0, 4.0 / max(rank, 1))).cuda() if field else None
    f_ref = torch.empty((n, 91), dtype=torch.float64, device='cuda') if field else None
    plu = _single(tabs[2], tfull, n, (lat0, rank, basis, f_ref) if field else None)
    # the chain: t holds the external rows only, in slot order (padded); out is padded too
    t = tfull[ext].contiguous()
    out = torch.full((4 + n_plume, ld + 3), np.nan, dtype=torch.float64, device='cuda')
    f = torch.empty((n, 91), dtype=torch.float64, device='cuda') if field else None
    arr = (_lib.SurrStage * 3)(*[_lib.SurrStage(a.data_ptr(), b.data_ptr(), c.data_ptr(), nb, no, na, lv) for a, b, c, nb, no, na, lv in tabs])
    _lib.check(_lib.load().pem_sparse_predict_chain_f64_dev(
        n, N_DIM, VCC, IB0, arr, vmap[0], vmap[1], imap[0], imap[1], C.c_void_p(t.data_ptr()), ld, C.c_void_p(out.data_ptr()), ld + 3,
        lat0, rank, 91, 1, 1.0, C.c_void_p(basis.data_ptr()) if field else None, C.c_void_p(f.data_ptr()) if field else None, None))
    torch.cuda.synchronize()
    got = out[:, :n]
    assert torch.equal(got[0], vcc) and torch.equal(got[1], thr[0]) and torch.equal(got[2], thr[1]), 'V_cc / I_B0 / T'
    assert torch.equal(got[3], plu[0]) and torch.equal(got[5:], plu[1:]), 'div_angle / plume outputs'
    assert torch.isnan(out[:, n:]).all(), 'wrote past n'
    if field:
        assert torch.equal(f, f_ref), 'field'
    tc = (thr[1] * torch.cos(plu[0])).cpu().numpy()
    assert np.all(np.abs(got[4].cpu().numpy() - tc) <= 2 * np.spacing(np.abs(tc))), 'T_c within 2 ulp'
    # long-double composition on a subset of the points
    sub = np.linspace(0, n - 1, min(n, ld_check)).astype(int)
    want = chain_np.compose_ld(stages, t[:, sub].cpu().numpy(), VCC, IB0, vmap, imap)
    g = got[:, sub].cpu().numpy()
    assert np.all(np.abs(g - want.astype(np.float64)) <= 1e-11 * np.maximum(np.abs(want).max(axis=1, keepdims=True), 1.0)), 'long double'
    if field:
        plume = np.concatenate([want[3:4], want[5:]])                                    # the plume stage's outputs 0 .. n_out - 1
        fw = 10.0 ** (plume[lat0:lat0 + rank].T @ basis.cpu().numpy().astype(hp.LD).T)
        assert np.all(np.abs(f[sub].cpu().numpy() - fw.astype(np.float64)) <= 1e-11 * np.abs(fw).astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize('n_plume', range(1, 17))
def test_chain_equals_three_launches_bit_for_bit(n_plume):
    import torch
    torch.manual_seed(n_plume)
    rng = np.random.default_rng(n_plume)
    # no field; the field from every latent after div_angle (rank n_out - 1, up to 15); at n_out 16 the field from all 16 outputs.
    # Odd widths put the coupling slots inside the coordinate table (V_cc at 1, I_B0 at 4), even ones last.
    fields = [(0, 0)] + ([(1, n_plume - 1)] if n_plume > 1 else []) + ([(0, 16)] if n_plume == 16 else [])
    for k, (lat0, rank) in enumerate(fields):
        outers = ((n_plume + k) % 5, (n_plume + 1 + k) % 5, (n_plume + 2 + k) % 5)
        _run_case(rng, 1000 + 3 * n_plume, n_plume, outers, lat0, rank, pad=7 * k, big=(n_plume % 4 == 0),
                  slots=(1, 4) if n_plume % 2 else (N_EXT, N_EXT + 1))


@pytest.mark.gpu
def test_chain_grid_stride_past_two_rounds():
    import torch
    torch.manual_seed(0)
    _run_case(np.random.default_rng(99), 2048 * 256 * 2 + 77, 5, (2, 3, 2), 1, 4, pad=13, ld_check=32, slots=(4, 2))


FIXED_SMALL = dict(P_b=1e-5, V_a=300.0, T_e=2.0, Pstar=3e-5, P_T=2e-5, mdot_a=5e-6, a_1=0.01, c0=0.5, c1=0.5, c4=1e20, c5=1e16,
                   sigma_cex=55e-20)


@pytest.mark.gpu
def test_fit_components_small_case(tmp_path):
    import torch
    from hallthrusterpem_amd.chain import ChainedSurrogate
    from hallthrusterpem_amd.surrogate import SparseGridSurrogate
    from hallthrusterpem_amd.system import PemV0System
    system = PemV0System(seed=2)
    xt = system.sample_inputs(2000, normalize=False)
    xt.update({k: np.full(2000, v) for k, v in FIXED_SMALL.items()})
    yt = system.predict(xt, use_model='best', normalized_inputs=False)
    hist = system.fit(targets=['V_cc', 'div_angle'], fixed=FIXED_SMALL, max_iter=8, max_tol=0.0, num_refine=500, test_set=(xt, yt),
                      components=True)
    assert isinstance(system.surrogate, ChainedSurrogate)
    assert len(hist) == 8 and all(h['component'] in PemV0System.COMPONENT_NAMES for h in hist)
    assert all(set(h['component_evals']) == set(PemV0System.COMPONENT_NAMES) for h in hist)
    cost_alloc, model_cost, overhead, evals = system.get_allocation()
    shares = [model_cost[c]['()'] for c in PemV0System.COMPONENT_NAMES]
    assert abs(sum(shares) - 1.0) < 1e-15 and overhead == 0.0 and evals.shape == (8,)
    total = sum(cost_alloc[c]['()'] for c in PemV0System.COMPONENT_NAMES)
    assert np.isclose(total, evals.sum(), rtol=1e-14) and np.isclose(total, hist[-1]['model_evals'], rtol=1e-14)
    assert all(np.isclose(cost_alloc[c]['()'], hist[-1]['component_evals'][c] * system[c].model_costs['()']) for c in cost_alloc)
    assert hist[-1]['test_error']['V_cc'] < 1e-2 and hist[-1]['test_error']['div_angle'] < 5e-2
    pred = system.predict(xt, normalized_inputs=False)
    assert {'V_cc', 'I_B0', 'T', 'div_angle', 'T_c'} <= set(pred) and pred['I_B0'].shape == (2000,)
    for k in ('I_B0', 'T', 'T_c'):
        assert np.linalg.norm(pred[k] - yt[k]) / np.linalg.norm(yt[k]) < 1e-2, k
    assert set(system.predict(xt, normalized_inputs=False, targets=['V_cc'])) == {'V_cc'}
    path = system.save_to_file('chain.pkl', save_dir=tmp_path)
    again = PemV0System.load_from_file(path)
    p2 = again.predict(xt, normalized_inputs=False)
    assert set(p2) == set(pred) and all(np.array_equal(p2[k], pred[k]) for k in pred)
    assert again.get_allocation()[1] == model_cost
    system.fit(targets=['V_cc'], fixed=FIXED_SMALL, max_iter=2, max_tol=0.0, num_refine=200)
    assert isinstance(system.surrogate, SparseGridSurrogate)
    assert all(abs(c.model_costs['()'] - 1 / 3) < 1e-15 for c in system.components)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_configs3_in_component_form():
    """BASELINE configs[3] (test_config_5e5_candidates_and_batched_predict's box) trained one surrogate per component; 5e5 seeded
    test points through the true coupled model"""
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    from hallthrusterpem_amd.chain import COST_SHARES, ChainedSurrogate
    fixed = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6, 'a_1': 0.01, 'sigma_cex': 55e-20, 'c4': 1e20, 'c5': 1e16}
    varied = ('T_e', 'V_vac', 'Pstar', 'P_T', 'c0', 'c1', 'c2', 'c3')
    s = ChainedSurrogate(varied, fixed)
    assert s.compression.relative_error <= 0.01
    n = 500_000
    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    t = torch.rand((len(varied), n), dtype=torch.float64, device='cuda', generator=g) * 2 - 1
    x = {k: np.full(n, v) for k, v in fixed.items()}
    x.update(s.stages[0].to_physical(t[:4].cpu().numpy()))
    x.update(s.stages[2].to_physical(torch.cat([t[4:], t[:1]]).cpu().numpy()))       # c0..c3 (the last row, I_B0, is replaced)
    del x['I_B0']
    batch = CoupledBatch(n, profile=True)
    batch.set_inputs(x)
    batch.run()
    lt = torch.log10(batch.j_ion)
    it = 0
    for it in range(1, 801):
        s.refine_step(num_refine=1000, seed=it)
        if it % 40:
            continue
        y = s.predict_fields(t)
        errs = {k: float(torch.linalg.norm(y[k] - batch.outputs()[k]) / torch.linalg.norm(batch.outputs()[k])) for k in ('V_cc', 'div_angle', 'T_c')}
        errs['j_ion'] = float(torch.linalg.norm(torch.log10(y['j_ion']) - lt) / torch.linalg.norm(lt))
        if max(errs['V_cc'], errs['div_angle'], errs['T_c']) < 1e-3 and errs['j_ion'] <= 0.01:
            break
    assert errs['V_cc'] < 1e-3 and errs['div_angle'] < 1e-3 and errs['T_c'] < 1e-3 and errs['j_ion'] <= 0.01, (it, errs)
    for k, slot in (('V_cc', 0), ('I_B0', 1)):
        lo, hi = s.domains[slot]
        assert lo <= float(y[k].min()) and float(y[k].max()) <= hi, k
    weighted = s.cost_weighted_evals()
    assert weighted < 17419, (weighted, s.model_evals)          # the monolith's 160 iterations (test_config_5e5_candidates_and_batched_predict)
    print(f'\nconfigs[3] in component form: {it} iterations, evaluations per component {s.model_evals}, cost-weighted {weighted:.0f} '
          f'(shares {COST_SHARES}), monolith 17419; errors {errs}')
