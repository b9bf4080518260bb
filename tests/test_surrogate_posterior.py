"""The surrogate posterior on the GPU: pem_chain_system_loglik_f64_dev against the composition it replaces
(pem_sparse_predict_chain_f64_dev with the field written, then long-double sums) over its dispatch space, and
calibration.SurrogatePosterior on a small real fit."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

NORMS = {1: 1.0, 2: 0.5, 0: 1.0}            # PEM_NORM_*: its norm_scale
DISCHARGE = (4.5, 0.2)


def _p(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _chain_case(rng, n, n_plume, outers, rank, slots, big, pad):
    """random stage tables as test_chained_surrogate._run_case builds them (the same value ranges), the coupling domains from
    single-table launches, and the chain launch's rows and field: the reference of everything below"""
    import torch
    import test_chained_surrogate as tc
    from hallthrusterpem_amd import _lib
    VCC, IB0 = slots
    ext = [d for d in range(tc.N_DIM) if d not in slots]
    stages = [tc._stage(rng, 1, outers[0], ext, big), tc._stage(rng, 2, outers[1], ext[:4] + [VCC], big),
              tc._stage(rng, n_plume, outers[2], ext[:4] + [IB0], big)]
    tabs = [tc._upload(*s) for s in stages]
    ld = n + pad
    tfull = torch.zeros((tc.N_DIM, ld), dtype=torch.float64, device='cuda')
    tfull[ext, :n] = torch.rand((tc.N_EXT, n), dtype=torch.float64, device='cuda') * 2 - 1
    vcc = tc._single(tabs[0], tfull, n)[0]
    vmap = tc._domain(vcc)
    tfull[VCC, :n] = 2.0 * (vcc - vmap[0]) / torch.tensor(vmap[1], dtype=torch.float64, device='cuda') - 1.0
    imap = tc._domain(tc._single(tabs[1], tfull, n)[0])
    t = tfull[ext].contiguous()
    arr = (_lib.SurrStage * 3)(*[_lib.SurrStage(a.data_ptr(), b.data_ptr(), c.data_ptr(), nb, no, na, lv) for a, b, c, nb, no, na, lv in tabs])
    basis = torch.from_numpy(rng.uniform(-0.3, 0.3, (91, max(rank, 1))) * min(1.0, 4.0 / max(rank, 1))).cuda() if rank else None
    return dict(n=n, ld=ld, t=t, arr=arr, keep=tabs, vmap=vmap, imap=imap, slots=slots, n_plume=n_plume, rank=rank, basis=basis)


def _chain(cs, norm, first=0, count=None):
    """pem_sparse_predict_chain_f64_dev over samples first .. first + count - 1: (rows padded with NaN columns, field or None)"""
    import torch
    from hallthrusterpem_amd import _lib
    n = cs['n'] - first if count is None else count
    out = torch.full((4 + cs['n_plume'], n + 3), np.nan, dtype=torch.float64, device='cuda')
    f = torch.empty((n, 91), dtype=torch.float64, device='cuda') if cs['rank'] else None
    _lib.check(_lib.load().pem_sparse_predict_chain_f64_dev(
        n, 7, cs['slots'][0], cs['slots'][1], cs['arr'], *cs['vmap'], *cs['imap'], C.c_void_p(cs['t'].data_ptr() + 8 * first), cs['ld'],
        _p(out), n + 3, 1, cs['rank'], 91, norm, NORMS[norm], _p(cs['basis']), _p(f), None))
    return out, f


def _loglik(cs, norm, rec, span, n_cond, a_1=None, want_out=True, want_pred=True, first=0, count=None, ld_pred_pad=5):
    import torch
    from hallthrusterpem_amd import _lib
    n = cs['n'] - first if count is None else count
    n_rec = rec.shape[0]
    rows = -(-n // n_cond)
    ll = torch.full((n + 2,), np.nan, dtype=torch.float64, device='cuda')
    out = torch.full((4 + cs['n_plume'], n + 3), np.nan, dtype=torch.float64, device='cuda') if want_out else None
    pred = torch.full((rows + 1, n_rec + ld_pred_pad), np.nan, dtype=torch.float64, device='cuda') if want_pred else None
    _lib.check(_lib.load().pem_chain_system_loglik_f64_dev(
        n, 7, cs['slots'][0], cs['slots'][1], cs['arr'], *cs['vmap'], *cs['imap'], C.c_void_p(cs['t'].data_ptr() + 8 * first), cs['ld'],
        1, cs['rank'], 91, norm, NORMS[norm], _p(cs['basis']), n_cond, n_rec, _p(rec), _p(span),
        C.c_void_p(a_1.data_ptr() + 8 * first) if a_1 is not None else None, DISCHARGE[0], DISCHARGE[1], _p(ll), _p(out), n + 3, _p(pred),
        n_rec + ld_pred_pad, None))
    torch.cuda.synchronize()
    return ll, out, pred


MIXES = {                                                # {kind: count} per condition, cycled over n_cond
    'jion': [{0: 40}, {0: 7}, {0: 12}],
    'vcc': [{1: 1}, {1: 2}],
    't': [{2: 1}],
    'all': [{0: 9, 1: 1, 2: 1}, {1: 1, 2: 2}, {0: 5}, {0: 3, 2: 1}, {1: 1}],
}

CASES = [
    # n_plume, rank, n_cond, n, mix, outers, slots, big, norm
    (1, 0, 3, 1003, 'vcc', (1, 2, 0), (5, 6), False, 1),
    (1, 0, 1, 777, 't', (0, 1, 2), (1, 4), False, 1),
    (2, 1, 16, 1009, 'jion', (2, 3, 1), (5, 6), False, 1),
    (3, 2, 3, 1010, 'all', (3, 4, 2), (1, 4), False, 2),
    (4, 3, 16, 1021, 'jion', (4, 0, 3), (5, 6), True, 1),         # 150 KB of bases and 14 KB of tables: read through the cache
    (6, 5, 1, 1001, 'jion', (0, 1, 4), (4, 2), False, 0),
    (6, 3, 3, 1207, 'all', (2, 2, 2), (5, 6), False, 1),           # fewer latents than the plume stage has outputs
    (16, 15, 16, 1013, 'all', (1, 2, 3), (1, 4), True, 1),
    (5, 4, 3, 2048 * 256 * 2 + 79, 'all', (2, 3, 2), (4, 2), False, 1),      # more than two grid-stride rounds
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=lambda c: f'w{c[0]}r{c[1]}c{c[2]}n{c[3]}{c[4]}')
def test_kernel_against_the_composition(case):
    import torch
    import chain_loglik_np as cl
    import hp_likelihood as hl
    from test_surrogate_posterior_host import _table
    n_plume, rank, n_cond, n, mix, outers, slots, big, norm = case
    assert n % n_cond or n_cond == 1
    assert n % 256
    torch.manual_seed(n)
    rng = np.random.default_rng(n + n_plume)
    cs = _chain_case(rng, n, n_plume, outers, rank, slots, big, pad=11)
    rec_h, span_h = _table(rng, [MIXES[mix][c % len(MIXES[mix])] for c in range(n_cond)])
    rec, span = torch.from_numpy(rec_h).cuda(), torch.from_numpy(span_h).cuda()
    n_rec = rec_h.shape[0]
    a_1 = torch.from_numpy(10.0 ** rng.uniform(-2.5, -1.0, n)).cuda()
    rows_ref, field = _chain(cs, norm)
    ll, out, pred = _loglik(cs, norm, rec, span, n_cond)
    # (a) the chain's rows, padding included
    assert torch.equal(out.isnan(), rows_ref.isnan()) and torch.equal(out[:, :n], rows_ref[:, :n]), 'rows'
    assert torch.isnan(ll[n:]).all() and torch.isfinite(ll[:n]).all()
    # (b) the model values, bit for bit, on a subset of the samples (all of a small batch); what is not a record stays NaN
    sub = np.arange(n) if n < 5000 else np.unique(np.concatenate([np.arange(600), np.linspace(0, n - 1, 600).astype(int), np.arange(n - 600, n)]))
    kind, w, y, s, k = cl.sample_tables(rec_h, span_h, n_cond, sub)
    r_h = rows_ref[:, sub].cpu().numpy()
    want = np.full(kind.shape, np.nan)
    if rank:
        f_h = field[sub].cpu().numpy()
        kj = np.where(kind == cl.JION, k, 0)
        mj = hl.interp_model(w, np.take_along_axis(f_h, kj, axis=1), np.take_along_axis(f_h, kj + 1, axis=1))
        want = np.where(kind == cl.JION, mj, want)
    want = np.where(kind == cl.VCC, r_h[0][:, None], want)
    want = np.where(kind == cl.T, r_h[2][:, None], want)
    assert np.isfinite(want[kind >= 0]).all()
    got = pred[torch.from_numpy(sub // n_cond).cuda()][:, :n_rec].cpu().numpy()              # row d of sample i = d n_cond + c
    assert np.array_equal(np.where(kind >= 0, got, np.nan), want, equal_nan=True), 'pred'
    written = torch.zeros(pred.shape, dtype=torch.bool, device='cuda')
    kc = cl.sample_tables(rec_h, span_h, n_cond, np.arange(n_cond))[0] >= 0                  # [n_cond][n_rec]: the records of each condition
    full = torch.from_numpy(kc.any(axis=0)).cuda()
    written[:n // n_cond, :n_rec] = full
    if n % n_cond:
        written[n // n_cond, :n_rec] = torch.from_numpy(kc[:n % n_cond].any(axis=0)).cuda()
    assert torch.equal(~pred.isnan(), written), 'padding records, padding columns and rows past n stay NaN'
    # (c) the sum within record_sum's bound of the long-double sum of these model values
    ref, bound = cl.sum_ref(want, kind, y, s)
    hl.assert_within(ll[:n].cpu().numpy()[sub], ref, bound, 'loglik')
    # ... and of the composition: the field interpolated exactly
    ref, bound = cl.composition_ref(f_h if rank else None, r_h, sub, rec_h, span_h, n_cond)
    hl.assert_within(ll[:n].cpu().numpy()[sub], ref, bound, 'loglik against the composition')
    # (d) the discharge term
    ll_d, _, pred_d = _loglik(cs, norm, rec, span, n_cond, a_1=a_1)
    assert torch.equal(pred_d.isnan(), pred.isnan()) and torch.equal(pred_d.nan_to_num(), pred.nan_to_num())
    a_h = a_1.cpu().numpy()[sub]
    ref, bound = cl.sum_ref(want, kind, y, s, r_h[1], a_h, DISCHARGE)
    hl.assert_within(ll_d[:n].cpu().numpy()[sub], ref, bound, 'loglik with the discharge term')
    assert not torch.equal(ll_d[:n], ll[:n])
    # (e) the same bits whatever is asked for
    for wo, wp in ((False, False), (True, False), (False, True)):
        assert torch.equal(_loglik(cs, norm, rec, span, n_cond, a_1=a_1, want_out=wo, want_pred=wp)[0][:n], ll_d[:n]), (wo, wp)
    # (f) a shifted, truncated batch that keeps i mod n_cond
    first, count = 5 * n_cond, n - 5 * n_cond - 301
    ll_s, out_s, pred_s = _loglik(cs, norm, rec, span, n_cond, a_1=a_1, first=first, count=count)
    assert torch.equal(ll_s[:count], ll_d[first:first + count]) and torch.equal(out_s[:, :count], out[:, first:first + count])
    whole = count // n_cond
    assert torch.equal(pred_s[:whole].nan_to_num(), pred[5:5 + whole].nan_to_num())


@pytest.mark.gpu
def test_kernel_marks_what_the_chain_cannot_give():
    import torch
    from test_surrogate_posterior_host import _table
    rng = np.random.default_rng(4)
    torch.manual_seed(4)
    rec_h, span_h = _table(rng, [{0: 3, 1: 1}, {1: 1, 3: 2}, {2: 1}])                       # u_ion records in the second condition
    rec, span = torch.from_numpy(rec_h).cuda(), torch.from_numpy(span_h).cuda()
    cond = torch.arange(500, device='cuda') % 3
    cs = _chain_case(rng, 500, 3, (1, 1, 1), 2, (5, 6), False, pad=0)
    ll = _loglik(cs, 1, rec, span, 3)[0][:500]
    assert torch.equal(ll.isnan(), cond == 1)
    cs = _chain_case(rng, 500, 3, (1, 1, 1), 0, (5, 6), False, pad=0)                       # no basis: the j_ion records of condition 0
    ll, _, pred = _loglik(cs, 1, rec, span, 3)
    assert torch.equal(ll[:500].isnan(), cond != 2) and torch.isfinite(ll[:500][cond == 2]).all()


# ---- calibration.SurrogatePosterior on a small real fit --------------------------------------------------------------------------
VARIED = ('P_b', 'V_a', 'T_e', 'V_vac', 'mdot_a', 'a_1', 'c0', 'c3')
FIXED = {'Pstar': 5e-5, 'P_T': 5e-5, 'c1': 0.3, 'c2': 5.0, 'c4': 1e20, 'c5': 1e16, 'sigma_cex': 55e-20}
NAMES = ('T_e', 'V_vac', 'c0', 'c3')
TRUTH = {'T_e': 3.0, 'V_vac': 30.0, 'c0': 0.35, 'c3': 0.6}


@pytest.fixture(scope='module')
def fit():
    import torch
    from hallthrusterpem_amd.calibration import OPERATING
    from hallthrusterpem_amd.chain import ChainedSurrogate
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.models.coupled import pem_v0_coupled
    from hallthrusterpem_amd.models.thruster import thruster_analytic
    s = ChainedSurrogate(VARIED, FIXED, max_level=3)
    for it in range(10):
        s.refine_step(num_refine=500, seed=it)
    rng = np.random.default_rng(8)
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)   # noqa: E731
    alpha = np.linspace(-1.5, 1.5, 14)
    grid = np.linspace(0, np.pi / 2, 91)

    def model(o):
        x = {k: np.full(o.shape[0], v) for k, v in {**FIXED, **TRUTH, 'a_1': 0.02}.items()}
        x.update({k: o[:, j] for j, k in enumerate(OPERATING)})
        out = pem_v0_coupled(x)
        th = thruster_analytic({'V_a': x['V_a'], 'V_cc': out['V_cc'], 'mdot_a': x['mdot_a'], 'a_1': x['a_1']})
        return out, th
    ops = {'V_cc': op(3), 'T': op(2), 'jion': op(3)}
    data = {}
    out, _ = model(ops['V_cc'])
    data['V_cc'] = {'x': ops['V_cc'], 'y': np.asarray(out['V_cc']), 'var_y': np.full(3, 0.5 ** 2)}
    _, th = model(ops['T'])
    data['T'] = {'x': ops['T'], 'y': np.asarray(th['T']), 'var_y': (0.05 * np.asarray(th['T'])) ** 2}
    out, _ = model(ops['jion'])
    j = np.stack([np.interp(np.abs(alpha), grid, np.asarray(out['j_ion'])[e]) for e in range(3)])
    data['jion'] = {'x': ops['jion'], 'y': j, 'var_y': (0.2 * j + 1e-3) ** 2, 'loc': np.stack([np.ones(alpha.size), alpha], 1)}
    torch.cuda.synchronize()
    return s, SystemLikelihood(data)


def _thetas(K, seed, outside=()):
    import torch
    from hallthrusterpem_amd.sampling import PEM_V0_PRIORS
    rng = np.random.default_rng(seed)
    th = np.stack([rng.uniform(PEM_V0_PRIORS[k].a, PEM_V0_PRIORS[k].b, K) for k in NAMES], axis=1)
    for row, col, v in outside:
        th[row, col] = v
    return torch.from_numpy(th).cuda()


@pytest.mark.gpu
def test_posterior_against_the_composition(fit):
    import torch
    import chain_loglik_np as cl
    import hp_likelihood as hl
    from hallthrusterpem_amd.calibration import SurrogatePosterior
    s, lik = fit
    K, M = 6, 7
    post = SurrogatePosterior(NAMES, lik, s, n_chains=K, n_nuisance=M, seed=3, fresh_nuisance=False)
    assert post.chain_discharge == (4.5, 0.2) and post.discharge is None
    theta = _thetas(K, 1, outside=[(2, 0, 5.5), (4, 3, 0.1)])                  # T_e above, c3 below their supports
    for with_prior in (False, True):
        got = (post.log_posterior if with_prior else post.log_likelihood)(theta).cpu().numpy()
        # the composition: the chain launch with the field written, long-double sums, the marginal, the prior
        rows, field = s.predict(post.coords)
        idx = np.arange(post.n)
        a_1 = post.batch.inputs[post._a1_row].cpu().numpy()
        ll, bound = cl.composition_ref(field.cpu().numpy(), rows.cpu().numpy(), idx, lik.rec.cpu().numpy(), lik.span.cpu().numpy(), lik.n_cond,
                                       a_1, post.chain_discharge)
        lp = lpb = None
        if with_prior:
            lp, lpb = hl.prior_ref(theta.cpu().numpy(), post._kind, post._a, post._b)
        want, wb = hl.marginal_ref(ll.reshape(K, M, lik.n_cond), bound.reshape(K, M, lik.n_cond), log_prior=lp)
        if with_prior:
            wb = wb + np.where(np.isfinite(want), lpb, 0)
            assert np.array_equal(np.isneginf(got), [False, False, True, False, True, False])      # exactly -inf outside the support
        fin = np.isfinite(want)
        print('max |err| / bound', float(np.max(np.abs(got[fin] - want[fin].astype(np.float64)) / wb[fin].astype(np.float64))))
        hl.assert_within(got, want, wb, 'log posterior' if with_prior else 'log likelihood')
    # the coordinates are the host map's, up to log10 (the device's and numpy's may round differently)
    t_h = post.map.coords(post.batch.inputs.cpu().numpy())
    assert np.abs(post.coords.cpu().numpy() - t_h).max() <= 4 * 2.0 ** -52 * 8
    lin = ~post.map.is_log
    assert np.array_equal(post.coords.cpu().numpy()[lin], t_h[lin])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_shared_nuisance_capture_and_record_predictions(fit):
    import torch
    from hallthrusterpem_amd.calibration import SurrogatePosterior
    s, lik = fit
    M = 5
    a = SurrogatePosterior(NAMES, lik, s, n_chains=4, n_nuisance=M, seed=3, fresh_nuisance=False, shared_nuisance=True)
    b = SurrogatePosterior(NAMES, lik, s, n_chains=9, n_nuisance=M, seed=3, fresh_nuisance=False, shared_nuisance=True)
    th = _thetas(9, 2)
    vb = b.log_posterior(th).clone()
    va = a.log_posterior(th[[7, 0, 3, 3]].contiguous())
    assert torch.isfinite(vb).all() and torch.equal(va, vb[[7, 0, 3, 3]])                  # neither the row nor K matters
    # capture() replays the eager evaluation bit for bit
    post = SurrogatePosterior(NAMES, lik, s, n_chains=5, n_nuisance=M, seed=1)
    replay = post.capture()
    for seed in (4, 5):
        theta = _thetas(5, seed, outside=[(1, 1, 70.0)] if seed == 5 else ())
        got = replay(theta).clone()
        fresh, post.fresh = post.fresh, False
        eager = post.log_posterior(theta)
        post.fresh = fresh
        assert torch.equal(got, eager) and torch.isfinite(got).sum() == (4 if seed == 5 else 5)
    # record_predictions is the launch's pred
    post = SurrogatePosterior(NAMES, lik, s, n_chains=3, n_nuisance=M, seed=2, fresh_nuisance=False)
    theta = _thetas(3, 6)
    got = post.record_predictions(theta)
    pred = torch.full((3 * M, lik.n_rec), float('nan'), dtype=torch.float64, device='cuda')
    ll = s.run_system_loglik(post.coords, lik, pred=pred)
    assert got.shape == (3 * M, lik.n_rec) and torch.equal(got.isnan(), pred.isnan()) and torch.equal(got.nan_to_num(), pred.nan_to_num())
    valid = ~torch.isnan(lik.rec[:, 1]) & (lik.rec[:, 2] != 0)
    assert torch.isfinite(got[:, valid]).all() and torch.isnan(got[:, ~valid]).all()
    # ... and the launch without the discharge term differs from the posterior's by that term only
    post.log_likelihood(theta)
    assert not torch.equal(ll, post.loglik) and torch.all(post.loglik < ll)


@pytest.mark.gpu
def test_optimizer_and_sampler_take_it_unchanged(fit):
    import torch
    from hallthrusterpem_amd.calibration import DRAM, SurrogatePosterior
    from hallthrusterpem_amd.optimize import DifferentialEvolution
    s, lik = fit
    de = DifferentialEvolution(None, NAMES, priors=s.priors, seed=3, tol=0.0, use_graph=True)
    de.f = SurrogatePosterior(NAMES, lik, s, n_chains=de.P, n_nuisance=4, seed=1, fresh_nuisance=False, shared_nuisance=True).log_posterior
    res = de.run(3, check_every=10)
    assert res.generations == 3 and np.isfinite(res.value) and np.all(np.isfinite(res.theta)) and np.all(np.diff(res.history) >= 0)
    K = 8
    post = SurrogatePosterior(NAMES, lik, s, n_chains=K, n_nuisance=4, seed=1, fresh_nuisance=False, shared_nuisance=True)
    sampler = DRAM(post.log_posterior, res.theta, cov0=np.diag([0.05, 1.0, 0.02, 0.02]) ** 2, n_chains=K, seed=2, adapt_after=20,
                   adapt_interval=10, device=post.device, use_graph=True)
    trace = sampler.run(50)
    torch.cuda.synchronize()
    acc = float(sampler.acceptance.sum(dim=0).mean())
    print('DE value', res.value, 'theta', res.theta, 'DRAM acceptance', acc)
    assert torch.isfinite(trace).all() and torch.isfinite(sampler.logp).all() and 0.0 < acc < 1.0
