"""The calibration likelihood kernels over their dispatch space, sample by sample against the long-double restatement of
tests/hp_likelihood.py: the stand-alone j_ion likelihood, the fused likelihood modes of plume_r1_kernel (JMODE 3: j_ion,
6: every quantity, 7: the record predictions), the marginal over nuisance draws and the prior.

Sample counts reach two full rounds of the persistent loops plus a ragged tail (derived from the device's CU count and the
kernels' grid rules, with two workgroups per CU as the upper bound), with small tables (two workgroups per CU) and with
tables past 12 KiB (one per CU).  Tables are built through the C ABI: record counts 0..17 per sample, conditions without a
kind, several V_cc / T records per condition, padding records that must never be read (NaN), u_ion at the first and last grid
interval, j_ion at 0, at grid nodes and at pi/2.  Every table limit is run exactly at the limit and refused one past it."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import hp_likelihood as hl

NANG = 91
SENTINEL = -12345.5
UION = (0.0, 0.08, 40)
STANDALONE_ROUND = 256 * 2 * 4 * 16      # pem_jion_loglik: at most 512 workgroups of 4 waves x 16-sample tiles


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from hallthrusterpem_amd import _lib
    return _lib


def _assert_refused(call):
    """the call is refused with PEM_ERR_INVALID_ARG (not any other failure)"""
    with pytest.raises(_lib().PemHipError) as refused:
        call()
    assert refused.value.code == _lib().PEM_ERR_INVALID_ARG, str(refused.value)


def _rounds_n(tail=37):
    """a sample count past two full rounds of the fused launch at two workgroups per CU (so at one per CU as well)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _, spr = _lib().persistent_grid(1 << 30, cus, 2, memory_bound=False)
    assert spr == cus * 2 * 4 * 64
    n = 2 * spr + 64 * 5 + tail
    wg, _ = _lib().persistent_grid(n, cus, 2, memory_bound=False)
    assert wg == cus * 2 and -(-n // 64) > 2 * wg * 4, 'the launch must reach a third round'
    return n


def _angles(rng, n):
    """(k, w) of n j_ion measurement angles, JionLikelihood's rule; 0, a grid node and pi/2 first"""
    alpha = np.concatenate([[0.0, 17 * (np.pi / 2) / 90, np.pi / 2], rng.uniform(0, np.pi / 2, max(n - 3, 0))])[:n]
    pos = np.minimum(alpha / ((np.pi / 2) / 90.0), 90.0)
    k = np.minimum(np.floor(pos).astype(np.int32), 89)
    return k, pos - k


# ---- the stand-alone kernel -------------------------------------------------------------------------------------------------
def _profiles(rng, n):
    """synthetic profiles: twelve decades, negative values, constant rows"""
    p = rng.choice([-1.0, 1.0], (n, NANG), p=[0.2, 0.8]) * 10.0 ** rng.uniform(-6, 6, (n, NANG))
    p[::7] = rng.uniform(-3, 3, (len(p[::7]), 1))
    return p


def _standalone(n, n_cond, n_ang, seed, misaligned=False):
    import torch
    rng = np.random.default_rng(seed)
    k, w = np.zeros((n_cond, n_ang), np.int32), np.zeros((n_cond, n_ang))
    for c in range(n_cond):
        k[c], w[c] = _angles(rng, n_ang)
    y = rng.choice([-1.0, 1.0], (n_cond, n_ang)) * 10.0 ** rng.uniform(-3, 3, (n_cond, n_ang))
    inv_std = 10.0 ** rng.uniform(-2, 1, (n_cond, n_ang))
    prof = _profiles(rng, n)
    buf = torch.empty(n * NANG + 1, dtype=torch.float64, device='cuda')
    j = buf[1:] if misaligned else buf[:-1]
    j.copy_(torch.from_numpy(prof.ravel()))
    assert (j.data_ptr() % 16 == 8) == misaligned
    tabs = [torch.as_tensor(np.ascontiguousarray(a), device='cuda') for a in (k, w, y, inv_std)]   # alive until the launch is done
    out = torch.full((n,), np.nan, dtype=torch.float64, device='cuda')
    rc = _lib().load().pem_jion_loglik_f64_dev(n, n_cond, n_ang, *map(_p, tabs), _p(j), _p(out), _stream())
    assert rc == 0, _lib().load().pem_last_error()
    cond = np.arange(n) % n_cond
    want, bound = hl.profile_sum(prof, k[cond], w[cond], y[cond], inv_std[cond])
    hl.assert_within(out.cpu().numpy(), want, bound, f'pem_jion_loglik n={n} n_cond={n_cond} n_ang={n_ang}')


@pytest.mark.gpu
def test_standalone_sample_counts_and_angle_counts():
    for n in (1, 15, 16, 17, 63, 64, 65, 1000 * 16 + 9):
        _standalone(n, 3, 9, seed=n)
    for n_ang in range(1, 10):
        for n_cond in (1, 7):
            _standalone(64 * 5 + 3, n_cond, n_ang, seed=100 + n_ang)
    for n_cond in (63, 65, 127):
        _standalone(1000, n_cond, 5, seed=n_cond)


@pytest.mark.gpu
def test_standalone_three_rounds_and_unaligned_profiles():
    """past the two-tile prefetch of the persistent loop (512 workgroups), vector and scalar loads"""
    n = 3 * STANDALONE_ROUND + 16 * 7 + 5
    _standalone(n, 5, 7, seed=1)
    _standalone(n, 5, 7, seed=1, misaligned=True)
    _standalone(64 * 9 + 3, 3, 9, seed=2, misaligned=True)


@pytest.mark.gpu
def test_standalone_at_and_past_the_table_limit():
    import torch
    lim = _lib().load().pem_jion_loglik_f64_dev
    _standalone(2000, 64, 64, seed=3)                              # PEM_LOGLIK_MAX_MEASUREMENTS = 4096
    _standalone(300, 1, 4096, seed=4)
    _standalone(4096 + 64 + 5, 4096, 1, seed=5)
    big = torch.zeros(4097 * 2, dtype=torch.float64, device='cuda')
    ki = torch.zeros(4097, dtype=torch.int32, device='cuda')
    j = torch.zeros(NANG, dtype=torch.float64, device='cuda')
    for n_cond, n_ang in ((1, 4097), (4097, 1), (65, 64)):
        assert lim(1, n_cond, n_ang, _p(ki), _p(big), _p(big), _p(big), _p(j), _p(big), _stream()) == _lib().PEM_ERR_INVALID_ARG


# ---- the fused modes ----------------------------------------------------------------------------------------------------------
def _batch(n, seed):
    from hallthrusterpem_amd.batch import CoupledBatch
    from hallthrusterpem_amd.sampling import Design
    b = CoupledBatch(n, profile=True, thruster_qoi=True)
    Design(seed=seed).fill(b.inputs)
    b.run()
    return b


def _jmode3(b, n_cond, n_ang, seed):
    import torch
    rng = np.random.default_rng(seed)
    k, w = np.zeros((n_cond, n_ang), np.int32), np.zeros((n_cond, n_ang))
    for c in range(n_cond):
        k[c], w[c] = _angles(rng, n_ang)
    y = rng.lognormal(0.0, 1.0, (n_cond, n_ang))
    inv_std = rng.uniform(0.3, 3.0, (n_cond, n_ang))
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device='cuda')   # noqa: E731
    lk = SimpleNamespace(n_cond=n_cond, n_ang=n_ang, kidx=dev(k), weight=dev(w), y=dev(y), inv_std=dev(inv_std))
    out = torch.full((b.n,), np.nan, dtype=torch.float64, device='cuda')
    b.run_loglik(lk, out=out)
    cond = torch.arange(b.n, device='cuda') % n_cond
    kk = lk.kidx.long()[cond]
    lo = torch.gather(b.j_ion, 1, kk).cpu().numpy()
    hi = torch.gather(b.j_ion, 1, kk + 1).cpu().numpy()
    c = cond.cpu().numpy()
    m = hl.interp_model(w[c], lo, hi)
    want, bound = hl.record_sum(m, y[c], inv_std[c])
    hl.assert_within(out.cpu().numpy(), want, bound, f'JMODE 3 n={b.n} n_cond={n_cond} n_ang={n_ang}')


@pytest.mark.gpu
def test_jmode3_record_counts_sample_counts_and_conditions():
    for n in (1, 63, 64, 65, 64 * 7 + 29):
        b = _batch(n, seed=n)
        _jmode3(b, 3, 11, seed=n)
    b = _batch(64 * 9 + 5, seed=7)
    for n_ang in range(1, 18):
        _jmode3(b, 5, n_ang, seed=n_ang)
    for n_cond in (1, 7, 63, 65, 127):
        _jmode3(b, n_cond, 3, seed=n_cond)


@pytest.mark.gpu
def test_jmode3_two_rounds_small_and_large_table():
    b = _batch(_rounds_n(), seed=11)
    _jmode3(b, 7, 9, seed=1)          # 7 x 9 x 32 B: two workgroups per CU
    _jmode3(b, 63, 7, seed=2)         # 63 x 7 x 32 B = 14 KiB: one per CU


@pytest.mark.gpu
def test_jmode3_at_and_past_the_table_limit():
    import torch
    b = _batch(64 * 20 + 3, seed=5)
    _jmode3(b, 1024, 1, seed=1)       # 1024 x (1 | 1) = PEM_FUSED_LOGLIK_MAX_MEASUREMENTS
    _jmode3(b, 32, 31, seed=2)        # 32 x 31 = 992
    _jmode3(b, 1, 1023, seed=3)
    z = torch.zeros(4096, dtype=torch.float64, device='cuda')
    zi = torch.zeros(4096, dtype=torch.int32, device='cuda')
    for n_cond, n_ang in ((32, 32), (1, 1024), (1025, 1), (512, 2)):    # even n_ang: (n_ang | 1) crosses the limit
        lk = SimpleNamespace(n_cond=n_cond, n_ang=n_ang, kidx=zi, weight=z, y=z, inv_std=z)
        _assert_refused(lambda: b.run_loglik(lk, out=z[:b.n]))


def _table(rng, n_cond, ncells=UION[2], counts=None, big=False):
    """a JMODE 6 / 7 table through the C ABI: per condition j_ion 0..17 records, V_cc and T 0..3, u_ion 0..4, in a shuffled
    kind order, NaN padding between conditions; u_ion node pairs cover the first and the last grid interval"""
    import torch
    blocks, span, first = [], np.zeros((n_cond, 4, 2), np.int32), 0
    node = [0, 1, ncells - 2, ncells - 1]
    for c in range(n_cond):
        nj, nv, nt, nu = counts(c) if counts else (c % 18, c % 4, (c // 4) % 4, (c // 2) % 5)
        order = rng.permutation(4)
        for kind in order:
            cnt = (nj, nv, nt, nu)[kind]
            r = np.zeros((cnt, 4))
            if kind == 0:
                k, w = _angles(rng, cnt)
                r[:, 0], r[:, 1], r[:, 2] = w, rng.lognormal(0, 1, cnt), rng.uniform(0.3, 3, cnt)
                r[:, 3] = k.astype(np.int64).view(np.float64)
            elif kind == 3:
                p = np.array([0, 2] + list(2 * rng.integers(0, len(node) // 2, max(cnt - 2, 0))), np.int64)[:cnt]
                if len(node) < min(4 * n_cond, 64):
                    g = int(rng.integers(0, ncells - 1))
                    node += [g, g + 1]
                r[:, 0] = rng.choice([0.0, 1.0, 0.5, 0.123], cnt)
                r[:, 1], r[:, 2], r[:, 3] = rng.uniform(1e3, 2e4, cnt), rng.uniform(1e-4, 1e-3, cnt), p.view(np.float64)
            else:
                r[:, 1], r[:, 2] = (rng.uniform(15, 35, cnt), rng.uniform(0.3, 2, cnt)) if kind == 1 else \
                    (rng.uniform(0.05, 0.12, cnt), rng.uniform(30, 300, cnt))
            span[c, kind] = (first, cnt)
            blocks.append(r)
            first += cnt
        pad = 1 + (c % 2) if not big else 0
        blocks.append(np.full((pad, 4), np.nan))
        first += pad
    rec = np.concatenate(blocks) if blocks else np.zeros((0, 4))
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device='cuda')   # noqa: E731
    nodes = np.asarray(node, np.int32)
    return SimpleNamespace(sweep_radius=1.0, uion_grid=(UION[0], UION[1], ncells), n_cond=n_cond, n_rec=rec.shape[0],
                           rec=dev(rec), span=dev(span), n_node=nodes.size, node=dev(nodes), np_rec=rec, np_span=span, np_node=nodes)


def _predict_ref(b, tab, ld):
    """JMODE 7's (rows, ld) predictions restated from what pem_coupled_f64_dev stores for the same inputs: j_ion records
    fma(w, j[k+1] - j[k], j[k]) of the stored profile, V_cc and T its scalars, u_ion records fma(w, u1 - u0, u0) of the nodes
    of pem_thruster_uion_f64_dev at the v_exh of pem_thruster_f64_dev -- bit for bit"""
    import torch
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    n = b.n
    x = b.inputs
    v_exh = torch.empty(n, dtype=torch.float64, device='cuda')
    lib = _lib().load()
    col = lambda k: _p(x[COUPLED_INPUTS.index(k)])                # noqa: E731
    assert lib.pem_thruster_f64_dev(n, col('V_a'), _p(b.qoi[0]), col('mdot_a'), col('a_1'), *[None] * 7, _p(v_exh), _stream()) == 0
    z0, z1, ncells = tab.uion_grid
    uion = torch.empty((n, ncells), dtype=torch.float64, device='cuda')
    assert lib.pem_thruster_uion_f64_dev(n, _p(v_exh), z0, z1, ncells, None, _p(uion), _stream()) == 0
    rows = -(-n // tab.n_cond)
    want = np.full((rows, ld), SENTINEL)
    V_cc, T = b.qoi[0].cpu().numpy(), b.T.cpu().numpy()
    rec, span, node = tab.np_rec, tab.np_span, tab.np_node
    for c in range(tab.n_cond):
        idx = np.arange(c, n, tab.n_cond)
        if idx.size == 0:
            continue
        d = idx // tab.n_cond
        it = torch.as_tensor(idx, device='cuda')
        f, cnt = span[c, 0]
        if cnt:
            r = rec[f:f + cnt]
            k = torch.as_tensor(r[:, 3].view(np.int64), device='cuda')
            lo = b.j_ion[it][:, k].cpu().numpy()
            hi = b.j_ion[it][:, k + 1].cpu().numpy()
            want[d[:, None], np.arange(f, f + cnt)] = hl.interp_model(r[:, 0], lo, hi)
        for kind, v in ((1, V_cc), (2, T)):
            f, cnt = span[c, kind]
            want[d[:, None], np.arange(f, f + cnt)] = v[idx][:, None]
        f, cnt = span[c, 3]
        if cnt:
            r = rec[f:f + cnt]
            p = r[:, 3].view(np.int64)
            u = uion[it]
            u0 = u[:, torch.as_tensor(node[p].astype(np.int64), device='cuda')].cpu().numpy()
            u1 = u[:, torch.as_tensor(node[p + 1].astype(np.int64), device='cuda')].cpu().numpy()
            want[d[:, None], np.arange(f, f + cnt)] = hl.interp_model(r[:, 0], u0, u1)
    return want


def _system(b, tab, extra_ld=0, check_predict=True):
    """JMODE 7 bit for bit against _predict_ref, then JMODE 6 against the long-double sum over JMODE 7's values"""
    import torch
    rows = -(-b.n // tab.n_cond)
    ld = tab.n_rec + extra_ld
    pred = torch.full((rows, ld), SENTINEL, dtype=torch.float64, device='cuda')
    b.run_system_predict(tab, pred)
    got = pred.cpu().numpy()
    what = f'n={b.n} n_cond={tab.n_cond} n_rec={tab.n_rec}'
    if check_predict:
        want = _predict_ref(b, tab, ld)
        bad = got.view(np.int64) != want.view(np.int64)
        if bad.any():
            i = np.argwhere(bad)[0]
            raise AssertionError(f'JMODE 7 {what}: {int(bad.sum())} predictions differ; first at {tuple(i)}: got {got[tuple(i)]!r} '
                                 f'want {want[tuple(i)]!r}')
    ll = torch.full((b.n,), np.nan, dtype=torch.float64, device='cuda')
    b.run_system_loglik(tab, out=ll)
    ll = ll.cpu().numpy()
    rec, span = tab.np_rec, tab.np_span
    want, bound = np.zeros(b.n, dtype=hl.LD), np.zeros(b.n, dtype=hl.LD)
    for c in range(tab.n_cond):
        idx = np.arange(c, b.n, tab.n_cond)
        r = np.concatenate([np.arange(span[c, kd, 0], span[c, kd, 0] + span[c, kd, 1]) for kd in range(4)]).astype(np.int64)
        if idx.size == 0 or r.size == 0:
            continue
        m = got[(idx // tab.n_cond)[:, None], r[None, :]]
        want[idx], bound[idx] = hl.record_sum(m, rec[r, 1], rec[r, 2])
    hl.assert_within(ll, want, bound, f'JMODE 6 {what}')
    return got


@pytest.mark.gpu
def test_system_modes_record_counts_and_conditions():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 64 * 6 + 17):
        _system(_batch(n, seed=n), _table(rng, 36))
    b = _batch(64 * 40 + 11, seed=3)
    for n_cond in (1, 7, 63, 65, 127):
        _system(b, _table(rng, n_cond) if n_cond < 63 else _table(rng, n_cond, counts=lambda c: (c % 6, c % 2, c % 3 // 2, c % 5 // 4)))
    # one kind per condition, kinds missing everywhere else; replicate V_cc and T records
    _system(b, _table(rng, 9, counts=lambda c: [(0, 3, 0, 0), (0, 0, 2, 0), (5, 0, 0, 0), (0, 0, 0, 3), (0, 0, 0, 0),
                                               (17, 2, 3, 4), (1, 1, 1, 1), (8, 0, 0, 0), (16, 3, 3, 0)][c]))
    got = _system(b, _table(rng, 5), extra_ld=5)                  # ld_pred > n_rec: the padding columns keep the sentinel
    assert np.all(got[:, -5:] == SENTINEL)


@pytest.mark.gpu
def test_system_modes_two_rounds_small_and_large_table():
    rng = np.random.default_rng(1)
    b = _batch(_rounds_n(tail=45), seed=21)
    small = _table(rng, 7, counts=lambda c: (c + 3, c % 2, 1, c % 3))
    assert 69696 + small.n_rec * 32 + 7 * 32 + max(small.n_node, 2) * 8 <= 160 * 1024 // 2
    _system(b, small)
    large = _table(rng, 127, counts=lambda c: (c % 18 // 3, 1, c % 2, 1 if c % 5 == 0 else 0))
    assert 69696 + large.n_rec * 32 + 127 * 32 + max(large.n_node, 2) * 8 > 160 * 1024 // 2
    _system(b, large)


@pytest.mark.gpu
def test_system_modes_at_and_past_the_table_limits():
    """PEM_FUSED_SYSTEM_MAX_RECORDS conditions and records, 2048 u_ion nodes (151 616 B of LDS); one more of each refused"""
    import torch
    rng = np.random.default_rng(2)
    b = _batch(64 * 33 + 5, seed=9)
    tab = _table(rng, 1024, counts=lambda c: [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)][c % 4], big=True)
    assert tab.n_rec == 1024
    node = np.concatenate([tab.np_node, np.tile([5, 6], (2048 - tab.np_node.size) // 2)]).astype(np.int32)
    tab.np_node, tab.node, tab.n_node = node, torch.as_tensor(node, device='cuda'), node.size
    assert tab.n_node == 2048
    _system(b, tab)
    for field, v in (('n_cond', 1025), ('n_rec', 1025), ('n_node', 2049)):
        bad = SimpleNamespace(**vars(tab))
        setattr(bad, field, v)
        bad.rec = torch.zeros((1025, 4), dtype=torch.float64, device='cuda')
        bad.span = torch.zeros((1025, 4, 2), dtype=torch.int32, device='cuda')
        bad.node = torch.zeros(2049, dtype=torch.int32, device='cuda')
        out = torch.empty(b.n, dtype=torch.float64, device='cuda')
        _assert_refused(lambda: b.run_system_loglik(bad, out=out))
        _assert_refused(lambda: b.run_system_predict(bad, torch.empty((b.n, 1025), dtype=torch.float64, device='cuda')))


@pytest.mark.gpu
def test_system_posterior_log_likelihood_past_two_rounds():
    """SystemPosterior.log_likelihood on the reference-shaped 16-condition table, K M n_cond past two rounds, against the
    long-double marginal of the JMODE 7 records of the same inputs"""
    import torch
    from test_predictive import _reference_shaped
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    lik = SystemLikelihood(_reference_shaped(0))
    assert lik.n_cond == 16
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
        ll[idx], llb[idx] = hl.record_sum(pred[idx // 16][:, r], rec[r, 1], rec[r, 2])
    x = post.batch.inputs.cpu().numpy()
    md, a1 = (x[COUPLED_INPUTS.index(k)].reshape(K, M, 16) for k in ('mdot_a', 'a_1'))
    want, bound = hl.marginal_ref(ll.reshape(K, M, 16), llb.reshape(K, M, 16), md, a1, *post.discharge)
    hl.assert_within(got, want, bound, 'SystemPosterior.log_likelihood')


# ---- marginal -----------------------------------------------------------------------------------------------------------------
def _marginal(ll, mdot_a=None, a_1=None, discharge=(4.5, 0.2), log_prior=None, what=''):
    import torch
    K, M, E = ll.shape
    dev = [torch.as_tensor(np.ascontiguousarray(a), device='cuda') if a is not None else None for a in (ll, mdot_a, a_1, log_prior)]
    out = torch.full((K,), 7.0, dtype=torch.float64, device='cuda')
    rc = _lib().load().pem_loglik_marginal_f64_dev(K, M, E, _p(dev[0]), _p(dev[1]), _p(dev[2]), discharge[0], discharge[1], _p(dev[3]),
                                                   _p(out), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    want, bound = hl.marginal_ref(ll, None, mdot_a, a_1, discharge[0], discharge[1], log_prior)
    hl.assert_within(out.cpu().numpy(), want, bound, f'marginal {what} K={K} M={M} E={E}')


@pytest.mark.gpu
def test_marginal_draws_conditions_discharge_and_prior():
    rng = np.random.default_rng(3)
    for M in (1, 63, 64, 256, 257, 1000):
        for E in range(1, 21):
            K = 5
            ll = -rng.exponential(30.0, (K, M, E)) * rng.choice([0.1, 1.0, 10.0], (K, 1, 1))   # sums over hundreds of units
            md, a1 = rng.uniform(2e-6, 7e-6, (K, M, E)), 10.0 ** rng.uniform(-2.5, -1, (K, M, E))
            lp = rng.uniform(-30, 5, K)
            _marginal(ll, what='plain')
            _marginal(ll, md, a1, what='discharge')
            _marginal(ll, md, a1, log_prior=lp, what='discharge + prior')
            _marginal(ll, log_prior=lp, what='prior')


@pytest.mark.gpu
def test_marginal_non_finite_rows():
    rng = np.random.default_rng(4)
    K, M, E = 6, 257, 3
    ll = -rng.exponential(5.0, (K, M, E))
    ll[0] = -np.inf                        # all -inf
    ll[1, 100, 1] = np.nan                 # one NaN
    ll[2, :200] = -np.inf                  # some -inf
    ll[3, 256, 2] = np.nan                 # NaN in the last draw, alone in its lane's second push
    lp = np.array([0.0, 1.0, -np.inf, 2.0, np.nan, -3.0])
    _marginal(ll, what='non-finite')
    _marginal(ll, log_prior=lp, what='non-finite + prior')
    md, a1 = rng.uniform(2e-6, 7e-6, (K, M, E)), 10.0 ** rng.uniform(-2.5, -1, (K, M, E))
    _marginal(ll, md, a1, log_prior=lp, what='non-finite + discharge + prior')


# ---- prior --------------------------------------------------------------------------------------------------------------------
def _prior(theta, kind, a, b, what=''):
    import torch
    from hallthrusterpem_amd.calibration import log_prior
    from hallthrusterpem_amd.sampling import Prior
    n, ndim = theta.shape
    out = torch.full((n,), 7.0, dtype=torch.float64, device='cuda')
    arr = lambda v, t: np.ascontiguousarray(v, dtype=t)          # noqa: E731
    ki, aa, bb = arr(kind, np.int32), arr(a, np.float64), arr(b, np.float64)
    # the log-uniform supports as the host rounds them (BatchedPosterior passes the same)
    lo = arr([10.0 ** a[d] if kind[d] == hl.LOGUNIFORM else a[d] for d in range(ndim)], np.float64)
    hi = arr([10.0 ** b[d] if kind[d] == hl.LOGUNIFORM else b[d] for d in range(ndim)], np.float64)
    th = torch.as_tensor(np.ascontiguousarray(theta), device='cuda')
    rc = _lib().load().pem_log_prior_f64_dev(n, ndim, *(C.c_void_p(v.ctypes.data) for v in (ki, aa, bb, lo, hi)), _p(th), _p(out),
                                             _stream())
    assert rc == 0
    got = out.cpu().numpy()
    names = [f'd{i}' for i in range(ndim)]
    host = log_prior(theta, names, {nm: Prior(int(kind[i]), float(a[i]), float(b[i]), '') for i, nm in enumerate(names)})
    assert np.array_equal(np.isneginf(got), np.isneginf(host)), \
        f'{what}: support differs from calibration.log_prior at {np.argwhere(np.isneginf(got) != np.isneginf(host)).ravel()[:8]}'
    want, bound = hl.prior_ref(theta, kind, a, b)
    hl.assert_within(got, want, bound, f'prior {what}')


def _edges(x):
    """x and its two neighbouring doubles"""
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


@pytest.mark.gpu
def test_prior_every_kind_and_dimension_count():
    rng = np.random.default_rng(5)
    for ndim in range(1, 33):
        kind = rng.integers(0, 3, ndim)
        a = np.where(kind == 2, rng.uniform(-5, 5, ndim), rng.uniform(-3, 1, ndim))
        b = np.where(kind == 2, rng.uniform(0.1, 3, ndim), a + rng.uniform(0.5, 4, ndim))
        n = 300 + ndim
        th = np.empty((n, ndim))
        for d in range(ndim):
            if kind[d] == 0:
                th[:, d] = rng.uniform(a[d] - 0.3, b[d] + 0.3, n)
            elif kind[d] == 1:
                th[:, d] = 10.0 ** rng.uniform(a[d] - 0.1, b[d] + 0.1, n)
            else:
                th[:, d] = rng.normal(a[d], 2 * b[d], n)
        inside = np.clip(th[: n // 2], np.where(kind == 1, 10.0 ** a, a), np.where(kind == 1, 10.0 ** b, b))
        th[: n // 2] = np.where(kind == 2, th[: n // 2], inside)      # half the rows inside every support
        _prior(th, kind, a, b, f'ndim={ndim}')


@pytest.mark.gpu
def test_prior_support_edges_of_the_pem_v0_and_sobol_priors():
    """theta at a, b, 10.0 ** a, 10.0 ** b and their neighbouring doubles: the support decision equals calibration.log_prior's"""
    from hallthrusterpem_amd import sobol
    from hallthrusterpem_amd.sampling import PEM_V0_PRIORS
    tables = [dict(PEM_V0_PRIORS)] + [sobol.sweep_priors(pb, g) for pb in sobol.DEFAULT_PRESSURES for g in sobol.GROUPS]
    for pri in tables:
        for name, p in pri.items():
            if p.kind == 2 or p.a == p.b:          # (pinned inputs are drawn, never given a density)
                continue
            lo, hi = (10.0 ** p.a, 10.0 ** p.b) if p.kind == 1 else (p.a, p.b)
            pts = _edges(lo) + _edges(hi) + _edges(p.a) + _edges(p.b) + [0.5 * (lo + hi)]
            th = np.asarray(pts, dtype=np.float64)[:, None]
            _prior(th, [p.kind], [p.a], [p.b], f'{name} edges')


@pytest.mark.gpu
def test_batched_posterior_prior_support_equals_log_prior_at_the_edges():
    """BatchedPosterior.log_prior, which hands the kernel its own edges, against calibration.log_prior at the log-uniform
    edges and their neighbouring doubles (c4 given P_b's prior, whose edges the device's pow(10, a) rounds otherwise)"""
    import torch
    from hallthrusterpem_amd.calibration import JionPosterior, log_prior
    from hallthrusterpem_amd.sampling import PEM_V0_PRIORS
    priors = dict(PEM_V0_PRIORS, c4=PEM_V0_PRIORS['P_b'])
    names = ('a_1', 'c4', 'c5', 'T_e')
    lo = np.array([10.0 ** priors[k].a if priors[k].kind == hl.LOGUNIFORM else priors[k].a for k in names])
    hi = np.array([10.0 ** priors[k].b if priors[k].kind == hl.LOGUNIFORM else priors[k].b for k in names])
    rows = []
    for d in range(len(names)):
        for v in _edges(lo[d]) + _edges(hi[d]):
            r = 0.5 * (lo + hi)
            r[d] = v
            rows.append(r)
    theta = np.asarray(rows)
    op = np.array([[1e-5, 300.0, 5e-6]])
    alpha = np.array([[0.0, 0.4, 1.0]])
    post = JionPosterior(names, op, alpha, np.ones((1, 3)), np.ones((1, 3)), n_chains=len(rows), n_nuisance=1, priors=priors,
                         fresh_nuisance=False)
    got = post.log_prior(torch.as_tensor(theta, device=post.device)).cpu().numpy()
    host = log_prior(theta, names, priors)
    assert np.array_equal(np.isneginf(got), np.isneginf(host)), np.argwhere(np.isneginf(got) != np.isneginf(host)).ravel()
    assert np.isneginf(got).sum() == 2 * len(names)                  # exactly the two outer neighbours of each dimension
    want, bound = hl.prior_ref(theta, [priors[k].kind for k in names], [priors[k].a for k in names], [priors[k].b for k in names])
    hl.assert_within(got, want, bound, 'BatchedPosterior.log_prior at the edges')
