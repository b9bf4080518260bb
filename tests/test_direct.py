"""optimize.Direct on the MI355X: the launch against its numpy restatement (tests/direct_np.py) bit for bit, launch by launch,
with the values of both taken from one device function; the driver against scipy's own DIRECT calling that device function one
row at a time; the driver (repeatability, graph replay, the evaluation limit, a NaN value); DIRECT followed by a Nelder-Mead
polish on a posterior with shared nuisance draws; the example."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import direct_np as dn
from test_nelder_mead import _priors, _quadratic, _theta_close

ROOT = Path(__file__).resolve().parents[1]
HIST_ROWS = 20                                       # the history is shorter than the runs: the rows past it are not written


# ------------------------------------------------------------------------------------------------------------ kernel
def _device_function(d, kind, a, b, device):
    """f of the rows of theta, on the device: a weighted quadratic of every input taken back to its prior's unit scale, plus a
    coupling of the first two; smooth, so the rounds look like a posterior's, and without ties"""
    import torch
    rng = np.random.default_rng(d)
    centre = torch.as_tensor(rng.uniform(0.2, 0.8, d), device=device)
    a_, b_ = torch.as_tensor(a, device=device), torch.as_tensor(b, device=device)

    def f(theta):
        cols = []
        for j in range(d):
            t = theta[:, j]
            cols.append((t - a_[j]) / (b_[j] - a_[j]) if kind[j] == 0 else (torch.log10(t) - a_[j]) / (b_[j] - a_[j]) if kind[j] == 1
                        else torch.special.ndtr((t - a_[j]) / b_[j]))
        v = torch.zeros_like(cols[0])
        for j in range(d):
            v = v + (j + 1.0) * (cols[j] - centre[j]) ** 2
        return -(v + 0.3 * torch.sin(5.0 * cols[0] * cols[-1]) + 2.0)
    return f


def _launch(d, rows, cap, n_depth, finalize, eps, max_iter, max_fun, kind, a, b, lb, ub, t):
    import torch
    from hallthrusterpem_amd import _lib
    p = lambda x: C.c_void_p(x.data_ptr())                                                  # noqa: E731
    ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                           # noqa: E731
    _lib.check(_lib.load().pem_direct_step_f64_dev(
        d, rows, cap, n_depth, finalize, eps, 1e-16, 1e-6, max_iter, max_fun, ptr(kind), ptr(a), ptr(b), ptr(lb), ptr(ub),
        p(t['thirds']), p(t['levels']), p(t['centres']), p(t['values']), p(t['expo']), p(t['level']), p(t['queue']),
        p(t['rowinfo']), p(t['cand_f']), p(t['theta']), p(t['state']), p(t['history']), HIST_ROWS,
        C.c_void_p(torch.cuda.current_stream().cuda_stream)))


SHAPES = [(2, 4, 40), (3, 7, 40), (6, 64, 25), (17, 34, 30), (17, 64, 30)]


def _drive(d, rows, launches, eps, device):
    """`launches` launches and a finalize of the kernel (device) beside the restatement, everything compared after every
    launch; without a device the restatement runs alone on the same function evaluated by the CPU"""
    import torch
    kind, a, b, lb, ub = _priors(d)
    f = _device_function(d, kind, a, b, 'cuda' if device else 'cpu')
    cap, max_iter, max_fun = 1 + rows * launches + 4096, 1000, 10 ** 6       # (a round is stored whole or not at all)
    thirds, levels = dn.tables(d)
    n_depth = thirds.size - 1
    want = dn.new_state(d, rows, cap)
    want['state'][1:] = 9                                # launch 0 zeroes what it finds
    want['rowinfo'][:] = 5
    hist = np.full((HIST_ROWS, 3), -7.0)
    if device:
        t = {k: torch.as_tensor(v.view(np.int64) if k == 'state' else v, device='cuda') for k, v in want.items()}
        t.update(thirds=torch.as_tensor(thirds, device='cuda'), levels=torch.as_tensor(levels, device='cuda'),
                 cand_f=torch.zeros(rows, dtype=torch.float64, device='cuda'), history=torch.as_tensor(hist, device='cuda'))
    cand_f = np.zeros(rows)
    seen = dict(partial=False, several=False, padded=False, whole=False, rounds=0)
    for launch in range(launches + 1):
        finalize = int(launch == launches)
        if device:
            _launch(d, rows, cap, n_depth, finalize, eps, max_iter, max_fun, kind, a, b, lb, ub, t)
        before = want['state'].copy()
        want = dn.step(finalize, eps, 1e-16, 1e-6, max_iter, max_fun, kind, a, b, lb, ub, thirds, levels, want, cand_f, hist)
        hist = want.pop('history')
        st = want['state']
        stored = int(st[dn.NFEV])
        if device:
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in t.items()}
            assert np.array_equal(got['state'].view(np.uint64), st), (launch, got['state'], st)
            n = stored + int(st[dn.PEND])                # the stored rectangles and the ones whose centres are out
            assert np.array_equal(got['centres'][:n], want['centres'][:n]), launch
            for k in ('values', 'expo', 'level'):
                assert np.array_equal(got[k][:stored], want[k][:stored]), (launch, k)
            assert np.array_equal(got['queue'][:int(st[dn.Q_LEN])], want['queue'][:int(st[dn.Q_LEN])]), launch
            assert np.array_equal(got['rowinfo'], want['rowinfo']) and np.array_equal(got['history'], hist), launch
            _theta_close(got['theta'], want['theta'], kind)
        assert st[dn.STATUS] == 0 and st[dn.TIES] == 0
        assert np.all(np.isfinite(want['theta']))
        if finalize:
            break
        pend = int(st[dn.PEND])
        parents = len(set(want['rowinfo'][:pend, 0].tolist()))
        seen['partial'] |= bool(st[dn.Q_HEAD] < st[dn.Q_LEN])
        seen['several'] |= parents > 1
        seen['padded'] |= pend < rows
        seen['whole'] |= bool(st[dn.NIT] > before[dn.NIT] and st[dn.Q_HEAD] == st[dn.Q_LEN] and parents > 1)
        seen['rounds'] = int(st[dn.NIT])
        if device:
            values = f(t['theta'])
            t['cand_f'].copy_(values)
        else:
            values = f(torch.as_tensor(want['theta']))
        cand_f = values.cpu().numpy()
        cand_f[pend:] = np.nan                            # the values of left-over rows are ignored (the kernel has the real ones)
    print(d, rows, eps, seen, 'nfev', stored)
    assert seen['rounds'] >= 3 and seen['padded']
    if rows == 64:                                       # several rectangles, and a whole round of them, in one launch
        assert seen['several'] and seen['whole']
    elif eps < 1.0:                                      # rounds that span launches (at eps = 1 a small round can fit)
        assert seen['partial']
    assert np.all(hist[HIST_ROWS - 1] != -7.0) and int(st[dn.LAUNCHES]) == launches


@pytest.mark.parametrize('eps', [1.0, 1e-4])
@pytest.mark.parametrize('d, rows, launches', SHAPES)
def test_the_restatement_alone_meets_the_conditions_of_the_kernel_test(d, rows, launches, eps):
    _drive(d, rows, launches, eps, device=False)


@pytest.mark.gpu
@pytest.mark.parametrize('eps', [1.0, 1e-4])
@pytest.mark.parametrize('d, rows, launches', SHAPES)
def test_direct_kernel_matches_the_numpy_restatement_bit_for_bit(d, rows, launches, eps):
    """theta (to _theta_close's tolerances: the uniform columns bit for bit), and with np.array_equal the centres, values,
    exponents and levels of every stored and every emitted rectangle, the queue, rowinfo, all ten state words and the history,
    after every launch and after the finalize.  Both take the values of the emitted rows from one device function of the
    kernel's theta.  (2, 4): one or two rectangles per launch, rounds over many launches; (3, 7): a left-over row, rectangles
    of 2, 4 and 6 points that do or do not fit; (6, 64): several rectangles and whole rounds in one launch; (17, .): the
    reference's dimension.  The priors are uniform, log-uniform and normal in turn, so lb and xs2 are not all zero."""
    _drive(d, rows, launches, eps, device=True)


# ------------------------------------------------------------------------------------------------------ against scipy
def _uniform_problem():
    """all-uniform priors with widths that are powers of two (theta = a + (b - a) u is reproduced bit for bit by numpy) and an f
    whose row value does not depend on the batch: explicit sums column by column"""
    import torch
    from hallthrusterpem_amd.sampling import UNIFORM, Prior
    d = 3
    names = tuple(f'x{j}' for j in range(d))
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([1.0, 4.0, 6.0])
    pri = {k: Prior(UNIFORM, lo[j], hi[j], 't') for j, k in enumerate(names)}
    centre = torch.as_tensor(lo + (hi - lo) * np.array([0.31, 0.77, 0.52]), device='cuda')
    w = [1.0, 7.0, 0.4]

    def f(theta):
        r = theta - centre
        v = w[0] * r[:, 0] * r[:, 0]
        for j in range(1, d):
            v = v + w[j] * r[:, j] * r[:, j]
        return -(v + 0.8 * (r[:, 0] * r[:, 1]) + 0.3 * torch.sin(3.0 * r[:, 2]))
    return f, names, pri


@pytest.mark.gpu
def test_direct_equals_scipy_calling_the_same_device_function():
    """scipy's direct on the host calls f one row at a time over the unit cube; the device search with 7 rows per launch must
    evaluate the same points in the same order and end with the same x, fun, nit, nfev and status"""
    import torch
    from scipy.optimize import direct
    from hallthrusterpem_amd.optimize import Direct
    f, names, pri = _uniform_problem()
    d = len(names)
    seen = []
    di = Direct(None, names, pri, rows=7, eps=1.0)

    def recording(theta):
        seen.append(theta[:int(di.state[7].item())].cpu().numpy())       # state word 7: the rows this launch emitted
        return f(theta)
    di.f = recording
    got = di.run(max_iterations=12)
    pts = []

    def g(u):
        th = dn.transform(di.kind, di.a, di.b, np.asarray(u, dtype=np.float64)[None])
        pts.append(th[0])
        return -float(f(torch.as_tensor(th, device='cuda'))[0])
    want = direct(g, [(0.0, 1.0)] * d, eps=1.0, maxiter=12, locally_biased=False)
    mine = np.concatenate(seen)[:got.nfev]               # (launches after the end emit nothing)
    print('scipy', want.x, want.fun, want.nit, want.nfev, want.status, 'device', got.u, got.value, got.nit, got.nfev, got.status)
    assert (got.nit, got.nfev, got.status) == (want.nit, want.nfev, want.status) and want.status == 2 and want.nit == 12
    assert mine.shape == (want.nfev, d) and np.array_equal(mine, np.stack(pts))
    assert np.array_equal(got.u, want.x) and got.value == -want.fun
    assert np.array_equal(got.theta, dn.transform(di.kind, di.a, di.b, want.x[None])[0])
    assert got.history.shape == (got.launches - 1, 3) and got.history[-1, 0] == got.value and got.history[-1, 1] == got.nfev


# ------------------------------------------------------------------------------------------------------------- driver
FIELDS = ('theta', 'u', 'value', 'nit', 'nfev', 'status', 'launches', 'history')


def _same(x, y):
    for k in FIELDS:
        assert np.array_equal(getattr(x, k), getattr(y, k)), k


@pytest.mark.gpu
def test_direct_driver_repeats_itself_replays_as_a_graph_and_stops_at_its_limits():
    import torch
    from hallthrusterpem_amd.optimize import Direct
    f, names, pri, ustar = _quadratic()
    d = len(names)
    runs = {}
    for key, kw in (('eager', {}), ('again', {}), ('graph', dict(use_graph=True))):
        di = Direct(f, names, pri, eps=1e-4, **kw)
        assert di.rows == 64
        runs[key] = di.run(max_iterations=25)
    r = runs['eager']
    _same(runs['again'], r)
    _same(runs['graph'], r)
    print('u', r.u, 'ustar', ustar, 'value', r.value, 'nit', r.nit, 'nfev', r.nfev, 'launches', r.launches)
    assert r.status == 2 and r.nit == 25 and r.theta.shape == r.u.shape == (d,)
    assert np.all(np.diff(r.history[:, 0]) >= 0) and r.history[-1, 0] == r.value and np.all(np.diff(r.history[:, 1]) >= 0)
    assert r.value > r.history[0, 0]                      # above the centre's value
    assert float(f(torch.as_tensor(r.theta[None], device='cuda'))[0]) == pytest.approx(r.value, rel=1e-12)
    # the graph runs again from the start, under an evaluation limit: the same search until a whole round has passed the limit
    few = di.run(max_evaluations=150, check_every=3)
    assert few.status == 1 and few.nfev > 150 and few.nit < r.nit
    n = few.history.shape[0]
    assert np.array_equal(few.history, r.history[:n])
    # a value that is not finite ends the search and freezes it
    calls = [0]

    def poisoned(theta):
        calls[0] += 1
        v = f(theta)
        if calls[0] == 6:
            v = v.clone()
            v[1] = float('nan')
        return v
    bad = Direct(poisoned, names, pri, eps=1e-4).run(max_iterations=25, check_every=4)
    assert bad.status == 7 and bad.launches == 7 and np.array_equal(bad.history[:5], r.history[:5])
    assert bad.nfev == int(r.history[4, 1]) and bad.value == r.history[4, 0] and np.array_equal(bad.history[5], bad.history[4])
    assert calls[0] == 8                                  # launches 7 and 8 found it frozen; the host looked after the 8th


# -------------------------------------------------------------------------------------------------------- a posterior
@pytest.mark.gpu
def test_direct_then_nelder_mead_on_synthetic_system_data():
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.optimize import Direct, NelderMead
    from test_optimize import _synthetic
    lik, names, star = _synthetic()
    mk = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=50, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)
    di = Direct(None, names, rows=64, eps=1.0, use_graph=True)
    di.f = mk(di.rows).log_posterior
    r = di.run(max_iterations=20)
    nm = NelderMead(None, names, x0=r.theta, use_graph=True)
    nm.f = mk(nm.rows).log_posterior
    p = nm.run(max_iterations=60)
    print('DIRECT', r.value, r.theta, r.nit, r.nfev, r.status, 'centre', r.history[0, 0], 'Nelder-Mead', p.value, p.theta[0], 'theta*', star)
    assert r.status == 2 and r.nit == 20
    assert r.value >= r.history[0, 0]                     # the first value consumed is the box centre's
    assert p.value[p.best] >= r.value


@pytest.mark.gpu
def test_direct_search_example_runs():
    out = subprocess.run([sys.executable, str(ROOT / 'examples' / 'direct_search.py'), '30'], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    assert 'DIRECT' in out.stdout and 'Nelder-Mead' in out.stdout, out.stdout
