"""optimize.Powell on the MI355X: the launch against its numpy restatement (tests/powell_np.py) bit for bit, launch by launch,
on a smooth-plus-rough function and under values with ties, NaN and -inf; the driver (optimum, repeatability, graph replay,
the two limits); scipy's own Powell calling the same device function; DE followed by Powell on a posterior with shared
nuisance draws; DE's Sobol' initial population; the example."""
import ctypes as C
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

import powell_np as pn
from test_nelder_mead import _priors, _quadratic, _theta_close

ROOT = Path(__file__).resolve().parents[1]
XTOL, FTOL = 1e-2, 1e-4                              # a loose xtol: shorter line searches, the same branches
HIST_ROWS = 50                                       # the history is shorter than the run: the rows past it are not written
MAX_LAUNCHES = 4000
EXTRA = 5                                            # launches after the condition below is met


# ------------------------------------------------------------------------------------------------------------ kernel
def _function(S, d, lb, ub, rng):
    """values of the emitted points: a coupled quadratic whose optimum lies outside the box for some searches (extrapolations
    get clipped) plus a small rough term (line searches that return a worse value); search 1 of three sees a flat function"""
    centre = lb + (ub - lb) * rng.uniform(-0.3, 1.3, (S, d))
    weight = np.logspace(0.0, 1.5, d)[rng.permutation(d)] if d > 1 else np.array([10.0])

    def f(x):
        r = x - centre
        v = -(0.5 * np.sum(weight * r * r, -1) + 2.0 * np.mean(r, -1) ** 2 + 2e-3 * np.sum(np.sin(90.0 * x + np.arange(d)), -1))
        if S == 3:
            v[1] = 1.5
        return v
    return f


def _hostile(rng, S, launch):
    """values with ties, NaN and -inf among them"""
    f = np.round(rng.normal(size=S), 1)
    f[rng.random(S) < 0.1] = np.nan
    f[rng.random(S) < 0.1] = -np.inf
    if launch % 3 == 2:
        f[:] = np.nan
    return f


def _launch(S, d, finalize, max_iter, kind, a, b, lb, ub, t):
    import torch
    from hallthrusterpem_amd import _lib
    p = lambda x: C.c_void_p(x.data_ptr())                                                  # noqa: E731
    ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                           # noqa: E731
    _lib.check(_lib.load().pem_powell_step_f64_dev(S, d, finalize, XTOL, FTOL, max_iter, pn.SQRT_EPS, pn.GOLDEN_MEAN, ptr(kind),
                                                   ptr(a), ptr(b), ptr(lb), ptr(ub), p(t['vec']), p(t['direc']), p(t['scal']),
                                                   p(t['cand_f']), p(t['theta']), p(t['state']), p(t['history']), HIST_ROWS,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _drive(S, d, source, n_launches=None, device=True):
    """Launches and two finalizes of the kernel (device) beside the restatement, everything compared after every launch.  On
    the function source the run ends EXTRA launches after every search has finished or consumed the value of an extrapolated
    point (about two iterations); the synthetic source runs as many launches (`n_launches`).  Returns the restatement's
    counters summed over the searches, the launches, and whether a finished search was seen beside a running one."""
    rng = np.random.default_rng(1000 * S + 10 * d + (source == 'function'))
    kind, a, b, lb, ub = _priors(d)
    max_iter = 6
    vec = np.zeros((S, pn.VEC_ROWS, d))
    vec[:, pn.X] = lb + (ub - lb) * rng.uniform(0.0, 1.0, (S, d))
    vec[0, pn.X, 0] = ub[0]                              # a start on the bound
    direc = np.broadcast_to(np.eye(d), (S, d, d)).copy()
    if S > 1 and d > 1:                                  # a caller's direction set, with a zero row in it
        direc[S - 1] = 0.5 * np.linalg.qr(rng.standard_normal((d, d)))[0]
        direc[S - 1, d // 2] = 0.0
    want = dict(vec=vec, direc=direc, scal=np.full((S, pn.SCALARS), 3.0), theta=np.zeros((S, d)),
                state=np.zeros((S, pn.STATE_WORDS), dtype=np.uint64), history=np.full((HIST_ROWS, S), -7.0))
    want['state'][:, 1:] = 9                             # launch 0 zeroes what it finds
    cand_f = np.zeros(S)
    f = _function(S, d, lb, ub, rng) if source == 'function' else None
    if device:
        import torch
        t = {k: torch.as_tensor(v.view(np.int64) if k == 'state' else v, device='cuda') for k, v in want.items()}
        t['cand_f'] = torch.zeros(S, dtype=torch.float64, device='cuda')
    extrapolated = np.zeros(S, dtype=bool)
    mixed, launch, stop = False, 0, n_launches
    while True:
        finalize = 0 if stop is None or launch < stop else 2 if launch == stop else 1   # ..., best_x, then x
        before = want['state'].copy()
        if device:
            _launch(S, d, finalize, max_iter, kind, a, b, lb, ub, t)
        want = pn.step(finalize, XTOL, FTOL, max_iter, kind, a, b, lb, ub, want['vec'], want['direc'], want['scal'], cand_f,
                       want['theta'], want['state'], want['history'])
        if device:
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in t.items()}
            assert np.array_equal(got['state'].view(np.uint64), want['state']), (launch, got['state'].view(np.uint64) - want['state'])
            for k in ('vec', 'direc', 'scal', 'history'):
                assert np.array_equal(got[k], want[k]), (launch, k, np.argwhere(got[k] != want[k])[:4])
            _theta_close(got['theta'], want['theta'], kind)
        pts = want['vec'][:, pn.CAND]
        assert np.all(np.isfinite(pts)) and np.all((pts >= lb) & (pts <= ub)) and np.all(np.isfinite(want['theta']))
        if finalize == 1:
            break
        status = want['state'][:, pn.STATUS]
        if not finalize:
            mixed = mixed or (status.min() == 0 and status.max() >= 1)
            extrapolated |= (before[:, pn.PHASE] == pn.PH_EXTRAP) & (before[:, pn.STATUS] == 0) & (before[:, pn.LAUNCHES] >= 1)
            if stop is None and np.all(extrapolated | (status != 0)):
                stop = launch + 1 + EXTRA
            assert launch < MAX_LAUNCHES
            cand_f = f(pts) if f is not None else _hostile(rng, S, launch)
            if device:
                t['cand_f'].copy_(torch.as_tensor(cand_f, device='cuda'))
        launch += 1
    assert np.all(want['state'][:, pn.LAUNCHES] == stop)
    running = want['state'][:, pn.STATUS] == 0
    assert np.all(want['state'][running, pn.NFEV] == stop - 1)
    if S == 3 and source == 'function':                  # the flat function: every line search returns what it started from
        assert want['state'][1, pn.STATUS] == 1 and want['state'][1, pn.NIT] == 1
    counters = want['state'][:, pn.N_LINES:pn.N_CAP + 1].astype(np.int64).sum(0)
    return dict(zip(pn.COUNTERS, counters)), stop, mixed


def _both(S, d, device):
    on_f, n, mixed = _drive(S, d, 'function', device=device)
    on_s, _, _ = _drive(S, d, 'synthetic', n_launches=n, device=device)
    total = {k: on_f[k] + on_s[k] for k in pn.COUNTERS}
    if S == 3:
        assert mixed                                      # a search had finished while another ran
    if S == 70:
        assert all(total[k] > 0 for k in pn.TABLE), total
        if d > 1:
            assert total['zero_dir'] > 0, total
    return total, n


@pytest.mark.parametrize('S', [1, 3, 70])
@pytest.mark.parametrize('d', [1, 2, 5, 17, 32])
def test_the_restatement_alone_meets_the_conditions_of_the_kernel_test(S, d):
    total, n = _both(S, d, device=False)
    print(S, d, 'launches', n, total)


@pytest.mark.gpu
@pytest.mark.parametrize('S', [1, 3, 70])
@pytest.mark.parametrize('d', [1, 2, 5, 17, 32])
def test_powell_kernel_matches_the_numpy_restatement_bit_for_bit(S, d):
    """state (all 24 words), vec (x, x1, p, xi, best_x, the emitted point), direc, the 20 scalars and history with
    np.array_equal, theta to _theta_close's tolerances, after every launch and both finalizes; the values are computed on the
    host and copied in, so that the kernel and the restatement see the same bits.  Two sources: a coupled quadratic plus a small
    rough term of the emitted point, and synthetic values rounded to one decimal with 10 % NaN, 10 % -inf and every third launch
    all NaN.  One of three searches sees a flat function and finishes after its first iteration while the others run; one start
    is on a bound; with more than one search the last has a caller's direction set with a zero row.  With S = 70 every branch
    counter of the table is non-zero."""
    _both(S, d, device=True)


# ------------------------------------------------------------------------------------------------------------- driver
FIELDS = ('theta', 'u', 'value', 'nit', 'nfev', 'converged', 'status', 'best_theta', 'best_u', 'best_value', 'direc')


def _same(x, y, history=True):
    for k in FIELDS + (('history',) if history else ()):
        assert np.array_equal(getattr(x, k), getattr(y, k)), k
    assert x.best == y.best and all(np.array_equal(x.counters[k], y.counters[k]) for k in pn.COUNTERS)


@pytest.mark.gpu
def test_powell_driver_reaches_the_optimum_repeats_itself_and_replays_as_a_graph():
    from hallthrusterpem_amd.optimize import Powell
    f, names, pri, ustar = _quadratic()
    d, S = 5, 8
    runs = {}
    for key, kw in (('eager', {}), ('again', {}), ('graph', dict(use_graph=True))):
        po = Powell(f, names, pri, n_starts=S, seed=3, **kw)
        assert po.rows == S
        runs[key] = po.run(check_every=50)
    r = runs['eager']
    _same(runs['again'], r)
    _same(runs['graph'], r)
    assert r.theta.shape == r.u.shape == r.best_theta.shape == (S, d) and r.value.shape == (S,) and r.direc.shape == (S, d, d)
    print('max|u - ustar| per start', np.abs(r.best_u - ustar).max(1), 'nit', r.nit, 'nfev', r.nfev, 'status', r.status)
    assert np.abs(r.best_u[r.best] - ustar).max() < 1e-3, r.best_u[r.best] - ustar
    assert np.abs(r.u[r.best] - ustar).max() < 1e-3, r.u[r.best] - ustar
    assert r.best == int(np.argmax(r.best_value)) and np.all(r.best_value >= r.value)
    assert np.all(r.best_value >= r.history[0])                           # every start ends no worse than its x0
    assert np.all(np.diff(r.history, axis=0) >= 0) and np.array_equal(r.history[-1], r.best_value)
    assert np.all(r.converged == (r.status == 1)) and r.converged[r.best]
    # the graph runs again from the start; the host looks more often: the same search, fewer launches after the end
    po = Powell(f, names, pri, n_starts=S, seed=3, use_graph=True)
    often = po.run(check_every=7)
    _same(often, r, history=False)
    n = often.history.shape[0]
    assert n <= r.history.shape[0] and np.array_equal(often.history, r.history[:n]) and np.all(r.history[n:] == r.best_value)
    # the two limits
    short = po.run(max_iterations=3)
    assert np.all(short.nit == 3) and np.all(short.status == 2) and not short.converged.any()
    m = int(short.nfev.min())                            # until the first search stops, the same search
    assert 0 < m < int(r.nfev.min()) and np.array_equal(short.history[:m], r.history[:m])
    few = po.run(max_evaluations=40, check_every=7)
    assert np.all(few.nfev == 40) and np.all(few.status == 3) and few.history.shape == (40, S)
    assert np.array_equal(few.history, r.history[:40])
    # theta is a point the search has had a value for, and `value` is that value (the same rows in the same places: the same
    # bits); that it is the point after the last completed line search is held to scipy's maxfev in the test below
    import torch
    assert np.array_equal(f(torch.as_tensor(few.theta, device='cuda')).cpu().numpy(), few.value)
    assert np.array_equal(f(torch.as_tensor(few.best_theta, device='cuda')).cpu().numpy(), few.best_value)
    # one start given as x0, to tighter tolerances
    one = Powell(f, names, pri, x0=r.best_theta[r.best], xtol=1e-6, ftol=1e-10).run()
    assert one.value.shape == (1,) and np.abs(one.best_u[0] - ustar).max() < 1e-4


# ------------------------------------------------------------------------------------------------------ against scipy
@pytest.mark.gpu
def test_powell_equals_scipy_calling_the_same_device_function():
    """All-uniform priors (theta = a + (b - a) u is reproduced bit for bit by numpy) and an f whose row value does not depend on
    the batch: an explicit sum column by column.  scipy's Powell on the host calls f one row at a time from the same x0 in search
    coordinates; one device search must give the same u, value, nit and nfev."""
    import torch
    from scipy.optimize import minimize
    from hallthrusterpem_amd.optimize import Powell
    from hallthrusterpem_amd.sampling import UNIFORM, Prior
    d = 4
    names = tuple(f'x{j}' for j in range(d))
    lo, hi = np.array([-1.0, 0.0, 2.0, -3.0]), np.array([1.0, 4.0, 6.0, -1.0])       # b - a a power of two: exact
    pri = {k: Prior(UNIFORM, lo[j], hi[j], 't') for j, k in enumerate(names)}
    centre = torch.as_tensor(lo + (hi - lo) * np.array([0.31, 0.77, 0.52, 0.12]), device='cuda')
    w = [1.0, 7.0, 0.4, 3.0]

    def f(theta):
        r = theta - centre
        v = w[0] * r[:, 0] * r[:, 0]
        for j in range(1, d):
            v = v + w[j] * r[:, j] * r[:, j]
        v = v + 0.8 * (r[:, 0] * r[:, 1]) + 0.3 * (r[:, 2] * r[:, 3]) * (r[:, 2] * r[:, 3])
        return -v
    po = Powell(f, names, pri, x0=lo + (hi - lo) * np.array([0.6, 0.2, 0.9, 0.5]))
    u0 = po.u0[0].cpu().numpy()                           # the start in search coordinates, as the device has it
    g = lambda u: -float(f(torch.as_tensor(pn.transform(po.kind, po.a, po.b, u[None]), device='cuda'))[0])    # noqa: E731
    for limits, opts, status in (({}, {}, (1, 0)), (dict(max_evaluations=40), dict(maxfev=40), (3, 1)),
                                 (dict(max_iterations=2), dict(maxiter=2), (2, 2))):
        got = po.run(**limits)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            want = minimize(g, u0, method='Powell', bounds=[(0.0, 1.0)] * d, options=dict(xtol=1e-4, ftol=1e-4, **opts))
        print('scipy', want.x, want.fun, want.nit, want.nfev, 'device', got.u[0], got.value[0], got.nit[0], got.nfev[0])
        assert (got.status[0], want.status) == status
        assert np.array_equal(got.u[0], want.x) and got.value[0] == -want.fun
        assert int(got.nit[0]) == want.nit and int(got.nfev[0]) == want.nfev
        assert np.array_equal(got.direc[0], want.direc)
        assert np.array_equal(got.theta[0], pn.transform(po.kind, po.a, po.b, want.x[None])[0])


# -------------------------------------------------------------------------------------------------------- a posterior
@pytest.mark.gpu
def test_powell_polishes_a_differential_evolution_map_on_synthetic_system_data():
    import torch
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.optimize import DifferentialEvolution, Powell
    from test_optimize import _synthetic
    lik, names, star = _synthetic()
    d, M = len(names), 50
    mk = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)
    de = DifferentialEvolution(None, names, seed=3, tol=1e-2, use_graph=True)
    de.f = mk(de.P).log_posterior
    res = de.run(1000, check_every=20)
    members = torch.argsort(de.pop_f, descending=True, stable=True)[:d + 1]
    po = Powell(None, names, x0=de.theta[members].cpu().numpy(), use_graph=True)
    assert po.rows == d + 1
    po.f = mk(po.rows).log_posterior
    r = po.run(max_iterations=10)
    one = mk(1)
    at = lambda th: float(one.log_posterior(torch.as_tensor(np.asarray(th)[None], device='cuda'))[0])   # noqa: E731
    print('DE', res.value, res.theta, 'Powell', r.best_value, r.best_theta[r.best], r.nit, r.nfev, r.status)
    assert r.best_value[r.best] >= r.history[0, r.best], (r.best_value, r.history[0])   # no worse than that start's own x0 row
    assert np.all(r.best_value >= r.history[0])
    assert at(r.best_theta[r.best]) == r.best_value[r.best]          # shared draws: the value does not depend on the row


# ------------------------------------------------------------------------------------------------------- small checks
@pytest.mark.gpu
def test_differential_evolution_takes_its_initial_population_from_the_sobol_design():
    from hallthrusterpem_amd.optimize import DifferentialEvolution
    from hallthrusterpem_amd.sampling import UNIFORM, Design, Prior
    f, names, pri, _ = _quadratic()
    de = DifferentialEvolution(f, names, pri, popsize=6, seed=5, init='sobol')
    unit = {k: Prior(UNIFORM, 0.0, 1.0, 'quantile') for k in names}
    want = Design(priors=unit, names=names, seed=5).sample(de.P, device='cuda', method='sobol').T
    assert np.array_equal(de.u0.cpu().numpy(), want.cpu().numpy())
    lhs = DifferentialEvolution(f, names, pri, popsize=6, seed=5)
    assert lhs.init == 'lhs' and not np.array_equal(lhs.u0.cpu().numpy(), de.u0.cpu().numpy())
    de.reset()                                            # the initial population is what the first launch evaluates
    assert np.array_equal(de.trial_u.cpu().numpy(), want.cpu().numpy())


@pytest.mark.gpu
def test_powell_search_example_runs():
    out = subprocess.run([sys.executable, str(ROOT / 'examples' / 'powell_search.py')], capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    assert 'differential evolution' in out.stdout and 'Powell' in out.stdout, out.stdout
