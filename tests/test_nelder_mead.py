"""optimize.NelderMead on the MI355X: the launch against its numpy restatement (tests/nm_np.py) bit for bit, launch by launch,
with ties, NaN and -inf among the values; the driver (optimum, repeatability, graph replay, counters, maxiter); DE followed by
Nelder-Mead on a posterior with shared nuisance draws; the example."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import nm_np
from hallthrusterpem_amd.sampling import LOGUNIFORM, NORMAL, UNIFORM, Prior

ROOT = Path(__file__).resolve().parents[1]
XATOL = FATOL = 1e-4
N_LAUNCHES, HIST_ROWS = 40, 30                       # the history is shorter than the run: the rows past it are not written


# ------------------------------------------------------------------------------------------------------------ kernel
def _theta_close(got, want, kind):
    """the sampler tests' tolerances: uniform bit for bit, log-uniform to 4e-15 relative, normal to 1e-12 absolute"""
    for j, k in enumerate(kind):
        if k == UNIFORM:
            assert np.array_equal(got[:, j], want[:, j]), j
        elif k == LOGUNIFORM:
            assert np.max(np.abs(got[:, j] / want[:, j] - 1)) < 4e-15, j
        else:
            assert np.max(np.abs(got[:, j] - want[:, j])) < 1e-12, j


def _priors(d):
    kinds = np.array([UNIFORM, LOGUNIFORM, NORMAL], dtype=np.int32)
    kind = np.ascontiguousarray(kinds[np.arange(d) % 3])
    a = np.where(kind == UNIFORM, -2.0, np.where(kind == LOGUNIFORM, 14.0, 30.0)) + np.arange(d)
    b = np.where(kind == UNIFORM, 3.0, np.where(kind == LOGUNIFORM, 18.0, 2.0)) + np.where(kind == NORMAL, 0.0, np.arange(d))
    lb = np.where(kind == NORMAL, 0.0013498980316300957, 0.0)
    ub = np.where(kind == NORMAL, 0.9986501019683699, 1.0)
    return kind, np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(lb), np.ascontiguousarray(ub)


def _start(rng, S, d, lb, ub, frozen):
    sim = np.stack([nm_np.initial_simplex(lb + (ub - lb) * rng.uniform(0.05, 0.99, d), lb, ub) for _ in range(S)])
    sim[0, 0, 0] = ub[0]                               # a vertex on the bound
    if frozen is not None:
        sim[frozen] = sim[frozen, 0]                   # all vertices equal: equal values, converged at the first test
    return sim


def _rough(x):
    """the rough function of the host test (minimised: f is its negative), row by row"""
    return -(np.sum(np.abs(x - 0.37), -1) + np.sum(np.sin(1000.0 * x) * np.cos(1700.0 * x[..., ::-1]), -1))


def _synthetic_values(rng, S, nc, launch):
    """values with ties, NaN and -inf among them"""
    f = np.round(rng.normal(size=(S, nc)), 1)          # few distinct values: many ties
    f[rng.random((S, nc)) < 0.1] = np.nan
    f[rng.random((S, nc)) < 0.1] = -np.inf
    if launch % 3 == 2:
        f[:] = np.nan                                   # nothing can be taken: a shrink onto +inf
    return f


def _launch(S, d, finalize, coef, kind, a, b, lb, ub, t):
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    p = lambda x: C.c_void_p(x.data_ptr())                                                  # noqa: E731
    ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                           # noqa: E731
    _lib.check(_lib.load().pem_nm_step_f64_dev(S, d, finalize, float(coef[0]), coef[1], coef[2], coef[3], XATOL, FATOL, ptr(kind),
                                               ptr(a), ptr(b), ptr(lb), ptr(ub), p(t['sim']), p(t['fsim']), p(t['cand_x']),
                                               p(t['cand_f']), p(t['theta']), p(t['state']), p(t['history']), HIST_ROWS,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _drive(S, d, source, device=True):
    """N_LAUNCHES launches and a finalize of the kernel (device) beside the restatement, everything compared after every
    launch.  Returns the restatement's operation counts and whether a frozen simplex was seen beside a running one."""
    rng = np.random.default_rng(1000 * S + 10 * d + (source == 'rough'))
    kind, a, b, lb, ub = _priors(d)
    coef = nm_np.coefficients(d, adaptive=(d % 2 == 1))           # both sets of coefficients over the d's
    frozen = 1 if S == 3 else None
    nc = d + 4
    want = dict(sim=_start(rng, S, d, lb, ub, frozen), fsim=np.zeros((S, d + 1)), cand_x=np.zeros((S, nc, d)),
                theta=np.zeros((S * nc, d)), state=np.zeros((S, 10), dtype=np.uint64), history=np.full((HIST_ROWS, S), -7.0))
    cand_f = np.zeros((S, nc))
    if device:
        import torch
        t = {k: torch.as_tensor(v.view(np.int64) if k == 'state' else v, device='cuda') for k, v in want.items()}
        t['cand_f'] = torch.zeros(S, nc, dtype=torch.float64, device='cuda')
    mixed = False
    for launch in range(N_LAUNCHES + 1):
        finalize = launch == N_LAUNCHES
        if device:
            _launch(S, d, int(finalize), coef, kind, a, b, lb, ub, t)
        want = nm_np.step(finalize, coef, XATOL, FATOL, kind, a, b, lb, ub, want['sim'], want['fsim'], want['cand_x'], cand_f,
                          want['theta'], want['state'], want['history'])
        if device:
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in t.items()}
            assert np.array_equal(got['state'].view(np.uint64), want['state']), (launch, got['state'], want['state'])
            assert np.array_equal(got['sim'], want['sim']), launch
            assert np.array_equal(got['fsim'], want['fsim'], equal_nan=True), launch
            assert np.array_equal(got['cand_x'], want['cand_x']), launch
            assert np.array_equal(got['history'], want['history']), launch
            _theta_close(got['theta'], want['theta'], kind)
        assert not np.isnan(want['fsim']).any()                    # a NaN value is stored as -inf
        status = want['state'][:, nm_np.STATUS]
        mixed = mixed or (status.min() == 0 and status.max() == 1)
        cand_f = _rough(want['cand_x']) if source == 'rough' else _synthetic_values(rng, S, nc, launch)
        if device:
            t['cand_f'].copy_(torch.as_tensor(cand_f, device='cuda'))
    assert np.all(want['state'][:, nm_np.LAUNCHES] == N_LAUNCHES)
    if frozen is not None and source == 'rough':
        assert want['state'][frozen, nm_np.STATUS] == 1 and want['state'][frozen, nm_np.NIT] == 1
    return want['state'][:, nm_np.N_REFLECT:nm_np.N_SHRINK + 1].astype(np.int64).sum(0), mixed


@pytest.mark.gpu
@pytest.mark.parametrize('S', [1, 3, 70])
@pytest.mark.parametrize('d', [1, 2, 5, 17, 32])
def test_nm_kernel_matches_the_numpy_restatement_bit_for_bit(S, d):
    """state (all ten words), sim, fsim, cand_x and history with np.array_equal, theta to _theta_close's tolerances, after every
    one of 40 launches and a finalize; the values are computed on the host and copied in, so that the kernel and the
    restatement see the same bits.  Two sources: the rough function of cand_x, and synthetic values rounded to one decimal
    with 10 % NaN, 10 % -inf and every third launch all NaN (many ties: the stable sort).  The restatement's counters must
    show all five operations in every case with S = 70; with 1 or 3 simplices an expansion (a reflection better than the best
    vertex, and an expansion better still) is too rare in 40 launches to demand, so there only a shrink is."""
    ops_rough, mixed = _drive(S, d, 'rough')
    ops_synth, _ = _drive(S, d, 'synthetic')
    ops = ops_rough + ops_synth
    if S == 3:
        assert mixed                                    # a simplex was frozen while another ran
    if S == 70:
        assert np.all(ops > 0), ops                     # all five operations were taken (an expansion is rare on these values:
    else:                                               # a few simplices may not meet one in 40 launches)
        assert ops.sum() > 0 and ops[4] > 0, ops


# ------------------------------------------------------------------------------------------------------------- driver
def _quadratic():
    """_quadratic() of tests/test_optimize.py: a correlated Gaussian in u over a uniform, a log-uniform and a normal prior (and
    two more uniforms)"""
    import torch
    names = ('T_e', 'c4', 'V_vac', 'c0', 'c3')
    pri = {'T_e': Prior(UNIFORM, 1.0, 5.0, 't'), 'c4': Prior(LOGUNIFORM, 18.0, 22.0, 't'), 'V_vac': Prior(NORMAL, 30.0, 2.0, 't'),
           'c0': Prior(UNIFORM, 0.0, 1.0, 't'), 'c3': Prior(UNIFORM, 0.2, 1.570796, 't')}
    ustar = np.array([0.3, 0.62, 0.45, 0.8, 0.15])
    rng = np.random.default_rng(0)
    Q = np.linalg.qr(rng.standard_normal((5, 5)))[0]
    A = torch.as_tensor(Q @ np.diag([1.0, 3.0, 10.0, 30.0, 100.0]) @ Q.T, device='cuda')
    us = torch.as_tensor(ustar, device='cuda')

    def f(theta):
        u = torch.stack([(theta[:, 0] - 1.0) / 4.0, (torch.log10(theta[:, 1]) - 18.0) / 4.0,
                         torch.special.ndtr((theta[:, 2] - 30.0) / 2.0), theta[:, 3], (theta[:, 4] - 0.2) / (1.570796 - 0.2)], 1)
        dd = u - us
        return -0.5 * torch.einsum('ki,ij,kj->k', dd, A, dd)
    return f, names, pri, ustar


def _same(x, y, history=True):
    for k in ('theta', 'u', 'value', 'nit', 'nfev', 'converged', 'operations') + (('history',) if history else ()):
        assert np.array_equal(getattr(x, k), getattr(y, k)), k
    assert x.best == y.best
    assert np.array_equal(x.final_simplex[0], y.final_simplex[0]) and np.array_equal(x.final_simplex[1], y.final_simplex[1])


@pytest.mark.gpu
def test_nm_driver_reaches_the_optimum_repeats_itself_and_replays_as_a_graph():
    from hallthrusterpem_amd.optimize import NelderMead
    f, names, pri, ustar = _quadratic()
    d, S = 5, 8
    runs = {}
    for key, kw in (('eager', {}), ('again', {}), ('graph', dict(use_graph=True))):
        nm = NelderMead(f, names, pri, n_starts=S, seed=3, **kw)
        assert nm.rows == S * (d + 4)
        runs[key] = nm.run(check_every=25)
    r = runs['eager']
    _same(runs['again'], r)
    _same(runs['graph'], r)
    assert r.theta.shape == r.u.shape == (S, d) and r.value.shape == (S,) and r.operations.shape == (S, 5)
    print('max|u - ustar| per start', np.abs(r.u - ustar).max(1), 'nit', r.nit, 'nfev', r.nfev)
    assert np.abs(r.u[r.best] - ustar).max() < 1e-3, r.u[r.best] - ustar
    assert r.best == int(np.argmax(r.value)) and r.converged[r.best]
    assert np.all(np.diff(r.history, axis=0) >= 0)                        # no simplex's best value ever gets worse
    assert np.array_equal(r.history[-1], r.value) and np.array_equal(r.final_simplex[1][:, 0], r.value)
    assert np.array_equal(r.final_simplex[0][:, 0], r.u)
    assert np.all(r.nfev <= (d + 1) + (d + 2) * (r.nit - 1)) and np.all(r.nfev >= (d + 1) + (r.nit - 1))
    assert np.array_equal(r.operations.sum(1), r.nit - 1)
    # the graph runs again from the start; maxiter
    nm = NelderMead(f, names, pri, n_starts=S, seed=3, use_graph=True)
    often = nm.run(check_every=7)                     # the host looks more often: the same search, fewer launches after it froze
    _same(often, r, history=False)
    n = often.history.shape[0]
    assert n <= r.history.shape[0] and np.array_equal(often.history, r.history[:n]) and np.all(r.history[n:] == r.value)
    short = nm.run(max_iterations=7)
    assert np.all(short.nit == 7) and not short.converged.any() and short.history.shape == (7, S)
    assert np.array_equal(short.history, r.history[:7])
    # one start given as x0, to tighter tolerances
    one = NelderMead(f, names, pri, x0=r.theta[r.best], xatol=1e-6, fatol=1e-8).run()
    assert one.value.shape == (1,) and np.abs(one.u[0] - ustar).max() < 1e-4


# -------------------------------------------------------------------------------------------------------- a posterior
@pytest.mark.gpu
def test_nelder_mead_polishes_a_differential_evolution_map_on_synthetic_system_data():
    import torch
    from hallthrusterpem_amd.calibration import SystemPosterior
    from hallthrusterpem_amd.optimize import DifferentialEvolution, NelderMead
    from test_optimize import _synthetic
    lik, names, star = _synthetic()
    d, M = len(names), 50
    mk = lambda K: SystemPosterior(names, lik, n_chains=K, n_nuisance=M, seed=1, fresh_nuisance=False,  # noqa: E731
                                   shared_nuisance=True)
    de = DifferentialEvolution(None, names, seed=3, tol=1e-2, use_graph=True)
    de.f = mk(de.P).log_posterior
    res = de.run(1000, check_every=20)
    members = torch.argsort(de.pop_f, descending=True, stable=True)[:d + 1]
    assert int(members[0]) == int(np.argmax(de.pop_f.cpu().numpy())) and float(de.pop_f[members[0]]) == res.value
    nm = NelderMead(None, names, initial_simplex=de.theta[members].cpu().numpy(), use_graph=True)
    assert nm.rows == d + 4
    nm.f = mk(nm.rows).log_posterior
    r = nm.run()
    one = mk(1)
    at = lambda th: float(one.log_posterior(torch.as_tensor(np.asarray(th)[None], device='cuda'))[0])   # noqa: E731
    print('DE', res.value, res.theta, 'NM', r.value, r.theta, r.nit, r.nfev, r.converged)
    # the simplex starts at DE's best members (through `quantile`, so to the round trip's rounding, not bit for bit) and the
    # search improves on them: DE stopped at tol 1e-2, a few hundredths of log posterior short
    assert r.value[r.best] >= res.value, (r.value, res.value)
    assert at(r.theta[r.best]) == r.value[r.best]                     # shared draws: the value does not depend on the row


@pytest.mark.gpu
def test_map_polish_example_runs():
    out = subprocess.run([sys.executable, str(ROOT / 'examples' / 'map_polish.py')], capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    assert 'differential evolution' in out.stdout and 'Nelder-Mead' in out.stdout and 'Laplace' in out.stdout, out.stdout
