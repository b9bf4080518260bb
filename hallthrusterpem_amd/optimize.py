"""Where to start the chains, and with what proposal: maximum a posteriori search, Laplace covariance and 1-D slices.

Restates the steps of scripts/pem_v0/mcmc.py that come before `run_mcmc`:

    run_mle(optimizer='evolution')   mcmc.py:170-231   `DifferentialEvolution`: scipy's differential_evolution (best1bin /
                                                       rand1bin, dithered F, CR 0.7, deferred updating) with the whole
                                                       population evaluated as the rows of ONE posterior launch
    run_mle(optimizer='nelder-mead') mcmc.py:170-231   `NelderMead`: scipy's bounded, adaptive Nelder-Mead (the default) for S
                                                       simplices at once; the d + 4 points an iteration can ask for are the
                                                       rows of ONE posterior launch, csrc/pem_nm.hip takes the decisions
    run_mle(optimizer='powell')      mcmc.py:170-231   `Powell`: scipy's bounded Powell for S searches at once; a line search wants
                                                       one value at a time, so one launch of csrc/pem_powell.hip advances every
                                                       search by one value and the S points are the rows of ONE posterior launch
    run_mle(optimizer='direct')      mcmc.py:170-231   `Direct`: scipy's DIRECT without local bias, pinned through the points it
                                                       evaluates; its rectangles live on the device and the 2 |I| points of every
                                                       rectangle a round divides are rows of ONE posterior launch (csrc/pem_direct.hip)
    run_laplace / show_laplace       mcmc.py:234-265  `hessian` (central differences, 2 d^2 + 1 points in one call) and
                                                       `Laplace` (cov = pinv(-H), nearest positive-definite fall-back, draws)
    pdf_slice                        mcmc.py:132-148   `slices`: log prior, likelihood and posterior along every axis

The search runs over the prior's quantile cube u in (0, 1)^d (theta = the prior transform of u, `pem::transform` of
csrc/pem_philox.h): log-uniform inputs mutate in log space, normals need no bounds.  One generation is one launch of
`pem_de_step_f64_dev` (csrc/pem_de.hip: selection, best member, convergence statistic and the next trials) followed by the
caller's `f`; with `use_graph` the two are one hipGraph replay.  `f` is what an optimizer compares across rows, so a
`JionPosterior` / `SystemPosterior` passed here is built with `shared_nuisance=True` (the same nuisance draws in every row).
"""
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._device_loop import RecordedLoop, zeros_on
from ._marshal import current_stream_ptr, np_ptr, t_ptr
from .sampling import LOGUNIFORM, NORMAL, PEM_V0_PRIORS, UNIFORM, Design, Prior

STRATEGIES = {'best1bin': _lib.DE_BEST1BIN, 'rand1bin': _lib.DE_RAND1BIN}


def _table(names, priors):
    priors = PEM_V0_PRIORS if priors is None else priors
    for k in names:
        if k not in priors:
            raise KeyError(f"no prior for '{k}'")
    pr = [priors[k] for k in names]
    return (np.ascontiguousarray([p.kind for p in pr], dtype=np.int32), np.ascontiguousarray([p.a for p in pr], dtype=np.float64),
            np.ascontiguousarray([p.b for p in pr], dtype=np.float64))


def support(prior: Prior):
    """(lo, hi) of a prior's support; a normal's is taken as mean +- 3 standard deviations"""
    if prior.kind == UNIFORM:
        return prior.a, prior.b
    if prior.kind == LOGUNIFORM:
        return 10.0 ** prior.a, 10.0 ** prior.b
    return prior.a - 3.0 * prior.b, prior.a + 3.0 * prior.b


class _Search(RecordedLoop):
    """What the searches share around their launch.  A subclass has `history` (one row per launch, grown here), `reset()` and
    its `_body`: one launch and f on the points it emitted."""

    def _record_key(self):
        return (self.history.data_ptr(), self.history.shape[0])

    def _record(self):
        self.reset()                       # a search starts over around a recording, where a sampler snapshots its state
        super()._record()

    def _prepare(self, n_launches: int):
        """history room for n_launches (the graph is recorded again when the buffer moves), then back to the start"""
        import torch
        if self.history.shape[0] < n_launches:
            self.history = torch.full((n_launches,) + tuple(self.history.shape[1:]), math.nan, dtype=torch.float64,
                                      device=self.device)
        super()._prepare()
        self.reset()

    def _search(self, n, check_every: int, first_check: int, finished):
        """Launch until the host, reading `finished()` after first_check launches and every check_every from there, sees the
        end, or n launches have run (None: no limit).  Returns (launches run, whether `finished()` ended them)."""
        c, check, check_every = 0, int(first_check), int(check_every)
        while n is None or c < n:
            m = check - c if n is None else min(check, n) - c
            self.advance(m)
            c += m
            if c == check:
                if finished():
                    return c, True
                check += check_every
        return c, False


@dataclass
class DEResult:
    theta: np.ndarray        # (d,) the best member
    u: np.ndarray            # (d,) its quantiles
    value: float             # f there
    generations: int         # generations evaluated after the initial population
    converged: bool          # std(f) <= atol + tol |mean(f)| was met
    history: np.ndarray      # (generations + 1,) best value of the initial population and of every generation


class DifferentialEvolution(_Search):
    """scipy's `differential_evolution(f, bounds, strategy, popsize=15, mutation=(0.5, 1), recombination=0.7, tol=0.01,
    updating='deferred', vectorized=True)` (mcmc.py:214-216), MAXIMISING f, on the device.

    f: callable (P, d) float64 device tensor -> (P,) values, P = popsize * d (`.P`), like `DRAM`'s `log_posterior`:
       `post.log_posterior` or `post.log_likelihood` of a posterior with n_chains = P and shared_nuisance=True.
    names, priors: the searched inputs and their priors (the search is over their quantiles).
    mutation: F, or (lo, hi) for F ~ U(lo, hi) drawn once per generation.  seed: the Philox key of every draw.
    The initial population is a Latin hypercube of u (`Design.fill(method='lhs')` over U(0, 1)), as scipy's default init.
    init: 'lhs' (that default) or 'sobol': the population is `Design.sample(P, method='sobol')` over U(0, 1), the project's
       shifted Sobol' points.  The reference calls differential_evolution(..., init='sobol'); scipy's own scrambling of the
       sequence is not reproduced, so the points differ from scipy's.
    use_graph: a generation (the DE launch and f's launches) is one hipGraph replay on one stream."""

    def __init__(self, f, names, priors=None, popsize: int = 15, mutation=(0.5, 1.0), recombination: float = 0.7,
                 strategy: str = 'best1bin', tol: float = 0.01, atol: float = 0.0, seed: int = 0, use_graph: bool = False,
                 device=None, init: str = 'lhs'):
        if init not in ('lhs', 'sobol'):
            raise ValueError(f"unknown init '{init}' (one of 'lhs', 'sobol')")
        self.init = init
        self.names = tuple(names)
        self.d = len(self.names)
        if len(set(self.names)) != self.d or self.d < 1:
            raise ValueError('names must be distinct and non-empty')
        if self.d > _lib.DE_MAX_DIM:
            raise ValueError(f'at most {_lib.DE_MAX_DIM} searched inputs (got {self.d})')
        self.P = int(popsize) * self.d
        if not 4 <= self.P <= _lib.DE_MAX_POP:
            raise ValueError(f'population popsize * d = {self.P} must be in [4, {_lib.DE_MAX_POP}]')
        if strategy not in STRATEGIES:
            raise ValueError(f"unknown strategy '{strategy}' (one of {sorted(STRATEGIES)})")
        lo, hi = (float(mutation), float(mutation)) if np.ndim(mutation) == 0 else (float(mutation[0]), float(mutation[1]))
        if not 0.0 <= lo <= hi <= 2.0:
            raise ValueError('mutation must be in [0, 2], a dither (lo, hi) with lo <= hi')
        if not 0.0 <= recombination <= 1.0:
            raise ValueError('recombination must be in [0, 1]')
        self.kind, self.a, self.b = _table(self.names, priors)
        self.f, self.strategy, self.mutation, self.cr = f, STRATEGIES[strategy], (lo, hi), float(recombination)
        self.tol, self.atol, self.seed = float(tol), float(atol), int(seed)

        import torch
        self._init_loop(device, use_graph)
        z = zeros_on(self.device)
        self.pop_u, self.trial_u, self.theta = z(self.P, self.d), z(self.P, self.d), z(self.P, self.d)
        self.pop_f, self.trial_f = z(self.P), z(self.P)
        self.state, self.record = z(1, dt=torch.int64), z(3)
        unit = {k: Prior(UNIFORM, 0.0, 1.0, 'quantile') for k in self.names}
        self.u0 = Design(priors=unit, names=self.names, seed=self.seed).sample(
            self.P, device=self.device, method=self.init).T.contiguous()
        self.history = z(0)

    def _launch(self, finalize: bool):
        import torch
        p, ptr = t_ptr, np_ptr
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_de_step_f64_dev(
                self.P, self.d, self.strategy, 1 if finalize else 0, self.seed, self.mutation[0], self.mutation[1], self.cr,
                self.tol, self.atol, ptr(self.kind), ptr(self.a), ptr(self.b), p(self.pop_u), p(self.pop_f), p(self.trial_u),
                p(self.trial_f), p(self.theta), p(self.state), p(self.record), p(self.history) if self.history.numel() else None,
                self.history.numel(), current_stream_ptr(self.device)))

    def _generation(self):
        self._launch(False)
        self.trial_f.copy_(self.f(self.theta))

    _body = _generation

    def reset(self):
        """Back to the initial population (the next launch evaluates it)."""
        self.state.zero_()
        self.trial_u.copy_(self.u0)

    def run(self, max_generations: int = 1000, check_every: int = 10) -> DEResult:
        """Evaluate the initial population and at most `max_generations` generations after it; every `check_every`
        generations the host reads the 3-double convergence record and stops once std(f) <= atol + tol |mean(f)|."""
        import torch
        if max_generations < 0 or check_every < 1:
            raise ValueError('max_generations >= 0 and check_every >= 1')
        self._prepare(int(max_generations) + 1)
        c, converged = self._search(int(max_generations) + 1, check_every, check_every + 1,
                                    lambda: self.record[2].item() == 1.0)
        self._launch(True)                     # selection of the last trials; theta = the population's
        rec = self.record.cpu().numpy()
        best = int(rec[1])
        torch.cuda.synchronize(self.device)
        return DEResult(theta=self.theta[best].cpu().numpy(), u=self.pop_u[best].cpu().numpy(), value=float(rec[0]),
                        generations=c - 1, converged=converged or bool(rec[2] == 1.0),
                        history=self.history[:c].cpu().numpy())


# -------------------------------------------------------------------------------------------------------- Nelder-Mead
def search_bounds(names, priors=None):
    """(lb, ub) of the search coordinates: the unit interval for a uniform or log-uniform prior, Phi(-+3) for a normal one
    (the quantiles of `support`)"""
    kind, _, _ = _table(names, priors)
    lo, hi = 0.5 * math.erfc(3.0 / math.sqrt(2.0)), 0.5 * math.erfc(-3.0 / math.sqrt(2.0))
    return (np.ascontiguousarray(np.where(kind == NORMAL, lo, 0.0)), np.ascontiguousarray(np.where(kind == NORMAL, hi, 1.0)))


def quantile(theta, names, priors=None):
    """The host inverse of the prior transform, theta (..., d) -> u: (theta - a) / (b - a) uniform, (log10 theta - a) / (b - a)
    log-uniform, Phi((theta - a) / b) normal."""
    kind, a, b = _table(tuple(names), priors)
    t = np.asarray(theta, dtype=np.float64)
    if t.ndim < 1 or t.shape[-1] != kind.size:
        raise ValueError(f'theta must have one entry per name ({kind.size}) along its last axis')
    u = np.empty_like(t)
    erfc = np.vectorize(math.erfc, otypes=[np.float64])
    for j, k in enumerate(kind):
        if k == UNIFORM:
            u[..., j] = (t[..., j] - a[j]) / (b[j] - a[j])
        elif k == LOGUNIFORM:
            u[..., j] = (np.log10(t[..., j]) - a[j]) / (b[j] - a[j])
        else:
            u[..., j] = 0.5 * erfc(-((t[..., j] - a[j]) / b[j]) / math.sqrt(2.0))
    return u


def nm_coefficients(d: int, adaptive: bool = True):
    """(rho, chi, psi, sigma) as scipy's `_minimize_neldermead` writes them"""
    if adaptive:
        dim = float(d)
        return 1.0, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim
    return 1.0, 2.0, 0.5, 0.5


def nm_simplex(x0, lb, ub, sim=None):
    """scipy's initial simplex in search coordinates, (..., d + 1, d): x0 clipped into [lb, ub]; vertex k + 1 is x0 with
    component k multiplied by 1.05, or set to 0.00025 where it is zero.  Then, for a caller's `sim` as well, entries above ub
    are reflected into the interior (2 ub - x) and everything is clipped."""
    if sim is None:
        x0 = np.clip(np.asarray(x0, dtype=np.float64), lb, ub)
        d = x0.shape[-1]
        sim = np.repeat(x0[..., None, :], d + 1, axis=-2)
        for k in range(d):
            y = x0[..., k]
            sim[..., k + 1, k] = np.where(y != 0, (1 + 0.05) * y, 0.00025)
    sim = np.asarray(sim, dtype=np.float64)
    sim = np.where(sim > ub, 2 * ub - sim, sim)
    return np.ascontiguousarray(np.clip(sim, lb, ub))


@dataclass
class NMResult:
    theta: np.ndarray        # (S, d) the best vertex of every simplex
    u: np.ndarray            # (S, d) in search coordinates
    value: np.ndarray        # (S,) f there
    nit: np.ndarray          # (S,) scipy's nit: 1 + the iterations taken
    nfev: np.ndarray         # (S,) the function values the sequential form would have spent
    converged: np.ndarray    # (S,) bool: the simplex met xatol and fatol
    operations: np.ndarray   # (S, 5) reflections, expansions, outside contractions, inside contractions, shrinks
    best: int                # the simplex of the largest value (ties to the lowest index)
    history: np.ndarray      # (launches, S) the best value of every simplex after each launch
    final_simplex: tuple     # (sim (S, d + 1, d), fsim (S, d + 1)) in search coordinates, best vertex first


class NelderMead(_Search):
    """scipy's `minimize(method='Nelder-Mead', bounds=..., options={'adaptive': True, 'xatol': ..., 'fatol': ...})`
    (run_mle's default optimizer, mcmc.py:170-231), MAXIMISING f, for S independent simplices on the device.

    Every point an iteration can ask for -- the reflection, the expansion, both contractions and the d shrunk vertices -- is a
    row of ONE call of f; `pem_nm_step_f64_dev` (csrc/pem_nm.hip, a workgroup per simplex) then takes scipy's decisions from
    the values and emits the next d + 4 points.  The search runs in the prior's quantile cube, bounded by `search_bounds`.

    f: callable (S (d + 4), d) float64 device tensor -> as many values (`.rows` of them), like `DifferentialEvolution`'s:
       `post.log_posterior` of a posterior built with n_chains = nm.rows, shared_nuisance=True and fresh_nuisance=False (f is
       compared across rows and across launches, so it must be a function of theta alone).
    Exactly one of (all in theta): x0 (d,) or (S, d), from which scipy's initial simplex is built in search coordinates;
    initial_simplex (d + 1, d) or (S, d + 1, d), e.g. the best d + 1 members of a DE population; n_starts Latin-hypercube points
    of the quantile cube (the `Design` call that makes DE's initial population, keyed by `seed`).  With none, n_starts = 8:
    a bounded simplex can be clipped flat onto a face of the box and stall there, which is what `NMResult.best` is for.
    use_graph: an iteration (the launch and f's launches) is one hipGraph replay on one stream."""

    def __init__(self, f, names, priors=None, x0=None, n_starts=None, initial_simplex=None, adaptive: bool = True,
                 xatol: float = 1e-4, fatol: float = 1e-4, seed: int = 0, use_graph: bool = False, device=None):
        self.names = tuple(names)
        self.d = d = len(self.names)
        if len(set(self.names)) != d or d < 1:
            raise ValueError('names must be distinct and non-empty')
        if d > _lib.NM_MAX_DIM:
            raise ValueError(f'at most {_lib.NM_MAX_DIM} searched inputs (got {d})')
        if sum(v is not None for v in (x0, n_starts, initial_simplex)) > 1:
            raise ValueError('give at most one of x0, n_starts and initial_simplex')
        if not (xatol >= 0.0 and fatol >= 0.0):
            raise ValueError('xatol and fatol must be >= 0')
        self.kind, self.a, self.b = _table(self.names, priors)
        self.lb, self.ub = search_bounds(self.names, priors)
        self._starts = None
        if x0 is not None:
            x0 = np.asarray(x0, dtype=np.float64)
            if x0.shape != (d,) and (x0.ndim != 2 or x0.shape[1] != d or x0.shape[0] < 1):
                raise ValueError(f'x0 must have the shape ({d},) or (S, {d})')
            with np.errstate(invalid='ignore', divide='ignore'):
                q = quantile(x0.reshape(-1, d), self.names, priors)
            if not np.isfinite(q).all():
                raise ValueError('x0 has no finite quantile under the priors (a NaN, or a value <= 0 under a log-uniform prior)')
            sim0 = nm_simplex(q, self.lb, self.ub)
        elif initial_simplex is not None:
            sim = np.asarray(initial_simplex, dtype=np.float64)
            if sim.shape != (d + 1, d) and (sim.ndim != 3 or sim.shape[1:] != (d + 1, d) or sim.shape[0] < 1):
                raise ValueError(f'initial_simplex must have the shape ({d + 1}, {d}) or (S, {d + 1}, {d})')
            with np.errstate(invalid='ignore', divide='ignore'):
                q = quantile(sim.reshape(-1, d + 1, d), self.names, priors)
            if not np.isfinite(q).all():
                raise ValueError('initial_simplex has no finite quantile under the priors (a NaN, or a value <= 0 under a '
                                 'log-uniform prior)')
            sim0 = nm_simplex(None, self.lb, self.ub, q)
        else:
            self._starts = 8 if n_starts is None else int(n_starts)
            if self._starts < 1:
                raise ValueError('n_starts must be >= 1')
            sim0 = None
        self.S = self._starts if sim0 is None else sim0.shape[0]
        self.rows = self.S * (d + 4)
        self.f, self.coef, self.adaptive = f, nm_coefficients(d, adaptive), bool(adaptive)
        self.xatol, self.fatol, self.seed = float(xatol), float(fatol), int(seed)

        import torch
        self._init_loop(device, use_graph)
        if sim0 is None:
            unit = {k: Prior(UNIFORM, 0.0, 1.0, 'quantile') for k in self.names}
            u0 = Design(priors=unit, names=self.names, seed=self.seed).sample(self.S, device=self.device, method='lhs').T
            sim0 = nm_simplex(u0.cpu().numpy(), self.lb, self.ub)
        z = zeros_on(self.device)
        self.sim0 = torch.as_tensor(sim0, device=self.device)
        self.sim, self.fsim = z(self.S, d + 1, d), z(self.S, d + 1)
        self.cand_x, self.cand_f, self.theta = z(self.S, d + 4, d), z(self.rows), z(self.rows, d)
        self.state = z(self.S, _lib.NM_STATE_WORDS, dt=torch.int64)
        self.history = z(0, self.S)

    def _launch(self, finalize: bool):
        import torch
        p, ptr = t_ptr, np_ptr
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_nm_step_f64_dev(
                self.S, self.d, 1 if finalize else 0, *self.coef, self.xatol, self.fatol, ptr(self.kind), ptr(self.a),
                ptr(self.b), ptr(self.lb), ptr(self.ub), p(self.sim), p(self.fsim), p(self.cand_x), p(self.cand_f), p(self.theta),
                p(self.state), p(self.history) if self.history.numel() else None, self.history.shape[0],
                current_stream_ptr(self.device)))

    def _iteration(self):
        self._launch(False)
        self.cand_f.copy_(self.f(self.theta))

    _body = _iteration

    def reset(self):
        """Back to the initial simplices (the next launch emits their vertices)."""
        self.state.zero_()
        self.sim.copy_(self.sim0)

    def run(self, max_iterations=None, check_every: int = 10) -> NMResult:
        """Iterate until every simplex has converged (the host reads `state` every `check_every` launches) or scipy's `nit`
        reaches `max_iterations` (default 200 d, scipy's maxiter): a simplex that does not converge ends with
        nit == max_iterations.  scipy's maxfev, which can abort in the middle of an iteration, is not reproduced: `nfev` is
        reported.  `converged` is the test on the simplex the search ends with."""
        import torch
        m = 200 * self.d if max_iterations is None else int(max_iterations)
        if m < 1 or check_every < 1:
            raise ValueError('max_iterations >= 1 and check_every >= 1')
        self._prepare(m)
        c, _ = self._search(m, check_every, check_every + 1, lambda: bool((self.state[:, 3] == 1).all().item()))
        self._launch(True)                    # the last values are resolved; theta = every simplex's best vertex
        torch.cuda.synchronize(self.device)
        st = self.state.cpu().numpy()
        sim, fsim = self.sim.cpu().numpy(), self.fsim.cpu().numpy()
        value = fsim[:, 0].copy()
        return NMResult(theta=self.theta.view(self.S, self.d + 4, self.d)[:, 0].cpu().numpy(), u=sim[:, 0].copy(), value=value,
                        nit=st[:, 1].copy(), nfev=st[:, 2].copy(), converged=st[:, 3] == 1, operations=st[:, 4:9].copy(),
                        best=int(np.argmax(value)), history=self.history[:c].cpu().numpy(), final_simplex=(sim, fsim))


# ------------------------------------------------------------------------------------------------------------- Powell
POWELL_COUNTERS = ('lines', 'golden', 'parabolic', 'rejected', 'off_end', 'tol1', 'clipped', 'extra', 'replaced', 'worse',
                   'zero_dir', 'zero_disp', 'degenerate', 'one_eval', 'cap')     # state words 8 ... 22 of pem_powell_step_f64_dev
POWELL_STATUS = {0: 'running', 1: 'ftol met', 2: 'max_iterations reached', 3: 'max_evaluations reached'}


@dataclass
class PowellResult:
    theta: np.ndarray        # (S, d) scipy's x: the point after the last completed line search of every search
    u: np.ndarray            # (S, d) in search coordinates
    value: np.ndarray        # (S,) f there (scipy's -fun); Powell's own value can go down, see best_value
    nit: np.ndarray          # (S,) completed iterations (scipy's nit)
    nfev: np.ndarray         # (S,) values consumed (scipy's nfev)
    converged: np.ndarray    # (S,) bool: the ftol test was met
    status: np.ndarray       # (S,) 1 the ftol test met, 2 max_iterations reached, 3 stopped by max_evaluations
    best_theta: np.ndarray   # (S, d) the best point a search has had a value for
    best_u: np.ndarray       # (S, d)
    best_value: np.ndarray   # (S,) f there
    direc: np.ndarray        # (S, d, d) the direction sets the searches end with, in search coordinates
    counters: dict           # name (POWELL_COUNTERS) -> (S,) how often every branch of the algorithm was taken
    best: int                # the search of the largest best_value (ties to the lowest index)
    history: np.ndarray      # (launches, S) best_value after every consumed value


class Powell(_Search):
    """scipy's `minimize(method='Powell', bounds=..., options={'xtol': ..., 'ftol': ...})` (run_mle(optimizer='powell'),
    mcmc.py:170-231), MAXIMISING f, for S independent searches on the device.

    Powell's line searches want one function value at a time.  One launch of `pem_powell_step_f64_dev` (csrc/pem_powell.hip, a
    workgroup per search) takes the value of the point a search emitted last, advances scipy's algorithm -- the bounded
    golden-section / parabolic line search, the direction loop, the extrapolated point, the direction replacement -- until
    the next value is needed and emits that point; the S points are the rows of ONE call of f.  The search runs in the prior's
    quantile cube, bounded by `search_bounds`; every point, the result, nit and nfev are scipy 1.15's bit for bit wherever
    scipy is defined (include/pem_hip.h says where it is not).

    f: callable (S, d) float64 device tensor -> S values (`.rows == S`), like `NelderMead`'s: `post.log_posterior` of a posterior
       built with n_chains = powell.rows, shared_nuisance=True and fresh_nuisance=False.
    At most one of: x0 (d,) or (S, d) in theta, taken to search coordinates by `quantile` and clipped into the bounds; n_starts
    Latin-hypercube points of the quantile cube (the `Design` call that makes DE's initial population, keyed by `seed`).  With
    neither, n_starts = 8.
    direc: the initial direction set in search coordinates, (d, d) or (S, d, d), one direction per row; the identity if None.
    use_graph: a step (the launch, f's launches and the copy of the values) is one hipGraph replay on one stream."""

    def __init__(self, f, names, priors=None, x0=None, n_starts=None, direc=None, xtol: float = 1e-4, ftol: float = 1e-4,
                 seed: int = 0, use_graph: bool = False, device=None):
        self.names = tuple(names)
        self.d = d = len(self.names)
        if len(set(self.names)) != d or d < 1:
            raise ValueError('names must be distinct and non-empty')
        if d > _lib.POWELL_MAX_DIM:
            raise ValueError(f'at most {_lib.POWELL_MAX_DIM} searched inputs (got {d})')
        if x0 is not None and n_starts is not None:
            raise ValueError('give at most one of x0 and n_starts')
        if not (xtol >= 0.0 and ftol >= 0.0):
            raise ValueError('xtol and ftol must be >= 0')
        self.kind, self.a, self.b = _table(self.names, priors)
        self.lb, self.ub = search_bounds(self.names, priors)
        u0 = None
        if x0 is not None:
            x0 = np.asarray(x0, dtype=np.float64)
            if x0.shape != (d,) and (x0.ndim != 2 or x0.shape[1] != d or x0.shape[0] < 1):
                raise ValueError(f'x0 must have the shape ({d},) or (S, {d})')
            with np.errstate(invalid='ignore', divide='ignore'):
                u0 = quantile(x0.reshape(-1, d), self.names, priors)
            if not np.isfinite(u0).all():
                raise ValueError('x0 has no finite quantile under the priors (a NaN, or a value <= 0 under a log-uniform prior)')
            u0 = np.clip(u0, self.lb, self.ub)
            self.S = u0.shape[0]
        else:
            self.S = 8 if n_starts is None else int(n_starts)
            if self.S < 1:
                raise ValueError('n_starts must be >= 1')
        if direc is None:
            direc0 = np.broadcast_to(np.eye(d), (self.S, d, d))
        else:
            direc0 = np.asarray(direc, dtype=np.float64)
            if direc0.shape != (d, d) and direc0.shape != (self.S, d, d):
                raise ValueError(f'direc must have the shape ({d}, {d}) or (S, {d}, {d})')
            if not np.isfinite(direc0).all():
                raise ValueError('direc must be finite')
            direc0 = np.broadcast_to(direc0, (self.S, d, d))
        self.rows = self.S
        self.f, self.xtol, self.ftol, self.seed = f, float(xtol), float(ftol), int(seed)
        self._max_iter = 0

        import torch
        self._init_loop(device, use_graph)
        if u0 is None:
            unit = {k: Prior(UNIFORM, 0.0, 1.0, 'quantile') for k in self.names}
            u0 = Design(priors=unit, names=self.names, seed=self.seed).sample(self.S, device=self.device, method='lhs').T
            u0 = np.clip(u0.cpu().numpy(), self.lb, self.ub)
        z = zeros_on(self.device)
        self.u0 = torch.as_tensor(np.ascontiguousarray(u0), device=self.device)
        self.direc0 = torch.as_tensor(np.array(direc0), device=self.device)               # (a copy: broadcast_to's is read-only)
        self.vec, self.direc, self.scal = z(self.S, _lib.POWELL_VEC_ROWS, d), z(self.S, d, d), z(self.S, _lib.POWELL_SCALARS)
        self.cand_f, self.theta = z(self.S), z(self.S, d)
        self.state = z(self.S, _lib.POWELL_STATE_WORDS, dt=torch.int64)
        self.history = z(0, self.S)

    def _launch(self, finalize: int):
        """finalize 0: a step; 1: theta = x; 2: theta = best_x"""
        import torch
        p, ptr = t_ptr, np_ptr
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_powell_step_f64_dev(
                self.S, self.d, int(finalize), self.xtol, self.ftol, self._max_iter, math.sqrt(2.2e-16),
                0.5 * (3.0 - math.sqrt(5.0)), ptr(self.kind), ptr(self.a), ptr(self.b), ptr(self.lb), ptr(self.ub), p(self.vec),
                p(self.direc), p(self.scal), p(self.cand_f), p(self.theta), p(self.state),
                p(self.history) if self.history.numel() else None, self.history.shape[0],
                current_stream_ptr(self.device)))

    def _step(self):
        self._launch(False)
        self.cand_f.copy_(self.f(self.theta))

    _body = _step

    def reset(self):
        """Back to the starts and the initial directions (the next launch emits the starts)."""
        self.state.zero_()
        self.vec[:, 0].copy_(self.u0)
        self.direc.copy_(self.direc0)

    def _record_key(self):
        return super()._record_key() + (self._max_iter,)

    def _prepare(self, n_launches: int, max_iter: int):
        """`_Search._prepare`; the graph is recorded again when max_iterations changes as well (it is a kernel argument)"""
        self._max_iter = max_iter
        super()._prepare(n_launches)

    def run(self, max_iterations=None, max_evaluations=None, check_every: int = 50) -> PowellResult:
        """Search until every start has finished -- the ftol test, or `max_iterations` completed iterations -- or has consumed
        `max_evaluations` values, then finalize.  scipy's rule for the limits: both None means 1000 d each, one given leaves
        the other unbounded.  Every running search consumes one value per launch, so a search stopped by `max_evaluations`
        ends exactly as scipy's does when maxfev interrupts it: theta is the point after the last completed line search.
        The host reads `state` every `check_every` launches."""
        import torch
        if max_iterations is None and max_evaluations is None:
            max_iterations = max_evaluations = 1000 * self.d
        if (max_iterations is not None and max_iterations < 1) or (max_evaluations is not None and max_evaluations < 1) \
                or check_every < 1:
            raise ValueError('max_iterations >= 1, max_evaluations >= 1 and check_every >= 1')
        # launch 0 emits the start and consumes nothing.  With max_evaluations unbounded the history keeps the first 1000 d
        # values (the kernel writes no row past the buffer) and the launches go on until every search has finished.
        n = None if max_evaluations is None else int(max_evaluations) + 1
        self._prepare(1000 * self.d + 1 if n is None else n, 0 if max_iterations is None else int(max_iterations))
        c, _ = self._search(n, check_every, check_every, lambda: bool((self.state[:, 3] != 0).all().item()))
        self._launch(2)                       # theta = every search's best_x, as f saw it
        best_theta = self.theta.cpu().numpy()
        self._launch(1)                        # theta = every search's x
        torch.cuda.synchronize(self.device)
        st = self.state.cpu().numpy()
        vec, scal = self.vec.cpu().numpy(), self.scal.cpu().numpy()
        best_value = scal[:, 19].copy()
        return PowellResult(theta=self.theta.cpu().numpy(), u=vec[:, 0].copy(), value=-scal[:, 16], nit=st[:, 1].copy(),
                            nfev=st[:, 2].copy(), converged=st[:, 3] == 1, status=np.where(st[:, 3] == 0, 3, st[:, 3]),
                            best_theta=best_theta, best_u=vec[:, 4].copy(), best_value=best_value, direc=self.direc.cpu().numpy(),
                            counters={k: st[:, 8 + j].copy() for j, k in enumerate(POWELL_COUNTERS)},
                            best=int(np.argmax(best_value)), history=self.history[:min(c - 1, self.history.shape[0])].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------- DIRECT
DIRECT_STATUS = {0: 'running', 1: 'max_evaluations exceeded', 2: 'max_iterations reached', 4: 'vol_tol met', 5: 'len_tol met',
                 6: 'the store or the level table cannot hold the next round', 7: 'a value was NaN or infinite'}


def direct_tables(d: int):
    """(thirds (D + 1,), levels (D d,)) of pem_direct_step_f64_dev as the host rounds them, D = the exponents the level table
    of PEM_DIRECT_MAX_LEVELS entries holds for d dimensions"""
    n = min(_lib.DIRECT_MAX_LEVELS // d, _lib.DIRECT_MAX_DEPTH)
    thirds = np.empty(n + 1)
    thirds[0] = 1.0
    h = 3.0
    for i in range(1, n + 1):
        thirds[i] = 1.0 / h
        h *= 3.0
    w = [math.sqrt(d - j + j / 9.) * 0.5 for j in range(d)]
    levels = np.empty(n * d)
    h = 1.0
    for i in range(n):
        for j in range(d):
            levels[i * d + j] = w[j] / h
        h *= 3.0
    return thirds, levels


@dataclass
class DirectResult:
    theta: np.ndarray        # (d,) the point of the best centre, as f saw it
    u: np.ndarray            # (d,) scipy's x in search coordinates: c xs1 + xs1 xs2 (an ulp from the point evaluated)
    value: float             # f there (scipy's -fun)
    nit: int                 # scipy's nit
    nfev: int                # values consumed (scipy's nfev)
    status: int              # DIRECT_STATUS; 1, 2, 4 and 5 are scipy's
    launches: int            # launches up to the one that ended the search
    history: np.ndarray      # (launches - 1, 3) best value, nfev and nit after every launch that consumed values


class Direct(_Search):
    """scipy's `direct(f, bounds, eps=..., vol_tol=..., len_tol=..., locally_biased=False)` (run_mle(optimizer='direct'),
    mcmc.py:170-231, which passes eps=1), MAXIMISING f, with the rectangles on the device.

    DIRECT needs no start, no covariance and no random numbers, and a selection round asks for the 2 |I| points of every
    rectangle it divides at once.  One launch of `pem_direct_step_f64_dev` (csrc/pem_direct.hip, one workgroup) takes the values
    of the rows it emitted last, completes those divisions, selects when the round is over and emits the points of as many
    selected rectangles as fit into `rows`; those are the rows of ONE call of f.  The search runs in the prior's quantile cube,
    bounded by `search_bounds`; every point, x, fun, nit, nfev and the status are scipy 1.15's bit for bit while no two values
    tie (include/pem_hip.h says what happens when they do, and which statuses are not scipy's).

    f: callable (rows, d) float64 device tensor -> rows values, like `Powell`'s: `post.log_posterior` of a posterior built with
       n_chains = direct.rows, shared_nuisance=True and fresh_nuisance=False.  Rows left over in a launch carry the best point
       and their values are ignored.
    rows: at least 2 d (one rectangle's points are never split); the smallest multiple of 64 that is if None.
    use_graph: a step (the launch, f's launches and the copy of the values) is one hipGraph replay on one stream."""

    def __init__(self, f, names, priors=None, rows=None, eps: float = 1e-4, vol_tol: float = 1e-16, len_tol: float = 1e-6,
                 use_graph: bool = False, device=None, locally_biased: bool = False):
        self.names = tuple(names)
        self.d = d = len(self.names)
        if len(set(self.names)) != d or d < 1:
            raise ValueError('names must be distinct and non-empty')
        if d > _lib.DIRECT_MAX_DIM:
            raise ValueError(f'at most {_lib.DIRECT_MAX_DIM} searched inputs (got {d})')
        if locally_biased:
            raise ValueError('locally_biased=True (DIRECT_L) is not restated; run_mle calls direct(..., locally_biased=False)')
        self.rows = -(-2 * d // 64) * 64 if rows is None else int(rows)
        if not 2 * d <= self.rows <= _lib.DIRECT_MAX_ROWS:
            raise ValueError(f'rows must be in [2 d = {2 * d}, {_lib.DIRECT_MAX_ROWS}] (got {self.rows})')
        if not (0.0 <= eps < math.inf):
            raise ValueError('eps must be finite and >= 0')
        if not (0.0 <= vol_tol <= 1.0 and 0.0 <= len_tol <= 1.0):
            raise ValueError('vol_tol and len_tol must be in [0, 1]')
        self.kind, self.a, self.b = _table(self.names, priors)
        self.lb, self.ub = search_bounds(self.names, priors)
        self.f, self.eps, self.vol_tol, self.len_tol = f, float(eps), float(vol_tol), float(len_tol)
        self._max_iter, self._max_fun, self.cap = 1000, 1000 * d, 0
        thirds, levels = direct_tables(d)
        self.n_depth = thirds.size - 1

        import torch
        self._init_loop(device, use_graph)
        z = zeros_on(self.device)
        self.thirds, self.levels = torch.as_tensor(thirds, device=self.device), torch.as_tensor(levels, device=self.device)
        self.cand_f, self.theta = z(self.rows), z(self.rows, d)
        self.queue, self.rowinfo = z(_lib.DIRECT_MAX_LEVELS, dt=torch.int32), z(self.rows, 2, dt=torch.int32)
        self.state = z(_lib.DIRECT_STATE_WORDS, dt=torch.int64)
        self.history = z(0, _lib.DIRECT_HISTORY_COLS)
        self._store(2 * d + 1)

    def _store(self, cap: int):
        """room for cap rectangles"""
        import torch
        if cap != self.cap:
            z = zeros_on(self.device)
            self.cap = cap
            self.centres, self.values = z(cap, self.d), z(cap)
            self.expo, self.level = z(cap, self.d, dt=torch.int32), z(cap, dt=torch.int32)

    def _launch(self, finalize: bool):
        import torch
        p, ptr = t_ptr, np_ptr
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_direct_step_f64_dev(
                self.d, self.rows, self.cap, self.n_depth, 1 if finalize else 0, self.eps, self.vol_tol, self.len_tol,
                self._max_iter, self._max_fun, ptr(self.kind), ptr(self.a), ptr(self.b), ptr(self.lb), ptr(self.ub),
                p(self.thirds), p(self.levels), p(self.centres), p(self.values), p(self.expo), p(self.level), p(self.queue),
                p(self.rowinfo), p(self.cand_f), p(self.theta), p(self.state),
                p(self.history) if self.history.numel() else None, self.history.shape[0], current_stream_ptr(self.device)))

    def _step(self):
        self._launch(False)
        self.cand_f.copy_(self.f(self.theta))

    _body = _step

    def reset(self):
        """Back to the start (the next launch emits the centre of the cube)."""
        self.state.zero_()

    def _record_key(self):
        return super()._record_key() + (self._max_iter, self._max_fun, self.cap, self.centres.data_ptr(), self.values.data_ptr(),
                                        self.expo.data_ptr(), self.level.data_ptr())

    def run(self, max_iterations: int = 1000, max_evaluations=None, check_every: int = 10) -> DirectResult:
        """Search until one of scipy's stops: `max_iterations` (its maxiter: the start's division and max_iterations - 2
        selection rounds), more than `max_evaluations` values after a whole round (its maxfun; None: 1000 d), vol_tol or
        len_tol.  The store is sized for max_evaluations and one more round; status 6 says it was too small.  The host reads
        the status every `check_every` launches."""
        import torch
        max_evaluations = 1000 * self.d if max_evaluations is None else int(max_evaluations)
        if max_iterations < 1 or max_evaluations < 1 or check_every < 1:
            raise ValueError('max_iterations >= 1, max_evaluations >= 1 and check_every >= 1')
        cap = max_evaluations + 1 + 2 * self.d * _lib.DIRECT_MAX_DEPTH
        if cap > _lib.DIRECT_MAX_STORE:
            raise ValueError(f'max_evaluations asks for a store of {cap} rectangles (at most {_lib.DIRECT_MAX_STORE})')
        self._store(cap)
        self._max_iter, self._max_fun = int(max_iterations), max_evaluations
        # every launch after the first stores at least two rectangles or ends the search
        n = cap // 2 + 3 + int(check_every)
        self._prepare(n)
        c, _ = self._search(n, check_every, check_every, lambda: self.state[3].item() != 0)
        self._launch(True)                      # row 0 of theta = the best centre's point
        torch.cuda.synchronize(self.device)
        st = self.state.cpu().numpy()
        best, end = int(st[6]), int(st[9]) if st[3] != 0 else c
        xs1 = self.ub - self.lb
        xs2 = self.lb / xs1
        centre = self.centres[best].cpu().numpy()
        return DirectResult(theta=self.theta[0].cpu().numpy(), u=centre * xs1 + xs1 * xs2,
                            value=-float(self.values[best].item()) if st[2] >= 1 else math.nan,
                            nit=int(st[1]), nfev=int(st[2]), status=int(st[3]), launches=end,
                            history=self.history[:max(end - 1, 0)].cpu().numpy())


# ----------------------------------------------------------------------------------------------------------- Laplace
def stencil_size(d: int) -> int:
    """rows of `hessian`'s stencil: the centre, +-h_i and +-h_i +-h_j"""
    return 2 * d * d + 1


def theta_steps(theta, names, priors=None, step: float = 1e-3):
    """h_j = step * d theta_j / d u_j at theta: (b - a) uniform, theta ln10 (b - a) log-uniform, sigma / phi(z) normal"""
    kind, a, b = _table(names, priors)
    t = np.asarray(theta, dtype=np.float64)
    h = np.where(kind == UNIFORM, b - a, 0.0)
    h = np.where(kind == LOGUNIFORM, t * math.log(10.0) * (b - a), h)
    z = np.where(kind == NORMAL, (t - a) / np.where(kind == NORMAL, b, 1.0), 0.0)
    h = np.where(kind == NORMAL, b * math.sqrt(2.0 * math.pi) * np.exp(0.5 * z * z), h)
    return step * h


def stencil(theta, h):
    """(2 d^2 + 1, d) points: the centre, then theta +- h_i e_i, then theta (+-) h_i e_i (+-) h_j e_j for i < j"""
    t, h = np.asarray(theta, dtype=np.float64), np.asarray(h, dtype=np.float64)
    d = t.size
    rows = [t.copy()]
    for i in range(d):
        for s in (1.0, -1.0):
            r = t.copy()
            r[i] += s * h[i]
            rows.append(r)
    for i in range(d):
        for j in range(i + 1, d):
            for si, sj in ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0)):
                r = t.copy()
                r[i] += si * h[i]
                r[j] += sj * h[j]
                rows.append(r)
    return np.stack(rows)


def hessian(f, theta, names, priors=None, step: float = 1e-3, device=None):
    """Central-difference Hessian of f at theta from ONE call of f on the (2 d^2 + 1, d) stencil (`stencil`), steps
    `theta_steps`.  f: (2 d^2 + 1, d) float64 tensor on `device` (default CPU) -> values, e.g. `post.log_posterior` of a
    posterior with n_chains = stencil_size(d) and shared_nuisance=True.  Every stencil point must lie in the prior support."""
    import torch
    names = tuple(names)
    priors_ = PEM_V0_PRIORS if priors is None else priors
    t = np.asarray(theta, dtype=np.float64)
    d = len(names)
    if t.shape != (d,):
        raise ValueError(f'theta must have one entry per name ({d})')
    h = theta_steps(t, names, priors_, step)
    pts = stencil(t, h)
    for j, k in enumerate(names):
        if priors_[k].kind == NORMAL:
            continue
        lo, hi = support(priors_[k])
        if pts[:, j].min() < lo or pts[:, j].max() > hi:
            raise ValueError(f"the Hessian stencil leaves the prior support of '{k}' ({lo:g}, {hi:g}) at {t[j]:g}: "
                             'a MAP on a bound has no Laplace approximation there')
    dev = torch.device('cpu') if device is None else torch.device(device)
    v = f(torch.as_tensor(pts, device=dev))
    v = (v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)).astype(np.float64)
    f0, k = v[0], 1 + 2 * d
    H = np.empty((d, d))
    for i in range(d):
        H[i, i] = (v[1 + 2 * i] - 2.0 * f0 + v[2 + 2 * i]) / (h[i] * h[i])
    for i in range(d):
        for j in range(i + 1, d):
            pp, pm, mp, mm = v[k:k + 4]
            H[i, j] = H[j, i] = (pp - pm - mp + mm) / (4.0 * h[i] * h[j])
            k += 4
    return H


def is_positive_definite(A) -> bool:
    try:
        np.linalg.cholesky(A)
        return True
    except np.linalg.LinAlgError:
        return False


def nearest_positive_definite(A):
    """Higham's nearest symmetric positive-definite matrix to A (Higham 1988, "Computing a nearest symmetric positive
    semidefinite matrix"): the mean of the symmetric part and its polar factor, then a diagonal shift by the smallest
    eigenvalue until a Cholesky factorisation succeeds.  A symmetric positive-definite A is returned unchanged."""
    A = np.asarray(A, dtype=np.float64)
    if np.array_equal(A, A.T) and is_positive_definite(A):
        return A.copy()
    B = 0.5 * (A + A.T)
    _, s, V = np.linalg.svd(B)
    X = 0.5 * (B + V.T @ np.diag(s) @ V)
    X = 0.5 * (X + X.T)
    spacing = np.spacing(np.linalg.norm(A))
    eye = np.eye(A.shape[0])
    k = 1
    while not is_positive_definite(X):
        X += eye * (-np.min(np.linalg.eigvalsh(X)) * k * k + spacing)
        k += 1
    return X


class Laplace:
    """Gaussian approximation of the posterior at its mode (run_laplace / show_laplace, mcmc.py:234-265): mean = the mode,
    hess = the Hessian of the log posterior there, cov = pinv(-hess), replaced by its nearest positive-definite matrix when
    it is not positive definite (`nearest_pd` records that).  The pseudo-inverse is taken in coordinates scaled by
    |hess_ii|^-1/2 (the same matrix when hess is invertible): the parameters span twelve decades (P_T ~ 1e-5, c4 ~ 1e20),
    and pinv's cut-off, relative to the largest singular value, would otherwise discard the directions of the large ones."""

    def __init__(self, mean, hess):
        self.mean = np.asarray(mean, dtype=np.float64).copy()
        self.hess = np.asarray(hess, dtype=np.float64).copy()
        dg = np.abs(np.diag(self.hess))
        s = np.where((dg > 0) & np.isfinite(dg), 1.0 / np.sqrt(np.where(dg > 0, dg, 1.0)), 1.0)
        cov = s[:, None] * np.linalg.pinv(-(s[:, None] * self.hess * s[None, :])) * s[None, :]
        cov = 0.5 * (cov + cov.T)
        self.nearest_pd = not is_positive_definite(cov)
        self.cov = nearest_positive_definite(cov) if self.nearest_pd else cov

    @classmethod
    def fit(cls, f, mean, names, priors=None, step: float = 1e-3, device=None):
        """`hessian(f, mean, ...)` and the approximation built from it"""
        return cls(mean, hessian(f, mean, names, priors, step=step, device=device))

    @property
    def std(self):
        return np.sqrt(np.diag(self.cov))

    def sample(self, n: int, seed: int = 0):
        """(n, d) draws of N(mean, cov)"""
        L = np.linalg.cholesky(self.cov)
        return self.mean + np.random.default_rng(seed).standard_normal((int(n), self.mean.size)) @ L.T

    def dram_start(self):
        """(theta0, cov0) for `samplers.DRAM`"""
        return self.mean.copy(), self.cov.copy()


# ------------------------------------------------------------------------------------------------------------ slices
def slice_points(names, x0, n_steps: int = 15, bounds=None, priors=None):
    """(d n_steps, d) rows: axis j of x0 swept over bounds[j] (default the prior support; geometric steps for a log-uniform
    prior), the other entries held at x0.  Bounds outside the support are refused."""
    names = tuple(names)
    priors = PEM_V0_PRIORS if priors is None else priors
    x0 = np.asarray(x0, dtype=np.float64)
    d = len(names)
    if x0.shape != (d,) or n_steps < 2:
        raise ValueError(f'x0 must have one entry per name ({d}) and n_steps >= 2')
    rows = np.repeat(x0[None], d * n_steps, axis=0)
    for j, k in enumerate(names):
        p = priors[k]
        lo, hi = support(p)
        blo, bhi = (lo, hi) if bounds is None else (float(bounds[j][0]), float(bounds[j][1]))
        if not (blo < bhi) or (p.kind != NORMAL and (blo < lo or bhi > hi)):
            raise ValueError(f"slice bounds ({blo:g}, {bhi:g}) of '{k}' are not an interval inside its prior support "
                             f'({lo:g}, {hi:g})')
        grid = np.geomspace(blo, bhi, n_steps) if p.kind == LOGUNIFORM else np.linspace(blo, bhi, n_steps)
        rows[j * n_steps:(j + 1) * n_steps, j] = grid
    return rows


def slices(post, x0, n_steps: int = 15, bounds=None):
    """1-D slices of the log prior, log likelihood and log posterior through x0 (pdf_slice, mcmc.py:132-148): a dict of
    (d, n_steps) arrays 'grid', 'prior', 'likelihood', 'posterior'.  post: a posterior with n_chains = d n_steps and
    shared_nuisance=True; one prior launch and one likelihood launch over all rows."""
    import torch
    d = len(post.names)
    if not getattr(post, 'shared', False):
        raise ValueError('slices compare rows: build the posterior with shared_nuisance=True')
    if post.K != d * n_steps:
        raise ValueError(f'the posterior has {post.K} rows, the slices need d * n_steps = {d * n_steps}')
    rows = slice_points(post.names, x0, n_steps, bounds, post.priors)
    theta = torch.as_tensor(rows, device=post.device)
    lp = post.log_prior(theta)
    ll = post.log_likelihood(theta)
    # the marginalisation kernel's rule for the posterior: prior + likelihood where both are usable, -inf elsewhere
    lpost = torch.where(torch.isfinite(lp) & ~torch.isnan(ll), lp + ll, torch.full_like(lp, -math.inf))
    grid = np.stack([rows[j * n_steps:(j + 1) * n_steps, j] for j in range(d)])
    out = {'grid': grid}
    for k, v in (('prior', lp), ('likelihood', ll), ('posterior', lpost)):
        out[k] = v.cpu().numpy().reshape(d, n_steps)
    return out
