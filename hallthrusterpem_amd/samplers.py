"""Samplers of a log posterior given as any callable on torch tensors: `calibration`'s posteriors, or a closed form.

`Metropolis` is K random-walk chains around a `calibration.BatchedPosterior`, a whole accept/reject step in one hipGraph replay.
`DRAM` restates the reference's sampler as torch operations around two posterior evaluations per step; `DeviceDRAM` is the same
algorithm with the sampler's own work in one launch per step (`pem_dram_step_f64_dev`) and both proposals in ONE evaluation.
`DeviceEnsemble` is the affine-invariant ensemble sampler (stretch and DE moves), which needs no proposal covariance: half an
ensemble's walkers per evaluation, one launch of `pem_ensemble_step_f64_dev` per half-step.
`DeviceTemperedEnsemble` is replica exchange over it for a posterior with more than one mode: a ladder of tempered ensembles per
replica, swaps between neighbouring temperatures inside `pem_tempered_ensemble_step_f64_dev`, the log evidence by thermodynamic
integration.
`DeviceSMC` is tempered sequential Monte Carlo (TMCMC) for when there is no start at all: populations of particles drawn from the
prior, the next temperature found from the particles, resampling and Metropolis moves in `pem_smc_stage_f64_dev` /
`pem_smc_move_f64_dev`, equally weighted posterior draws and the log evidence in one pass.

The device samplers record their step into a hipGraph and replay it; `_device_loop` holds that loop and its rules.
"""
import math

import numpy as np

from . import _device_loop as loop
from . import _lib
from ._device_loop import RecordedLoop, TracedLoop, capture_graph
from ._marshal import current_stream_ptr, t_ptr
from .sampling import Design


class Metropolis:
    """K independent random-walk Metropolis chains advanced together, one hipGraph replay per step.

    A stand-in for the delayed-rejection adaptive Metropolis of the reference (`mcmciterators`, third-party, absent;
    call site mcmc.py:283-300): same role -- draw from `log_posterior` -- simplest valid kernel.  Proposal:
    theta' = theta + scale * N(0, I) with a per-parameter `scale`; the nuisance draws inside the posterior are the
    recorded ones (common random numbers), i.e. the chain targets the M-sample marginal likelihood estimate."""

    def __init__(self, posterior, theta0, scale, seed: int = 0, use_graph: bool = True):
        import torch
        self.post = posterior
        dev = posterior.device
        self.theta = torch.as_tensor(np.asarray(theta0, dtype=np.float64), device=dev).expand(
            posterior.K, len(posterior.names)).contiguous()
        self.scale = torch.as_tensor(np.asarray(scale, dtype=np.float64), device=dev)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.accepted = torch.zeros(posterior.K, dtype=torch.int64, device=dev)
        fresh, posterior.fresh = posterior.fresh, False
        self.logp = posterior.log_posterior(self.theta).clone()
        posterior.fresh = fresh
        self.steps = 0
        self._graph = None
        if use_graph:           # the warm-up steps before the recording are undone: the chain starts at theta0
            theta_start, logp_start = self.theta.clone(), self.logp.clone()
            posterior.fresh = False
            self._graph, _ = capture_graph(self._step, dev, generator=self.gen)
            posterior.fresh = fresh
            self.theta.copy_(theta_start)
            self.logp.copy_(logp_start)
            self.accepted.zero_()

    def _step(self):
        import torch
        prop = self.theta + self.scale * torch.randn(self.theta.shape, dtype=torch.float64, device=self.theta.device,
                                                     generator=self.gen)
        logp = self.post.log_posterior(prop)
        u = torch.rand(self.post.K, dtype=torch.float64, device=self.theta.device, generator=self.gen)
        accept = torch.log(u) < (logp - self.logp)                 # -inf proposals are never accepted; NaN compares false
        self.theta.copy_(torch.where(accept[:, None], prop, self.theta))
        self.logp.copy_(torch.where(accept, logp, self.logp))
        self.accepted.add_(accept.to(torch.int64))

    def run(self, n_steps: int, keep: bool = True):
        """Advance every chain n_steps; returns the (n_steps, K, n_theta) trace (device tensor) if `keep`."""
        import torch
        trace = (torch.empty((n_steps,) + tuple(self.theta.shape), dtype=torch.float64, device=self.theta.device)
                 if keep else None)
        for i in range(n_steps):
            if self._graph is not None:
                self._graph.replay()
            else:
                self._step()
            if keep:
                trace[i].copy_(self.theta)
        self.steps += n_steps
        return trace

    @property
    def acceptance(self):
        return self.accepted.double() / max(1, self.steps)


class DRAM:
    """K chains of delayed-rejection adaptive Metropolis (Haario, Laine, Mira & Saksman 2006) advanced together -- the
    algorithm behind the reference's `uq.dram(fun, p0, niter, cov0=None, adapt_after=5000, adapt_interval=1000, eps=1e-12,
    gamma=0.1)` (scripts/pem_v0/mcmc.py:297-298; `uqtils` is third-party and absent: parity UNPINNED, the keyword names and
    their meaning are that call's).  Per step and chain:

      stage 1   y1 = x + L z1,  L L^T = C;  accepted with a1 = min(1, pi(y1) / pi(x))
      stage 2   (on rejection) y2 = x + sqrt(gamma) L z2, accepted with
                a2 = min(1, pi(y2) q(y1 | y2) [1 - a1(y2 -> y1)] / (pi(x) q(y1 | x) [1 - a1(x -> y1)]))
      adaptation  after `adapt_after` steps, every `adapt_interval` steps: C = (2.4^2 / d) (cov(chain so far) + eps I), from a
                running mean / scatter matrix per chain (Welford)

    `log_posterior(theta[K, d]) -> logp[K]` is any callable on torch tensors (a `JionPosterior` / `SystemPosterior`
    `.log_posterior`, or a closed form
    on the CPU in the tests).  Both stages are evaluated for all chains every step (a fixed launch sequence: with
    `use_graph` the step is one hipGraph replay, as `Metropolis`); the adaptation runs between replays and updates `L` in place."""

    def __init__(self, log_posterior, theta0, cov0=None, n_chains: int | None = None, seed: int = 0, adapt_after: int = 5000,
                 adapt_interval: int = 1000, eps: float = 1e-12, gamma: float = 0.1, device=None, use_graph: bool = False):
        import torch
        self.f = log_posterior
        t0 = np.atleast_1d(np.asarray(theta0, dtype=np.float64))
        if t0.ndim == 1:
            t0 = np.broadcast_to(t0, (int(n_chains or 1), t0.size))
        self.K, self.d = t0.shape
        dev = torch.device(device) if device is not None else torch.device('cpu')
        self.theta = torch.as_tensor(np.ascontiguousarray(t0), device=dev).clone()
        c0 = np.eye(self.d) if cov0 is None else np.asarray(cov0, dtype=np.float64)
        if c0.ndim == 1:
            c0 = np.diag(c0)
        self.L = torch.linalg.cholesky(torch.as_tensor(c0, device=dev)).expand(self.K, self.d, self.d).contiguous()
        self.adapt_after, self.adapt_interval, self.eps, self.gamma = int(adapt_after), int(adapt_interval), float(eps), float(gamma)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.logp = self.f(self.theta).clone()
        self.accepted = torch.zeros((2, self.K), dtype=torch.int64, device=dev)          # per stage
        self.mean = self.theta.clone()                                                    # running moments of the chain
        self.scatter = torch.zeros((self.K, self.d, self.d), dtype=torch.float64, device=dev)
        self.count = 1
        self.steps = 0
        self._graph = None
        if use_graph:
            state = [t.clone() for t in (self.theta, self.logp, self.accepted)]
            self._graph, _ = capture_graph(self._step, dev, generator=self.gen)
            for t, s in zip((self.theta, self.logp, self.accepted), state):
                t.copy_(s)

    def _step(self):
        import torch
        K, d, dev = self.K, self.d, self.theta.device
        x, lp0, L = self.theta, self.logp, self.L
        z = torch.randn((2, K, d), dtype=torch.float64, device=dev, generator=self.gen)
        u = torch.rand((2, K), dtype=torch.float64, device=dev, generator=self.gen)
        y1 = x + torch.einsum('kij,kj->ki', L, z[0])
        lp1 = self.f(y1)
        a1 = torch.exp((lp1 - lp0).clamp(max=0.0))                        # NaN (e.g. -inf - -inf) compares false below: rejected
        acc1 = u[0] < a1
        y2 = x + math.sqrt(self.gamma) * torch.einsum('kij,kj->ki', L, z[1])
        lp2 = self.f(y2)
        a1_rev = torch.exp((lp1 - lp2).clamp(max=0.0))                    # first-stage acceptance of y1 seen from y2
        w = torch.linalg.solve_triangular(L, (y1 - y2).unsqueeze(-1), upper=False).squeeze(-1)
        log_q = -0.5 * ((w * w).sum(dim=1) - (z[0] * z[0]).sum(dim=1))    # log q(y1 | y2) - log q(y1 | x)
        log_a2 = (lp2 - lp0) + log_q + torch.log1p(-a1_rev) - torch.log1p(-a1)
        acc2 = (~acc1) & (torch.log(u[1]) < log_a2)                        # a1 = 1 is accepted at stage 1; a1_rev = 1 gives -inf
        self.theta.copy_(torch.where(acc1[:, None], y1, torch.where(acc2[:, None], y2, x)))
        self.logp.copy_(torch.where(acc1, lp1, torch.where(acc2, lp2, lp0)))
        self.accepted[0].add_(acc1.to(torch.int64))
        self.accepted[1].add_(acc2.to(torch.int64))

    def _adapt(self):
        import torch
        n = self.count
        if n < 2:
            return
        cov = self.scatter / (n - 1) + self.eps * torch.eye(self.d, dtype=torch.float64, device=self.theta.device)
        self.L.copy_(torch.linalg.cholesky((2.4 ** 2 / self.d) * cov))

    def run(self, n_steps: int, keep: bool = True):
        """Advance every chain n_steps; returns the (n_steps, K, d) trace if `keep`."""
        import torch
        trace = torch.empty((n_steps, self.K, self.d), dtype=torch.float64, device=self.theta.device) if keep else None
        for i in range(n_steps):
            if self._graph is not None:
                self._graph.replay()
            else:
                self._step()
            self.steps += 1
            self.count += 1                                               # Welford update of the chain's mean and scatter
            delta = self.theta - self.mean
            self.mean += delta / self.count
            self.scatter += delta[:, :, None] * (self.theta - self.mean)[:, None, :]
            if self.steps >= self.adapt_after and (self.steps - self.adapt_after) % self.adapt_interval == 0:
                self._adapt()
            if keep:
                trace[i].copy_(self.theta)
        return trace

    @property
    def acceptance(self):
        """(2, K): fraction of steps accepted at the first and at the delayed stage"""
        return self.accepted.double() / max(1, self.steps)


class DeviceDRAM(TracedLoop):
    """`DRAM` with the whole sampler on the device: K chains of delayed-rejection adaptive Metropolis, one launch of
    `pem_dram_step_f64_dev` (csrc/pem_dram.hip) per step.  That launch resolves the step whose two proposals were just
    evaluated -- accept decisions, point, Welford moments, adaptation of L, trace row -- and draws both proposals of the next
    step, so a step is [log_posterior(prop) ; the launch], with `use_graph` one hipGraph replay, and nothing runs on the host
    between steps.  The keywords are `DRAM`'s and mean what they mean there; the draws are Philox4x32-10 keyed by `seed`
    (include/pem_hip.h), not torch's generator, so the two samplers visit different states.

    log_posterior: callable on a (2K, d) float64 device tensor returning (2K,) values, as `DifferentialEvolution`'s f takes
    (P, d).  Rows k and K + k are chain k's first-stage and delayed-stage proposals.  ITS VALUE MUST NOT DEPEND ON THE ROW:
    a closed form, or `.log_posterior` of a `SystemPosterior` / `JionPosterior` / `SurrogatePosterior` built with
    n_chains=2K, shared_nuisance=True, fresh_nuisance=False.  Otherwise a chain's kept logp and its next proposal would be
    judged under different nuisance draws.

    The constructor evaluates theta0 once, through the same 2K-row call, and draws the proposals of step 1.  `run` continues
    across calls: run(a) followed by run(b) visits the states of run(a + b).  There is no CPU path."""

    def __init__(self, log_posterior, theta0, cov0=None, n_chains: int | None = None, seed: int = 0, adapt_after: int = 5000,
                 adapt_interval: int = 1000, eps: float = 1e-12, gamma: float = 0.1, device=None, use_graph: bool = True):
        import torch
        t0, device = loop.starts(theta0, device)
        t0 = np.atleast_1d(t0)
        if t0.ndim == 1:
            t0 = np.broadcast_to(t0, (int(n_chains or 1), t0.size))
        if t0.ndim != 2 or t0.shape[0] < 1:
            raise ValueError('theta0 must be (d,) or (K, d)')
        self.K, self.d = t0.shape
        if not 1 <= self.d <= _lib.DRAM_MAX_DIM:
            raise ValueError(f'DeviceDRAM samples 1 to {_lib.DRAM_MAX_DIM} parameters (got {self.d})')
        loop.require_cuda('DeviceDRAM', device, ': use DRAM for CPU tensors')
        if not gamma > 0.0 or eps < 0.0 or int(adapt_interval) < 1 or int(adapt_after) < 0:
            raise ValueError('need gamma > 0, eps >= 0, adapt_interval >= 1 and adapt_after >= 0')
        c0 = np.eye(self.d) if cov0 is None else np.asarray(cov0, dtype=np.float64)
        if c0.ndim == 1:
            c0 = np.diag(c0)
        if c0.shape != (self.d, self.d):
            raise ValueError(f'cov0 must be ({self.d},) or ({self.d}, {self.d})')
        self.f, self.seed = log_posterior, int(seed)
        self.adapt_after, self.adapt_interval, self.eps, self.gamma = int(adapt_after), int(adapt_interval), float(eps), float(gamma)
        self._init_loop(device, use_graph)
        K, d, dev = self.K, self.d, self.device
        z = loop.zeros_on(dev)
        self.theta = torch.as_tensor(np.ascontiguousarray(t0), device=dev).clone()
        self.L = torch.linalg.cholesky(torch.as_tensor(c0, device=dev)).expand(K, d, d).contiguous()
        self.mean, self.scatter = self.theta.clone(), z(K, d, d)                             # running moments of the chain
        self.prop, self.prop_logp = z(2, K, d), z(2, K)
        self.state, self.accepted, self.flags = z(K, dt=torch.int64), z(2, K, dt=torch.int64), z(K, dt=torch.int32)
        self.steps = 0
        self._init_trace((K, d), (K,))                                                       # the trace and its logp
        self.prop.copy_(self.theta.expand(2, K, d))
        self.logp = self.f(self.prop.view(2 * K, d))[:K].clone()
        self._launch()                                                                       # launch 0: the proposals of step 1

    def _launch(self):
        import torch
        p = t_ptr
        first, length, thin = self._window
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_dram_step_f64_dev(
                self.K, self.d, self.seed, self.gamma, self.eps, self.adapt_after, self.adapt_interval, first, length, thin,
                p(self.theta), p(self.logp), p(self.L), p(self.mean), p(self.scatter), p(self.prop), p(self.prop_logp),
                p(self.state), p(self.accepted), p(self.flags), p(self._traces[0]), p(self._traces[1]), None,
                current_stream_ptr(self.device)))

    def _step(self):
        self.prop_logp.view(-1).copy_(self.f(self.prop.view(2 * self.K, self.d)))
        self._launch()

    _body = _step

    def _state(self):
        return (self.theta, self.logp, self.L, self.mean, self.scatter, self.prop, self.prop_logp, self.state, self.accepted,
                self.flags)

    def run(self, n_steps: int, keep: bool = True, thin: int = 1, keep_logp: bool = False):
        """Advance every chain n_steps.  Returns the (ceil(n_steps / thin), K, d) trace as a device tensor if `keep` -- steps
        1, 1 + thin, ... of this call -- and with `keep_logp` the pair (trace, logp trace (ceil(n_steps / thin), K))."""
        trace, logp_trace = self._run(n_steps, thin, (keep, keep and keep_logp))
        if not keep:
            return None
        return (trace, logp_trace) if keep_logp else trace

    @property
    def acceptance(self):
        """(2, K): fraction of steps accepted at the first and at the delayed stage"""
        return self.accepted.double() / max(1, self.steps)

    @property
    def adaptation_failures(self) -> int:
        """chains that skipped an adaptation because their covariance had a pivot that was not > 0 (`DRAM` would raise there)"""
        return int((self.flags & 1).sum())


class DeviceEnsemble(TracedLoop):
    """The affine-invariant ensemble sampler (Goodman & Weare 2010, the algorithm of emcee; third-party and absent here: parity
    UNPINNED) with the whole sampler on the device: E independent ensembles of K walkers, one launch of
    `pem_ensemble_step_f64_dev` (csrc/pem_ensemble.hip) per half-step.  It needs NO proposal covariance and behaves identically
    under any affine change of the parameters, which is what a posterior whose parameters span forty decades asks for.

    An ensemble's walkers are two fixed halves of H = K / 2.  A step moves half 0 against half 1, then half 1 against the new
    half 0; each launch resolves the half-step whose H proposals were just evaluated and proposes the next, so a step is
    [log_posterior(prop) ; launch ; log_posterior(prop) ; launch] on one stream, with `use_graph` one hipGraph replay without
    parallel branches.  Per (ensemble, half-step) the half takes the DE move (ter Braak; y = x + g (x_j1 - x_j2), g = g0 (1 +
    sigma n), g0 = 2.38 / sqrt(2d) by default) with probability `de_fraction`, otherwise the stretch move of scale `a`
    (y = x_j + z (x - x_j), z = ((a - 1) u + 1)^2 / a, weight z^(d - 1)).  emcee's random re-split of the halves is not done.
    The draws are Philox4x32-10 keyed by `seed` (include/pem_hip.h).

    log_posterior: callable on an (E H, d) float64 device tensor returning (E H,) values.  ITS VALUE MUST NOT DEPEND ON THE
    ROW, as for `DeviceDRAM`: a closed form, or `.log_posterior` of a `SystemPosterior` / `JionPosterior` / `SurrogatePosterior`
    built with n_chains=E*H, shared_nuisance=True, fresh_nuisance=False.

    theta0: (K, d) starts (n_ensembles == 1) or (E, K, d); K even and >= 2d, as emcee asks.  Every start must have a finite
    log posterior (they are evaluated half by half through the same call).  `ball` draws starts around a point.  `run`
    continues across calls.  There is no CPU path.

    Reading the result: the trace is (rows, E, K, d).  THE WALKERS OF ONE ENSEMBLE ARE NOT INDEPENDENT CHAINS -- each moves
    along lines through the others -- so R-hat and ESS belong on the E ensemble-mean series,
    `diagnostics.summary(trace.mean(dim=2))`, while `trace.reshape(rows, E * K, d)` is what `marginals` pools."""

    def __init__(self, log_posterior, theta0, n_ensembles: int = 1, seed: int = 0, a: float = 2.0, de_fraction: float = 0.0,
                 g0: float | None = None, sigma: float = 1e-5, device=None, use_graph: bool = True):
        import torch
        t0, device = loop.starts(theta0, device)
        if t0.ndim == 2 and int(n_ensembles) == 1:
            t0 = t0[None]
        if t0.ndim != 3 or (int(n_ensembles) not in (1, t0.shape[0])):
            raise ValueError('theta0 must be (K, d) with n_ensembles == 1, or (E, K, d)')
        self.E, self.K, self.d = t0.shape
        g0 = loop.ensemble_parameters('DeviceEnsemble', self.E, self.K, self.d, a, de_fraction, g0, sigma)
        loop.require_cuda('DeviceEnsemble', device)
        self.f, self.seed = log_posterior, int(seed)
        self.a, self.de_fraction, self.g0, self.sigma = float(a), float(de_fraction), g0, float(sigma)
        self._init_loop(device, use_graph)
        E, K, d, dev = self.E, self.K, self.d, self.device
        H = self.H = K // 2
        z = loop.zeros_on(dev)
        self.theta = torch.as_tensor(np.ascontiguousarray(t0), device=dev).clone()
        self.prop, self.prop_logp, self.log_q = z(E, H, d), z(E, H), z(E, H)
        self.state, self.accepted = z(E, dt=torch.int64), z(E, K, dt=torch.int64)
        self.steps = 0
        self._init_trace((E, K, d), (E, K))                                                  # the trace and its logp
        halves = []
        for h in (0, 1):                                                                     # the starts, half by half
            self.prop.copy_(self.theta[:, h * H:(h + 1) * H])
            halves.append(self.f(self.prop.view(E * H, d)).reshape(E, H).clone())
        self.logp = torch.cat(halves, dim=1).contiguous()
        if not bool(torch.isfinite(self.logp).all()):
            bad = int((~torch.isfinite(self.logp)).sum())
            raise ValueError(f'{bad} of the {E * K} starts have a log posterior that is not finite: every walker must start '
                             'inside the support')
        self._launch()                                                                       # launch 0: the proposals of half-step 1

    @staticmethod
    def ball(center, scale, n_walkers: int, n_ensembles: int = 1, seed: int = 0):
        """(n_ensembles, n_walkers, d) starts center + scale * N(0, 1) from np.random.default_rng(seed); `scale` a number or
        one per parameter (a fraction of |center|, the width of a prior).  The final population of
        `optimize.DifferentialEvolution` and draws from `optimize.Laplace` are natural starts as well: they already have the
        posterior's shape, and this sampler needs nothing else."""
        return loop.ball(center, scale, (n_ensembles, n_walkers), seed)

    def _launch(self):
        import torch
        p = t_ptr
        first, length, thin = self._window
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_ensemble_step_f64_dev(
                self.E, self.K, self.d, self.seed, self.a, self.de_fraction, self.g0, self.sigma, first, length, thin,
                p(self.theta), p(self.logp), p(self.prop), p(self.prop_logp), p(self.log_q), p(self.state), p(self.accepted),
                p(self._traces[0]), p(self._traces[1]), None, current_stream_ptr(self.device)))

    def _step(self):
        for _ in range(2):
            self.prop_logp.view(-1).copy_(self.f(self.prop.view(self.E * self.H, self.d)))
            self._launch()

    _body = _step

    def _state(self):
        return (self.theta, self.logp, self.prop, self.prop_logp, self.log_q, self.state, self.accepted)

    def run(self, n_steps: int, keep: bool = True, thin: int = 1, keep_logp: bool = False):
        """Advance every ensemble n_steps whole steps (each walker is proposed to once per step).  Returns the
        (ceil(n_steps / thin), E, K, d) trace as a device tensor if `keep` -- steps 1, 1 + thin, ... of this call -- and with
        `keep_logp` the pair (trace, logp trace (ceil(n_steps / thin), E, K))."""
        trace, logp_trace = self._run(n_steps, thin, (keep, keep and keep_logp))
        if not keep:
            return None
        return (trace, logp_trace) if keep_logp else trace

    @property
    def acceptance(self):
        """(E, K): fraction of its proposals each walker accepted"""
        return self.accepted.double() / max(1, self.steps)


class DeviceTemperedEnsemble(TracedLoop):
    """Replica exchange (parallel tempering) over `DeviceEnsemble`, for a posterior with more than one mode: R independent
    replicas of a ladder of T inverse temperatures 1 = beta_0 > beta_1 > ... >= 0, at every (replica, temperature) one ensemble
    of K walkers that samples prior(x) likelihood(x)^beta_t, E = R T ensembles in all, one launch of
    `pem_tempered_ensemble_step_f64_dev` (csrc/pem_tempering.hip) per half-step.  ptemcee, which runs this over emcee, is
    third-party and absent here: parity UNPINNED; the rules are this project's own (include/pem_hip.h) and
    tests/tempering_np.py restates them.

    The moves are `DeviceEnsemble`'s stretch and DE moves with the same draws, accepted iff
    log u < log q + (pi' - pi) + beta_t (l' - l); a proposal whose l or pi is not finite is refused at every temperature, beta = 0
    included.  After the second half-step of step n (n = 1, 2, ...) the pairs (t, t + 1) with t = n mod 2 (mod 2) are visited:
    walker k of t and walker k of t + 1 exchange places iff log u < (beta_t - beta_{t+1}) (l_{t+1,k} - l_{t,k}).  The hot
    ensembles cross between modes, the swaps hand their points down, and t = 0 is the posterior itself.  A step is
    [l(prop), pi(prop) ; launch ; l(prop), pi(prop) ; launch] on one stream, with `use_graph` one hipGraph replay without
    parallel branches.

    log_likelihood, log_prior: callables on an (E H, d) float64 device tensor (H = K / 2) returning (E H,) values THAT DO NOT
    DEPEND ON THE ROW: closed forms, or `.log_likelihood` and `.log_prior` of a `SystemPosterior` / `JionPosterior` /
    `SurrogatePosterior` built with n_chains=E*H, shared_nuisance=True, fresh_nuisance=False.

    betas: the ladder, strictly decreasing from 1, finite, >= 0; None: `ladder(n_temperatures, beta_min, include_prior)`, the
    geometric ladder from 1 down to beta_min with a final 0 appended when include_prior (thermodynamic integration needs it).
    theta0: (K, d), (T, K, d) or (R, T, K, d) starts, K even and >= 2d; every start must have a finite l and pi.  `ball` draws
    starts around a point.  `run` continues across calls.  There is no CPU path.

    Reading the result: the trace is (rows, R, T, K, d) with `loglik_trace` and `logprior_trace` (rows, R, T, K) beside it (the
    last kept run's).  `cold()` is its t = 0 slice, the posterior's draws; the other temperatures are not.  `swap_rates()` is
    what a ladder is tuned by: a rate near 0 between two temperatures means they do not talk.  `log_evidence()` integrates the
    mean log likelihood over beta."""

    def __init__(self, log_likelihood, log_prior, theta0, betas=None, n_temperatures: int = 8, n_replicas: int = 1,
                 beta_min: float = 1e-2, include_prior: bool = False, seed: int = 0, a: float = 2.0, de_fraction: float = 0.0,
                 g0: float | None = None, sigma: float = 1e-5, device=None, use_graph: bool = True):
        import torch
        t0, device = loop.starts(theta0, device)
        self.betas = self.ladder(n_temperatures, beta_min, include_prior) if betas is None else self.check_ladder(betas)
        T, R = self.betas.size, int(n_replicas)
        if R < 1 or t0.ndim not in (2, 3, 4) or (t0.ndim >= 3 and t0.shape[-3] != T) or (t0.ndim == 4 and t0.shape[0] != R):
            raise ValueError(f'theta0 must be (K, d), (T, K, d) or (R, T, K, d) with T = {T} temperatures and R = n_replicas = {R} '
                             f'(got {t0.shape})')
        t0 = np.array(np.broadcast_to(t0, (R, T) + t0.shape[-2:]))
        self.R, self.T, self.K, self.d = t0.shape
        self.E = self.R * self.T
        g0 = loop.ensemble_parameters('DeviceTemperedEnsemble', self.E, self.K, self.d, a, de_fraction, g0, sigma)
        if not np.isfinite(t0).all():
            bad = int((~np.isfinite(t0).all(axis=-1)).sum())
            raise ValueError(f'{bad} of the {self.E * self.K} starts have a coordinate that is not finite')
        loop.require_cuda('DeviceTemperedEnsemble', device)
        self.f_lik, self.f_prior, self.seed = log_likelihood, log_prior, int(seed)
        self.a, self.de_fraction, self.g0, self.sigma = float(a), float(de_fraction), g0, float(sigma)
        self._init_loop(device, use_graph)
        E, K, d, dev = self.E, self.K, self.d, self.device
        H = self.H = K // 2
        z = loop.zeros_on(dev)
        self._beta = torch.as_tensor(self.betas, device=dev).clone()
        self.theta = torch.as_tensor(np.ascontiguousarray(t0.reshape(E, K, d)), device=dev).clone()
        self.prop, self.prop_loglik, self.prop_logprior, self.log_q = z(E, H, d), z(E, H), z(E, H), z(E, H)
        self.state, self.accepted = z(R, dt=torch.int64), z(E, K, dt=torch.int64)
        self.swap_attempts, self.swap_accepted = z(R, T - 1, dt=torch.int64), z(R, T - 1, dt=torch.int64)
        self.steps = 0
        self.trace = self.loglik_trace = self.logprior_trace = None                          # of the last kept run
        self._init_trace((E, K, d), (E, K), (E, K))                                          # the trace, its loglik and logprior
        halves = ([], [])
        for h in (0, 1):                                                                     # the starts, half by half
            self.prop.copy_(self.theta[:, h * H:(h + 1) * H])
            for f, got in zip((self.f_lik, self.f_prior), halves):
                got.append(f(self.prop.view(E * H, d)).reshape(E, H).clone())
        self.loglik, self.logprior = (torch.cat(got, dim=1).contiguous() for got in halves)
        finite = torch.isfinite(self.loglik) & torch.isfinite(self.logprior)
        if not bool(finite.all()):
            raise ValueError(f'{int((~finite).sum())} of the {E * K} starts have a log likelihood or a log prior that is not '
                             'finite: every walker must start inside the support')
        self._launch()                                                                       # launch 0: the proposals of half-step 1

    @staticmethod
    def check_ladder(betas):
        """the ladder as a float64 array, or ValueError: T >= 1, finite, strictly decreasing from 1, >= 0"""
        b = np.array(betas, dtype=np.float64).reshape(-1)
        if b.size < 1 or not np.isfinite(b).all():
            raise ValueError(f'the ladder needs T >= 1 finite inverse temperatures (got {betas})')
        if b[0] != 1.0 or np.any(np.diff(b) >= 0.0) or b[-1] < 0.0:
            raise ValueError(f'the ladder must decrease strictly from 1 and stay >= 0 (got {b.tolist()})')
        return b

    @staticmethod
    def ladder(n_temperatures: int = 8, beta_min: float = 1e-2, include_prior: bool = False):
        """n_temperatures inverse temperatures beta_min^(t / (n - 1)), from 1 down to beta_min, and a final 0 when include_prior
        (T = n_temperatures + 1 then)"""
        n = int(n_temperatures)
        if n < 1 or (n > 1 and not 0.0 < beta_min < 1.0):
            raise ValueError('the ladder needs n_temperatures >= 1 and 0 < beta_min < 1')
        b = np.ones(1) if n == 1 else float(beta_min) ** (np.arange(n) / (n - 1.0))
        b[0] = 1.0
        return DeviceTemperedEnsemble.check_ladder(np.append(b, 0.0) if include_prior else b)

    @staticmethod
    def ball(center, scale, n_walkers: int, n_temperatures: int = 1, n_replicas: int = 1, seed: int = 0):
        """(n_replicas, n_temperatures, n_walkers, d) starts center + scale * N(0, 1) from np.random.default_rng(seed), as
        `DeviceEnsemble.ball`"""
        return loop.ball(center, scale, (n_replicas, n_temperatures, n_walkers), seed)

    def _launch(self):
        import torch
        p = t_ptr
        first, length, thin = self._window
        swaps = (p(self.swap_attempts), p(self.swap_accepted)) if self.T > 1 else (None, None)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_tempered_ensemble_step_f64_dev(
                self.R, self.T, self.K, self.d, self.seed, self.a, self.de_fraction, self.g0, self.sigma, p(self._beta), first, length,
                thin, p(self.theta), p(self.loglik), p(self.logprior), p(self.prop), p(self.prop_loglik), p(self.prop_logprior),
                p(self.log_q), p(self.state), p(self.accepted), *swaps, *[p(t) for t in self._traces], None,
                current_stream_ptr(self.device)))

    def _step(self):
        for _ in range(2):
            flat = self.prop.view(self.E * self.H, self.d)
            self.prop_loglik.view(-1).copy_(self.f_lik(flat))
            self.prop_logprior.view(-1).copy_(self.f_prior(flat))
            self._launch()

    _body = _step

    def _state(self):
        return (self.theta, self.loglik, self.logprior, self.prop, self.prop_loglik, self.prop_logprior, self.log_q, self.state,
                self.accepted, self.swap_attempts, self.swap_accepted)

    def run(self, n_steps: int, keep: bool = True, thin: int = 1):
        """Advance every ensemble n_steps whole steps (two half-steps and the swaps that are due).  Returns the
        (ceil(n_steps / thin), R, T, K, d) trace as a device tensor if `keep` -- steps 1, 1 + thin, ... of this call, each as the
        swaps left it -- and keeps it with its (rows, R, T, K) log likelihoods and log priors as `trace`, `loglik_trace`,
        `logprior_trace` for `cold`, `mean_loglik` and `log_evidence`."""
        traces = self._run(n_steps, thin, (keep, keep, keep))
        if not keep:
            self.trace = self.loglik_trace = self.logprior_trace = None
            return None
        shape = (traces[0].shape[0], self.R, self.T, self.K)
        self.trace, self.loglik_trace, self.logprior_trace = traces[0].view(*shape, self.d), traces[1].view(shape), traces[2].view(shape)
        return self.trace

    def _kept(self):
        if self.trace is None:
            raise ValueError('no trace: the last run was not kept')
        return self.trace

    def cold(self, means: bool = False):
        """the t = 0 slice of the last kept trace, (rows, R, K, d): the posterior's draws, which `marginals` pools as
        cold().reshape(rows, R * K, d); with `means` the R ensemble-mean series (rows, R, d) that `diagnostics.summary` reads
        (the walkers of one ensemble are not independent chains)"""
        cold = self._kept()[:, :, 0]
        return cold.mean(dim=2) if means else cold

    def swap_rates(self):
        """(R, T - 1): the fraction of the walker pairs of (t, t + 1) offered a swap that took it"""
        return self.swap_accepted.double() / self.swap_attempts.double().clamp(min=1.0)

    def move_rates(self):
        """(R, T): the fraction of its move proposals an ensemble's walkers accepted"""
        return self.accepted.double().mean(dim=1).view(self.R, self.T) / max(1, self.steps)

    def mean_loglik(self, burn: int = 0):
        """(R, T): the mean log likelihood at every temperature over the walkers and the rows [burn:] of the last kept run"""
        self._kept()
        if not 0 <= int(burn) < self.loglik_trace.shape[0]:
            raise ValueError(f'burn must leave a row of the {self.loglik_trace.shape[0]} kept')
        return self.loglik_trace[int(burn):].mean(dim=(0, 3))

    @staticmethod
    def evidence_from(mean_loglik, betas):
        """Thermodynamic integration, log Z = integral over [0, 1] of E_beta[l] d beta, by the trapezoid rule on the ladder.
        mean_loglik: (R, T).  Returns dict(log_z (R,) per replica, discretisation (R,): |log_z - the trapezoid over every second
        ladder point (both ends kept)|, NaN for T < 3; mean: of log_z; spread: its standard deviation over the replicas, NaN for
        R = 1).  ValueError when the ladder does not end at 0: the integral needs the prior's end."""
        b = DeviceTemperedEnsemble.check_ladder(betas)
        if b[-1] != 0.0:
            raise ValueError(f'log_evidence needs a ladder that ends at beta = 0 (include_prior=True); this one ends at {b[-1]}')
        ml = np.asarray(mean_loglik, dtype=np.float64).reshape(-1, b.size)
        trap = lambda idx: (0.5 * (ml[:, idx[:-1]] + ml[:, idx[1:]]) * (b[idx[:-1]] - b[idx[1:]])).sum(axis=1)   # noqa: E731
        fine = np.arange(b.size)
        coarse = np.union1d(fine[::2], fine[-1:])
        log_z = trap(fine)
        disc = np.abs(log_z - trap(coarse)) if b.size >= 3 else np.full_like(log_z, np.nan)
        return dict(log_z=log_z, discretisation=disc, mean=float(log_z.mean()),
                    spread=float(log_z.std(ddof=1)) if log_z.size > 1 else float('nan'))

    def log_evidence(self, burn: int = 0):
        """`evidence_from(mean_loglik(burn), betas)`: the log evidence per replica, its discretisation estimate and its spread
        over the replicas"""
        ml = self.mean_loglik(burn).cpu().numpy() if self.betas[-1] == 0.0 else np.zeros((self.R, self.T))   # (no ladder end: raises)
        return self.evidence_from(ml, self.betas)


class SMCResult:
    """What `DeviceSMC.run` returns.  theta (R, N, d), loglik, logprior (R, N): device tensors, N equally weighted draws of the
    posterior per population.  log_evidence (R,), stages (R,), converged (R,) (beta reached 1), flags (R,) (bit 0: a Cholesky
    factor was refused and the previous one kept; bit 1: no particle had a finite log likelihood): host arrays.  betas, ess,
    acceptance, log_evidence_increments: (R, stages) host arrays, one column per stage, NaN past a population's last stage."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def as_trace(self):
        """The particles as an (N, R, d) trace: N rows of R 'chains', what `marginals.corner(trace, names, burnin=0)` and
        `predictive.flatten_chain` read.  The rows are equally weighted draws, not successive states of a chain: `diagnostics`
        (split R-hat, autocorrelation, chain ESS) DOES NOT APPLY to them; `ess` per stage is the particle diagnostic."""
        return self.theta.permute(1, 0, 2).contiguous()


class DeviceSMC(RecordedLoop):
    """Tempered sequential Monte Carlo (TMCMC, Ching & Chen 2007; the SMC sampler of Del Moral et al. 2006; PyMC's sample_smc --
    all third-party and absent here: parity UNPINNED; the rules are this project's own, include/pem_hip.h and DESIGN.md 4.6.9, and
    tests/smc_np.py restates them) with the whole sampler on the device: R independent populations of N particles are carried
    from the prior to the posterior along prior x likelihood^beta.  It needs NO start, NO proposal covariance and NO ladder: the
    next beta is the one that brings the effective sample size of the incremental weights down to tau N (bisection inside
    `pem_smc_stage_f64_dev`), the proposal is the weighted covariance of the particles, and the result is N equally weighted
    posterior draws per population AND the log evidence.

    One stage is [stage launch ; (log_likelihood(prop), log_prior(prop) ; move launch) x n_mcmc] on one stream: the stage launch
    (one workgroup per population) finds beta', adds log mean w to the evidence, factorises scale^2 cov + eps I, resamples
    systematically and proposes; each move launch (`pem_smc_move_f64_dev`, all R N particles) resolves a random-walk Metropolis
    proposal against prior x likelihood^beta' and proposes the next, the last one with propose = 0.  With `use_graph` a stage is
    one hipGraph replay without parallel branches.  A finished population ignores further replays.

    log_likelihood, log_prior: callables on an (R N, d) float64 device tensor returning (R N,) values THAT DO NOT DEPEND ON THE
    ROW: closed forms, or `.log_likelihood` and `.log_prior` of a `SystemPosterior` / `JionPosterior` / `SurrogatePosterior` built
    with n_chains=R*N, shared_nuisance=True, fresh_nuisance=False.

    theta0: (N, d) or (R, N, d) draws FROM THE PRIOR (`prior_draws` makes them).  THE EVIDENCE IS THE MEAN OF THE LIKELIHOOD UNDER
    THE LAW theta0 WAS DRAWN FROM: starts from anything else give the evidence against that law, and posterior draws only if
    log_prior is that law's density.  Every start needs a finite log prior; a log likelihood that is not finite is allowed and
    has weight 0; a population without any finite log likelihood is refused.  scale: None = 2.38 / sqrt(d).  There is no CPU
    path."""

    def __init__(self, log_likelihood, log_prior, theta0, n_populations: int = 1, tau: float = 0.5, n_mcmc: int = 3,
                 scale: float | None = None, eps: float = 1e-12, seed: int = 0, device=None, use_graph: bool = True):
        import torch
        t0, device = loop.starts(theta0, device)
        if t0.ndim == 2 and int(n_populations) == 1:
            t0 = t0[None]
        if t0.ndim != 3 or int(n_populations) not in (1, t0.shape[0]):
            raise ValueError('theta0 must be (N, d) with n_populations == 1, or (R, N, d)')
        self.R, self.N, self.d = t0.shape
        if not 1 <= self.d <= _lib.SMC_MAX_DIM:
            raise ValueError(f'DeviceSMC samples 1 to {_lib.SMC_MAX_DIM} parameters (got {self.d})')
        if self.R < 1 or not 2 <= self.N <= _lib.SMC_MAX_PARTICLES:
            raise ValueError(f'DeviceSMC needs 2 <= N <= {_lib.SMC_MAX_PARTICLES} particles per population (got {self.N})')
        if not np.isfinite(t0).all():
            raise ValueError(f'{int((~np.isfinite(t0).all(axis=-1)).sum())} of the {self.R * self.N} starts have a coordinate that is '
                             'not finite')
        if not 0.0 < tau < 1.0:
            raise ValueError(f'tau must be in (0, 1) (got {tau})')
        if int(n_mcmc) != n_mcmc or int(n_mcmc) < 1:
            raise ValueError(f'n_mcmc must be a whole number >= 1 (got {n_mcmc})')
        scale = 2.38 / math.sqrt(self.d) if scale is None else float(scale)
        if not (scale > 0.0 and math.isfinite(scale) and eps >= 0.0):
            raise ValueError('need a finite scale > 0 and eps >= 0')
        loop.require_cuda('DeviceSMC', device)
        self.f_lik, self.f_prior, self.seed = log_likelihood, log_prior, int(seed)
        self.tau, self.n_mcmc, self.scale, self.eps = float(tau), int(n_mcmc), scale, float(eps)
        self._init_loop(device, use_graph)
        R, N, d, dev = self.R, self.N, self.d, self.device
        z = loop.zeros_on(dev)
        self.theta = torch.as_tensor(np.ascontiguousarray(t0), device=dev).clone()
        flat = self.theta.view(R * N, d)
        self.loglik = self.f_lik(flat).reshape(R, N).clone()
        self.logprior = self.f_prior(flat).reshape(R, N).clone()
        if not bool(torch.isfinite(self.logprior).all()):
            raise ValueError(f'{int((~torch.isfinite(self.logprior)).sum())} of the {R * N} starts have a log prior that is not '
                             'finite: the starts are draws from the prior')
        if not bool(torch.isfinite(self.loglik).any(dim=1).all()):
            raise ValueError('a population has no start with a finite log likelihood')
        self.beta, self.log_evidence, self.stage = z(R), z(R), z(R, dt=torch.int64)
        self.L, self.prop, self.prop_loglik, self.prop_logprior = z(R, d, d), z(R, N, d), z(R, N), z(R, N)
        self.accept_count, self.accepted = z(R, N, dt=torch.int32), z(R, dt=torch.int64)
        self.flags, self.moves_active = z(R, dt=torch.int32), z(R, dt=torch.int32)
        self.scratch = z(R, N, d + 2)
        self._hist = None                                                                    # (4, R, history_len), made by run

    @staticmethod
    def prior_draws(names, priors=None, n_particles: int = 1024, n_populations: int = 1, seed: int = 0, method: str = 'sobol',
                    device=None):
        """(n_populations, n_particles, len(names)) draws of `names` from their priors (None: PEM_V0_PRIORS) as a device tensor,
        through `sampling.Design`: population r is points 0 ... n_particles - 1 of the design with (seed, stream = r) -- for
        'sobol' a Sobol' set with its own random digital shift per population, for 'mc' independent draws."""
        import torch
        if method not in ('sobol', 'mc'):
            raise ValueError(f"method must be 'sobol' or 'mc' (got '{method}')")
        dev = loop.cuda_device(device)
        out = torch.empty((int(n_populations), len(names), int(n_particles)), dtype=torch.float64, device=dev)
        for r in range(int(n_populations)):
            Design(priors=priors, names=names, seed=seed, stream=r).fill(out[r], method=method)
        return out.transpose(1, 2).contiguous()

    def _args(self):
        return (self.R, self.N, self.d, self.seed, self.tau, self.scale, self.eps, self.n_mcmc)

    def _launch_stage(self, record=None):
        import torch
        p = t_ptr
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_smc_stage_f64_dev(
                *self._args(), p(self.theta), p(self.loglik), p(self.logprior), p(self.beta), p(self.log_evidence), p(self.stage),
                p(self.L), p(self.prop), p(self.accept_count), p(self.accepted), p(self.flags), p(self.moves_active), p(self.scratch),
                *[p(h) for h in self._hist], self._hist.shape[2], p(record), current_stream_ptr(self.device)))

    def _launch_move(self, move: int, propose: bool, record=None):
        import torch
        p = t_ptr
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_smc_move_f64_dev(
                *self._args(), int(move), 1 if propose else 0, p(self.theta), p(self.loglik), p(self.logprior), p(self.beta),
                p(self.stage), p(self.L), p(self.prop), p(self.prop_loglik), p(self.prop_logprior), p(self.accept_count),
                p(self.moves_active), p(record), current_stream_ptr(self.device)))

    def _stage(self):
        self._launch_stage()
        flat = self.prop.view(self.R * self.N, self.d)
        for m in range(1, self.n_mcmc + 1):
            self.prop_loglik.view(-1).copy_(self.f_lik(flat))
            self.prop_logprior.view(-1).copy_(self.f_prior(flat))
            self._launch_move(m, m < self.n_mcmc)

    _body = _stage

    def _state(self):
        return (self.theta, self.loglik, self.logprior, self.beta, self.log_evidence, self.stage, self.L, self.prop, self.prop_loglik,
                self.prop_logprior, self.accept_count, self.accepted, self.flags, self.moves_active, self.scratch, self._hist)

    def _record_key(self):
        return (self._hist.data_ptr(), self._hist.shape[2])

    def _prepare(self, history_len: int):
        """the history arrays grow to hold every stage of this run and keep what they hold; they are part of the record key"""
        if self._hist is None or self._hist.shape[2] < history_len:
            hist = loop.zeros_on(self.device)(4, self.R, history_len)
            if self._hist is not None:
                hist[:, :, :self._hist.shape[2]] = self._hist
            self._hist = hist
        super()._prepare()

    def run(self, max_stages: int = 200, check_every: int = 4):
        """Replay stages, reading beta and flags back once per `check_every` stages, until every population is at beta = 1, or
        flag bit 1 is up, or max_stages stages of this call have run.  The result does not depend on check_every: a finished
        population ignores the replays past its end.  Returns an `SMCResult`; a later call continues."""
        max_stages, check_every = int(max_stages), int(check_every)
        if max_stages < 0 or check_every < 1:
            raise ValueError('max_stages >= 0 and check_every >= 1')
        done = int(self.stage.max())
        self._prepare(done + max(max_stages, 1))
        ran = 0
        while ran < max_stages:
            beta, flags = self.beta.cpu().numpy(), self.flags.cpu().numpy()
            if (beta == 1.0).all() or (flags & 2).any():
                break
            n = min(check_every, max_stages - ran)
            self.advance(n)
            ran += n
        return self.result()

    def result(self):
        """the `SMCResult` of the state as it stands"""
        stages = self.stage.cpu().numpy().astype(np.int64)
        hist = self._hist.cpu().numpy().copy() if self._hist is not None else np.zeros((4, self.R, 0))
        n = int(stages.max()) if stages.size else 0
        hist = hist[:, :, :n]
        # the acceptance of a stage is closed by the stage launch that follows it; where none has followed, from the same counts
        count = self.accept_count.cpu().numpy().astype(np.int64).sum(axis=1)
        active = self.moves_active.cpu().numpy().astype(bool)
        for r in np.nonzero(active & (stages >= 1) & (stages <= hist.shape[2]))[0]:
            hist[2, r, stages[r] - 1] = float(count[r]) / (float(self.N) * float(self.n_mcmc))
        hist[:, np.arange(n)[None, :] >= stages[:, None]] = np.nan
        beta = self.beta.cpu().numpy()
        return SMCResult(theta=self.theta.clone(), loglik=self.loglik.clone(), logprior=self.logprior.clone(),
                         log_evidence=self.log_evidence.cpu().numpy(), betas=hist[0], ess=hist[1], acceptance=hist[2],
                         log_evidence_increments=hist[3], stages=stages, converged=beta == 1.0,
                         flags=self.flags.cpu().numpy().astype(np.uint32))
