"""Posterior of PEM-v0 calibration parameters given measured ion current density, evaluated for many chains at once.

Restates the flow of `spt100_log_likelihood` / `spt100_log_prior` / `spt100_log_posterior`
(scripts/pem_v0/mcmc.py:57-130) for the `jion` quantity with the TRUE coupled model in place of the surrogate:

    theta (K, n_theta)  ->  inputs of shape (K, M, Ne): operating conditions fixed per experiment e, theta broadcast,
                            every other variable drawn from its prior (M nuisance draws)          mcmc.py:60-63
                        ->  model + Gaussian log-likelihood summed over the Ne x Na measurements   mcmc.py:76-98
                        ->  + discharge-current weight, summed over Ne                              mcmc.py:102-104
                        ->  log-sum-exp over the M nuisance draws (constants dropped)               mcmc.py:106-107

One posterior evaluation is five launches: `pem_log_prior_f64_dev`, `pem_sample_f64_dev` (nuisance draws), two row
scatters, ONE `pem_coupled_loglik_f64_dev` (the profile never leaves LDS) and `pem_loglik_marginal_f64_dev`.  At MCMC batch
sizes (K M Ne ~ 1e4..1e5 samples) every launch is latency-bound, so `capture()` records the whole evaluation --
and `Metropolis` a whole accept/reject step -- into a hipGraph (torch.cuda.CUDAGraph) and replays it.

The reference scripts are stale and untested, its sampler (`mcmciterators` DRAM) and surrogate are third-party and
absent: parity UNPINNED.  The likelihood is checked against the oracle + numpy (tests/test_calibration.py); the
discharge current of the analytic thruster test double is I_d = I_B0 / (1 - 2 a_1) (tests/sim_hallthruster.jl:35-48;
its `c1` is the anomalous-transport coefficient, PEM variable `a_1`).

`SystemPosterior` is the same flow for the reference's `System` calibration (mcmc.py:28-45, QOIS = V_cc, T, uion, jion): each
quantity from its own dataset at its own operating conditions (`likelihood.SystemLikelihood`), all compared in ONE fused launch
(`pem_coupled_system_loglik_f64_dev`), so that the cathode parameters are constrained by data as well as the plume's.

`SurrogatePosterior` is that flow as the reference runs it: the trained component surrogates (`chain.ChainedSurrogate`) in the
model's place, j_ion rebuilt from its SVD latents and I_D taken from the surrogate's output, all in ONE launch
(`pem_chain_system_loglik_f64_dev`) -- what a plugged-in thruster solver that costs seconds per sample needs.

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
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .batch import CoupledBatch
from .likelihood import JionLikelihood, SystemLikelihood
from .models.coupled import COUPLED_INPUTS
from .sampling import LOGUNIFORM, NORMAL, PEM_V0_PRIORS, UNIFORM, Design

Q_OVER_M = 1.6e-19 / 2.18e-25           # tests/sim_hallthruster.jl:36-37
OPERATING = ('P_b', 'V_a', 'mdot_a')    # XE_ARRAY columns, mcmc.py:46


def log_prior(theta, names, priors=None):
    """Sum of the log prior densities of `names` at theta (..., len(names)); -inf outside the bounds
    (mcmc.py:110-121).  Works on numpy arrays and on torch tensors (any device)."""
    priors = PEM_V0_PRIORS if priors is None else priors
    is_np = isinstance(theta, np.ndarray)
    if is_np:
        xp, total = np, np.zeros(theta.shape[:-1])
    else:
        import torch
        xp, total = torch, torch.zeros(theta.shape[:-1], dtype=theta.dtype, device=theta.device)
    ninf = -math.inf
    for i, k in enumerate(names):
        p, x = priors[k], theta[..., i]
        if p.kind == UNIFORM:
            lp = xp.where((x >= p.a) & (x <= p.b), xp.zeros_like(x) - math.log(p.b - p.a), ninf)
        elif p.kind == LOGUNIFORM:      # density of 10^U(a, b): 1 / (x ln10 (b - a))
            inside = (x >= 10.0 ** p.a) & (x <= 10.0 ** p.b)
            safe = xp.where(inside, x, xp.ones_like(x))
            lp = xp.where(inside, -xp.log(safe) - math.log(math.log(10.0) * (p.b - p.a)), ninf)
        elif p.kind == NORMAL:
            lp = -0.5 * ((x - p.a) / p.b) ** 2 - math.log(p.b * math.sqrt(2.0 * math.pi))
        else:
            raise ValueError(f'unknown prior kind {p.kind}')
        total = total + lp
    return total


class BatchedPosterior:
    """What the posteriors of this module share: K chains x M nuisance draws x Ne operating conditions in one `CoupledBatch`,
    the prior on the device, marginalisation, graph capture.  A subclass builds its likelihood and runs it (`_run_loglik`)."""

    def _setup(self, theta_names, operating, make_likelihood, n_chains, n_nuisance, priors, seed, discharge, sweep_radius,
               fresh_nuisance, shared_nuisance=False):
        import torch
        if shared_nuisance and fresh_nuisance:
            raise ValueError('shared_nuisance needs fresh_nuisance=False: shared draws are the same on every evaluation')
        self.names = tuple(theta_names)
        for k in self.names:
            if k not in COUPLED_INPUTS or k in OPERATING:
                raise KeyError(f"'{k}' is not a calibratable input of the coupled model")
        op = np.atleast_2d(np.asarray(operating, dtype=np.float64))
        self.K, self.M, self.Ne = int(n_chains), int(n_nuisance), op.shape[0]
        if op.shape[1] != len(OPERATING):
            raise ValueError('operating conditions are rows of (P_b, V_a, mdot_a)')
        self.priors = PEM_V0_PRIORS if priors is None else priors
        self.lik = make_likelihood()
        if self.lik.n_cond != self.Ne:
            raise ValueError('one row of measurements per operating condition')
        self.n = self.K * self.M * self.Ne
        self.batch = CoupledBatch(self.n, device=self.lik.device, profile=False, sweep_radius=sweep_radius,
                                  thruster_qoi=False)
        self.device = self.batch.device
        self.design = Design(priors=self.priors, seed=seed)
        self.operating = torch.as_tensor(op, device=self.device)                       # (Ne, 3)
        self.theta_rows = [COUPLED_INPUTS.index(k) for k in self.names]
        self.op_rows = [COUPLED_INPUTS.index(k) for k in OPERATING]
        self.discharge = None if discharge is None else (float(discharge[0]), float(discharge[1]))
        self.fresh = bool(fresh_nuisance)
        self.shared = bool(shared_nuisance)
        self.first_index = 0
        if self.shared:         # draws 0 .. M Ne - 1 of the design, broadcast over the K rows on every evaluation
            self._shared_block = self.design.fill(torch.empty((len(COUPLED_INPUTS), self.M * self.Ne), dtype=torch.float64,
                                                              device=self.device))
        self.loglik = torch.empty(self.n, dtype=torch.float64, device=self.device)
        self._view = lambda t: t.view(self.K, self.M, self.Ne)
        # few launches per evaluation (every one is latency-bound): row scatter indices and the prior table on device
        dev_i = lambda rows: torch.as_tensor(rows, dtype=torch.int64, device=self.device)                   # noqa: E731
        self._op_idx, self._theta_idx = dev_i(self.op_rows), dev_i(self.theta_rows)
        self._op_vals = self.operating.T.contiguous()[:, None, None, :]                 # (3, 1, 1, Ne)
        pr = [self.priors[k] for k in self.names]
        self._kind = np.ascontiguousarray([q.kind for q in pr], dtype=np.int32)
        self._a = np.ascontiguousarray([q.a for q in pr], dtype=np.float64)
        self._b = np.ascontiguousarray([q.b for q in pr], dtype=np.float64)
        # the log-uniform supports as log_prior decides them (10.0 ** a, 10.0 ** b on the host), for the device to compare against
        self._lo = np.ascontiguousarray([10.0 ** q.a if q.kind == LOGUNIFORM else q.a for q in pr], dtype=np.float64)
        self._hi = np.ascontiguousarray([10.0 ** q.b if q.kind == LOGUNIFORM else q.b for q in pr], dtype=np.float64)
        self._lp = torch.empty(self.K, dtype=torch.float64, device=self.device)
        self._out = torch.empty(self.K, dtype=torch.float64, device=self.device)

    def _run_loglik(self):
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------------ evaluation
    def assemble_inputs(self, theta):
        """Fill the batch: nuisance draws for everything, then the operating columns and theta broadcast over them."""
        x = self.batch.inputs.view(len(COUPLED_INPUTS), self.K, self.M, self.Ne)
        if self.shared:
            x.copy_(self._shared_block.view(len(COUPLED_INPUTS), 1, self.M, self.Ne).expand(-1, self.K, -1, -1))
        else:
            self.design.fill(self.batch.inputs, first_index=self.first_index)
            if self.fresh:
                self.first_index += self.n
        x.index_copy_(0, self._op_idx, self._op_vals.expand(-1, self.K, self.M, -1))
        x.index_copy_(0, self._theta_idx, theta.T[:, :, None, None].expand(-1, -1, self.M, self.Ne))

    def _marginal(self, log_prior, out):
        import torch
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                                    # noqa: E731
        x = self.batch.inputs
        d = self.discharge
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_loglik_marginal_f64_dev(
                self.K, self.M, self.Ne, p(self.loglik), p(x[COUPLED_INPUTS.index('mdot_a')]) if d else None,
                p(x[COUPLED_INPUTS.index('a_1')]) if d else None, d[0] if d else 0.0, d[1] if d else 1.0, p(log_prior),
                p(out), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    def log_likelihood(self, theta, out=None):
        """theta: (K, n_theta) float64 tensor on the device -> (K,) marginal log-likelihoods."""
        import torch
        assert theta.shape == (self.K, len(self.names)) and theta.dtype == torch.float64 and theta.device == self.device
        self.assemble_inputs(theta)
        self._run_loglik()
        return self._marginal(None, torch.empty_like(self._out) if out is None else out)

    def log_prior(self, theta, out=None):
        """`log_prior(theta, names, priors)` of this module for a (K, n_theta) device tensor (`pem_log_prior_f64_dev`)."""
        import torch
        theta = theta.contiguous()
        out = torch.empty(theta.shape[0], dtype=torch.float64, device=self.device) if out is None else out
        ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                                        # noqa: E731
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_log_prior_f64_dev(
                theta.shape[0], len(self.names), ptr(self._kind), ptr(self._a), ptr(self._b), ptr(self._lo), ptr(self._hi),
                C.c_void_p(theta.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    def log_posterior(self, theta, out=None):
        """Prior + likelihood; -inf outside the prior support and where the model produced NaN (mcmc.py:124-130 --
        there only in-support rows are evaluated; here all K rows run, shapes stay static for graph capture).
        Five launches: nuisance draws, two row scatters, model + likelihood, marginalisation + prior."""
        import torch
        assert theta.shape == (self.K, len(self.names)) and theta.dtype == torch.float64 and theta.device == self.device
        self.log_prior(theta, out=self._lp)
        self.assemble_inputs(theta)
        self._run_loglik()
        return self._marginal(self._lp, torch.empty_like(self._out) if out is None else out)

    # ---------------------------------------------------------------------------------------------- graph capture
    def capture(self):
        """Record `log_posterior` into a hipGraph.  Returns `replay(theta) -> (K,) tensor` (a static output buffer)."""
        import torch
        static_theta = torch.zeros((self.K, len(self.names)), dtype=torch.float64, device=self.device)
        for j, k in enumerate(self.names):                     # a point inside the support for the warm-up runs
            p = self.priors[k]
            static_theta[:, j] = 10.0 ** (0.5 * (p.a + p.b)) if p.kind == LOGUNIFORM else (p.a if p.kind == NORMAL else 0.5 * (p.a + p.b))
        fresh, self.fresh = self.fresh, False                  # a recorded launch carries its sample offset by value
        graph, out = capture_graph(lambda: self.log_posterior(static_theta), self.device)
        self.fresh = fresh

        def replay(theta):
            static_theta.copy_(theta)
            graph.replay()
            return out
        replay.graph, replay.theta, replay.out = graph, static_theta, out
        return replay


class JionPosterior(BatchedPosterior):
    def __init__(self, theta_names, operating, alpha, y, std, n_chains: int, n_nuisance: int = 100, priors=None,
                 seed: int = 0, discharge=(4.5, 0.2), sweep_radius: float = 1.0, fresh_nuisance: bool = True,
                 device=None, shared_nuisance: bool = False):
        """theta_names: calibrated inputs (subset of the 15 coupled inputs, not operating ones);
        operating: (Ne, 3) array of `P_b [Torr], V_a [V], mdot_a [kg/s]` per experiment;
        alpha, y, std: (Ne, Na) measurement angles [rad], current densities and standard deviations at `sweep_radius`;
        discharge: (I_d, sigma) of the extra discharge-current weight (mcmc.py:48-49,102-104) or None;
        fresh_nuisance: new nuisance draws on every evaluation (as the reference) -- inside a captured graph the
        draws are whatever was recorded (common random numbers);
        shared_nuisance: every row uses draws 0 .. M Ne - 1 of the design, so that a value depends on theta, seed, M and the
        data and not on the row or on K (what an optimizer or a finite-difference Hessian comparing rows needs); requires
        fresh_nuisance=False.  Otherwise row k uses draws k M Ne .. (k + 1) M Ne - 1."""
        self._setup(theta_names, operating, lambda: JionLikelihood(alpha, y, std, device=device), n_chains, n_nuisance, priors,
                    seed, discharge, sweep_radius, fresh_nuisance, shared_nuisance)

    def _run_loglik(self):
        self.batch.run_loglik(self.lik, out=self.loglik)


class SystemPosterior(BatchedPosterior):
    def __init__(self, theta_names, likelihood: SystemLikelihood, n_chains: int, n_nuisance: int = 100, priors=None,
                 seed: int = 0, discharge=(4.5, 0.2), fresh_nuisance: bool = True, shared_nuisance: bool = False):
        """The posterior of the reference's `System` calibration (mcmc.py:28-130): V_cc, thrust, ion velocity and ion current
        density, each from its own dataset (`likelihood.SystemLikelihood`, whose conditions are the Ne operating conditions
        here), evaluated by ONE fused launch (`pem_coupled_system_loglik_f64_dev`) per evaluation.  The interface of
        `JionPosterior`; theta_names, n_chains, n_nuisance, priors, seed, fresh_nuisance, shared_nuisance as there.
        discharge: (I_d, sigma) of the discharge-current weight added for every condition, or None; dropped when the
        likelihood's component is 'Cathode' (mcmc.py:100-101)."""
        if not likelihood.use_discharge:
            discharge = None
        self._setup(theta_names, likelihood.operating, lambda: likelihood, n_chains, n_nuisance, priors, seed, discharge,
                    likelihood.sweep_radius, fresh_nuisance, shared_nuisance)

    def _run_loglik(self):
        self.batch.run_system_loglik(self.lik, out=self.loglik)


class SurrogateInputMap:
    """Which rows of the (15, n) physical inputs a chained surrogate reads and how they become its normalised coordinates; which
    rows it holds fixed.  Built and checked on the host (`surrogate_input_map`); `coords` is the numpy form of the map."""

    def __init__(self, rows, is_log, a, b, fixed_rows, fixed_vals):
        self.rows = np.asarray(rows, dtype=np.int64)                 # COUPLED_INPUTS rows of the surrogate's varied inputs, in its order
        self.is_log = np.asarray(is_log, dtype=bool)
        self.a, self.b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        self.fixed_rows = np.asarray(fixed_rows, dtype=np.int64)
        self.fixed_vals = np.asarray(fixed_vals, dtype=np.float64)

    def coords(self, x):
        """x: (15, n) physical inputs -> (n_ext, n) coordinates, the expression of `PemV0System._external_coords`: log10 for
        the log-uniform variables, then 2.0 * (u - a) / (b - a) - 1.0 left to right"""
        x = np.asarray(x, dtype=np.float64)
        t = np.empty((len(self.rows), x.shape[1]))
        for d, r in enumerate(self.rows):
            u = np.log10(x[r]) if self.is_log[d] else x[r]
            t[d] = 2.0 * (u - self.a[d]) / (self.b[d] - self.a[d]) - 1.0
        return t


def surrogate_input_map(theta_names, operating, varied, fixed, priors, qois=(), field: bool = True, uion: bool = False):
    """The input map of a posterior evaluated through a chained surrogate (`chain.ChainedSurrogate`: its `varied`, `fixed`,
    `priors`, whether it carries the j_ion latents (`field`) and the u_ion latents (`uion`)) for the calibrated `theta_names`, the
    (Ne, 3) `operating` rows of P_b, V_a, mdot_a and the measured `qois`.  Runs without a device.  ValueError for what the
    surrogate cannot serve."""
    varied, fixed = tuple(varied), dict(fixed)
    for k in theta_names:
        if k in fixed:
            raise ValueError(f"'{k}' cannot be calibrated: the surrogate holds it fixed at {fixed[k]}")
        if k not in varied:
            raise ValueError(f"'{k}' cannot be calibrated: the surrogate does not know it (its varied inputs are {varied})")
    if 'uion' in qois and not uion:
        raise ValueError("the likelihood holds 'uion' records: the chain carries no u_ion latents yet (the thruster stage predicts "
                         "I_B0 and T only)")
    if 'jion' in qois and not field:
        raise ValueError("the likelihood holds 'jion' records and the surrogate was built with field=False: it carries no j_ion latents")
    op = np.atleast_2d(np.asarray(operating, dtype=np.float64))
    for j, k in enumerate(OPERATING):
        v = op[:, j]
        if k in fixed:
            if not np.all(v == fixed[k]):
                raise ValueError(f"the surrogate holds the operating input '{k}' fixed at {fixed[k]}; conditions ask for "
                                 f"{v[v != fixed[k]]}")
        elif k in varied:
            p = priors[k]
            if p.kind == NORMAL:
                raise ValueError(f"'{k}': a surrogate's box is uniform or log-uniform")
            with np.errstate(divide='ignore', invalid='ignore'):
                u = np.log10(v) if p.kind == LOGUNIFORM else v
            out = ~((u >= p.a) & (u <= p.b))
            if out.any():
                lo, hi = (10.0 ** p.a, 10.0 ** p.b) if p.kind == LOGUNIFORM else (p.a, p.b)
                raise ValueError(f"operating values of '{k}' outside the surrogate's box [{lo}, {hi}]: {v[out]}")
        else:
            raise ValueError(f"the surrogate neither varies nor fixes the operating input '{k}'")
    for k in varied:
        if priors[k].kind == NORMAL:
            raise ValueError(f"'{k}': a surrogate's box is uniform or log-uniform")
    fx = [k for k in COUPLED_INPUTS if k in fixed]
    return SurrogateInputMap([COUPLED_INPUTS.index(k) for k in varied], [priors[k].kind == LOGUNIFORM for k in varied],
                             [priors[k].a for k in varied], [priors[k].b for k in varied],
                             [COUPLED_INPUTS.index(k) for k in fx], [float(fixed[k]) for k in fx])


class SurrogatePosterior(BatchedPosterior):
    def __init__(self, theta_names, likelihood: SystemLikelihood, surrogate, n_chains: int, n_nuisance: int = 100, seed: int = 0,
                 discharge=(4.5, 0.2), fresh_nuisance: bool = True, shared_nuisance: bool = False):
        """`SystemPosterior` with a trained `chain.ChainedSurrogate` in the model's place, as the reference calibrates
        (mcmc.py:57-106: `SURR.predict`, `jion_reconstruct`, I_D from the surrogate's output).  The interface of
        `SystemPosterior`.  The priors are the surrogate's (its coordinates are defined over them); inputs it holds fixed are
        written as constants; every other varied input that is neither calibrated nor operating is a nuisance draw.  One
        evaluation: the physical inputs assembled as in `BatchedPosterior`, the surrogate's rows mapped to coordinates on the
        device, ONE `pem_chain_system_loglik_f64_dev` (chain, j_ion nodes, Gaussian sums and the discharge term from the
        surrogate's I_B0), then `pem_loglik_marginal_f64_dev` without a discharge term of its own.  `likelihood` may hold V_cc, T
        and jion records, and uion records when the surrogate was built with `u_ion` (the launch is then
        `pem_chain_fields_loglik_f64_dev`: all four quantities of `QOI_MAP['System']`); otherwise uion is refused
        (`surrogate_input_map`)."""
        import torch
        if len(likelihood.sweep_radii) > 1:
            raise ValueError(f'the likelihood holds j_ion at several sweep radii {likelihood.sweep_radii}: the plume surrogate is '
                             f'trained at one radius')
        if not likelihood.use_discharge:
            discharge = None
        self.surrogate = surrogate
        self.map = surrogate_input_map(theta_names, likelihood.operating, surrogate.varied, surrogate.fixed, surrogate.priors,
                                       likelihood.qois, field=surrogate.field is not None,
                                       uion=getattr(surrogate, 'u_compression', None) is not None)
        if likelihood.device != surrogate.device:
            raise ValueError(f'the likelihood lives on {likelihood.device}, the surrogate on {surrogate.device}')
        self._setup(theta_names, likelihood.operating, lambda: likelihood, n_chains, n_nuisance, surrogate.priors, seed, None,
                    likelihood.sweep_radius, fresh_nuisance, shared_nuisance)
        self.chain_discharge = None if discharge is None else (float(discharge[0]), float(discharge[1]))   # added by the launch
        dev = lambda a, **kw: torch.as_tensor(a, device=self.device, **kw)                                   # noqa: E731
        m = self.map
        self._lin_src, self._log_src = dev(m.rows[~m.is_log]), dev(m.rows[m.is_log])
        self._lin_dst, self._log_dst = dev(np.nonzero(~m.is_log)[0]), dev(np.nonzero(m.is_log)[0])
        self._ca, self._cw = dev(m.a)[:, None], dev(m.b)[:, None] - dev(m.a)[:, None]        # the width divides as a device tensor
        self._fixed_idx = dev(m.fixed_rows)
        self._fixed_vals = dev(m.fixed_vals)[:, None]
        self._u = torch.empty((len(m.rows), self.n), dtype=torch.float64, device=self.device)
        self.coords = torch.empty_like(self._u)                                                # the last evaluation's coordinates
        self._a1_row = COUPLED_INPUTS.index('a_1')

    def assemble_inputs(self, theta):
        """`BatchedPosterior.assemble_inputs`, then the inputs the surrogate holds fixed as constants, then its coordinates:
        log10 for the log-uniform rows and 2.0 * (u - a) / (b - a) - 1.0 left to right (`PemV0System._external_coords`)"""
        import torch
        super().assemble_inputs(theta)
        x = self.batch.inputs
        if self._fixed_idx.numel():
            x.index_copy_(0, self._fixed_idx, self._fixed_vals.expand(-1, self.n))
        if self._lin_src.numel():
            self._u.index_copy_(0, self._lin_dst, x.index_select(0, self._lin_src))
        if self._log_src.numel():
            self._u.index_copy_(0, self._log_dst, torch.log10(x.index_select(0, self._log_src)))
        torch.sub(2.0 * (self._u - self._ca) / self._cw, 1.0, out=self.coords)

    def _run_loglik(self, pred=None):
        d = self.chain_discharge
        self.surrogate.run_system_loglik(self.coords, self.lik, a_1=self.batch.inputs[self._a1_row] if d else None, discharge=d,
                                         out=self.loglik, pred=pred)

    def record_predictions(self, theta):
        """(K M, n_rec) model values of the surrogate at every record of the table for theta (K, n_theta): row k M + m holds
        draw m of chain k, conditions side by side as in `SystemLikelihood.rec`; padding records are NaN.  The nuisance draws
        are those of the next evaluation and are not used up."""
        import torch
        assert theta.shape == (self.K, len(self.names)) and theta.dtype == torch.float64 and theta.device == self.device
        pred = torch.full((self.K * self.M, self.lik.n_rec), math.nan, dtype=torch.float64, device=self.device)
        fresh, self.fresh = self.fresh, False
        self.assemble_inputs(theta)
        self.fresh = fresh
        self._run_loglik(pred=pred)
        return pred


def capture_graph(body, device, warmup: int = 2, generator=None):
    """Run `body` (libpem_hip launches and torch ops on the current stream) `warmup` times on a side stream, then
    record it once into a torch.cuda.CUDAGraph (a hipGraph).  A non-default torch `generator` that `body` draws from is
    registered with the graph so that every replay advances its Philox offset.  Returns (graph, body's return value =
    static output)."""
    import torch
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(warmup):
            body()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    if generator is not None:
        graph.register_generator_state(generator)
    with torch.cuda.graph(graph):
        out = body()
    return graph, out


class Metropolis:
    """K independent random-walk Metropolis chains advanced together, one hipGraph replay per step.

    A stand-in for the delayed-rejection adaptive Metropolis of the reference (`mcmciterators`, third-party, absent;
    call site mcmc.py:283-300): same role -- draw from `log_posterior` -- simplest valid kernel.  Proposal:
    theta' = theta + scale * N(0, I) with a per-parameter `scale`; the nuisance draws inside the posterior are the
    recorded ones (common random numbers), i.e. the chain targets the M-sample marginal likelihood estimate."""

    def __init__(self, posterior: BatchedPosterior, theta0, scale, seed: int = 0, use_graph: bool = True):
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
    `.log_posterior`, or a closed
    form on the CPU in the tests).  Both stages are evaluated for all chains every step (a fixed launch sequence: with
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


class DeviceDRAM:
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
        if isinstance(theta0, torch.Tensor):
            if device is None:
                device = theta0.device
            theta0 = theta0.detach().cpu().numpy()
        t0 = np.atleast_1d(np.asarray(theta0, dtype=np.float64))
        if t0.ndim == 1:
            t0 = np.broadcast_to(t0, (int(n_chains or 1), t0.size))
        if t0.ndim != 2 or t0.shape[0] < 1:
            raise ValueError('theta0 must be (d,) or (K, d)')
        self.K, self.d = t0.shape
        if not 1 <= self.d <= _lib.DRAM_MAX_DIM:
            raise ValueError(f'DeviceDRAM samples 1 to {_lib.DRAM_MAX_DIM} parameters (got {self.d})')
        if device is not None and torch.device(device).type != 'cuda':
            raise ValueError(f"DeviceDRAM runs on the GPU only (got device '{device}'): use DRAM for CPU tensors")
        if not gamma > 0.0 or eps < 0.0 or int(adapt_interval) < 1 or int(adapt_after) < 0:
            raise ValueError('need gamma > 0, eps >= 0, adapt_interval >= 1 and adapt_after >= 0')
        c0 = np.eye(self.d) if cov0 is None else np.asarray(cov0, dtype=np.float64)
        if c0.ndim == 1:
            c0 = np.diag(c0)
        if c0.shape != (self.d, self.d):
            raise ValueError(f'cov0 must be ({self.d},) or ({self.d}, {self.d})')
        self.f, self.seed, self.use_graph = log_posterior, int(seed), bool(use_graph)
        self.adapt_after, self.adapt_interval, self.eps, self.gamma = int(adapt_after), int(adapt_interval), float(eps), float(gamma)
        dev = self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        K, d = self.K, self.d
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)                # noqa: E731
        self.theta = torch.as_tensor(np.ascontiguousarray(t0), device=dev).clone()
        self.L = torch.linalg.cholesky(torch.as_tensor(c0, device=dev)).expand(K, d, d).contiguous()
        self.mean, self.scatter = self.theta.clone(), z(K, d, d)                             # running moments of the chain
        self.prop, self.prop_logp = z(2, K, d), z(2, K)
        self.state, self.accepted, self.flags = z(K, dt=torch.int64), z(2, K, dt=torch.int64), z(K, dt=torch.int32)
        self.steps = 0
        self._trace = self._logp_trace = None
        self._window = (0, 0, 1)                                                             # trace_first, trace_len, thin
        self._graph, self._graph_key = None, None
        self.prop.copy_(self.theta.expand(2, K, d))
        self.logp = self.f(self.prop.view(2 * K, d))[:K].clone()
        self._launch()                                                                       # launch 0: the proposals of step 1

    def _launch(self):
        import torch
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                    # noqa: E731
        first, length, thin = self._window
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_dram_step_f64_dev(
                self.K, self.d, self.seed, self.gamma, self.eps, self.adapt_after, self.adapt_interval, first, length, thin,
                p(self.theta), p(self.logp), p(self.L), p(self.mean), p(self.scatter), p(self.prop), p(self.prop_logp),
                p(self.state), p(self.accepted), p(self.flags), p(self._trace), p(self._logp_trace), None,
                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _step(self):
        self.prop_logp.view(-1).copy_(self.f(self.prop.view(2 * self.K, self.d)))
        self._launch()

    def _prepare(self):
        """the graph is (re)recorded when a trace buffer or the trace window moves: a recorded launch carries them by value.
        The steps that recording runs are undone."""
        key = (self._trace.data_ptr() if self._trace is not None else 0,
               self._logp_trace.data_ptr() if self._logp_trace is not None else 0) + self._window
        if not self.use_graph or (self._graph is not None and self._graph_key == key):
            return
        kept = (self.theta, self.logp, self.L, self.mean, self.scatter, self.prop, self.prop_logp, self.state, self.accepted,
                self.flags)
        saved = [t.clone() for t in kept]
        self._graph = None                                                                   # (frees the old recording first)
        self._graph, _ = capture_graph(self._step, self.device)
        self._graph_key = key
        for t, s in zip(kept, saved):
            t.copy_(s)

    def run(self, n_steps: int, keep: bool = True, thin: int = 1, keep_logp: bool = False):
        """Advance every chain n_steps.  Returns the (ceil(n_steps / thin), K, d) trace as a device tensor if `keep` -- steps
        1, 1 + thin, ... of this call -- and with `keep_logp` the pair (trace, logp trace (ceil(n_steps / thin), K))."""
        import torch
        n_steps, thin = int(n_steps), int(thin)
        if n_steps < 0 or thin < 1:
            raise ValueError('n_steps >= 0 and thin >= 1')
        rows = -(-n_steps // thin)
        new = lambda *s: torch.empty(s, dtype=torch.float64, device=self.device)              # noqa: E731
        self._trace = new(rows, self.K, self.d) if keep and rows else None
        self._logp_trace = new(rows, self.K) if keep and keep_logp and rows else None
        self._window = (self.steps, rows, thin) if self._trace is not None else (0, 0, 1)
        if n_steps:
            self._prepare()
        for _ in range(n_steps):
            if self.use_graph:
                self._graph.replay()
            else:
                self._step()
        self.steps += n_steps
        trace, logp_trace = self._trace, self._logp_trace
        if keep and trace is None:
            trace = new(0, self.K, self.d)
            logp_trace = new(0, self.K) if keep_logp else None
        self._trace = self._logp_trace = None
        self._window = (0, 0, 1)
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


class DeviceEnsemble:
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
        if isinstance(theta0, torch.Tensor):
            if device is None:
                device = theta0.device
            theta0 = theta0.detach().cpu().numpy()
        t0 = np.asarray(theta0, dtype=np.float64)
        if t0.ndim == 2 and int(n_ensembles) == 1:
            t0 = t0[None]
        if t0.ndim != 3 or (int(n_ensembles) not in (1, t0.shape[0])):
            raise ValueError('theta0 must be (K, d) with n_ensembles == 1, or (E, K, d)')
        self.E, self.K, self.d = t0.shape
        if not 1 <= self.d <= _lib.ENSEMBLE_MAX_DIM:
            raise ValueError(f'DeviceEnsemble samples 1 to {_lib.ENSEMBLE_MAX_DIM} parameters (got {self.d})')
        if self.E < 1 or self.K % 2 or self.K < 2 * self.d or self.K > _lib.ENSEMBLE_MAX_WALKERS:
            raise ValueError(f'DeviceEnsemble needs an even number of walkers K with 2 d = {2 * self.d} <= K <= '
                             f'{_lib.ENSEMBLE_MAX_WALKERS} per ensemble (got {self.K})')
        if device is not None and torch.device(device).type != 'cuda':
            raise ValueError(f"DeviceEnsemble runs on the GPU only (got device '{device}')")
        g0 = 2.38 / math.sqrt(2.0 * self.d) if g0 is None else float(g0)
        if not (0.0 <= de_fraction <= 1.0):
            raise ValueError(f'de_fraction must be in [0, 1] (got {de_fraction})')
        if de_fraction > 0.0 and self.K < 4:
            raise ValueError('the DE move needs two partners in the other half: K >= 4')
        if not (a > 1.0 and math.isfinite(a) and g0 > 0.0 and math.isfinite(g0) and sigma >= 0.0 and math.isfinite(sigma)):
            raise ValueError('need finite a > 1, g0 > 0 and sigma >= 0')
        self.f, self.seed, self.use_graph = log_posterior, int(seed), bool(use_graph)
        self.a, self.de_fraction, self.g0, self.sigma = float(a), float(de_fraction), g0, float(sigma)
        dev = self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        E, K, d = self.E, self.K, self.d
        H = self.H = K // 2
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)                # noqa: E731
        self.theta = torch.as_tensor(np.ascontiguousarray(t0), device=dev).clone()
        self.prop, self.prop_logp, self.log_q = z(E, H, d), z(E, H), z(E, H)
        self.state, self.accepted = z(E, dt=torch.int64), z(E, K, dt=torch.int64)
        self.steps = 0
        self._trace = self._logp_trace = None
        self._window = (0, 0, 1)                                                             # trace_first, trace_len, thin
        self._graph, self._graph_key = None, None
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
        center = np.atleast_1d(np.asarray(center, dtype=np.float64))
        rng = np.random.default_rng(seed)
        return center + np.asarray(scale, dtype=np.float64) * rng.standard_normal((int(n_ensembles), int(n_walkers), center.size))

    def _launch(self):
        import torch
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                    # noqa: E731
        first, length, thin = self._window
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_ensemble_step_f64_dev(
                self.E, self.K, self.d, self.seed, self.a, self.de_fraction, self.g0, self.sigma, first, length, thin,
                p(self.theta), p(self.logp), p(self.prop), p(self.prop_logp), p(self.log_q), p(self.state), p(self.accepted),
                p(self._trace), p(self._logp_trace), None, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _step(self):
        for _ in range(2):
            self.prop_logp.view(-1).copy_(self.f(self.prop.view(self.E * self.H, self.d)))
            self._launch()

    def _prepare(self):
        """the graph is (re)recorded when a trace buffer or the trace window moves: a recorded launch carries them by value.
        The steps that recording runs are undone."""
        key = (self._trace.data_ptr() if self._trace is not None else 0,
               self._logp_trace.data_ptr() if self._logp_trace is not None else 0) + self._window
        if not self.use_graph or (self._graph is not None and self._graph_key == key):
            return
        kept = (self.theta, self.logp, self.prop, self.prop_logp, self.log_q, self.state, self.accepted)
        saved = [t.clone() for t in kept]
        self._graph = None                                                                   # (frees the old recording first)
        self._graph, _ = capture_graph(self._step, self.device)
        self._graph_key = key
        for t, s in zip(kept, saved):
            t.copy_(s)

    def run(self, n_steps: int, keep: bool = True, thin: int = 1, keep_logp: bool = False):
        """Advance every ensemble n_steps whole steps (each walker is proposed to once per step).  Returns the
        (ceil(n_steps / thin), E, K, d) trace as a device tensor if `keep` -- steps 1, 1 + thin, ... of this call -- and with
        `keep_logp` the pair (trace, logp trace (ceil(n_steps / thin), E, K))."""
        import torch
        n_steps, thin = int(n_steps), int(thin)
        if n_steps < 0 or thin < 1:
            raise ValueError('n_steps >= 0 and thin >= 1')
        rows = -(-n_steps // thin)
        new = lambda *s: torch.empty(s, dtype=torch.float64, device=self.device)              # noqa: E731
        self._trace = new(rows, self.E, self.K, self.d) if keep and rows else None
        self._logp_trace = new(rows, self.E, self.K) if keep and keep_logp and rows else None
        self._window = (self.steps, rows, thin) if self._trace is not None else (0, 0, 1)
        if n_steps:
            self._prepare()
        for _ in range(n_steps):
            if self.use_graph:
                self._graph.replay()
            else:
                self._step()
        self.steps += n_steps
        trace, logp_trace = self._trace, self._logp_trace
        if keep and trace is None:
            trace = new(0, self.E, self.K, self.d)
            logp_trace = new(0, self.E, self.K) if keep_logp else None
        self._trace = self._logp_trace = None
        self._window = (0, 0, 1)
        if not keep:
            return None
        return (trace, logp_trace) if keep_logp else trace

    @property
    def acceptance(self):
        """(E, K): fraction of its proposals each walker accepted"""
        return self.accepted.double() / max(1, self.steps)


class DeviceTemperedEnsemble:
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
        if isinstance(theta0, torch.Tensor):
            if device is None:
                device = theta0.device
            theta0 = theta0.detach().cpu().numpy()
        self.betas = self.ladder(n_temperatures, beta_min, include_prior) if betas is None else self.check_ladder(betas)
        T, R = self.betas.size, int(n_replicas)
        t0 = np.asarray(theta0, dtype=np.float64)
        if R < 1 or t0.ndim not in (2, 3, 4) or (t0.ndim >= 3 and t0.shape[-3] != T) or (t0.ndim == 4 and t0.shape[0] != R):
            raise ValueError(f'theta0 must be (K, d), (T, K, d) or (R, T, K, d) with T = {T} temperatures and R = n_replicas = {R} '
                             f'(got {t0.shape})')
        t0 = np.array(np.broadcast_to(t0, (R, T) + t0.shape[-2:]))
        self.R, self.T, self.K, self.d = t0.shape
        self.E = self.R * self.T
        if not 1 <= self.d <= _lib.ENSEMBLE_MAX_DIM:
            raise ValueError(f'DeviceTemperedEnsemble samples 1 to {_lib.ENSEMBLE_MAX_DIM} parameters (got {self.d})')
        if self.K % 2 or self.K < 2 * self.d or self.K > _lib.ENSEMBLE_MAX_WALKERS:
            raise ValueError(f'DeviceTemperedEnsemble needs an even number of walkers K with 2 d = {2 * self.d} <= K <= '
                             f'{_lib.ENSEMBLE_MAX_WALKERS} per ensemble (got {self.K})')
        if not np.isfinite(t0).all():
            bad = int((~np.isfinite(t0).all(axis=-1)).sum())
            raise ValueError(f'{bad} of the {self.E * self.K} starts have a coordinate that is not finite')
        if device is not None and torch.device(device).type != 'cuda':
            raise ValueError(f"DeviceTemperedEnsemble runs on the GPU only (got device '{device}')")
        g0 = 2.38 / math.sqrt(2.0 * self.d) if g0 is None else float(g0)
        if not (0.0 <= de_fraction <= 1.0):
            raise ValueError(f'de_fraction must be in [0, 1] (got {de_fraction})')
        if de_fraction > 0.0 and self.K < 4:
            raise ValueError('the DE move needs two partners in the other half: K >= 4')
        if not (a > 1.0 and math.isfinite(a) and g0 > 0.0 and math.isfinite(g0) and sigma >= 0.0 and math.isfinite(sigma)):
            raise ValueError('need finite a > 1, g0 > 0 and sigma >= 0')
        self.f_lik, self.f_prior, self.seed, self.use_graph = log_likelihood, log_prior, int(seed), bool(use_graph)
        self.a, self.de_fraction, self.g0, self.sigma = float(a), float(de_fraction), g0, float(sigma)
        dev = self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        E, K, d = self.E, self.K, self.d
        H = self.H = K // 2
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)                # noqa: E731
        self._beta = torch.as_tensor(self.betas, device=dev).clone()
        self.theta = torch.as_tensor(np.ascontiguousarray(t0.reshape(E, K, d)), device=dev).clone()
        self.prop, self.prop_loglik, self.prop_logprior, self.log_q = z(E, H, d), z(E, H), z(E, H), z(E, H)
        self.state, self.accepted = z(R, dt=torch.int64), z(E, K, dt=torch.int64)
        self.swap_attempts, self.swap_accepted = z(R, T - 1, dt=torch.int64), z(R, T - 1, dt=torch.int64)
        self.steps = 0
        self.trace = self.loglik_trace = self.logprior_trace = None                          # of the last kept run
        self._traces = (None, None, None)
        self._window = (0, 0, 1)                                                             # trace_first, trace_len, thin
        self._graph, self._graph_key = None, None
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
        center = np.atleast_1d(np.asarray(center, dtype=np.float64))
        rng = np.random.default_rng(seed)
        return center + np.asarray(scale, dtype=np.float64) * rng.standard_normal((int(n_replicas), int(n_temperatures),
                                                                                   int(n_walkers), center.size))

    def _launch(self):
        import torch
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                    # noqa: E731
        first, length, thin = self._window
        swaps = (p(self.swap_attempts), p(self.swap_accepted)) if self.T > 1 else (None, None)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_tempered_ensemble_step_f64_dev(
                self.R, self.T, self.K, self.d, self.seed, self.a, self.de_fraction, self.g0, self.sigma, p(self._beta), first, length,
                thin, p(self.theta), p(self.loglik), p(self.logprior), p(self.prop), p(self.prop_loglik), p(self.prop_logprior),
                p(self.log_q), p(self.state), p(self.accepted), *swaps, *[p(t) for t in self._traces], None,
                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _step(self):
        for _ in range(2):
            flat = self.prop.view(self.E * self.H, self.d)
            self.prop_loglik.view(-1).copy_(self.f_lik(flat))
            self.prop_logprior.view(-1).copy_(self.f_prior(flat))
            self._launch()

    def _prepare(self):
        """the graph is (re)recorded when a trace buffer or the trace window moves: a recorded launch carries them by value.
        The steps that recording runs are undone."""
        key = tuple(t.data_ptr() if t is not None else 0 for t in self._traces) + self._window
        if not self.use_graph or (self._graph is not None and self._graph_key == key):
            return
        kept = (self.theta, self.loglik, self.logprior, self.prop, self.prop_loglik, self.prop_logprior, self.log_q, self.state,
                self.accepted, self.swap_attempts, self.swap_accepted)
        saved = [t.clone() for t in kept]
        self._graph = None                                                                   # (frees the old recording first)
        self._graph, _ = capture_graph(self._step, self.device)
        self._graph_key = key
        for t, s in zip(kept, saved):
            t.copy_(s)

    def run(self, n_steps: int, keep: bool = True, thin: int = 1):
        """Advance every ensemble n_steps whole steps (two half-steps and the swaps that are due).  Returns the
        (ceil(n_steps / thin), R, T, K, d) trace as a device tensor if `keep` -- steps 1, 1 + thin, ... of this call, each as the
        swaps left it -- and keeps it with its (rows, R, T, K) log likelihoods and log priors as `trace`, `loglik_trace`,
        `logprior_trace` for `cold`, `mean_loglik` and `log_evidence`."""
        import torch
        n_steps, thin = int(n_steps), int(thin)
        if n_steps < 0 or thin < 1:
            raise ValueError('n_steps >= 0 and thin >= 1')
        rows = -(-n_steps // thin)
        E, K, d = self.E, self.K, self.d
        new = lambda *s: torch.empty(s, dtype=torch.float64, device=self.device)              # noqa: E731
        self._traces = (new(rows, E, K, d), new(rows, E, K), new(rows, E, K)) if keep and rows else (None, None, None)
        self._window = (self.steps, rows, thin) if self._traces[0] is not None else (0, 0, 1)
        if n_steps:
            self._prepare()
        for _ in range(n_steps):
            if self.use_graph:
                self._graph.replay()
            else:
                self._step()
        self.steps += n_steps
        traces = self._traces if self._traces[0] is not None or not keep else (new(0, E, K, d), new(0, E, K), new(0, E, K))
        self._traces = (None, None, None)
        self._window = (0, 0, 1)
        if not keep:
            self.trace = self.loglik_trace = self.logprior_trace = None
            return None
        shape = (traces[0].shape[0], self.R, self.T, K)
        self.trace, self.loglik_trace, self.logprior_trace = traces[0].view(*shape, d), traces[1].view(shape), traces[2].view(shape)
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


class DeviceSMC:
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
        if isinstance(theta0, torch.Tensor):
            if device is None:
                device = theta0.device
            theta0 = theta0.detach().cpu().numpy()
        t0 = np.asarray(theta0, dtype=np.float64)
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
        if device is not None and torch.device(device).type != 'cuda':
            raise ValueError(f"DeviceSMC runs on the GPU only (got device '{device}')")
        self.f_lik, self.f_prior, self.seed, self.use_graph = log_likelihood, log_prior, int(seed), bool(use_graph)
        self.tau, self.n_mcmc, self.scale, self.eps = float(tau), int(n_mcmc), scale, float(eps)
        dev = self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        R, N, d = self.R, self.N, self.d
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)                # noqa: E731
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
        self._graph = None

    @staticmethod
    def prior_draws(names, priors=None, n_particles: int = 1024, n_populations: int = 1, seed: int = 0, method: str = 'sobol',
                    device=None):
        """(n_populations, n_particles, len(names)) draws of `names` from their priors (None: PEM_V0_PRIORS) as a device tensor,
        through `sampling.Design`: population r is points 0 ... n_particles - 1 of the design with (seed, stream = r) -- for
        'sobol' a Sobol' set with its own random digital shift per population, for 'mc' independent draws."""
        import torch
        if method not in ('sobol', 'mc'):
            raise ValueError(f"method must be 'sobol' or 'mc' (got '{method}')")
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        out = torch.empty((int(n_populations), len(names), int(n_particles)), dtype=torch.float64, device=dev)
        for r in range(int(n_populations)):
            Design(priors=priors, names=names, seed=seed, stream=r).fill(out[r], method=method)
        return out.transpose(1, 2).contiguous()

    def _args(self):
        return (self.R, self.N, self.d, self.seed, self.tau, self.scale, self.eps, self.n_mcmc)

    def _launch_stage(self, record=None):
        import torch
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                    # noqa: E731
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_smc_stage_f64_dev(
                *self._args(), p(self.theta), p(self.loglik), p(self.logprior), p(self.beta), p(self.log_evidence), p(self.stage),
                p(self.L), p(self.prop), p(self.accept_count), p(self.accepted), p(self.flags), p(self.moves_active), p(self.scratch),
                *[p(h) for h in self._hist], self._hist.shape[2], p(record),
                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _launch_move(self, move: int, propose: bool, record=None):
        import torch
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                    # noqa: E731
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_smc_move_f64_dev(
                *self._args(), int(move), 1 if propose else 0, p(self.theta), p(self.loglik), p(self.logprior), p(self.beta),
                p(self.stage), p(self.L), p(self.prop), p(self.prop_loglik), p(self.prop_logprior), p(self.accept_count),
                p(self.moves_active), p(record), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _stage(self):
        self._launch_stage()
        flat = self.prop.view(self.R * self.N, self.d)
        for m in range(1, self.n_mcmc + 1):
            self.prop_loglik.view(-1).copy_(self.f_lik(flat))
            self.prop_logprior.view(-1).copy_(self.f_prior(flat))
            self._launch_move(m, m < self.n_mcmc)

    def _state(self):
        return (self.theta, self.loglik, self.logprior, self.beta, self.log_evidence, self.stage, self.L, self.prop, self.prop_loglik,
                self.prop_logprior, self.accept_count, self.accepted, self.flags, self.moves_active, self.scratch, self._hist)

    def _prepare(self, history_len: int):
        """the history arrays grow to hold every stage of this run; a recorded launch carries them by value, so the graph is
        recorded again when they move.  The stages that recording runs are undone."""
        import torch
        if self._hist is None or self._hist.shape[2] < history_len:
            hist = torch.zeros((4, self.R, history_len), dtype=torch.float64, device=self.device)
            if self._hist is not None:
                hist[:, :, :self._hist.shape[2]] = self._hist
            self._hist, self._graph = hist, None
        if not self.use_graph or self._graph is not None:
            return
        saved = [t.clone() for t in self._state()]
        self._graph, _ = capture_graph(self._stage, self.device)
        for t, s in zip(self._state(), saved):
            t.copy_(s)

    def run(self, max_stages: int = 200, check_every: int = 4):
        """Replay stages, reading beta and flags back once per `check_every` stages, until every population is at beta = 1, or
        flag bit 1 is up, or max_stages stages of this call have run.  The result does not depend on check_every: a finished
        population ignores the replays past its end.  Returns an `SMCResult`; a later call continues."""
        import torch
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
            for _ in range(min(check_every, max_stages - ran)):
                if self.use_graph:
                    self._graph.replay()
                else:
                    self._stage()
                ran += 1
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
