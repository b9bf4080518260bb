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

The samplers that draw from these posteriors (`Metropolis`, `DRAM`, `DeviceDRAM`, `DeviceEnsemble`, `DeviceTemperedEnsemble`,
`DeviceSMC`) take any callable and live in `samplers.py`; their names stay importable from here.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._device_loop import capture_graph
from .batch import CoupledBatch
from .likelihood import JionLikelihood, SystemLikelihood
from .models.coupled import COUPLED_INPUTS
from .samplers import DRAM, DeviceDRAM, DeviceEnsemble, DeviceSMC, DeviceTemperedEnsemble, Metropolis, SMCResult  # noqa: F401
from .sampling import LOGUNIFORM, NORMAL, PEM_V0_PRIORS, UNIFORM, Design, Prior

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


NOISE_PREFIX = 'noise_'
NOISE_DISCHARGE = 'I_D'                 # the name of the discharge-current term among the noise scales
NOISE_PRIOR = Prior(LOGUNIFORM, -1.0, 1.0, 'noise scale: s in [0.1, 10], density proportional to 1 / s')


def noise_scale_table(noise_scales, qois, has_discharge, priors=None):
    """The bookkeeping of `noise_scales` (DESIGN.md "Noise scales"), on the host: (scaled, merged) -- the scaled quantities in the
    order given and a copy of `priors` that also holds their priors under 'noise_<name>'.  `noise_scales`: a sequence of names from
    `qois` (and 'I_D' when the posterior has a discharge term of its own), or a dict {name: Prior}; the default prior is
    `NOISE_PRIOR`.  ValueError for an unknown or repeated name, a NORMAL prior and a prior whose support reaches 0 or below."""
    priors = PEM_V0_PRIORS if priors is None else priors
    if isinstance(noise_scales, str):
        noise_scales = (noise_scales,)
    given = dict(noise_scales) if isinstance(noise_scales, dict) else {k: NOISE_PRIOR for k in noise_scales}
    scaled = tuple(noise_scales)
    offered = tuple(qois) + ((NOISE_DISCHARGE,) if has_discharge else ())
    if not scaled:
        raise ValueError(f'noise_scales names at least one of {offered} (None: no noise scale)')
    merged = dict(priors)
    for i, k in enumerate(scaled):
        if k not in offered:
            raise ValueError(f'noise_scales: unknown name {k!r}; this posterior offers {offered}')
        if k in scaled[:i]:
            raise ValueError(f'noise_scales: {k!r} is given twice')
        p = given[k]
        if not isinstance(p, Prior):
            raise ValueError(f'noise_scales[{k!r}]: a sampling.Prior is needed, got {p!r}')
        if p.kind == NORMAL:
            raise ValueError(f'noise_scales[{k!r}]: a NORMAL prior puts mass on scales <= 0; use UNIFORM or LOGUNIFORM')
        if p.kind not in (UNIFORM, LOGUNIFORM) or not (math.isfinite(p.a) and math.isfinite(p.b) and p.b > p.a):
            raise ValueError(f'noise_scales[{k!r}]: a UNIFORM or LOGUNIFORM prior with finite a < b is needed, got {p!r}')
        if p.kind == UNIFORM and not p.a > 0.0:
            raise ValueError(f'noise_scales[{k!r}]: the support [{p.a}, {p.b}] reaches 0 or below; a scale is positive')
        merged[NOISE_PREFIX + k] = p
    return scaled, merged


def noise_groups(lik):
    """(qois, group_end int32, group_count float64) of a likelihood's table: one group of conditions per QoI in the order of
    `SystemLikelihood.conditions`, each with its number of measured records (`span`; padding records are not counted).  A
    `JionLikelihood` is one group."""
    if not hasattr(lik, 'conditions'):
        return ('jion',), np.asarray([lik.n_cond], dtype=np.int32), np.asarray([lik.n_cond * lik.n_ang], dtype=np.float64)
    span = lik.span.cpu().numpy()
    ends, counts, first = [], [], 0
    for q in lik.qois:
        sl = lik.conditions[q]
        if sl.start != first or sl.stop <= sl.start:
            raise ValueError(f'the conditions of {q!r} are {sl}: one contiguous ascending block per QoI is needed')
        first = sl.stop
        ends.append(sl.stop)
        counts.append(float(span[sl, :, 1].sum()))
    if first != lik.n_cond or len(ends) > _lib.NOISE_MAX_GROUPS:
        raise ValueError(f'{len(ends)} groups ending at {first}: at most PEM_NOISE_MAX_GROUPS = {_lib.NOISE_MAX_GROUPS} groups '
                         f'covering the {lik.n_cond} conditions')
    return tuple(lik.qois), np.asarray(ends, dtype=np.int32), np.asarray(counts, dtype=np.float64)


class BatchedPosterior:
    """What the posteriors of this module share: K chains x M nuisance draws x Ne operating conditions in one `CoupledBatch`,
    the prior on the device, marginalisation, graph capture.  A subclass builds its likelihood and runs it (`_run_loglik`).

    noise_scales (None, names or {name: Prior}; `noise_scale_table`): one multiplicative scale of the stated std per named measured
    quantity, sampled with theta.  `names` is then `model_names` followed by 'noise_<name>', `priors` holds their priors, every
    method takes the (K, d_model + d_noise) table and the marginalisation is `pem_loglik_marginal_scaled_f64_dev` reading the
    scales from theta itself.  None is the path without scales, launch for launch."""

    def _setup(self, theta_names, operating, make_likelihood, n_chains, n_nuisance, priors, seed, discharge, sweep_radius,
               fresh_nuisance, shared_nuisance=False, noise_scales=None, qois=('jion',)):
        import torch
        if shared_nuisance and fresh_nuisance:
            raise ValueError('shared_nuisance needs fresh_nuisance=False: shared draws are the same on every evaluation')
        self.model_names = tuple(theta_names)
        self.noise = None
        if noise_scales is not None:
            self.noise, priors = noise_scale_table(noise_scales, qois, discharge is not None, priors)
        self.names = self.model_names + tuple(NOISE_PREFIX + k for k in self.noise or ())
        for k in self.model_names:
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
        self.theta_rows = [COUPLED_INPUTS.index(k) for k in self.model_names]
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
        if self.noise is not None:      # the groups of the scaled marginal: host arrays, passed by value with every launch
            group_qois, self._group_end, self._group_count = noise_groups(self.lik)
            col = {k: len(self.model_names) + j for j, k in enumerate(self.noise)}
            self._scale_col = np.ascontiguousarray([col.get(q, -1) for q in group_qois], dtype=np.int32)
            self._discharge_col = col.get(NOISE_DISCHARGE, -1)
            self.noise_groups, self.noise_counts = group_qois, self._group_count      # the groups of chi and their record counts

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
        if self.noise is not None:      # the model reads its own columns; the scales are the marginal's
            theta = theta[:, :len(self.model_names)]
        x.index_copy_(0, self._theta_idx, theta.T[:, :, None, None].expand(-1, -1, self.M, self.Ne))

    def _marginal(self, log_prior, out, theta=None, ess=None, chi=None):
        import torch
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                                    # noqa: E731
        x = self.batch.inputs
        d = self.discharge
        with torch.cuda.device(self.device):
            if self.noise is None:
                _lib.check(_lib.load().pem_loglik_marginal_f64_dev(
                    self.K, self.M, self.Ne, p(self.loglik), p(x[COUPLED_INPUTS.index('mdot_a')]) if d else None,
                    p(x[COUPLED_INPUTS.index('a_1')]) if d else None, d[0] if d else 0.0, d[1] if d else 1.0, p(log_prior),
                    p(out), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
            else:                       # the scales are columns of theta itself: no gather, nothing extra in a captured graph
                ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                                # noqa: E731
                _lib.check(_lib.load().pem_loglik_marginal_scaled_f64_dev(
                    self.K, self.M, self.Ne, p(self.loglik), p(x[COUPLED_INPUTS.index('mdot_a')]) if d else None,
                    p(x[COUPLED_INPUTS.index('a_1')]) if d else None, d[0] if d else 0.0, d[1] if d else 1.0, p(log_prior),
                    len(self._group_end), ptr(self._group_end), ptr(self._group_count), p(theta), theta.shape[1], theta.stride(0),
                    ptr(self._scale_col), self._discharge_col, p(ess), p(chi), chi.stride(0) if chi is not None else 0, p(out),
                    C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    def log_likelihood(self, theta, out=None, diagnostics=False):
        """theta: (K, n_theta) float64 tensor on the device -> (K,) marginal log-likelihoods.  diagnostics (with noise_scales):
        (out, ess, chi) -- ess (K,) the effective number of nuisance draws behind each value, chi (K, n_groups + 1) the
        likelihood-weighted unscaled sum of each group of `noise_groups` and of the discharge term (its last column)."""
        import torch
        assert theta.shape == (self.K, len(self.names)) and theta.dtype == torch.float64 and theta.device == self.device
        if diagnostics and self.noise is None:
            raise ValueError('diagnostics come from the scaled marginal: build the posterior with noise_scales')
        theta = theta.contiguous() if self.noise is not None else theta
        self.assemble_inputs(theta)
        self._run_loglik()
        out = torch.empty_like(self._out) if out is None else out
        if not diagnostics:
            return self._marginal(None, out, theta)
        ess = torch.empty_like(self._out)
        chi = torch.empty((self.K, len(self._group_end) + 1), dtype=torch.float64, device=self.device)
        return self._marginal(None, out, theta, ess, chi), ess, chi

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
        theta = theta.contiguous() if self.noise is not None else theta
        self.log_prior(theta, out=self._lp)
        self.assemble_inputs(theta)
        self._run_loglik()
        return self._marginal(self._lp, torch.empty_like(self._out) if out is None else out, theta)

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
                 device=None, shared_nuisance: bool = False, noise_scales=None):
        """theta_names: calibrated inputs (subset of the 15 coupled inputs, not operating ones);
        operating: (Ne, 3) array of `P_b [Torr], V_a [V], mdot_a [kg/s]` per experiment;
        alpha, y, std: (Ne, Na) measurement angles [rad], current densities and standard deviations at `sweep_radius`;
        discharge: (I_d, sigma) of the extra discharge-current weight (mcmc.py:48-49,102-104) or None;
        fresh_nuisance: new nuisance draws on every evaluation (as the reference) -- inside a captured graph the
        draws are whatever was recorded (common random numbers);
        shared_nuisance: every row uses draws 0 .. M Ne - 1 of the design, so that a value depends on theta, seed, M and the
        data and not on the row or on K (what an optimizer or a finite-difference Hessian comparing rows needs); requires
        fresh_nuisance=False.  Otherwise row k uses draws k M Ne .. (k + 1) M Ne - 1;
        noise_scales: None, ('jion',), ('jion', 'I_D') or {name: Prior} (`BatchedPosterior`): all measurements are one group."""
        self._setup(theta_names, operating, lambda: JionLikelihood(alpha, y, std, device=device), n_chains, n_nuisance, priors,
                    seed, discharge, sweep_radius, fresh_nuisance, shared_nuisance, noise_scales, ('jion',))

    def _run_loglik(self):
        self.batch.run_loglik(self.lik, out=self.loglik)


class SystemPosterior(BatchedPosterior):
    def __init__(self, theta_names, likelihood: SystemLikelihood, n_chains: int, n_nuisance: int = 100, priors=None,
                 seed: int = 0, discharge=(4.5, 0.2), fresh_nuisance: bool = True, shared_nuisance: bool = False, noise_scales=None):
        """The posterior of the reference's `System` calibration (mcmc.py:28-130): V_cc, thrust, ion velocity and ion current
        density, each from its own dataset (`likelihood.SystemLikelihood`, whose conditions are the Ne operating conditions
        here), evaluated by ONE fused launch (`pem_coupled_system_loglik_f64_dev`) per evaluation.  The interface of
        `JionPosterior`; theta_names, n_chains, n_nuisance, priors, seed, fresh_nuisance, shared_nuisance as there.
        discharge: (I_d, sigma) of the discharge-current weight added for every condition, or None; dropped when the
        likelihood's component is 'Cathode' (mcmc.py:100-101).
        noise_scales: None, names from `likelihood.qois` (and 'I_D' while there is a discharge term) or {name: Prior}
        (`BatchedPosterior`): one group of conditions per QoI."""
        if not likelihood.use_discharge:
            discharge = None
        self._setup(theta_names, likelihood.operating, lambda: likelihood, n_chains, n_nuisance, priors, seed, discharge,
                    likelihood.sweep_radius, fresh_nuisance, shared_nuisance, noise_scales, likelihood.qois)

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
                 discharge=(4.5, 0.2), fresh_nuisance: bool = True, shared_nuisance: bool = False, noise_scales=None):
        """`SystemPosterior` with a trained `chain.ChainedSurrogate` in the model's place, as the reference calibrates
        (mcmc.py:57-106: `SURR.predict`, `jion_reconstruct`, I_D from the surrogate's output).  The interface of
        `SystemPosterior`.  The priors are the surrogate's (its coordinates are defined over them); inputs it holds fixed are
        written as constants; every other varied input that is neither calibrated nor operating is a nuisance draw.  One
        evaluation: the physical inputs assembled as in `BatchedPosterior`, the surrogate's rows mapped to coordinates on the
        device, ONE `pem_chain_system_loglik_f64_dev` (chain, j_ion nodes, Gaussian sums and the discharge term from the
        surrogate's I_B0), then `pem_loglik_marginal_f64_dev` without a discharge term of its own.  `likelihood` may hold V_cc, T
        and jion records, and uion records when the surrogate was built with `u_ion` (the launch is then
        `pem_chain_fields_loglik_f64_dev`: all four quantities of `QOI_MAP['System']`); otherwise uion is refused
        (`surrogate_input_map`).
        noise_scales: as `SystemPosterior`'s, with discharge=None only: this launch adds the discharge term into the per-sample
        sums, which are then not separable by quantity; 'I_D' is not offered."""
        import torch
        if len(likelihood.sweep_radii) > 1:
            raise ValueError(f'the likelihood holds j_ion at several sweep radii {likelihood.sweep_radii}: the plume surrogate is '
                             f'trained at one radius')
        if not likelihood.use_discharge:
            discharge = None
        if noise_scales is not None and discharge is not None:
            raise ValueError('noise_scales needs discharge=None here: the chained launch adds the discharge term into the per-sample '
                             'sums, so they cannot be scaled per quantity afterwards')
        self.surrogate = surrogate
        self.map = surrogate_input_map(theta_names, likelihood.operating, surrogate.varied, surrogate.fixed, surrogate.priors,
                                       likelihood.qois, field=surrogate.field is not None,
                                       uion=getattr(surrogate, 'u_compression', None) is not None)
        if likelihood.device != surrogate.device:
            raise ValueError(f'the likelihood lives on {likelihood.device}, the surrogate on {surrogate.device}')
        self._setup(theta_names, likelihood.operating, lambda: likelihood, n_chains, n_nuisance, surrogate.priors, seed, None,
                    likelihood.sweep_radius, fresh_nuisance, shared_nuisance, noise_scales, likelihood.qois)
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
