"""Posterior and prior predictive checks against the calibration data: the validation step of the reference,
scripts/pem_v0/monte_carlo.py.

    theta             a chain after a 10 % burn-in, steps x chains flattened (:42-46), drawn with replacement (posterior_sampler,
                      :48-53) -- or the prior (prior_sampler, :56-60)
    nuisance inputs   from their priors; operating inputs = each dataset's operating conditions (run_models, :63-300)
    predictions       the model at every measurement of every dataset: V_cc, thrust T, u_ion at the measured axial positions,
                      j_ion at the measured angles -- the values `SystemLikelihood` compares with the data
    bands             5 / 50 / 95 % of the predictions over the draws (np.percentile(..., axis=0), :363, :378), and 5 / 95 % of a
                      copy with Gaussian measurement noise, sigma = mean(sqrt(var_y)) of the dataset (:358-359, :377)
    relative L2       of every draw against the data (relative_l2, :303-305), reported as print_l2_error does (:308-336)

`Predictive.run` is a fixed number of launches whatever the number of datasets: the inputs (`pem_predictive_inputs_f64_dev`),
the predictions (`pem_coupled_system_predict_f64_dev`, JMODE 7 of the fused likelihood kernel: the j_ion profile stays in LDS),
one column gather that drops the table's padding records, optionally the noise (`pem_predictive_noise_f64_dev`), and one
`drivers.column_percentiles` over every column.  The reference's surrogate rows ("Surr-Data", "Surr-Model") and its discharge
current check are not restated: of the reference's three analyses on its trained surrogate, the calibration
(`calibration.SurrogatePosterior`) and the Sobol' study (`drivers.sobol_sweep(surrogate=)`) take a `chain.ChainedSurrogate`,
this one runs the model only.  The reference's driver layer is stale and third-party: parity UNPINNED; the predictions are
held to the oracle, the bands to numpy (tests/test_predictive.py).
"""
import ctypes as C

import numpy as np

from . import _lib, constants
from .calibration import OPERATING
from .drivers import column_percentiles
from .likelihood import _KIND, SystemLikelihood
from .models.coupled import COUPLED_INPUTS
from .sampling import PEM_V0_PRIORS, Design

PERCENTILES = (5.0, 50.0, 95.0)
THETA_STREAM_OFFSET = 2     # Philox stream of the theta index: the design's stream + 2 (stream + 1 is Saltelli's matrix B)
NOISE_STREAM_OFFSET = 3     # Philox stream of the measurement noise


def relative_l2(pred, targ):
    """monte_carlo.py:303-305: sqrt(mean((pred - targ)^2) / mean(targ^2)) over the last axis.  numpy arrays or torch tensors."""
    if isinstance(pred, np.ndarray) or not hasattr(pred, 'dim'):
        targ = np.atleast_1d(targ)
        return np.sqrt(np.mean((pred - targ) ** 2, axis=-1) / np.mean(targ ** 2, axis=-1))
    import torch
    targ = torch.as_tensor(targ, dtype=pred.dtype, device=pred.device)
    if targ.dim() == 0:
        targ = targ.reshape(1)
    return torch.sqrt(torch.mean((pred - targ) ** 2, dim=-1) / torch.mean(targ ** 2, dim=-1))


def flatten_chain(samples, burnin: float = 0.1):
    """monte_carlo.py:44-46: a trace (n_steps, n_chains, d) loses its first int(burnin n_steps) steps and is flattened to
    (-1, d); an (S, d) table is taken as it is (no burn-in).  numpy arrays or torch tensors; refuses an empty result."""
    if not 0.0 <= float(burnin) < 1.0:
        raise ValueError(f'burnin is a fraction of the steps in [0, 1), got {burnin}')
    if samples.ndim == 3:
        n_steps = samples.shape[0]
        samples = samples[int(burnin * n_steps):].reshape(-1, samples.shape[-1])
    elif samples.ndim != 2:
        raise ValueError(f'samples: an (n_steps, n_chains, d) trace or an (S, d) table, got shape {tuple(samples.shape)}')
    if samples.shape[0] < 1:
        raise ValueError('no samples are left after the burn-in')
    return samples


def l2_table(rows, noise):
    """print_l2_error's columns (monte_carlo.py:313-336) for `rows = {qoi: (rel_l2 prior, rel_l2 posterior)}`: mean, std and
    mean / noise level of each, prior against posterior, one row per QoI.  Returns the text."""
    lines = [f'{"Case":>20} {"Prior mu":>8} {"Prior s":>8} {"Prior r":>8} {"Post mu":>8} {"Post s":>8} {"Post r":>8}']
    for q, (e_prior, e_post) in rows.items():
        e_prior, e_post = (np.asarray(e.cpu() if hasattr(e, 'cpu') else e, dtype=np.float64) for e in (e_prior, e_post))
        r = float(noise[q])
        lines.append(f'{q:>20} {np.mean(e_prior):>8.3f} {np.std(e_prior):>8.3f} {np.mean(e_prior) / r:>8.3f} '
                     f'{np.mean(e_post):>8.3f} {np.std(e_post):>8.3f} {np.mean(e_post) / r:>8.3f}')
    return '\n'.join(lines)


class Predictive:
    """Predictive checks of a `likelihood.SystemLikelihood`'s datasets.

    :param likelihood: the measurement table (datasets, operating conditions, sweep radius, u_ion grid).
    :param theta_names: the calibrated inputs, the columns of the `samples` given to `run` (not operating inputs).
    :param priors: priors of every coupled input (default PEM_V0_PRIORS): the nuisance draws and the prior predictive.
    :param seed: seed of the counter-based design; theta indices and noise use streams THETA_STREAM_OFFSET / NOISE_STREAM_OFFSET.
    """

    def __init__(self, likelihood: SystemLikelihood, theta_names, priors=None, seed: int = 0):
        import torch
        self.names = tuple(theta_names)
        for k in self.names:                                   # as BatchedPosterior._setup
            if k not in COUPLED_INPUTS or k in OPERATING:
                raise KeyError(f"'{k}' is not a calibratable input of the coupled model")
        if len(set(self.names)) != len(self.names):
            raise ValueError(f'theta names repeat: {self.names}')
        self.lik = lik = likelihood
        self.priors = PEM_V0_PRIORS if priors is None else priors
        self.design = Design(priors=self.priors, seed=seed)
        self.device = dev = lik.device
        self.operating = torch.as_tensor(np.ascontiguousarray(lik.operating, dtype=np.float64), device=dev)   # (n_cond, 3)
        self._theta_rows = np.ascontiguousarray([COUPLED_INPUTS.index(k) for k in self.names], dtype=np.int32)
        # the measured records of the table in its order (padding dropped): QoI q is the column range views[q]
        span = lik.span.cpu().numpy()
        cols, sigma, y = [], [], []
        self.views = {}
        for q in lik.qois:
            sl, d = lik.conditions[q], lik.data[q]
            start = len(cols)
            for c in range(sl.start, sl.stop):
                first, count = span[c, _KIND[q]]
                cols += range(int(first), int(first) + int(count))
            yq = np.asarray(d['y'], dtype=np.float64)
            self.views[q] = (start, len(cols), yq.shape)
            sigma += [float(np.mean(np.sqrt(np.asarray(d['var_y'], dtype=np.float64))))] * (len(cols) - start)   # :358-359
            y.append(yq.reshape(-1))
        self.n_cols = len(cols)
        self.cols = torch.as_tensor(np.asarray(cols, dtype=np.int64), device=dev)
        self.sigma = torch.as_tensor(np.asarray(sigma, dtype=np.float64), device=dev)
        self.y = {q: torch.as_tensor(np.asarray(lik.data[q]['y'], dtype=np.float64), device=dev) for q in lik.qois}
        self.batch = None

    # ------------------------------------------------------------------------------------------------ launches
    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def theta_table(self, samples, burnin: float = 0.1):
        """The (S, n_theta) float64 device table `run` draws theta from (None for the prior predictive)."""
        import torch
        if samples is None:
            return None
        if samples.ndim not in (2, 3) or samples.shape[-1] != len(self.names):
            raise ValueError(f'samples must be (n_steps, n_chains, {len(self.names)}) or (S, {len(self.names)}) -- one column per '
                             f'theta name {self.names} -- got shape {tuple(samples.shape)}')
        flat = flatten_chain(samples, burnin)
        if flat.shape[0] >= 2 ** 32:
            raise ValueError('at most 2^32 - 1 posterior samples')
        return torch.as_tensor(flat, dtype=torch.float64).to(self.device).contiguous()

    def assemble_inputs(self, table, n_draws: int, first_index: int = 0):
        """[15][n_draws n_cond] inputs of the batch (`pem_predictive_inputs_f64_dev`): sample i = d n_cond + c is draw
        first_index + i of the design, with condition c's operating row and theta from `table` (kept from the prior if None)."""
        from .batch import CoupledBatch
        n = int(n_draws) * self.lik.n_cond
        if self.batch is None or self.batch.n != n:
            self.batch = CoupledBatch(n, device=self.device, profile=False, sweep_radius=self.lik.sweep_radius, thruster_qoi=False)
        x, ds = self.batch.inputs, self.design
        ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                           # noqa: E731
        with_theta = table is not None
        _lib.check(_lib.load().pem_predictive_inputs_f64_dev(
            n, self.lik.n_cond, int(first_index), ds.seed, ds.stream, ptr(ds.kind), ptr(ds.a), ptr(ds.b),
            C.c_void_p(self.operating.data_ptr()), C.c_void_p(table.data_ptr()) if with_theta else None,
            table.shape[0] if with_theta else 0, len(self.names), ptr(self._theta_rows), ds.stream + THETA_STREAM_OFFSET,
            C.c_void_p(x.data_ptr()), x.stride(0), self._stream()))
        return x

    def predict(self, n_draws: int, out=None):
        """(n_draws, n_rec) model values at every record of the table (`pem_coupled_system_predict_f64_dev`) for the batch's
        inputs; padding records are left as they are in `out`."""
        import torch
        if out is None:
            out = torch.empty((int(n_draws), max(self.lik.n_rec, 1)), dtype=torch.float64, device=self.device)
        self.batch.run_system_predict(self.lik, out)
        return out

    def add_noise(self, compact, first_row: int = 0):
        """compact (n_draws, n_cols) + N(0, sigma_q^2) per column (`pem_predictive_noise_f64_dev`, counter-based)."""
        import torch
        out = torch.empty_like(compact)
        _lib.check(_lib.load().pem_predictive_noise_f64_dev(
            compact.shape[0], compact.shape[1], C.c_void_p(compact.data_ptr()), compact.stride(0), C.c_void_p(self.sigma.data_ptr()),
            int(first_row), self.design.seed, self.design.stream + NOISE_STREAM_OFFSET, C.c_void_p(out.data_ptr()), out.stride(0),
            self._stream()))
        return out

    # ------------------------------------------------------------------------------------------------ driver
    def run(self, samples=None, n_draws: int = 1000, burnin: float = 0.1, noise: bool = False, first_index: int = 0):
        """Predictions at every dataset's conditions and locations for n_draws draws, their bands and relative L2 errors.

        :param samples: a trace (n_steps, n_chains, d) of `Metropolis.run` / `DRAM.run` (burn-in dropped, then flattened),
                        an (S, d) table of theta values, or None for the prior predictive.  Columns follow `theta_names`.
        :param first_index: the first design index; draw d of condition c uses index first_index + d n_cond + c.
        Returns {qoi: {'pred', 'bands', 'bands_noisy' (noise only), 'noisy' (noise only), 'rel_l2', 'y'}}: 'pred' is
        (n_draws, Ne) for V_cc / T and (n_draws, Ne, Nloc) for u_ion / j_ion (a view of one (n_draws, n_cols) tensor),
        'bands' np.percentile(pred, (5, 50, 95), axis=0), 'bands_noisy' 5 / 95 % of the noisy copy, 'rel_l2' relative_l2(pred, y).
        """
        import torch
        if int(n_draws) != n_draws or n_draws < 1:
            raise ValueError(f'n_draws must be a positive integer, got {n_draws}')
        n_draws = int(n_draws)
        table = self.theta_table(samples, burnin)
        with torch.cuda.device(self.device):
            self.assemble_inputs(table, n_draws, first_index)
            pred = self.predict(n_draws)
            compact = pred.index_select(1, self.cols)                   # the measured records, padding dropped
            noisy = self.add_noise(compact, first_index // self.lik.n_cond) if noise else None
            bands = column_percentiles(torch.cat([compact, noisy], dim=1) if noise else compact, PERCENTILES)
        out = {}
        for q in self.lik.qois:
            a, b, shape = self.views[q]
            r = {'pred': compact[:, a:b].reshape((n_draws,) + shape), 'bands': bands[:, a:b].reshape((3,) + shape),
                 'y': self.y[q]}
            if noise:
                r['noisy'] = noisy[:, a:b].reshape((n_draws,) + shape)
                nb = bands[:, self.n_cols + a:self.n_cols + b]
                r['bands_noisy'] = nb[[0, 2]].reshape((2,) + shape)
            r['rel_l2'] = relative_l2(r['pred'], self.y[q])
            out[q] = r
        return out

    def table(self, prior, post, noise):
        """print_l2_error's columns for the model rows: relative L2 of prior and posterior predictions, per QoI.
        noise: {qoi: measurement noise level} (the `exp_noise` of monte_carlo.py).  Returns the text."""
        return l2_table({q: (prior[q]['rel_l2'], post[q]['rel_l2']) for q in self.lik.qois if q in prior and q in post}, noise)
