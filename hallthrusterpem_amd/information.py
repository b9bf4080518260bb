"""Expected information gain of the calibration data, per group of measurements: which of the measurements constrain the
inputs, and which operating condition would be worth measuring next.  The reference has no such analysis (nothing to pin); the
estimator is the nested Monte Carlo one of Ryan (2003) and Huan & Marzouk (2013), stated here once and restated in long double
by tests/information_np.py.

    Zo[N][K]   the standardised observations of the N outer draws: Zo[i][k] = g_k(x_i) / sigma_k + eps[i][k], g_k the model's
               value at record k of the measurement table, sigma_k that record's own standard deviation, eps ~ N(0, 1)
    Zi[M][K]   the standardised predictions of the M inner draws: Zi[j][k] = g_k(x_j) / sigma_k
    groups     the K columns partitioned into C contiguous, non-empty groups by group_end[0 .. C-1] (ascending, the last = K);
               index C stands for the union of all columns

    for c = 0 ... C:
        d2_c(i, j) = sum_{k in c} (Zo[i][k] - Zi[j][k])^2        (the union: the sum of the groups' d2 of the same (i, j))
        l = -d2 / 2,   m_c(i) = max_j l,   s1 = sum_j exp(l - m),   s2 = sum_j exp(2 (l - m))
        lse_c(i) = m + log s1 - log M            ess_c(i) = s1^2 / s2
        u_c(i)   = -1/2 sum_{k in c} eps[i][k]^2 - lse_c(i)
        EIG_c    = mean_i u_c(i)                 stderr_c = std_i(u_c, ddof=1) / sqrt(N)

The constants of the Gaussian cancel between the two terms of u.

A draw is ONE sampled input vector: theta from the prior or from a caller's table together with the nuisance inputs from their
priors, shared by every operating condition of the table -- only the operating inputs differ between the conditions of a draw.
`Predictive.assemble_inputs` draws every (draw, condition) sample independently, which is right for predictive bands and wrong
here: a group that spans conditions would then measure the information about as many independent copies of the inputs, the sum of
the per-condition gains.  So `InformationGain.assemble_shared` takes `assemble_inputs`' samples and gives every condition of a draw
the non-operating inputs of the draw's first condition (design index first_index + d n_cond for draw d) before the predictions.
The gain above is therefore about (theta, nuisance) JOINTLY, for groups within one condition and across conditions alike.
The discharge-current weight of the likelihood is not a measurement and takes no part.

The gain about a SUBSET of the inputs (`about=`) -- the calibrated theta alone, or one parameter -- takes a third nest: the
likelihood with the other inputs averaged out, p(y | A) = mean_B p(y | A, B), the quantity the posterior, the MAP searches and the
samplers work with.  `about` is a non-empty subset A of the non-operating coupled inputs, B the rest of the non-operating inputs:

    Zc[N][L][K]  the conditional set of outer draw i: L = n_conditional input vectors that take the A-rows of outer draw i and fresh
                 B-rows, each one vector shared by all of its conditions (`assemble_shared`); vector l of outer draw d (d counted
                 BEFORE any draw is dropped) has design index first_index + (n_outer + n_inner + d L + l) n_cond, whatever `reuse`
                 is.  Zc[i][l][k] = fl64(pred * inv_std) over the same compact columns in the same `perm` order.

    for c = 0 ... C:
        d2c_c(i, l)   = sum_{k in c} (Zo[i][k] - Zc[i][l][k])^2   (the union: the sum of the groups' d2c of the same (i, l))
        a row l is used iff its union d2c is finite; used(i) counts them
        lse_cond_c(i) = logmeanexp_l(-d2c / 2) over the used rows,   ess_cond_c(i) as ess
        u_about_c(i)  = lse_cond_c(i) - lse_c(i)                  the gain about A (the 1/2 |eps|^2 terms cancel)
        u_rest_c(i)   = -1/2 sum_{k in c} eps[i][k]^2 - lse_cond_c(i)   the gain about B once A is known
        u_c(i)        = u_about_c(i) + u_rest_c(i)                the chain rule, per draw
        EIG and stderr of each as above

An outer draw with used = 0 is dropped from every mean and counted.  The independence rule: A's values of a draw are kept while
B is drawn anew, which is a draw from p(B | A) only where A and B are independent.  With samples=None every input has its own
prior and A may be any subset; with a theta table the theta columns are dependent among themselves, so A must hold every
theta name (it may add prior-drawn inputs).  A median `ess_cond` near 1 means n_conditional is too small for that group: the log
of a mean of few terms is biased downward (Jensen), which pulls u_about down and pushes u_rest up, as the same bias of lse pushes
u_about and u up.  With n_conditional = n_inner the two biases of u_about cancel for a group that A does not reach.

`ess` is the number of inner draws that carry the inner sum of an outer draw.  A group whose median ess is near 1 is saturated:
its inner sums are single terms and u_i = log M + (d2_min - |eps_i|^2) / 2, the draws are too few for that group.  What the
number then means depends on the inner set:
    reuse=True    the term j = i is in the sum and d2(i, i) = |eps_i|^2, so u_i <= log M and EIG_c <= log M: a saturated number is
                  a LOWER bound of the gain, at most log M
    reuse=False   (the default: a separate inner set) u_i is not bounded, the nested estimator is biased upward (Jensen), and a
                  saturated number is an unreliable, upward-biased one -- not a bound of either kind.  Ask for more draws or
                  narrower groups.

The all-pairs part is one fused launch (`pem_pairwise_lse_f64_dev`, csrc/pem_information.hip) that never writes an N x M matrix;
the model runs are `Predictive`'s two launches per set of draws.  The conditional part is one launch per chunk of outer draws
(`pem_conditional_lse_f64_dev`, csrc/pem_information_theta.hip) that reads the chunk's raw predictions once: the gather of the
measured records, their scaling and the (N L, K) tensor are never written.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .calibration import OPERATING
from .models.coupled import COUPLED_INPUTS
from .predictive import NOISE_STREAM_OFFSET, Predictive

EPS_STREAM_OFFSET = NOISE_STREAM_OFFSET + 1     # Philox stream of the estimator's noise: the design's stream + 4
SATURATED_ESS = 2.0                             # a group whose median ess is below this is flagged by `saturated`


def check_group_end(group_end, n_col: int):
    """group_end as an int32 array, refused unless it has 1 ... PEM_INFORMATION_MAX_GROUPS strictly ascending entries in
    (0, n_col] and ends at n_col.  Host only."""
    ge = np.asarray(group_end)
    if ge.ndim != 1 or ge.size < 1 or not np.issubdtype(ge.dtype, np.integer):
        raise ValueError(f'group_end: a non-empty 1-D array of integers, got {group_end!r}')
    if ge.size > _lib.INFORMATION_MAX_GROUPS:
        raise ValueError(f'{ge.size} groups: at most PEM_INFORMATION_MAX_GROUPS = {_lib.INFORMATION_MAX_GROUPS}')
    if np.any(np.diff(np.concatenate([[0], ge])) <= 0):
        raise ValueError(f'group_end must ascend strictly from above 0 (an empty group otherwise), got {ge.tolist()}')
    if int(ge[-1]) != int(n_col):
        raise ValueError(f'the last group must end at the number of columns {n_col}, got {int(ge[-1])}')
    return np.ascontiguousarray(ge, dtype=np.int32)


def group_columns(labels):
    """(perm, group_end, values) for one integer label per column: `perm` (stable) makes the columns of a label contiguous, the
    groups follow in the order of the label values 0 ... G-1, G = max + 1.  Refused: a negative label, more than
    PEM_INFORMATION_MAX_GROUPS groups, a label value without a column (an empty group).  Host only."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.size < 1 or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError('group labels: one integer per column')
    if lab.min() < 0:
        raise ValueError(f'group labels are 0 ... G-1, got {int(lab.min())}')
    n_groups = int(lab.max()) + 1
    if n_groups > _lib.INFORMATION_MAX_GROUPS:
        raise ValueError(f'{n_groups} groups: at most PEM_INFORMATION_MAX_GROUPS = {_lib.INFORMATION_MAX_GROUPS}')
    counts = np.bincount(lab, minlength=n_groups)
    if np.any(counts == 0):
        raise ValueError(f'group {int(np.flatnonzero(counts == 0)[0])} is empty')
    perm = np.argsort(lab, kind='stable').astype(np.int64)
    return perm, np.cumsum(counts).astype(np.int32), np.arange(n_groups)


def finite_draws(z_in_outer, eps, z_in_inner, reuse: bool = False):
    """The draws whose standardised values are finite in every column: (z_in_outer, eps, z_in_inner, dropped) with the other
    rows removed from both sets and counted ((outer, inner); with `reuse` the inner set is the outer one).  Refused when fewer
    than two draws remain on either side."""
    import torch
    keep_o = torch.isfinite(z_in_outer).all(dim=1) & torch.isfinite(eps).all(dim=1)
    keep_i = keep_o if reuse else torch.isfinite(z_in_inner).all(dim=1)
    dropped = (int((~keep_o).sum()), int((~keep_i).sum()))
    if dropped[0]:
        z_in_outer, eps = z_in_outer[keep_o], eps[keep_o]
    if reuse:
        z_in_inner = z_in_outer
    elif dropped[1]:
        z_in_inner = z_in_inner[keep_i]
    if z_in_outer.shape[0] < 2 or z_in_inner.shape[0] < 2:
        raise ValueError(f'fewer than two draws are left after dropping the non-finite ones: {z_in_outer.shape[0]} outer, '
                         f'{z_in_inner.shape[0]} inner')
    return z_in_outer, eps, z_in_inner, dropped


def _rows(t, name):
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float64:
        raise ValueError(f'{name}: a 2-D float64 tensor, got {type(t).__name__} '
                         f'{tuple(t.shape) if hasattr(t, "shape") else ""} {getattr(t, "dtype", "")}')
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def pairwise_information(z_in_outer, eps, z_in_inner, group_end):
    """The estimator of the module docstring for standardised predictions of the outer draws `z_in_outer` (N, K), their noise
    `eps` (N, K) and standardised predictions of the inner draws `z_in_inner` (M, K): float64 device tensors, finite.
    Returns {'eig', 'stderr', 'ess_median', 'ess_min': (C+1,), 'lse', 'ess': (N, C+1), 'log_M'}; index C is the union."""
    import torch
    z_in_outer, eps, z_in_inner = _rows(z_in_outer, 'z_in_outer'), _rows(eps, 'eps'), _rows(z_in_inner, 'z_in_inner')
    n, k = z_in_outer.shape
    m = z_in_inner.shape[0]
    if eps.shape != z_in_outer.shape or z_in_inner.shape[1] != k:
        raise ValueError(f'shapes: z_in_outer {tuple(z_in_outer.shape)}, eps {tuple(eps.shape)}, z_in_inner {tuple(z_in_inner.shape)}')
    if n < 1 or m < 1 or k < 1:
        raise ValueError(f'empty operands: {n} outer draws, {m} inner draws, {k} columns')
    ge = check_group_end(group_end, k)
    dev = z_in_outer.device
    if dev.type != 'cuda' or eps.device != dev or z_in_inner.device != dev:
        raise ValueError('z_in_outer, eps and z_in_inner must be tensors of one GPU: hallthrusterpem_amd has no CPU path')
    lib = _lib.load()
    sets = ge.size + 1
    with torch.cuda.device(dev):
        z_out = z_in_outer + eps
        lse = torch.empty((n, sets), dtype=torch.float64, device=dev)
        ess = torch.empty_like(lse)
        work = torch.empty(int(lib.pem_pairwise_lse_work_len(n, m, ge.size)), dtype=torch.float64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())                                                          # noqa: E731
        _lib.check(lib.pem_pairwise_lse_f64_dev(n, m, k, p(z_out), z_out.stride(0), p(z_in_inner), z_in_inner.stride(0), ge.size,
                                                C.c_void_p(ge.ctypes.data), p(lse), p(ess), p(work), work.numel(),
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        u = -0.5 * _noise_norms(eps, ge) - lse
        eig, stderr = _mean_stderr(u)
        out = {'eig': eig, 'stderr': stderr,
               'ess_median': ess.quantile(0.5, dim=0), 'ess_min': ess.min(dim=0).values, 'lse': lse, 'ess': ess,
               'log_M': math.log(m)}
    return out


def _noise_norms(eps, ge):
    """(N, C+1): sum_{k in c} eps[i][k]^2 of every group and of all columns"""
    import torch
    e2 = eps * eps
    first = [0] + ge[:-1].tolist()
    return torch.stack([e2[:, a:b].sum(dim=1) for a, b in zip(first, ge.tolist())] + [e2.sum(dim=1)], dim=1)


def _mean_stderr(u):
    """the mean over the draws and its standard error (NaN for one draw), per set"""
    import torch
    n = u.shape[0]
    return u.mean(dim=0), u.std(dim=0, unbiased=True) / math.sqrt(n) if n > 1 else torch.full_like(u[0], math.nan)


def conditional_information(z_out, pred, n_per: int, group_end, col=None, scale=None):
    """The conditional term of the module docstring in one launch (`pem_conditional_lse_f64_dev`): for every row i of the
    standardised observations `z_out` (N, K) the log-mean-exp of -d2 / 2 over ITS rows i n_per ... (i + 1) n_per - 1 of `pred`
    (N n_per, R), the raw predictions.  Column k of the estimator is record `col[k]` of `pred` (an integer device tensor of K
    record indices in [0, R); None: record k) times `scale[k]` (a float64 device tensor; None: 1), the product rounded to fp64
    before the subtraction.  A row of `pred` whose d2 over all columns is not finite is left out of every set.
    Returns {'lse', 'ess': (N, C+1) float64, 'used': (N,) int32}; index C is the union; used = 0 gives NaN."""
    import torch
    z_out, pred = _rows(z_out, 'z_out'), _rows(pred, 'pred')
    n, k = z_out.shape
    if int(n_per) != n_per or n_per < 1:
        raise ValueError(f'n_per must be a positive integer, got {n_per}')
    n_per = int(n_per)
    if n < 1 or k < 1 or pred.shape[1] < 1:
        raise ValueError(f'empty operands: z_out {tuple(z_out.shape)}, pred {tuple(pred.shape)}')
    if pred.shape[0] != n * n_per:
        raise ValueError(f'pred has {pred.shape[0]} rows: {n} rows of z_out x n_per {n_per} = {n * n_per} expected')
    ge = check_group_end(group_end, k)
    dev = z_out.device
    if col is not None:
        if not isinstance(col, torch.Tensor) or col.dim() != 1 or col.numel() != k or col.dtype not in (torch.int32, torch.int64):
            raise ValueError(f'col: one int32 or int64 record index per column ({k})')
    elif pred.shape[1] < k:
        raise ValueError(f'pred has {pred.shape[1]} records for {k} columns and no col')
    if scale is not None and (not isinstance(scale, torch.Tensor) or scale.shape != (k,) or scale.dtype != torch.float64):
        raise ValueError(f'scale: one float64 factor per column ({k})')
    if dev.type != 'cuda' or any(t is not None and t.device != dev for t in (pred, col, scale)):
        raise ValueError('z_out, pred, col and scale must be tensors of one GPU: hallthrusterpem_amd has no CPU path')
    lib = _lib.load()
    with torch.cuda.device(dev):
        if col is not None:
            if int(col.min()) < 0 or int(col.max()) >= pred.shape[1]:
                raise ValueError(f'col: record indices in [0, {pred.shape[1]}), got {int(col.min())} ... {int(col.max())}')
            col = col.to(torch.int32).contiguous()
        if scale is not None:
            scale = scale.contiguous()
        lse = torch.empty((n, ge.size + 1), dtype=torch.float64, device=dev)
        ess = torch.empty_like(lse)
        used = torch.empty(n, dtype=torch.int32, device=dev)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                                   # noqa: E731
        _lib.check(lib.pem_conditional_lse_f64_dev(n, n_per, k, p(z_out), z_out.stride(0), p(pred), pred.stride(0), p(col), p(scale),
                                                   ge.size, C.c_void_p(ge.ctypes.data), p(lse), p(ess), p(used),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return {'lse': lse, 'ess': ess, 'used': used}


def saturated(result):
    """per set: True where the median ess is below SATURATED_ESS -- with a reused inner set the estimate is then a lower bound (at
    most log M), with a separate one it is biased upward and unreliable (module docstring)"""
    return result['ess_median'] < SATURATED_ESS


class InformationGain:
    """Expected information gain of the datasets of a `Predictive`'s measurement table, per group of measurements.

    :param predictive: the `predictive.Predictive` whose likelihood table, theta names, priors and design are used.  The
                       standardisation is the per-record 1/std of the likelihood's record table, NOT `Predictive.sigma`
                       (the per-dataset mean the reference uses for plotting bands).
    """

    def __init__(self, predictive: Predictive):
        import torch
        self.pred = pred = predictive
        lik = pred.lik
        self.inv_std = lik.rec[:, 2].index_select(0, pred.cols).contiguous()          # (n_cols,), in the compact column order
        span = lik.span.cpu().numpy()
        qoi, cond = [], []
        from .likelihood import _KIND
        for iq, q in enumerate(lik.qois):
            sl = lik.conditions[q]
            for c in range(sl.start, sl.stop):
                count = int(span[c, _KIND[q], 1])
                qoi += [iq] * count
                cond += [c] * count
        self.column_qoi = np.asarray(qoi, dtype=np.int64)
        self.column_condition = np.asarray(cond, dtype=np.int64)
        if self.column_qoi.size != int(pred.cols.numel()):
            raise ValueError('the measurement table and the predictive\'s columns disagree')
        self._ones = torch.ones_like(self.inv_std)
        self._cond_batch = None                                 # the batch of the conditional sets' chunks (`_conditional`)
        self._shared_rows = torch.as_tensor([i for i, k in enumerate(COUPLED_INPUTS) if k not in OPERATING], device=self.inv_std.device)

    def groups(self, by='qoi'):
        """(perm, group_end, labels): the column permutation (indices into the compact columns) that makes the groups
        contiguous, the groups' ends and their labels.  by='qoi': one group per measured quantity; by='condition': one per
        (quantity, operating condition) block of the table, labelled 'qoi[e]'; or one integer label 0 ... G-1 per compact
        column.  ValueError for more than PEM_INFORMATION_MAX_GROUPS groups or an empty group."""
        lik = self.pred.lik
        if isinstance(by, str):
            if by == 'qoi':
                lab, names = self.column_qoi, list(lik.qois)
            elif by == 'condition':
                lab = self.column_condition
                names = {c: f'{q}[{c - lik.conditions[q].start}]' for q in lik.qois
                         for c in range(lik.conditions[q].start, lik.conditions[q].stop)}
            else:
                raise ValueError(f"by: 'qoi', 'condition' or one integer label per column, got {by!r}")
            present, compact = np.unique(lab, return_inverse=True)      # a block without a measured record makes no group
            perm, ge, values = group_columns(compact.astype(np.int64))
            return perm, ge, [names[present[v]] for v in values]
        lab = np.asarray(by)
        if lab.shape != self.column_qoi.shape:
            raise ValueError(f'by: one label per compact column ({self.column_qoi.size}), got shape {lab.shape}')
        perm, ge, values = group_columns(lab)
        return perm, ge, [int(v) for v in values]

    def assemble_shared(self, table, n_draws: int, first_index: int = 0):
        """`Predictive.assemble_inputs`' [15][n_draws n_cond] inputs with ONE input vector per draw: every condition c of draw d
        keeps its own operating row and takes the other inputs -- theta and nuisance -- of sample d n_cond, the draw's first
        condition (design index first_index + d n_cond).  Returns the batch's input tensor."""
        pred = self.pred
        x = pred.assemble_inputs(table, n_draws, first_index)
        v = x[:, :n_draws * pred.lik.n_cond].view(x.shape[0], n_draws, pred.lik.n_cond)
        v[self._shared_rows] = v[self._shared_rows, :, :1].clone()
        return x

    def standardised(self, table, n_draws: int, first_index: int, perm):
        """(n_draws, K) model values at the measured records over their standard deviations, columns in the order `perm`, for
        the draws whose first design index is `first_index` (`assemble_shared` + `Predictive.predict`)."""
        self.assemble_shared(table, n_draws, first_index)
        return self._standardise(n_draws, perm)

    def _standardise(self, n_draws: int, perm):
        """`standardised` for the inputs the batch holds"""
        compact = self.pred.predict(n_draws).index_select(1, self.pred.cols)
        return (compact * self.inv_std).index_select(1, perm)

    def noise(self, n_draws: int, first_row: int, perm):
        """(n_draws, K) standard normal draws (`pem_predictive_noise_f64_dev` with unit sigma on stream EPS_STREAM_OFFSET),
        keyed by (draw index, compact column) and then put in the order `perm`: the same whatever the grouping."""
        import torch
        pred = self.pred
        zero = torch.zeros((n_draws, self.inv_std.numel()), dtype=torch.float64, device=pred.device)
        out = torch.empty_like(zero)
        _lib.check(_lib.load().pem_predictive_noise_f64_dev(
            n_draws, zero.shape[1], C.c_void_p(zero.data_ptr()), zero.stride(0), C.c_void_p(self._ones.data_ptr()), int(first_row),
            pred.design.seed, pred.design.stream + EPS_STREAM_OFFSET, C.c_void_p(out.data_ptr()), out.stride(0), pred._stream()))
        return out.index_select(1, perm)

    def check_about(self, about, samples=None):
        """`about` as a tuple of input names, refused unless it is a non-empty set of non-operating coupled inputs without
        repeats that -- with a theta table -- holds every theta name (the independence rule of the module docstring).  Host only."""
        names = (about,) if isinstance(about, str) else tuple(about)
        if not names:
            raise ValueError('about: at least one input name')
        for k in names:
            if k not in COUPLED_INPUTS or k in OPERATING:
                raise ValueError(f"about: '{k}' is not a non-operating input of the coupled model")
        if len(set(names)) != len(names):
            raise ValueError(f'about: names repeat: {names}')
        if samples is not None:
            missing = [k for k in self.pred.names if k not in names]
            if missing:
                raise ValueError(f'about: with a theta table the theta columns are drawn together, so about must hold every theta '
                                 f'name; missing {missing}')
        return names

    def run(self, samples=None, n_outer: int = 4096, n_inner: int = 4096, by='qoi', reuse: bool = False, burnin: float = 0.1,
            first_index: int = 0, keep: bool = False, about=None, n_conditional: int = 128, chunk_samples: int = 2 ** 20):
        """The expected information gain of every group of `groups(by)` and of all measurements together.

        :param samples: as `Predictive.run`: None for the prior -- the gain expected from the data before any is used -- or a
                        trace / table of theta values: the gain relative to that posterior.
        :param n_outer, n_inner: the outer draws start at design index `first_index` (as `Predictive.run` counts it: draw d is
                        the input vector of index first_index + d n_cond, shared by its conditions), the inner draws are the next
                        n_inner.  With reuse=True the inner set IS the outer set, as Huan & Marzouk reuse it, and the term j = i
                        stays in (n_inner is not used): then EIG <= log M.
        :param keep: also return 'z_outer' (the standardised observations), 'eps' and 'z_inner', columns in the groups' order.
        :param about: None, or the inputs A whose share of the gain is wanted (module docstring): a name or names of non-operating
                        coupled inputs; with `samples` it must hold every theta name.  None runs nothing more and changes no bit.
        :param n_conditional: L, the input vectors of every outer draw's conditional set.
        :param chunk_samples: the conditional sets are predicted max(1, chunk_samples // (n_conditional n_cond)) outer draws at a
                        time, in a batch of their own; no result depends on it.
        Returns `pairwise_information`'s dict plus 'labels' (the last is 'all'), 'perm', 'group_end', 'n_outer', 'n_inner' (the
        draws used), 'reuse' and 'dropped' ((outer, inner) draws with a non-finite value in some column).  With `about` also
        'about', 'eig_about', 'stderr_about', 'eig_rest', 'stderr_rest', 'ess_cond_median' (C+1,), 'lse_cond', 'ess_cond', 'u_about',
        'u_rest' (n_outer, C+1), 'used' (n_outer,), 'used_min', 'n_conditional' and 'dropped_conditional': the outer draws
        without a used row, left out of every mean ('eig' and 'stderr' included); with `keep`, 'z_cond' (n_outer, L, K)."""
        n_outer, n_inner, first_index = self._counts(n_outer, n_inner, first_index)
        if about is not None:
            about = self.check_about(about, samples)
            n_conditional, chunk_samples = self._conditional_counts(n_conditional, chunk_samples)
        out, state = self._joint(samples, n_outer, n_inner, by, reuse, burnin, first_index, keep, about is not None)
        if about is not None:
            out.update(self._conditional(state, out, about, n_conditional, chunk_samples, keep))
        return out

    @staticmethod
    def _counts(n_outer, n_inner, first_index):
        for name, v in (('n_outer', n_outer), ('n_inner', n_inner), ('first_index', first_index)):
            if int(v) != v or v < (0 if name == 'first_index' else 1):
                raise ValueError(f'{name} must be a {"non-negative" if name == "first_index" else "positive"} integer, got {v}')
        return int(n_outer), int(n_inner), int(first_index)

    @staticmethod
    def _conditional_counts(n_conditional, chunk_samples):
        for name, v in (('n_conditional', n_conditional), ('chunk_samples', chunk_samples)):
            if int(v) != v or v < 1:
                raise ValueError(f'{name} must be a positive integer, got {v}')
        return int(n_conditional), int(chunk_samples)

    def _joint(self, samples, n_outer, n_inner, by, reuse, burnin, first_index, keep, conditional):
        """the joint gain (one outer set, one inner set, one pairwise launch) and, for `_conditional`, what it needs of the outer
        draws BEFORE any is dropped: their input vectors, their observations and which of them are kept"""
        import torch
        pred = self.pred
        perm_np, ge, labels = self.groups(by)
        table = pred.theta_table(samples, burnin)
        n_cond = pred.lik.n_cond
        state = None
        with torch.cuda.device(pred.device):
            perm = torch.as_tensor(perm_np, device=pred.device)
            if conditional:
                x = self.assemble_shared(table, n_outer, first_index)
                inputs = x[:, :n_outer * n_cond:n_cond].clone()                      # (15, n_outer): one input vector per draw
                z_o = self._standardise(n_outer, perm)
            else:
                z_o = self.standardised(table, n_outer, first_index, perm)
            eps = self.noise(n_outer, first_index // n_cond, perm)
            if conditional:
                state = dict(table=table, perm=perm, group_end=ge, inputs=inputs, z_obs=z_o + eps, first_index=first_index,
                             kept=torch.isfinite(z_o).all(dim=1) & torch.isfinite(eps).all(dim=1),     # `finite_draws`' outer filter
                             first_conditional=first_index + (n_outer + n_inner) * n_cond)
            z_i = z_o if reuse else self.standardised(table, n_inner, first_index + n_outer * n_cond, perm)
            z_o, eps, z_i, dropped = finite_draws(z_o, eps, z_i, reuse)
            out = pairwise_information(z_o, eps, z_i, ge)
            out.update(labels=list(labels) + ['all'], perm=perm_np, group_end=ge, n_outer=z_o.shape[0], n_inner=z_i.shape[0],
                       reuse=bool(reuse), dropped=dropped)
            if keep:
                out.update(z_outer=z_o + eps, eps=eps, z_inner=z_i)
            if conditional:
                state['eps'] = eps
        return out, state

    def _conditional(self, state, joint, about, n_conditional: int, chunk_samples: int, keep: bool):
        """the conditional nest of the module docstring for the inputs `about`, on the outer draws of `_joint`: per chunk of outer
        draws one `assemble_shared` on a batch of its own, the A-rows overwritten with the chunk's outer values, one predict and
        one `conditional_information` launch.  Returns what `run` adds to the joint result (which is not changed here)."""
        import torch
        pred = self.pred
        n_cond, L, ge = pred.lik.n_cond, n_conditional, state['group_end']
        n_all = state['z_obs'].shape[0]
        chunk = min(n_all, max(1, chunk_samples // (L * n_cond)))
        with torch.cuda.device(pred.device):
            a_rows = torch.as_tensor([COUPLED_INPUTS.index(k) for k in about], device=pred.device)
            col = pred.cols.index_select(0, state['perm'])
            scale = self.inv_std.index_select(0, state['perm'])
            raw = torch.empty((chunk * L, max(pred.lik.n_rec, 1)), dtype=torch.float64, device=pred.device)
            parts, z_cond = [], []
            main, pred.batch = pred.batch, self._cond_batch              # the chunks' batch: `Predictive.batch` keeps its size
            try:
                for d0 in range(0, n_all, chunk):
                    nb = min(chunk, n_all - d0)                          # (a ragged last chunk runs at the full size: one batch)
                    x = self.assemble_shared(state['table'], chunk * L, state['first_conditional'] + d0 * L * n_cond)
                    v = x[:, :chunk * L * n_cond].view(x.shape[0], chunk, L * n_cond)
                    v[a_rows, :nb] = state['inputs'][a_rows, d0:d0 + nb, None]
                    pred.predict(chunk * L, out=raw)
                    parts.append(conditional_information(state['z_obs'][d0:d0 + nb], raw[:nb * L], L, ge, col, scale))
                    if keep:
                        z_cond.append((raw[:nb * L].index_select(1, col) * scale).view(nb, L, -1))
            finally:
                self._cond_batch, pred.batch = pred.batch, main
            kept = state['kept']
            lse_c, ess_c, used = (torch.cat([p[k] for p in parts])[kept] for k in ('lse', 'ess', 'used'))
            good = used > 0
            n_bad = int((~good).sum())
            if n_bad == used.numel():
                raise ValueError('no outer draw has a finite row in its conditional set')
            half, lse = _noise_norms(state['eps'], ge), joint['lse']
            u_about, u_rest = lse_c - lse, -0.5 * half - lse_c
            add = dict(about=tuple(about), n_conditional=L, lse_cond=lse_c, ess_cond=ess_c, used=used, used_min=int(used.min()),
                       u_about=u_about, u_rest=u_rest, dropped_conditional=n_bad)
            if n_bad:
                u_about, u_rest, ess_c = u_about[good], u_rest[good], ess_c[good]
                add['eig'], add['stderr'] = _mean_stderr((-0.5 * half - lse)[good])
            add['eig_about'], add['stderr_about'] = _mean_stderr(u_about)
            add['eig_rest'], add['stderr_rest'] = _mean_stderr(u_rest)
            add['ess_cond_median'] = ess_c.quantile(0.5, dim=0)
            if keep:
                add['z_cond'] = torch.cat(z_cond)[kept]
        return add

    def by_parameter(self, samples=None, n_outer: int = 4096, n_inner: int = 4096, by='qoi', reuse: bool = False, burnin: float = 0.1,
                     first_index: int = 0, n_conditional: int = 128, chunk_samples: int = 2 ** 20):
        """Which measurement informs which parameter: one outer set, one inner set and one pairwise launch as `run`, then the
        conditional nest with about=(name,) for every theta name -- each row is what `run(about=(name,))` returns.  From the prior
        only: with a theta table of more than one column the independence rule refuses a single name.
        Returns {'names', 'labels', 'eig_about', 'stderr_about', 'eig_rest', 'stderr_rest', 'ess_cond_median': (n_theta, C+1),
        'used_min', 'dropped_conditional': per name, 'joint': the joint result, 'table': the text}."""
        import torch
        n_outer, n_inner, first_index = self._counts(n_outer, n_inner, first_index)
        n_conditional, chunk_samples = self._conditional_counts(n_conditional, chunk_samples)
        abouts = [self.check_about((k,), samples) for k in self.pred.names]
        joint, state = self._joint(samples, n_outer, n_inner, by, reuse, burnin, first_index, False, True)
        rows = [self._conditional(state, joint, a, n_conditional, chunk_samples, False) for a in abouts]
        out = {k: torch.stack([r[k] for r in rows]) for k in ('eig_about', 'stderr_about', 'eig_rest', 'stderr_rest', 'ess_cond_median')}
        out.update(names=list(self.pred.names), labels=joint['labels'], joint=joint, n_conditional=n_conditional,
                   used_min=[r['used_min'] for r in rows], dropped_conditional=[r['dropped_conditional'] for r in rows])
        eig, se = out['eig_about'].cpu().numpy(), out['stderr_about'].cpu().numpy()
        tot, tot_se = joint['eig'].cpu().numpy(), joint['stderr'].cpu().numpy()
        cell = lambda a, b: f'{a:>8.3f} +- {b:<6.3f}'                                                    # noqa: E731
        lines = [f'{"EIG about":>14} ' + ' '.join(f'{str(lab):>18}' for lab in out['labels'])]
        lines += [f'{name:>14} ' + ' '.join(cell(eig[p, c], se[p, c]) for c in range(eig.shape[1])) for p, name in enumerate(out['names'])]
        lines.append(f'{"all inputs":>14} ' + ' '.join(cell(tot[c], tot_se[c]) for c in range(tot.shape[0])))
        out['table'] = '\n'.join(lines)
        return out

    def table(self, result):
        """the groups ranked by their gain, as text: EIG +- stderr [nats], median and minimum ess, and the saturation flag: with
        a reused inner set a lower bound (at most log M), with a separate one an upward-biased, unreliable number"""
        eig, se = result['eig'].cpu().numpy(), result['stderr'].cpu().numpy()
        med, low = result['ess_median'].cpu().numpy(), result['ess_min'].cpu().numpy()
        cond = 'eig_about' in result
        if cond:
            ea, sa, er, sr, mc = (result[k].cpu().numpy() for k in ('eig_about', 'stderr_about', 'eig_rest', 'stderr_rest', 'ess_cond_median'))
        head = f' {"about":>8} {"stderr":>8} {"rest":>8} {"stderr":>8} {"ess cond":>9}' if cond else ''
        tail = f', about = {", ".join(result["about"])}, L = {result["n_conditional"]}' if cond else ''
        lines = [f'{"group":>14} {"EIG":>8} {"stderr":>8} {"ess med":>9} {"ess min":>9}{head}   (log M = {result["log_M"]:.3f}{tail})']
        for c in sorted(range(len(eig)), key=lambda c: -eig[c]):
            flag = '' if med[c] >= SATURATED_ESS else ('  saturated: a lower bound' if result.get('reuse') else
                                                       '  saturated: biased upward, unreliable (more draws or narrower groups)')
            more = f' {ea[c]:>8.3f} {sa[c]:>8.3f} {er[c]:>8.3f} {sr[c]:>8.3f} {mc[c]:>9.1f}' if cond else ''
            lines.append(f'{str(result["labels"][c]):>14} {eig[c]:>8.3f} {se[c]:>8.3f} {med[c]:>9.1f} {low[c]:>9.2f}{more}{flag}')
        return '\n'.join(lines)
