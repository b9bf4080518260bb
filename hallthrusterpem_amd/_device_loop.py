"""A body of launches recorded into a hipGraph and replayed: what the device samplers (`samplers.py`) and searches
(`optimize.py`) share on the host.  The two rules of such a recording are stated here once:

  * a recorded launch carries its pointer and scalar arguments BY VALUE, so the graph is recorded again when one of them moves
    (`RecordedLoop._prepare`, against the `_record_key()` the subclass supplies);
  * recording runs the body (two warm-ups and the capture), so the steps it runs are undone (`RecordedLoop._record`, over the
    tensors the subclass names in `_state()`).
"""
import math

import numpy as np

from . import _lib


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


# ------------------------------------------------------------------------------------------- what the constructors share
def starts(theta0, device=None):
    """Starts given as a tensor or as anything numpy reads -> (float64 numpy array, device): a tensor's own device where none
    was asked for."""
    import torch
    if isinstance(theta0, torch.Tensor):
        if device is None:
            device = theta0.device
        theta0 = theta0.detach().cpu().numpy()
    return np.asarray(theta0, dtype=np.float64), device


def require_cuda(who: str, device, hint: str = ''):
    import torch
    if device is not None and torch.device(device).type != 'cuda':
        raise ValueError(f"{who} runs on the GPU only (got device '{device}'){hint}")


def cuda_device(device=None):
    """`device`, or the current CUDA device"""
    import torch
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def zeros_on(device):
    """z(*shape, dt=float64): a zero tensor on `device`"""
    import torch
    return lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=device)


def ensemble_parameters(who: str, E: int, K: int, d: int, a, de_fraction, g0, sigma) -> float:
    """The checks of an affine-invariant ensemble of K walkers in d dimensions and of its stretch (a) and DE (de_fraction, g0,
    sigma) moves; returns g0 (None: 2.38 / sqrt(2d))."""
    if not 1 <= d <= _lib.ENSEMBLE_MAX_DIM:
        raise ValueError(f'{who} samples 1 to {_lib.ENSEMBLE_MAX_DIM} parameters (got {d})')
    if E < 1 or K % 2 or K < 2 * d or K > _lib.ENSEMBLE_MAX_WALKERS:
        raise ValueError(f'{who} needs an even number of walkers K with 2 d = {2 * d} <= K <= {_lib.ENSEMBLE_MAX_WALKERS} per '
                         f'ensemble (got {K})')
    g0 = 2.38 / math.sqrt(2.0 * d) if g0 is None else float(g0)
    if not (0.0 <= de_fraction <= 1.0):
        raise ValueError(f'de_fraction must be in [0, 1] (got {de_fraction})')
    if de_fraction > 0.0 and K < 4:
        raise ValueError('the DE move needs two partners in the other half: K >= 4')
    if not (a > 1.0 and math.isfinite(a) and g0 > 0.0 and math.isfinite(g0) and sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError('need finite a > 1, g0 > 0 and sigma >= 0')
    return g0


def ball(center, scale, shape, seed: int = 0):
    """shape + (d,) starts center + scale * N(0, 1) from np.random.default_rng(seed); `scale` a number or one per parameter"""
    center = np.atleast_1d(np.asarray(center, dtype=np.float64))
    rng = np.random.default_rng(seed)
    return center + np.asarray(scale, dtype=np.float64) * rng.standard_normal(tuple(int(n) for n in shape) + (center.size,))


def trace_window(steps: int, n_steps: int, thin: int, keep: bool = True):
    """(rows, (trace_first, trace_len, thin)) of a run of n_steps from step `steps` that keeps steps 1, 1 + thin, ... of the
    call: rows = ceil(n_steps / thin); the window is (0, 0, 1) when nothing is kept"""
    if n_steps < 0 or thin < 1:
        raise ValueError('n_steps >= 0 and thin >= 1')
    rows = -(-n_steps // thin)
    return rows, ((steps, rows, thin) if keep and rows else (0, 0, 1))


# --------------------------------------------------------------------------------------------------- the recorded loop
class RecordedLoop:
    """A body recorded into a hipGraph and replayed.  A subclass supplies `_body` (one step: launches on the current stream, no
    host readback), `_state()` (the tensors a step changes) and `_record_key()` (everything a recorded launch carries by value
    that can change between runs), calls `_init_loop` from its constructor, `_prepare()` before and `advance(n)` to run."""

    def _init_loop(self, device, use_graph: bool):
        self.device, self.use_graph = cuda_device(device), bool(use_graph)
        self._graph, self._graph_key = None, None

    def _state(self):
        return ()

    def _record(self):
        """record `_body`; the steps that recording runs are undone"""
        saved = [t.clone() for t in self._state()]
        self._graph = None                                                                   # (frees the old recording first)
        self._graph, _ = capture_graph(self._body, self.device)
        for t, s in zip(self._state(), saved):
            t.copy_(s)

    def _prepare(self):
        """the graph is (re)recorded when the record key has changed: a recorded launch carries its arguments by value"""
        key = self._record_key()
        if self.use_graph and (self._graph is None or self._graph_key != key):
            self._record()
            self._graph_key = key

    def advance(self, n: int):
        """n steps: n replays of the recording, or n eager calls of the body"""
        if self.use_graph:
            for _ in range(n):
                self._graph.replay()
        else:
            for _ in range(n):
                self._body()


class TracedLoop(RecordedLoop):
    """`RecordedLoop` for a step sampler whose launch writes rows of trace tensors through a window (trace_first, trace_len,
    thin) of its step counter `steps`.  `_init_trace` takes the shape of one row of every trace tensor."""

    def _init_trace(self, *row_shapes):
        self._row_shapes = row_shapes
        self._traces = (None,) * len(row_shapes)
        self._window = (0, 0, 1)                                                             # trace_first, trace_len, thin

    def _record_key(self):
        return tuple(t.data_ptr() if t is not None else 0 for t in self._traces) + self._window

    def _run(self, n_steps: int, thin: int, keep):
        """Advance n_steps, writing the traces whose `keep` flag is set (the first one decides whether anything is kept).
        Returns one tensor of ceil(n_steps / thin) rows, or None, per trace."""
        import torch
        n_steps = int(n_steps)
        rows, self._window = trace_window(self.steps, n_steps, int(thin), keep[0])
        new = lambda r, shape: torch.empty((r,) + shape, dtype=torch.float64, device=self.device)        # noqa: E731
        live = self._window[1] > 0
        self._traces = tuple(new(rows, s) if k and live else None for k, s in zip(keep, self._row_shapes))
        if n_steps:
            self._prepare()
        self.advance(n_steps)
        self.steps += n_steps
        traces = self._traces
        if keep[0] and not live:
            traces = tuple(new(0, s) if k else None for k, s in zip(keep, self._row_shapes))
        self._traces = (None,) * len(self._row_shapes)
        self._window = (0, 0, 1)
        return traces
