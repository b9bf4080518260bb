"""The coupled model's exact Jacobian and the derivative-based sensitivity measures built on it (csrc/pem_jacobian.hip;
`drivers.derivative_sensitivity` is the driver).

  jacobian        d(V_cc, div_angle, T_c) / d(inputs) for every sample, written out: one launch of `pem_coupled_jacobian_f64_dev`
  gradient_sums   one fused launch: the design's samples generated on chip, the Jacobian taken in the prior's own coordinates,
                  and only the sums below returned
  measures        DGSM nu_i = E[g_i^2] with its standard error, the bound ST_i <= C_i nu_i / Var f (Sobol' & Kucherenko 2009;
                  Lamboni et al. 2013), and the active subspace of each QoI (Constantine 2015) from those sums

The gradient is taken in the coordinate z_i the prior is stated in: x_i for uniform and normal inputs, log10 x_i for log-uniform
ones, g_i = x_i ln 10 df/dx_i.  Rows of the sums, per QoI with centre c and d varied inputs:
    0                 sum (f - c)            1                   sum (f - c)^2
    2 .. 1 + d        sum g_i                2 + d .. 1 + 2 d    sum g_i^4
    2 + 2 d ..        sum g_i g_j for i <= j, the upper triangle row by row

The derivative is that of the branch the evaluation takes: where V_cc is clamped to 0 its row is zero and T sees no cathode input,
where it is clamped to V_a dV_cc/dV_a = 1, where a1 is clipped at pi/2 it has no derivative.  At the kinks themselves the model
has none.

Not provided: other QoIs, the j_ion profile, an fp32 model, sharding over a process group, the surrogate.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, _marshal as m, constants
from .models.coupled import COUPLED_INPUTS

QOI_NAMES = ('V_cc', 'div_angle', 'T_c')
DEFAULT_BLOCKS = 512      # two workgroups per CU (57 KB of LDS each)
UNIFORM, LOGUNIFORM, NORMAL = 0, 1, 2


def n_rows(nv: int) -> int:
    return 2 + 2 * nv + nv * (nv + 1) // 2


def _columns(wrt):
    names = list(COUPLED_INPUTS if wrt is None else wrt)
    for k in names:
        if k not in COUPLED_INPUTS:
            raise ValueError(f"jacobian: '{k}' is not an input of the coupled model {COUPLED_INPUTS}")
    if len(set(names)) != len(names):
        raise ValueError(f'jacobian: wrt names an input twice: {names}')
    return np.ascontiguousarray([COUPLED_INPUTS.index(k) for k in names], dtype=np.int32)


def jacobian(inputs: dict, wrt=None, radius: float = 1.0) -> dict:
    """The three reduced QoIs of the coupled fp64 model and their exact derivatives with respect to the inputs named in `wrt`
    (default: all 15, in COUPLED_INPUTS order), in physical units.

    inputs: the 15 arrays of COUPLED_INPUTS, scalars broadcast as in `pem_v0_coupled`.  numpy in -> numpy out; CUDA tensors in ->
    CUDA tensors out on the current stream.
    Returns {'V_cc', 'div_angle', 'T_c': the loop shape; 'jacobian': (3, len(wrt)) + the loop shape, rows in that order of QoIs;
    'flags': uint8, bit 0 a non-physical thruster result, bit 1 an invalid plume row}.
    Not provided: other QoIs, the j_ion profile, an fp32 model."""
    cols = _columns(wrt)
    if not radius > 0:
        raise ValueError(f'jacobian: radius must be positive, got {radius}')
    missing = [k for k in COUPLED_INPUTS if k not in inputs]
    if missing:
        raise ValueError(f'jacobian: missing inputs {missing}')
    import torch
    vals = [inputs[k] for k in COUPLED_INPUTS]
    shape = m.loop_shape(vals)
    n = int(np.prod(shape))
    on_device = m.any_device_tensor(vals)
    dev = m.pick_device(vals) if on_device else torch.device('cuda', torch.cuda.current_device())
    nv = int(cols.size)
    with torch.cuda.device(dev):
        x = torch.stack([m.dev_flat(v, shape, dev) for v in vals]).contiguous()
        qoi = torch.empty((3, n), dtype=torch.float64, device=dev)
        jac = torch.empty((3, nv, n), dtype=torch.float64, device=dev)
        flags = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().pem_coupled_jacobian_f64_dev(n, m.t_ptr(x), nv, C.c_void_p(cols.ctypes.data) if nv else None,
                                                            constants.TORR_2_PA, float(radius), m.t_ptr(qoi), m.t_ptr(jac) if nv else None,
                                                            m.t_ptr(flags), m.current_stream_ptr(dev)))
    out = {k: qoi[i].reshape(shape) for i, k in enumerate(QOI_NAMES)}
    out['jacobian'] = jac.reshape((3, nv) + shape)
    out['flags'] = flags.reshape(shape)
    if not on_device:
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return out


def gradient_sums(design, varied, n: int, centre=None, first_index: int = 0, method: str = 'mc', scramble: bool = True,
                  radius: float = 1.0, n_blocks: int | None = None, device=None, stream=None):
    """One launch of `pem_gradient_sums_f64_dev` / `pem_gradient_sums_qmc_f64_dev`: samples first_index .. first_index + n - 1 of
    `design` (exactly `design.sample(n, first_index=..., method=...)`), the coupled fp64 model and its Jacobian on each, the gradient
    with respect to the inputs `varied` (indices 0..14 in any order, at most 15, possibly none) in the prior's own coordinates.
    `centre`: 3 numbers (a tensor on the device is used in place) or None for zeros; method 'mc' or 'sobol' as in `Design.fill`.
    Returns (sums [2 + 2 d + d (d + 1) / 2][3] float64 CUDA tensor, rows as in the module docstring; counts [3] int64: non-physical
    thruster results, invalid plume rows, and skipped samples -- those with an f or a g that is not finite, left out of every sum)."""
    if method not in ('mc', 'sobol'):
        raise ValueError(f"gradient_sums: method must be 'mc' or 'sobol', got '{method}'")
    if n < 0 or first_index < 0:
        raise ValueError('gradient_sums: n and first_index must not be negative')
    if method == 'sobol' and first_index + n > 1 << 30:
        raise ValueError(f"the Sobol' sequence has 2^30 points: first_index + n = {first_index + n}")
    if not radius > 0:
        raise ValueError(f'gradient_sums: radius must be positive, got {radius}')
    varied = np.ascontiguousarray(varied, dtype=np.int32).reshape(-1)
    nv = int(varied.size)
    if nv > 15:
        raise ValueError(f'gradient_sums: at most 15 varied inputs, got {nv}')
    if nv and (varied.min() < 0 or varied.max() > 14):
        raise ValueError(f'gradient_sums: varied holds indices 0..14, got {varied.tolist()}')
    import torch
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    n_blocks = DEFAULT_BLOCKS if n_blocks is None else int(n_blocks)
    if centre is not None:
        centre = torch.as_tensor(centre, dtype=torch.float64).to(dev).contiguous()
        if centre.shape != (3,):
            raise ValueError(f'gradient_sums: centre holds one number per QoI (3), got {tuple(centre.shape)}')
    partial = torch.empty((max(n_blocks, 1), n_rows(nv), 3), dtype=torch.float64, device=dev)
    flags = torch.empty((max(n_blocks, 1), 3), dtype=torch.int64, device=dev)
    ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                               # noqa: E731
    with torch.cuda.device(dev), torch.cuda.stream(s):
        lib = _lib.load()
        tail = (ptr(design.kind), ptr(design.a), ptr(design.b), nv, ptr(varied) if nv else None,
                C.c_void_p(centre.data_ptr()) if centre is not None else None, constants.TORR_2_PA, float(radius),
                C.c_void_p(partial.data_ptr()), C.c_void_p(flags.data_ptr()), n_blocks, C.c_void_p(s.cuda_stream))
        if method == 'sobol':
            _lib.check(lib.pem_gradient_sums_qmc_f64_dev(int(n), int(first_index), design.seed, design.stream, int(bool(scramble)), *tail))
        else:
            _lib.check(lib.pem_gradient_sums_f64_dev(int(n), int(first_index), design.seed, design.stream, *tail))
        return partial.sum(dim=0), flags.sum(dim=0)


def measures(sums, n_used, kinds, a, b):
    """The estimates from sums [2 + 2 d + d (d + 1) / 2][3] over N = n_used samples (pure tensor arithmetic: the sums may come from
    anywhere).  kinds, a, b: the prior of each of the d inputs as `sampling.Prior` stores it (log-uniform: a, b are log10 bounds).
        mean_q - c_q = row0 / N        var_q = row1 / N - (row0 / N)^2        mean_gradient_qi = row(2 + i) / N
        nu_qi = E[g_i^2] = (the diagonal of the pair rows) / N        nu_se = sqrt((row(2 + d + i) / N - nu^2) / N)
        bound_ST_qi = C_i nu_qi / var_q,  C_i = (b - a)^2 / pi^2 for uniform and log-uniform inputs, b^2 for normal ones
        C_q = diag(s) E[g g^T] diag(s),  s_i = (b - a) / 2 or sigma: the gradient in standardised coordinates
        eigenvalues (descending) and eigenvectors of C_q (torch.linalg.eigh);  activity_qi = sum_k lambda_k w_ik^2
    Returns {'mean' (without the centre: add it), 'var': [3]; 'mean_gradient', 'nu', 'nu_se', 'bound_ST', 'activity': [3][d];
    'C', 'eigenvectors': [3][d][d]; 'eigenvalues': [3][d]}.  Where var == 0 the bound is the division's own inf or NaN."""
    import torch
    sums = torch.as_tensor(sums, dtype=torch.float64)
    dev = sums.device
    kinds = torch.as_tensor(np.asarray(kinds), dtype=torch.int64, device=dev)
    a = torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)
    b = torch.as_tensor(np.asarray(b, dtype=np.float64), device=dev)
    d = int(kinds.numel())
    if sums.shape != (n_rows(d), 3):
        raise ValueError(f'measures: {d} inputs take sums of shape ({n_rows(d)}, 3), got {tuple(sums.shape)}')
    N = float(n_used)
    m0 = sums[0] / N
    var = sums[1] / N - m0 * m0
    iu = torch.triu_indices(d, d, device=dev)
    M = torch.zeros((3, d, d), dtype=torch.float64, device=dev)
    pairs = (sums[2 + 2 * d:] / N).T                                  # [3][d (d + 1) / 2]
    M[:, iu[0], iu[1]] = pairs
    M[:, iu[1], iu[0]] = pairs
    nu = torch.diagonal(M, dim1=1, dim2=2)                            # [3][d]
    g4 = (sums[2 + d:2 + 2 * d] / N).T
    normal = kinds == NORMAL
    Cp = torch.where(normal, b * b, (b - a) ** 2 / math.pi ** 2)
    s = torch.where(normal, b, (b - a) / 2)
    Chat = s[None, :, None] * M * s[None, None, :]
    lam, W = torch.linalg.eigh(Chat)
    lam, W = lam.flip(-1), W.flip(-1)
    return {'mean': m0, 'var': var, 'mean_gradient': (sums[2:2 + d] / N).T, 'nu': nu, 'nu_se': torch.sqrt(torch.clamp_min(g4 - nu * nu, 0.0) / N),
            'bound_ST': Cp[None, :] * nu / var[:, None], 'C': Chat, 'eigenvalues': lam, 'eigenvectors': W,
            'activity': torch.einsum('qk,qik->qi', lam, W * W)}
