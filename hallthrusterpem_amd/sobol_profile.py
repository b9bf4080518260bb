"""First-order and total Sobol' indices of the whole 91-angle j_ion profile: the fused Saltelli launch of
csrc/pem_saltelli_profile.hip and the arithmetic that turns its sums into indices (`drivers.sobol_profile` is the driver).

  profile_sums   one launch: the sums of the estimator terms per angle, for base samples first_index .. first_index + n_base - 1
  indices        S1, ST, their standard errors, mean, var and the variance-weighted aggregates GS1, GST from those sums

Rows of the sums, c_k the centre of angle k, f = j_ion or log10 j_ion:
    0        sum (fA - c) + (fB - c)                1        sum (fA - c)^2 + (fB - c)^2
    2 + 4 j  sum t1,  t1 = (fB - c)(fAB_j - fA)     3 + 4 j  sum t1^2
    4 + 4 j  sum t2,  t2 = (fA - fAB_j)^2           5 + 4 j  sum t2^2
"""
import ctypes as C

import numpy as np

from . import _lib, constants

NORMS = {'none': 0, 'log10': 1}
DEFAULT_BLOCKS = 512      # two workgroups per CU (72 KB of LDS each)


def n_rows(nv: int) -> int:
    return 2 + 4 * nv


def profile_sums(design, varied, n_base: int, centre=None, first_index: int = 0, norm: str = 'log10', radius: float = 1.0,
                 n_blocks: int | None = None, method: str = 'mc', scramble: bool = True, device=None, stream=None):
    """One launch of `pem_saltelli_profile_f64_dev` / `pem_saltelli_profile_qmc_f64_dev`: base samples first_index ..
    first_index + n_base - 1 of `design` (rows A and B exactly those of `fp32.saltelli_sums`), the coupled fp64 model on A, B and
    AB_j for the inputs `varied` (indices 0..14, at most 15, possibly none), the 91-angle profile of every evaluation formed on chip.
    `centre`: 91 numbers (a tensor on the device is used in place) or None for zeros; norm 'log10' (the YAML's norm of j_ion) or
    'none'; method 'mc' or 'sobol' as in `Design.fill`.
    Returns (sums [2 + 4 nv][91] float64 CUDA tensor, rows as in the module docstring; flags [2] int64: non-physical thruster
    results and invalid plume rows over all n_base (nv + 2) evaluations)."""
    if method not in ('mc', 'sobol'):
        raise ValueError(f"profile_sums: method must be 'mc' or 'sobol', got '{method}'")
    if norm not in NORMS:
        raise ValueError(f"profile_sums: norm must be 'log10' or 'none', got '{norm}'")
    if n_base < 0 or first_index < 0:
        raise ValueError('profile_sums: n_base and first_index must not be negative')
    if method == 'sobol' and first_index + n_base > 1 << 30:
        raise ValueError(f"the Sobol' sequence has 2^30 points: first_index + n_base = {first_index + n_base}")
    if not radius > 0:
        raise ValueError(f'profile_sums: radius must be positive, got {radius}')
    varied = np.ascontiguousarray(varied, dtype=np.int32).reshape(-1)
    nv = int(varied.size)
    if nv > 15:
        raise ValueError(f'profile_sums: at most 15 varied inputs, got {nv}')
    import torch
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    n_blocks = DEFAULT_BLOCKS if n_blocks is None else int(n_blocks)
    if centre is not None:
        centre = torch.as_tensor(centre, dtype=torch.float64).to(dev).contiguous()
        if centre.shape != (_lib.NANGLE,):
            raise ValueError(f'profile_sums: centre holds one number per angle ({_lib.NANGLE}), got {tuple(centre.shape)}')
    partial = torch.empty((max(n_blocks, 1), n_rows(nv), _lib.NANGLE), dtype=torch.float64, device=dev)
    flags = torch.empty((max(n_blocks, 1), 2), dtype=torch.int64, device=dev)
    ptr = lambda arr: C.c_void_p(arr.ctypes.data)                                               # noqa: E731
    with torch.cuda.device(dev), torch.cuda.stream(s):
        lib = _lib.load()
        tail = (ptr(design.kind), ptr(design.a), ptr(design.b), nv, ptr(varied) if nv else None, NORMS[norm],
                C.c_void_p(centre.data_ptr()) if centre is not None else None, constants.TORR_2_PA, float(radius),
                C.c_void_p(partial.data_ptr()), C.c_void_p(flags.data_ptr()), n_blocks, C.c_void_p(s.cuda_stream))
        if method == 'sobol':
            _lib.check(lib.pem_saltelli_profile_qmc_f64_dev(int(n_base), int(first_index), design.seed, design.stream, int(bool(scramble)), *tail))
        else:
            _lib.check(lib.pem_saltelli_profile_f64_dev(int(n_base), int(first_index), design.seed, design.stream, *tail))
        return partial.sum(dim=0), flags.sum(dim=0)


def indices(sums, n_base: int, centre):
    """The estimates from the [2 + 4 d][91] sums over N = n_base base samples and the centre c [91] they were taken about (tensors):
        mean_k = c_k + row0_k / 2N              var_k = row1_k / 2N - (row0_k / 2N)^2
        S1_kj  = (row(2+4j)_k / N) / var_k      ST_kj = (row(4+4j)_k / N) / (2 var_k)
        S1_se  = sqrt((row(3+4j)/N - (row(2+4j)/N)^2) / N) / var_k,  ST_se likewise from rows 5+4j, 4+4j over 2 var_k
        GS1_j  = sum_k row(2+4j)_k / N / sum_k var_k        GST_j = sum_k row(4+4j)_k / (2N) / sum_k var_k
    (Saltelli et al. 2010 and Jansen 1999 per angle; the aggregates are the variance-weighted means over the profile of Lamboni et
    al. 2011 and Gamboa et al. 2014.)  Where var_k == 0 the indices are the division's own NaN.
    Returns {'S1', 'ST', 'S1_se', 'ST_se': [91][d];  'mean', 'var': [91];  'GS1', 'GST': [d]}."""
    import torch
    sums = torch.as_tensor(sums, dtype=torch.float64)
    centre = torch.as_tensor(centre, dtype=torch.float64).to(sums.device)
    N = float(n_base)
    m0 = sums[0] / (2 * N)
    var = sums[1] / (2 * N) - m0 * m0
    t1, t1sq, t2, t2sq = (sums[2 + r::4] / N for r in range(4))                      # [d][91] each: the means of the terms
    se = lambda m, msq: torch.sqrt(torch.clamp_min(msq - m * m, 0.0) / N)          # noqa: E731
    return {'S1': (t1 / var).T, 'ST': (t2 / (2 * var)).T, 'S1_se': (se(t1, t1sq) / var).T, 'ST_se': (se(t2, t2sq) / (2 * var)).T,
            'mean': centre + m0, 'var': var, 'GS1': t1.sum(dim=1) / var.sum(), 'GST': t2.sum(dim=1) / (2 * var.sum())}
