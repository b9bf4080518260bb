"""One set of interpolation node doubles.  The model is evaluated at surrogate.nodes (the training values Y), the kernel
interpolates with its LOBATTO_NODES / LOBATTO_INVDEN tables (csrc/pem_surrogate.hip), the numpy restatement uses
oracle/surrogate_np.nodes: all three are the correctly rounded doubles of -cos(pi j / (m - 1)), so that the interpolant goes
through its training values exactly."""
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from hallthrusterpem_amd import surrogate
from oracle import surrogate_np

SRC = Path(__file__).resolve().parents[1] / 'hallthrusterpem_amd' / 'csrc' / 'pem_surrogate.hip'
OFFSETS = {1: 0, 2: 3, 3: 8, 4: 17}


def _exact_nodes(level):
    import mpmath
    m = 2 ** level + 1
    with mpmath.workprec(400):
        return [-mpmath.cospi(mpmath.mpf(j) / (m - 1)) for j in range(m)]


def _kernel_table(name):
    body = re.search(name + r'\[34\] = \{(.*?)\};', SRC.read_text(), re.S).group(1)
    vals = [s.strip() for s in body.split(',')]
    return [float.fromhex(s) if 'x' in s else float(s) for s in vals]


def test_nodes_are_correctly_rounded_nested_and_antisymmetric():
    import mpmath
    for level in range(1, 5):
        x = surrogate.nodes(level)
        exact = _exact_nodes(level)
        assert x.dtype == np.float64 and x.size == 2 ** level + 1
        for j, (v, e) in enumerate(zip(x, exact)):
            # correctly rounded: both neighbouring doubles are farther from the exact value (cos(pi j / 2^l) is 0, +-1 or
            # irrational, so there are no ties)
            with mpmath.workprec(400):
                d = abs(mpmath.mpf(v) - e)
                for w in (np.nextafter(v, -2.0), np.nextafter(v, 2.0)):
                    assert d < abs(mpmath.mpf(float(w)) - e), (level, j)
        assert np.array_equal(x, -x[::-1]), level                       # antisymmetric
        assert x[(x.size - 1) // 2] == 0.0 and not np.signbit(x[(x.size - 1) // 2])
        if level > 1:
            assert np.array_equal(surrogate.nodes(level)[::2], surrogate.nodes(level - 1)), level     # nested
        assert np.array_equal(surrogate_np.nodes(level), x), level      # the restatement's nodes are the same doubles
    assert np.array_equal(surrogate.nodes(0), [0.0]) and np.array_equal(surrogate_np.nodes(0), [0.0])


def test_kernel_node_and_denominator_tables_are_those_doubles():
    nodes, invden = _kernel_table('LOBATTO_NODES'), _kernel_table('LOBATTO_INVDEN')
    assert len(nodes) == len(invden) == 34
    for level, off in OFFSETS.items():
        m = 2 ** level + 1
        x = surrogate.nodes(level)
        assert [v.hex() for v in nodes[off:off + m]] == [float(v).hex() for v in x], level
        fx = [Fraction(float(v)) for v in x]
        for j in range(m):
            p = Fraction(1)
            for i in range(m):
                if i != j:
                    p *= fx[j] - fx[i]
            assert invden[off + j] == float(1 / p), (level, j)           # Fraction -> float rounds to nearest


@pytest.mark.gpu
@pytest.mark.parametrize('outer', [False, True])
def test_one_hot_table_vanishes_exactly_at_the_other_nodes(outer):
    """A table whose values are one-hot at node i, evaluated at node j of surrogate.nodes: exactly 0.0 for j != i -- the
    product-form basis has the factor t - t_j = 0 exactly only when the kernel's node double IS the training node double --
    and 1 within m ulp at j = i.  outer: the level's dimension is an outer one (bases staged in LDS), the innermost is a
    level-1 dimension evaluated at its node -1 (basis (1, 0, 0) exactly)."""
    import ctypes as C
    import torch
    from hallthrusterpem_amd import _lib
    import hp_reference as hr
    lib = _lib.load()
    for level in range(1, 5):
        m = 2 ** level + 1
        x = surrogate.nodes(level)
        D = 2
        beta = (level, 1) if outer else (level, 0)
        rows = m * (3 if outer else 1)
        t = np.stack([x, np.full(m, -1.0)])
        dt = torch.from_numpy(np.ascontiguousarray(t)).cuda()
        got = np.empty((m, m))
        for c0 in range(0, m, 16):                                      # one output column per node, at most 16 per launch
            cols = list(range(c0, min(m, c0 + 16)))
            y = np.zeros((rows, len(cols)))
            for o, i in enumerate(cols):
                y[i * 3 if outer else i, o] = 1.0                       # (outer: the innermost node 0 of the row)
            idx, vals = hr.index_table([beta], [y])
            d_idx, d_val = torch.from_numpy(idx).cuda(), torch.from_numpy(vals).cuda()
            coef = torch.ones(1, dtype=torch.float64, device='cuda')
            out = torch.full((len(cols), m), np.nan, dtype=torch.float64, device='cuda')
            _lib.check(lib.pem_sparse_predict_f64_dev(m, D, 1, hr.ptr(d_idx), hr.ptr(coef), hr.ptr(d_val), len(cols), hr.ptr(dt), m,
                                                      hr.ptr(out), m, 2 if outer else 1, level,
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            got[cols] = out.cpu().numpy()                               # got[i][j]: basis i at node j
        off = got[~np.eye(m, dtype=bool)]
        assert np.all(off == 0.0), (level, outer, np.abs(off).max())
        assert np.all(np.abs(np.diag(got) - 1.0) <= m * np.spacing(1.0)), (level, outer, np.diag(got) - 1.0)
