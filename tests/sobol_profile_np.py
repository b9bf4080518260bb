"""numpy restatement of the Saltelli estimator for the 91-angle j_ion profile (drivers.sobol_profile, hallthrusterpem_amd/
sobol_profile.py, csrc/pem_saltelli_profile.hip).  TEST INFRASTRUCTURE ONLY.

With f the model ([inputs][n] -> [K][n], K outputs), A and B the two matrices of the design, AB_j = A with column varied[j] from B
(made here by a column copy), c a constant per output and N base samples:

    row 0        sum (fA - c) + (fB - c)                row 1        sum (fA - c)^2 + (fB - c)^2
    row 2 + 4 j  sum t1,  t1 = (fB - c)(fAB_j - fA)     row 3 + 4 j  sum t1^2
    row 4 + 4 j  sum t2,  t2 = (fA - fAB_j)^2           row 5 + 4 j  sum t2^2

    mean = c + row0 / 2N     var = row1 / 2N - (row0 / 2N)^2
    S1_j = (row(2+4j) / N) / var                        ST_j = (row(4+4j) / N) / (2 var)
    S1_se = sqrt((row(3+4j)/N - (row(2+4j)/N)^2) / N) / var,   ST_se the same from rows 5+4j, 4+4j over 2 var
    GS1_j = sum_k row(2+4j)_k / N / sum_k var_k         GST_j = sum_k row(4+4j)_k / (2N) / sum_k var_k

`terms` returns the per-sample terms of every row, their magnitudes and the roundings that form a term in the kernel; `sums` adds
them up (in np.longdouble on request); `indices` turns the rows into the estimates."""
import numpy as np

LD = np.longdouble


def n_rows(nv):
    return 2 + 4 * nv


def evaluate(f, A, B, varied):
    """fA, fB [K][n], fAB [nv][K][n]: the nv + 2 evaluations, the swapped blocks made by a column copy"""
    fA, fB = f(A), f(B)
    fAB = []
    for d in varied:
        X = A.copy()
        X[d] = B[d]
        fAB.append(f(X))
    return fA, fB, np.array(fAB).reshape(len(varied), *fA.shape)


def _rows(a, b, ab, c):
    """one (terms [K][n], magnitudes [K][n], roundings) per row of the partial, in its order.  The roundings of forming a term as
    the kernel forms it: va = a - c and vb = b - c round once each;
      va + vb: the difference a term came from and the sum, 2;  fma(va, va, vb * vb): vb enters squared (2), the product and the fma, 4;
      t1 = vb * (ab - a): two differences and the product, 3;  t1 * t1: t1 twice and the product, 7;
      t2 = dd * dd, dd = ab - a: 3;  t2 * t2: 7."""
    va, vb = a - c, b - c
    yield va + vb, np.abs(va) + np.abs(vb), 2
    yield va * va + vb * vb, va * va + vb * vb, 4
    for j in range(ab.shape[0]):
        dd = ab[j] - a
        t1, t2 = vb * dd, dd * dd
        yield t1, np.abs(t1), 3
        yield t1 * t1, t1 * t1, 7
        yield t2, t2, 3
        yield t2 * t2, t2 * t2, 7


def _conv(dtype):
    return lambda v: np.asarray(v, dtype=np.float64).astype(dtype)


def terms(fA, fB, fAB, centre, dtype=np.float64):
    """(t, mag, form): [rows][K][n] per-sample terms, their magnitudes as the error analysis of a sum wants them, and per row the
    roundings that form a term in the kernel"""
    conv = _conv(dtype)
    t, mag, form = zip(*_rows(conv(fA), conv(fB), conv(fAB), conv(centre)[:, None]))
    assert len(t) == n_rows(np.asarray(fAB).shape[0])
    return np.array(t), np.array(mag), np.array(form)


def sums_of(fA, fB, fAB, centre, dtype=np.float64):
    """(rows [rows][K], magnitudes [rows][K], form [rows]) from the evaluations, one row at a time"""
    conv = _conv(dtype)
    rows, mags, form = [], [], []
    for t, m, r in _rows(conv(fA), conv(fB), conv(fAB), conv(centre)[:, None]):
        rows.append(t.sum(axis=1))
        mags.append(m.sum(axis=1))
        form.append(r)
    return np.array(rows), np.array(mags), np.array(form)


def sums(f, A, B, varied, centre, dtype=np.float64):
    return sums_of(*evaluate(f, A, B, varied), centre, dtype=dtype)


def indices(rows, n, centre):
    """the estimates from the [rows][K] sums over n base samples taken about `centre` [K]: S1, ST, S1_se, ST_se [K][nv]; mean, var
    [K]; GS1, GST [nv]"""
    rows = np.asarray(rows)
    m0 = rows[0] / (2 * n)
    var = rows[1] / (2 * n) - m0 * m0
    t1, t1sq, t2, t2sq = (rows[2 + r::4] / n for r in range(4))                  # [nv][K]
    with np.errstate(divide='ignore', invalid='ignore'):
        se1 = np.sqrt(np.maximum(t1sq - t1 * t1, 0) / n) / var
        seT = np.sqrt(np.maximum(t2sq - t2 * t2, 0) / n) / (2 * var)
        return {'mean': np.asarray(centre) + m0, 'var': var, 'S1': (t1 / var).T, 'ST': (t2 / (2 * var)).T, 'S1_se': se1.T, 'ST_se': seT.T,
                'GS1': t1.sum(axis=1) / var.sum(), 'GST': t2.sum(axis=1) / (2 * var.sum())}


def pilot_centre(fA, fB):
    """c = sum (fA + fB) / (2 n) over the pilot's evaluations (the pilot's row 0 over 2 n_pilot, its own centre zero)"""
    return (fA + fB).sum(axis=1) / (2 * fA.shape[1])
