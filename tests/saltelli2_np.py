"""numpy restatement of the second-order Saltelli estimator (drivers.sobol_indices(second_order=True), csrc/pem_saltelli2.hip).
TEST INFRASTRUCTURE ONLY.

With f the model ([15][n] -> [3][n]), A and B the two matrices of the design, AB_j = A with column varied[j] from B, BA_j = B with
column varied[j] from A (both made here by a column copy), c a constant per QoI and N base samples:

    rows 0, 1                       sum fA + fB,  sum fA^2 + fB^2
    rows 2 + 2 j, 3 + 2 j           sum fB (fAB_j - fA),  sum (fA - fAB_j)^2
    rows 2 + 2 nv + 2 j, + 1        sum fA (fBA_j - fB),  sum (fB - fBA_j)^2            (the mirror)
    row  2 + 4 nv                   D = sum (fA - c)(fB - c)
    rows 3 + 4 nv + p               C_ij = sum (fBA_i - c)(fAB_j - c),  i < j, p counting the pairs lexicographically

    mean = row0 / 2N   Var = row1 / 2N - mean^2   S1_j = row(2 + 2j) / N / Var   ST_j = row(3 + 2j) / N / (2 Var)
    S2_ij = (C_ij - D) / N / Var - S1_i - S1_j

`terms` returns the per-sample terms of every row, `sums` adds them up (in np.longdouble on request) together with the sums of their
magnitudes and the roundings that form a term in the kernel, `indices` turns the rows into the estimates."""
import numpy as np

LD = np.longdouble


def n_rows(nv):
    return 3 + 4 * nv + nv * (nv - 1) // 2


def pairs(nv):
    return [(i, j) for i in range(nv) for j in range(i + 1, nv)]


def evaluate(f, A, B, varied):
    """fA, fB [3][n], fAB, fBA [nv][3][n]: the 2 nv + 2 evaluations, the swapped blocks made by a column copy"""
    fA, fB = f(A), f(B)
    fAB, fBA = [], []
    for d in varied:
        X = A.copy()
        X[d] = B[d]
        fAB.append(f(X))
        X = B.copy()
        X[d] = A[d]
        fBA.append(f(X))
    return fA, fB, np.array(fAB).reshape(len(varied), *fA.shape), np.array(fBA).reshape(len(varied), *fA.shape)


def terms(fA, fB, fAB, fBA, centre, dtype=np.float64):
    """(t, mag, form): [rows][3][n] per-sample terms, their magnitudes as the error analysis of a sum wants them (|a| + |b| for
    a + b, |b| |ab - a| for b (ab - a)), and per row the roundings that form a term in the kernel:
      a + b: 1;  fma(a, a, b * b): 2;  b * (ab - a): the difference and the product, 2;  (a - ab)^2: the difference enters squared
      and the product rounds, 3;  (x - c)(y - c): two differences and the product, 3."""
    conv = (lambda v: np.asarray(v, dtype=object)) if dtype is object else (lambda v: np.asarray(v, dtype=np.float64).astype(dtype))
    a, b, ab, ba = (conv(v) for v in (fA, fB, fAB, fBA))                      # (dtype=object: exact arithmetic on fractions.Fraction)
    c = conv(centre)[:, None]
    t, mag, form = zip(*_rows(a, b, ab, ba, c))
    assert len(t) == n_rows(ab.shape[0])
    return np.array(t), np.array(mag), np.array(form)


def _rows(a, b, ab, ba, c):
    """one (terms [3][n], magnitudes [3][n], roundings) per row of the partial, in its order"""
    nv = ab.shape[0]
    yield a + b, np.abs(a) + np.abs(b), 1
    yield a * a + b * b, a * a + b * b, 2
    for j in range(nv):
        yield b * (ab[j] - a), np.abs(b) * np.abs(ab[j] - a), 2
        yield (a - ab[j]) ** 2, (a - ab[j]) ** 2, 3
    for j in range(nv):
        yield a * (ba[j] - b), np.abs(a) * np.abs(ba[j] - b), 2
        yield (b - ba[j]) ** 2, (b - ba[j]) ** 2, 3
    yield (a - c) * (b - c), np.abs((a - c) * (b - c)), 3
    for i, j in pairs(nv):
        t = (ba[i] - c) * (ab[j] - c)
        yield t, np.abs(t), 3


def sums_of(fA, fB, fAB, fBA, centre, dtype=np.float64):
    """(rows [rows][3], magnitudes [rows][3], form [rows]) from the evaluations, one row at a time (a 20 000-sample design at
    nv = 15 in long double would otherwise hold 200 MB of terms)"""
    conv = (lambda v: np.asarray(v, dtype=object)) if dtype is object else (lambda v: np.asarray(v, dtype=np.float64).astype(dtype))
    a, b, ab, ba = (conv(v) for v in (fA, fB, fAB, fBA))
    rows, mags, form = [], [], []
    for t, m, r in _rows(a, b, ab, ba, conv(centre)[:, None]):
        rows.append(t.sum(axis=1))
        mags.append(m.sum(axis=1))
        form.append(r)
    return np.array(rows), np.array(mags), np.array(form)


def sums(f, A, B, varied, centre, dtype=np.float64):
    """(rows [rows][3], magnitudes [rows][3], form [rows]) of the design blocks A, B through the model f; dtype=LD sums in long
    double, dtype=object in whatever exact type f returns"""
    return sums_of(*evaluate(f, A, B, varied), centre, dtype=dtype)


def indices(rows, n, nv):
    """the estimates from the [rows][3] sums over n base samples: S1, ST, S1_mirror, ST_mirror [nv][3], S2 [3][nv][nv], mean, var [3]"""
    rows = np.asarray(rows)
    mean = rows[0] / (2 * n)
    var = rows[1] / (2 * n) - mean * mean
    first, mirror = rows[2:2 + 2 * nv], rows[2 + 2 * nv:2 + 4 * nv]
    out = {'mean': mean, 'var': var, 'S1': first[0::2] / n / var, 'ST': first[1::2] / n / (2 * var),
           'S1_mirror': mirror[0::2] / n / var, 'ST_mirror': mirror[1::2] / n / (2 * var)}
    D, C = rows[2 + 4 * nv], rows[3 + 4 * nv:]
    S2 = np.zeros((rows.shape[1], nv, nv), dtype=rows.dtype)
    for p, (i, j) in enumerate(pairs(nv)):
        S2[:, i, j] = S2[:, j, i] = (C[p] - D) / n / var - out['S1'][i] - out['S1'][j]
    out['S2'] = S2
    return out


def pilot_centre(f, A, B):
    """c = sum (fA + fB) / (2 n) over the pilot's blocks A, B (the pilot's row 0 over 2 n_pilot)"""
    return (f(A) + f(B)).sum(axis=1) / (2 * A.shape[1])
