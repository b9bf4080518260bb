"""The nested Monte Carlo estimator of hallthrusterpem_amd/information.py restated in numpy long double, brute force over the
pairs (i, j).  A restatement, not a test: tests/test_information_host.py and tests/test_information.py use it."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def group_slices(group_end):
    ge = [int(e) for e in group_end]
    return [slice(a, b) for a, b in zip([0] + ge[:-1], ge)]


def pairwise_d2(z_out, z_in, group_end):
    """d2[c][i][j] for c = 0 ... C (the last the union: the sum of the groups' d2 of the same pair), long double"""
    zo, zi = np.asarray(z_out, dtype=LD), np.asarray(z_in, dtype=LD)
    d2 = []
    for sl in group_slices(group_end):
        acc = np.zeros((zo.shape[0], zi.shape[0]), dtype=LD)
        for k in range(sl.start, sl.stop):                       # (no N x M x K intermediate)
            d = zo[:, k:k + 1] - zi[None, :, k]
            acc += d * d
        d2.append(acc)
    d2.append(sum(d2[1:], d2[0].copy()))
    return np.stack(d2)


def lse_ess(z_out, z_in, group_end):
    """(lse, ess, d2_min), each (N, C + 1): lse = m + log s1 - log M, ess = s1^2 / s2 and min_j d2, in long double"""
    lse, ess, low = [], [], []
    for d2 in pairwise_d2(z_out, z_in, group_end):               # one set at a time: (N, M) long doubles each
        l = -d2 / 2
        m = l.max(axis=1)
        s1, s2 = np.exp(l - m[:, None]).sum(axis=1), np.exp(2 * (l - m[:, None])).sum(axis=1)
        lse.append(m + np.log(s1) - np.log(LD(d2.shape[1])))
        ess.append(s1 * s1 / s2)
        low.append(d2.min(axis=1))
    return np.stack(lse, axis=1), np.stack(ess, axis=1), np.stack(low, axis=1)


def estimate(z_in_outer, eps, z_in_inner, group_end):
    """the whole estimator: {'eig', 'stderr', 'ess_median', 'ess_min': (C+1,), 'lse', 'ess', 'u', 'd2_min': (N, C+1)}"""
    z_out = np.asarray(z_in_outer, dtype=np.float64) + np.asarray(eps, dtype=np.float64)   # the observations are fp64 numbers
    eps = np.asarray(eps, dtype=LD)
    lse, ess, d2_min = lse_ess(z_out, z_in_inner, group_end)
    e2 = eps * eps
    half = np.stack([e2[:, sl].sum(axis=1) for sl in group_slices(group_end)] + [e2.sum(axis=1)], axis=1)
    u = -half / 2 - lse
    n = u.shape[0]
    return {'eig': u.mean(axis=0), 'stderr': u.std(axis=0, ddof=1) / np.sqrt(LD(n)) if n > 1 else np.full(u.shape[1], np.nan),
            'ess_median': np.median(ess, axis=0), 'ess_min': ess.min(axis=0), 'lse': lse, 'ess': ess, 'u': u, 'd2_min': d2_min}


def lse_bound(group_end, d2_min):
    """(N, C+1) bound on |lse - its long double value| for an fp64 evaluation by fma chains.  The sum of K_c non-negative squares
    carries a relative error of at most (K_c + 3) 2^-53 (a rounded difference, K_c rounded fmas, the halving exact); the error
    of term j enters lse weighted by exp(-(d2_j - d2_min) / 2) / s1 <= its share of the sum, so the d2 errors move lse by at most
    (K_c + 3) 2^-53 (d2_min / 2 + sum_j w_j (d2_j - d2_min) / 2) and x e^-x <= 1 bounds the tail by one unit.  With the roundings
    of the sums, the rescalings and m + log s1 - log M (a handful of units) and a factor 4 for the ulps of exp and log:
    2^-50 (K_c + 8) (1 + d2_min / 2)."""
    widths = [sl.stop - sl.start for sl in group_slices(group_end)]
    k = np.asarray(widths + [sum(widths)], dtype=np.float64)
    return 2.0 ** -50 * (k + 8.0) * (1.0 + 0.5 * np.asarray(d2_min, dtype=np.float64))


def closed_form_case(seed=0, n=2048, m=2048):
    """theta ~ N(0, 1), g_k = a_k theta, a = (1, 1, 1, 1, 2), unit sigma, groups {0, 1, 2} and {3, 4}: the exact gains are
    1/2 log(1 + sum a^2) = 1/2 log 4, 1/2 log 6 and (all five) 1/2 log 9.  Drawn in the order theta_outer, theta_inner, eps."""
    rng = np.random.default_rng(seed)
    a = np.array([1.0, 1.0, 1.0, 1.0, 2.0])
    t_out, t_in = rng.standard_normal(n), rng.standard_normal(m)
    eps = rng.standard_normal((n, a.size))
    exact = 0.5 * np.log([4.0, 6.0, 9.0])
    return t_out[:, None] * a, eps, t_in[:, None] * a, np.array([3, 5], dtype=np.int32), exact
