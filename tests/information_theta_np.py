"""The conditional nest of hallthrusterpem_amd/information.py (`about=`: the gain about a subset A of the inputs) restated in
numpy long double, brute force over the rows (i, l).  A restatement, not a test: tests/test_information_theta_host.py and
tests/test_information_theta.py use it, on top of tests/information_np.py (the joint estimator)."""
import numpy as np

import information_np as inf

LD = inf.LD


def conditional_d2(z_out, z_cond, group_end):
    """d2c[c][i][l] for c = 0 ... C (the last the union: the sum of the groups' d2c of the same row), long double.
    z_out (N, K) the observations, z_cond (N, L, K) the fp64 standardised predictions of every outer draw's own set."""
    zo, zc = np.asarray(z_out, dtype=LD), np.asarray(z_cond, dtype=LD)
    d2 = []
    with np.errstate(invalid='ignore', over='ignore'):
        for sl in inf.group_slices(group_end):
            acc = np.zeros(zc.shape[:2], dtype=LD)
            for k in range(sl.start, sl.stop):
                d = zo[:, None, k] - zc[:, :, k]
                acc += d * d
            d2.append(acc)
        d2.append(sum(d2[1:], d2[0].copy()))
    return np.stack(d2)


def conditional_lse(z_out, z_cond, group_end):
    """(lse_cond, ess_cond, used, d2_min): (N, C+1) long double, (N,) int and (N, C+1): a row l is used iff its union d2c is
    finite AS AN FP64 NUMBER (the launch's test; the long double sum could stay finite where the fp64 one overflows, which no
    test here approaches); lse = logmeanexp_l(-d2c / 2) and ess = s1^2 / s2 over the used rows, NaN where used = 0; d2_min the
    smallest used d2c (for information_np.lse_bound)"""
    d2 = conditional_d2(z_out, z_cond, group_end)
    with np.errstate(invalid='ignore', over='ignore'):
        use = np.isfinite(d2[-1].astype(np.float64))                                           # (N, L)
    used = use.sum(axis=1)
    n, sets = d2.shape[1], d2.shape[0]
    lse, ess, low = (np.full((n, sets), np.nan, dtype=LD) for _ in range(3))
    for i in range(n):
        if not used[i]:
            continue
        l = -d2[:, i, use[i]] / 2                                                              # (C+1, used)
        m = l.max(axis=1, keepdims=True)
        s1, s2 = np.exp(l - m).sum(axis=1), np.exp(2 * (l - m)).sum(axis=1)
        lse[i] = m[:, 0] + np.log(s1) - np.log(LD(used[i]))
        ess[i] = s1 * s1 / s2
        low[i] = d2[:, i, use[i]].min(axis=1)
    return lse, ess, used, low


def noise_norms(eps, group_end):
    e2 = np.asarray(eps, dtype=LD) ** 2
    return np.stack([e2[:, sl].sum(axis=1) for sl in inf.group_slices(group_end)] + [e2.sum(axis=1)], axis=1)


def mean_stderr(u):
    n = u.shape[0]
    return u.mean(axis=0), u.std(axis=0, ddof=1) / np.sqrt(LD(n)) if n > 1 else np.full(u.shape[1], np.nan)


def estimate(z_in_outer, eps, z_in_inner, z_cond, group_end):
    """the whole estimator: information_np.estimate's joint part (over every draw given) plus 'lse_cond', 'ess_cond', 'used',
    'd2c_min', 'u_about' = lse_cond - lse, 'u_rest' = -|eps_c|^2 / 2 - lse_cond (per draw, (N, C+1)) and the means and standard
    errors 'eig_about', 'stderr_about', 'eig_rest', 'stderr_rest', 'ess_cond_median' over the draws with used > 0, over which
    'eig' and 'stderr' are then taken too; 'dropped_conditional' counts the others"""
    out = inf.estimate(z_in_outer, eps, z_in_inner, group_end)
    z_out = np.asarray(z_in_outer, dtype=np.float64) + np.asarray(eps, dtype=np.float64)
    lse_c, ess_c, used, low = conditional_lse(z_out, z_cond, group_end)
    u_about, u_rest = lse_c - out['lse'], -noise_norms(eps, group_end) / 2 - lse_c
    good = used > 0
    out.update(lse_cond=lse_c, ess_cond=ess_c, used=used, d2c_min=low, u_about=u_about, u_rest=u_rest, dropped_conditional=int((~good).sum()),
               ess_cond_median=np.median(ess_c[good], axis=0))
    out['eig_about'], out['stderr_about'] = mean_stderr(u_about[good])
    out['eig_rest'], out['stderr_rest'] = mean_stderr(u_rest[good])
    if not good.all():
        out['eig'], out['stderr'] = mean_stderr(out['u'][good])
    return out


A = np.array([1.0, 1.0, 1.0, 1.0, 2.0])
B = np.array([0.5, -1.0, 2.0, 0.0, 1.0])
GROUP_END = np.array([3, 5], dtype=np.int32)


def closed_form_exact():
    """theta, eta ~ N(0, 1), g = a theta + b eta, unit noise: y | theta ~ N(a theta, I + b b^T) and y ~ N(0, I + a a^T + b b^T), so
    EIG_theta = 1/2 [log det(I + a a^T + b b^T) - log det(I + b b^T)]; EIG_joint = 1/2 log det(I + a a^T + b b^T); on the sets
    {0, 1, 2}, {3, 4} and all five.  Returns (about, joint, rest = joint - about), each (3,)."""
    about, joint = [], []
    for idx in ([0, 1, 2], [3, 4], [0, 1, 2, 3, 4]):
        a, b, eye = A[idx], B[idx], np.eye(len(idx))
        full = np.linalg.slogdet(eye + np.outer(a, a) + np.outer(b, b))[1]
        about.append(0.5 * (full - np.linalg.slogdet(eye + np.outer(b, b))[1]))
        joint.append(0.5 * full)
    about, joint = np.array(about), np.array(joint)
    return about, joint, joint - about


def closed_form_case(seed=0, n=2048, m=2048, l=256):
    """the case of `closed_form_exact`, drawn in the order theta_outer, eta_outer, theta_inner, eta_inner, eps, eta_conditional:
    (z_in_outer (n, 5), eps, z_in_inner (m, 5), z_cond (n, l, 5), group_end)"""
    rng = np.random.default_rng(seed)
    t_out, e_out, t_in, e_in = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    eps = rng.standard_normal((n, A.size))
    e_cond = rng.standard_normal((n, l))
    z_cond = t_out[:, None, None] * A + e_cond[:, :, None] * B
    return t_out[:, None] * A + e_out[:, None] * B, eps, t_in[:, None] * A + e_in[:, None] * B, z_cond, GROUP_END
