"""Closed-form targets, exact draws of them and the statistics of the invariance tests (tests/test_stationarity_host.py on the numpy
restatements, tests/test_stationarity.py on the device).  A transition kernel that preserves its target turns exact draws of the
target into exact draws of the target, so after any number of steps every statistic below has the null distribution that its
closed-form standard error states: no autocorrelation enters and nothing is fitted to the code under test.  The draws come from
numpy's default_rng; nothing here uses the project's Philox or a device.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import smc_cases

D = 3
START_SEED = 20240911                                  # of every case's starts: default_rng([START_SEED, case number])

# ------------------------------------------------------------------------------------------------------------------ sizes
# (fixed by the mutant runs of tests/test_stationarity_host.py: the smallest at which every required mutant reaches |z| >= 10)
GAMMA = 0.1
DRAM_K, DRAM_STEPS, DRAM_SEED = 1 << 16, 8, 31
ENS_E, ENS_K, ENS_STEPS, ENS_SEED = 2048, 6, 16, 32
TEMP_R, TEMP_K, TEMP_STEPS, TEMP_SEED, TEMP_BETAS = 4096, 6, 8, 33, (1.0, 0.3, 0.05)
SMC_R, SMC_N, SMC_MOVES, SMC_SEED, SMC_BETAS = 512, 64, 6, 34, (0.25, 1.0)
SMC_L = np.array([[0.5, 0.0, 0.0], [0.2, 0.4, 0.0], [-0.1, 0.15, 0.45]])          # the fixed factor of the move's proposals

Z_DEVICE, Z_HOST, Z_MUTANT = 5.0, 4.0, 10.0


# ---------------------------------------------------------------------------------------------------------------- targets
def _lower_tail_moments(c):
    """raw moments 1 ... 4 of a standard normal kept above c: m_k = (k - 1) m_{k-2} + c^(k-1) lam, lam = phi(c) / (1 - Phi(c))"""
    from scipy.special import ndtr
    lam = np.exp(-0.5 * c * c) / np.sqrt(2.0 * np.pi) / ndtr(-c)
    m2 = 1.0 + c * lam
    return np.array([lam, m2, 2.0 * lam + c * c * lam, 3.0 * m2 + c ** 3 * lam])


class Target:
    """N(mean, chol chol^T) in d dimensions, with `edge` = (j, low) only where x_j > low.  `white` maps points to coordinates
    that are independent under the target: y = chol^-1 (x - mean), and with an edge y reflected so that its first coordinate runs
    along row j of chol -- a standard normal kept above c = (low - mean_j) / |chol_j|, beside d - 1 standard normals.  `moments`
    (4, d) are the raw moments 1 ... 4 of those coordinates."""

    def __init__(self, mean, chol, edge=None):
        self.mean, self.chol, self.edge = np.asarray(mean, dtype=np.float64), np.asarray(chol, dtype=np.float64), edge
        self.d = self.mean.size
        self.cov = self.chol @ self.chol.T
        self.prec = np.linalg.inv(self.cov)
        self.inv_chol = np.linalg.inv(self.chol)
        self.moments = np.tile(np.array([0.0, 1.0, 0.0, 3.0])[:, None], (1, self.d))
        self.reflect = np.eye(self.d)
        if edge is not None:
            j, low = edge
            row = self.chol[j]
            e = row / np.linalg.norm(row)
            v = e - np.eye(self.d)[0]
            if v @ v > 0.0:                            # Householder: symmetric, orthogonal, first row e
                self.reflect = np.eye(self.d) - 2.0 * np.outer(v, v) / (v @ v)
            self.moments[:, 0] = _lower_tail_moments((low - self.mean[j]) / np.linalg.norm(row))

    def inside(self, x):
        return np.ones(x.shape[:-1], dtype=bool) if self.edge is None else x[..., self.edge[0]] > self.edge[1]

    def draw(self, rng, n):
        """(n, d) exact draws (with an edge: by rejection, candidates in blocks, the first n kept)"""
        kept, have = [], 0
        while have < n:
            x = self.mean + rng.standard_normal((n + n // 64 + 64, self.d)) @ self.chol.T
            x = x[self.inside(x)]
            kept.append(x)
            have += len(x)
        return np.concatenate(kept)[:n]

    def logp(self, x):
        r = x - self.mean
        with np.errstate(all='ignore'):
            lp = -0.5 * np.einsum('...i,ij,...j->...', r, self.prec, r)
        return np.where(self.inside(x), lp, -np.inf)

    def white(self, x):
        return (x.reshape(-1, self.d) - self.mean) @ self.inv_chol.T @ self.reflect.T


# (A), (B): the Gaussian of tests/test_device_dram.py::_gaussian, without and with its hard edge t[:, 2] > -1
MU = np.array([1.0, -2.0, 0.5])
CHOL = np.array([[1.0, 0.0, 0.0], [0.8, 0.6, 0.0], [-0.3, 0.2, 0.4]])
EDGE = (2, -1.0)
TARGET_A = Target(MU, CHOL)
TARGET_B = Target(MU, CHOL, edge=EDGE)
DRAM_COV0 = (2.4 * 2.4 / D) * TARGET_A.cov

# (C): prior N(0, s0^2 I) times likelihood exp(-|x - m|^2 / (2 s^2))^beta with the constants of smc_cases.gauss_*; that problem
# has d = 2, and its m = (1, -2) gets a third coordinate 0.5 here
PRIOR_STD, LIK_STD = smc_cases.PRIOR_STD, smc_cases.LIK_STD
LIK_MEAN = np.append(smc_cases.LIK_MEAN, 0.5)


def gauss_loglik(x):
    return -0.5 * (((x - LIK_MEAN) / LIK_STD) ** 2).sum(axis=-1)


def gauss_logprior(x):
    return -0.5 * ((x / PRIOR_STD) ** 2).sum(axis=-1)


def tempered(beta):
    """prior x likelihood^beta: N(m (beta / s^2) / lam, I / lam), lam = 1 / s0^2 + beta / s^2"""
    lam = 1.0 / PRIOR_STD ** 2 + beta / LIK_STD ** 2
    return Target(LIK_MEAN * (beta / LIK_STD ** 2) / lam, np.eye(D) / np.sqrt(lam))


def dram_starts(target):
    return target.draw(np.random.default_rng([START_SEED, 1, target.edge is not None]), DRAM_K)


def ensemble_starts(target):
    rng = np.random.default_rng([START_SEED, 2, target.edge is not None])
    return target.draw(rng, ENS_E * ENS_K).reshape(ENS_E, ENS_K, D)


def tempering_starts():
    """(R, T, K, d): every (replica, rung) from its own tempered Gaussian"""
    rng = np.random.default_rng([START_SEED, 3])
    return np.stack([tempered(b).draw(rng, TEMP_R * TEMP_K).reshape(TEMP_R, TEMP_K, D) for b in TEMP_BETAS], axis=1)


def smc_starts(beta):
    rng = np.random.default_rng([START_SEED, 4, int(round(100 * beta))])
    return tempered(beta).draw(rng, SMC_R * SMC_N).reshape(SMC_R, SMC_N, D)


# ------------------------------------------------------------------------------------------------------------- statistics
def z_scores(target, x, units, pearson=False):
    """name -> z of the points x (..., d) under `target`: the mean of every independent coordinate w_i, of every w_i w_j (i <= j)
    and of q = |w|^2, each less its exact value over its exact standard error, which is that of ONE point over sqrt(units).
    `units` is the number of independent units the points come from: with K dependent walkers per unit every walker is used and
    the standard error is that of units independent points -- at least the true one, whatever the dependence (the mean over a
    unit has at most a single point's variance), so no |z| is larger than the null allows.  pearson (targets without an edge):
    Pearson's statistic of q over 16 equiprobable cells of the chi^2_d law, times units / points for the same reason, as the z
    whose two-sided normal tail is the statistic's chi^2_15 tail: it is within a limit exactly when the statistic is at or below
    the chi^2_15 quantile of that limit's tail probability."""
    from scipy.special import chdtr, chdtrc, ndtri
    w = target.white(np.asarray(x, dtype=np.float64))
    n, d = w.shape
    m1, m2, _, m4 = target.moments
    root = np.sqrt(float(units))
    z = {}
    for i in range(d):
        z[f'w{i}'] = (w[:, i].mean() - m1[i]) / np.sqrt(m2[i] - m1[i] ** 2) * root
        z[f'w{i}w{i}'] = ((w[:, i] ** 2).mean() - m2[i]) / np.sqrt(m4[i] - m2[i] ** 2) * root
        for j in range(i + 1, d):
            z[f'w{i}w{j}'] = ((w[:, i] * w[:, j]).mean() - m1[i] * m1[j]) / np.sqrt(m2[i] * m2[j] - (m1[i] * m1[j]) ** 2) * root
    q = (w * w).sum(axis=1)
    z['q'] = (q.mean() - m2.sum()) / np.sqrt((m4 - m2 ** 2).sum()) * root
    if pearson:
        assert target.edge is None
        cells = np.minimum((16.0 * chdtr(d, q)).astype(np.int64), 15)
        counts = np.bincount(cells, minlength=16).astype(np.float64)
        stat = ((counts - n / 16.0) ** 2 / (n / 16.0)).sum() * (units / float(n))
        z['pearson'] = float(-ndtri(0.5 * chdtrc(15, stat)))
    return {k: float(v) for k, v in z.items()}


def dram_z(theta, target):
    """the final points (K, d) of independent chains"""
    return z_scores(target, theta, DRAM_K, pearson=target.edge is None)


def ensemble_z(theta, target):
    """the final walkers (E, K, d): the unit is the ensemble"""
    return z_scores(target, theta, ENS_E, pearson=target.edge is None)


def tempering_z(theta):
    """the final walkers (R T, K, d), ensemble r T + t at rung t, each rung against its own Gaussian: the unit is the replica"""
    th = np.asarray(theta).reshape(TEMP_R, len(TEMP_BETAS), TEMP_K, D)
    return {f'beta={b:g} {k}': v for t, b in enumerate(TEMP_BETAS)
            for k, v in z_scores(tempered(b), th[:, t], TEMP_R, pearson=True).items()}


def smc_z(theta, beta):
    """the final particles (R, N, d): the unit is the population"""
    return z_scores(tempered(beta), theta, SMC_R, pearson=True)


def worst(z):
    """(name, |z|) of the largest |z|; a z that is not finite counts as infinite"""
    k = max(z, key=lambda name: abs(z[name]) if np.isfinite(z[name]) else np.inf)
    return k, (abs(z[k]) if np.isfinite(z[k]) else np.inf)


def report(label, z):
    k, v = worst(z)
    print(f'{label}: largest |z| {v:.2f} ({k})')
    return v
