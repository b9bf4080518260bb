"""Inputs and closed-form problems shared by tests/test_smc_host.py and tests/test_smc.py.  TEST INFRASTRUCTURE ONLY."""
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]

TAU, N_MCMC, EPS, SEED = 0.5, 2, 1e-12, 20240607
ULP = 2.0 ** -52

# ---------------------------------------------------------------------------------------------- launch-by-launch inputs
SHAPES = [(1, 2, 1), (1, 64, 1), (2, 65, 2), (1, 130, 17), (1, 1025, 3), (1, 16384, 2), (3, 257, 32)]


SPREAD = 1.2e3


def launch_inputs(R, N, d, kind, seed=SEED):
    """theta (R, N, d), loglik, logprior (R, N) of a first stage launch.  The finite log likelihoods lie in [-200, 0] (-1.5 chi^2_d:
    beyond -200 is out of reach of these sizes; the hostile ones are clipped to 100 below their largest) except the one hostile
    particle 1e3 above the rest, and `proposal_values` hands out values in [-40, 0] later: every population of the three stages has
    its finite log likelihoods within SPREAD = 1.2e3 of each other, which the ESS bound of tests/test_smc.py leans on and that test
    asserts before every stage launch.  'hostile': a
    tenth of the log likelihoods NaN / -inf / +inf, one particle ahead of the rest by 1e3 in log, the first population's finite
    values all equal when there are several populations; N = 2: one of the two NaN."""
    rng = np.random.default_rng([seed, R, N, d, 0 if kind == 'smooth' else 1])
    theta = rng.standard_normal((R, N, d)) * (10.0 ** rng.uniform(-2, 2, size=d))
    loglik = -0.5 * (rng.standard_normal((R, N, d)) ** 2).sum(axis=2) * 3.0
    logprior = -0.5 * (rng.standard_normal((R, N)) ** 2)
    if kind == 'hostile' and N > 2:
        for r in range(R):
            if R > 1 and r == 0:
                loglik[r] = -7.25                                         # ties everywhere: ESS(1) = N, one stage to beta = 1
            else:
                loglik[r] = np.maximum(loglik[r], loglik[r].max() - 100.0)
                loglik[r, rng.integers(N)] = loglik[r].max() + 1e3        # dominates by 1e3
            bad = rng.choice(N, size=max(1, N // 10), replace=False)
            bad = bad[loglik[r, bad] < loglik[r].max()]                   # (the dominating particle stays)
            loglik[r, bad] = rng.choice([np.nan, -np.inf, np.inf], size=bad.size)
    if kind == 'hostile' and N == 2:
        loglik[:, 0] = np.nan
    return theta, loglik, logprior


def proposal_values(prop, kind, rng):
    """log likelihood (in [-40, 0] for every d) and log prior 'evaluated' at the proposals (R, N, d): smooth functions of the
    point; 'hostile' sets a tenth of each to NaN / +-inf"""
    with np.errstate(all='ignore'):
        s = prop / np.maximum(np.abs(prop).max(axis=(0, 1)), 1e-300)
        ll = -40.0 * (s ** 2).mean(axis=2)
        lp = -0.5 * (s.sum(axis=2) ** 2)
    if kind == 'hostile':
        for a in (ll, lp):
            bad = rng.random(a.shape) < 0.1
            a[bad] = rng.choice([np.nan, -np.inf, np.inf], size=int(bad.sum()))
    return ll, lp


def ties(rec, ulps=4):
    """decisions whose two sides agree to within `ulps` ulp of log(u): (R, N) bool"""
    with np.errstate(all='ignore'):
        return np.abs(rec['lhs'] - rec['rhs']) <= ulps * ULP * np.abs(rec['lhs'])


# ---------------------------------------------------------------------------------------------- closed forms, d = 2
PRIOR_STD, LIK_STD, LIK_MEAN = 3.0, 0.3, np.array([1.0, -2.0])
# integral of N(x; 0, s0^2) exp(-(x - m)^2 / (2 s^2)) dx = sqrt(s^2 / (s0^2 + s^2)) exp(-m^2 / (2 (s0^2 + s^2))), per coordinate
GAUSS_LOG_Z = float(np.log(LIK_STD ** 2 / (PRIOR_STD ** 2 + LIK_STD ** 2)) - (LIK_MEAN ** 2).sum() / (2.0 * (PRIOR_STD ** 2 + LIK_STD ** 2)))


def gauss_starts(R, N, seed=11):
    return np.random.default_rng(seed).standard_normal((R, N, 2)) * PRIOR_STD


def gauss_loglik(x):
    return -0.5 * (((x - LIK_MEAN) / LIK_STD) ** 2).sum(axis=-1)


def gauss_logprior(x):
    return -0.5 * ((x / PRIOR_STD) ** 2).sum(axis=-1) - 2.0 * np.log(PRIOR_STD * np.sqrt(2.0 * np.pi))


BOX, MODE_A, MODE_B, MODE_STD, MASS_A = 10.0, np.array([-3.0, 0.5]), np.array([3.0, -0.5]), 0.5, 0.7


def modes_starts(R, N, seed=12):
    return np.random.default_rng(seed).uniform(-BOX, BOX, size=(R, N, 2))


def modes_loglik(x):
    """log(0.7 N(x; a, s^2 I) + 0.3 N(x; b, s^2 I)) up to a constant: two modes 12 s apart, masses 0.7 and 0.3"""
    qa = -0.5 * (((x - MODE_A) / MODE_STD) ** 2).sum(axis=-1) + np.log(MASS_A)
    qb = -0.5 * (((x - MODE_B) / MODE_STD) ** 2).sum(axis=-1) + np.log(1.0 - MASS_A)
    return np.logaddexp(qa, qb)


def modes_logprior(x):
    inside = (np.abs(x) <= BOX).all(axis=-1)
    return np.where(inside, -np.log((2.0 * BOX) ** 2), -np.inf)


def check_run(st, tau, N):
    """what holds for every run that reached beta = 1: per population the betas increase strictly and end at exactly 1, the ESS
    of every stage but the last is at tau N within the bisection's resolution (2^-52 in beta x a spread of the log likelihoods
    that the tempering keeps far below 1e6: 1e-9 N is generous), and the increments add up to log_evidence"""
    for r in range(st['theta'].shape[0]):
        n = int(st['stage'][r])
        b = st['hist_beta'][r, :n]
        assert n >= 1 and b[-1] == 1.0 and st['beta'][r] == 1.0, (r, b)
        assert np.all(np.diff(np.concatenate([[0.0], b])) > 0.0), (r, b)
        assert np.all(np.abs(st['hist_ess'][r, :n - 1] - tau * N) <= 1e-9 * N), (r, st['hist_ess'][r, :n])
        assert st['hist_ess'][r, n - 1] >= tau * N - 1e-9 * N
        total = 0.0
        for inc in st['hist_dlogz'][r, :n]:
            total = total + inc
        assert total == st['log_evidence'][r], (r, total, st['log_evidence'][r])
