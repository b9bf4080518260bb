"""Tempered sequential Monte Carlo without a GPU: the two entry points of csrc/pem_smc.hip are declared, bound, built and exported
and refuse every malformed call before they look for a device; DeviceSMC refuses what it cannot run before it touches a device;
the numpy restatement of the launches (tests/smc_np.py) is the algorithm: it recovers a closed-form evidence and the masses of
two modes from prior draws, and every run has the stated properties."""
import ctypes as C
import re

import numpy as np
import pytest

import smc_cases as cases
import smc_np
from smc_cases import ROOT

STAGE, MOVE = 'pem_smc_stage_f64_dev', 'pem_smc_move_f64_dev'


def test_the_entry_points_are_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    for name, n_args in ((STAGE, 28), (MOVE, 23)):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header)
        assert m and len(m.group(1).split(',')) == n_args
        assert len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(_lib.load(), name)
    for macro, value in (('PEM_SMC_MAX_DIM', _lib.SMC_MAX_DIM), ('PEM_SMC_MAX_PARTICLES', _lib.SMC_MAX_PARTICLES),
                         ('PEM_SMC_BISECTIONS', _lib.SMC_BISECTIONS)):
        assert re.search(r'#define %s (\d+)' % macro, header).group(1) == str(value)
    assert _lib.SMC_MAX_DIM == 32 and _lib.SMC_MAX_PARTICLES >= 4096 and smc_np.BISECTIONS == _lib.SMC_BISECTIONS
    assert build.PKG / 'csrc' / 'pem_smc.hip' in build.SRCS


FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host
STAGE_ARRAYS = ('theta', 'loglik', 'logprior', 'beta', 'log_evidence', 'stage', 'L', 'prop', 'accept_count', 'accepted', 'flags',
                'moves_active', 'scratch', 'hist_beta', 'hist_ess', 'hist_accept', 'hist_dlogz')
MOVE_ARRAYS = ('theta', 'loglik', 'logprior', 'beta', 'stage', 'L', 'prop', 'prop_loglik', 'prop_logprior', 'accept_count',
               'moves_active')
NAN, INF = float('nan'), float('inf')


def _stage(R=2, N=8, d=3, seed=1, tau=0.5, scale=1.2, eps=1e-12, n_mcmc=3, history_len=8, record=False, **null):
    from hallthrusterpem_amd import _lib
    ptrs = [None if null.get(n) else FAKE for n in STAGE_ARRAYS]          # name=True: that array is NULL
    return _lib.load().pem_smc_stage_f64_dev(R, N, d, seed, tau, scale, eps, n_mcmc, *ptrs, history_len, FAKE if record else None, None)


def _move(R=2, N=8, d=3, seed=1, tau=0.5, scale=1.2, eps=1e-12, n_mcmc=3, move=1, propose=1, record=False, **null):
    from hallthrusterpem_amd import _lib
    ptrs = [None if null.get(n) else FAKE for n in MOVE_ARRAYS]
    return _lib.load().pem_smc_move_f64_dev(R, N, d, seed, tau, scale, eps, n_mcmc, move, propose, *ptrs, FAKE if record else None, None)


COMMON_BAD = [dict(R=0), dict(N=0), dict(N=1), dict(N=-4), dict(N=16385), dict(d=0), dict(d=-1), dict(d=33), dict(tau=0.0),
              dict(tau=1.0), dict(tau=-0.5), dict(tau=1.5), dict(tau=NAN), dict(scale=0.0), dict(scale=-1.0), dict(scale=NAN),
              dict(scale=INF), dict(eps=-1e-12), dict(eps=NAN), dict(n_mcmc=0), dict(R=1 << 20, N=8192)]


@pytest.mark.parametrize('bad', COMMON_BAD + [dict(history_len=0)] + [{n: True} for n in STAGE_ARRAYS])
def test_malformed_stage_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _stage(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_smc_stage' in _lib.load().pem_last_error()


@pytest.mark.parametrize('bad', COMMON_BAD + [dict(move=0), dict(move=4), dict(move=3, propose=1), dict(n_mcmc=1, move=1, propose=1)]
                         + [{n: True} for n in MOVE_ARRAYS])
def test_malformed_move_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _move(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_smc_move' in _lib.load().pem_last_error()


def test_well_formed_calls_get_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    for call, last in ((_stage, {}), (_move, dict(propose=0))):          # (the last move of a stage proposes nothing)
        assert call() == _lib.PEM_ERR_NO_DEVICE
        assert call(R=1, N=2, d=1, n_mcmc=1, **last) == _lib.PEM_ERR_NO_DEVICE
        assert call(N=16384, d=32, eps=0.0, record=True) == _lib.PEM_ERR_NO_DEVICE
    assert _move(move=3, propose=0) == _lib.PEM_ERR_NO_DEVICE


def _f(theta):
    raise AssertionError('the callables must not be called')


@pytest.mark.parametrize('kw, match', [
    (dict(theta0=np.zeros((8, 3)), tau=0.0), r'tau must be in \(0, 1\)'),
    (dict(theta0=np.zeros((8, 3)), tau=1.0), r'tau must be in \(0, 1\)'),
    (dict(theta0=np.zeros((8, 3)), tau=float('nan')), r'tau must be in \(0, 1\)'),
    (dict(theta0=np.zeros((8, 3)), n_mcmc=0), 'n_mcmc'),
    (dict(theta0=np.zeros((8, 3)), n_mcmc=1.5), 'n_mcmc'),
    (dict(theta0=np.zeros((8, 3)), scale=0.0), 'scale > 0'),
    (dict(theta0=np.zeros((8, 3)), eps=-1.0), 'eps >= 0'),
    (dict(theta0=np.zeros((1, 3))), '2 <= N <= 16384'),
    (dict(theta0=np.zeros((16385, 2))), '2 <= N <= 16384'),
    (dict(theta0=np.zeros((8, 33))), '1 to 32 parameters'),
    (dict(theta0=np.zeros(3)), r'\(R, N, d\)'),
    (dict(theta0=np.zeros((8, 3)), n_populations=2), r'\(R, N, d\)'),
    (dict(theta0=np.zeros((3, 8, 3)), n_populations=2), r'\(R, N, d\)'),
    (dict(theta0=np.full((8, 3), np.inf)), 'not finite'),
    (dict(theta0=np.zeros((8, 3)), device='cpu'), 'GPU only'),
    (dict(theta0='tensor'), 'GPU only'),                                  # a CPU tensor as the start points
])
def test_the_driver_refuses_what_it_cannot_run_before_touching_a_device(kw, match, monkeypatch):
    import torch
    from hallthrusterpem_amd.calibration import DeviceSMC
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    if isinstance(kw['theta0'], str):
        kw = dict(kw, theta0=torch.zeros((8, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match=match):
        DeviceSMC(_f, _f, **kw)
    with pytest.raises(ValueError, match="'sobol' or 'mc'"):
        DeviceSMC.prior_draws(('c0', 'c1'), method='lhs')


# --------------------------------------------------------------------------------------------- the restatement is the algorithm
R_HOST, N_HOST = 16, 1024


@pytest.fixture(scope='module')
def gauss_run():
    return smc_np.run(cases.gauss_loglik, cases.gauss_logprior, cases.gauss_starts(R_HOST, N_HOST), seed=3, tau=0.5, n_mcmc=3)


@pytest.fixture(scope='module')
def modes_run():
    return smc_np.run(cases.modes_loglik, cases.modes_logprior, cases.modes_starts(R_HOST, N_HOST), seed=4, tau=0.5, n_mcmc=3)


def test_the_restatement_recovers_a_closed_form_evidence(gauss_run):
    """d = 2, prior N(0, 3^2 I), likelihood exp(-|x - (1, -2)|^2 / (2 0.3^2)): log Z = -4.8901 exactly.  R = 16 populations of
    N = 1024 from prior draws reach beta = 1 in 4 or 5 stages; observed mean log_evidence -4.8843, standard error of the mean
    (population spread / sqrt(R)) 0.0184: 0.3 standard errors off, so the O(1 / N) bias is below the standard error at N = 1024
    and N was not raised."""
    st = gauss_run
    cases.check_run(st, 0.5, N_HOST)
    le = st['log_evidence']
    se = le.std(ddof=1) / np.sqrt(R_HOST)
    print(f'log Z exact {cases.GAUSS_LOG_Z:.4f} mean {le.mean():.4f} standard error {se:.4f} stages {st["stage"].tolist()}')
    assert abs(le.mean() - cases.GAUSS_LOG_Z) <= 5.0 * se, (le.mean(), cases.GAUSS_LOG_Z, se)
    assert se < 0.05                                                      # (the test can tell a wrong evidence from a right one)
    # the particles are the posterior N(m s0^2 / (s0^2 + s^2), s0^2 s^2 / (s0^2 + s^2)): pooled mean within 5 standard errors
    post_mean = cases.LIK_MEAN * cases.PRIOR_STD ** 2 / (cases.PRIOR_STD ** 2 + cases.LIK_STD ** 2)
    means = st['theta'].mean(axis=1)
    assert np.all(np.abs(means.mean(axis=0) - post_mean) <= 5.0 * means.std(axis=0, ddof=1) / np.sqrt(R_HOST))
    acc = st['hist_accept'][0, :int(st['stage'][0])]
    assert np.all((acc > 0.05) & (acc < 0.95)), acc                       # it moved, and it refused
    assert not st['flags'].any() and not st['moves_active'].any()


def test_the_restatement_finds_both_modes_from_prior_draws(modes_run):
    """likelihood 0.7 N(a, 0.5^2 I) + 0.3 N(b, 0.5^2 I), modes 12 standard deviations apart, uniform prior on [-10, 10]^2: the share
    of the particles in the heavier mode is 0.7.  Observed 0.6951 with standard error 0.0079 over the 16 populations."""
    st = modes_run
    cases.check_run(st, 0.5, N_HOST)
    share = (st['theta'][:, :, 0] < 0.0).mean(axis=1)
    se = share.std(ddof=1) / np.sqrt(R_HOST)
    print(f'share of the heavier mode {share.mean():.4f} standard error {se:.4f}')
    assert abs(share.mean() - cases.MASS_A) <= 5.0 * se, (share.mean(), se)
    assert se < 0.03
    assert np.all(np.abs(st['theta']) <= cases.BOX)                       # nothing left the support


@pytest.mark.parametrize('shape', cases.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['smooth', 'hostile'])
def test_the_launch_inputs_of_the_device_test_show_no_tie_in_the_restatement(shape, kind):
    """the decisions of tests/test_smc.py's three stages, taken by the restatement alone on the same seeds, for all seven shapes of
    that test and both value sources: no decision has its two sides within 4 ulp of log(u) (0 ties in every one of the 14 cases,
    about 98 000 decisions in each of the two at N = 16384), so a tie seen on the device comes from the device's last bits"""
    R, N, d = shape
    theta, loglik, logprior = cases.launch_inputs(R, N, d, kind)
    st = smc_np.new_state(theta, loglik, logprior, history_len=2)
    rng = np.random.default_rng(5)
    for _ in range(3):
        st, _ = smc_np.stage(st, cases.SEED, cases.TAU, 2.38 / np.sqrt(d), cases.EPS, cases.N_MCMC)
        for m in range(1, cases.N_MCMC + 1):
            ll, lp = cases.proposal_values(st['prop'], kind, rng)
            st, rec = smc_np.move(st, ll, lp, cases.SEED, cases.N_MCMC, m, propose_next=m < cases.N_MCMC)
            assert not cases.ties(rec).any()


def test_the_cumulative_weights_never_decrease():
    """the stated order of the scan: every level starts where the one below ends"""
    rng = np.random.default_rng(6)
    for N in (2, 65, 1025, 5000, 16384):
        w = rng.random(N) * 10.0 ** rng.uniform(-300, 0, size=N)
        w[rng.random(N) < 0.3] = 0.0
        w[rng.integers(N)] = 1.0
        C = smc_np.cumulative(w)
        assert np.all(np.diff(C) >= 0.0) and abs(C[-1] - w.sum()) <= 1e-12 * w.sum()
        anc, _ = smc_np.ancestors(w, 0.37)
        assert np.all(w[anc] > 0.0) and np.all(np.diff(anc) >= 0)
