"""Replica exchange over the ensemble sampler on the MI355X: the launch against its numpy restatement (tests/tempering_np.py)
launch by launch, the driver pinned to DeviceEnsemble at one temperature and to itself under graph replay, on a two-mode target
(what tempering is for), on a target whose evidence is closed form, and on a SystemPosterior.

    python tests/test_tempering.py        prints the CPU deviations of the restatement that the margins below come from
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import tempering_np
from hallthrusterpem_amd._lib import ENSEMBLE_MAX_WALKERS

ARRAYS = ('beta', 'theta', 'loglik', 'logprior', 'prop', 'prop_loglik', 'prop_logprior', 'log_q', 'state', 'accepted', 'swap_attempts',
          'swap_accepted', 'trace', 'loglik_trace', 'logprior_trace', 'draws')
STATE = ('theta', 'loglik', 'logprior', 'prop', 'log_q', 'state', 'accepted', 'swap_attempts', 'swap_accepted', 'trace', 'loglik_trace',
         'logprior_trace')


# ------------------------------------------------------------------------------------------------------------ the kernel
def _launch(t, R, T, K, d, seed, a, fraction, g0, sigma, first, length, thin):
    import torch
    from hallthrusterpem_amd import _lib
    p = lambda n: C.c_void_p(t[n].data_ptr()) if t[n].numel() else None                          # noqa: E731
    _lib.check(_lib.load().pem_tempered_ensemble_step_f64_dev(R, T, K, d, seed, a, fraction, g0, sigma, p('beta'), first, length, thin,
                                                              *[p(n) for n in ARRAYS[1:]],
                                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _smooth(x):
    """a closed form: a narrow Gaussian likelihood and a wide Gaussian prior"""
    return -0.5 * np.sum((x - 0.5) ** 2, axis=-1) / 0.25, -0.5 * np.sum(x ** 2, axis=-1) / 9.0


def _hostile(rng, l_now, shape):
    """values that try every branch of the decision: ties with the walker's own value, NaN, +inf and -inf in l, -inf in pi"""
    ll = l_now + rng.normal(size=shape) * 2.0
    ll = np.where(rng.random(shape) < 0.15, l_now, ll)
    for value, share in ((np.nan, 0.08), (np.inf, 0.08), (-np.inf, 0.08)):
        ll[rng.random(shape) < share] = value
    lp = rng.normal(size=shape)
    lp[rng.random(shape) < 0.1] = -np.inf
    return ll, lp


@pytest.mark.gpu
@pytest.mark.parametrize('source', ['smooth', 'hostile'])
@pytest.mark.parametrize('R, T, K, d', [(1, 1, 2, 1), (1, 2, 4, 2), (2, 3, 4, 2), (1, 5, 8, 3), (1, 2, 34, 17),
                                        (2, 4, ENSEMBLE_MAX_WALKERS, 1), (1, 8, 260, 2)])
def test_tempering_kernel_matches_the_numpy_restatement_launch_by_launch(R, T, K, d, source):
    """The smallest shapes at which the half split, the odd ladder, the idle top, the replica stride, the dimension limit and the
    walker limit can each go wrong, and (1, 8, 260, 2), whose ladder the kernel walks three ensembles and three pairs at a time
    with a remainder of either.  25 launches (12 steps) with trace_first=1, trace_len=4, thin=2 and two guard rows of NaN, then the
    window moves to trace_first=12, trace_len=3, thin=1 with fresh buffers for 6 launches more; ladder linspace(1, 0, T), so the
    last temperature is beta = 0 and the first beta = 1; de_fraction 0.5 (K >= 4).  The test writes prop_loglik and prop_logprior
    itself: a closed form of the device's proposals, or hostile values (ties, NaN, +-inf in l, -inf in pi), which must never enter whatever beta
    is.  The numpy state is re-read from the device before every launch.  Given the device's g (the library's normcdfinv), theta,
    l, pi, the proposals, log q, state, the move and swap counters and the three traces equal the restatement's bit for bit after
    every launch, the decisions being the restatement's own; the stretch's z equals numpy's bit for bit, g within 1e-12, partners
    and uniforms bit for bit.  (log q is bit for bit because the launch takes the log of z through IEEE operations that
    tempering_np.log_restated repeats; against the library log of the ensemble kernel, and against numpy's, it is held to
    4 ulp: two library logs disagree in the last bit on about 2 % of these arguments.)"""
    import torch
    seed, a, sigma = (7 << 32) + 4321 + K + T, 2.0, 1e-5
    fraction = 0.5 if K >= 4 else 0.0
    E, H = R * T, K // 2
    g0 = 2.38 / np.sqrt(2.0 * d)
    beta = np.linspace(1.0, 0.0, T) if T > 1 else np.ones(1)
    rng = np.random.default_rng(1000 * T + 10 * K + d + (source == 'hostile'))
    theta0 = rng.normal(size=(E, K, d))
    l0, p0 = _smooth(theta0) if source == 'smooth' else (rng.normal(size=(E, K)) - 3.0, rng.normal(size=(E, K)))

    def buffers(length):
        return dict(trace=np.full((length + 2, E, K, d), np.nan), loglik_trace=np.full((length + 2, E, K), np.nan),
                    logprior_trace=np.full((length + 2, E, K), np.nan))
    host = dict(beta=beta, theta=theta0, loglik=l0, logprior=p0, prop=np.zeros((E, H, d)), prop_loglik=np.zeros((E, H)),
                prop_logprior=np.zeros((E, H)), log_q=np.zeros((E, H)), state=np.zeros(R, dtype=np.int64),
                accepted=np.zeros((E, K), dtype=np.int64), swap_attempts=np.zeros((R, T - 1), dtype=np.int64),
                swap_accepted=np.zeros((R, T - 1), dtype=np.int64), draws=np.full((E, H, 6), np.nan), **buffers(4))
    t = {k: torch.as_tensor(v, device='cuda').contiguous() for k, v in host.items()}
    read = lambda: {k: v.cpu().numpy() for k, v in t.items()}                                    # noqa: E731
    window = (1, 4, 2)
    refused = seen_de = 0
    for s in range(31):
        if s == 25:                                             # the window moves: rows 12, 13, 14 (steps 13, 14, 15), new buffers
            window = (12, 3, 1)
            t.update({k: torch.as_tensor(v, device='cuda') for k, v in buffers(3).items()})
        before = read()
        half = (s - 1) % 2                                      # the half whose values this launch resolves (s >= 1)
        if source == 'smooth':
            ll, lp = _smooth(before['prop'])
        else:
            ll, lp = _hostile(rng, before['loglik'][:, half * H:(half + 1) * H], (E, H))
        t['prop_loglik'].copy_(torch.as_tensor(ll, device='cuda'))
        t['prop_logprior'].copy_(torch.as_tensor(lp, device='cuda'))
        _launch(t, R, T, K, d, seed, a, fraction, g0, sigma, *window)
        got = read()
        dr = got['draws']
        kw = dict(beta=beta, seed=seed, a=a, de_fraction=fraction, g0=g0, sigma=sigma, trace_first=window[0], trace_len=window[1],
                  thin=window[2])
        want, rec, mv, swaps = tempering_np.step({k: before[k] for k in STATE}, ll, lp, coef=dr[:, :, 1], **kw)
        own = tempering_np.step({k: before[k] for k in STATE}, ll, lp, **kw)[2]                  # numpy's own z / g
        for name in STATE:
            assert np.array_equal(got[name], want[name], equal_nan=True), (s, name)
        assert np.all(got['state'] == s + 1)
        # the draws: uniforms and partners bit for bit, z bit for bit, g within 1e-12; log q is a log: within 4 ulp of numpy's
        assert np.array_equal(dr[:, :, 5], np.broadcast_to(mv['u_move'][:, None], (E, H))), s
        assert np.array_equal(dr[:, :, 2], mv['j1']) and np.array_equal(dr[:, :, 3], mv['j2']), s
        stretch = ~np.broadcast_to(mv['de'][:, None], (E, H))
        assert np.array_equal(dr[:, :, 1][stretch], own['coef'][stretch]), s
        assert np.max(np.abs(dr[:, :, 1] - own['coef']) / np.abs(own['coef'])) < 1e-12, s
        with np.errstate(all='ignore'):
            library = (float(d - 1) * np.log(dr[:, :, 1]))[stretch]
            assert np.allclose(got['log_q'][stretch], library, rtol=4 * np.finfo(float).eps, atol=0.0), s
        seen_de += int(mv['de'].sum())
        if s >= 1:
            assert np.array_equal(dr[:, :, 4], rec['u_acc']), s
            bad = ~(np.isfinite(ll) & np.isfinite(lp))
            assert not rec['acc'][bad].any()
            refused += int(bad.sum())
            assert np.isfinite(got['loglik']).all() and np.isfinite(got['logprior']).all()      # nothing that is not finite entered
        if swaps is not None and s >= 2:
            assert swaps['pairs'] == [p for p in range(T - 1) if p % 2 == (s // 2) % 2]
    final = read()
    print(f'{source} {(R, T, K, d)}: moves accepted {int(final["accepted"].sum())}, swaps {int(final["swap_accepted"].sum())} of '
          f'{int(final["swap_attempts"].sum())}, '
          f'values refused as not finite {refused}')
    assert 0 < final['accepted'].sum() < 15 * E * K
    if K >= 4:
        assert 0 < seen_de < 31 * E                             # both moves were met
    if source == 'hostile':
        assert refused > 0
    if T > 1:                                                   # 15 steps: pair t is due on 7 or 8 of them
        due = np.array([sum(1 for n in range(1, 16) if n % 2 == p % 2) for p in range(T - 1)])
        assert np.array_equal(final['swap_attempts'], np.broadcast_to(due * K, (R, T - 1)))
        assert 0 < final['swap_accepted'].sum() <= final['swap_attempts'].sum()
        assert np.all(final['swap_accepted'] <= final['swap_attempts'])
    # the second window: its three rows are written, its two guard rows keep their NaN
    rows_written = ~np.isnan(final['trace']).all(axis=(1, 2, 3))
    assert rows_written.tolist() == [True] * 3 + [False, False]
    assert np.array_equal(np.isnan(final['loglik_trace']).all(axis=(1, 2)), ~rows_written)
    assert np.array_equal(np.isnan(final['logprior_trace']).all(axis=(1, 2)), ~rows_written)
    assert np.array_equal(final['trace'][2], final['theta']) and np.array_equal(final['loglik_trace'][2], final['loglik'])


# ------------------------------------------------------------------------------------------------------------ the driver
@pytest.mark.gpu
def test_one_temperature_is_device_ensemble_bit_for_bit_and_graph_replay_is_eager():
    """T = 1 with log_likelihood = f and log_prior = 0 against DeviceEnsemble(f), same seed, 30 steps of 3 ensembles of 12 walkers
    in d = 5 with both moves: the same trace and state, bit for bit.  T = 3: graph replay and eager launches give the same
    traces, and a run continues across calls."""
    import torch
    from hallthrusterpem_amd.calibration import DeviceEnsemble, DeviceTemperedEnsemble
    from test_ensemble import MU, _gaussian
    f = _gaussian(bound=True)
    zero = lambda x: torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)               # noqa: E731
    x0 = DeviceEnsemble.ball(MU, 0.5, 12, n_ensembles=3, seed=8)
    ens = DeviceEnsemble(f, x0, seed=5, de_fraction=0.5)
    want, want_lp = ens.run(30, keep_logp=True)
    one = DeviceTemperedEnsemble(f, zero, x0[:, None], betas=[1.0], n_replicas=3, seed=5, de_fraction=0.5)
    got = one.run(30)
    assert got.shape == (30, 3, 1, 12, 5) and torch.equal(got[:, :, 0], want) and torch.equal(one.loglik_trace[:, :, 0], want_lp)
    assert torch.equal(one.cold(), want) and not bool(one.logprior_trace.any())
    for mine, theirs in (('theta', 'theta'), ('loglik', 'logp'), ('prop', 'prop'), ('state', 'state'), ('accepted', 'accepted')):
        assert torch.equal(getattr(one, mine), getattr(ens, theirs)), mine
    assert torch.allclose(one.log_q, ens.log_q, rtol=4 * 2.0 ** -52, atol=0.0)       # its own log against the library's
    assert one.swap_rates().shape == (3, 0) and torch.allclose(one.move_rates(), ens.acceptance.mean(dim=1, keepdim=True), rtol=1e-14)
    # T = 3
    prior = lambda x: -0.5 * (x * x).sum(dim=1) / 25.0                                           # noqa: E731
    y0 = DeviceTemperedEnsemble.ball(MU, 0.3, 12, n_temperatures=3, n_replicas=2, seed=9)    # (every start inside the hard edge)
    mk = lambda **kw: DeviceTemperedEnsemble(f, prior, y0, betas=[1.0, 0.3, 0.0], n_replicas=2, seed=6, de_fraction=0.5, **kw)  # noqa: E731
    graph, eager, split = mk(), mk(use_graph=False), mk()
    whole = graph.run(40)
    assert whole.shape == (40, 2, 3, 12, 5) and torch.equal(eager.run(40), whole)
    a, b = split.run(25), split.run(15, thin=2)
    assert torch.equal(a, whole[:25]) and torch.equal(b, whole[25::2]) and split.steps == 40
    for other in (eager, split):
        for name in ('theta', 'loglik', 'logprior', 'prop', 'log_q', 'state', 'accepted', 'swap_attempts', 'swap_accepted'):
            assert torch.equal(getattr(other, name), getattr(graph, name)), name
    assert torch.equal(eager.loglik_trace, graph.loglik_trace) and torch.equal(eager.logprior_trace, graph.logprior_trace)
    flat = whole.reshape(-1, 5)
    # (another batch size than the run's: torch may add in another order)
    assert torch.allclose(graph.loglik_trace.reshape(-1), f(flat), rtol=1e-12, atol=0)
    assert torch.allclose(graph.logprior_trace.reshape(-1), prior(flat), rtol=1e-12, atol=0)
    assert int(graph.state[0]) == 81 and graph.swap_attempts.tolist() == [[20 * 12, 20 * 12]] * 2
    rates = graph.swap_rates()
    assert rates.shape == (2, 2) and 0.0 < float(rates.min()) and float(rates.max()) <= 1.0
    assert graph.move_rates().shape == (2, 3) and graph.cold(means=True).shape == (40, 2, 5)
    assert graph.run(3, keep=False) is None and graph.trace is None
    with pytest.raises(ValueError, match='no trace'):
        graph.cold()
    with pytest.raises(ValueError, match='ends at beta = 0'):
        DeviceTemperedEnsemble(f, prior, y0[:, :2], betas=[1.0, 0.3], n_replicas=2).log_evidence()
    x0[1, 7, 2] = MU[2] - 2.0                                               # past the hard edge of coordinate 2
    with pytest.raises(ValueError, match='1 of the 36 starts have a log likelihood'):
        DeviceTemperedEnsemble(f, zero, x0[:, None], betas=[1.0], n_replicas=3)


# ------------------------------------------------------------------------------------------- what tempering is for: two modes
M1, M2 = np.array([-5.0, 0.0]), np.array([5.0, 0.0])
MIX_R, MIX_T, MIX_K, MIX_STEPS, MIX_BURN, MIX_BETA_MIN = 4, 6, 16, 800, 200, 0.01
MIX_MARGIN = 2 * 0.0263                                 # twice the largest CPU deviation below


def mix_loglik(x):
    a = np.log(0.3) - 0.5 * np.sum((x - M1) ** 2, axis=-1)
    b = np.log(0.7) - 0.5 * np.sum((x - M2) ** 2, axis=-1)
    return np.logaddexp(a, b) - np.log(2.0 * np.pi)


def mix_logprior(x):
    return np.where(np.all(np.abs(x) <= 15.0, axis=-1), -np.log(900.0), -np.inf)


def mix_on_device():
    """the two functions above on torch tensors, their constants on the device before anything is recorded into a graph"""
    import torch
    m1, m2 = (torch.as_tensor(m, device='cuda') for m in (M1, M2))
    inside, outside = (torch.tensor(v, dtype=torch.float64, device='cuda') for v in (-np.log(900.0), -np.inf))

    def loglik(x):
        a = np.log(0.3) - 0.5 * ((x - m1) ** 2).sum(dim=-1)
        b = np.log(0.7) - 0.5 * ((x - m2) ** 2).sum(dim=-1)
        return torch.logaddexp(a, b) - np.log(2.0 * np.pi)

    def logprior(x):
        return torch.where((x.abs() <= 15.0).all(dim=-1), inside, outside)
    return loglik, logprior


def mix_starts(seed):
    return M1 + np.random.default_rng(1000 + seed).standard_normal((MIX_R, MIX_T, MIX_K, 2))


def mix_fraction(trace):
    """the share of the cold ensembles' draws after the burn-in that sit in the 0.7 mode; trace (rows, R, T, K, 2)"""
    return float((np.asarray(trace)[MIX_BURN:, :, 0, :, 0] > 0.0).mean())


@pytest.mark.gpu
def test_tempering_finds_the_mode_it_was_not_started_in():
    """0.3 N((-5, 0), I) + 0.7 N((5, 0), I) as the likelihood, a uniform prior on [-15, 15]^2, every walker started round (-5, 0):
    R = 4, T = 6 (geometric ladder down to 0.01), K = 16, 800 steps, the first 200 dropped.  The cold ensembles' share of draws in
    the 0.7 mode is within MIX_MARGIN of 0.7.  The margin is twice the largest deviation of the restatement on the CPU at this
    length over seeds 100 ... 119 (python tests/test_tempering.py):

        deviations -0.0003 -0.0112 0.0263 0.0132 -0.0009 -0.0142 0.0148 -0.0026 -0.0088 0.0057 -0.0037 -0.0260 -0.0099 0.0081
                   0.0005 -0.0090 -0.0127 -0.0203 0.0033 -0.0051
        largest 0.0263 -> MIX_MARGIN 0.0526 (limit: 0.1)

    A DeviceEnsemble from the same starts never leaves the 0.3 mode (examples/tempered_ensemble.py reports it)."""
    from hallthrusterpem_amd.calibration import DeviceTemperedEnsemble
    assert MIX_MARGIN <= 0.1
    s = DeviceTemperedEnsemble(*mix_on_device(), mix_starts(7), n_temperatures=MIX_T, beta_min=MIX_BETA_MIN, n_replicas=MIX_R, seed=7)
    trace = s.run(MIX_STEPS)
    assert trace.shape == (MIX_STEPS, MIX_R, MIX_T, MIX_K, 2)
    got = mix_fraction(trace.cpu().numpy())
    print(f'share of cold draws in the 0.7 mode {got:.4f}; swap rates {s.swap_rates().mean(dim=0).cpu().numpy().round(2)}; '
          f'move rates {s.move_rates().mean(dim=0).cpu().numpy().round(2)}')
    assert abs(got - 0.7) <= MIX_MARGIN, got
    assert float(s.swap_rates().min()) > 0.2                    # every pair of neighbours talks


# ------------------------------------------------------------------------------------------------------------ the evidence
EV_D, EV_S, EV_SP, EV_M = 3, 0.5, 2.0, np.array([1.0, -0.5, 0.5])
EV_R, EV_K, EV_STEPS, EV_BURN = 4, 8, 2000, 500
EV_LOGZ = -0.5 * EV_D * np.log(2 * np.pi * (EV_S ** 2 + EV_SP ** 2)) - np.sum(EV_M ** 2) / (2 * (EV_S ** 2 + EV_SP ** 2))
# the restatement's CPU spread (python tests/test_tempering.py): twice the largest deviation over seeds 100 ... 119 of the
# replica-mean of mean_loglik from the exact curve, per temperature, and of the mean log evidence from the exact trapezoid
EV_CURVE_FLOOR = 2 * np.array([0.0194, 0.0331, 0.0679, 0.0776, 0.0535, 0.1066, 0.1554, 0.2170, 0.1882, 0.2665, 0.3166, 0.5632])
EV_LOGZ_FLOOR = 2 * 0.0402


def ev_loglik(x, m=EV_M):
    return -0.5 * ((x - m) ** 2).sum(-1) / EV_S ** 2 - 0.5 * EV_D * np.log(2 * np.pi * EV_S ** 2)


def ev_logprior(x):
    return -0.5 * (x ** 2).sum(-1) / EV_SP ** 2 - 0.5 * EV_D * np.log(2 * np.pi * EV_SP ** 2)


def ev_exact_curve(beta):
    """E_beta[l] under prior x likelihood^beta, a Gaussian of precision 1 / sp^2 + beta / s^2 per coordinate"""
    lam = 1.0 / EV_SP ** 2 + beta / EV_S ** 2
    mu = (beta[:, None] * EV_M / EV_S ** 2) / lam[:, None]
    return -0.5 * EV_D * np.log(2 * np.pi * EV_S ** 2) - (EV_D / lam + np.sum((mu - EV_M) ** 2, axis=1)) / (2 * EV_S ** 2)


def ev_ladder():
    from hallthrusterpem_amd.calibration import DeviceTemperedEnsemble
    return DeviceTemperedEnsemble.ladder(11, 1e-2, include_prior=True)


def ev_starts(seed, T):
    return EV_M + 0.5 * np.random.default_rng(2000 + seed).standard_normal((EV_R, T, EV_K, EV_D))


@pytest.mark.gpu
def test_thermodynamic_integration_recovers_a_closed_form_evidence():
    """l = log N(x; m, 0.5^2 I), prior N(0, 2^2 I), d = 3: log Z = log N(m; 0, (0.5^2 + 2^2) I) = -5.1037 and E_beta[l] is closed
    form.  T = 12 (11 geometric temperatures down to 0.01, and 0), R = 4, K = 8, 2000 steps, the first 500 dropped.  The replica-mean
    of mean_loglik is within max(4 standard errors of the replica spread, EV_CURVE_FLOOR) of the exact curve at every beta; the mean
    log evidence within max(4 standard errors, EV_LOGZ_FLOOR) of the trapezoid of the exact curve on the same ladder (-5.1874), and
    within that plus the returned discretisation estimate (exact curve: 0.2524, true error 0.0838) of the closed form.  The floors
    are twice the largest deviation of the restatement on the CPU over seeds 100 ... 119 (python tests/test_tempering.py):

        max |mean_loglik - exact| per beta 0.0194 0.0331 0.0679 0.0776 0.0535 0.1066 0.1554 0.2170 0.1882 0.2665 0.3166 0.5632
        max |log Z - exact trapezoid| 0.0402"""
    import torch
    from hallthrusterpem_amd.calibration import DeviceTemperedEnsemble
    beta = ev_ladder()
    assert beta.size == 12 and beta[-1] == 0.0
    exact = ev_exact_curve(beta)
    exact_ev = DeviceTemperedEnsemble.evidence_from(exact[None], beta)
    assert abs(exact_ev['log_z'][0] - EV_LOGZ) <= exact_ev['discretisation'][0]     # the estimate covers the rule's own error
    m = torch.as_tensor(EV_M, device='cuda')                             # (on the device before anything is recorded into a graph)
    loglik = lambda x: ev_loglik(x, m)                                   # noqa: E731
    s = DeviceTemperedEnsemble(loglik, ev_logprior, ev_starts(3, beta.size), betas=beta, n_replicas=EV_R, seed=3)
    s.run(EV_STEPS)
    ml = s.mean_loglik(EV_BURN)
    assert ml.shape == (EV_R, 12)
    ml = ml.cpu().numpy()
    margin = np.maximum(4.0 * ml.std(axis=0, ddof=1) / np.sqrt(EV_R), EV_CURVE_FLOOR)
    dev = ml.mean(axis=0) - exact
    ev = s.log_evidence(EV_BURN)
    z_margin = max(4.0 * ev['spread'] / np.sqrt(EV_R), EV_LOGZ_FLOOR)
    print(f'mean_loglik - exact {np.round(dev, 4).tolist()}\nmargins {np.round(margin, 4).tolist()}\nlog Z {ev["mean"]:.4f} (replicas '
          f'{np.round(ev["log_z"], 4).tolist()}, spread {ev["spread"]:.4f}), exact trapezoid {exact_ev["log_z"][0]:.4f}, closed form '
          f'{EV_LOGZ:.4f}, discretisation {np.round(ev["discretisation"], 4).tolist()}, margin {z_margin:.4f}')
    assert np.all(np.abs(dev) <= margin), (dev, margin)
    assert ev['log_z'].shape == (EV_R,) and ev['discretisation'].shape == (EV_R,)
    assert abs(ev['mean'] - exact_ev['log_z'][0]) <= z_margin
    assert abs(ev['mean'] - EV_LOGZ) <= float(ev['discretisation'].mean()) + z_margin
    assert torch.allclose(s.loglik_trace.reshape(-1), loglik(s.trace.reshape(-1, EV_D)), rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------------------------------- on a posterior
@pytest.mark.gpu
def test_tempered_ensemble_on_a_shared_nuisance_system_posterior():
    """the posterior of test_device_ensemble_on_a_shared_nuisance_system_posterior (R = 1, T = 2: the same E = 2 ensembles of
    K = 2 d walkers), beta = (1, 0.5), 3 steps: the stored l + pi at the final positions equal post.log_likelihood + post.log_prior
    called afterwards, exactly, and so do the kept traces; the one swap visit (step 2) is in the counters"""
    import torch
    from hallthrusterpem_amd.calibration import DeviceTemperedEnsemble, SystemPosterior
    from test_optimize import _synthetic
    lik, names, star = _synthetic()
    star = np.asarray(star, dtype=np.float64)
    d, T, n = len(names), 2, 3
    K = 2 * d
    rows = T * K // 2
    post = SystemPosterior(names, lik, n_chains=rows, n_nuisance=50, seed=1, fresh_nuisance=False, shared_nuisance=True)
    s = DeviceTemperedEnsemble(post.log_likelihood, post.log_prior,
                               DeviceTemperedEnsemble.ball(star, 0.005 * np.abs(star), K, n_temperatures=T, seed=3), betas=[1.0, 0.5],
                               seed=2, device=post.device)
    trace = s.run(n)
    assert trace.shape == (n, 1, T, K, d) and s.loglik_trace.shape == (n, 1, T, K)

    def both(flat):
        chunks = [flat[i:i + rows].contiguous() for i in range(0, flat.shape[0], rows)]
        return (torch.cat([post.log_likelihood(c).clone() for c in chunks]), torch.cat([post.log_prior(c).clone() for c in chunks]))
    ll, lp = both(s.theta.reshape(-1, d))
    assert torch.equal(s.loglik.reshape(-1) + s.logprior.reshape(-1), ll + lp)
    assert torch.equal(s.loglik.reshape(-1), ll) and torch.equal(s.logprior.reshape(-1), lp)
    ll, lp = both(trace.reshape(-1, d))
    assert torch.equal(s.loglik_trace.reshape(-1), ll) and torch.equal(s.logprior_trace.reshape(-1), lp)
    assert torch.isfinite(s.loglik_trace).all() and torch.isfinite(s.logprior_trace).all()
    assert torch.equal(s.theta, trace[-1].reshape(T, K, d))
    assert s.swap_attempts.tolist() == [[K]] and 0 <= int(s.swap_accepted) <= K               # steps 1 and 3 visit no pair of T = 2
    # step 3 has no swap: what changed between rows 2 and 3 are accepted moves, which the move counters saw
    assert int(s.state[0]) == 2 * n + 1 and int(s.accepted.sum()) >= int((trace[2] != trace[1]).any(dim=-1).sum())
    assert 0.0 <= float(s.move_rates().min()) and float(s.move_rates().max()) <= 1.0


if __name__ == '__main__':
    devs = []
    for seed in range(100, 120):
        st = tempering_np.run(mix_loglik, mix_logprior, mix_starts(seed), 0.01 ** (np.arange(MIX_T) / (MIX_T - 1.0)), MIX_STEPS, seed=seed)
        devs.append(mix_fraction(st['trace'].reshape(MIX_STEPS, MIX_R, MIX_T, MIX_K, 2)) - 0.7)
        print(f'mixture seed {seed}: deviation {devs[-1]:+.4f}', flush=True)
    print(f'largest {np.max(np.abs(devs)):.4f} -> MIX_MARGIN {2 * np.max(np.abs(devs)):.4f}')
    from hallthrusterpem_amd.calibration import DeviceTemperedEnsemble as D
    beta = ev_ladder()
    exact = ev_exact_curve(beta)
    exact_z = D.evidence_from(exact[None], beta)
    print(f'closed form {EV_LOGZ:.4f}, exact trapezoid {exact_z["log_z"][0]:.4f}, discretisation {exact_z["discretisation"][0]:.4f}')
    dev_ml, dev_z = [], []
    for seed in range(100, 120):
        st = tempering_np.run(ev_loglik, ev_logprior, ev_starts(seed, beta.size), beta, EV_STEPS, seed=seed, keep_theta=False)
        ml = st['loglik_trace'].reshape(-1, EV_R, beta.size, EV_K)[EV_BURN:].mean(axis=(0, 3))
        dev_ml.append(ml.mean(axis=0) - exact)
        dev_z.append(D.evidence_from(ml, beta)['mean'] - exact_z['log_z'][0])
        print(f'evidence seed {seed}: log Z deviation {dev_z[-1]:+.4f}, curve {np.round(dev_ml[-1], 3).tolist()}', flush=True)
    print('max |mean_loglik - exact| per beta ' + ' '.join(f'{v:.4f}' for v in np.max(np.abs(dev_ml), axis=0)))
    print(f'max |log Z - exact trapezoid| {np.max(np.abs(dev_z)):.4f}')
