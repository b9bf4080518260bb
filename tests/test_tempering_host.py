"""Replica exchange over the ensemble sampler without a GPU: pem_tempered_ensemble_step_f64_dev is declared, bound, built and
exported, refuses every malformed call before it looks for a device and compiles without scratch; DeviceTemperedEnsemble refuses
what it cannot run before it touches a device; the numpy restatement of the launch (tests/tempering_np.py) is tests/ensemble_np.py
at one temperature, keeps the books of the even-odd swaps as the rules state them, and its swap is in detailed balance."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAME = 'pem_tempered_ensemble_step_f64_dev'


def test_the_entry_point_is_declared_bound_built_and_exported():
    from hallthrusterpem_amd import _lib, build
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % NAME, header)
    assert m and len(m.group(1).split(',')) == 29
    assert len(_lib.SIGNATURES[NAME][1]) == 29
    assert hasattr(_lib.load(), NAME)
    assert build.PKG / 'csrc' / 'pem_tempering.hip' in build.SRCS
    assert '0x454E0003' in header                                        # the swap's key layout sits beside the ensemble's


FAKE = C.c_void_p(4096)                        # never dereferenced: every check runs on the host
ARRAYS = ('beta', 'theta', 'loglik', 'logprior', 'prop', 'prop_loglik', 'prop_logprior', 'log_q', 'state', 'accepted', 'swap_attempts',
          'swap_accepted', 'trace', 'loglik_trace', 'logprior_trace', 'draws')
OPTIONAL = ('trace', 'loglik_trace', 'logprior_trace', 'draws')


def _call(R=2, T=3, K=8, d=3, seed=1, a=2.0, de_fraction=0.5, g0=0.9, sigma=1e-5, trace_first=0, trace_len=8, thin=1, **null):
    from hallthrusterpem_amd import _lib
    ptr = {n: None if null.get(n, n in ('logprior_trace', 'draws')) else FAKE for n in ARRAYS}   # name=True: that array is NULL
    return _lib.load().pem_tempered_ensemble_step_f64_dev(R, T, K, d, seed, a, de_fraction, g0, sigma, ptr['beta'], trace_first,
                                                          trace_len, thin, *[ptr[n] for n in ARRAYS[1:]], None)


NAN, INF = float('nan'), float('inf')


@pytest.mark.parametrize('bad', [
    dict(R=0), dict(T=0), dict(T=-1), dict(R=1 << 20, T=1 << 20), dict(T=1 << 20, K=1024, d=32), dict(K=7), dict(K=0), dict(K=1),
    dict(K=-2), dict(K=1026), dict(K=2, d=1, de_fraction=0.5), dict(d=0), dict(d=-1), dict(d=33), dict(a=1.0), dict(a=NAN),
    dict(a=INF), dict(de_fraction=-0.1), dict(de_fraction=1.5), dict(de_fraction=NAN), dict(g0=0.0), dict(g0=NAN), dict(g0=INF),
    dict(sigma=-1e-5), dict(sigma=NAN), dict(sigma=INF), dict(thin=0), dict(trace_len=0),
    dict(trace_len=0, trace=True, loglik_trace=True, logprior_trace=False),                     # one trace alone needs rows as well
] + [{n: True} for n in ARRAYS if n not in OPTIONAL])
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_tempered_ensemble_step' in _lib.load().pem_last_error()


def test_a_well_formed_call_gets_as_far_as_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _call() == _lib.PEM_ERR_NO_DEVICE
    assert _call(trace=True, loglik_trace=True, trace_len=0) == _lib.PEM_ERR_NO_DEVICE            # no trace: trace_len is not looked at
    assert _call(T=1, swap_attempts=True, swap_accepted=True) == _lib.PEM_ERR_NO_DEVICE           # one temperature: nothing to count
    assert _call(R=1, T=1, K=2, d=1, de_fraction=0.0) == _lib.PEM_ERR_NO_DEVICE
    assert _call(K=1024, d=32, de_fraction=1.0, sigma=0.0) == _lib.PEM_ERR_NO_DEVICE


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_tempering_kernel_cross_compiles_without_scratch_and_vector_spills():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'),
                          str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_tempering.hip')], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+) kernarg\s+(\d+) lds\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), vspill=int(m.group(5)), scratch=int(m.group(6)), lds=int(m.group(8)))
    assert list(rows) == ['tempered_ensemble_step_kernel'], rows
    r = rows['tempered_ensemble_step_kernel']   # moves of up to 512 walkers and the flags of up to 1024 walker pairs in LDS
    assert r['vspill'] == 0 and r['scratch'] == 0 and r['lds'] <= 16 * 1024 and r['vgpr'] <= 128, r


# ------------------------------------------------------------------------------------------------------------- the driver
def _f(theta):
    raise AssertionError('neither callable may be called')


@pytest.mark.parametrize('kw, match', [
    (dict(theta0=np.zeros((8, 3)), betas=[]), 'T >= 1'),
    (dict(theta0=np.zeros((8, 3)), betas=[0.9, 0.5]), 'decrease strictly from 1'),
    (dict(theta0=np.zeros((8, 3)), betas=[1.0, 0.5, 0.5]), 'decrease strictly from 1'),
    (dict(theta0=np.zeros((8, 3)), betas=[1.0, 0.2, 0.4]), 'decrease strictly from 1'),
    (dict(theta0=np.zeros((8, 3)), betas=[1.0, 0.5, -0.1]), 'stay >= 0'),
    (dict(theta0=np.zeros((8, 3)), betas=[1.0, float('nan')]), 'finite'),
    (dict(theta0=np.zeros((8, 3)), betas=[1.0, float('-inf')]), 'finite'),
    (dict(theta0=np.zeros((8, 3)), n_temperatures=0), 'n_temperatures >= 1'),
    (dict(theta0=np.zeros((8, 3)), n_temperatures=4, beta_min=1.0), '0 < beta_min < 1'),
    (dict(theta0=np.zeros((7, 2))), 'even number of walkers'),
    (dict(theta0=np.zeros((2, 7, 2)), betas=[1.0, 0.5]), 'even number of walkers'),
    (dict(theta0=np.zeros((8, 5))), '2 d = 10 <= K'),
    (dict(theta0=np.zeros((80, 33))), '1 to 32 parameters'),
    (dict(theta0=np.zeros((1026, 3))), 'K <= 1024'),
    (dict(theta0=np.zeros((3, 8, 3)), betas=[1.0, 0.5]), r'\(R, T, K, d\) with T = 2'),
    (dict(theta0=np.zeros((3, 2, 8, 3)), betas=[1.0, 0.5], n_replicas=2), r'R = n_replicas = 2'),
    (dict(theta0=np.zeros(3)), r'\(R, T, K, d\)'),
    (dict(theta0=np.zeros((8, 3)), n_replicas=0), r'\(R, T, K, d\)'),
    (dict(theta0='nan'), '2 of the 16 starts have a coordinate that is not finite'),
    (dict(theta0=np.zeros((8, 3)), device='cpu'), 'GPU only'),
    (dict(theta0='tensor'), 'GPU only'),                                  # a CPU tensor as the start points
    (dict(theta0=np.zeros((8, 3)), de_fraction=1.1), r'de_fraction must be in \[0, 1\]'),
    (dict(theta0=np.zeros((2, 1)), de_fraction=0.5), 'K >= 4'),
    (dict(theta0=np.zeros((8, 3)), a=1.0), 'a > 1'),
])
def test_the_driver_refuses_what_it_cannot_run_before_touching_a_device(kw, match, monkeypatch):
    import torch
    from hallthrusterpem_amd.calibration import DeviceTemperedEnsemble
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('touched a device'))
    if isinstance(kw['theta0'], str) and kw['theta0'] == 'tensor':
        kw = dict(kw, theta0=torch.zeros((8, 3), dtype=torch.float64))
    elif isinstance(kw['theta0'], str):                                   # T = 2 ladders of 8 walkers, two of them not finite
        x0 = np.zeros((2, 8, 3))
        x0[0, 1, 2], x0[1, 7, 0], x0[1, 7, 1] = np.nan, np.inf, -np.inf
        kw = dict(kw, theta0=x0, betas=[1.0, 0.0])
    with pytest.raises(ValueError, match=match):
        DeviceTemperedEnsemble(_f, _f, **kw)


def test_ladders_balls_and_the_evidence_integral():
    from hallthrusterpem_amd.calibration import DeviceTemperedEnsemble as D
    assert D.ladder(1).tolist() == [1.0] and D.ladder(1, include_prior=True).tolist() == [1.0, 0.0]
    b = D.ladder(5, 1e-4, include_prior=True)
    assert b.shape == (6,) and b[0] == 1.0 and b[-1] == 0.0 and np.allclose(b[1:5] / b[:4], 0.1)
    c, s = np.array([1.0, -2.0, 1e20]), np.array([0.1, 0.2, 1e18])
    got = D.ball(c, s, 6, n_temperatures=3, n_replicas=2, seed=5)
    assert np.array_equal(got, c + s * np.random.default_rng(5).standard_normal((2, 3, 6, 3)))
    # the trapezoid rule is exact on a curve that is linear in beta, on any ladder; the coarse rule as well
    ml = np.stack([3.0 - 2.0 * b, 1.0 + 4.0 * b])
    ev = D.evidence_from(ml, b)
    assert np.allclose(ev['log_z'], [2.0, 3.0], rtol=1e-14) and np.allclose(ev['discretisation'], 0.0, atol=1e-14)
    assert ev['mean'] == pytest.approx(2.5) and ev['spread'] == pytest.approx(np.std([2.0, 3.0], ddof=1))
    # on beta^2 the coarse rule over (1, 0.5, 0) is off by four times the error of the fine one over (1, 0.75, 0.5, 0.25, 0)
    q = np.array([1.0, 0.75, 0.5, 0.25, 0.0])
    ev = D.evidence_from(q[None] ** 2, q)
    assert ev['log_z'][0] == pytest.approx(1 / 3 + 1 / 96) and ev['discretisation'][0] == pytest.approx(3 / 96) and np.isnan(ev['spread'])
    assert np.isnan(D.evidence_from([[1.0, 0.0]], [1.0, 0.0])['discretisation'][0])
    with pytest.raises(ValueError, match='ends at beta = 0'):
        D.evidence_from(np.zeros((1, 3)), [1.0, 0.1, 0.01])


# --------------------------------------------------------------------------------------------------------- the restatement
def test_the_restated_log_is_a_log_to_the_last_bit_but_one():
    """tempering_np.log_restated (what the launch computes log q with) within 1 ulp of numpy's log over the stretch variable's
    range for a = 2 and a = 1e3, across the binades, next to 1 and at the reduction's own switch points"""
    import tempering_np
    rng = np.random.default_rng(1)
    x = np.concatenate([(rng.random(20000) + 1.0) ** 2 / 2.0, (999.0 * rng.random(20000) + 1.0) ** 2 / 1e3, np.exp(rng.uniform(-700, 700, 5000)),
                        1.0 + rng.uniform(-3e-6, 3e-6, 3000), [1.0, 2.0, 0.5, 2.0 ** -1022, 1.7e308, np.sqrt(2.0), np.sqrt(0.5)]])
    got, ref = tempering_np.log_restated(x), np.log(x)
    assert np.all(np.abs(got - ref) <= 2 * np.spacing(np.abs(ref))) and tempering_np.log_restated(np.array([1.0]))[0] == 0.0
    with np.errstate(all='ignore'):
        odd = np.array([0.0, -1.0, np.inf, np.nan, 1e-310])
        assert np.array_equal(tempering_np.log_restated(odd), np.log(odd), equal_nan=True)


def _state(rng, R, T, K, d, rows=0):
    E, H = R * T, K // 2
    st = dict(theta=rng.standard_normal((E, K, d)), loglik=2.0 * rng.standard_normal((E, K)), logprior=rng.standard_normal((E, K)),
              prop=np.zeros((E, H, d)), log_q=np.zeros((E, H)), state=np.zeros(R, dtype=np.int64),
              accepted=np.zeros((E, K), dtype=np.int64), swap_attempts=np.zeros((R, T - 1), dtype=np.int64),
              swap_accepted=np.zeros((R, T - 1), dtype=np.int64))
    if rows:
        st.update(trace=np.full((rows, E, K, d), np.nan), loglik_trace=np.full((rows, E, K), np.nan),
                  logprior_trace=np.full((rows, E, K), np.nan))
    return st


@pytest.mark.parametrize('K, d', [(4, 2), (8, 3)])
def test_one_temperature_is_the_ensemble_restatement_bit_for_bit(K, d):
    """T = 1, beta = (1,), l = logp and pi = 0: theta and every accept decision of 20 steps equal tests/ensemble_np.py's"""
    import ensemble_np
    import tempering_np
    R, H, seed = 3, K // 2, (5 << 32) + 77
    logp = lambda x: -0.5 * np.sum((x - 0.3) ** 2 * np.arange(1, d + 1), axis=1)                 # noqa: E731
    rng = np.random.default_rng(K)
    te = _state(rng, R, 1, K, d)
    te['loglik'] = logp(te['theta'].reshape(-1, d)).reshape(R, K)
    te['logprior'] = np.zeros((R, K))
    en = dict(theta=te['theta'], logp=te['loglik'], prop=te['prop'], log_q=te['log_q'], state=te['state'], accepted=te['accepted'])
    kw = dict(seed=seed, de_fraction=0.5)
    moves = set()
    for s in range(41):
        lp_e, lp_t = logp(en['prop'].reshape(-1, d)).reshape(R, H), logp(te['prop'].reshape(-1, d)).reshape(R, H)
        en, rec_e, mv = ensemble_np.step(en, lp_e, **kw)
        te, rec_t, _, swaps = tempering_np.step(te, lp_t, np.zeros((R, H)), [1.0], **kw)
        assert np.array_equal(te['theta'], en['theta']) and np.array_equal(te['prop'], en['prop']), s
        assert np.array_equal(te['loglik'], en['logp']), s
        assert np.allclose(te['log_q'], en['log_q'], rtol=4 * np.finfo(float).eps, atol=0.0), s   # log_restated against numpy's log
        assert np.array_equal(te['accepted'], en['accepted']) and np.all(te['state'] == s + 1)
        if s >= 1:
            assert np.array_equal(rec_t['acc'], rec_e['acc']), s
        assert swaps is None or swaps['pairs'] == []
        moves |= set(mv['de'].tolist())
    assert moves == {False, True} and 0 < en['accepted'].sum() < 20 * R * K


@pytest.mark.parametrize('T', [2, 3, 5])
def test_swaps_are_attempted_even_odd_and_exchange_theta_loglik_and_logprior_together(T):
    """R = 2, K = 4, d = 2, the moves frozen (every proposal is offered -inf), 10 steps: pair (t, t + 1) is attempted exactly on the
    steps n with n = t (mod 2); what a step changes in the trace is the exchange of the swapped walker pairs and nothing else --
    theta, loglik and logprior together --, the top of an odd ladder stands still when its pair is not due, and the counters add up
    to those changes"""
    import tempering_np
    R, K, d, n_steps = 2, 4, 2, 10
    H = K // 2
    beta = np.linspace(1.0, 0.0, T)
    st = _state(np.random.default_rng(T), R, T, K, d, rows=n_steps)
    start = {n: st[n].reshape((R, T, K) + st[n].shape[2:]).copy() for n in ('theta', 'loglik', 'logprior')}
    kw = dict(beta=beta, seed=11, trace_len=n_steps)
    frozen = np.full((R * T, H), -np.inf)
    records = {}
    for s in range(2 * n_steps + 1):
        before = {n: st[n].copy() for n in ('swap_attempts', 'swap_accepted')}
        st, rec, _, swaps = tempering_np.step(st, frozen, np.zeros((R * T, H)), **kw)
        assert rec is None or not rec['acc'].any()
        if s >= 2 and s % 2 == 0:
            n = s // 2
            assert swaps['pairs'] == [t for t in range(T - 1) if t % 2 == n % 2]
            due = np.isin(np.arange(T - 1), swaps['pairs'])
            assert np.array_equal(st['swap_attempts'] - before['swap_attempts'], np.broadcast_to(due * K, (R, T - 1)))
            assert np.array_equal(st['swap_accepted'] - before['swap_accepted'], swaps['acc'].sum(axis=2))
            assert not swaps['acc'][:, ~due].any()
            records[n] = swaps
        else:
            assert swaps is None and all(np.array_equal(st[n], before[n]) for n in before)
    assert not st['accepted'].any()
    changed = 0
    prev = start
    for n in range(1, n_steps + 1):
        now = {name: st[key][n - 1].reshape(prev[name].shape) for name, key in
               (('theta', 'trace'), ('loglik', 'loglik_trace'), ('logprior', 'logprior_trace'))}
        want = {name: v.copy() for name, v in prev.items()}
        for t in records[n]['pairs']:
            sw = records[n]['acc'][:, t]
            for name in want:
                want[name][:, t][sw], want[name][:, t + 1][sw] = prev[name][:, t + 1][sw], prev[name][:, t][sw]
        for name in want:
            assert np.array_equal(now[name], want[name]), (n, name)
        if T % 2 == 1 and (T - 2) % 2 != n % 2:                               # the top's pair (T - 2, T - 1) is not due
            assert all(np.array_equal(now[name][:, T - 1], prev[name][:, T - 1]) for name in now)
        changed += int((now['loglik'] != prev['loglik']).sum())
        prev = now
    assert changed == 2 * st['swap_accepted'].sum() and 0 < st['swap_accepted'].sum() < st['swap_attempts'].sum()
    assert st['swap_attempts'].sum() == R * K * sum(len(records[n]['pairs']) for n in records)


def test_loglik_and_logprior_travel_with_theta_through_moves_and_swaps():
    """a live run (R = 2, T = 3, K = 8, d = 2, 60 steps): every kept l and pi is the function's value at the kept theta"""
    import tempering_np
    loglik = lambda x: -0.5 * np.sum((x - 1.0) ** 2, axis=1) / 0.3 ** 2                          # noqa: E731
    logprior = lambda x: -0.5 * np.sum(x ** 2, axis=1) / 4.0                                     # noqa: E731
    x0 = 1.0 + 0.3 * np.random.default_rng(1).standard_normal((2, 3, 8, 2))
    st = tempering_np.run(loglik, logprior, x0, [1.0, 0.3, 0.0], 60, seed=4, de_fraction=0.3)
    flat = st['trace'].reshape(-1, 2)
    assert np.array_equal(st['loglik_trace'].reshape(-1), loglik(flat)) and np.array_equal(st['logprior_trace'].reshape(-1), logprior(flat))
    assert np.array_equal(st['trace'][-1], st['theta']) and st['swap_accepted'].sum() > 0 and st['accepted'].sum() > 0
    assert np.array_equal(st['swap_attempts'], [[30 * 8, 30 * 8]] * 2)                           # 60 steps: each pair on every other


def test_the_swap_is_in_detailed_balance():
    """two temperatures beta = (1, 0.3), K = 2 walkers held fixed (de_fraction 0, every proposal's likelihood -inf), l_a = -1 at
    t = 0 and l_b = 0 at t = 1, so Delta = (beta_0 - beta_1)(l_b - l_a) = 0.7: a walker pair sits in the swapped arrangement (l_b at
    beta = 1) for e^Delta / (1 + e^Delta) of the time.  R = 50 replicas x 2 walker pairs x 200 visits of the pair = 20 000 swap
    draws after 10 visits of burn-in (every pair starts unswapped).  Margin: 4 binomial standard errors (successive draws of a
    pair are negatively correlated -- from unswapped it always swaps --, so the binomial error is an upper bound)."""
    import tempering_np
    R, T, K, d, visits, burn = 50, 2, 2, 1, 200, 10
    beta = np.array([1.0, 0.3])
    st = _state(np.random.default_rng(0), R, T, K, d)
    st['loglik'] = np.tile(np.array([[-1.0], [0.0]]), (R, K))
    st['logprior'] = np.zeros((R * T, K))
    theta0 = st['theta'].copy()
    delta = (beta[0] - beta[1]) * (0.0 - -1.0)
    assert delta == pytest.approx(0.7)
    frozen, zeros = np.full((R * T, K // 2), -np.inf), np.zeros((R * T, K // 2))
    swapped = draws = 0
    for s in range(2 * 2 * (visits + burn) + 1):
        st, _, _, swaps = tempering_np.step(st, frozen, zeros, beta, seed=(3 << 32) + 9, copy=False)
        if swaps is not None and swaps['pairs'] and s // 4 > burn:          # step n = s / 2 visits the pair when n is even
            swapped += int((st['loglik'][0::2] == 0.0).sum())
            draws += R * K
    assert draws == 20000 and not st['accepted'].any()
    assert np.array_equal(np.sort(st['theta'].reshape(R, T * K), axis=1), np.sort(theta0.reshape(R, T * K), axis=1))
    p = np.exp(delta) / (1.0 + np.exp(delta))
    got, margin = swapped / draws, 4.0 * np.sqrt(p * (1.0 - p) / draws)
    print(f'swapped {got:.4f}, expected {p:.4f}, margin {margin:.4f}')
    assert abs(got - p) <= margin, (got, p, margin)
    assert st['swap_accepted'].sum() / st['swap_attempts'].sum() == pytest.approx(2 * p * np.exp(-delta), abs=3 * margin)
