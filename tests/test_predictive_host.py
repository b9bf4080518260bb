"""predictive.Predictive on the host (no GPU): the C ABI of its three launches, burn-in and flattening as monte_carlo.py:44-46,
what `run` refuses, relative_l2 and the table of print_l2_error (monte_carlo.py:303-336) against numpy, and the resources of the
record-prediction kernel (JMODE 7 of plume_r1_kernel)."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from hallthrusterpem_amd import _lib
from hallthrusterpem_amd.likelihood import SystemLikelihood
from hallthrusterpem_amd.predictive import Predictive, flatten_chain, l2_table, relative_l2

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ('pem_coupled_system_predict_f64_dev', 'pem_predictive_inputs_f64_dev', 'pem_predictive_noise_f64_dev')


def _lik():
    rng = np.random.default_rng(0)
    x = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
    na = 4                                                             # padded to 5 records per condition
    return SystemLikelihood({
        'V_cc': {'x': x(2), 'y': rng.uniform(15, 35, 2), 'var_y': np.ones(2)},
        'T': {'x': x(3), 'y': rng.uniform(0.05, 0.1, 3), 'var_y': np.full(3, 1e-4)},
        'jion': {'x': x(2), 'y': rng.lognormal(0, 1, (2, na)), 'var_y': np.full((2, na), 0.25),
                 'loc': np.stack([np.ones(na), np.linspace(0, 1.5, na)], 1)}}, device='cpu')


def test_the_new_entry_points_are_declared_bound_and_exported():
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(rf'\bint {name}\(', header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    # the prediction launch takes the likelihood launch's arguments with `loglik` replaced by `pred`, `ld_pred`
    ll = _lib.SIGNATURES['pem_coupled_system_loglik_f64_dev'][1]
    pr = _lib.SIGNATURES['pem_coupled_system_predict_f64_dev'][1]
    assert len(pr) == len(ll) + 1 and pr[:-4] == ll[:-3] and pr[-3] is _lib._sz


def test_burn_in_and_flattening_follow_monte_carlo():
    trace = np.random.default_rng(1).normal(size=(50, 4, 3))
    want = trace[int(0.1 * 50):, ...].reshape((-1, 3))                # monte_carlo.py:44-46
    assert np.array_equal(flatten_chain(trace, 0.1), want)
    assert np.array_equal(flatten_chain(trace, 0.0), trace.reshape(-1, 3))
    assert flatten_chain(trace, 0.33).shape == (4 * (50 - 16), 3)
    table = trace[0]
    assert flatten_chain(table, 0.5) is table                         # an (S, d) table has no steps to burn
    assert flatten_chain(trace[:1], 0.9).shape == (4, 3)              # int(0.9 * 1) = 0 steps dropped
    with pytest.raises(ValueError, match='no samples'):
        flatten_chain(trace[:0], 0.1)
    with pytest.raises(ValueError, match='no samples'):
        flatten_chain(trace[:, :0], 0.1)
    with pytest.raises(ValueError, match='burnin'):
        flatten_chain(trace, 1.0)


def test_flattening_keeps_step_major_order_of_torch_traces():
    torch = pytest.importorskip('torch')
    trace = torch.arange(5 * 2 * 3, dtype=torch.float64).reshape(5, 2, 3)
    assert torch.equal(flatten_chain(trace, 0.2), trace[1:].reshape(-1, 3))


def test_run_refuses_bad_arguments_before_touching_a_device():
    lik = _lik()
    with pytest.raises(KeyError, match='calibratable'):
        Predictive(lik, ('T_e', 'V_a'))                                # an operating input
    with pytest.raises(KeyError, match='calibratable'):
        Predictive(lik, ('T_e', 'nope'))
    with pytest.raises(ValueError, match='repeat'):
        Predictive(lik, ('T_e', 'T_e'))
    pp = Predictive(lik, ('T_e', 'c0'))
    with pytest.raises(ValueError, match='one column per'):
        pp.run(samples=np.zeros((10, 3)), n_draws=4)
    with pytest.raises(ValueError, match='one column per'):
        pp.run(samples=np.zeros((10, 2, 3)), n_draws=4)
    with pytest.raises(ValueError, match='one column per'):
        pp.run(samples=np.zeros(10), n_draws=4)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='n_draws'):
            pp.run(samples=None, n_draws=bad)
    with pytest.raises(ValueError, match='no samples'):
        pp.run(samples=np.zeros((0, 4, 2)), n_draws=4)
    with pytest.raises(ValueError, match='burnin'):
        pp.run(samples=np.zeros((10, 4, 2)), n_draws=4, burnin=1.0)
    with pytest.raises(ValueError, match='no samples'):
        pp.run(samples=np.zeros((0, 2)), n_draws=4)


def test_column_map_drops_the_padding_records_and_sigma_is_the_mean_std():
    lik = _lik()
    pp = Predictive(lik, ('c0',))
    cols = pp.cols.numpy()
    span = lik.span.numpy()
    assert pp.n_cols == 2 + 3 + 2 * 4 and len(np.unique(cols)) == pp.n_cols and np.all(np.diff(cols) > 0)
    assert lik.n_rec > pp.n_cols                                       # the table has padding records, the columns do not
    assert pp.views == {'V_cc': (0, 2, (2,)), 'T': (2, 5, (3,)), 'jion': (5, 13, (2, 4))}
    assert np.array_equal(cols[5:9], np.arange(span[5, 0, 0], span[5, 0, 0] + 4))
    assert np.array_equal(cols[9:13], np.arange(span[6, 0, 0], span[6, 0, 0] + 4)) and span[6, 0, 0] == span[5, 0, 0] + 5
    sig = pp.sigma.numpy()
    assert np.all(sig[:2] == 1.0) and np.allclose(sig[2:5], 1e-2) and np.all(sig[5:] == 0.5)   # mean(sqrt(var_y)), :358-359


def test_relative_l2_and_the_table_restate_monte_carlo():
    rng = np.random.default_rng(2)
    pred, y = rng.normal(1, 0.2, (100, 3, 7)), rng.normal(1, 0.1, (3, 7))
    want = np.sqrt(np.mean((pred - y) ** 2, axis=-1) / np.mean(y ** 2, axis=-1))     # monte_carlo.py:303-305
    assert np.array_equal(relative_l2(pred, y), want)
    scalar_pred, scalar_y = rng.normal(20, 1, (100, 4)), rng.normal(20, 1, 4)
    assert relative_l2(scalar_pred, scalar_y).shape == (100,)
    torch = pytest.importorskip('torch')
    assert np.allclose(relative_l2(torch.as_tensor(pred), y).numpy(), want, rtol=1e-14, atol=0)
    e_prior, e_post = want * 3, want
    text = l2_table({'jion': (e_prior, e_post), 'V_cc': (relative_l2(scalar_pred, scalar_y), relative_l2(scalar_pred, scalar_y) / 2)},
                    {'jion': 0.2, 'V_cc': 0.01})
    lines = text.splitlines()
    assert lines[0].split() == ['Case', 'Prior', 'mu', 'Prior', 's', 'Prior', 'r', 'Post', 'mu', 'Post', 's', 'Post', 'r']
    row = lines[1].split()
    assert row[0] == 'jion'
    want_row = [np.mean(e_prior), np.std(e_prior), np.mean(e_prior) / 0.2, np.mean(e_post), np.std(e_post), np.mean(e_post) / 0.2]
    assert row[1:] == [f'{v:.3f}' for v in want_row]
    assert lines[2].split()[0] == 'V_cc' and len(lines) == 3


def test_record_prediction_kernel_has_no_spills_and_no_scratch():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_kernels.hip'),
                          '--grep', 'plume_r1_kernel'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\w+(?:<[^>]*>)?)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), vspill=int(m.group(5)), scratch=int(m.group(6)))
    r = rows.get('plume_r1_kernel<4, true, 7, false, 0, false>')
    assert r is not None, sorted(rows)
    assert r['vgpr'] <= 256 and r['vspill'] == 0 and r['scratch'] == 0, r
