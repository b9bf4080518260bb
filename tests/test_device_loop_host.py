"""The pieces the device samplers and searches share on the host (hallthrusterpem_amd/_device_loop.py), without a device."""
import numpy as np
import pytest
import torch

from hallthrusterpem_amd import _device_loop as loop
from hallthrusterpem_amd.samplers import DeviceEnsemble, DeviceTemperedEnsemble


@pytest.mark.parametrize('shape', [(3,), (5, 3)])
@pytest.mark.parametrize('as_tensor', [False, True])
def test_starts_become_a_float64_array_and_a_tensor_names_its_device(shape, as_tensor):
    x = np.arange(np.prod(shape), dtype=np.float32).reshape(shape)
    t0, device = loop.starts(torch.from_numpy(x) if as_tensor else x.tolist())
    assert isinstance(t0, np.ndarray) and t0.dtype == np.float64 and t0.shape == shape and np.array_equal(t0, x)
    assert device == (torch.device('cpu') if as_tensor else None)
    assert loop.starts(torch.from_numpy(x), device='cuda:1')[1] == 'cuda:1'          # a device that was asked for wins


def test_starts_refuse_what_is_no_array_of_numbers():
    for bad in ('tensor', [[1.0, 2.0], [3.0]], [1.0, 'x']):
        with pytest.raises(ValueError):
            loop.starts(bad)


def test_a_device_that_is_not_cuda_is_refused_with_the_class_name():
    with pytest.raises(ValueError, match=r"^Toy runs on the GPU only \(got device 'cpu'\): use X$"):
        loop.require_cuda('Toy', torch.device('cpu'), ': use X')
    loop.require_cuda('Toy', None)
    loop.require_cuda('Toy', 'cuda:0')


FAULTS = [                                                                             # K, d, keywords, the text
    (7, 3, {}, 'Toy needs an even number of walkers K with 2 d = 6 <= K <= 1024 per ensemble (got 7)'),            # odd K
    (4, 3, {}, 'Toy needs an even number of walkers K with 2 d = 6 <= K <= 1024 per ensemble (got 4)'),            # K < 2d
    (8, 3, dict(de_fraction=-0.1), 'de_fraction must be in [0, 1] (got -0.1)'),
    (8, 3, dict(de_fraction=1.5), 'de_fraction must be in [0, 1] (got 1.5)'),
    (2, 1, dict(de_fraction=0.5), 'the DE move needs two partners in the other half: K >= 4'),
    (8, 3, dict(a=1.0), 'need finite a > 1, g0 > 0 and sigma >= 0'),
    (8, 3, dict(a=0.5), 'need finite a > 1, g0 > 0 and sigma >= 0'),
]


@pytest.mark.parametrize('K, d, kw, text', FAULTS)
def test_ensemble_parameters_are_refused_with_one_text_by_both_ensemble_samplers(K, d, kw, text):
    full = dict(a=2.0, de_fraction=0.0, g0=None, sigma=1e-5)
    full.update(kw)
    with pytest.raises(ValueError) as shared:
        loop.ensemble_parameters('Toy', 1, K, d, **full)
    assert str(shared.value) == text
    f = lambda x: pytest.fail('evaluated a start')                                                      # noqa: E731
    raised = {}
    for cls, make in ((DeviceEnsemble, lambda: DeviceEnsemble(f, np.zeros((K, d)), **kw)),
                      (DeviceTemperedEnsemble, lambda: DeviceTemperedEnsemble(f, f, np.zeros((K, d)), **kw))):
        with pytest.raises(ValueError) as e:
            make()
        raised[cls] = str(e.value)
        assert raised[cls] == text.replace('Toy', cls.__name__)                       # the same text, under the class's own name
    assert raised[DeviceEnsemble].replace('DeviceEnsemble', 'X') == raised[DeviceTemperedEnsemble].replace('DeviceTemperedEnsemble', 'X')


def test_ensemble_parameters_return_g0():
    assert loop.ensemble_parameters('Toy', 1, 8, 2, 2.0, 0.0, None, 1e-5) == 2.38 / np.sqrt(4.0)
    assert loop.ensemble_parameters('Toy', 1, 8, 2, 2.0, 0.0, 0.7, 0.0) == 0.7


@pytest.mark.parametrize('thin', [1, 2, 4])
@pytest.mark.parametrize('n_steps', [0, 1, 4, 5])
def test_trace_window_arithmetic(n_steps, thin):
    want = {0: 0, 1: 1, 4: {1: 4, 2: 2, 4: 1}[thin], 5: {1: 5, 2: 3, 4: 2}[thin]}[n_steps]     # 0, 1, then ceil(n / thin)
    rows, window = loop.trace_window(17, n_steps, thin)
    assert rows == want and window == ((17, want, thin) if want else (0, 0, 1))
    assert loop.trace_window(17, n_steps, thin, keep=False) == (want, (0, 0, 1))                # nothing kept: no window


def test_trace_window_refusals():
    for n_steps, thin in ((-1, 1), (3, 0)):
        with pytest.raises(ValueError, match='n_steps >= 0 and thin >= 1'):
            loop.trace_window(0, n_steps, thin)


def test_ball_is_the_draw_both_ensemble_samplers_make():
    rng = np.random.default_rng(5)
    want = np.array([1.0, -2.0]) + np.array([0.1, 0.2]) * rng.standard_normal((3, 6, 2))
    assert np.array_equal(loop.ball([1.0, -2.0], [0.1, 0.2], (3, 6), seed=5), want)
    assert np.array_equal(DeviceEnsemble.ball([1.0, -2.0], [0.1, 0.2], 6, n_ensembles=3, seed=5), want)
    got = DeviceTemperedEnsemble.ball([1.0, -2.0], [0.1, 0.2], 6, n_temperatures=3, seed=5)
    assert got.shape == (1, 3, 6, 2) and np.array_equal(got[0], want)
