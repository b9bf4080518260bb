"""The recorded loop the device samplers and searches share (hallthrusterpem_amd/_device_loop.py), on a toy body."""
import pytest
import torch

from hallthrusterpem_amd import _device_loop as loop

pytestmark = pytest.mark.gpu


class Toy(loop.TracedLoop):
    """state: x (4,) float64 and an int64 step counter; a step adds 1 + salt to x and 1 to the counter and writes x into the
    trace row the window gives this step.  salt, the trace and the window reach a recording by value."""

    def __init__(self, use_graph: bool):
        self._init_loop(None, use_graph)
        z = loop.zeros_on(self.device)
        self.x, self.count = z(4), z(1, dt=torch.int64)
        self.steps, self.salt, self.calls = 0, 0.0, 0
        self._init_trace((4,))

    def _state(self):
        return (self.x, self.count)

    def _record_key(self):
        return super()._record_key() + (self.salt,)

    def _step(self):
        self.calls += 1
        self.x += 1.0 + self.salt
        self.count += 1
        trace = self._traces[0]
        if trace is not None:
            first, length, thin = self._window
            hit = torch.arange(length, device=self.device) * thin == self.count - 1 - first    # row r holds step first + 1 + r thin
            trace.copy_(torch.where(hit[:, None], self.x[None, :], trace))

    _body = _step


def test_recording_leaves_the_state_as_it_was_after_running_the_body_three_times():
    toy = Toy(True)
    toy.x.copy_(torch.tensor([1.0, 2.0, 3.0, 4.0]))
    toy.count.fill_(7)
    toy._prepare()
    assert toy.calls == 3 and toy._graph is not None                                  # two warm-ups and the capture
    assert toy.x.tolist() == [1.0, 2.0, 3.0, 4.0] and toy.count.item() == 7


def test_advance_gives_the_same_state_replayed_and_eager():
    states = []
    for use_graph in (True, False):
        toy = Toy(use_graph)
        toy._prepare()
        toy.advance(5)
        states.append((toy.x.tolist(), toy.count.item()))
        assert (toy._graph is not None) == use_graph and toy.calls == (3 if use_graph else 5)
    assert states[0] == states[1] == ([5.0] * 4, 5)


def test_a_changed_record_key_and_only_that_records_again():
    toy = Toy(True)
    toy._prepare()
    graph = toy._graph
    toy.advance(1)
    toy._prepare()
    assert toy._graph is graph and toy.calls == 3                                     # the same key: the same recording
    toy.salt = 1.0
    toy._prepare()
    assert toy._graph is not graph and toy.calls == 6
    toy.advance(1)
    assert toy.x.tolist() == [3.0] * 4 and toy.count.item() == 2                       # 1, then 1 + salt: the new recording ran


@pytest.mark.parametrize('use_graph', [True, False])
def test_a_second_run_writes_its_own_trace_and_leaves_the_first_alone(use_graph):
    toy = Toy(use_graph)
    first, = toy._run(5, 2, (True,))                                                  # steps 1, 3, 5
    assert first.shape == (3, 4) and first[:, 0].tolist() == [1.0, 3.0, 5.0] and bool((first == first[:, :1]).all())
    kept = first.clone()
    graph = toy._graph
    second, = toy._run(4, 2, (True,))                                                 # steps 6, 8 of the chain
    assert second.data_ptr() != first.data_ptr() and second[:, 0].tolist() == [6.0, 8.0]
    assert torch.equal(first, kept)                                                   # a stale recording would have written here
    assert toy.steps == 9 and toy.count.item() == 9 and toy._window == (0, 0, 1) and toy._traces == (None,)
    assert (toy._graph is not graph) == use_graph
    assert toy._run(0, 1, (True,))[0].shape == (0, 4) and toy._run(3, 1, (False,)) == (None,)
