"""
What DeviceEGVM, GreedyBatch and DeviceBeamSearch share (`_NetStepped` in librubiks_amd/solving/agents.py), without a GPU: the three
are its subclasses, a fresh agent owns nothing, and `_free` on an agent that owns nothing does nothing, however often it is called.
"""
import numpy as np
import pytest

from librubiks_amd.solving.agents import _KeptGraph, _NetStepped, DeviceBeamSearch, DeviceEGVM, GreedyBatch


class Net:
	def eval(self):
		return self


MAKE = {
	"egvm": lambda: DeviceEGVM(Net(), 0.3, 3, 4, poll=2),
	"greedy": lambda: GreedyBatch(Net(), "value", 4),
	"beam": lambda: DeviceBeamSearch(Net(), 22, 9),
}
GRAPHS = {"egvm": 2, "greedy": 1, "beam": 1}


@pytest.mark.parametrize("name", sorted(MAKE))
def test_fresh_agent_owns_nothing_and_free_is_a_no_op(name):
	agent = MAKE[name]()
	assert isinstance(agent, _NetStepped) and type(agent).__mro__[1] is _NetStepped
	for method in ("_net_in", "_free", "_net_batches", "_kept_steps", "_strict_ints"):
		assert method not in vars(type(agent)), method                 # one copy, the base's
	holders = agent._holders()
	assert len(holders) == GRAPHS[name]
	assert holders == (agent,) or all(isinstance(g, _KeptGraph) for g in holders)
	for _ in range(2):
		assert agent._h is None and agent.captures == 0 and agent._batch is None
		assert all(g._graph_cache is None and g.captures == 0 for g in holders)
		agent._free()


@pytest.mark.parametrize("name", sorted(MAKE))
def test_free_drops_graphs_and_batches_before_the_engine(name, monkeypatch):
	"""On an agent that holds something (stand-ins): when the engine is destroyed, the graphs and the batch tensors are gone."""
	from librubiks_amd import _ffi
	seen = []

	class Lib:
		def destroy(self, h):
			seen.append((h, agent._batch, [g._graph_cache for g in agent._holders()]))

	agent = MAKE[name]()
	for g in agent._holders():
		g._graph_cache = ("key", "graph")
	agent._batch = (0, "tensor")
	agent._h, agent._destroy = "engine", "destroy"
	monkeypatch.setattr(_ffi, "lib", Lib)
	agent._free()
	agent._free()
	assert seen == [("engine", None, [None] * GRAPHS[name])] and agent._h is None


@pytest.mark.parametrize("bad", [True, False, 2.0, "4", None, 0, -1, 6, np.float32(2), np.bool_(True)])
def test_strict_integers_refuse(bad):
	with pytest.raises(ValueError, match=r"^n must be an integer in 1\.\.5, got "):
		_NetStepped._strict_ints(("m", 1, 5), ("n", bad, 5))


def test_strict_integers_accept():
	got = _NetStepped._strict_ints(("a", 1, 5), ("b", np.int64(5), 5), ("c", np.uint8(2), 2))
	assert got == [1, 5, 2] and all(type(v) is int for v in got)
