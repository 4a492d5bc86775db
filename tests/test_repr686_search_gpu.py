"""
The search engines with a net of the 6x8x6 representation (cube.set_is2024(False)): they run on 20-byte states and hand the net
the 6x8x6 one-hot of each (rk_oh686_from2024).  Every array must equal the unmodified reference's 6x8x6 run with the same exact
stub net (tests/golden/repr686_search.npz, tools/gen_golden_repr686.py).
"""
import os

import numpy as np
import pytest
import torch

from librubiks_amd import cube
from librubiks_amd.solving.agents import AStar, AStarBatch, EGVM, MCTS, MCTSBatch, ValueSearch
from tests.repr686_nets import StubNet686, NoisyStubNet686, PolicyStubNet686
from tests.test_repr686_cpu import as_states

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def trace():
	with np.load(os.path.join(GOLDEN, "repr686_search.npz")) as z:
		return {k: z[k] for k in z.files}


def _astar_net(t, tag, dtype=torch.float32):
	return NoisyStubNet686(1, dtype) if int(t[f"astar_{tag}_params"][4]) else StubNet686(dtype)


def _check_astar(t, tag, states, G, parents, pact, queue, n, solved):
	p = f"astar_{tag}_"
	assert n == int(t[p + "n"]) and solved == bool(t[p + "solved"])
	assert states.shape[1:] == (6, 8, 6) and (states[1:n + 1] == as_states(t[p + "states"])).all()
	assert (G[1:n + 1] == t[p + "G"]).all()
	assert (parents[2:n + 1] == t[p + "parents"]).all() and (pact[2:n + 1] == t[p + "parent_actions"]).all()
	assert list(queue) == t[p + "action_queue"].tolist()


@pytest.mark.parametrize("mode", ["eager", "hipgraph", "exact_batch", "bf16"])
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_astar_equals_reference(trace, tag, mode):
	t, p = trace, f"astar_{tag}_"
	seed, depth, N, max_states, _ = (int(x) for x in t[p + "params"])
	cube.set_is2024(False)
	agent = AStar(_astar_net(t, tag, torch.bfloat16 if mode == "bf16" else torch.float32), float(t[p + "lambda"]), N,
	              use_hipgraph=mode == "hipgraph", exact_batch=mode == "exact_batch")
	agent.record_pops = mode == "eager"
	solved = agent.search(t[p + "start"], time_limit=None, max_states=max_states)
	_check_astar(t, tag, agent.states, agent.G, agent.parents, agent.parent_actions, agent.action_queue, len(agent), solved)
	if agent.record_pops:
		assert [len(q) for q in agent.pops] == t[p + "pop_lens"].tolist()
		assert (np.concatenate(agent.pops) == t[p + "pops"]).all()
	root = as_states(t[p + "states"][:1])[0]
	assert agent.index_of(root) == 1
	if mode == "hipgraph":
		captures = agent.captures
		assert agent.search(t[p + "start"], time_limit=None, max_states=max_states) == solved
		assert agent.captures == captures                                       # the stable adapter: the kept graph is replayed
		_check_astar(t, tag, agent.states, agent.G, agent.parents, agent.parent_actions, agent.action_queue, len(agent), solved)
	cube.set_is2024(True)                                                       # the exports follow the search, not the switch
	agent._cache = None
	assert agent.states.shape[1:] == (6, 8, 6)


@pytest.mark.parametrize("compact", [False, True])
def test_astar_batch_equals_each_single_trace(trace, compact):
	t = trace
	cube.set_is2024(False)
	# one engine holds one lambda and N: three searches of case a side by side
	p = "astar_a_"
	seed, depth, N, max_states, _ = (int(x) for x in t[p + "params"])
	agent = AStarBatch(StubNet686(), float(t[p + "lambda"]), N, 3, capacity=max_states + 16)
	solved = agent.search(np.stack([t[p + "start"]] * 3), max_states=max_states, exact_batch=compact)
	for s in range(3):
		st, G, par, pact = agent.arrays_of(s)
		_check_astar(t, "a", st, G, par, pact, agent.action_queue_of(s), len(st) - 1, bool(solved[s]))


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("batch", [False, True])
def test_mcts_equals_reference(trace, tag, batch):
	t, p = trace, f"mcts_{tag}_"
	seed, depth, graph, max_states, policy = (int(x) for x in t[p + "params"])
	net = PolicyStubNet686() if policy else StubNet686()
	cube.set_is2024(False)
	if batch:
		agent = MCTSBatch(net, float(t[p + "c"]), 3, capacity=max_states + 16, search_graph=bool(graph))
		solved = agent.search(np.stack([t[p + "start"]] * 3), max_states=max_states, use_graph=True)
		trees = [(agent.tree_arrays(k), agent.action_queue_of(k), bool(solved[k])) for k in range(3)]
	else:
		agent = MCTS(net, float(t[p + "c"]), bool(graph))
		solved = agent.search(t[p + "start"], time_limit=None, max_states=max_states)
		trees = [(agent._export(), agent.action_queue, solved)]
	n = int(t[p + "n"])
	for arr, queue, ok in trees:
		assert ok == bool(t[p + "solved"]) and arr["n"] == n
		assert arr["states"].shape[1:] == (6, 8, 6) and (arr["states"][1:n + 1] == as_states(t[p + "states"])).all()
		assert (arr["neighbors"][1:n + 1] == t[p + "neighbors"]).all() and (arr["leaves"][1:n + 1] == t[p + "leaves"]).all()
		for k in ("N", "W", "L", "V", "P"):
			assert (arr[k][1:n + 1] == t[p + k]).all(), k
		assert list(queue) == t[p + "action_queue"].tolist()


def test_egvm_and_value_search_equal_reference(trace):
	t = trace
	agents = {"egvm": lambda: EGVM(NoisyStubNet686(2), epsilon=0.3, workers=20, depth=8),
	          "egvm_policy": lambda: EGVM(PolicyStubNet686(), epsilon=0.5, workers=16, depth=6),
	          "value": lambda: ValueSearch(StubNet686()), "value_3": lambda: ValueSearch(StubNet686())}
	for tag, make in agents.items():
		seed, depth, max_states = (int(x) for x in t[f"{tag}_params"])
		cube.set_is2024(False)
		np.random.seed(seed)
		state, _, _ = cube.scramble(depth, True)
		assert (state == t[f"{tag}_start"]).all()
		agent = make()
		solved = agent.search(state, time_limit=None if "egvm" in tag else 30, max_states=max_states)
		assert solved == bool(t[f"{tag}_solved"]) and len(agent) == int(t[f"{tag}_len"]), tag
		assert [int(a) for a in agent.action_queue] == t[f"{tag}_action_queue"].tolist(), tag
		assert np.random.randint(0, 2 ** 31 - 1) == int(t[f"{tag}_rng_after"]), tag


def test_refusals(trace):
	t = trace
	cube.set_is2024(False)
	with pytest.raises(ValueError, match="fused_first_layer"):
		AStar(StubNet686(), 0.5, 10, fused_first_layer=True).search(t["astar_a_start"], max_states=1000)
	from librubiks_amd.solving.sharded import ShardedAStar
	with pytest.raises(NotImplementedError):
		ShardedAStar(StubNet686(), 0.5, 10, capacity=2000).search(t["astar_a_start"], max_states=1000)
