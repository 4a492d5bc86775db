"""
DeviceBFS (engine rk_bfs_*) against the reference's BFS (agents.py:92-129):
  * every case of tests/golden/bfs_trace.npz (tools/gen_golden_bfs.py), in both representations and with the cut landing inside
    a batch and on its edges (pops 1, 7, 4096): return value, len, action queue, the states dict's digest and its first keys;
  * the evaluator's BFS fixtures, played through the agent protocol;
  * the pool of the host agent `agents.BFS` at 5e5 states, node for node;
  * the level sizes of the quarter-turn Cayley graph up to depth 7 (about 9.2 M states, no fixture);
  * growth of the pool, an exhausted pool, a solved start, an illegal 6x8x6 start, repeated searches on one agent;
  * a search stopped by its budget and resumed with a larger one (rk_bfs_set_budget) = one search with the larger budget.
"""
import ctypes as C
import hashlib
import os
import warnings

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import CapacityExhausted, DeviceBFS
from librubiks_amd.solving.evaluation import Evaluator

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRACE = np.load(os.path.join(GOLDEN, "bfs_trace.npz"))
EVAL = np.load(os.path.join(GOLDEN, "evaluator_trace.npz"))
TAGS = sorted({k[:-len("_params")] for k in TRACE.files if k.endswith("_params")})
REPRS = ("2024", "686")

#: states at distance 0 .. 7 in the quarter-turn metric (the same from every vertex of the Cayley graph)
LEVELS = [1, 12, 114, 1_068, 10_011, 93_840, 878_880, 8_221_632]


def digest(states: dict) -> str:
	"""tools/gen_golden_bfs.py::digest."""
	h = hashlib.sha256()
	for k, (p, a) in states.items():
		h.update(k)
		h.update(p if p is not None else b"")
		h.update(bytes([255 if a is None else int(a)]))
	return h.hexdigest()


def _case(tag, rep):
	return (TRACE[f"{tag}_{rep}_start"], int(TRACE[f"{tag}_params"][2]), TRACE[f"{tag}_{rep}_result"],
	        TRACE[f"{tag}_{rep}_queue"].tolist(), str(TRACE[f"{tag}_{rep}_sha"]), TRACE[f"{tag}_{rep}_keys"])


def _check_case(agent, tag, rep):
	start, budget, result, queue, sha, keys = _case(tag, rep)
	cube.set_is2024(rep == "2024")
	ok = agent.search(start.copy(), max_states=budget)
	assert [int(ok), len(agent), len(agent.action_queue)] == result.tolist(), (tag, rep)
	assert list(agent.action_queue) == queue
	states = agent.states
	assert len(states) == len(agent)
	got_keys = list(states)[:len(keys)]
	assert [np.frombuffer(k, np.uint8).tolist() for k in got_keys] == keys.tolist()
	assert digest(states) == sha, (tag, rep)


def _scramble(seed: int, depth: int = 40) -> np.ndarray:
	rng = np.random.RandomState(seed)
	s = cube.get_solved()
	for a in rng.randint(0, 12, depth):
		s = cube.rotate(s, *cube.action_space[a])
	return s


def _depths(parents: np.ndarray) -> np.ndarray:
	"""Depth of every node from its parent index (nodes 1..n, the start's parent is 0): a node's parent comes earlier."""
	d = np.zeros(len(parents), np.int64)
	p = parents[1:] - 1
	for _ in range(64):
		nxt = d[p] + 1
		if (nxt == d[1:]).all():
			return d
		d[1:] = nxt
	raise AssertionError("parent chains longer than 64")


@pytest.mark.parametrize("pops", [1, 7, 4096])
@pytest.mark.parametrize("rep", REPRS)
@pytest.mark.parametrize("tag", TAGS)
def test_reference_parity(tag, rep, pops):
	_check_case(DeviceBFS(pops=pops, poll=64 if pops == 1 else 8), tag, rep)


@pytest.mark.parametrize("tag", ["bfs", "bfs_budget"])
def test_through_the_evaluator(tag):
	seed, games, max_states, deep = (int(x) for x in EVAL[f"{tag}_params"])
	np.random.seed(seed)
	ev = Evaluator(games, range(0) if deep else [int(d) for d in EVAL[f"{tag}_depths"]], None, max_states)
	res, states, _ = ev.eval(DeviceBFS(pops=512), batched=False)
	assert ev.last_mode == "sequential"
	assert (res == EVAL[f"{tag}_res"]).all() and (states == EVAL[f"{tag}_states"]).all()
	with pytest.raises(TypeError):
		Evaluator(2, [2], max_states=500).eval(DeviceBFS(), batched=True)


def test_against_the_host_agent_at_scale():
	start = _scramble(7)
	host = agents.BFS()
	assert not host.search(start, max_states=500_000)
	dev = DeviceBFS(pops=8192)
	assert not dev.search(start, max_states=500_000)
	assert len(dev) == len(host) >= 500_000
	states, parents, actions = dev.arrays()
	keys = list(host.states)
	assert (np.frombuffer(b"".join(keys), np.int8).reshape(-1, 20) == states).all()
	index = {k: i + 1 for i, k in enumerate(keys)}
	want_p = np.array([0 if p is None else index[p] for p, _ in host.states.values()], np.int64)
	want_a = np.array([-1 if a is None else a for _, a in host.states.values()], np.int64)
	assert (parents == want_p).all() and (actions == want_a).all()


def test_level_sizes_to_depth_7():
	# the list first, against the oracle's BFS to depth 5 (105 056 states)
	from oracle.search_oracle import BFSOracle
	start = _scramble(40)
	orc = BFSOracle()
	assert not orc.search(start.copy(), max_states=sum(LEVELS[:6]))
	keys = list(orc.states)
	index = {k: i for i, k in enumerate(keys)}
	depth = np.zeros(len(keys), np.int64)
	for i, (p, _) in enumerate(orc.states.values()):
		if p is not None:
			depth[i] = depth[index[p]] + 1
	assert np.bincount(depth).tolist() == LEVELS[:6]
	# then the device search to depth 7: 9.2 M states, dedup against everything seen
	agent = DeviceBFS(pops=16_384)
	assert not agent.search(start, max_states=sum(LEVELS))
	assert len(agent) == sum(LEVELS)
	_, parents, _ = agent.arrays()
	assert np.bincount(_depths(parents)).tolist() == LEVELS


@pytest.mark.parametrize("pops", [7, 64])
def test_growth_changes_nothing(pops):
	for tag in ("d5_solved", "d6_large", "d4_budget"):
		for rep in REPRS:
			agent = DeviceBFS(pops=pops, capacity=1_000, poll=16)
			_check_case(agent, tag, rep)
			if len(agent) > 4_000:
				assert agent.grown >= 2
			assert not agent.capacity_exhausted
	big = DeviceBFS(pops=pops, capacity=400_000)
	small = DeviceBFS(pops=pops, capacity=1_000)
	start = _scramble(11)
	assert not big.search(start, max_states=150_000) and not small.search(start, max_states=150_000)
	assert big.grown == 0 and small.grown >= 5
	for x, y in zip(big.arrays(), small.arrays()):
		assert (x == y).all()


def test_exhausted_pool_warns():
	agent = DeviceBFS(pops=64, capacity=1_000, max_capacity=4_000)
	with pytest.warns(CapacityExhausted):
		assert not agent.search(_scramble(12), max_states=100_000)
	assert agent.capacity_exhausted and 0 < len(agent) <= 4_000
	agent = DeviceBFS(pops=4096, capacity=1_000, max_capacity=20_000)          # cannot take even one iteration
	with pytest.warns(CapacityExhausted):
		assert not agent.search(_scramble(12), max_states=100_000)
	assert agent.capacity_exhausted and agent.iterations == 0


def test_solved_and_illegal_starts_and_repeated_searches():
	agent = DeviceBFS(pops=7)
	for rep in REPRS:
		cube.set_is2024(rep == "2024")
		assert agent.search(cube.get_solved(), max_states=100)
		assert len(agent) == 0 and list(agent.action_queue) == [] and agent.states == {}
	cube.set_is2024(False)
	bad = np.zeros((6, 8, 6), np.int8)
	with pytest.raises(ValueError):
		agent.search(bad, max_states=100)
	cube.set_is2024(True)
	# one agent, several searches: none sees the table of the one before
	with warnings.catch_warnings():
		warnings.simplefilter("error")
		for tag, rep in [("d5_solved", "2024"), ("d6_large", "686"), ("d5_solved", "2024"), ("d3_budget", "686"), ("d4_solved", "2024")]:
			_check_case(agent, tag, rep)
	# a budget of one state: the start alone, as the reference's loop guard (agents.py:105)
	cube.set_is2024(True)
	assert not agent.search(_scramble(3), max_states=1) and len(agent) == 1


def _run_to_end(agent):
	"""Drives the agent's engine through the C ABI until it is done; the agent then exports what the engine holds."""
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	st = (C.c_longlong * 8)()
	_ffi.check(lib.rk_bfs_status(agent._h, st, stream))
	while not st[0]:
		_ffi.check(lib.rk_bfs_run(agent._h, 1, stream))
		_ffi.check(lib.rk_bfs_status(agent._h, st, stream))
	assert st[6] == 0
	agent._n, agent._cache = int(st[2]), None
	return list(st)


@pytest.mark.parametrize("pops", [7, 4096])
def test_resume_after_a_budget_stop(pops):
	"""A budget stop inside a batch leaves tentative claims in the table; rk_bfs_set_budget must drop them before the search goes on."""
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	start = _scramble(21)
	once = DeviceBFS(pops=pops, capacity=200_000)
	assert not once.search(start, max_states=60_001)
	for b1 in (1_237, 12_347, 30_011):
		resumed = DeviceBFS(pops=pops, capacity=200_000)
		assert not resumed.search(start, max_states=b1)
		assert b1 <= len(resumed) < b1 + 12
		_ffi.check(lib.rk_bfs_set_budget(resumed._h, 60_001, stream))
		st = _run_to_end(resumed)
		assert st[5] == 2 and len(resumed) == len(once)
		for x, y in zip(once.arrays(), resumed.arrays()):
			assert (x == y).all()
	# a budget the pool already holds stops the search again at once
	_ffi.check(lib.rk_bfs_set_budget(resumed._h, len(resumed), stream))
	assert _run_to_end(resumed)[2] == len(once)


def test_c_entries_refuse_bad_arguments():
	lib = _ffi.lib()
	h = C.c_void_p()
	_ffi.check(lib.rk_bfs_create(C.byref(h), 1_000, 8))
	try:
		buf = np.zeros(20, np.int8)
		assert lib.rk_bfs_export(h, 1, 1, buf.ctypes.data, None, None, _ffi.stream_ptr()) == -4       # RK_ESTATE: not reset
		assert lib.rk_bfs_path(h, None, 16, _ffi.stream_ptr()) == -4
		start = _scramble(5)
		_ffi.check(lib.rk_bfs_reset(h, start.ctypes.data, 100, _ffi.stream_ptr()))
		assert lib.rk_bfs_path(h, None, 16, _ffi.stream_ptr()) == -1                                    # RK_EINVAL: null output
	finally:
		lib.rk_bfs_destroy(h)
