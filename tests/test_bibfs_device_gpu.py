"""
DeviceBiBFS (engine rk_bibfs_*) on the GPU:
  * against the plain-Python model of the protocol (tests/bibfs_model.py), bit for bit: seeded scrambles of 1, 2, 3, 5, 6, 7 and 8
    moves, two seeds each, pops 1 / 7 / 4096 (the cut on a batch's edge, inside a batch, the whole level in one batch), in both
    representations: return value, queue, len, depths, meeting and arrays() -- and the three runs equal to each other;
  * optimality against the one-sided DeviceBFS on 7-move scrambles, and the queue solves the cube;
  * a 12-move scramble, deeper than one side reaches: the queue solves it, the depths follow from its length and the complete
    levels of both sides have the sizes of the quarter-turn Cayley graph;
  * the state budget, the pool (growth, exhaustion) and the edges (solved and illegal starts, all starts one move from solved).

Two statements of the issue that introduced the engine are narrowed here, because the protocol it sets decides otherwise:
  * depths: S grows first (f == b), so a solution of length L leaves (f, b) = (L // 2, (L + 1) // 2 - 1): (1, 0) for L = 2,
    not (0, 1).  The model, pinned against a one-sided search in tests/test_bibfs_device_cpu.py, says the same.
  * "a budget equal to the unbounded search's final len changes nothing" holds only where the pop that meets stores a child
    before the meeting: otherwise len was already final before that pop and the per-pop rule refuses it (a 1-move scramble
    undone by action 0 ends with len 2, and a budget of 2 stops before the first pop).  So every budget is compared with the
    model, and the equality with the unbounded run is asserted on a start where the model shows it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import CapacityExhausted, DeviceBFS, DeviceBiBFS
from tests import bibfs_model as model

pytestmark = pytest.mark.gpu

REPRS = ("2024", "686")
POPS = (1, 7, 4096)
STARTS = [(d, s) for d in (1, 2, 3, 5, 6, 7, 8) for s in (0, 1)]

#: states at distance 0 .. 7 in the quarter-turn metric (the same from every vertex of the Cayley graph)
LEVELS = [1, 12, 114, 1_068, 10_011, 93_840, 878_880, 8_221_632]


def _start(depth: int, seed: int) -> np.ndarray:
	return model.scramble(1000 * depth + seed, depth)


@functools.lru_cache(maxsize=None)
def _model(depth: int, seed: int, budget: int = None):
	return model.search(_start(depth, seed), max_states=budget)


def _in_repr(states20: np.ndarray) -> np.ndarray:
	"""20-byte states in the current representation."""
	return states20 if cube.get_is2024() else cube.as686(states20)


def _assert_equals_model(agent, ok, want):
	assert ok == want.result
	assert list(agent.action_queue) == want.queue
	assert len(agent) == want.len and agent.depths == want.depths
	if want.meeting is None:
		assert agent.meeting is None
	else:
		assert (agent.meeting == _in_repr(want.meeting)).all()
	states, parents, actions, sides = agent.arrays()
	assert states.dtype == np.int8 and states.shape[0] == want.len
	assert (states == _in_repr(want.states)).all()
	assert (parents == want.parents).all() and (actions == want.actions).all() and (sides == want.sides).all()


def _depths(parents: np.ndarray) -> np.ndarray:
	"""Depth of every node within its side from its parent index (row i = node i + 1; a node's parent comes earlier)."""
	d = np.zeros(len(parents), np.int64)
	p = np.maximum(parents - 1, 0)
	for _ in range(64):
		nxt = np.where(parents > 0, d[p] + 1, 0)
		if (nxt == d).all():
			return d
		d = nxt
	raise AssertionError("parent chains longer than 64")


@pytest.mark.parametrize("rep", REPRS)
@pytest.mark.parametrize("depth,seed", STARTS)
def test_against_the_model_and_independent_of_pops(depth, seed, rep):
	want = _model(depth, seed)
	assert want.result and want.len <= 2 * 11_200 + 2
	cube.set_is2024(rep == "2024")
	start = _in_repr(_start(depth, seed))
	runs = []
	for pops in POPS:
		agent = DeviceBiBFS(pops=pops, poll=64 if pops == 1 else 8)
		ok = agent.search(start.copy())
		_assert_equals_model(agent, ok, want)
		runs.append((ok, list(agent.action_queue), len(agent), agent.depths, agent.meeting, agent.arrays(), agent.popped))
	for other in runs[1:]:
		assert other[:4] == runs[0][:4] and other[6] == runs[0][6]
		assert (other[4] == runs[0][4]).all()
		for x, y in zip(other[5], runs[0][5]):
			assert (x == y).all()
	if len(want.queue) <= 2:                               # found in the first iteration of the side that grows
		assert want.depths == (len(want.queue) - 1, 0)


def test_optimal_against_the_one_sided_search():
	two, one = DeviceBiBFS(), DeviceBFS()
	lengths = []
	for seed in range(8):
		start = model.scramble(7000 + seed, 7)
		assert one.search(start.copy(), max_states=10_000_000)
		assert two.search(start.copy())
		assert len(two.action_queue) == len(one.action_queue) <= 7
		assert model.orc.is_solved(model.apply(start, two.action_queue))
		lengths.append(len(two.action_queue))
	assert max(lengths) == 7


def test_deeper_than_one_side_reaches():
	start = model.scramble(12_001, 12)
	agent = DeviceBiBFS()
	assert agent.search(start.copy())
	L = len(agent.action_queue)
	print(f"12-move scramble: length {L}, {len(agent)} states, depths {agent.depths}, {agent.iterations} iterations")
	assert L <= 12 and L % 2 == 0
	assert L == 12                                         # what the model finds for this seed (5 s of Python: not repeated here)
	assert model.orc.is_solved(model.apply(start, agent.action_queue))
	f, b = agent.depths
	assert (f, b) == (L // 2, (L + 1) // 2 - 1)            # S grows first (the module's docstring)
	states, parents, actions, sides = agent.arrays()
	depth = _depths(parents)
	for side, complete in ((0, f), (1, b)):
		sizes = np.bincount(depth[sides == side]).tolist()
		assert sizes[:complete + 1] == LEVELS[:complete + 1]
		assert len(sizes) <= complete + 2                   # at most the level that was growing beyond them
	assert (agent.meeting == model.apply(start, list(agent.action_queue)[:(L + 1) // 2])).all()


@pytest.mark.parametrize("pops", [7, 4096])
def test_budget(pops):
	depth, seed = 7, 0
	start = _start(depth, seed)
	full = _model(depth, seed)
	agent = DeviceBiBFS(pops=pops)
	# the budget the unbounded search ends with: on this start the meeting pop stores children first, so nothing changes
	same = _model(depth, seed, full.len)
	assert (same.result, same.queue, same.len) == (full.result, full.queue, full.len)
	ok = agent.search(start.copy(), max_states=full.len)
	_assert_equals_model(agent, ok, full)
	# smaller budgets: False, with the model's len and pool (2: before the first pop; 3: after one pop)
	for budget in (2, 3, 150, 5_000, full.len - 12):
		want = _model(depth, seed, budget)
		assert not want.result and budget <= want.len < budget + 12
		ok = agent.search(start.copy(), max_states=budget)
		_assert_equals_model(agent, ok, want)
	# where the meeting pop stores nothing before it meets, the same budget refuses that pop: the model's answer, not the unbounded one
	d2, s2 = 5, 0
	unbounded, cut = _model(d2, s2), _model(d2, s2, _model(d2, s2).len)
	assert unbounded.result and not cut.result and cut.len == unbounded.len
	ok = agent.search(_start(d2, s2), max_states=unbounded.len)
	_assert_equals_model(agent, ok, cut)
	# the agent is reusable: an unbounded search after those equals a fresh agent's
	ok = agent.search(start.copy())
	_assert_equals_model(agent, ok, full)
	fresh = DeviceBiBFS(pops=pops)
	assert fresh.search(start.copy()) == ok and list(fresh.action_queue) == list(agent.action_queue)
	for x, y in zip(fresh.arrays(), agent.arrays()):
		assert (x == y).all()


@pytest.mark.parametrize("pops", [7, 64])
def test_growth_changes_nothing(pops):
	for depth, seed in ((7, 0), (8, 1)):
		agent = DeviceBiBFS(pops=pops, capacity=2 * 12 * pops, poll=16)
		ok = agent.search(_start(depth, seed))
		assert agent.grown > 0 and not agent.capacity_exhausted
		_assert_equals_model(agent, ok, _model(depth, seed))


def test_exhausted_pool_warns():
	agent = DeviceBiBFS(pops=64, capacity=2 * 12 * 64, max_capacity=4_000)
	with pytest.warns(CapacityExhausted):
		assert not agent.search(_start(8, 0))
	assert agent.capacity_exhausted and 2 < len(agent) <= 4_000 and list(agent.action_queue) == []
	want = _model(8, 0)
	states, parents, _, sides = agent.arrays()
	assert (states == want.states[:len(agent)]).all() and (parents == want.parents[:len(agent)]).all()
	assert (sides == want.sides[:len(agent)]).all()


def test_solved_illegal_and_one_move_starts():
	agent = DeviceBiBFS(pops=7)
	for rep in REPRS:
		cube.set_is2024(rep == "2024")
		assert agent.search(cube.get_solved(), max_states=100)
		assert len(agent) == 0 and list(agent.action_queue) == [] and agent.depths == (0, 0) and agent.meeting is None
		assert [len(x) for x in agent.arrays()] == [0, 0, 0, 0]
		assert agent.iterations == 0 and agent.popped == 0
	cube.set_is2024(False)
	with pytest.raises(ValueError):
		agent.search(np.zeros((6, 8, 6), np.int8), max_states=100)
	for rep in REPRS:
		cube.set_is2024(rep == "2024")
		for a in range(12):
			start = cube.rotate(cube.get_solved(), *cube.action_space[a])
			assert agent.search(start)
			assert list(agent.action_queue) == [cube.rev_action(a)] and agent.depths == (0, 0)
			assert cube.is_solved(agent.meeting) and agent.popped == 1
			assert len(agent) == 2 + cube.rev_action(a)         # the children before the one that meets were stored


def test_c_entries_refuse_bad_arguments():
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	h = C.c_void_p()
	_ffi.check(lib.rk_bibfs_create(C.byref(h), 1_000, 8))
	try:
		buf = np.zeros(20, np.int8)
		assert lib.rk_bibfs_export(h, 1, 1, buf.ctypes.data, None, None, None, stream) == -4         # RK_ESTATE: not reset
		assert lib.rk_bibfs_path(h, None, 16, stream) == -4
		assert lib.rk_bibfs_run(h, 1, stream) == -4
		assert lib.rk_bibfs_reset(h, model.orc.SOLVED.ctypes.data, 100, stream) == -1                # RK_EINVAL: a solved start
		start = model.scramble(5, 5)
		_ffi.check(lib.rk_bibfs_reset(h, start.ctypes.data, 100, stream))
		assert lib.rk_bibfs_size(h) == 2
		assert lib.rk_bibfs_path(h, None, 16, stream) == -1                                          # RK_EINVAL: null output
		out = (C.c_longlong * 16)()
		assert lib.rk_bibfs_path(h, out, 16, stream) == -4                                           # RK_ESTATE: not met
		assert lib.rk_bibfs_export(h, 1, 1_001, buf.ctypes.data, None, None, None, stream) == -1     # rows outside the pool
		assert lib.rk_bibfs_grow(h, 500, stream) == -1
		# driven through the C ABI alone, one iteration per poll, to the budget
		st = (C.c_longlong * 12)()
		for _ in range(64):
			_ffi.check(lib.rk_bibfs_run(h, 1, stream))
			_ffi.check(lib.rk_bibfs_status(h, st, stream))
			if st[0]:
				break
		assert st[0] == 1 and st[1] == 0 and st[5] == 2 and 100 <= st[2] < 112                       # stopped by its budget
	finally:
		lib.rk_bibfs_destroy(h)
