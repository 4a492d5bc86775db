"""
DeviceBallSearchBatch (engine rk_bsearchb_*) on the GPU: every state of a batch gets what the plain-Python model
(tests/ball_model.py) and the single engine `DeviceBallSearch` give it alone, bit for bit.
  * the starts of tests/test_goal_ball_gpu.py (seeded scrambles of 1, 2, 3, 5, 6, 7 and 8 moves, two seeds each) against balls of
    radius 2 and 4 in one call, with 14, 5 and 1 slots (5: slots are refilled mid-run; 1: the single engine by another road),
    pops 1 / 7 / 4096, both representations: result, queue, len, depth, meeting depth and pool against the model, and the runs
    equal to each other;
  * the same starts one by one through DeviceBallSearch;
  * reversed input with a state five times over; a long search beside slots refilled at every poll;
  * optimality on 10- to 12-move starts against a radius-6 ball with DeviceBiBFS's lengths;
  * per-state budgets, a pool that is full, the edges, the C entries and the Evaluator.
The models and the device balls are those of tests/test_goal_ball_gpu.py, computed once per session.
"""
import ctypes as C

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import DeviceBallSearch, DeviceBallSearchBatch, DeviceBiBFS, DeviceGoalBall
from librubiks_amd.solving.evaluation import Evaluator
from tests import ball_model as model
from tests.test_goal_ball_gpu import POPS, REPRS, STARTS, _ball, _in_repr, _model, _model_ball, _start

pytestmark = pytest.mark.gpu

SLOTS = (14, 5, 1)
_across = {}                     # (rep, radius) -> what the first run of that pair gave: every other run must give the same


def _starts20(starts=STARTS) -> np.ndarray:
	return np.stack([_start(d, s) for d, s in starts])


def _assert_state_equals_model(b: DeviceBallSearchBatch, i: int, ok: bool, want, arrays: bool = True):
	assert bool(ok) == want.result
	assert list(b.action_queue_of(i)) == want.queue
	assert b.lengths[i] == (len(want.queue) if want.result else -1)
	assert b.sizes[i] == want.len and b.status[i, 2] == want.len and b.depths[i] == want.depth
	assert b.meeting_depths[i] == (-1 if want.meeting is None else want.meeting_depth)
	assert b.status[i, 0] == 1 and b.status[i, 1] == int(want.result) and b.status[i, 6] == 0
	if arrays:
		states, parents, actions = b.arrays(i)
		assert states.dtype == np.int8 and states.shape[0] == want.len and parents.dtype == np.int64 and actions.dtype == np.int64
		assert (states == _in_repr(want.states)).all()
		assert (parents == want.parents).all() and (actions == want.actions).all()


@pytest.mark.parametrize("rep", REPRS)
@pytest.mark.parametrize("radius", [2, 4])
@pytest.mark.parametrize("pops", POPS)
def test_against_the_model_and_independent_of_slots_and_pops(pops, radius, rep):
	cube.set_is2024(rep == "2024")
	starts = _in_repr(_starts20())
	for searches in SLOTS:
		b = DeviceBallSearchBatch(_ball(radius), searches=searches, pops=pops, poll=256 if pops == 1 else 8)
		solved = b.search(starts.copy(), keep_arrays=True)
		assert solved.dtype == bool and solved.shape == (len(STARTS),) and solved.all()
		assert b.lengths.dtype == np.int64 and b.status.dtype == np.int64 and b.status.shape == (len(STARTS), 10)
		assert not b.capacity_exhausted.any() and (b.stops == 1).all()
		for i, (depth, seed) in enumerate(STARTS):
			_assert_state_equals_model(b, i, solved[i], _model(radius, depth, seed))
		run = (b.lengths.tolist(), b.sizes.tolist(), b.depths.tolist(), b.popped.tolist(), b.meeting_depths.tolist(), b.status[:, 9].tolist())
		assert _across.setdefault((rep, radius), run) == run         # (popped and the meeting node are not the model's to give)
		inside = b.lengths == b.meeting_depths                          # the ball holds the start: answered at the reset
		assert (b.iterations[inside] == 0).all() and (b.popped[inside] == 0).all() and (b.iterations[~inside] >= 1).all()


@pytest.mark.parametrize("radius", [2, 4])
def test_against_the_engine_that_ships(radius):
	b = DeviceBallSearchBatch(_ball(radius), searches=5, pops=7)
	solved = b.search(_starts20())
	agent = DeviceBallSearch(_ball(radius), pops=7)
	for i, (depth, seed) in enumerate(STARTS):
		assert agent.search(_start(depth, seed)) == solved[i]
		assert list(b.action_queue_of(i)) == list(agent.action_queue)
		assert (b.sizes[i], b.depths[i], b.popped[i], b.iterations[i]) == (len(agent), agent.depth, agent.popped, agent.iterations)
		assert b.meeting_depths[i] == agent.meeting_depth and b.status[i, 9] == agent._meet


def test_order_independence_and_duplicates():
	forward = DeviceBallSearchBatch(_ball(2), searches=6, pops=7)
	forward.search(_starts20(), keep_arrays=True)
	dup = STARTS.index((7, 1))
	order = list(range(len(STARTS)))[::-1]
	order = order[:4] + [dup] * 5 + order[4:]                         # five slots hold the same start at once
	b = DeviceBallSearchBatch(_ball(2), searches=6, pops=7)
	solved = b.search(_starts20()[order], keep_arrays=True)
	for j, i in enumerate(order):
		assert solved[j] and list(b.action_queue_of(j)) == list(forward.action_queue_of(i))
		assert (b.status[j] == forward.status[i]).all() and b.lengths[j] == forward.lengths[i]
		for x, y in zip(b.arrays(j), forward.arrays(i)):
			assert (x == y).all()
		_assert_state_equals_model(b, j, solved[j], _model(2, *STARTS[i]))


def test_isolation_on_refill():
	"""A long search in one of two slots while the other is reset at every poll: a reset that cleared a neighbour's table or
	scratch would change the long search's pool."""
	short = [(d, s) for d in (1, 2, 3) for s in (0, 1)] * 20
	starts = [(8, 0)] + short
	b = DeviceBallSearchBatch(_ball(2), searches=2, pops=7, poll=1)
	solved = b.search(_starts20(starts), keep_arrays=True)
	assert solved.all() and b.iterations[0] > len(short)               # it ran while every short one came and went
	for i, (depth, seed) in enumerate(starts):
		_assert_state_equals_model(b, i, solved[i], _model(2, depth, seed))


def test_optimal_against_the_two_sided_search():
	ball = _ball(6)
	moves = [12] + [10 + s % 3 for s in range(15)]
	starts = np.stack([model.scramble(12_001, 12)] + [model.scramble(12_100 + s, moves[1 + s]) for s in range(15)])
	b = DeviceBallSearchBatch(ball, searches=16, capacity=2_000_000)
	solved = b.search(starts)
	assert solved.all() and not b.capacity_exhausted.any()
	two = DeviceBiBFS()
	for i, start in enumerate(starts):
		assert two.search(start.copy())
		queue = list(b.action_queue_of(i))
		assert len(queue) == len(two.action_queue) == b.lengths[i] <= moves[i]
		assert model.orc.is_solved(model.apply(start, queue))
		assert b.lengths[i] <= 6 or (b.meeting_depths[i] == 6 and b.lengths[i] == b.depths[i] + 1 + 6)
	print(f"lengths {b.lengths.tolist()}, states {b.sizes.tolist()}, {b.lockstep_iterations} lock-step iterations")
	assert b.lengths[0] == 12                                          # (tests/test_goal_ball_gpu.py: this start needs 12 moves)


@pytest.mark.parametrize("pops", [7, 4096])
def test_budget_per_state(pops):
	full = _model(2, 7, 0)
	cases = [((7, 0), 150), ((7, 1), None), ((7, 0), 5_000), ((5, 0), None), ((7, 0), 1), ((7, 0), full.len - 12), ((7, 0), full.len),
	         ((6, 1), 2), ((3, 0), 1), ((8, 1), None)]
	starts = _starts20([c[0] for c in cases])
	budgets = np.array([b or 10 ** 10 for _, b in cases], np.int64)
	b = DeviceBallSearchBatch(_ball(2), searches=4, pops=pops)
	solved = b.search(starts, max_states=budgets, keep_arrays=True)
	for i, ((depth, seed), budget) in enumerate(cases):
		want = _model(2, depth, seed, budget)
		_assert_state_equals_model(b, i, solved[i], want)
		assert b.stops[i] == (1 if want.result else 2)
	assert not solved[0] and solved[1] and not solved[4]
	# one budget for all
	solved = b.search(starts, max_states=150, keep_arrays=True)
	for i, ((depth, seed), _) in enumerate(cases):
		_assert_state_equals_model(b, i, solved[i], _model(2, depth, seed, 150))


def test_pool_full():
	capacity, pops = 3_000, 64
	starts = [(5, 0), (8, 0), (3, 1), (5, 1), (2, 0), (3, 0), (1, 1)]
	want = _model(2, 8, 0)
	assert want.len > capacity and all(_model(2, d, s).len + 12 * pops <= capacity for d, s in starts if d != 8)
	b = DeviceBallSearchBatch(_ball(2), searches=3, pops=pops, capacity=capacity)
	solved = b.search(_starts20(starts), keep_arrays=True)
	assert not solved[1] and b.capacity_exhausted.tolist() == [False, True] + [False] * 5
	assert b.stops[1] == 5 and b.status[1, 0] == 1 and b.status[1, 1] == 0 and b.status[1, 6] == 0      # done, not won, no error
	assert b.lengths[1] == -1 and list(b.action_queue_of(1)) == [] and b.meeting_depths[1] == -1
	n = int(b.sizes[1])
	assert capacity - 12 * pops < n <= capacity                       # it stopped because 12 x (at most `pops`) children might not fit
	states, parents, actions = b.arrays(1)
	assert len(states) == n
	assert (states == want.states[:n]).all() and (parents == want.parents[:n]).all() and (actions == want.actions[:n]).all()
	for i, (depth, seed) in enumerate(starts):
		if i != 1:
			_assert_state_equals_model(b, i, solved[i], _model(2, depth, seed))


def test_edges():
	ball = _ball(2)
	b = DeviceBallSearchBatch(ball, searches=3, pops=7)
	solved = b.search(np.zeros((0, 20), np.int8))
	assert solved.shape == (0,) and solved.dtype == bool and b._h is None                      # the device was not touched
	assert b.lengths.shape == (0,) and b.status.shape == (0, 10) and b.meeting_depths.shape == (0,)
	solved = b.search(_start(6, 0)[None], keep_arrays=True)                                     # n = 1
	_assert_state_equals_model(b, 0, solved[0], _model(2, 6, 0))
	with pytest.raises(IndexError):
		b.action_queue_of(1)
	solved = b.search(_start(6, 0)[None])
	with pytest.raises(ValueError):
		b.arrays(0)
	for rep in REPRS:
		cube.set_is2024(rep == "2024")
		solved = b.search(np.stack([cube.get_solved(), _in_repr(_start(5, 0)[None])[0], cube.get_solved()]))
		assert solved.all() and b.lengths.tolist() == [0, len(_model(2, 5, 0).queue), 0]
		assert b.sizes.tolist()[::2] == [1, 1] and b.iterations.tolist()[::2] == [0, 0] and b.meeting_depths.tolist()[::2] == [0, 0]
		assert list(b.action_queue_of(0)) == [] and b.status[0, 9] == 1
	cube.set_is2024(False)
	fresh = DeviceBallSearchBatch(ball, searches=3, pops=7)
	bad = np.stack([cube.get_solved(), np.zeros((6, 8, 6), np.int8), cube.get_solved()])
	with pytest.raises(ValueError):
		fresh.search(bad)
	assert fresh._h is None and fresh.status.shape == (0, 10)                                   # nothing of the call was run


def test_time_limit_bounds_the_whole_call(monkeypatch):
	b = DeviceBallSearchBatch(_ball(2), searches=2, pops=1, poll=1)
	starts = [(8, 0), (8, 1), (7, 0), (2, 0)]
	solved = b.search(_starts20(starts), time_limit=1e-9)             # passed before the first poll: nothing is started
	assert not solved.any() and not b.status.any() and (b.lengths == -1).all() and b.lockstep_iterations == 0
	# a clock that moves one second per look: the call starts two searches, runs two iterations and is out of time at its
	# fourth poll, with two searches running (an 8-move start pops one node per iteration here) and two waiting
	clock = iter(range(1_000))
	monkeypatch.setattr(agents.time, "perf_counter", lambda: float(next(clock)))
	solved = b.search(_starts20(starts), time_limit=3.5, keep_arrays=True)
	monkeypatch.undo()
	assert not solved.any() and (b.stops == 0).all() and (b.lengths == -1).all() and not b.capacity_exhausted.any()
	assert b.lockstep_iterations == 2 and b.iterations.tolist() == [2, 2, 0, 0] and b.popped.tolist() == [2, 2, 0, 0]
	assert (b.sizes[:2] > 1).all() and b.sizes[2:].tolist() == [0, 0] and (b.status[:, 0] == 0).all()
	for i in (0, 1):
		want, (states, parents, actions) = _model(2, *starts[i]), b.arrays(i)
		n = int(b.sizes[i])
		assert len(states) == n and (states == want.states[:n]).all() and (parents == want.parents[:n]).all()
	assert [len(x) for x in b.arrays(2)] == [0, 0, 0]
	solved = b.search(_starts20(starts))                               # and the engine is as good as new
	for i, (depth, seed) in enumerate(starts):
		_assert_state_equals_model(b, i, solved[i], _model(2, depth, seed), arrays=False)


def test_c_entries_refuse_bad_arguments():
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	ball, h = C.c_void_p(), C.c_void_p()
	_ffi.check(lib.rk_ball_create(C.byref(ball), 2, 8))
	_ffi.check(lib.rk_bsearchb_create(C.byref(h), ball, 3, 5_000, 8))
	try:
		starts = np.ascontiguousarray(_starts20([(5, 0), (6, 0), (2, 0)]))
		budgets = np.full(3, 10 ** 10, np.int64)
		buf = np.zeros(20, np.int8)
		st = np.zeros((3, 10), np.int64)
		paths = np.zeros((3, 17), np.int32)

		def reset(slots):
			sl = np.array(slots, np.int32)
			return lib.rk_bsearchb_reset(h, len(sl), sl.ctypes.data, starts.ctypes.data, budgets.ctypes.data, stream)
		# the ball is not built
		assert reset([0, 1, 2]) == -4 and lib.rk_bsearchb_run(h, 1, stream) == -4                     # RK_ESTATE
		assert lib.rk_bsearchb_paths(h, paths.ctypes.data, 16, stream) == -4
		_ffi.check(lib.rk_ball_build(ball, 8, stream))
		# a ball with a batch attached refuses to go
		assert lib.rk_ball_destroy(ball) == -4 and b"search" in lib.rk_last_error()
		# slots
		assert reset([0, 3]) == -1 and reset([-1]) == -1                                              # RK_EINVAL: out of range
		assert reset([1, 1]) == -1 and b"twice" in lib.rk_last_error()                               # duplicates
		assert reset([0, 1, 2, 0]) == -1                                                              # more slots than there are
		assert lib.rk_bsearchb_reset(h, 1, None, starts.ctypes.data, budgets.ctypes.data, stream) == -1
		assert lib.rk_bsearchb_export(h, 3, 1, 1, buf.ctypes.data, None, None, stream) == -1
		assert lib.rk_bsearchb_export(h, -1, 1, 1, buf.ctypes.data, None, None, stream) == -1
		assert lib.rk_bsearchb_export(h, 0, 1, 5_001, buf.ctypes.data, None, None, stream) == -1     # rows outside the pool
		assert lib.rk_bsearchb_run(h, -1, stream) == -1
		assert lib.rk_bsearchb_paths(h, paths.ctypes.data, 4097, stream) == -1 and lib.rk_bsearchb_paths(h, None, 16, stream) == -1
		# nothing was started by the refused calls: every slot passes an iteration by
		_ffi.check(lib.rk_bsearchb_run(h, 2, stream))
		_ffi.check(lib.rk_bsearchb_status(h, st.ctypes.data, stream))
		assert not st.any()
		_ffi.check(lib.rk_bsearchb_paths(h, paths.ctypes.data, 16, stream))
		assert paths[:, 0].tolist() == [-1, -1, -1]
		# the batch through the C ABI alone: slots 2 and 0 run states 0 and 1, slot 1 is never started
		_ffi.check(reset([2, 0]))
		_ffi.check(lib.rk_bsearchb_run(h, 64, stream))
		_ffi.check(lib.rk_bsearchb_status(h, st.ctypes.data, stream))
		_ffi.check(lib.rk_bsearchb_paths(h, paths.ctypes.data, 16, stream))
		for slot, (depth, seed) in ((2, (5, 0)), (0, (6, 0))):
			want = model.search(_start(depth, seed), _model_ball(2))
			assert st[slot, :3].tolist() == [1, 1, want.len] and st[slot, 8] == want.depth
			assert paths[slot, 0] == len(want.queue) and paths[slot, 1:1 + paths[slot, 0]].tolist() == want.queue
			_ffi.check(lib.rk_bsearchb_export(h, slot, 1, 1, buf.ctypes.data, None, None, stream))
			assert (buf == _start(depth, seed)).all()
		assert not st[1].any() and paths[1, 0] == -1
	finally:
		assert lib.rk_bsearchb_destroy(h) == 0
		assert lib.rk_ball_destroy(ball) == 0


def test_evaluator_batched_equals_sequential():
	ball = _ball(4)
	agent = DeviceBallSearch(ball, pops=64)
	ev = Evaluator(8, [3, 6], max_states=100)
	np.random.seed(7)
	res_b, states_b, _ = ev.eval(agent)
	assert ev.last_mode == "batched"
	np.random.seed(7)
	res_s, states_s, _ = ev.eval(agent, batched=False)
	assert ev.last_mode == "sequential"
	assert res_b.shape == (2, 8) and (res_b == res_s).all() and (states_b == states_s).all()
	assert (res_b[0] >= 0).all() and (res_b[0] <= 3).all() and (res_b <= 6).all()
