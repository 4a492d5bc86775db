"""
DeviceBallSearchBatch (engine rk_bsearchb_*) on the GPU: every state of a batch gets what the plain-Python model
(tests/ball_model.py) and the single engine `DeviceBallSearch` give it alone, bit for bit.
  * the starts of tests/test_goal_ball_gpu.py (seeded scrambles of 1, 2, 3, 5, 6, 7 and 8 moves, two seeds each) against balls of
    radius 2 and 4 in one call, with 14, 5 and 1 slots (5: slots are refilled mid-run; 1: the single engine by another road),
    pops 1 / 7 / 4096, both representations: result, queue, len, depth, meeting depth and pool against the model, and the runs
    equal to each other;
  * the same starts one by one through DeviceBallSearch;
  * optimality on 10- to 12-move starts against a radius-6 ball with DeviceBiBFS's lengths;
  * the C entries.
Reversed input with duplicates, isolation on refill, per-state budgets, a pool that is full, the edges, the time limit and the
Evaluator are what this batch shares with the symmetry ball's: tests/test_ball_readers_batch_gpu.py.
The models and the device balls are those of tests/test_goal_ball_gpu.py, computed once per session.
"""
import ctypes as C

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceBallSearch, DeviceBallSearchBatch, DeviceBiBFS
from tests import ball_model as model
from tests.ball_kinds import PLAIN, assert_state_equals_model
from tests.test_goal_ball_gpu import POPS, REPRS, STARTS, _ball, _in_repr, _model, _model_ball, _start

pytestmark = pytest.mark.gpu

SLOTS = (14, 5, 1)
_across = {}                     # (rep, radius) -> what the first run of that pair gave: every other run must give the same


@pytest.mark.parametrize("rep", REPRS)
@pytest.mark.parametrize("radius", [2, 4])
@pytest.mark.parametrize("pops", POPS)
def test_against_the_model_and_independent_of_slots_and_pops(pops, radius, rep):
	cube.set_is2024(rep == "2024")
	starts = _in_repr(PLAIN.states(STARTS))
	for searches in SLOTS:
		b = DeviceBallSearchBatch(_ball(radius), searches=searches, pops=pops, poll=256 if pops == 1 else 8)
		solved = b.search(starts.copy(), keep_arrays=True)
		assert solved.dtype == bool and solved.shape == (len(STARTS),) and solved.all()
		assert b.lengths.dtype == np.int64 and b.status.dtype == np.int64 and b.status.shape == (len(STARTS), 10)
		assert not b.capacity_exhausted.any() and (b.stops == 1).all()
		for i, (depth, seed) in enumerate(STARTS):
			assert_state_equals_model(b, i, solved[i], _model(radius, depth, seed))
		run = (b.lengths.tolist(), b.sizes.tolist(), b.depths.tolist(), b.popped.tolist(), b.meeting_depths.tolist(), b.status[:, 9].tolist())
		assert _across.setdefault((rep, radius), run) == run         # (popped and the meeting node are not the model's to give)
		inside = b.lengths == b.meeting_depths                          # the ball holds the start: answered at the reset
		assert (b.iterations[inside] == 0).all() and (b.popped[inside] == 0).all() and (b.iterations[~inside] >= 1).all()


@pytest.mark.parametrize("radius", [2, 4])
def test_against_the_engine_that_ships(radius):
	b = DeviceBallSearchBatch(_ball(radius), searches=5, pops=7)
	solved = b.search(PLAIN.states(STARTS))
	agent = DeviceBallSearch(_ball(radius), pops=7)
	for i, (depth, seed) in enumerate(STARTS):
		assert agent.search(_start(depth, seed)) == solved[i]
		assert list(b.action_queue_of(i)) == list(agent.action_queue)
		assert (b.sizes[i], b.depths[i], b.popped[i], b.iterations[i]) == (len(agent), agent.depth, agent.popped, agent.iterations)
		assert b.meeting_depths[i] == agent.meeting_depth and b.status[i, 9] == agent._meet


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


def test_c_entries_refuse_bad_arguments():
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	ball, h = C.c_void_p(), C.c_void_p()
	_ffi.check(lib.rk_ball_create(C.byref(ball), 2, 8))
	_ffi.check(lib.rk_bsearchb_create(C.byref(h), ball, 3, 5_000, 8))
	try:
		starts = np.ascontiguousarray(PLAIN.states([(5, 0), (6, 0), (2, 0)]))
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
