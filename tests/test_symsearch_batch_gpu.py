"""
DeviceSymBallSearchBatch (engine rk_ssearchb_*) on the GPU: every state of a batch gets what the plain-Python model
(tests/symsearch_model.py), the single engine `DeviceSymBallSearch` and -- but for the ball's half of the queue -- a slot of
`DeviceBallSearchBatch` on a plain ball of the same radius give it alone, bit for bit.
  * the 24 starts of tests/test_symsearch_cpu.py (radius 3: inside the ball and own depths 0..4, a meeting in the first child of
    the first pop, two meeting children in one batch) in one call, with 25, 5 and 1 slots (5: slots are refilled mid-run; 1: the
    single engine by another road), pops 1 / 5 / 16 / 16 384, both representations: result, queue, lengths, sizes, depths, popped,
    meeting depths and pools against the model, and the runs equal to each other, the meeting nodes included;
  * the same starts one by one through DeviceSymBallSearch, and through DeviceBallSearchBatch on DeviceGoalBall(3);
  * symmetric states as starts, the superflip under a budget; optimality at radius 6 with DeviceBiBFS's lengths; the C entries.
One start five times over in six slots in another order, a long search beside a slot refilled at every poll, per-state budgets, a
pool that is full, the time limit, the edges and the Evaluator are what this batch shares with the plain ball's:
tests/test_ball_readers_batch_gpu.py.
The models and the device balls are those of tests/test_symsearch_cpu.py and tests/test_symsearch_gpu.py, made once per session.
"""
import ctypes as C

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceBallSearchBatch, DeviceBiBFS, DeviceSymBallSearch, DeviceSymBallSearchBatch
from tests import ball_model
from tests import sym_model
from tests import symsearch_model as model
from tests.ball_kinds import CAPACITY, SYM, assert_state_equals_model
from tests.test_symsearch_cpu import RADIUS, modelled, starts, sym_ball
from tests.test_symsearch_gpu import POPS, _deep_starts, _in_repr, _pball, _sball, _symmetric

pytestmark = pytest.mark.gpu

orc = ball_model.orc
SLOTS = (25, 5, 1)
_across = []                     # what the first run gave: every other run -- any slots, pops, representation -- must give the same


@pytest.mark.parametrize("rep", ["2024", "686"])
@pytest.mark.parametrize("pops", POPS)
def test_against_the_model_and_independent_of_slots_and_pops(pops, rep):
	cube.set_is2024(rep == "2024")
	ball = _sball(RADIUS)
	given = _in_repr(SYM.states(SYM.keys))
	for searches in SLOTS:
		b = DeviceSymBallSearchBatch(ball, searches=searches, pops=pops, capacity=CAPACITY, poll=256 if pops == 1 else 8)
		solved = b.search(given.copy(), keep_arrays=True)
		assert solved.dtype == bool and solved.shape == (24,) and solved.all()
		assert b.lengths.dtype == np.int64 and b.status.dtype == np.int64 and b.status.shape == (24, 10)
		assert not b.capacity_exhausted.any() and (b.stops == 1).all()
		for i, (seed, moves, _) in enumerate(starts()):
			want, popped = modelled(seed, moves)
			assert_state_equals_model(b, i, solved[i], want, popped)
		assert (b.meeting_nodes == b.status[:, 9]).all()
		assert (ball.level_start[b.meeting_depths] <= b.meeting_nodes).all() and (b.meeting_nodes < ball.level_start[b.meeting_depths + 1]).all()
		run = (b.lengths.tolist(), b.sizes.tolist(), b.depths.tolist(), b.popped.tolist(), b.meeting_depths.tolist(), b.status[:, 9].tolist())
		_across.append(run)
		assert _across[0] == run
		inside = b.popped == 0                                         # the ball holds the start's orbit: answered at the reset
		assert inside.sum() == 9 and (b.lengths[inside] == b.meeting_depths[inside]).all() and (b.sizes[inside] == 1).all()
		assert (b.iterations[inside] == 0).all() and (b.iterations[~inside] >= -(-b.popped[~inside] // pops)).all()
		assert (b.meeting_depths[~inside] == RADIUS).all() and (b.lengths[~inside] == b.depths[~inside] + 1 + RADIUS).all()


def test_against_the_engines_that_ship():
	b = DeviceSymBallSearchBatch(_sball(RADIUS), searches=5, pops=5, capacity=CAPACITY)
	solved = b.search(SYM.states(SYM.keys), keep_arrays=True)
	agent = DeviceSymBallSearch(_sball(RADIUS), pops=5)
	for i, (_, _, start) in enumerate(starts()):
		assert agent.search(start.copy()) == solved[i]
		assert list(b.action_queue_of(i)) == list(agent.action_queue) and b.lengths[i] == len(agent.action_queue)
		assert (b.sizes[i], b.depths[i], b.popped[i], b.iterations[i]) == (len(agent), agent.depth, agent.popped, agent.iterations)
		assert b.meeting_depths[i] == agent.meeting_depth and b.meeting_nodes[i] == agent._meet
	# a slot of the plain batch on a plain ball of the same radius: everything but the meeting node and the ball's half of the queue
	plain = DeviceBallSearchBatch(_pball(RADIUS), searches=5, pops=5, capacity=CAPACITY)
	solved_plain = plain.search(SYM.states(SYM.keys), keep_arrays=True)
	assert (solved == solved_plain).all() and (b.status[:, :9] == plain.status[:, :9]).all()
	assert (b.lengths == plain.lengths).all() and (b.meeting_depths == plain.meeting_depths).all()
	for i, (_, _, start) in enumerate(starts()):
		for x, y in zip(b.arrays(i), plain.arrays(i)):
			assert x.shape == y.shape and (x == y).all()
		mine, theirs = list(b.action_queue_of(i)), list(plain.action_queue_of(i))
		own = len(mine) - int(b.meeting_depths[i])
		assert len(mine) == len(theirs) and mine[:own] == theirs[:own]
		assert orc.is_solved(ball_model.apply(start, mine)) and orc.is_solved(ball_model.apply(start, theirs))


def test_symmetric_states_and_the_superflip():
	names, states, orbits = zip(*_symmetric())
	# near solved, at radius 2: solved and U D / U D' lie inside, (U D)2 at own depth 1
	want_ball = sym_model.build(2)
	b = DeviceSymBallSearchBatch(_sball(2), searches=3, pops=5, capacity=CAPACITY)
	solved = b.search(np.stack(states[:4]), keep_arrays=True)
	for i in range(4):
		want, popped = model.search(states[i], want_ball)
		assert want.result, names[i]
		assert_state_equals_model(b, i, solved[i], want, popped)
	assert b.popped.tolist()[:3] == [0, 0, 0] and b.popped[3] > 0 and b.meeting_nodes[0] == 1
	# the superflip and its neighbours are 20 and more moves from solved: a budget ends the search; the pool is the plain batch's
	b = DeviceSymBallSearchBatch(_sball(RADIUS), searches=3, pops=16, capacity=CAPACITY)
	plain = DeviceBallSearchBatch(_pball(RADIUS), searches=3, pops=16, capacity=CAPACITY)
	far = np.stack(states[4:])
	solved, solved_plain = b.search(far, max_states=3_000, keep_arrays=True), plain.search(far, max_states=3_000, keep_arrays=True)
	assert len(far) == 3 and not solved.any() and not solved_plain.any()
	assert (b.stops == 2).all() and (b.lengths == -1).all() and (b.meeting_nodes == 0).all() and (b.meeting_depths == -1).all()
	assert ((3_000 <= b.sizes) & (b.sizes < 3_012)).all() and (b.status == plain.status).all()
	for i in range(3):
		assert list(b.action_queue_of(i)) == []
		for x, y in zip(b.arrays(i), plain.arrays(i)):
			assert x.shape == y.shape and (x == y).all()


def test_optimal_against_the_two_sided_search():
	given = np.stack(_deep_starts())                                  # the 7..11-move prefixes of the radius-6 scramble (seed 604)
	b = DeviceSymBallSearchBatch(_sball(6), searches=5, capacity=400_000)
	solved = b.search(given)
	assert solved.all() and not b.capacity_exhausted.any() and b.lengths.tolist() == [7, 8, 9, 10, 11]
	two = DeviceBiBFS()
	for i, start in enumerate(given):
		assert two.search(start.copy())
		queue = list(b.action_queue_of(i))
		assert len(queue) == len(two.action_queue) == b.lengths[i]
		assert orc.is_solved(ball_model.apply(start, queue))
		assert b.meeting_depths[i] == 6 and b.lengths[i] == b.depths[i] + 1 + 6
	print(f"lengths {b.lengths.tolist()}, states {b.sizes.tolist()}, {b.lockstep_iterations} lock-step iterations")


def test_c_entries_refuse_bad_arguments():
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	ball, h = C.c_void_p(), C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(ball), RADIUS, 8, 0))
	# the ball is not built: nothing is made, nothing attached
	assert lib.rk_ssearchb_create(C.byref(h), ball, 3, 5_000, 8) == -4 and h.value is None          # RK_ESTATE
	_ffi.check(lib.rk_symball_build(ball, 8, stream))
	_ffi.check(lib.rk_ssearchb_create(C.byref(h), ball, 3, 5_000, 8))
	try:
		picked = [starts()[4], starts()[5], starts()[1]]             # own depths 1 and 2, and inside the ball
		given = np.ascontiguousarray(SYM.states([4, 5, 1]))
		budgets = np.full(3, 10 ** 10, np.int64)
		buf = np.zeros(20, np.int8)
		st = np.zeros((3, 10), np.int64)
		paths = np.zeros((3, 17), np.int32)

		def reset(slots):
			sl = np.array(slots, np.int32)
			return lib.rk_ssearchb_reset(h, len(sl), sl.ctypes.data, given.ctypes.data, budgets.ctypes.data, stream)
		# a ball with a batch attached refuses to go
		assert lib.rk_symball_destroy(ball) == -4 and b"search" in lib.rk_last_error()
		# slots
		assert reset([0, 3]) == -1 and reset([-1]) == -1                                              # RK_EINVAL: out of range
		assert reset([1, 1]) == -1 and b"twice" in lib.rk_last_error()                               # duplicates
		assert reset([0, 1, 2, 0]) == -1                                                              # more slots than there are
		assert lib.rk_ssearchb_reset(h, 1, None, given.ctypes.data, budgets.ctypes.data, stream) == -1
		assert lib.rk_ssearchb_reset(h, 1, np.zeros(1, np.int32).ctypes.data, None, budgets.ctypes.data, stream) == -1
		assert lib.rk_ssearchb_reset(h, 1, np.zeros(1, np.int32).ctypes.data, given.ctypes.data, None, stream) == -1
		assert lib.rk_ssearchb_export(h, 3, 1, 1, buf.ctypes.data, None, None, stream) == -1
		assert lib.rk_ssearchb_export(h, -1, 1, 1, buf.ctypes.data, None, None, stream) == -1
		assert lib.rk_ssearchb_export(h, 0, 1, 5_001, buf.ctypes.data, None, None, stream) == -1     # rows outside the pool
		assert lib.rk_ssearchb_run(h, -1, stream) == -1
		assert lib.rk_ssearchb_paths(h, paths.ctypes.data, 4097, stream) == -1 and lib.rk_ssearchb_paths(h, None, 16, stream) == -1
		assert lib.rk_ssearchb_status(h, None, stream) == -1
		# nothing was started by the refused calls: every slot passes an iteration by
		_ffi.check(lib.rk_ssearchb_run(h, 2, stream))
		_ffi.check(lib.rk_ssearchb_status(h, st.ctypes.data, stream))
		assert not st.any()
		_ffi.check(lib.rk_ssearchb_paths(h, paths.ctypes.data, 16, stream))
		assert paths[:, 0].tolist() == [-1, -1, -1]
		# the batch through the C ABI alone: slots 2 and 0 run states 0 and 1, slot 1 is never started
		_ffi.check(reset([2, 0]))
		_ffi.check(lib.rk_ssearchb_run(h, 64, stream))
		_ffi.check(lib.rk_ssearchb_status(h, st.ctypes.data, stream))
		_ffi.check(lib.rk_ssearchb_paths(h, paths.ctypes.data, 16, stream))
		for slot, (seed, moves, start) in ((2, picked[0]), (0, picked[1])):
			want, popped = modelled(seed, moves)
			assert st[slot, :3].tolist() == [1, 1, want.len] and st[slot, 4] == popped and st[slot, 8] == want.depth
			assert sym_ball().level_start[RADIUS] <= st[slot, 9] < sym_ball().level_start[RADIUS + 1]
			assert paths[slot, 0] == len(want.queue) and paths[slot, 1:1 + paths[slot, 0]].tolist() == want.queue
			_ffi.check(lib.rk_ssearchb_export(h, slot, 1, 1, buf.ctypes.data, None, None, stream))
			assert (buf == start).all()
		assert not st[1].any() and paths[1, 0] == -1
		# then slot 1 alone: a start whose orbit the ball holds is done at the reset, the others stay where they were
		before = st.copy()
		sl = np.array([1], np.int32)
		_ffi.check(lib.rk_ssearchb_reset(h, 1, sl.ctypes.data, given[2:].ctypes.data, budgets.ctypes.data, stream))
		_ffi.check(lib.rk_ssearchb_status(h, st.ctypes.data, stream))
		want, _ = modelled(*picked[2][:2])
		assert st[1, :5].tolist() == [1, 1, 1, 0, 0] and st[1, 5] == 1 and (st[[0, 2]] == before[[0, 2]]).all()
		_ffi.check(lib.rk_ssearchb_paths(h, paths.ctypes.data, 16, stream))
		assert paths[1, 0] == len(want.queue) and paths[1, 1:1 + paths[1, 0]].tolist() == want.queue
	finally:
		assert lib.rk_ssearchb_destroy(h) == 0
		assert lib.rk_symball_destroy(ball) == 0
