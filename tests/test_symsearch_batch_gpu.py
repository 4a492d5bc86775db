"""
DeviceSymBallSearchBatch (engine rk_ssearchb_*) on the GPU: every state of a batch gets what the plain-Python model
(tests/symsearch_model.py), the single engine `DeviceSymBallSearch` and -- but for the ball's half of the queue -- a slot of
`DeviceBallSearchBatch` on a plain ball of the same radius give it alone, bit for bit.
  * the 24 starts of tests/test_symsearch_cpu.py (radius 3: inside the ball and own depths 0..4, a meeting in the first child of
    the first pop, two meeting children in one batch) in one call, with 25, 5 and 1 slots (5: slots are refilled mid-run; 1: the
    single engine by another road), pops 1 / 5 / 16 / 16 384, both representations: result, queue, lengths, sizes, depths, popped,
    meeting depths and pools against the model, and the runs equal to each other, the meeting nodes included;
  * the same starts one by one through DeviceSymBallSearch, and through DeviceBallSearchBatch on DeviceGoalBall(3);
  * one start five times over in six slots, in another order; a long search beside a slot refilled at every poll;
  * symmetric states as starts, the superflip under a budget; per-state budgets; a pool that is full; optimality at radius 6
    with DeviceBiBFS's lengths; the time limit; the edges; the C entries; the Evaluator.
The models and the device balls are those of tests/test_symsearch_cpu.py and tests/test_symsearch_gpu.py, made once per session.
"""
import ctypes as C

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import DeviceBallSearchBatch, DeviceBiBFS, DeviceSymBallSearch, DeviceSymBallSearchBatch
from librubiks_amd.solving.evaluation import Evaluator
from tests import ball_model
from tests import sym_model
from tests import symsearch_model as model
from tests.test_symsearch_cpu import RADIUS, modelled, starts, sym_ball
from tests.test_symsearch_gpu import POPS, _deep_starts, _in_repr, _pball, _sball, _symmetric

pytestmark = pytest.mark.gpu

orc = ball_model.orc
SLOTS = (25, 5, 1)
CAPACITY = 300_000               # per slot: the largest pool of starts() (33 055 states) and the widest iteration behind it fit
_across = []                     # what the first run gave: every other run -- any slots, pops, representation -- must give the same


def _starts20(picked=None) -> np.ndarray:
	return np.stack([s for _, _, s in (starts() if picked is None else picked)])


def _assert_state_equals_model(b, i: int, ok: bool, want, popped=None, arrays: bool = True):
	assert bool(ok) == want.result
	assert list(b.action_queue_of(i)) == want.queue
	assert b.lengths[i] == (len(want.queue) if want.result else -1)
	assert b.sizes[i] == want.len and b.status[i, 2] == want.len and b.depths[i] == want.depth
	assert b.meeting_depths[i] == (-1 if want.meeting is None else want.meeting_depth)
	assert (b.meeting_nodes[i] == 0) == (want.meeting is None)
	assert b.status[i, 0] == 1 and b.status[i, 1] == int(want.result) and b.status[i, 6] == 0
	if popped is not None:
		assert b.popped[i] == popped
	if arrays:
		states, parents, actions = b.arrays(i)
		assert states.dtype == np.int8 and states.shape[0] == want.len and parents.dtype == np.int64 and actions.dtype == np.int64
		assert (states == _in_repr(want.states)).all()
		assert (parents == want.parents).all() and (actions == want.actions).all()


@pytest.mark.parametrize("rep", ["2024", "686"])
@pytest.mark.parametrize("pops", POPS)
def test_against_the_model_and_independent_of_slots_and_pops(pops, rep):
	cube.set_is2024(rep == "2024")
	ball = _sball(RADIUS)
	given = _in_repr(_starts20())
	for searches in SLOTS:
		b = DeviceSymBallSearchBatch(ball, searches=searches, pops=pops, capacity=CAPACITY, poll=256 if pops == 1 else 8)
		solved = b.search(given.copy(), keep_arrays=True)
		assert solved.dtype == bool and solved.shape == (24,) and solved.all()
		assert b.lengths.dtype == np.int64 and b.status.dtype == np.int64 and b.status.shape == (24, 10)
		assert not b.capacity_exhausted.any() and (b.stops == 1).all()
		for i, (seed, moves, _) in enumerate(starts()):
			want, popped = modelled(seed, moves)
			_assert_state_equals_model(b, i, solved[i], want, popped)
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
	solved = b.search(_starts20(), keep_arrays=True)
	agent = DeviceSymBallSearch(_sball(RADIUS), pops=5)
	for i, (_, _, start) in enumerate(starts()):
		assert agent.search(start.copy()) == solved[i]
		assert list(b.action_queue_of(i)) == list(agent.action_queue) and b.lengths[i] == len(agent.action_queue)
		assert (b.sizes[i], b.depths[i], b.popped[i], b.iterations[i]) == (len(agent), agent.depth, agent.popped, agent.iterations)
		assert b.meeting_depths[i] == agent.meeting_depth and b.meeting_nodes[i] == agent._meet
	# a slot of the plain batch on a plain ball of the same radius: everything but the meeting node and the ball's half of the queue
	plain = DeviceBallSearchBatch(_pball(RADIUS), searches=5, pops=5, capacity=CAPACITY)
	solved_plain = plain.search(_starts20(), keep_arrays=True)
	assert (solved == solved_plain).all() and (b.status[:, :9] == plain.status[:, :9]).all()
	assert (b.lengths == plain.lengths).all() and (b.meeting_depths == plain.meeting_depths).all()
	for i, (_, _, start) in enumerate(starts()):
		for x, y in zip(b.arrays(i), plain.arrays(i)):
			assert x.shape == y.shape and (x == y).all()
		mine, theirs = list(b.action_queue_of(i)), list(plain.action_queue_of(i))
		own = len(mine) - int(b.meeting_depths[i])
		assert len(mine) == len(theirs) and mine[:own] == theirs[:own]
		assert orc.is_solved(ball_model.apply(start, mine)) and orc.is_solved(ball_model.apply(start, theirs))


def test_order_independence_and_duplicates():
	forward = DeviceSymBallSearchBatch(_sball(RADIUS), searches=6, pops=5, capacity=CAPACITY)
	forward.search(_starts20(), keep_arrays=True)
	dup = 6                                                            # own depth 3
	order = list(range(24))[::-1]
	order = order[:4] + [dup] * 5 + order[4:]                          # five slots hold the same start at once
	b = DeviceSymBallSearchBatch(_sball(RADIUS), searches=6, pops=5, capacity=CAPACITY)
	solved = b.search(_starts20()[order], keep_arrays=True)
	for j, i in enumerate(order):
		assert solved[j] and list(b.action_queue_of(j)) == list(forward.action_queue_of(i))
		assert (b.status[j] == forward.status[i]).all() and b.lengths[j] == forward.lengths[i]
		for x, y in zip(b.arrays(j), forward.arrays(i)):
			assert (x == y).all()
		seed, moves, _ = starts()[i]
		_assert_state_equals_model(b, j, solved[j], *modelled(seed, moves))


def test_isolation_on_refill():
	"""A depth-4 search in one of two slots while sixty short ones come and go in the other, which is reset at every poll: a reset
	that cleared a neighbour's table, scratch or `hit` words would change the long search's pool."""
	short = [s for s in starts() if s[1] <= 4] * 5
	picked = [starts()[7]] + short
	assert len(short) == 60 and modelled(*starts()[7][:2])[0].depth == 4
	b = DeviceSymBallSearchBatch(_sball(RADIUS), searches=2, pops=5, capacity=CAPACITY, poll=1)
	solved = b.search(_starts20(picked), keep_arrays=True)
	assert solved.all() and b.iterations[0] > len(short)              # it ran while every short one came and went
	for i, (seed, moves, _) in enumerate(picked):
		_assert_state_equals_model(b, i, solved[i], *modelled(seed, moves))


def test_symmetric_states_and_the_superflip():
	names, states, orbits = zip(*_symmetric())
	# near solved, at radius 2: solved and U D / U D' lie inside, (U D)2 at own depth 1
	want_ball = sym_model.build(2)
	b = DeviceSymBallSearchBatch(_sball(2), searches=3, pops=5, capacity=CAPACITY)
	solved = b.search(np.stack(states[:4]), keep_arrays=True)
	for i in range(4):
		want, popped = model.search(states[i], want_ball)
		assert want.result, names[i]
		_assert_state_equals_model(b, i, solved[i], want, popped)
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


@pytest.mark.parametrize("pops", [5, 16_384])
def test_budget_per_state(pops):
	seed, moves, start = starts()[6]                                 # own depth 3
	full, _ = modelled(seed, moves)
	assert full.result and full.len > 5_012
	cases = [(6, 150), (5, None), (6, 5_000), (3, None), (6, 1), (6, full.len - 12), (6, full.len), (12, 2), (2, 1), (14, None)]
	picked = [starts()[i] for i, _ in cases]
	budgets = np.array([x or 10 ** 10 for _, x in cases], np.int64)
	b = DeviceSymBallSearchBatch(_sball(RADIUS), searches=4, pops=pops, capacity=CAPACITY)
	solved = b.search(_starts20(picked), max_states=budgets, keep_arrays=True)
	for i, (k, budget) in enumerate(cases):
		want, _ = model.search(starts()[k][2], sym_ball(), max_states=budget)
		_assert_state_equals_model(b, i, solved[i], want)
		assert b.stops[i] == (1 if want.result else 2)
	assert not solved[0] and solved[1] and not solved[4] and not solved[5] and solved[6]
	# one budget for all
	solved = b.search(_starts20(picked), max_states=150, keep_arrays=True)
	for i, (k, _) in enumerate(cases):
		want, _ = model.search(starts()[k][2], sym_ball(), max_states=150)
		_assert_state_equals_model(b, i, solved[i], want)
		assert b.stops[i] == (1 if want.result else 2)
	assert not solved[0] and (b.stops == 2).any() and (b.stops == 1).any()


def test_pool_full():
	capacity, pops = 3_000, 64
	picked = [starts()[i] for i in (4, 6, 2, 12, 1, 9, 16)]
	want, _ = modelled(*picked[1][:2])
	assert want.len > capacity and all(modelled(sd, n)[0].len + 12 * pops <= capacity for sd, n, _ in picked[:1] + picked[2:])
	b = DeviceSymBallSearchBatch(_sball(RADIUS), searches=3, pops=pops, capacity=capacity)
	solved = b.search(_starts20(picked), keep_arrays=True)
	assert not solved[1] and b.capacity_exhausted.tolist() == [False, True] + [False] * 5
	assert b.stops[1] == 5 and b.status[1, 0] == 1 and b.status[1, 1] == 0 and b.status[1, 6] == 0      # done, not won, no error
	assert b.lengths[1] == -1 and list(b.action_queue_of(1)) == [] and b.meeting_depths[1] == -1 and b.meeting_nodes[1] == 0
	n = int(b.sizes[1])
	assert capacity - 12 * pops < n <= capacity                       # it stopped because 12 x (at most `pops`) children might not fit
	states, parents, actions = b.arrays(1)
	assert len(states) == n
	assert (states == want.states[:n]).all() and (parents == want.parents[:n]).all() and (actions == want.actions[:n]).all()
	for i, (seed, moves, _) in enumerate(picked):
		if i != 1:
			_assert_state_equals_model(b, i, solved[i], *modelled(seed, moves))


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


def test_edges():
	ball = _sball(2)
	b = DeviceSymBallSearchBatch(ball, searches=3, pops=7, capacity=CAPACITY)
	solved = b.search(np.zeros((0, 20), np.int8))
	assert solved.shape == (0,) and solved.dtype == bool and b._h is None                      # the device was not touched
	seed, moves, start = starts()[5]
	want, popped = model.search(start, sym_model.build(2))
	solved = b.search(start[None], keep_arrays=True)                                            # n = 1
	_assert_state_equals_model(b, 0, solved[0], want, popped)
	with pytest.raises(IndexError):
		b.action_queue_of(1)
	solved = b.search(start[None])
	with pytest.raises(ValueError):
		b.arrays(0)
	for is2024 in (True, False):
		cube.set_is2024(is2024)
		solved = b.search(np.stack([cube.get_solved(), _in_repr(start[None])[0], cube.get_solved()]))
		assert solved.all() and b.lengths.tolist() == [0, len(want.queue), 0]
		assert b.sizes.tolist()[::2] == [1, 1] and b.iterations.tolist()[::2] == [0, 0] and b.meeting_depths.tolist()[::2] == [0, 0]
		assert list(b.action_queue_of(0)) == [] and b.meeting_nodes[0] == 1
	cube.set_is2024(False)
	fresh = DeviceSymBallSearchBatch(ball, searches=3, pops=7)
	bad = np.stack([cube.get_solved(), np.zeros((6, 8, 6), np.int8), cube.get_solved()])
	with pytest.raises(ValueError):
		fresh.search(bad)                                                                        # an illegal 6x8x6 state: before anything runs
	assert fresh._h is None and fresh.status.shape == (0, 10)


def test_time_limit_bounds_the_whole_call(monkeypatch):
	b = DeviceSymBallSearchBatch(_sball(RADIUS), searches=2, pops=1, capacity=CAPACITY, poll=1)
	picked = [starts()[7], starts()[15], starts()[6], starts()[1]]
	solved = b.search(_starts20(picked), time_limit=1e-9)             # passed before the first poll: nothing is started
	assert not solved.any() and not b.status.any() and (b.lengths == -1).all() and b.lockstep_iterations == 0
	# a clock that moves one second per look: the call starts two searches, runs two iterations and is out of time at its
	# fourth poll, with two searches running (an 8-move start pops one node per iteration here) and two waiting
	clock = iter(range(1_000))
	monkeypatch.setattr(agents.time, "perf_counter", lambda: float(next(clock)))
	solved = b.search(_starts20(picked), time_limit=3.5, keep_arrays=True)
	monkeypatch.undo()
	assert not solved.any() and (b.stops == 0).all() and (b.lengths == -1).all() and not b.capacity_exhausted.any()
	assert b.lockstep_iterations == 2 and b.iterations.tolist() == [2, 2, 0, 0] and b.popped.tolist() == [2, 2, 0, 0]
	assert (b.sizes[:2] > 1).all() and b.sizes[2:].tolist() == [0, 0] and (b.status[:, 0] == 0).all()
	for i in (0, 1):
		want, (states, parents, actions) = modelled(*picked[i][:2])[0], b.arrays(i)
		n = int(b.sizes[i])
		assert len(states) == n and (states == want.states[:n]).all() and (parents == want.parents[:n]).all()
	assert [len(x) for x in b.arrays(2)] == [0, 0, 0]
	solved = b.search(_starts20(picked[2:]))                          # and the engine is as good as new
	for i, (seed, moves, _) in enumerate(picked[2:]):
		_assert_state_equals_model(b, i, solved[i], *modelled(seed, moves), arrays=False)


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
		given = np.ascontiguousarray(_starts20(picked))
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


def test_evaluator_batched_equals_sequential():
	agent = DeviceSymBallSearch(_sball(4), pops=64)
	ev = Evaluator(8, [3, 6], max_states=100)
	np.random.seed(7)
	res_b, states_b, _ = ev.eval(agent)
	assert ev.last_mode == "batched"
	np.random.seed(7)
	res_s, states_s, _ = ev.eval(agent, batched=False)
	assert ev.last_mode == "sequential"
	assert res_b.shape == (2, 8) and (res_b == res_s).all() and (states_b == states_s).all()
	assert (res_b[0] >= 0).all() and (res_b[0] <= 3).all() and (res_b <= 6).all()
