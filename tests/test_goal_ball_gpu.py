"""
DeviceGoalBall (engine rk_ball_*) and DeviceBallSearch (engine rk_bsearch_*) on the GPU:
  * the radius-4 ball (11 206 states) against the plain-Python model (tests/ball_model.py), bit for bit, built with pops 1 / 7 /
    4096 (a level boundary on a batch's edge, inside a batch, a whole level in one batch), in both representations;
  * `depth` and `solve` on every state of that ball (11 206 is no multiple of 256), on all of level 5 and on 20-move scrambles
    (outside: -1), on n = 0 and n = 1, and in the 6x8x6 form;
  * the search against the model: balls of radius 2 and 4, seeded scrambles of 1, 2, 3, 5, 6, 7 and 8 moves, two seeds each, pops
    1 / 7 / 4096, both representations: return value, queue, len, depth, meeting, meeting_depth and arrays() -- and the three runs
    equal to each other;
  * radius 0 is DeviceBFS: queue, len and arrays() of the engine that already ships;
  * optimality: a 12-move start against a radius-6 ball and 7-move starts, with the lengths DeviceBiBFS finds;
  * the state budget, the pool (growth, exhaustion), the edges and the C entries.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import CapacityExhausted, DeviceBallSearch, DeviceBFS, DeviceBiBFS, DeviceGoalBall
from tests import ball_model as model
from tests.test_bibfs_device_gpu import LEVELS

pytestmark = pytest.mark.gpu

REPRS = ("2024", "686")
POPS = (1, 7, 4096)
STARTS = [(d, s) for d in (1, 2, 3, 5, 6, 7, 8) for s in (0, 1)]

_device_balls = {}


def _start(depth: int, seed: int) -> np.ndarray:
	return model.scramble(1000 * depth + seed, depth)


@functools.lru_cache(maxsize=None)
def _model_ball(radius: int):
	return model.build(radius)


@functools.lru_cache(maxsize=None)
def _model(radius: int, depth: int, seed: int, budget: int = None):
	return model.search(_start(depth, seed), _model_ball(radius), max_states=budget)


def _ball(radius: int) -> DeviceGoalBall:
	"""One device ball per radius for the whole module (it is read-only once built)."""
	if radius not in _device_balls:
		_device_balls[radius] = DeviceGoalBall(radius).build()
	return _device_balls[radius]


def _in_repr(states20: np.ndarray) -> np.ndarray:
	"""20-byte states in the current representation."""
	return states20 if cube.get_is2024() else cube.as686(states20)


def _apply_rows(states20: np.ndarray, actions: np.ndarray) -> np.ndarray:
	"""Row i of `actions` (padded with -1) applied to state i, with the oracle's moves."""
	out = np.array(states20, np.int8)
	for k in range(actions.shape[1]):
		rows = np.nonzero(actions[:, k] >= 0)[0]
		if len(rows):
			a = actions[rows, k]
			out[rows] = model.orc.multi_rotate(out[rows], a // 2, 1 - a % 2)
	return out


def _assert_ball_equals_model(ball: DeviceGoalBall, want):
	assert len(ball) == want.len and ball.built
	assert ball.level_start.dtype == np.int64 and ball.level_start.tolist() == want.level_start.tolist()
	states, parents, actions = ball.arrays()
	assert states.dtype == np.int8 and parents.dtype == np.int64 and actions.dtype == np.int64
	assert (states == _in_repr(want.states)).all() and (parents == want.parents).all() and (actions == want.actions).all()


def _assert_equals_model(agent, ok, want):
	assert ok == want.result
	assert list(agent.action_queue) == want.queue
	assert len(agent) == want.len and agent.depth == want.depth
	if want.meeting is None:
		assert agent.meeting is None and agent.meeting_depth is None
	else:
		assert (agent.meeting == _in_repr(want.meeting)).all() and agent.meeting_depth == want.meeting_depth
	states, parents, actions = agent.arrays()
	assert states.dtype == np.int8 and states.shape[0] == want.len
	assert (states == _in_repr(want.states)).all()
	assert (parents == want.parents).all() and (actions == want.actions).all()


@pytest.mark.parametrize("rep", REPRS)
def test_ball_against_the_model_and_independent_of_pops(rep):
	want = _model_ball(4)
	assert want.len == 11_206 and np.diff(want.level_start).tolist() == LEVELS[:5]
	cube.set_is2024(rep == "2024")
	runs = []
	for pops in POPS:
		ball = DeviceGoalBall(4, pops=pops)
		_assert_ball_equals_model(ball, want)
		assert ball.iterations == sum(-(-n // pops) for n in LEVELS[:4])        # no batch crosses a level boundary
		runs.append((len(ball), ball.level_start, *ball.arrays()))
	for other in runs[1:]:
		assert other[0] == runs[0][0]
		for x, y in zip(other[1:], runs[0][1:]):
			assert (x == y).all()


def test_small_balls():
	zero = DeviceGoalBall(0, pops=7)
	assert len(zero) == 1 and zero.level_start.tolist() == [1, 2] and zero.iterations == 0
	states, parents, actions = zero.arrays()
	assert (states == cube.get_solved()[None]).all() and parents.tolist() == [0] and actions.tolist() == [-1]
	assert zero.depth(cube.get_solved()[None]).tolist() == [0] and zero.depth(_start(1, 0)[None]).tolist() == [-1]
	lengths, acts = zero.solve(np.stack([cube.get_solved(), _start(1, 0)]))
	assert lengths.tolist() == [0, -1] and acts.shape == (2, 0)
	for radius in (1, 2, 3):
		_assert_ball_equals_model(DeviceGoalBall(radius, pops=5), _model_ball(radius))
	assert zero.build() is zero and len(zero) == 1                            # building again does nothing


@pytest.mark.parametrize("rep", REPRS)
def test_depth_and_solve(rep):
	want, ball = _model_ball(4), _ball(4)
	cube.set_is2024(rep == "2024")
	# every state of the ball: the model's depth and the model's path, and every row solves its cube
	depths = ball.depth(_in_repr(want.states))
	assert depths.dtype == np.int64 and depths.shape == (want.len,)
	want_depths = np.searchsorted(want.level_start, np.arange(1, want.len + 1), side="right") - 1
	assert (depths == want_depths).all() and np.bincount(depths).tolist() == LEVELS[:5]
	lengths, actions = ball.solve(_in_repr(want.states))
	assert lengths.dtype == np.int64 and actions.dtype == np.int64 and actions.shape == (want.len, 4)
	assert (lengths == want_depths).all()
	assert ((actions >= 0).sum(axis=1) == lengths).all() and (actions[np.arange(4)[None] >= lengths[:, None]] == -1).all()
	for node in range(1, want.len + 1, 37):
		assert actions[node - 1, :lengths[node - 1]].tolist() == model.ball_path(want, node)
	assert model.orc.multi_is_solved(_apply_rows(want.states, actions)).all()
	# outside: all of level 5 (every child of level 4 that the ball does not hold) and 20-move scrambles
	level4 = want.states[want.level_start[4] - 1:]
	children = model.orc.expand12(level4)
	level5 = np.unique(children[[c.tobytes() not in want.index for c in children]], axis=0)
	assert len(level5) == LEVELS[5]
	far = np.stack([model.scramble(20_000 + s, 20) for s in range(16)])
	assert all(model.depth(want, s) == -1 for s in far)
	for outside in (level5, far):
		assert (ball.depth(_in_repr(outside)) == -1).all()
		lengths, actions = ball.solve(_in_repr(outside))
		assert (lengths == -1).all() and (actions == -1).all() and actions.shape == (len(outside), 4)
	# a mixed batch, n = 1 and n = 0
	mixed = np.concatenate([far[:3], want.states[[0, 5, 11_205]], level5[:2]])
	assert ball.depth(_in_repr(mixed)).tolist() == [-1, -1, -1, 0, 1, 4, -1, -1]
	assert ball.solve(_in_repr(mixed))[0].tolist() == [-1, -1, -1, 0, 1, 4, -1, -1]
	one = _in_repr(want.states[200:201])
	assert ball.depth(one).tolist() == [int(want_depths[200])] and ball.solve(one)[1][0].tolist() == actions_of(want, 201)
	none = _in_repr(want.states[:0])
	assert ball.depth(none).shape == (0,) and ball.depth(none).dtype == np.int64
	lengths, actions = ball.solve(none)
	assert lengths.shape == (0,) and actions.shape == (0, 4)
	with pytest.raises(ValueError):
		ball.depth(np.zeros((3, 19), np.int8))


def actions_of(ball, node: int) -> list:
	path = model.ball_path(ball, node)
	return path + [-1] * (ball.radius - len(path))


@pytest.mark.parametrize("rep", REPRS)
@pytest.mark.parametrize("radius", [2, 4])
@pytest.mark.parametrize("depth,seed", STARTS)
def test_search_against_the_model_and_independent_of_pops(depth, seed, radius, rep):
	want = _model(radius, depth, seed)
	assert want.result
	cube.set_is2024(rep == "2024")
	start = _in_repr(_start(depth, seed))
	runs = []
	for pops in POPS:
		agent = DeviceBallSearch(_ball(radius), pops=pops, poll=256 if pops == 1 else 8)
		ok = agent.search(start.copy())
		_assert_equals_model(agent, ok, want)
		if len(want.queue) == want.meeting_depth:              # the ball holds the start (len == 1 alone does not say so: the
			assert want.len == 1 and agent.iterations == 0 and agent.popped == 0        # first child of the first pop may meet)
		else:
			assert want.meeting_depth == radius and agent.iterations >= 1 and agent.popped >= 1
		runs.append((ok, list(agent.action_queue), len(agent), agent.depth, agent.meeting_depth, agent.meeting, agent.arrays(), agent.popped))
	for other in runs[1:]:
		assert other[:5] == runs[0][:5] and other[7] == runs[0][7]
		assert (other[5] == runs[0][5]).all()
		for x, y in zip(other[6], runs[0][6]):
			assert (x == y).all()


@pytest.mark.parametrize("depth,seed", [(5, 0), (5, 1), (6, 0), (6, 1)])
def test_radius_zero_is_the_one_sided_search(depth, seed):
	start = _start(depth, seed)
	one = DeviceBFS(pops=7)
	assert one.search(start.copy(), max_states=10_000_000)
	for pops in (7, 4096):
		agent = DeviceBallSearch(_ball(0), pops=pops)
		assert agent.search(start.copy(), max_states=10_000_000)
		assert list(agent.action_queue) == list(one.action_queue) and len(agent) == len(one)
		assert agent.meeting_depth == 0 and cube.is_solved(agent.meeting) and agent.depth == len(one.action_queue) - 1
		for x, y in zip(agent.arrays(), one.arrays()):
			assert (x == y).all()
	# the budget too: the same prefix of the pool and the same refusal
	budget = len(one) // 2
	assert not one.search(start.copy(), max_states=budget)
	agent = DeviceBallSearch(_ball(0), pops=7)
	assert not agent.search(start.copy(), max_states=budget) and len(agent) == len(one)
	for x, y in zip(agent.arrays(), one.arrays()):
		assert (x == y).all()


def test_optimal_against_the_two_sided_search():
	ball = _ball(6)
	assert len(ball) == sum(LEVELS[:7]) and np.diff(ball.level_start).tolist() == LEVELS[:7]
	two, agent = DeviceBiBFS(), DeviceBallSearch(ball)
	start = model.scramble(12_001, 12)
	assert two.search(start.copy()) and len(two.action_queue) == 12
	assert agent.search(start.copy())
	print(f"12-move scramble: length {len(agent.action_queue)}, {len(agent)} states (two-sided: {len(two)}), depth {agent.depth}, "
	      f"{agent.iterations} iterations")
	assert len(agent.action_queue) == 12 == agent.depth + 1 + 6 and agent.meeting_depth == 6
	assert model.orc.is_solved(model.apply(start, agent.action_queue))
	assert (agent.meeting == model.apply(start, list(agent.action_queue)[:agent.depth + 1])).all()
	assert ball.depth(agent.meeting[None]).tolist() == [6]
	lengths = []
	for seed in range(8):
		start = model.scramble(7000 + seed, 7)
		assert two.search(start.copy()) and agent.search(start.copy())
		assert len(agent.action_queue) == len(two.action_queue) <= 7
		assert model.orc.is_solved(model.apply(start, agent.action_queue))
		lengths.append(len(agent.action_queue))
	assert max(lengths) == 7


@pytest.mark.parametrize("pops", [7, 4096])
def test_budget(pops):
	radius, depth, seed = 2, 7, 0
	start = _start(depth, seed)
	full = _model(radius, depth, seed)
	assert full.result and full.len > 5_012
	agent = DeviceBallSearch(_ball(radius), pops=pops)
	for budget in (1, 2, 150, 5_000, full.len - 12, full.len):
		want = _model(radius, depth, seed, budget)
		assert want.len < budget + 12 and (want.result or budget <= want.len)
		ok = agent.search(start.copy(), max_states=budget)
		_assert_equals_model(agent, ok, want)
		assert len(agent) < budget + 12
	assert not _model(radius, depth, seed, full.len - 12).result
	# the agent is reusable: an unbounded search after those equals a fresh agent's
	ok = agent.search(start.copy())
	_assert_equals_model(agent, ok, full)
	fresh = DeviceBallSearch(_ball(radius), pops=pops)
	assert fresh.search(start.copy()) == ok and list(fresh.action_queue) == list(agent.action_queue)
	for x, y in zip(fresh.arrays(), agent.arrays()):
		assert (x == y).all()


@pytest.mark.parametrize("pops", [7, 64])
def test_growth_changes_nothing(pops):
	for depth, seed in ((7, 0), (8, 1)):
		agent = DeviceBallSearch(_ball(2), pops=pops, capacity=2 * 12 * pops, poll=16)
		ok = agent.search(_start(depth, seed))
		assert agent.grown > 0 and not agent.capacity_exhausted
		_assert_equals_model(agent, ok, _model(2, depth, seed))


def test_exhausted_pool_warns():
	agent = DeviceBallSearch(_ball(2), pops=64, capacity=2 * 12 * 64, max_capacity=4_000)
	with pytest.warns(CapacityExhausted):
		assert not agent.search(_start(8, 0))
	assert agent.capacity_exhausted and 1 < len(agent) <= 4_000 and list(agent.action_queue) == [] and agent.meeting is None
	want = _model(2, 8, 0)
	states, parents, actions = agent.arrays()
	n = len(agent)
	assert (states == want.states[:n]).all() and (parents == want.parents[:n]).all() and (actions == want.actions[:n]).all()


def test_solved_inside_illegal_and_one_move_starts():
	for rep in REPRS:
		cube.set_is2024(rep == "2024")
		for radius in (0, 2):
			agent = DeviceBallSearch(_ball(radius), pops=7)
			assert agent.search(cube.get_solved(), max_states=100)
			assert len(agent) == 1 and list(agent.action_queue) == [] and agent.depth == 0
			assert cube.is_solved(agent.meeting) and agent.meeting_depth == 0
			assert agent.iterations == 0 and agent.popped == 0 and [len(x) for x in agent.arrays()] == [1, 1, 1]
			for a in range(12):
				start = cube.rotate(cube.get_solved(), *cube.action_space[a])
				assert agent.search(start)
				assert list(agent.action_queue) == [cube.rev_action(a)] and agent.depth == 0
				if radius == 0:                                      # the children before the one that meets were stored
					assert cube.is_solved(agent.meeting) and agent.popped == 1 and len(agent) == 1 + cube.rev_action(a)
					assert agent.meeting_depth == 0 and agent.iterations == 1
				else:                                                # the ball holds the start
					assert (agent.meeting == start).all() and agent.popped == 0 and len(agent) == 1
					assert agent.meeting_depth == 1 and agent.iterations == 0
		# a start inside the ball: the ball's path, whatever the budget
		inside = DeviceBallSearch(_ball(4), pops=7)
		for depth, seed in ((2, 0), (3, 0), (6, 0)):
			want = _model(4, depth, seed)
			assert want.result and want.len == 1 and len(want.queue) == want.meeting_depth
			ok = inside.search(_in_repr(_start(depth, seed)), max_states=1)
			_assert_equals_model(inside, ok, want)
			assert inside.iterations == 0 and inside.popped == 0
	cube.set_is2024(False)
	bad = np.zeros((6, 8, 6), np.int8)
	with pytest.raises(ValueError):
		DeviceBallSearch(_ball(2)).search(bad, max_states=100)
	with pytest.raises(ValueError):
		_ball(2).depth(bad[None])
	with pytest.raises(ValueError):
		_ball(2).solve(bad[None])


def test_two_agents_share_one_ball():
	ball = DeviceGoalBall(2, pops=64)
	a, b = DeviceBallSearch(ball, pops=7), DeviceBallSearch(ball, pops=4096)
	assert a.ball is ball and b.ball is ball
	ok_a = a.search(_start(6, 1))
	ok_b = b.search(_start(7, 1))
	_assert_equals_model(a, ok_a, _model(2, 6, 1))                      # read after the other agent searched
	_assert_equals_model(b, ok_b, _model(2, 7, 1))
	ok_a = a.search(_start(7, 0))
	_assert_equals_model(b, ok_b, _model(2, 7, 1))
	_assert_equals_model(a, ok_a, _model(2, 7, 0))
	ok_b = b.search(_start(5, 1))
	_assert_equals_model(b, ok_b, _model(2, 5, 1))
	_assert_ball_equals_model(ball, _model_ball(2))                     # and the ball is what it was
	status = (C.c_longlong * 16)()
	_ffi.check(_ffi.lib().rk_ball_status(ball._h, status))
	assert status[5] == 2
	del a
	_ffi.check(_ffi.lib().rk_ball_status(ball._h, status))
	assert status[5] == 1


def test_c_entries_refuse_bad_arguments():
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	ball, h = C.c_void_p(), C.c_void_p()
	_ffi.check(lib.rk_ball_create(C.byref(ball), 2, 8))
	_ffi.check(lib.rk_bsearch_create(C.byref(h), ball, 1_000, 8))
	try:
		buf = np.zeros(20, np.int8)
		start = model.scramble(5, 5)
		status = (C.c_longlong * 16)()
		queries = torch.from_numpy(np.stack([model.orc.SOLVED, start]).astype(np.int8)).to("cuda")
		out = torch.full((2,), 7, dtype=torch.int32, device="cuda")
		acts = torch.full((2, 2), 7, dtype=torch.int8, device="cuda")
		# before the build
		assert lib.rk_ball_export(ball, 1, 1, buf.ctypes.data, None, None, stream) == -4             # RK_ESTATE
		assert lib.rk_ball_depth(ball, queries.data_ptr(), 2, out.data_ptr(), stream) == -4
		assert lib.rk_ball_solve(ball, queries.data_ptr(), 2, out.data_ptr(), acts.data_ptr(), stream) == -4
		assert lib.rk_bsearch_reset(h, start.ctypes.data, 100, stream) == -4
		assert lib.rk_bsearch_run(h, 1, stream) == -4 and lib.rk_bsearch_path(h, None, 16, stream) == -4
		assert lib.rk_bsearch_export(h, 1, 1, buf.ctypes.data, None, None, stream) == -4
		_ffi.check(lib.rk_ball_build(ball, 8, stream))
		_ffi.check(lib.rk_ball_build(ball, 8, stream))                                               # built: nothing to do
		_ffi.check(lib.rk_ball_status(ball, status))
		assert list(status[:10]) == [1, 127, 3, 2, 127, 1, 1, 2, 14, 128]                            # 1 + 2 iterations of at most 8 pops
		# the queries
		assert lib.rk_ball_depth(ball, None, 2, out.data_ptr(), stream) == -1                        # RK_EINVAL: null pointers
		assert lib.rk_ball_depth(ball, queries.data_ptr(), 2, None, stream) == -1
		assert lib.rk_ball_depth(ball, queries.data_ptr() + 1, 1, out.data_ptr(), stream) == -1      # misaligned
		assert lib.rk_ball_solve(ball, queries.data_ptr(), 2, out.data_ptr(), None, stream) == -1
		assert lib.rk_ball_solve(ball, queries.data_ptr(), 2, None, acts.data_ptr(), stream) == -1
		assert lib.rk_ball_depth(ball, None, 0, None, stream) == 0                                   # no queries: nothing to do
		_ffi.check(lib.rk_ball_depth(ball, queries.data_ptr(), 2, out.data_ptr(), stream))
		assert out.tolist() == [0, -1]
		_ffi.check(lib.rk_ball_solve(ball, queries.data_ptr(), 2, out.data_ptr(), acts.data_ptr(), stream))
		assert out.tolist() == [0, -1] and acts.tolist() == [[-1, -1], [-1, -1]]
		assert lib.rk_ball_export(ball, 1, 128, buf.ctypes.data, None, None, stream) == -1           # rows outside the pool
		assert lib.rk_ball_export(ball, 128, 1, buf.ctypes.data, None, None, stream) == -1
		_ffi.check(lib.rk_ball_export(ball, 1, 1, buf.ctypes.data, None, None, stream))
		assert (buf == model.orc.SOLVED).all()
		# a ball with a search attached refuses to go
		assert lib.rk_ball_destroy(ball) == -4 and b"search" in lib.rk_last_error()
		# the search, through the C ABI alone
		assert lib.rk_bsearch_reset(h, None, 100, stream) == -1
		_ffi.check(lib.rk_bsearch_reset(h, start.ctypes.data, 100, stream))
		assert lib.rk_bsearch_size(h) == 1
		assert lib.rk_bsearch_path(h, None, 16, stream) == -1                                        # RK_EINVAL: null output
		path = (C.c_longlong * 16)()
		assert lib.rk_bsearch_path(h, path, 16, stream) == -4                                        # RK_ESTATE: not met
		assert lib.rk_bsearch_export(h, 1, 1_001, buf.ctypes.data, None, None, stream) == -1         # rows outside the pool
		assert lib.rk_bsearch_grow(h, 500, stream) == -1
		assert lib.rk_bsearch_run(h, -1, stream) == -1
		st = (C.c_longlong * 10)()
		for _ in range(64):
			_ffi.check(lib.rk_bsearch_run(h, 1, stream))
			_ffi.check(lib.rk_bsearch_status(h, st, stream))
			if st[0]:
				break
		assert st[0] == 1 and st[1] == 0 and st[5] == 2 and 100 <= st[2] < 112                       # stopped by its budget
		_ffi.check(lib.rk_bsearch_reset(h, start.ctypes.data, 1_000, stream))
		_ffi.check(lib.rk_bsearch_run(h, 64, stream))
		_ffi.check(lib.rk_bsearch_status(h, st, stream))
		want = model.search(start, _model_ball(2))
		assert st[0] == 1 and st[1] == 1 and st[2] == want.len and st[8] == want.depth
		n = lib.rk_bsearch_path(h, path, 16, stream)
		assert list(path[:n]) == want.queue
	finally:
		assert lib.rk_bsearch_destroy(h) == 0
		assert lib.rk_ball_destroy(ball) == 0
