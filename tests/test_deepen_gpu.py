"""
Depth-first probes past the symmetry ball on the GPU (engines rk_sdeepen and rk_sdeepen_*), balls of radius 2 and 3.
  * `DeviceSymBall.solve_beyond`, words and lengths bit for bit against tests/deepen_model.py: all states of levels R + 1 and
    R + 2 and a seeded few hundred of R + 3, states inside the ball and states with fewer than 48 conjugates mixed in; n of 1, 63,
    64, 65 and 130; with and without last actions; `extra` too small; the launch cap lowered so that a round takes several launches
    whose first word is no multiple of a wave's 121 ranks; lengths against `DeviceBiBFS`;
  * `DeviceSymBallSearch(deepen=E)` on a radius-2 ball with a pool of 1 500 states, which holds the own levels 0..3 (1 195 states)
    and not level 4: starts of optimal length 7, 8 and 9 come back solved with `deepened` 2, 3 and 4 and the model's queue, at pops
    1, 16 and 4 096, frontier chunks of 1, 3 and more than the frontier, and a lowered launch cap; a start where a later frontier
    node has a lower-ranked word than the winning node; `deepen=0` unchanged;
  * the entries' error paths.  Nothing here provokes a fault: out-of-range arguments are refused on the host before any launch.
"""
import ctypes as C
import functools
import time
import warnings

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, gpu
from librubiks_amd.solving.agents import CapacityExhausted, DeviceBiBFS, DeviceSymBall, DeviceSymBallSearch
from tests import ball_model
from tests import deepen_model as model
from tests import sym_model
from tests.test_deepen_cpu import level_states, plain_ball, sym_ball

pytestmark = pytest.mark.gpu

orc = ball_model.orc
POOL = 1_500                                       # the own levels 0..3 of a far start hold 1 + 12 + 114 + 1 068 = 1 195 states
#: starts 7, 8 and 9 quarter turns from solved: (seed, moves) of a seeded scramble
FAR = {7: (3, 9), 8: (3, 10), 9: (0, 9)}
#: 8 quarter turns from solved; in round 3 frontier node 144 has a hit and node 146 one of lower rank: node 144 must win
TWO_HITS = (0, 2, 4, 6, 8, 10, 1, 3)
_balls = {}


def _ball(radius: int) -> DeviceSymBall:
	if radius not in _balls:
		_balls[radius] = DeviceSymBall(radius).build()
	return _balls[radius]


def _far(length: int) -> np.ndarray:
	seed, moves = FAR[length]
	return ball_model.apply(orc.SOLVED, np.random.RandomState(seed).randint(0, 12, moves))


@functools.lru_cache(maxsize=None)
def _queries(radius: int):
	"""(states, extra that answers all): levels R + 1 and R + 2, a seeded 300 of R + 3, 40 states inside the ball and the
	symmetric states that lie within R + 3, shuffled."""
	rng = np.random.RandomState(radius)
	known = plain_ball(radius + 2)
	kids = orc.expand12(level_states(radius, radius + 2)[rng.choice(len(level_states(radius, radius + 2)), 400, replace=False)])
	beyond = np.array([k for k in kids if k.tobytes() not in known.index][:300])                 # R + 3 quarter turns from solved
	inside = plain_ball(radius).states[rng.choice(plain_ball(radius).len, 40)]
	symmetric = np.array([ball_model.apply(orc.SOLVED, w) for w in ((4, 6), (4, 7), (4, 6, 4), (4, 6, 4, 6), (4, 7, 4, 7), (0, 2, 0, 2), (4, 6, 4, 6, 0))])
	assert (sym_model.canonical(symmetric)[2] < 48).all()
	states = np.concatenate([level_states(radius, radius + 1), level_states(radius, radius + 2), beyond, inside, symmetric])
	return states[rng.permutation(len(states))]


@functools.lru_cache(maxsize=None)
def _modelled(radius: int):
	return model.solve_beyond(sym_ball(radius), _queries(radius), 3)


@pytest.mark.parametrize("radius", (2, 3))
def test_solve_beyond_equals_the_model(radius):
	ball, states = _ball(radius), _queries(radius)
	want_len, want_act = _modelled(radius)
	assert set(want_len.tolist()) >= {radius, radius + 1, radius + 2, radius + 3} and (want_len >= 0).all() and (want_len < radius).any()
	lengths, actions = ball.solve_beyond(states, 3)
	assert lengths.dtype == np.int64 and actions.dtype == np.int64 and actions.shape == (len(states), 3 + radius)
	assert (lengths == want_len).all() and (actions == want_act).all()
	# the launch cap lowered: a state's 1 331 .. 1 584 words of round 3 go in ranges of 500, whose first word is no multiple of 121
	few = states[:700]
	try:
		ball.deepen_cap = 500
		split_len, split_act = ball.solve_beyond(few, 3)
	finally:
		ball.deepen_cap = None
	assert (split_len == want_len[:700]).all() and (split_act == want_act[:700]).all()
	# extra too small: -1, and what the ball holds or a smaller extra reaches is still answered
	short_len, short_act = ball.solve_beyond(few, 1)
	far = want_len[:700] > radius + 1
	assert far.any() and (short_len[far] == -1).all() and (short_act[far] == -1).all()
	assert (short_len[~far] == want_len[:700][~far]).all() and (short_act[~far] == want_act[:700][~far][:, :1 + radius]).all()
	# extra = 0 is solve
	for got, ref in zip(ball.solve_beyond(few, 0), ball.solve(few)):
		assert (got == ref).all()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_solve_beyond_batch_sizes(n):
	ball, states = _ball(2), _queries(2)[100:100 + n]
	want_len, want_act = _modelled(2)
	lengths, actions = ball.solve_beyond(states, 3)
	assert (lengths == want_len[100:100 + n]).all() and (actions == want_act[100:100 + n]).all()


@pytest.mark.parametrize("radius", (2, 3))
def test_solve_beyond_with_last_actions(radius):
	ball = _ball(radius)
	rng = np.random.RandomState(10 + radius)
	states = _queries(radius)[:600]
	last = rng.randint(-1, 12, len(states))
	last[::7] = -1                                                       # none among real ones
	want_len, want_act = model.solve_beyond(sym_ball(radius), states, 3, last)
	free = _modelled(radius)[0][:600]
	assert (want_len != free).any() and (want_len[last < 0] == free[last < 0]).all()      # the pruned turn was some state's only way
	lengths, actions = ball.solve_beyond(states, 3, last_actions=last)
	assert (lengths == want_len).all() and (actions == want_act).all()
	with pytest.raises(ValueError):
		ball.solve_beyond(states, 3, last_actions=last[:-1])
	with pytest.raises(ValueError):
		ball.solve_beyond(states, 3, last_actions=np.full(len(states), 12))


@pytest.mark.parametrize("radius", (2, 3))
def test_solve_beyond_lengths_are_bibfs_lengths(radius):
	"""An independent engine on the same states: a seeded 300 of the queries, levels R + 1, R + 2 and R + 3 among them."""
	ball, bibfs = _ball(radius), DeviceBiBFS(pops=256)
	want = _modelled(radius)[0]
	pick = np.concatenate([np.nonzero(want == radius + e)[0][:100] for e in (1, 2, 3)])
	assert len(pick) == 300
	states = _queries(radius)[pick]
	lengths, actions = ball.solve_beyond(states, 3)
	assert {radius + 1, radius + 2, radius + 3} == set(lengths.tolist())
	for s, n, acts in zip(states, lengths, actions):
		assert bibfs.search(s.copy()) and len(bibfs.action_queue) == n
		assert orc.is_solved(ball_model.apply(s, acts[:n]))


# ---- DeviceSymBallSearch(deepen=E) -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _continued(start: bytes):
	return model.continue_from_frontier(np.frombuffer(start, np.int8), sym_ball(2), POOL, 4)


def _deep_agent(**kw) -> DeviceSymBallSearch:
	return DeviceSymBallSearch(_ball(2), capacity=POOL, max_capacity=POOL, poll=64, deepen=4, **kw)


def _assert_continued(agent, ok, start, want):
	assert ok and want.result and list(agent.action_queue) == want.queue
	assert agent.deepened == want.deepened and agent.capacity_exhausted and agent.probes > 0
	assert len(agent) == want.len and agent.depth == want.level and agent.meeting is None
	assert orc.is_solved(ball_model.apply(start, agent.action_queue))
	states, parents, actions = agent.arrays()
	assert (states == want.states).all() and (parents == want.parents).all() and (actions == want.actions).all()


@pytest.mark.parametrize("length", (7, 8, 9))
def test_deepened_search_equals_the_model_whatever_the_pops_the_chunk_and_the_cap(length):
	start = _far(length)
	want = _continued(start.tobytes())
	assert want.frontier == (128, 1195) and want.level == 3 and want.deepened == length - 3 - 2 and len(want.queue) == length
	ample = DeviceSymBallSearch(_ball(2), pops=256)
	assert ample.search(start.copy()) and len(ample.action_queue) == length and ample.deepened == 0
	for pops in (1, 16, 4096):
		agent = _deep_agent(pops=pops)
		with warnings.catch_warnings():
			warnings.simplefilter("error", CapacityExhausted)            # a search that deepening finishes does not warn
			ok = agent.search(start.copy())
		_assert_continued(agent, ok, start, want)
	agent = _deep_agent(pops=16)
	for chunk in (1, 3, 5000):
		agent.deepen_chunk = chunk
		_assert_continued(agent, agent.search(start.copy()), start, want)
	try:
		agent.deepen_chunk, agent.ball.deepen_cap = None, 3000          # rounds 2.. of a chunk take several launches
		_assert_continued(agent, agent.search(start.copy()), start, want)
	finally:
		agent.ball.deepen_cap = None


def test_the_lowest_frontier_node_wins_over_a_lower_word():
	start = ball_model.apply(orc.SOLVED, TWO_HITS)
	want = _continued(start.tobytes())
	frontier = np.arange(want.frontier[0], want.frontier[1] + 1)
	rank = model.lowest_hits(sym_ball(2), want.states[frontier - 1], want.actions[frontier - 1], want.deepened)
	later = (rank >= 0) & (rank < want.rank) & (frontier > want.node)
	assert want.deepened == 3 and later.any()                            # what this case was arranged for
	for chunk in (None, 1, 2, 5000):                                     # the two nodes in one chunk and in two
		agent = _deep_agent(pops=64)
		agent.deepen_chunk = chunk
		_assert_continued(agent, agent.search(start.copy()), start, want)


def test_without_deepen_nothing_changes():
	start = _far(8)
	plain = DeviceSymBallSearch(_ball(2), pops=16, capacity=POOL, max_capacity=POOL)
	with pytest.warns(CapacityExhausted):
		assert plain.search(start.copy()) is False
	assert plain.capacity_exhausted and plain.deepen == 0 and plain.deepened == 0 and len(plain.action_queue) == 0
	# too few rounds: unsolved, and now it warns
	short = DeviceSymBallSearch(_ball(2), pops=16, capacity=POOL, max_capacity=POOL, deepen=2)
	with pytest.warns(CapacityExhausted):
		assert short.search(start.copy()) is False
	assert short.capacity_exhausted and short.deepened == 0 and short.probes == 1068 * (11 + 121)
	# a search that fits its pool: field for field today's
	near = ball_model.apply(orc.SOLVED, np.random.RandomState(3).randint(0, 12, 9)[:5])
	a, b = DeviceSymBallSearch(_ball(2), pops=16), DeviceSymBallSearch(_ball(2), pops=16, deepen=4)
	assert a.search(near.copy()) and b.search(near.copy()) and b.deepened == 0 and b.probes == 0 and not b.capacity_exhausted
	assert list(a.action_queue) == list(b.action_queue)
	assert (len(a), a.depth, a.popped, a.iterations, a.meeting_node, a.meeting_depth) == (len(b), b.depth, b.popped, b.iterations, b.meeting_node, b.meeting_depth)
	assert (a.meeting == b.meeting).all() and all((x == y).all() for x, y in zip(a.arrays(), b.arrays()))
	# a time limit that ends the pool phase: no deepening at all
	late = _deep_agent(pops=16)
	assert late.search(_far(9).copy(), time_limit=1e-9) is False and late.deepened == 0 and late.probes == 0


def test_the_time_limit_ends_the_rounds_without_a_warning():
	"""The limit is looked at after every deepening launch, counted from the start the pool phase had.  The pool phase of a search
	is run to its end, then the rounds are entered as `search` enters them, with a start time that lies further back than the limit."""
	agent, start = _deep_agent(pops=16), _far(8)
	assert agent.search(start.copy()) and agent.deepened == 3
	queue = list(agent.action_queue)
	for chunk, launches in ((None, 1), (100, 1)):
		agent.deepen_chunk, agent.probes, agent.deepened, agent.action_queue = chunk, 0, 0, type(agent.action_queue)()
		with warnings.catch_warnings():
			warnings.simplefilter("error", CapacityExhausted)            # out of time is not "no state of the ball within reach"
			assert agent._pool_full(agent._h, time.perf_counter() - 100.0, 50.0) is False
		assert agent.deepened == 0 and len(agent.action_queue) == 0
		assert agent.probes == launches * min(chunk or 1068, 1068) * 11                      # ended after the first launch of round 1
	# with time left the same call finishes the search
	agent.deepen_chunk = None
	assert agent._pool_full(agent._h, time.perf_counter(), 1e10) is True and list(agent.action_queue) == queue and agent.deepened == 3


def test_error_paths():
	lib, ball = _ffi.lib(), _ball(2)
	states = torch.from_numpy(level_states(2, 3)[:8].copy()).to(gpu)
	best = torch.full((8,), -1, dtype=torch.int32, device=gpu)
	args = (ball._h, states.data_ptr(), None, 8)
	for extra in (0, 9):
		assert lib.rk_sdeepen(*args, extra, 0, 1, best.data_ptr(), None) == -1
	assert lib.rk_sdeepen(ball._h, states.data_ptr(), None, 1 << 20, 3, 0, 1 << 10, best.data_ptr(), None) == -1      # 2^30 probes
	assert lib.rk_sdeepen(*args, 1, 0, 12, None, None) == -1
	torch.cuda.synchronize()
	assert (best.cpu().numpy() == -1).all()                                # refused before any launch
	unbuilt = C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(unbuilt), 2, 64, 0))
	try:
		assert lib.rk_sdeepen(unbuilt, states.data_ptr(), None, 8, 1, 0, 12, best.data_ptr(), None) == -4
	finally:
		lib.rk_symball_destroy(unbuilt)
	# a search's entries: ranges, and a word that does not lead into the ball
	agent = _deep_agent(pops=16)
	start = _far(7)
	assert agent.search(start.copy()) and agent.deepened == 2
	level = (C.c_longlong * 2)()
	_ffi.check(lib.rk_sdeepen_frontier(agent._h, level, None))
	assert (level[0], level[1]) == (128, 1195)
	buf = (C.c_longlong * 64)()
	assert lib.rk_sdeepen_nodes(agent._h, 0, 128, 8, 0, 1, best.data_ptr(), None) == -1
	assert lib.rk_sdeepen_nodes(agent._h, 1, 0, 8, 0, 1, best.data_ptr(), None) == -1
	assert lib.rk_sdeepen_nodes(agent._h, 1, POOL, 8, 0, 1, best.data_ptr(), None) == -1
	assert lib.rk_sdeepen_path(agent._h, 0, 1, 0, buf, 64, None) == -1
	assert lib.rk_sdeepen_path(agent._h, len(agent) + 1, 1, 0, buf, 64, None) == -1
	assert lib.rk_sdeepen_path(agent._h, 128, 9, 0, buf, 64, None) == -1
	assert lib.rk_sdeepen_path(agent._h, 128, 1, 0, buf, 64, None) == -4       # round 1 had no hit: the word leads nowhere
	assert lib.rk_sdeepen_path(agent._h, 128, 1, 11, buf, 64, None) == -4      # a node with a last move has words 0..10
	assert lib.rk_sdeepen_set_pops(agent._h, 0, None) == -1 and lib.rk_sdeepen_set_pops(agent._h, 17, None) == -1
	want = _continued(start.tobytes())
	n = lib.rk_sdeepen_path(agent._h, want.node, 2, want.rank, buf, 64, None)
	assert n == 7 and list(buf[:7]) == want.queue
