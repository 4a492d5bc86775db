"""
What DeviceBallSearchBatch (engine rk_bsearchb_*) and DeviceSymBallSearchBatch (engine rk_ssearchb_*) promise alike, stated once
and run on the GPU for `plain` and `sym`, each against its plain-Python model bit for bit (tests/ball_kinds.py names the starts,
the radii, the pop counts and the capacities of each kind):
  * reversed input with one start five times over in six slots; a long search beside a slot refilled at every poll;
  * per-state budgets and one budget for all; a pool that is full; the time limit; the edges; the Evaluator.
What differs in more than names and constants stays with its kind, in tests/test_ball_batch_gpu.py and
tests/test_symsearch_batch_gpu.py: the model comparison over slots and pops, the engines that ship, optimality against the two-sided
search, the C entries, and the symmetric starts.
The models and the device balls are those of tests/test_goal_ball_gpu.py, tests/test_symsearch_cpu.py and
tests/test_symsearch_gpu.py, made once per session.
"""
import numpy as np
import pytest

from librubiks_amd import cube
from librubiks_amd.solving import agents
from librubiks_amd.solving.evaluation import Evaluator
from tests.ball_kinds import IDS, KINDS, SYM, assert_state_equals_model
from tests.test_goal_ball_gpu import REPRS, _in_repr

pytestmark = pytest.mark.gpu

both_kinds = pytest.mark.parametrize("kind", KINDS, ids=IDS)


@both_kinds
def test_order_independence_and_duplicates(kind):
	ball, keys = kind.search_ball(kind.radius), list(kind.keys)
	forward = kind.batch(ball, searches=6, pops=kind.pops, **kind.batch_kw)
	forward.search(kind.states(keys), keep_arrays=True)
	order = list(range(len(keys)))[::-1]
	order = order[:4] + [keys.index(kind.duplicate)] * 5 + order[4:]  # five slots hold the same start at once
	b = kind.batch(ball, searches=6, pops=kind.pops, **kind.batch_kw)
	solved = b.search(kind.states(keys)[order], keep_arrays=True)
	for j, i in enumerate(order):
		assert solved[j] and list(b.action_queue_of(j)) == list(forward.action_queue_of(i))
		assert (b.status[j] == forward.status[i]).all() and b.lengths[j] == forward.lengths[i]
		for x, y in zip(b.arrays(j), forward.arrays(i)):
			assert (x == y).all()
		assert_state_equals_model(b, j, solved[j], *kind.model(kind.radius, keys[i]))


@both_kinds
def test_isolation_on_refill(kind):
	"""A long search in one of two slots while the short ones come and go in the other, which is reset at every poll: a reset that
	cleared a neighbour's table, scratch or `hit` words would change the long search's pool."""
	short = list(kind.refill_short)
	picked = [kind.refill_long] + short
	if kind is SYM:
		assert len(short) == 60 and kind.model(kind.radius, kind.refill_long)[0].depth == 4
	b = kind.batch(kind.search_ball(kind.radius), searches=2, pops=kind.pops, poll=1, **kind.batch_kw)
	solved = b.search(kind.states(picked), keep_arrays=True)
	assert solved.all() and b.iterations[0] > len(short)               # it ran while every short one came and went
	for i, key in enumerate(picked):
		assert_state_equals_model(b, i, solved[i], *kind.model(kind.radius, key))


def _pops_of_the_budget_test():
	return [pytest.param(k, pops, id=f"{k.name}-{pops}") for k in KINDS for pops in k.budget_pops]


@pytest.mark.parametrize("kind,pops", _pops_of_the_budget_test())
def test_budget_per_state(kind, pops):
	full, _ = kind.model(kind.radius, kind.budget_full)
	if kind is SYM:
		assert full.result and full.len > 5_012
	cases = kind.budget_cases(full.len)
	starts = kind.states([key for key, _ in cases])
	budgets = np.array([x or 10 ** 10 for _, x in cases], np.int64)
	b = kind.batch(kind.search_ball(kind.radius), searches=4, pops=pops, **kind.batch_kw)
	solved = b.search(starts, max_states=budgets, keep_arrays=True)
	for i, (key, budget) in enumerate(cases):
		want, _ = kind.model(kind.radius, key, budget)
		assert_state_equals_model(b, i, solved[i], want)
		assert b.stops[i] == (1 if want.result else 2)
	assert not solved[0] and solved[1] and not solved[4]
	if kind is SYM:
		assert not solved[5] and solved[6]
	# one budget for all
	solved = b.search(starts, max_states=150, keep_arrays=True)
	for i, (key, _) in enumerate(cases):
		want, _ = kind.model(kind.radius, key, 150)
		assert_state_equals_model(b, i, solved[i], want)
		if kind is SYM:
			assert b.stops[i] == (1 if want.result else 2)
	if kind is SYM:
		assert not solved[0] and (b.stops == 2).any() and (b.stops == 1).any()


@both_kinds
def test_pool_full(kind):
	capacity, pops = 3_000, 64
	picked = list(kind.pool_full)
	want, _ = kind.model(kind.radius, picked[1])
	assert want.len > capacity and all(kind.model(kind.radius, key)[0].len + 12 * pops <= capacity for key in picked[:1] + picked[2:])
	b = kind.batch(kind.search_ball(kind.radius), searches=3, pops=pops, capacity=capacity)
	solved = b.search(kind.states(picked), keep_arrays=True)
	assert not solved[1] and b.capacity_exhausted.tolist() == [False, True] + [False] * 5
	assert b.stops[1] == 5 and b.status[1, 0] == 1 and b.status[1, 1] == 0 and b.status[1, 6] == 0      # done, not won, no error
	assert b.lengths[1] == -1 and list(b.action_queue_of(1)) == [] and b.meeting_depths[1] == -1 and b.status[1, 9] == 0
	n = int(b.sizes[1])
	assert capacity - 12 * pops < n <= capacity                       # it stopped because 12 x (at most `pops`) children might not fit
	states, parents, actions = b.arrays(1)
	assert len(states) == n
	assert (states == want.states[:n]).all() and (parents == want.parents[:n]).all() and (actions == want.actions[:n]).all()
	for i, key in enumerate(picked):
		if i != 1:
			assert_state_equals_model(b, i, solved[i], *kind.model(kind.radius, key))


@both_kinds
def test_edges(kind):
	ball = kind.search_ball(2)
	b = kind.batch(ball, searches=3, pops=7, **kind.batch_kw)
	solved = b.search(np.zeros((0, 20), np.int8))
	assert solved.shape == (0,) and solved.dtype == bool and b._h is None                      # the device was not touched
	assert b.lengths.shape == (0,) and b.status.shape == (0, 10) and b.meeting_depths.shape == (0,)
	start = kind.state(kind.edge)
	want, popped = kind.model(2, kind.edge)
	solved = b.search(start[None], keep_arrays=True)                                            # n = 1
	assert_state_equals_model(b, 0, solved[0], want, popped)
	with pytest.raises(IndexError):
		b.action_queue_of(1)
	solved = b.search(start[None])
	with pytest.raises(ValueError):
		b.arrays(0)
	start, (want, _) = kind.state(kind.edge_between), kind.model(2, kind.edge_between)
	for rep in REPRS:
		cube.set_is2024(rep == "2024")
		solved = b.search(np.stack([cube.get_solved(), _in_repr(start[None])[0], cube.get_solved()]))
		assert solved.all() and b.lengths.tolist() == [0, len(want.queue), 0]
		assert b.sizes.tolist()[::2] == [1, 1] and b.iterations.tolist()[::2] == [0, 0] and b.meeting_depths.tolist()[::2] == [0, 0]
		assert list(b.action_queue_of(0)) == [] and b.status[0, 9] == 1                          # the meeting node: the ball's node 1
	cube.set_is2024(False)
	fresh = kind.batch(ball, searches=3, pops=7)
	bad = np.stack([cube.get_solved(), np.zeros((6, 8, 6), np.int8), cube.get_solved()])
	with pytest.raises(ValueError):
		fresh.search(bad)                                                                        # an illegal 6x8x6 state: before anything runs
	assert fresh._h is None and fresh.status.shape == (0, 10)                                   # nothing of the call was run


@both_kinds
def test_time_limit_bounds_the_whole_call(monkeypatch, kind):
	b = kind.batch(kind.search_ball(kind.radius), searches=2, pops=1, poll=1, **kind.batch_kw)
	picked = list(kind.time_limit)
	solved = b.search(kind.states(picked), time_limit=1e-9)           # passed before the first poll: nothing is started
	assert not solved.any() and not b.status.any() and (b.lengths == -1).all() and b.lockstep_iterations == 0
	# a clock that moves one second per look: the call starts two searches, runs two iterations and is out of time at its
	# fourth poll, with two searches running (a long start pops one node per iteration here) and two waiting
	clock = iter(range(1_000))
	monkeypatch.setattr(agents.time, "perf_counter", lambda: float(next(clock)))
	solved = b.search(kind.states(picked), time_limit=3.5, keep_arrays=True)
	monkeypatch.undo()
	assert not solved.any() and (b.stops == 0).all() and (b.lengths == -1).all() and not b.capacity_exhausted.any()
	assert b.lockstep_iterations == 2 and b.iterations.tolist() == [2, 2, 0, 0] and b.popped.tolist() == [2, 2, 0, 0]
	assert (b.sizes[:2] > 1).all() and b.sizes[2:].tolist() == [0, 0] and (b.status[:, 0] == 0).all()
	for i in (0, 1):
		want, (states, parents, actions) = kind.model(kind.radius, picked[i])[0], b.arrays(i)
		n = int(b.sizes[i])
		assert len(states) == n and (states == want.states[:n]).all() and (parents == want.parents[:n]).all()
	assert [len(x) for x in b.arrays(2)] == [0, 0, 0]
	again = picked[kind.time_limit_again]
	solved = b.search(kind.states(again))                             # and the engine is as good as new
	for i, key in enumerate(again):
		assert_state_equals_model(b, i, solved[i], *kind.model(kind.radius, key), arrays=False)


@both_kinds
def test_evaluator_batched_equals_sequential(kind):
	agent = kind.search(kind.search_ball(4), pops=64)
	ev = Evaluator(8, [3, 6], max_states=100)
	np.random.seed(7)
	res_b, states_b, _ = ev.eval(agent)
	assert ev.last_mode == "batched"
	np.random.seed(7)
	res_s, states_s, _ = ev.eval(agent, batched=False)
	assert ev.last_mode == "sequential"
	assert res_b.shape == (2, 8) and (res_b == res_s).all() and (states_b == states_s).all()
	assert (res_b[0] >= 0).all() and (res_b[0] <= 3).all() and (res_b <= 6).all()
