"""
DeviceSymBallSearchBatch(deepen=E) on the GPU (engine rk_ssearchb_* with rk_sdeepenb_*): a slot whose pool is full goes on by
probes of the ball, and every state gets bit for bit what tests/deepen_model.py's `continue_from_frontier` and the single agent
`DeviceSymBallSearch(deepen=E)` give it alone.  The fixtures are those of tests/test_deepen_gpu.py: the radius-2 symmetry ball, a
pool of 1 500 states per slot -- the own levels 0..3 of a far start hold 1 195 --, the starts of optimal length 7 / 8 / 9 that
rounds 2 / 3 / 4 answer from level 3, and TWO_HITS, where a later frontier node has a lower word than the node that wins.
  * the nine states of STATES at (slots, pops) (1, 16), (3, 1), (8, 4 096): queue, round, size, level, pool, stop reason, no
    meeting against the model and the single agent; the states the pool answers against the batch at deepen=0; lengths against
    DeviceBiBFS; no CapacityExhausted warning;
  * the launch cap lowered to 3 000 and 500 probes, so that a round of a slot takes many launches and word ranges start at
    ranks that are no multiple of 121; 2 slots with refills, where a launch serves slots in different rounds, and a permutation;
  * deepen=0 is the engine as it was; too few rounds; a budget stop is not deepened; the time limit; 6x8x6 states;
  * the entries' error paths.  Nothing here provokes a fault: out-of-range arguments are refused on the host before any launch.
"""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import CapacityExhausted, DeviceBiBFS, DeviceSymBallSearch, DeviceSymBallSearchBatch
from tests import ball_model
from tests import deepen_model as model
from tests.test_deepen_cpu import sym_ball
from tests.test_deepen_gpu import FAR, POOL, TWO_HITS, _ball, _continued, _far

pytestmark = pytest.mark.gpu

orc = ball_model.orc
NEAR = np.random.RandomState(3).randint(0, 12, 9)[:5]      # a 5-move scramble: the pool answers it alone
INSIDE = (0, 2)                                            # two quarter turns: the ball holds it
SIX = (0, 6)                                               # (seed, moves) of a start 6 quarter turns from solved that fills its pool
KEY_NONE = 0xFFFFFFFFFFFFFFFF


@functools.lru_cache(maxsize=None)
def _states() -> np.ndarray:
	"""The three far starts, TWO_HITS, the 5-move scramble, a state inside the ball, the solved state, one far start again."""
	rows = [_far(7), _far(8), _far(9), ball_model.apply(orc.SOLVED, TWO_HITS), ball_model.apply(orc.SOLVED, NEAR),
	        ball_model.apply(orc.SOLVED, INSIDE), orc.SOLVED.copy(), _far(8)]
	out = np.stack(rows + [_far(9)]).astype(np.int8)
	out.setflags(write=False)
	return out


DEEP = (0, 1, 2, 3, 7, 8)                                  # positions in _states() that deepening finishes, in rounds ...
ROUNDS = (2, 3, 4, 3, 3, 4)


def _batch(searches: int, pops: int, deepen: int = 4, **kw) -> DeviceSymBallSearchBatch:
	return DeviceSymBallSearchBatch(_ball(2), searches=searches, pops=pops, capacity=POOL, poll=64, deepen=deepen, **kw)


class Run:
	"""What a call left behind, copied: later calls on the same object must not change what a test compares with."""
	def __init__(self, b, solved, n):
		self.solved, self.status, self.lengths = solved.copy(), b.status.copy(), b.lengths.copy()
		self.queues = [list(b.action_queue_of(i)) for i in range(n)]
		self.arrays = [b.arrays(i) for i in range(n)] if b._arrays is not None else None
		self.deepened, self.probes = np.array(getattr(b, "deepened", np.zeros(n, np.int64))), getattr(b, "probes", 0)


@functools.lru_cache(maxsize=None)
def _plain_run(pops: int) -> Run:
	"""The states through the batch at deepen=0: what the pool phase gives every state (computed once per pops, never changed)."""
	b = _batch(4, pops, deepen=0)
	return Run(b, b.search(_states().copy(), keep_arrays=True), len(_states()))


@functools.lru_cache(maxsize=None)
def _bibfs_lengths() -> tuple:
	two = DeviceBiBFS(pops=256)
	out = []
	for s in _states():
		assert two.search(s.copy())
		out.append(len(two.action_queue))
	return tuple(out)


def _want(i: int):
	return _continued(_states()[i].tobytes())


def _assert_deepened(b, solved, i: int, want, start):
	assert solved[i] and want.result and list(b.action_queue_of(i)) == want.queue and b.lengths[i] == len(want.queue)
	assert b.deepened[i] == want.deepened
	assert b.sizes[i] == want.len and b.depths[i] == want.level
	assert b.stops[i] == 5 and b.capacity_exhausted[i] and b.meeting_depths[i] == -1 and b.meeting_nodes[i] == 0
	assert b.status[i, 0] == 1 and b.status[i, 1] == 0 and b.status[i, 6] == 0
	assert orc.is_solved(ball_model.apply(start, b.action_queue_of(i)))
	if b._arrays is not None:
		states, parents, actions = b.arrays(i)
		if states.ndim == 2:
			assert (states == want.states).all()
		assert (parents == want.parents).all() and (actions == want.actions).all()


def _assert_run(b, solved, order=None, arrays: bool = True):
	"""A call on _states() (or on its rows `order`) against the model, the deepen=0 batch and DeviceBiBFS."""
	order = list(range(len(_states()))) if order is None else list(order)
	plain = _plain_run(b.pops)
	assert solved.dtype == bool and solved.all() and (solved == (b.lengths >= 0)).all()
	assert b.deepened.dtype == np.int64 and b.deepened.shape == (len(order),)
	for k, i in enumerate(order):
		if i in DEEP:
			want = _want(i)
			assert want.deepened == ROUNDS[DEEP.index(i)] and want.frontier == (128, 1195) and want.level == 3
			_assert_deepened(b, solved, k, want, _states()[i])
			assert not plain.solved[i] and plain.status[i, 5] == 5          # (what deepening is for)
		else:
			assert b.deepened[k] == 0 and plain.solved[i]
			assert (b.status[k] == plain.status[i]).all() and b.lengths[k] == plain.lengths[i]
			assert list(b.action_queue_of(k)) == plain.queues[i]
			if arrays:
				for x, y in zip(b.arrays(k), plain.arrays[i]):
					assert x.shape == y.shape and (x == y).all()
		assert b.lengths[k] == _bibfs_lengths()[i]
	assert type(b.probes) is int and b.probes > 0


@pytest.mark.parametrize("searches, pops", ((1, 16), (3, 1), (8, 4096)))
def test_equal_to_the_model_and_to_the_single_agent(searches, pops):
	given = _states()
	assert [len(_want(i).queue) for i in DEEP] == [7, 8, 9, 8, 8, 9]
	b = _batch(searches, pops)
	with warnings.catch_warnings():
		warnings.simplefilter("error", CapacityExhausted)                # a state that deepening finishes raises no warning
		solved = b.search(given.copy(), keep_arrays=True)
	_assert_run(b, solved)
	# the single agent alone in a pool of the slot's size
	agent = DeviceSymBallSearch(_ball(2), pops=16, capacity=POOL, max_capacity=POOL, deepen=4)
	for i in DEEP[:4]:
		assert agent.search(given[i].copy())
		assert list(b.action_queue_of(i)) == list(agent.action_queue) and b.deepened[i] == agent.deepened
		assert (b.sizes[i], b.depths[i], b.popped[i]) == (len(agent), agent.depth, agent.popped)
		assert agent.capacity_exhausted and agent.meeting is None
		for x, y in zip(b.arrays(i), agent.arrays()):
			assert x.shape == y.shape and (x == y).all()


@pytest.mark.parametrize("cap", (3000, 500))
def test_the_division_of_the_cap_shows_nowhere(cap):
	b, ball = _batch(8, 64), _ball(2)
	seen, starts = [], set()                                             # the rounds the slots were in, launch by launch; the first words
	launch = b._deepen_launch

	def spy(h):
		seen.append(tuple(sorted(c[0] for c in b._deep.values())))
		starts.update(c[2] for c in b._deep.values())
		before = b.probes
		launch(h)
		assert b.probes - before <= cap
	b._deepen_launch = spy
	try:
		ball.deepen_cap = cap
		solved = b.search(_states().copy(), keep_arrays=True)
	finally:
		ball.deepen_cap = None
	_assert_run(b, solved)
	assert len(seen) > 1000                                              # a round of one slot took many launches
	assert any(first % 121 for first in starts)                          # word ranges start at ranks that are no multiple of 121
	print(f"cap {cap}: {len(seen)} launches, rounds in one launch {sorted(set(seen))[-3:]}, {b.probes} probes")


@pytest.mark.parametrize("cap", (None, 500))
def test_the_lowest_node_wins_over_a_lower_word(cap):
	start = ball_model.apply(orc.SOLVED, TWO_HITS)
	want = _continued(start.tobytes())
	frontier = np.arange(want.frontier[0], want.frontier[1] + 1)
	rank = model.lowest_hits(sym_ball(2), want.states[frontier - 1], want.actions[frontier - 1], want.deepened)
	later = (rank >= 0) & (rank < want.rank) & (frontier > want.node)
	assert want.deepened == 3 and later.any()                            # what this case was arranged for
	given = np.stack([_far(7), start, _far(8), _far(9)])
	b, ball = _batch(4, 64), _ball(2)
	try:
		ball.deepen_cap = cap
		solved = b.search(given.copy(), keep_arrays=True)
	finally:
		ball.deepen_cap = None
	for i, s in enumerate(given):
		_assert_deepened(b, solved, i, _continued(s.tobytes()), s)
	# the node and the word of the model: the own path to the node, then the word
	queue = list(b.action_queue_of(1))
	path, i = [], want.node
	while want.parents[i - 1]:
		path.append(int(want.actions[i - 1]))
		i = int(want.parents[i - 1])
	assert queue[:3] == path[::-1] and queue[3:6] == model.word_of(want.rank, 3, int(want.actions[want.node - 1]))


def test_refill_and_order():
	order = [2, 4, 5, 0, 6, 4, 3, 5, 1]                                  # deepened states among states the pool answers
	given = _states()[order]
	b, ball = _batch(2, 64), _ball(2)
	polls = []                                                           # (slots deepening, states the pool had answered) at every poll
	b.on_poll = lambda status: polls.append((len(b._deep), int((status[:, 1] != 0).sum())))
	seen, launch = set(), b._deepen_launch

	def spy(h):
		seen.add(tuple(sorted(c[0] for c in b._deep.values())))
		launch(h)
	b._deepen_launch = spy
	try:
		ball.deepen_cap = 3000                                           # the first state deepens over many polls
		solved = b.search(given.copy(), keep_arrays=True)
		_assert_run(b, solved, order)
		# a slot deepened while its neighbour finished pool searches and was refilled
		during = [won for deep, won in polls if deep >= 1]
		assert len(during) > 2 and during[-1] - during[0] >= 2
		assert any(len(set(rounds)) == 2 for rounds in seen)             # two slots in different rounds in one launch
		first = Run(b, solved, len(order))
		perm = np.random.RandomState(7).permutation(len(order))
		again = b.search(given[perm].copy(), keep_arrays=True)
	finally:
		ball.deepen_cap = None
	_assert_run(b, again, [order[p] for p in perm])
	for k, p in enumerate(perm):
		assert list(b.action_queue_of(k)) == first.queues[p] and b.deepened[k] == first.deepened[p] and b.lengths[k] == first.lengths[p]
		assert (b.status[k, [0, 1, 2, 4, 5, 6, 8, 9]] == first.status[p, [0, 1, 2, 4, 5, 6, 8, 9]]).all()      # (all but the iterations and the next pops)


def test_deepen_0_changes_nothing():
	given = _states()
	plain = _plain_run(16)
	absent = DeviceSymBallSearchBatch(_ball(2), searches=4, pops=16, capacity=POOL, poll=64)
	assert absent.deepen == 0
	deep = _batch(4, 16)
	assert deep.search(given.copy()).all()                              # a deepen=4 call on the same ball in between
	for b in (absent, _batch(4, 16, deepen=0)):
		solved = b.search(given.copy(), keep_arrays=True)
		assert (solved == (b.status[:, 1] != 0)).all() and (solved == plain.solved).all()
		assert (b.status == plain.status).all() and (b.lengths == plain.lengths).all()
		assert [list(b.action_queue_of(i)) for i in range(len(given))] == plain.queues
		assert (b.deepened == 0).all() and b.probes == 0
	for i in DEEP:                                                       # the far starts: unsolved, pool full, today's rule
		assert not plain.solved[i] and plain.status[i, 5] == 5 and plain.lengths[i] == -1 and plain.queues[i] == []
		assert POOL - 12 * 16 < plain.status[i, 2] <= POOL and plain.status[i, 8] == 3       # stopped before 16 pops that might not fit
		assert plain.status[i, 2] < _want(i).len                         # (the clipped rule goes further)


def test_too_few_rounds():
	six = ball_model.apply(orc.SOLVED, np.random.RandomState(SIX[0]).randint(0, 12, SIX[1]))
	want = model.continue_from_frontier(six, sym_ball(2), POOL, 1)
	assert want.result and want.deepened == 1 and len(want.queue) == 6 and want.level == 3
	given = np.stack([_far(8), six, _far(9), ball_model.apply(orc.SOLVED, NEAR), _far(7), orc.SOLVED])
	b = _batch(3, 64, deepen=1)
	solved = b.search(given.copy(), keep_arrays=True)
	assert solved.tolist() == [False, True, False, True, False, True]
	for i in (0, 2, 4):                                                  # round 1 has no hit: as today, with the pool of pops = 1
		far = _continued(given[i].tobytes())
		assert b.stops[i] == 5 and b.deepened[i] == 0 and b.lengths[i] == -1 and list(b.action_queue_of(i)) == []
		assert b.sizes[i] == far.len and b.depths[i] == far.level and b.capacity_exhausted[i]
		assert (b.arrays(i)[0] == far.states).all()
	_assert_deepened(b, solved, 1, want, six)
	assert b.probes >= 3 * 1068 * 11 + (want.node - 127) * 11           # whole rounds of the far starts, and up to the node that hit
	plain = _plain_run(64)
	for i, at in ((3, 4), (5, 6)):                                       # the other states are undisturbed
		assert (b.status[i] == plain.status[at]).all() and list(b.action_queue_of(i)) == plain.queues[at] and b.deepened[i] == 0


def test_a_budget_stop_is_not_deepened():
	b = _batch(2, 16)
	solved = b.search(_far(8)[None].copy(), max_states=500, keep_arrays=True)
	assert not solved[0] and b.stops[0] == 2 and b.deepened[0] == 0 and b.probes == 0 and 500 <= b.sizes[0] < 512
	assert not b.capacity_exhausted[0] and list(b.action_queue_of(0)) == []
	# one budget per state: the stopped search beside deepened neighbours
	given = np.stack([_far(7), _far(8), _far(9)])
	solved = b.search(given.copy(), max_states=np.array([10 ** 9, 500, 10 ** 9]), keep_arrays=True)
	assert solved.tolist() == [True, False, True] and b.stops.tolist() == [5, 2, 5] and b.deepened.tolist() == [2, 0, 4]
	for i in (0, 2):
		_assert_deepened(b, solved, i, _continued(given[i].tobytes()), given[i])


def test_the_time_limit(monkeypatch):
	b = _batch(8, 64)
	with warnings.catch_warnings():
		warnings.simplefilter("error")
		solved = b.search(_states().copy(), time_limit=1e-9, keep_arrays=True)
	assert solved.shape == (9,) and not solved.any() and (b.lengths == -1).all() and (b.deepened == 0).all()
	# out of time in the rounds: the clock jumps behind the first probe launch; the slot that deepens comes back unsolved and is
	# put to rest, the state the pool answered in the meantime is kept
	calls, jump = [], [0.0]
	launch, real = b._deepen_launch, agents.time.perf_counter

	def late(h):
		launch(h)
		calls.append(1)
		jump[0] = 1e6
	b._deepen_launch = late
	monkeypatch.setattr(agents.time, "perf_counter", lambda: real() + jump[0])
	try:
		with warnings.catch_warnings():
			warnings.simplefilter("error")
			solved = b.search(np.stack([_far(9), ball_model.apply(orc.SOLVED, NEAR)]).copy(), time_limit=1e5)
	finally:
		monkeypatch.undo()
		b._deepen_launch = launch
	assert len(calls) == 1 and solved.tolist() == [False, True] and b.deepened.tolist() == [0, 0] and b.stops.tolist() == [5, 1]
	assert b.probes == 1068 * 11 and not b._deep
	# the engine is as usable as before
	_assert_run(b, b.search(_states().copy(), keep_arrays=True))


def test_686_states():
	given = _states().copy()
	_plain_run(64), _bibfs_lengths()                                     # (the references are made on 20-byte states)
	try:
		cube.set_is2024(False)
		b = _batch(3, 64)
		solved = b.search(np.asarray(cube.as686(given)).reshape(len(given), 6, 8, 6), keep_arrays=True)
		_assert_run(b, solved, arrays=False)
		for i in range(len(given)):
			states = b.arrays(i)[0]
			assert states.shape == (b.sizes[i], 6, 8, 6)
			want = _want(i).states if i in DEEP else _plain_run(64).arrays[i][0]
			assert (states == np.asarray(cube.as686(want)).reshape(len(want), 6, 8, 6)).all()
	finally:
		cube.set_is2024(True)


def test_error_paths_of_the_entries():
	lib, stream, ball = _ffi.lib(), _ffi.stream_ptr(), _ball(2)
	h = C.c_void_p()
	_ffi.check(lib.rk_ssearchb_create(C.byref(h), ball._h, 3, POOL, 16))
	try:
		want = _continued(_far(7).tobytes())
		st, level, keys = np.zeros((3, 10), np.int64), np.zeros((3, 2), np.int64), np.zeros(3, np.uint64)
		out = np.zeros((3, 17), np.int32)

		def probe(*jobs, n=None):
			rows = np.array(jobs, np.uint32).reshape(-1, 8)
			return lib.rk_sdeepenb_probe(h, len(rows) if n is None else n, rows.ctypes.data, stream)

		def paths(slots, nodes, extras, ranks, max_len=16, n=None):
			cols = [np.array(c, t) for c, t in ((slots, np.int32), (nodes, np.int64), (extras, np.int32), (ranks, np.uint32))]
			return lib.rk_sdeepenb_paths(h, len(slots) if n is None else n, *(c.ctypes.data for c in cols), out.ctypes.data, max_len, stream)

		def refused(code, got, text):
			assert got == code and lib.rk_last_error().startswith(text.encode()), (got, lib.rk_last_error())
		_ffi.check(lib.rk_sdeepenb_set(h, 1))
		slots, budgets = np.array([1, 0], np.int32), np.full(2, 10 ** 10, np.int64)
		given = np.ascontiguousarray(np.stack([_far(7), _far(8)]))
		_ffi.check(lib.rk_ssearchb_reset(h, 2, slots.ctypes.data, given.ctypes.data, budgets.ctypes.data, stream))
		_ffi.check(lib.rk_ssearchb_run(h, 64, stream))
		_ffi.check(lib.rk_ssearchb_status(h, st.ctypes.data, stream))
		assert st[:2, 5].tolist() == [5, 5] and st[:2, 2].tolist() == [want.len, want.len] and not st[2].any()
		# the engine has not read the frontiers yet
		refused(-4, probe((1, 1, 128, 8, 0, 11, 1, 0)), "rk_sdeepenb_probe: slot 1 had not stopped")
		refused(-4, paths([1], [128], [1], [0]), "rk_sdeepenb_paths: slot 1 had not stopped")
		_ffi.check(lib.rk_sdeepenb_frontiers(h, level.ctypes.data, stream))
		assert level.tolist() == [[128, 1195], [128, 1195], [0, 0]]
		# a job outside the slot's frontier, or outside the words of its round
		for job in ((1, 1, 127, 8, 0, 11, 1, 0), (1, 1, 1196, 1, 0, 11, 1, 0), (1, 1, 1190, 7, 0, 11, 1, 0), (1, 1, 128, 0, 0, 11, 1, 0),
		            (1, 1, 128, 1069, 0, 11, 1, 0), (1, 1, 128, 8, 0, 12, 1, 0), (1, 1, 128, 8, 11, 1, 1, 0), (1, 1, 128, 8, 0, 0, 1, 0),
		            (1, 3, 128, 1, 1331, 1, 1, 0), (1, 2, 128, 1, 120, 2, 1, 0)):
			refused(-1, probe(job), "rk_sdeepenb_probe: ")
		refused(-1, probe((1, 1, 128, 8, 0, 11, 1, 0), (1, 2, 128, 8, 0, 121, 1, 0)), "rk_sdeepenb_probe: slot 1 is named twice")
		for extra in (0, 9):
			refused(-1, probe((1, extra, 128, 8, 0, 11, 1, 0)), "rk_sdeepenb_probe: extra")
		refused(-1, probe((3, 1, 128, 8, 0, 11, 1, 0)), "rk_sdeepenb_probe: slot 3 outside")
		# more than 2^28 probes: 1 068 nodes x 11^6 words, and two jobs that pass it together
		refused(-1, probe((1, 6, 128, 1068, 0, 11 ** 6, 1, 0)), "rk_sdeepenb_probe: more than")
		refused(-1, probe((1, 6, 128, 100, 0, 11 ** 6, 1, 0), (0, 6, 128, 100, 0, 11 ** 6, 1, 0)), "rk_sdeepenb_probe: more than")
		refused(-1, lib.rk_sdeepenb_probe(h, 1, None, stream), "rk_sdeepenb_probe: null jobs")
		refused(-1, probe((1, 1, 128, 8, 0, 11, 1, 0), n=4), "rk_sdeepenb_probe: 4 jobs")
		refused(-1, probe((1, 1, 128, 8, 0, 11, 1, 0), n=-1), "rk_sdeepenb_probe: -1 jobs")
		refused(-4, probe((2, 1, 1, 1, 0, 12, 1, 0)), "rk_sdeepenb_probe: slot 2 had not stopped")      # never started
		refused(-4, probe((1, 1, 128, 8, 0, 11, 0, 0)), "rk_sdeepenb_probe: the first job of slot 1")    # no round was started
		assert lib.rk_sdeepenb_probe(h, 0, None, stream) == 0
		refused(-1, lib.rk_sdeepenb_keys(h, None, stream), "rk_sdeepenb_keys: null")
		refused(-1, lib.rk_sdeepenb_frontiers(h, None, stream), "rk_sdeepenb_frontiers: null")
		refused(-1, paths([1], [0], [1], [0]), "rk_sdeepenb_paths: node 0")
		refused(-1, paths([1], [want.len + 1], [1], [0]), "rk_sdeepenb_paths: node")
		refused(-1, paths([1], [128], [9], [0]), "rk_sdeepenb_paths: extra 9")
		refused(-1, paths([1], [128], [0], [0]), "rk_sdeepenb_paths: extra 0")
		refused(-1, paths([3], [128], [1], [0]), "rk_sdeepenb_paths: slot 3")
		refused(-1, paths([1], [128], [1], [0], max_len=4097), "rk_sdeepenb_paths: max_len")
		refused(-1, paths([1, 0, 1, 0], [128] * 4, [1] * 4, [0] * 4), "rk_sdeepenb_paths: 4 rows")
		refused(-1, lib.rk_sdeepenb_paths(h, 1, None, None, None, None, out.ctypes.data, 16, stream), "rk_sdeepenb_paths: null")
		refused(-1, lib.rk_sdeepenb_paths(h, 1, slots.ctypes.data, budgets.ctypes.data, slots.ctypes.data, slots.ctypes.data, None, 16, stream),
		        "rk_sdeepenb_paths: null")
		# none of them launched: every key is "none"
		_ffi.check(lib.rk_sdeepenb_keys(h, keys.ctypes.data, stream))
		assert (keys == KEY_NONE).all()
		# the rounds through the C ABI alone: round 1 of both slots has no hit, round 2 of slot 1 in two launches, round 2 of slot 0 has none
		assert probe((1, 1, 128, 1068, 0, 11, 1, 0), (0, 1, 128, 1068, 0, 11, 1, 0)) == 0
		_ffi.check(lib.rk_sdeepenb_keys(h, keys.ctypes.data, stream))
		assert (keys == KEY_NONE).all()
		assert probe((0, 2, 128, 1068, 0, 121, 1, 0), (1, 2, 128, 500, 0, 121, 1, 0)) == 0
		assert probe((1, 2, 628, 568, 0, 121, 0, 0)) == 0
		_ffi.check(lib.rk_sdeepenb_keys(h, keys.ctypes.data, stream))
		assert keys.tolist() == [KEY_NONE, want.node << 32 | want.rank, KEY_NONE]
		assert paths([1], [want.node], [2], [want.rank]) == 0
		assert out[0, 0] == 7 and out[0, 1:8].tolist() == want.queue
		assert paths([1, 1], [want.node, 128], [2, 1], [want.rank + 121, 0]) == 0
		assert out[:2, 0].tolist() == [-1, -2]                           # no such word; a word that does not lead into the ball
		# a reset forgets the slot's frontier
		_ffi.check(lib.rk_ssearchb_reset(h, 1, slots.ctypes.data, given.ctypes.data, budgets.ctypes.data, stream))
		refused(-4, probe((1, 2, 628, 568, 0, 121, 0, 0)), "rk_sdeepenb_probe: slot 1 had not stopped")
	finally:
		assert lib.rk_ssearchb_destroy(h) == 0
