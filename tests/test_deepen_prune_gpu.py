"""
The probes past the symmetry ball pruned by pattern databases, on the GPU (engines rk_bound_*, rk_sdeepen_pruned and
rk_sdeepen_nodes_pruned), balls of radius 2 and 3 and the three small databases of tests/deepen_prune_model.py.
  * `DevicePatternBound.depth` against `DevicePatternDB.lower_bound` and the NumPy model: n of 0, 1, 255, 256, 257 and one past the
    capped grid, rows that one database answers -1;
  * `solve_beyond(prune=)`: lengths and actions array for array those of the unpruned call and of tests/deepen_model.py, words of
    1..4 moves, with and without last actions, n of 1, 63, 64, 65 and 130, the launch cap lowered into the middle of an item;
  * the look-ups of rounds in which nothing hits, EXACTLY the model's surviving words, and fewer than the words issued; a bound
    that cannot cut anything makes as many look-ups as there are words;
  * `DeviceSymBallSearch(deepen=E, prune=)`: the queue, `deepened` and `probes` of the search without `prune` and of the model;
  * the error paths, and both new launches on a side stream behind a gate.
Nothing here provokes a fault: every table read is behind the engine's own guards and wrong arguments are refused on the host.
"""
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, gpu
from librubiks_amd.solving.agents import DevicePatternBound, DevicePatternDB, DeviceSymBall, DeviceSymBallSearch
from tests import ball_model
from tests import deepen_model
from tests import deepen_prune_model as model
from tests import side_stream as S
from tests.test_deepen_cpu import sym_ball

pytestmark = pytest.mark.gpu

orc = ball_model.orc
NAMES = ("cross", "corners3", "mixed")
POOL = 1_500                                       # the own levels 0..3 of a far start hold 1 195 states, level 4 does not fit
_balls = {}


def _ball(radius: int) -> DeviceSymBall:
	if radius not in _balls:
		_balls[radius] = DeviceSymBall(radius).build()
	return _balls[radius]


@functools.lru_cache(maxsize=None)
def _db(name: str) -> DevicePatternDB:
	return DevicePatternDB(*model.PATTERNS[name]).build()


@functools.lru_cache(maxsize=None)
def _bound(names=NAMES) -> DevicePatternBound:
	return DevicePatternBound([_db(n) for n in names])


def _walks(n: int, moves, seed: int):
	"""(states, last actions): n seeded walks from solved without a turn straight back, walk i of moves[i % len(moves)] moves"""
	rng = np.random.RandomState(seed)
	states, last = np.empty((n, 20), np.int8), np.empty(n, np.int64)
	for i in range(n):
		word = []
		while len(word) < moves[i % len(moves)]:
			a = int(rng.randint(12))
			if not word or a != (word[-1] ^ 1):
				word.append(a)
		states[i], last[i] = ball_model.apply(orc.SOLVED, word), word[-1]
	return states, last


# ---- the bound ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base():
	"""(4 096 states 0..20 moves deep with two rows that one database refuses, the model's depths of them)"""
	base = S.mixed_depths(4096, 20, 28_001)
	base[1, 8 + model.CROSS_D[0]] = 24                                   # a selected code of 24: the cross answers -1
	base[2, 1] = base[2, 0]                                              # corners 0 and 1 on one position: corners3 answers -1
	return base, model.depths(model.tables(NAMES), base)


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, DevicePatternDB.GRID_ROWS + 300))
def test_bound_depth_is_lower_bound_in_one_launch(n):
	base, depth = _base()
	rows = np.arange(n) % len(base)
	states, want = base[rows], depth[rows]
	bound, dbs = _bound(), [_db(name) for name in NAMES]
	got = bound.depth(states)
	assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (n,)
	assert (got == want).all() and (got == DevicePatternDB.lower_bound(states, dbs)).all()
	q = torch.from_numpy(states).to(gpu)
	dev = bound.depth(q)
	assert isinstance(dev, torch.Tensor) and dev.dtype == torch.int32 and dev.is_cuda and (dev.cpu().numpy() == want).all()
	assert torch.equal(dev, DevicePatternDB.lower_bound(q, dbs))
	if n > 2:                                                            # a database that answers -1 does not spoil the others' maximum
		assert _db("cross").depth(states[1:2])[0] == -1 and _db("corners3").depth(states[2:3])[0] == -1
		assert got[1] >= 0 and got[2] >= 0 and got[1] == max(db.depth(states[1:2])[0] for db in dbs)
		alone = DevicePatternBound([_db("cross")]).depth(states[:3])
		assert alone[1] == -1 and (alone == _db("cross").depth(states[:3])).all()        # -1 where every database answers -1


# ---- solve_beyond ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _far_walks(radius: int):
	"""130 walks of radius + 1 .. radius + 4 moves and the moves they ended with"""
	return _walks(130, (radius + 1, radius + 2, radius + 3, radius + 4), 40 + radius)


@functools.lru_cache(maxsize=None)
def _want(radius: int, extra: int, with_last: bool):
	states, last = _far_walks(radius)
	return deepen_model.solve_beyond(sym_ball(radius), states, extra, last if with_last else None)


@pytest.mark.parametrize("extra", (1, 2, 3, 4))
@pytest.mark.parametrize("radius", (2, 3))
def test_pruned_solve_beyond_is_the_unpruned_one_and_the_model(radius, extra):
	ball, bound = _ball(radius), _bound()
	states, last = _far_walks(radius)
	for with_last in (False, True):
		kw = {"last_actions": last} if with_last else {}
		want_len, want_act = _want(radius, extra, with_last)
		plain_len, plain_act = ball.solve_beyond(states, extra, **kw)
		plain = (ball.probes, ball.lookups)
		lengths, actions = ball.solve_beyond(states, extra, prune=bound, **kw)
		print(f"radius {radius} extra {extra} last {with_last}: probes {ball.probes}, look-ups {ball.lookups}; unpruned {plain}")
		assert lengths.dtype == np.int64 and actions.shape == (len(states), extra + radius)
		assert (lengths == plain_len).all() and (actions == plain_act).all()
		assert (lengths == want_len).all() and (actions == want_act).all()
		assert plain[0] == plain[1] == ball.probes and 0 < ball.lookups <= ball.probes
	assert (want_len >= 0).any() and ((want_len < 0).any() or extra == 4)
	# a list of databases is wrapped into a bound
	listed_len, listed_act = ball.solve_beyond(states, extra, prune=[_db("cross"), _db("mixed")])
	free_len, free_act = _want(radius, extra, False)
	assert (listed_len == free_len).all() and (listed_act == free_act).all()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_pruned_solve_beyond_batch_sizes_and_a_split_item(n):
	ball, bound = _ball(2), _bound()
	states = _far_walks(2)[0][:n]
	want_len, want_act = _want(2, 3, False)
	lengths, actions = ball.solve_beyond(states, 3, prune=bound)
	assert (lengths == want_len[:n]).all() and (actions == want_act[:n]).all()
	try:                                                                 # a state's 1 584 words of round 3 in ranges of 500 and less: no multiple of 121
		ball.deepen_cap = 500
		split_len, split_act = ball.solve_beyond(states, 3, prune=bound)
	finally:
		ball.deepen_cap = None
	assert (split_len == want_len[:n]).all() and (split_act == want_act[:n]).all()


def test_distance_and_path_take_prune():
	ball, bound = _ball(2), _bound()
	a, _ = _walks(64, (3, 4, 5), 5)
	b, _ = _walks(64, (1, 2), 6)
	plain_len, plain_act = ball.path(a, b, extra=3)
	lengths, actions = ball.path(a, b, extra=3, prune=bound)
	assert (lengths == plain_len).all() and (actions == plain_act).all() and ball.lookups <= ball.probes
	assert (ball.distance(a, b, extra=3, prune=bound) == plain_len).all() and (plain_len > 2).any()


# ---- the look-ups ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _out_of_reach(radius: int, extra: int):
	"""(40 states one move farther out than `extra` reaches, the moves that led to them): walks of radius + extra + 1 moves that the
	model finds no word of 1..extra moves for"""
	states, last = _walks(160, (radius + extra + 1,), 90 + 10 * radius + extra)
	far = np.nonzero(deepen_model.solve_beyond(sym_ball(radius), states, extra)[0] == -1)[0][:40]
	assert len(far) == 40
	return states[far], last[far]


@pytest.mark.parametrize("names", (NAMES, ("corners3",)))
@pytest.mark.parametrize("extra", (1, 2, 3, 4))
@pytest.mark.parametrize("radius", (2, 3))
def test_lookups_without_a_hit_are_the_models_surviving_words(radius, extra, names):
	ball, bound, tabs = _ball(radius), _bound(names), model.tables(names)
	states, ended = _out_of_reach(radius, extra)
	for with_last in (False, True):
		last = ended if with_last else np.full(len(states), -1, np.int64)
		kw = {"last_actions": last} if with_last else {}
		assert (deepen_model.solve_beyond(sym_ball(radius), states, extra, last)[0] == -1).all()      # no hit, says the model
		want = sum(int(model.surviving_words(radius, tabs, states, last, e).sum()) for e in range(1, extra + 1))
		issued = sum(len(states) * deepen_model.word_count(e, 0 if with_last else -1) for e in range(1, extra + 1))
		lengths, _ = ball.solve_beyond(states, extra, prune=bound, **kw)
		print(f"radius {radius} extra {extra} last {with_last}: {ball.lookups} look-ups of {ball.probes} words, the model says {want}")
		assert (lengths == -1).all() and ball.probes == issued
		assert ball.lookups == want and ball.lookups < ball.probes
		plain, _ = ball.solve_beyond(states, extra, **kw)
		assert (plain == -1).all() and ball.lookups == ball.probes == issued
		try:                                                             # the same words in launches that split items
			ball.deepen_cap = 500
			ball.solve_beyond(states, extra, prune=bound, **kw)
		finally:
			ball.deepen_cap = None
		assert ball.lookups == want and ball.probes == issued


def test_a_bound_that_cannot_cut_makes_every_lookup():
	"""The three corners at home, every other cubie scrambled: the pattern's entry is 0 there and at most k after k moves, which is
	never above radius + (moves left) while the words are no longer than the radius."""
	p, table = model.table("corners3")
	far, _ = _walks(60, (20,), 17)
	_, word = p.solve(table, far, int(table.max()))
	states = np.array([ball_model.apply(s, w[w >= 0]) for s, w in zip(far, word)], np.int8)
	assert (p.depth(table, states) == 0).all()
	ball, bound = _ball(2), _bound(("corners3",))
	assert (deepen_model.solve_beyond(sym_ball(2), states, 2)[0] == -1).all()              # a round without a hit
	nobody = np.full(len(states), -1, np.int64)
	assert all((model.surviving_words(2, [(p, table)], states, nobody, e) == deepen_model.word_count(e)).all() for e in (1, 2))
	lengths, _ = ball.solve_beyond(states, 2, prune=bound)
	assert (lengths == -1).all() and ball.lookups == ball.probes == len(states) * (12 + 132)


# ---- DeviceSymBallSearch(deepen=E, prune=) --------------------------------------------------------------------------------
#: starts 7, 8 and 9 quarter turns from solved: (seed, moves) of a seeded scramble
FAR = {7: (3, 9), 8: (3, 10), 9: (0, 9)}


@functools.lru_cache(maxsize=None)
def _continued(length: int):
	seed, moves = FAR[length]
	start = ball_model.apply(orc.SOLVED, np.random.RandomState(seed).randint(0, 12, moves))
	return start, deepen_model.continue_from_frontier(start, sym_ball(3), POOL, 4)


@pytest.mark.parametrize("length", (7, 8, 9))
def test_pruned_deepened_search_is_the_unpruned_one_and_the_model(length):
	start, want = _continued(length)
	assert want.result and want.deepened == length - 3 - 3 and len(want.queue) == length and want.frontier == (128, 1195)
	for pops, chunk in ((16, None), (4096, 3), (16, 100)):
		runs = []
		for prune in (None, _bound()):
			agent = DeviceSymBallSearch(_ball(3), pops=pops, capacity=POOL, max_capacity=POOL, poll=64, deepen=4, prune=prune)
			agent.deepen_chunk = chunk
			assert agent.search(start.copy()) and orc.is_solved(ball_model.apply(start, agent.action_queue))
			runs.append((list(agent.action_queue), agent.deepened, agent.probes, len(agent), agent.depth, agent.lookups))
		print(f"length {length} pops {pops} chunk {chunk}: probes {runs[1][2]}, look-ups {runs[1][5]}")
		assert runs[0][:5] == runs[1][:5] and runs[0][5] == runs[0][2] and 0 < runs[1][5] <= runs[1][2]
		assert runs[1][0] == want.queue and runs[1][1] == want.deepened and runs[1][3] == want.len and runs[1][4] == want.level


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_error_paths():
	fresh = DevicePatternDB(corners=(5,))
	assert not fresh.built
	bound = DevicePatternBound([fresh, _db("cross")])                     # an unbuilt database gets built
	assert fresh.built and bound.dbs == (fresh, _db("cross"))
	states = _far_walks(2)[0][:8]
	assert (bound.depth(states) == DevicePatternDB.lower_bound(states, [fresh, _db("cross")])).all()
	for bad in ([], [fresh] * 2, [_db("cross"), _db("mixed"), _db("corners3"), fresh, DevicePatternDB(edges=(3,))], [fresh, None]):
		with pytest.raises(ValueError):
			DevicePatternBound(bad)
	ball = _ball(2)
	with pytest.raises(ValueError):
		DeviceSymBallSearch(ball, prune=bound)                                # prune needs deepen > 0
	with pytest.raises(ValueError):
		ball.solve_beyond(states, 2, prune="cross")
	# a freed bound, and a bound whose database was freed: refused on the host, nothing is launched
	lib, calls = _ffi.lib(), []
	entries = {name: getattr(lib, name) for name in ("rk_sdeepen_pruned", "rk_sdeepen", "rk_symball_solve", "rk_bound_depth")}
	try:
		for name, entry in entries.items():
			setattr(lib, name, lambda *args, _name=name, _entry=entry: calls.append(_name) or _entry(*args))
		bound._free()
		with pytest.raises(ValueError):
			ball.solve_beyond(states, 2, prune=bound)
		with pytest.raises(ValueError):
			bound.depth(states)
		other = DevicePatternBound([fresh])
		fresh._free()
		with pytest.raises(ValueError):
			ball.solve_beyond(states, 2, prune=other)
		agent = DeviceSymBallSearch(ball, deepen=2, prune=other)
		with pytest.raises(ValueError):
			agent.search(states[0].copy())
		assert calls == []
	finally:
		for name, entry in entries.items():
			setattr(lib, name, entry)
	# the entries' own checks: a null bound, a counter that is not 8-byte aligned
	q = torch.from_numpy(states).to(gpu)
	best = torch.full((8,), -1, dtype=torch.int32, device=gpu)
	looked = torch.zeros(2, dtype=torch.int64, device=gpu)
	live = _bound()
	assert lib.rk_sdeepen_pruned(ball._h, None, q.data_ptr(), None, 8, 1, 0, 12, best.data_ptr(), looked.data_ptr(), None) == -1
	assert lib.rk_sdeepen_pruned(ball._h, live._h, q.data_ptr(), None, 8, 1, 0, 12, best.data_ptr(), looked.data_ptr() + 4, None) == -1
	assert lib.rk_sdeepen_pruned(ball._h, live._h, q.data_ptr(), None, 8, 9, 0, 12, best.data_ptr(), looked.data_ptr(), None) == -1
	assert lib.rk_sdeepen_pruned(ball._h, live._h, q.data_ptr(), None, 8, 1, 0, 12, best.data_ptr(), None, _ffi.stream_ptr()) == 0     # not counted
	torch.cuda.synchronize()
	assert looked.tolist() == [0, 0]


# ---- a side stream ----------------------------------------------------------------------------------------------------------
def test_bound_depth_and_a_pruned_round_on_a_side_stream():
	"""Pattern A of tests/side_stream.py: the inputs arrive and the outputs are initialised BEHIND the gate, so a launch sent to
	stream 0 runs during the gate on the decoy states and is overwritten, or shows in the bits."""
	N, extra, words = 256, 2, 132
	lib, ball, bound = _ffi.lib(), _ball(2), _bound()
	true = torch.from_numpy(np.concatenate([_far_walks(2)[0], _out_of_reach(2, 2)[0], _far_walks(3)[0]])[:N].copy()).to(gpu)
	decoy = torch.from_numpy(S.mixed_depths(N, 6, 28_002)).to(gpu)

	def run(q, out):
		depth, best, looked = out
		st = _ffi.stream_ptr()
		best.fill_(-1)
		looked.zero_()
		_ffi.check(lib.rk_bound_depth(bound._h, q.data_ptr(), N, depth.data_ptr(), st))
		_ffi.check(lib.rk_sdeepen_pruned(ball._h, bound._h, q.data_ptr(), None, N, extra, 0, words, best.data_ptr(), looked.data_ptr(), st))

	def outputs():
		return [S.sentinel((N,), torch.int32), S.sentinel((N,), torch.int32), S.sentinel((1,), torch.int64)]
	want, other = outputs(), outputs()
	run(true, want)
	run(decoy, other)
	torch.cuda.synchronize()
	s = S.side_stream()
	got, buf = outputs(), decoy.clone()
	torch.cuda.synchronize()
	s.wait_stream(torch.cuda.default_stream())
	with torch.cuda.stream(s):
		ev = S.gate(s)
		buf.copy_(true, non_blocking=True)
		run(buf, got)
		S.held(ev)
		s.synchronize()
	assert S.same_bits(got[0], want[0]) and S.same_bits(got[1], want[1])
	assert not S.same_bits(other[0], want[0]) and not S.same_bits(other[1], want[1])     # a launch that read the decoy would have shown
	rank = want[1].cpu().numpy().view(np.uint32)
	assert (rank != 0xFFFFFFFF).any() and (rank == 0xFFFFFFFF).any()
	assert 0 < int(got[2]) <= N * words and 0 < int(want[2]) <= N * words                # (with hits the count depends on the schedule)
