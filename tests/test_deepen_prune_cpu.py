"""
Pruning the probes past the symmetry ball by pattern databases, without a GPU: the argument that no answer changes, exercised on
the NumPy models (tests/deepen_prune_model.py over tests/deepen_model.py and tests/pdb_model.py), and the host-side checks of the
new entries and arguments.
  * on a radius-2 ball, for 200 seeded scrambles of 3..6 moves and words of 1..4 moves: every lowest word that hits the ball
    survives the cuts (no prefix of it has a bound above radius + moves left), with and without last actions;
  * the words that survive are at most the words there are, and strictly fewer in some case;
  * the bound is admissible on those states: never above the breadth-first distance;
  * rk_bound_* and the pruned entries refuse null arguments, and the agents check `prune`.
"""
import ctypes as C

import numpy as np
import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DevicePatternBound, DevicePatternDB, DeviceSymBall, DeviceSymBallSearch
from tests import ball_model
from tests import deepen_model
from tests import deepen_prune_model as model
from tests.test_deepen_cpu import plain_ball, sym_ball

orc = ball_model.orc
RADIUS = 2
NAMES = ("cross", "corners3", "mixed")


def _scrambles(n: int, seed: int):
	"""(states, last actions): n seeded scrambles of 3..6 moves without a turn straight back, and the move each ended with"""
	rng = np.random.RandomState(seed)
	states, last = np.empty((n, 20), np.int8), np.empty(n, np.int64)
	for i in range(n):
		word = []
		while len(word) < 3 + i % 4:
			a = int(rng.randint(12))
			if not word or a != (word[-1] ^ 1):
				word.append(a)
		states[i], last[i] = ball_model.apply(orc.SOLVED, word), word[-1]
	return states, last


def test_the_bound_is_admissible():
	tabs = model.tables(NAMES)
	ball = plain_ball(5)
	pick = np.random.RandomState(1).choice(ball.len, 4000, replace=False)
	depth = np.searchsorted(np.asarray(ball.level_start[1:]) - 1, pick, side="right")      # the level of row `pick` of the ball's states
	got = model.bound(tabs, ball.states[pick])
	assert (got <= depth).all() and (got == depth).any() and got.max() >= 4
	assert (model.depths(tabs, ball.states[pick]) == got).all()                              # legal states: every table has an entry


@pytest.mark.parametrize("with_last", (False, True))
def test_every_hit_word_survives_and_some_words_do_not(with_last):
	tabs, ball = model.tables(NAMES), sym_ball(RADIUS)
	states, ended = _scrambles(200, 7)
	last = ended if with_last else np.full(len(states), -1, np.int64)
	hits = fewer = 0
	for extra in (1, 2, 3, 4):
		rows = np.arange(len(states))[(np.arange(len(states)) % 4) == extra - 1] if extra == 4 else np.arange(len(states))
		s, l = states[rows], last[rows]
		rank = deepen_model.lowest_hits(ball, s, l, extra)
		for i in np.nonzero(rank >= 0)[0]:
			assert model.word_survives(RADIUS, tabs, s[i], int(l[i]), int(rank[i]), extra), (extra, int(rows[i]), int(rank[i]))
			hits += 1
		left = model.surviving_words(RADIUS, tabs, s, l, extra)
		words = np.array([deepen_model.word_count(extra, int(v)) for v in l])
		assert (left >= 0).all() and (left <= words).all()
		assert (left[rank >= 0] >= 1).all()                                                  # at least the word that hits
		fewer += int((left < words).sum())
	assert hits > 0 and fewer > 0                                                   # otherwise this shows nothing


def test_a_table_without_an_entry_counts_zero():
	tabs = model.tables(NAMES)
	states = _scrambles(8, 3)[0]
	states[1, 8 + model.CROSS_D[0]] = 24                                                     # a selected code of 24: no entry in the cross
	states[2, 1] = states[2, 0]                                                              # two selected corners on one position
	assert model.depths([tabs[0]], states)[1] == -1 and model.depths([tabs[1]], states)[2] == -1
	want = model.depths(tabs, states)
	assert (want >= 0).all() and (model.bound(tabs, states) == want).all()                   # the other tables still answer
	assert model.bound([tabs[0]], states)[1] == 0 and model.bound([tabs[1]], states)[2] == 0


def test_entries_refuse_null_arguments_and_agents_check_prune():
	lib = _ffi.lib()
	h = C.c_void_p()
	assert lib.rk_bound_create(None, None, 1) == -1 and lib.rk_bound_create(C.byref(h), None, 1) == -1
	for n in (0, 5, -1):
		assert lib.rk_bound_create(C.byref(h), None, n) == -1 and b"outside 1..4" in lib.rk_last_error()
	nulls = (C.c_void_p * 2)()
	assert lib.rk_bound_create(C.byref(h), nulls, 2) == -1 and b"null" in lib.rk_last_error()
	db = C.c_void_p()
	corners = np.array([0], np.uint8)
	_ffi.check(lib.rk_pdb_create(C.byref(db), corners.ctypes.data, 1, None, 0))
	try:
		assert lib.rk_bound_create(C.byref(h), (C.c_void_p * 2)(db.value, db.value), 2) == -1 and b"the same" in lib.rk_last_error()
		assert lib.rk_bound_create(C.byref(h), (C.c_void_p * 1)(db.value), 1) == -4 and b"build" in lib.rk_last_error()
	finally:
		lib.rk_pdb_destroy(db)
	assert h.value is None and lib.rk_bound_destroy(None) == 0
	assert lib.rk_bound_depth(None, None, 0, None, None) == -1
	assert lib.rk_sdeepen_pruned(None, None, None, None, 0, 1, 0, 1, None, None, None) == -1 and b"null bound" in lib.rk_last_error()
	assert lib.rk_sdeepen_nodes_pruned(None, None, 1, 1, 1, 0, 1, None, None, None) == -1 and b"null bound" in lib.rk_last_error()
	cross = DevicePatternDB.cross("D")
	for bad in ([], [cross] * 2, [cross, DevicePatternDB.corners(), DevicePatternDB(corners=(0,)), DevicePatternDB(corners=(1,)), DevicePatternDB(edges=(1,))],
	            [cross, "corners"], 7):
		with pytest.raises(ValueError):
			DevicePatternBound(bad)
	ball = DeviceSymBall(2)
	with pytest.raises(ValueError):
		DeviceSymBallSearch(ball, prune=[cross])                                              # prune needs deepen > 0
	with pytest.raises(ValueError):
		DeviceSymBallSearch(ball, deepen=0, prune=[cross])
	agent = DeviceSymBallSearch(ball, deepen=3)
	assert agent.prune is None and (agent.probes, agent.lookups) == (0, 0) and (ball.probes, ball.lookups) == (0, 0)
