"""
The depth-first probes past the symmetry ball without a GPU: the plain-Python model (tests/deepen_model.py) against breadth-first
distances, the numbering of the words, and the host-side checks of the new entries and arguments.
  * rank <-> word round trips, the counts 11^e and 12 * 11^(e-1), rank order = lexicographic order;
  * on model balls of radius 2 and 3: the model's solve_beyond lengths equal the breadth-first distances of tests/ball_model.py
    for every state within R + 2 quarter turns (R + 3 at radius 2), every hit lies at ball depth exactly R, and a seeded 50
    answers per level solve their states;
  * the model's frontier continuation gives an optimal queue and names the lowest frontier node, then its lowest word;
  * the entries refuse null handles, and the agents check their new arguments.
"""
import functools
import itertools

import numpy as np
import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceSymBall, DeviceSymBallSearch, _words_of
from tests import ball_model
from tests import deepen_model as model
from tests import sym_model

orc = ball_model.orc


@functools.lru_cache(maxsize=None)
def sym_ball(radius: int):
	return sym_model.build(radius)


@functools.lru_cache(maxsize=None)
def plain_ball(radius: int):
	return ball_model.build(radius)


def level_states(radius: int, level: int) -> np.ndarray:
	"""Every state at exactly `level` quarter turns from solved, in the plain ball's index order."""
	ball = plain_ball(max(radius, level))
	return ball.states[ball.level_start[level] - 1:ball.level_start[level + 1] - 1]


def test_words_and_ranks():
	for e, last in itertools.product((1, 2, 3), (-1, 0, 1, 6, 11)):
		n = model.word_count(e, last)
		assert n == (11 ** e if last >= 0 else 12 * 11 ** (e - 1))
		words = [model.word_of(r, e, last) for r in range(n)]
		assert words == sorted(words) and len(set(map(tuple, words))) == n          # rank order is lexicographic order
		want = [list(w) for w in itertools.product(range(12), repeat=e)
		        if all(a != (p ^ 1) for p, a in zip((last,) + w[:-1], w) if p >= 0)]
		assert words == want
		assert [model.rank_of(w, last) for w in words] == list(range(n))
		assert (_words_of(np.arange(n), e, np.full(n, last)) == np.array(words)).all()      # the agents' decoder
	for e in (4, 8):
		assert model.word_count(e, 3) == 11 ** e and model.word_count(e) == 12 * 11 ** (e - 1)
		for r in (0, 1, 120, 121, 11 ** e - 1, model.word_count(e) - 1):
			assert model.rank_of(model.word_of(r, e), -1) == r
	with pytest.raises(AssertionError):
		model.word_of(11 ** 3, 3, 5)


@pytest.mark.parametrize("radius, beyond", [(2, 3), (3, 2)])
def test_model_lengths_are_breadth_first_distances(radius, beyond):
	"""Every state of every level from R to R + beyond: at radius 2 all 93 840 states of level 5 with their 1 584 words of round 3."""
	ball = sym_ball(radius)
	# membership by the plain ball's raw states is membership by representatives (what the model's first look relies on)
	near = np.concatenate([level_states(radius, l) for l in range(radius + 2)])
	assert ((sym_model.depth(ball, near) >= 0) == (np.arange(len(near)) < plain_ball(radius).len)).all()
	for extra in range(beyond + 1):
		states = level_states(radius, radius + extra)
		lengths, actions = model.solve_beyond(ball, states, beyond)
		assert (lengths == radius + extra).all()
		assert ((actions >= 0).sum(axis=1) == lengths).all() and (actions[:, radius + extra:] == -1).all()
		for i in np.random.RandomState(extra).choice(len(states), min(len(states), 50), replace=False):
			assert orc.is_solved(ball_model.apply(states[i], actions[i, :lengths[i]]))
			moved = ball_model.apply(states[i], actions[i, :extra])
			assert sym_model.depth(ball, moved[None]).tolist() == [radius]                  # the hit lies on the ball's surface
		if extra:
			assert (model.solve_beyond(ball, states[:40], extra - 1)[0] == -1).all()          # too few moves: no answer


def test_model_last_action_prunes_only_its_opposite():
	ball = sym_ball(2)
	rng = np.random.RandomState(5)
	states = level_states(2, 4)[rng.choice(10_011, 300, replace=False)]
	last = rng.randint(-1, 12, 300)
	free, _ = model.solve_beyond(ball, states, 3)
	pruned, actions = model.solve_beyond(ball, states, 3, last)
	assert (free == 4).all() and ((pruned == 4) | (pruned == -1)).all()                     # (6 = 4 + 2 would take a fourth round)
	assert ((actions[:, 0] != (last ^ 1)) | (last < 0)).all()
	assert (pruned[last < 0] == 4).all() and (pruned == -1).any()         # every shortest word may begin with the pruned turn


def test_model_frontier_continuation():
	ball = sym_ball(2)
	start = ball_model.apply(orc.SOLVED, np.random.RandomState(3).randint(0, 12, 9))      # 7 quarter turns from solved
	want = len(ball_model.search(start, plain_ball(2)).queue)
	assert want == 7
	got = model.continue_from_frontier(start, ball, 200, 8)                                  # levels 0..2 fit: 127 states
	assert got.result and got.level == 2 and got.frontier == (14, 127) and got.deepened == want - 2 - 2
	assert len(got.queue) == want and orc.is_solved(ball_model.apply(start, got.queue))
	# no lower node has a hit in that round, and the word is the node's lowest
	states, last = got.states[13:got.node - 1], got.actions[13:got.node - 1]
	assert (model.lowest_hits(ball, states, last, got.deepened) == -1).all()
	word = got.queue[2:2 + got.deepened]
	assert model.rank_of(word, int(got.actions[got.node - 1])) == got.rank
	assert not model.continue_from_frontier(start, ball, 200, got.deepened - 1).result


def test_entries_refuse_null_handles_and_agents_check_arguments():
	lib = _ffi.lib()
	assert lib.rk_sdeepen_max_probes() == 1 << 28
	assert lib.rk_sdeepen(None, None, None, 0, 1, 0, 1, None, None) == -1
	assert lib.rk_sdeepen_nodes(None, 1, 1, 1, 0, 1, None, None) == -4
	assert lib.rk_sdeepen_frontier(None, None, None) == -4 and lib.rk_sdeepen_set_pops(None, 1, None) == -4
	assert lib.rk_sdeepen_path(None, 1, 1, 0, None, 0, None) == -4
	ball = DeviceSymBall(2)
	for bad in (-1, 9, 1.5, True):
		with pytest.raises(ValueError):
			DeviceSymBallSearch(ball, deepen=bad)
	agent = DeviceSymBallSearch(ball, deepen=8)
	assert (agent.deepen, agent.deepened, agent.probes) == (8, 0, 0) and DeviceSymBallSearch(ball).deepen == 0
