"""
The model of the two-phase search (tests/twophase_model.py) against the oracle alone, without a GPU: the four pruning tables reach
their counts, the table indices are closed under their generators, each phase's first solution is optimal on shallow cases
(against breadth-first searches that use no table) and the model's answers solve.
"""
import numpy as np
import pytest

from oracle import cube_oracle as orc
from tests import chain_model as CM
from tests import twophase_model as T
from tests.test_chain_cpu import _words

PAIRS = 2000
UNLIMITED = 1 << 40


@pytest.mark.parametrize("table", range(4))
def test_table_counts(table):
	t = T.table(table)
	assert len(t) == T.SIZES[table] and (t != 255).sum() == T.COUNTS[table] == T.SIZES[table] - (t == 255).sum()
	assert (t == 0).sum() == 1 and t[T.table_index(table, CM.SOLVED)[0]] == 0


@pytest.mark.parametrize("table", range(4))
def test_a_generator_maps_equal_indices_to_equal_indices(table):
	"""Pairs of DIFFERENT states of one index under the same word.  Tables 1, 2: solved and a state of the subgroup.  Tables 3, 4:
	solved and solved with two cubies that the index does not read exchanged in place."""
	rs = np.random.RandomState(2900 + table)
	gens = T.GENERATORS[table >= 2]
	solved = np.repeat(CM.SOLVED, PAIRS, axis=0)
	if table < 2:
		other = _words(rs, solved, T.GENERATORS[1], 25)
	else:
		other = solved.copy()
		if table == 2:
			o = list(CM.OUTSIDE0[:2])
			other[:, [8 + o[0], 8 + o[1]]] = other[:, [8 + o[1], 8 + o[0]]]
		else:
			other[:, [0, 1]] = other[:, [1, 0]]
	assert (T.table_index(table, other) == T.table_index(table, CM.SOLVED)[0]).all()
	state = rs.get_state()
	a = _words(rs, solved, gens, 30)
	rs.set_state(state)
	b = _words(rs, other, gens, 30)
	assert (a != b).any(axis=1).sum() > PAIRS // 2
	assert (T.table_index(table, a) == T.table_index(table, b)).all()
	for gen in gens:
		assert (T.table_index(table, CM.apply_generator(a, gen)) == T.table_index(table, CM.apply_generator(b, gen))).all()


def test_move_pruning_keeps_a_cheapest_word_per_element():
	"""every element within 4 quarter turns (and within cost 5 of the subgroup's generators) is reached by a word of the rule at its
	distance: the words of the rule, level by level, cover the breadth-first levels"""
	for phase, gens, depth in ((1, T.GENERATORS[0], 4), (2, T.GENERATORS[1], 5)):
		seen, words = {tuple(CM.SOLVED[0].tolist())}, {0: [(CM.SOLVED[0], 255, 255)]}
		plain = {0: {tuple(CM.SOLVED[0].tolist())}}
		for d in range(1, depth + 1):
			words[d], plain[d] = [], set()
			for gen in gens:
				for s, last, last2 in words.get(d - len(gen), []):
					if T.allowed(phase, last, last2) >> gen[0] & 1:
						words[d].append((CM.apply_generator(s[None], gen)[0], gen[0], last))
				for k in plain.get(d - len(gen), ()):
					c = tuple(CM.apply_generator(np.array(k)[None], gen)[0].tolist())
					if c not in seen:
						plain[d].add(c)
			seen |= plain[d]
			assert plain[d] <= {tuple(s.tolist()) for s, _, _ in words[d]}, (phase, d)


def test_first_solutions_are_optimal_on_shallow_cases():
	rs = np.random.RandomState(29)
	# phase 1: states within 4 turns, against the breadth-first coset distance
	near = _words(rs, np.repeat(CM.SOLVED, 200, axis=0), T.GENERATORS[0], 4)
	near[:13] = np.concatenate([CM.SOLVED] + [CM.move(CM.SOLVED, a) for a in range(12)])
	lengths, actions, phases, reason, nodes = T.solve(near, 1, 2048)
	dist = T.coset_distances(4)
	want = np.array([dist[k] for k in T.coset_key(near)])
	improved = reason == 0
	assert improved.any() and (phases[improved, 0] == want[improved]).all()
	assert (T.replay(near, lengths, actions) == CM.SOLVED).all() and (lengths <= CM.solve(near)[0]).all()
	# phase 2: the subgroup's states of cost <= 6, against their breadth-first cost
	states, cost = T.subgroup_states(6)
	lengths, actions, phases, reason, nodes = T.solve(states, 1, UNLIMITED)
	assert (phases[:, 0] == 0).all() and (lengths == cost).all() and (reason != 1).all()
	assert (T.replay(states, lengths, actions) == CM.SOLVED).all()


def test_model_answers_solve_under_the_oracle():
	states = T.scrambles(29_100, 1 + np.arange(24) * 4 % 60)
	chain = CM.solve(states)[0]
	for tries, max_nodes in ((1, 512), (3, 4096)):
		lengths, actions, phases, reason, nodes = T.solve(states, tries, max_nodes)
		assert (lengths <= chain).all() and ((reason == 2) == (lengths == chain)).all() and (nodes <= max_nodes).all()
		assert (phases.sum(axis=1) == lengths).all() and ((nodes == max_nodes) | (reason != 1)).all()
		out = states.copy()
		for t in range(actions.shape[1]):
			live = np.nonzero(lengths > t)[0]
			a = actions[live, t]
			assert ((a >= 0) & (a < 12)).all()
			out[live] = orc.multi_rotate(out[live], a // 2, 1 - a % 2)
		assert orc.multi_is_solved(out).all()
		assert (np.where(np.arange(actions.shape[1])[None, :] >= lengths[:, None], actions, -1) == -1).all()
