"""
The model of the subgroup chain (tests/chain_model.py) against the oracle alone, without a GPU: the coset counts of the four
stages, that a generator's effect on a signature depends on the signature alone, and that the model's solutions solve.
"""
import numpy as np
import pytest

from oracle import cube_oracle as orc
from tests import chain_model as M

PAIRS = 3000


def _words(rs, start, gens, length):
	"""the rows of `start`, each moved by `length` seeded generators"""
	s = np.array(start, np.int64)
	for _ in range(length):
		pick = rs.randint(0, len(gens), len(s))
		for g, gen in enumerate(gens):
			m = pick == g
			s[m] = M.apply_generator(s[m], gen)
	return s


def test_what_the_move_table_gives():
	assert M.AXES == ((0, 1), (2, 3), (4, 5))
	assert M.SLICES == ((4, 5, 6, 7), (1, 3, 9, 11), (0, 2, 8, 10))
	assert [len(g) for g in M.GENERATORS] == [12, 10, 8, 6]
	assert M.GENERATORS[1] == ((0,), (1,), (2,), (3,), (4, 4), (6, 6), (8,), (9,), (10,), (11,))
	assert M.GENERATORS[2] == ((0,), (1,), (2,), (3,), (4, 4), (6, 6), (8, 8), (10, 10))
	assert len(M.c3()) == 96 and M.coset_count() == 420


@pytest.mark.parametrize("stage", range(4))
def test_coset_counts(stage):
	dist = M.search(stage)
	assert len(dist) == M.COUNTS[stage]
	t = M.table(stage)
	assert (t == 0).sum() == 1 and (t != M.UNREACHED).sum() == M.COUNTS[stage]
	assert t[M.index(stage, M.signature(stage, M.SOLVED))[0]] == 0


@pytest.mark.parametrize("stage", range(4))
def test_a_generator_maps_equal_signatures_to_equal_signatures(stage):
	"""Pairs of DIFFERENT states of one signature: the same word of the stage's generators from solved and from another state of
	the goal's signature -- a word of the next stage's generators (they keep the goal of this stage); for stage 4, whose
	signature names its state inside the half-turn group, solved with two edges flipped in place."""
	rs = np.random.RandomState(2700 + stage)
	gens = M.GENERATORS[stage]
	solved = np.repeat(M.SOLVED, PAIRS, axis=0)
	if stage < 3:
		other = _words(rs, solved, M.GENERATORS[stage + 1], 25)
	else:
		other = solved.copy()
		other[:, 8:10] ^= 1
	assert (M.signature(stage, other) == M.signature(stage, M.SOLVED)[0]).all()
	state = rs.get_state()
	a = _words(rs, solved, gens, 30)
	rs.set_state(state)                                                    # the same words
	b = _words(rs, other, gens, 30)
	assert (a != b).any(axis=1).sum() > PAIRS // 2
	assert (M.signature(stage, a) == M.signature(stage, b)).all()
	for gen in gens:
		assert (M.signature(stage, M.apply_generator(a, gen)) == M.signature(stage, M.apply_generator(b, gen))).all()


def test_model_solutions_solve():
	rs = np.random.RandomState(27)
	n = 2000
	s = orc.repeat_state(orc.SOLVED, n)
	for _ in range(60):
		s = orc.multi_rotate(s, rs.randint(0, 6, n), rs.randint(0, 2, n))
	lengths, actions, stages = M.solve(s)
	assert (stages.sum(axis=1) == lengths).all() and lengths.max() <= M.max_length() and (stages <= np.array(M.max_depths())).all()
	out = s.copy()
	for t in range(actions.shape[1]):
		live = np.nonzero(lengths > t)[0]
		a = actions[live, t]
		assert ((a >= 0) & (a < 12)).all()
		out[live] = orc.multi_rotate(out[live], a // 2, 1 - a % 2)
	assert orc.multi_is_solved(out).all()
	assert (np.where(np.arange(actions.shape[1])[None, :] >= lengths[:, None], actions, -1) == -1).all()
