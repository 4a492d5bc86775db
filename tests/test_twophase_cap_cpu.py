"""
The model of the capped two-phase search (tests/twophase_cap_model.py) without a GPU: with a cap that cannot bind, and with none,
it is the model of tests/twophase_model.py on that model's own case sets (tests/test_twophase_cpu.py); with a cap every improved
row has at most C moves inside the subgroup, the answers solve and are never longer than the chain's, and the two counts are
consistent.
"""
import numpy as np
import pytest

from tests import chain_model as CM
from tests import twophase_cap_model as M
from tests import twophase_model as T
from tests.test_chain_cpu import _words
from tests.test_twophase_cpu import UNLIMITED

MOST_TRIES = (1 << 31) - 1


def _near():
	rs = np.random.RandomState(29)
	near = _words(rs, np.repeat(CM.SOLVED, 200, axis=0), T.GENERATORS[0], 4)
	near[:13] = np.concatenate([CM.SOLVED] + [CM.move(CM.SOLVED, a) for a in range(12)])
	return near


# the case sets of tests/test_twophase_cpu.py: (states, tries, max_nodes)
SETS = {
	"near": lambda: (_near(), 1, 2048),
	"subgroup": lambda: (T.subgroup_states(6)[0], 1, UNLIMITED),
	"scrambles 1 512": lambda: (T.scrambles(29_100, 1 + np.arange(24) * 4 % 60), 1, 512),
	"scrambles 3 4096": lambda: (T.scrambles(29_100, 1 + np.arange(24) * 4 % 60), 3, 4096),
}


@pytest.mark.parametrize("name", list(SETS))
def test_a_cap_that_cannot_bind_is_the_uncapped_model(name):
	states, tries, max_nodes = SETS[name]()
	want = T.solve(states, tries, max_nodes)
	for cap in (CM.max_length(), None):
		got = M.solve(states, tries, max_nodes, cap)
		assert len(got) == 6
		for g, w in zip(got, want):
			assert np.array_equal(g, w), cap
		found, entered = got[5][:, 0], got[5][:, 1]
		assert (entered <= found).all() and (found <= tries).all() and (entered >= 0).all()


@pytest.mark.parametrize("cap", [1, 4, 8, 12])
@pytest.mark.parametrize("tries", [3, MOST_TRIES])
def test_capped_answers(cap, tries):
	states = T.scrambles(32_100, 1 + np.arange(24) % 16)
	chain = CM.solve(states)[0]
	trace = {}
	lengths, actions, phases, reason, nodes, counts = M.solve(states, tries, 2048, cap, trace=trace)
	assert (lengths <= chain).all() and ((reason == 2) == (lengths == chain)).all() and (nodes <= 2048).all()
	assert (phases.sum(axis=1) == lengths).all() and ((nodes == 2048) | (reason != 1)).all()
	assert (T.replay(states, lengths, actions) == CM.SOLVED).all()
	improved = reason != 2
	assert improved.any() and (phases[improved, 1] <= cap).all()
	found, entered = counts[:, 0], counts[:, 1]
	assert (entered <= found).all() and (found <= tries).all() and (entered >= 0).all()
	assert (trace["gave_up"] <= entered).all() and (~trace["first_rejected"] | (found >= 1)).all()
	if tries == 3:
		assert (found == 3).any()                                      # the limit is reached, so found <= tries is a check
