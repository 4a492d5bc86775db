"""
The groups of states that tests/test_beam_batch_gpu.py plays on DeviceBeamSearchBatch, with the answer of the plain-Python model
(tests/beam_model.py::search) for every state ALONE -- a batch result is compared state by state with these.  A helper for
tests/test_beam_batch_*.py, not a test module; tests/test_beam_batch_cpu.py shows on the model alone that the groups are not weak.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import cube_oracle as orc
from tests import beam_model as bm

#: net, width, slots, number of states, max_depth, prune_inverse, the first state's k (below).  The single engine's widths: 12, 60, 72, 264, 4 104 and 16 392
#: children in a depth; the last two run many commit tiles and look-back rounds per slot, at different epochs side by side.
Group = namedtuple("Group", "net width slots states max_depth prune first", defaults=(0,))
GROUPS = [
	Group("noisy", 1, 3, 7, 12, True),
	Group("noisy", 5, 1, 9, 12, True),
	Group("lookup_special", 6, 7, 9, 12, True),
	Group("lookup", 22, 3, 9, 12, True),
	Group("lookup_bf16", 22, 4, 9, 12, False),
	Group("linear_bf16", 22, 3, 7, 12, False),
	Group("noisy", 342, 3, 5, 12, True),
	Group("lookup", 1366, 2, 3, 5, True, 3),             # (from the 6-move scramble on: two of the three fill the beam)
]
SCRAMBLES = (1, 3, 4, 6, 9)
BALL_SCRAMBLES = (2, 4, 6, 9)
#: to the radius-3 ball: (net, width, slots, states); a solved start is added behind the scrambled ones
BALL_GROUPS = [("noisy", 5, 3, 8), ("noisy", 22, 3, 8)]
#: the group whose states get budgets of their own, and the states: I its own explored count, J its count minus one (status 2)
BUDGET_GROUP, BUDGET_I, BUDGET_J = GROUPS[3], 2, 4


def group_id(g) -> str:
	return "-".join(str(x) for x in g)


def starts_of(n: int, scrambles=SCRAMBLES, first: int = 0) -> np.ndarray:
	"""(n, 20): state k = first .. first + n - 1 is the scramble of seed 700 + k, scrambles[k % len(scrambles)] moves deep"""
	return np.array([bm.start_of(700 + k, scrambles[k % len(scrambles)]) for k in range(first, first + n)], np.int8)


def group_starts(g) -> np.ndarray:
	return starts_of(g.states, SCRAMBLES, g.first)


@functools.lru_cache(maxsize=None)
def alone(net: str, width: int, max_depth: int, prune: bool, k: int, budget: int = None, scrambles=SCRAMBLES, radius: int = None) -> bm.Result:
	"""The model's answer for state k alone; computed once per process and shared (treat it as read-only)."""
	ball = bm.ball_model(radius) if radius is not None else None
	return bm.search(bm.values_of(bm.net_of(net)), bm.start_of(700 + k, scrambles[k % len(scrambles)]), width, max_depth, ball, prune, budget)


def references(g: Group) -> list:
	return [alone(g.net, g.width, g.max_depth, g.prune, k) for k in range(g.first, g.first + g.states)]


def ball_starts(n: int) -> np.ndarray:
	return np.concatenate([starts_of(n, BALL_SCRAMBLES), orc.SOLVED[None]]).astype(np.int8)


def ball_references(net: str, width: int, n: int) -> list:
	solved = bm.search(bm.values_of(bm.net_of(net)), orc.SOLVED, width, 12, bm.ball_model(bm.BALL_RADIUS))
	return [alone(net, width, 12, True, k, None, BALL_SCRAMBLES, bm.BALL_RADIUS) for k in range(n)] + [solved]


def budgets_and_references() -> tuple:
	"""(budgets, one per state with None for no budget; the model's answers under them) for BUDGET_GROUP"""
	g = BUDGET_GROUP
	free = references(g)
	budgets = [None] * g.states
	budgets[BUDGET_I], budgets[BUDGET_J] = free[BUDGET_I].explored, free[BUDGET_J].explored - 1
	return budgets, [alone(g.net, g.width, g.max_depth, g.prune, k, budgets[k]) for k in range(g.states)]
