"""
The probes past the symmetry ball pruned by pattern databases (engines rk_bound_*, rk_sdeepen_pruned, rk_sdeepen_nodes_pruned)
restated in NumPy on top of tests/pdb_model.py and tests/deepen_model.py.  A helper for tests/test_deepen_prune_*.py, not a test
module.

The bound of a state is the greatest of its entries over some pattern tables; a table in which the state has no entry, or an
unreached one, counts 0.  A pattern's entry never exceeds the distance to solved, so the bound is admissible.

The cut.  With R the ball's radius, a word of e moves survives when for every k = 0..e the state after its first k moves has
bound <= R + (e - k): the start, every state on the way, the next-to-last state (R + 1) and the leaf (R).  A word that hits
survives -- the state after k of its moves is at most (e - k) + R from solved -- and only a survivor costs a look-up in the ball.
"""
import functools

import numpy as np

from oracle import c_oracle
from oracle import cube_oracle as orc
from tests import deepen_model
from tests import pdb_model

CROSS_D = tuple(sorted(int(e) for e in orc._FACES[3][1]))
#: the small patterns of the tests: (corners, edges)
PATTERNS = {"cross": ((), CROSS_D), "corners3": ((0, 1, 2), ()), "mixed": ((3, 4), (0, 5))}


@functools.lru_cache(maxsize=None)
def table(name: str):
	"""(Pattern, its table) of one of PATTERNS"""
	p = pdb_model.Pattern(*PATTERNS[name])
	return p, p.table()[0]


def tables(names) -> list:
	return [table(n) for n in names]


def depths(tabs, states20) -> np.ndarray:
	"""int64 (n,): the greatest of the tables' depths, -1 only where every table answers -1 (DevicePatternDB.lower_bound)"""
	states20 = np.asarray(states20).reshape(-1, 20)
	return np.max([p.depth(t, states20) for p, t in tabs], axis=0) if len(states20) else np.zeros(0, np.int64)


def bound(tabs, states20) -> np.ndarray:
	"""int64 (n,): the bound the probes prune by: as `depths`, a table without an entry for the state or with 255 counting 0"""
	states20 = np.asarray(states20).reshape(-1, 20)
	out = np.zeros(len(states20), np.int64)
	for p, t in tabs:
		d = p.depth(t, states20)
		out = np.maximum(out, np.where((d < 0) | (d == pdb_model.UNREACHED), 0, d))
	return out


def word_survives(ball_radius: int, tabs, state20, last: int, rank: int, extra: int) -> bool:
	"""Whether no prefix of word `rank` of `extra` moves behind `last` is cut."""
	word = deepen_model.words_of(np.array([rank]), extra, np.array([last]))[0]
	s = np.asarray(state20, np.int8).reshape(1, 20)
	for k in range(extra + 1):
		if bound(tabs, s)[0] > ball_radius + extra - k:
			return False
		if k < extra:
			s = c_oracle.multi_rotate(s, np.array([word[k]], np.uint8))
	return True


def surviving_words(ball_radius: int, tabs, states20, last, extra: int) -> np.ndarray:
	"""int64 (n,): the words of `extra` moves of each state (behind its last action, -1: none) that pass every cut: the look-ups
	of a round in which nothing hits.  Level by level: what is cut at k moves is not moved on."""
	s = np.ascontiguousarray(states20, np.int8).reshape(-1, 20)
	n = len(s)
	prev, owner = np.asarray(last, np.int64).reshape(-1).copy(), np.arange(n)
	for k in range(extra + 1):
		keep = bound(tabs, s) <= ball_radius + extra - k
		s, prev, owner = s[keep], prev[keep], owner[keep]
		if k == extra:
			break
		a = np.tile(np.arange(12), len(s))
		p = np.repeat(prev, 12)
		allowed = (p < 0) | (a != (p ^ 1))
		s = c_oracle.multi_rotate(np.repeat(s, 12, axis=0)[allowed], a[allowed].astype(np.uint8)) if allowed.any() else np.zeros((0, 20), np.int8)
		prev, owner = a[allowed], np.repeat(owner, 12)[allowed]
	return np.bincount(owner, minlength=n).astype(np.int64)
