"""
The two-sided breadth-first search of DeviceBiBFS (engine rk_bibfs_*) restated in plain Python over a dict, with the oracle's
moves: what the device engine has to reproduce bit for bit.  A helper for tests/test_bibfs_device_*.py, not a test module.

One pool in index order.  Node 1 is the start (side S = 0), node 2 the solved state (side G = 1); f and b count the complete
levels of S and G.  S grows while f == b, else G.  The parents of the newest level of the side that grows are popped in index
order, before every pop `len >= max_states` ends the search with False; each parent's children are taken in action order 0..11:
  * a child whose state the growing side holds (an earlier child of this level included) is skipped;
  * a child whose state the other side holds is the meeting: the search ends with True and the child is not stored;
  * any other child is appended with its parent, its action and its side.
A level exhausted without a meeting makes that side's depth += 1.  Side G's actions were applied moving away from solved, so the
queue walks them back inverted (rev).
"""
from collections import namedtuple

import numpy as np

from oracle import c_oracle
from oracle import cube_oracle as orc

Result = namedtuple("Result", "result queue len depths meeting states parents actions sides")


def _path(parents, actions, node):
	"""actions root -> node"""
	out = []
	while parents[node]:
		out.append(actions[node])
		node = parents[node]
	return out[::-1]


def search(start20: np.ndarray, max_states: int = None) -> Result:
	"""`start20`: a 20-byte state.  states (n, 20) int8, parents / actions / sides int64 in index order (row i = node i + 1; the
	parent of nodes 1 and 2 is 0, their action -1); meeting: the 20-byte state where the sides met, or None."""
	max_states = max_states or int(1e10)
	start = np.ascontiguousarray(start20, np.int8).reshape(20)
	if orc.is_solved(start):
		return Result(True, [], 0, (0, 0), None, np.zeros((0, 20), np.int8), *(np.zeros(0, np.int64) for _ in range(3)))
	states = [None, start, orc.SOLVED.copy()]                 # index 0 unused
	parents, actions, sides = [0, 0, 0], [-1, -1, -1], [0, 0, 1]
	index = {start.tobytes(): 1, orc.SOLVED.tobytes(): 2}
	level = {0: [1], 1: [2]}
	depth = [0, 0]

	def done(result, queue=(), meeting=None):
		n = len(states) - 1
		return Result(result, list(queue), n, tuple(depth), meeting, np.array(states[1:], np.int8).reshape(n, 20),
		              np.array(parents[1:], np.int64), np.array(actions[1:], np.int64), np.array(sides[1:], np.int64))

	while True:
		side = 0 if depth[0] == depth[1] else 1
		if not level[side]:
			return done(False)                                 # the whole graph was seen
		children, _ = c_oracle.expand12(np.array([states[p] for p in level[side]], np.int8))
		new = []
		for j, p in enumerate(level[side]):
			if len(states) - 1 >= max_states:
				return done(False)
			for a in range(12):
				child = children[12 * j + a]
				hit = index.get(child.tobytes())
				if hit is None:
					states.append(child.copy()); parents.append(p); actions.append(a); sides.append(side)
					index[child.tobytes()] = len(states) - 1
					new.append(len(states) - 1)
				elif sides[hit] != side:
					if side == 0:
						queue = _path(parents, actions, p) + [a] + [orc.rev_action(x) for x in _path(parents, actions, hit)[::-1]]
					else:
						queue = _path(parents, actions, hit) + [orc.rev_action(a)] + [orc.rev_action(x) for x in _path(parents, actions, p)[::-1]]
					return done(True, queue, child.copy())
		level[side] = new
		depth[side] += 1


def one_sided_length(start20: np.ndarray, limit: int = 8) -> int:
	"""Length of a shortest solution by a plain breadth-first search from the start alone (dict, oracle moves), level by level."""
	start = np.ascontiguousarray(start20, np.int8).reshape(1, 20)
	if orc.is_solved(start[0]):
		return 0
	seen = {start[0].tobytes()}
	level = start
	for d in range(1, limit + 1):
		children = orc.expand12(level)
		if orc.multi_is_solved(children).any():
			return d
		nxt = []
		for c in children:
			k = c.tobytes()
			if k not in seen:
				seen.add(k)
				nxt.append(c)
		level = np.array(nxt, np.int8)
	raise AssertionError(f"no solution within {limit} moves")


def scramble(seed: int, depth: int) -> np.ndarray:
	"""A seeded scramble of `depth` moves as a 20-byte state, and nothing of the global generator."""
	rng = np.random.RandomState(seed)
	s = orc.SOLVED.copy()
	for a in rng.randint(0, 12, depth):
		s = orc.rotate(s, a // 2, 1 - a % 2)
	return s


def apply(state20: np.ndarray, queue) -> np.ndarray:
	s = np.asarray(state20, np.int8)
	for a in queue:
		s = orc.rotate(s, a // 2, 1 - a % 2)
	return s
