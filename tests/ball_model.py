"""
The goal ball of DeviceGoalBall (engine rk_ball_*) and the search of DeviceBallSearch (engine rk_bsearch_*) restated in plain
Python over dicts, with the oracle's moves: what the device engines have to reproduce bit for bit.  A helper for
tests/test_goal_ball_*.py, not a test module.

The ball.  Node 1 is the solved state, the pool is in index order.  A level's parents are popped in index order, their children
taken in action order 0..11; a child the pool holds (an earlier child of the level included) is skipped, every other is appended
with its parent and its action -- the move away from solved.  Level `radius` is stored and never expanded.  Level l is the index
range level_start[l] .. level_start[l + 1] - 1.

The search.  Node 1 of a pool of its own is the start.  If the ball holds the start, the answer is the ball's path and nothing is
popped.  Otherwise the parents of the newest level are popped in index order; before every pop `len >= max_states` ends the
search with False; each parent's children are taken in action order:
  * a child the own pool holds is skipped;
  * a child the ball holds is the meeting: the search ends with True and the child is not stored;
  * any other child is appended with its parent and its action.
A level exhausted without a meeting makes `depth` += 1.  The queue is the path from the start to the popped parent, the meeting
action, then the ball's path from the meeting node: the inverse of every stored action on the way back to node 1.
"""
from collections import namedtuple

import numpy as np

from oracle import c_oracle
from oracle import cube_oracle as orc
from tests.bibfs_model import apply, scramble  # noqa: F401  (the tests take them from here)

Ball = namedtuple("Ball", "radius len level_start states parents actions index")
Result = namedtuple("Result", "result queue len depth meeting meeting_depth states parents actions")


def _children(keys) -> bytes:
	"""The 12 children of every 20-byte key, parent-major / action-minor, as one bytes object (20 bytes per child)."""
	parents = np.frombuffer(b"".join(keys), np.int8).reshape(-1, 20)
	children, _ = c_oracle.expand12(np.ascontiguousarray(parents))
	return np.ascontiguousarray(children, np.int8).tobytes()


def _arrays(keys, parents, actions):
	n = len(keys) - 1
	return (np.frombuffer(b"".join(keys[1:]), np.int8).reshape(n, 20).copy(), np.array(parents[1:], np.int64),
	        np.array(actions[1:], np.int64))


def build(radius: int) -> Ball:
	"""states (n, 20) int8, parents / actions int64 in index order (row i = node i + 1; node 1 has parent 0 and action -1);
	level_start int64 (radius + 2,); index: state bytes -> node."""
	keys = [None, orc.SOLVED.astype(np.int8).tobytes()]           # index 0 unused
	parents, actions = [0, 0], [-1, -1]
	index = {keys[1]: 1}
	level_start = [1, 2]
	level = [1]
	for _ in range(radius):
		buf = _children([keys[p] for p in level])
		new = []
		for j, p in enumerate(level):
			for a in range(12):
				k = buf[20 * (12 * j + a):20 * (12 * j + a) + 20]
				if k in index:
					continue
				keys.append(k); parents.append(p); actions.append(a)
				index[k] = len(keys) - 1
				new.append(len(keys) - 1)
		level = new
		level_start.append(len(keys))
	return Ball(radius, len(keys) - 1, np.array(level_start, np.int64), *_arrays(keys, parents, actions), index)


def depth_of(ball: Ball, node: int) -> int:
	return int(np.searchsorted(ball.level_start, node, side="right")) - 1


def depth(ball: Ball, state20: np.ndarray) -> int:
	"""Exact distance to solved of a state the ball holds, else -1."""
	node = ball.index.get(np.ascontiguousarray(state20, np.int8).tobytes())
	return -1 if node is None else depth_of(ball, node)


def ball_path(ball: Ball, node: int) -> list:
	"""The moves from node `node` to the solved state."""
	out = []
	while node != 1:
		out.append(orc.rev_action(int(ball.actions[node - 1])))
		node = int(ball.parents[node - 1])
	return out


def solve(ball: Ball, state20: np.ndarray):
	"""The shortest solution of a state the ball holds, else None."""
	node = ball.index.get(np.ascontiguousarray(state20, np.int8).tobytes())
	return None if node is None else ball_path(ball, node)


def search(start20: np.ndarray, ball: Ball, max_states: int = None) -> Result:
	"""`start20`: a 20-byte state.  states / parents / actions: the own pool in index order (the start has parent 0, action -1);
	meeting: the 20-byte state that the ball holds (the start itself when the ball holds it), meeting_depth its depth there."""
	max_states = max_states or int(1e10)
	keys = [None, np.ascontiguousarray(start20, np.int8).reshape(20).tobytes()]
	parents, actions = [0, 0], [-1, -1]
	depth_ = 0

	def done(result, queue=(), node=None, meeting=None):
		return Result(result, list(queue), len(keys) - 1, depth_, None if meeting is None else np.frombuffer(meeting, np.int8).copy(),
		              None if node is None else depth_of(ball, node), *_arrays(keys, parents, actions))

	def path(node):
		out = []
		while parents[node]:
			out.append(actions[node])
			node = parents[node]
		return out[::-1]

	hit = ball.index.get(keys[1])
	if hit is not None:
		return done(True, ball_path(ball, hit), hit, keys[1])
	index = {keys[1]: 1}
	level = [1]
	while True:
		if not level:
			return done(False)                                 # the whole graph was seen
		buf = _children([keys[p] for p in level])
		new = []
		for j, p in enumerate(level):
			if len(keys) - 1 >= max_states:
				return done(False)
			for a in range(12):
				k = buf[20 * (12 * j + a):20 * (12 * j + a) + 20]
				if k in index:
					continue
				hit = ball.index.get(k)
				if hit is not None:
					return done(True, path(p) + [a] + ball_path(ball, hit), hit, k)
				keys.append(k); parents.append(p); actions.append(a)
				index[k] = len(keys) - 1
				new.append(len(keys) - 1)
		level = new
		depth_ += 1
