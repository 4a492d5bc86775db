"""
The search of DeviceSymBallSearch (engine rk_ssearch_*) restated in plain Python: tests/ball_model.py's `search` with the test
"the ball holds this child" replaced by "tests/sym_model.py's ball of representatives holds canonical(child)", and the ball's
half of the queue taken from sym_model.solve on the meeting state (the descent: the lowest action that gets one level nearer).
The own pool holds raw states.  A helper for tests/test_symsearch_*.py, not a test module.

`Result` is ball_model's; `meeting` is the RAW state that met (the child that was not stored, or the start), `meeting_depth` the
level of its representative.  `popped` is kept beside it: the parents popped, the one whose child met included -- defined for a
search that met or exhausted the graph (a budget refuses a pop that the count would have to split).
"""
import numpy as np

from tests import ball_model
from tests import sym_model
from tests.ball_model import Result, _arrays, _children, apply, scramble  # noqa: F401  (the tests take them from here)

CHUNK = 12 << 10                                   # states canonicalised at once (48 conjugates each)


def _nodes(ball: sym_model.SymBall, states: bytes) -> list:
	"""The ball's node of the representative of every 20-byte state of `states`, 0 where the ball does not hold it."""
	x = np.frombuffer(states, np.int8).reshape(-1, 20)
	out = []
	for at in range(0, len(x), CHUNK):
		reps, _, _ = sym_model.canonical(x[at:at + CHUNK])
		out += [ball.index.get(r.tobytes(), 0) for r in reps]
	return out


def search(start20: np.ndarray, ball: sym_model.SymBall, max_states: int = None):
	"""(Result, popped): as ball_model.search(start20, the plain ball of the same radius, max_states)."""
	max_states = max_states or int(1e10)
	keys = [None, np.ascontiguousarray(start20, np.int8).reshape(20).tobytes()]
	parents, actions = [0, 0], [-1, -1]
	depth_ = 0
	popped = 0

	def done(result, queue=(), node=None, meeting=None):
		return Result(result, list(queue), len(keys) - 1, depth_, None if meeting is None else np.frombuffer(meeting, np.int8).copy(),
		              None if node is None else int(np.searchsorted(ball.level_start, node, side="right")) - 1,
		              *_arrays(keys, parents, actions)), popped

	def path(node):
		out = []
		while parents[node]:
			out.append(actions[node])
			node = parents[node]
		return out[::-1]

	def ball_half(state: bytes) -> list:
		lengths, acts = sym_model.solve(ball, np.frombuffer(state, np.int8)[None])
		return [int(a) for a in acts[0, :lengths[0]]]

	hit = _nodes(ball, keys[1])[0]
	if hit:
		return done(True, ball_half(keys[1]), hit, keys[1])
	index = {keys[1]: 1}
	level = [1]
	while True:
		if not level:
			return done(False)                                 # the whole graph was seen
		new = []
		for at in range(0, len(level), CHUNK // 12):           # (a part of the level at a time: the meeting is often early in it)
			part = level[at:at + CHUNK // 12]
			buf = _children([keys[p] for p in part])
			held = _nodes(ball, buf)
			for j, p in enumerate(part):
				if len(keys) - 1 >= max_states:
					return done(False)
				popped += 1
				for a in range(12):
					k = buf[20 * (12 * j + a):20 * (12 * j + a) + 20]
					if k in index:
						continue
					hit = held[12 * j + a]
					if hit:
						return done(True, path(p) + [a] + ball_half(k), hit, k)
					keys.append(k); parents.append(p); actions.append(a)
					index[k] = len(keys) - 1
					new.append(len(keys) - 1)
		level = new
		depth_ += 1


def meetings_in_batch(start20: np.ndarray, ball: sym_model.SymBall, pops: int) -> int:
	"""How many children of the batch of `pops` parents in which the search from start20 meets are held by the ball: with more
	than one, the lowest batch position has to win.  0 for a start the ball holds."""
	res, popped = search(start20, ball)
	if not res.result or popped == 0:
		return 0
	# the parents of the last level in index order; the batch that holds the winning parent
	level = [i + 1 for i in range(res.len) if _level_of(res, i + 1) == res.depth]
	won = popped - (sum(1 for i in range(res.len) if _level_of(res, i + 1) < res.depth))       # 1-based position in the level
	first = (won - 1) // pops * pops
	batch = level[first:first + pops]
	return sum(1 for h in _nodes(ball, _children([res.states[p - 1].tobytes() for p in batch])) if h)      # (no state is in both pools)


def _level_of(res: Result, node: int) -> int:
	d = 0
	while res.parents[node - 1]:
		node = int(res.parents[node - 1])
		d += 1
	return d
