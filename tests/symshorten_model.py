"""
Shortening action queues against the symmetry-reduced goal ball (DeviceSymBall.shorten, engine rk_sshorten) restated in plain
Python: tests/shorten_model.py's pass with the ball of representatives of tests/sym_model.py in the place of the plain ball.
What the device has to reproduce bit for bit.  A helper for tests/test_symball_shorten_*.py, not a test module.

One pass over a word a[0 .. L-1] with a symmetry ball of radius R and a window W >= 1 is shorten_model.one_pass with
  * d(i, j) = sym_model.depth of X(i, j), the solved state after a[i], ..., a[j-1]: the level of its representative, -1 outside;
  * the same edges, the same cost, ties to the largest i, the same copy rule;
  * a replaced segment written as the INVERSE OF THE DESCENT: shorten_model.inverse(sym_model.solve(ball, X(i, j))) -- the ball
    stores no word, solve descends from X(i, j) to solved (the lowest action that gets one level nearer first), and that word
    reversed with every turn the opposite one leads from solved to X(i, j), hence from s_i to s_j.
Conjugation keeps the distance to solved, so d(i, j) is the plain ball's at the same radius and the lengths are
shorten_model's; the replaced words may differ.

Canonical forms are taken in batches (as tests/symsearch_model.py does) and kept: X(i, j) depends on the moves a[i .. j-1] alone,
so the windows of a word, of what a pass makes of it and of the same word at another radius or window share most of them.
"""
import numpy as np

from oracle import cube_oracle as orc
from tests import shorten_model
from tests import sym_model
from tests.shorten_model import MAX_LEN, detour_word, inverse, rev  # noqa: F401  (the tests take them from here)

LENGTHS = (0, 1, 2, 63, 64, 65, 129, 300)         # tests/test_ball_shorten_gpu.py's mixed batch: the edges of a wave's 64-move chunk


def commuting_word(seed: int, a: int) -> list:
	"""Turns of two opposite faces commute, so a b a b a (b = a ^ 2: the opposite face, the same sense) is a' b b: five moves at
	depth three, with no shorter window inside -- a segment that is replaced by a word of THREE moves, of which the ball has several
	(a' b b, b a' b, b b a').  detour_word's detours all cancel through windows of depth 0 or 1, whose word is unique.  Seeded
	moves in front and behind."""
	rng = np.random.RandomState(seed)
	return [int(v) for v in rng.randint(0, 12, 6)] + [a, a ^ 2, a, a ^ 2, a] + [int(v) for v in rng.randint(0, 12, 6)]


def mixed_batch() -> tuple:
	"""The words of tests/test_ball_shorten_gpu.py -- seeded scrambles with detours, cut to LENGTHS -- and four commuting words."""
	words = [tuple(detour_word(40 + k, min(n, 20), n)[:n]) for k, n in enumerate(LENGTHS)]
	return tuple(words + [tuple(commuting_word(70 + k, a)) for k, a in enumerate((0, 3, 5, 10))])


CHUNK = 12 << 10                                   # states canonicalised at once (48 conjugates each)

_reps = {}                                         # 20-byte state -> 20-byte representative


def representatives(states20: np.ndarray) -> list:
	"""The representative of every row, as bytes."""
	keys = [np.ascontiguousarray(s, np.int8).tobytes() for s in np.asarray(states20, np.int8).reshape(-1, 20)]
	missing = sorted({k for k in keys if k not in _reps})
	for at in range(0, len(missing), CHUNK):
		part = missing[at:at + CHUNK]
		reps, _, _ = sym_model.canonical(np.frombuffer(b"".join(part), np.int8).reshape(-1, 20))
		for k, r in zip(part, reps):
			_reps[k] = r.tobytes()
	return [_reps[k] for k in keys]


def window_states(word, window: int):
	"""(pairs [(i, j)], states int8 (len(pairs), 20)): X(i, j) of every window of at most `window` moves, all starts advancing
	together, one offset at a time (shorten_model.window_nodes' walk)."""
	a = np.asarray(word, np.int64)
	L = len(a)
	pairs, rows = [], []
	states = orc.repeat_state(orc.SOLVED, L) if L else np.zeros((0, 20), np.int8)
	for k in range(1, min(window, L) + 1):
		m = L - k + 1
		act = a[k - 1:k - 1 + m]
		states = orc.multi_rotate(states[:m], act // 2, 1 - act % 2)
		pairs += [(i, i + k) for i in range(m)]
		rows.append(np.array(states, np.int8))
	return pairs, (np.concatenate(rows) if rows else np.zeros((0, 20), np.int8))


def window_depths(ball: sym_model.SymBall, word, window: int) -> dict:
	"""(i, j) -> d(i, j) for the windows whose representative the ball holds."""
	pairs, states = window_states(word, window)
	out = {}
	for ij, rep in zip(pairs, representatives(states)):
		node = ball.index.get(rep)
		if node is not None:
			out[ij] = int(np.searchsorted(ball.level_start, node, side="right")) - 1
	return out


def sym_word(ball: sym_model.SymBall, segment) -> list:
	"""The word a replaced segment gets: the inverse of the descent from the segment's net effect."""
	seg = np.asarray(segment, np.int64)
	x = orc.SOLVED.astype(np.int8)[None]
	for a in seg:
		x = orc.multi_rotate(x, np.array([a // 2]), np.array([1 - a % 2]))
	lengths, actions = sym_model.solve(ball, x)
	assert lengths[0] >= 0
	return inverse([int(v) for v in actions[0, :lengths[0]]])


def one_pass(ball: sym_model.SymBall, word, window: int = None, replaced: list = None) -> list:
	"""`replaced`, if given, collects (segment, its replacement) of every segment that was not copied."""
	word = [int(a) for a in word]
	L = len(word)
	if L > MAX_LEN or any(not 0 <= a < 12 for a in word):
		raise ValueError("a word is at most 4096 actions 0..11")
	W = max(L, 1) if window is None else int(window)
	if W < 1:
		raise ValueError("window < 1")
	depths = window_depths(ball, word, W)

	def weight(i, j):
		d = depths.get((i, j))
		if d is not None:
			return d
		return 1 if j - i == 1 else None

	cost, pred = [0] * (L + 1), [0] * (L + 1)
	for j in range(1, L + 1):
		best = None
		for i in range(max(0, j - W), j):                           # ascending, `<=`: the largest i among equal costs
			w = weight(i, j)
			if w is not None and (best is None or cost[i] + w <= best):
				best, pred[j] = cost[i] + w, i
		cost[j] = best
	segments = []
	j = L
	while j > 0:
		segments.append((pred[j], j))
		j = pred[j]
	out = []
	for i, j in reversed(segments):
		if weight(i, j) == j - i:
			out += word[i:j]
		else:
			new = sym_word(ball, word[i:j])
			assert len(new) == depths[(i, j)]
			if replaced is not None:
				replaced.append((word[i:j], new))
			out += new
	assert len(out) == cost[L] <= L
	return out


def shorten(ball: sym_model.SymBall, word, window: int = None, passes: int = None) -> list:
	"""Passes until one does not reduce the length, or `passes` of them."""
	word = [int(a) for a in word]
	done = 0
	while passes is None or done < passes:
		new = one_pass(ball, word, window)
		done += 1
		shorter = len(new) < len(word)
		word = new
		if not shorter:
			break
	return word
