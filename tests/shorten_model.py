"""
Shortening action queues against the goal ball (DeviceGoalBall.shorten, engine rk_bshorten_*) restated in plain Python over the
ball of tests/ball_model.py, with the oracle's moves: what the device has to reproduce bit for bit.  A helper for
tests/test_ball_shorten_*.py, not a test module.

Cube states are a group: the moves a[i .. j-1] of a word lead from its state s_i to s_j whatever the start, so the distance
between s_i and s_j is the distance to solved of X(i, j), the solved state after a[i], ..., a[j-1] -- and any word that reaches
X(i, j) from solved leads from s_i to s_j too.

One pass over a word a[0 .. L-1] with a ball of radius R and a window W >= 1:
  * for every 0 <= i < j <= L with j - i <= W: d(i, j) = the ball depth of X(i, j), -1 outside the ball;
  * the edge i -> j has weight d(i, j) if that is >= 0, weight 1 if j - i == 1 (a single move outside the ball: R = 0 only), and
    does not exist otherwise;
  * cost[0] = 0, cost[j] = min over i in [max(0, j - W), j - 1] of cost[i] + w(i, j); on ties the LARGEST i wins; pred[j] = that i;
  * back from L along pred; a segment with w(i, j) == j - i is copied, a segment with w < j - i is replaced by the ball's word for
    X(i, j): the stored actions from node 1 down to the node.
The output has cost[L] <= L moves.  `shorten` repeats passes until one does not reduce the length (or `passes` of them are done).
At that fixed point every window of at most W moves whose X the ball holds has exactly d moves, and the pass gives the word back
unchanged.
"""
import numpy as np

from oracle import cube_oracle as orc
from tests import ball_model

MAX_LEN = 4096


def rev(a: int) -> int:
	return orc.rev_action(int(a))


def inverse(word) -> list:
	"""The word that undoes `word`."""
	return [rev(a) for a in reversed(list(word))]


def ball_word(ball: ball_model.Ball, node: int) -> list:
	"""The stored actions from node 1 down to `node`: the ball's word that reaches the node's state from solved."""
	return [rev(x) for x in reversed(ball_model.ball_path(ball, node))]


def window_nodes(ball: ball_model.Ball, word, window: int) -> dict:
	"""(i, j) -> the ball's node of X(i, j), for the windows the ball holds.  All starts advance together, one offset at a time."""
	a = np.asarray(word, np.int64)
	L = len(a)
	nodes = {}
	states = orc.repeat_state(orc.SOLVED, L) if L else np.zeros((0, 20), np.int8)
	for k in range(1, min(window, L) + 1):
		m = L - k + 1                                              # starts 0 .. L - k have a window of k moves
		act = a[k - 1:k - 1 + m]
		states = orc.multi_rotate(states[:m], act // 2, 1 - act % 2)
		for i in range(m):
			node = ball.index.get(np.ascontiguousarray(states[i], np.int8).tobytes())
			if node is not None:
				nodes[(i, i + k)] = node
	return nodes


def window_depths(ball: ball_model.Ball, word, window: int) -> dict:
	"""(i, j) -> d(i, j) for the windows the ball holds."""
	return {ij: ball_model.depth_of(ball, node) for ij, node in window_nodes(ball, word, window).items()}


def one_pass(ball: ball_model.Ball, word, window: int = None) -> list:
	word = [int(a) for a in word]
	L = len(word)
	if L > MAX_LEN or any(not 0 <= a < 12 for a in word):
		raise ValueError("a word is at most 4096 actions 0..11")
	W = max(L, 1) if window is None else int(window)
	if W < 1:
		raise ValueError("window < 1")
	nodes = window_nodes(ball, word, W)

	def weight(i, j):
		node = nodes.get((i, j))
		if node is not None:
			return ball_model.depth_of(ball, node)
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
		out += word[i:j] if weight(i, j) == j - i else ball_word(ball, nodes[(i, j)])
	assert len(out) == cost[L] <= L
	return out


def shorten(ball: ball_model.Ball, word, window: int = None, passes: int = None) -> list:
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


def detour_word(seed: int, depth: int, target: int) -> list:
	"""A seeded scramble of `depth` moves inflated to about `target` moves by seeded detours that leave its effect as it was: a
	random word of 2-6 moves and its inverse inserted somewhere, or a move written as the three opposite turns."""
	rng = np.random.RandomState(seed)
	word = [int(a) for a in rng.randint(0, 12, depth)]
	while len(word) < target:
		at = int(rng.randint(0, len(word) + 1))
		if rng.randint(0, 2) or not word:
			w = [int(a) for a in rng.randint(0, 12, int(rng.randint(2, 7)))]
			word[at:at] = w + inverse(w)
		else:
			at = min(at, len(word) - 1)
			word[at:at + 1] = [rev(word[at])] * 3
	return word
