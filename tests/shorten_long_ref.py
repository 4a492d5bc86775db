"""
A fast exact reference of one shortening pass (tests/shorten_model.py, tests/symshorten_model.py) for queues at the engines' limit
of 4 096 moves and windows of up to the whole queue, in NumPy, without a device; and the seeded 4 096-move words that take the
kernels to that limit.  A helper for tests/test_shorten_limits_*.py, not a test module.

The models look every window up in a dict (and the symmetry model canonicalises every window's state first): O(L * W) Python
steps per word, which L = W = 4 096 puts out of a test's reach.  Here
  * d(i, j) of all windows comes from the models' walk -- all starts advance together, one offset at a time
    (shorten_model.window_nodes) -- with the states of an offset looked up at once: the plain model ball's states
    (ball_model.build) sorted as 20-byte keys, np.searchsorted on the window's states, a hit confirmed by equality, the depth from
    level_start.  Conjugation keeps the distance to solved, so these are the symmetry ball's depths too (symshorten_model's
    header): one routine for both kinds, nothing canonicalised;
  * the DP is the models' rule, vectorised per j over i: cost[i] + d(i, j) over the held windows, a single move outside the ball
    costs 1, the least cost and among equal costs the largest i;
  * the emit walks pred back from L; an edge with d >= span or d < 0 is copied, a replaced edge gets the kind's own word for
    X(i, j) from the models: shorten_model.ball_word (plain), the inverse of sym_model.solve's descent (sym) -- only the few
    replaced edges go through them.
tests/test_shorten_limits_cpu.py pins one pass of it to both models, word for word, on the batches the GPU suites already use.

The depth table is laid out as the engines' scratch is -- row j - 1, column j - i - 1 -- because the DP reads a row per j; nothing
else is taken from the device code.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import cube_oracle as orc
from tests import ball_model
from tests import shorten_model
from tests import sym_model
from tests.shorten_model import detour_word, inverse, rev

LIMIT = 4096                                       # the engines' longest queue and widest window
KINDS = ("plain", "sym")

#: word: the new word (tuple); cost: cost[L]; pred: int64 (L + 1,); replaced: ((i, j, d), ...) in word order; ties: the number of j
#: whose minimum more than one i attains; tie_spread: ((j, the largest distance between the tied i), ...) for those j
Pass = namedtuple("Pass", "word cost pred replaced ties tie_spread")

_KEY = np.dtype("V20")


@functools.lru_cache(maxsize=None)
def plain_ball(radius: int) -> ball_model.Ball:
	return ball_model.build(radius)


@functools.lru_cache(maxsize=None)
def sym_ball(radius: int) -> sym_model.SymBall:
	return sym_model.build(radius)


@functools.lru_cache(maxsize=None)
def _sorted_ball(radius: int):
	"""(the ball's states as sorted 20-byte keys, the depth of each)."""
	ball = plain_ball(radius)
	keys = np.ascontiguousarray(ball.states, np.int8).view(_KEY).reshape(-1)
	order = np.argsort(keys, kind="stable")
	depth = np.searchsorted(ball.level_start, order + 1, side="right") - 1      # row r is node r + 1
	return keys[order], depth.astype(np.int8)


def ball_depths(radius: int, states20: np.ndarray) -> np.ndarray:
	"""int8 (n,): the exact distance to solved of every state the ball of `radius` holds, -1 for the others."""
	keys, depth = _sorted_ball(radius)
	q = np.ascontiguousarray(states20, np.int8).view(_KEY).reshape(-1)
	at = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
	return np.where(keys[at] == q, depth[at], np.int8(-1)).astype(np.int8)


_tables = []                                       # the last few tables of long words: (radius, word, table), 16 MB each


def window_depths(word, radius: int, window: int) -> np.ndarray:
	"""int8 (L, W), W = min(window, L): [j - 1, j - i - 1] = d(i, j), -1 outside the ball (and where i would be < 0).  d(i, j)
	depends on the moves i .. j-1 alone, so a prefix of a word and a narrower window read the table of the word: the tables of
	long words are kept."""
	word = tuple(int(v) for v in word)
	L = len(word)
	W = min(window, L)
	for r, known, table in _tables:
		if r == radius and table.shape[1] >= W and known[:L] == word:
			return table[:L, :W]
	table = _window_depths(word, radius, W)
	if L >= 1024:
		_tables.insert(0, (radius, word, table))
		del _tables[4:]
	return table


def _window_depths(word: tuple, radius: int, W: int) -> np.ndarray:
	a = np.asarray(word, np.int64)
	L = len(a)
	table = np.full((L, W), -1, np.int8)
	states = orc.repeat_state(orc.SOLVED, L) if L else np.zeros((0, 20), np.int8)
	for k in range(1, W + 1):
		m = L - k + 1                                              # starts 0 .. L - k have a window of k moves
		act = a[k - 1:k - 1 + m]
		states = orc.multi_rotate(states[:m], act // 2, 1 - act % 2)
		table[np.arange(k - 1, L), k - 1] = ball_depths(radius, states)     # start i ends at j = i + k
	return table


@functools.lru_cache(maxsize=None)
def _dp(word: tuple, radius: int, window: int):
	"""(cost int64 (L + 1,), pred int64 (L + 1,), the edges (i, j, d) of the path in word order, ties, tie_spread)."""
	L = len(word)
	table = window_depths(word, radius, window)
	cost, pred = np.zeros(L + 1, np.int64), np.zeros(L + 1, np.int64)
	never = np.int64(1) << 40
	ties, spread = 0, []
	for j in range(1, L + 1):
		kmax = min(window, j)
		d = table[j - 1, :kmax].astype(np.int64)                        # column k - 1: i = j - k
		wgt = np.where(d >= 0, d, never)
		if d[0] < 0:
			wgt[0] = 1                                                 # a single move outside the ball
		cand = cost[j - kmax:j][::-1] + wgt
		best = cand.min()
		at = np.nonzero(cand == best)[0]                                # ascending k: the first is the largest i
		cost[j], pred[j] = best, j - 1 - at[0]
		if len(at) > 1:
			ties += 1
			spread.append((j, int(at[-1] - at[0])))
	edges = []
	j = L
	while j > 0:
		i = int(pred[j])
		edges.append((i, j, int(table[j - 1, j - i - 1])))
		j = i
	return cost, pred, tuple(reversed(edges)), ties, tuple(spread)


def effect(word) -> np.ndarray:
	"""The solved state after `word`."""
	x = orc.SOLVED.astype(np.int8)[None]
	for a in word:
		x = orc.multi_rotate(x, np.array([a // 2]), np.array([1 - a % 2]))
	return x[0]


def _words_for(kind: str, radius: int, states: np.ndarray) -> list:
	"""The kind's word for every state (all of them in the ball)."""
	if kind == "plain":
		ball = plain_ball(radius)
		return [shorten_model.ball_word(ball, ball.index[np.ascontiguousarray(s, np.int8).tobytes()]) for s in states]
	assert kind == "sym"
	lengths, actions = sym_model.solve(sym_ball(radius), states)         # as symshorten_model.sym_word, for all edges at once
	assert (lengths >= 0).all()
	return [inverse([int(v) for v in actions[r, :lengths[r]]]) for r in range(len(states))]


@functools.lru_cache(maxsize=None)
def _one_pass(kind: str, word: tuple, radius: int, window: int) -> Pass:
	L = len(word)
	cost, pred, edges, ties, spread = _dp(word, radius, window)
	replaced = tuple((i, j, d) for i, j, d in edges if 0 <= d < j - i)
	new = {}
	todo = [(i, j) for i, j, d in replaced if d > 0]
	if todo:
		for (i, j), w in zip(todo, _words_for(kind, radius, np.stack([effect(word[i:j]) for i, j in todo]))):
			new[i, j] = w
	out = []
	for i, j, d in edges:
		if d < 0 or d >= j - i:
			out += word[i:j]
		elif d > 0:
			assert len(new[i, j]) == d
			out += new[i, j]
	assert len(out) == cost[L] <= L
	return Pass(tuple(out), int(cost[L]), pred, replaced, ties, spread)


def one_pass(kind: str, word, radius: int, window: int = None) -> Pass:
	"""One pass of the kind's model (shorten_model.one_pass, symshorten_model.one_pass) over `word`, kept per argument tuple."""
	word = tuple(int(a) for a in word)
	if len(word) > LIMIT or any(not 0 <= a < 12 for a in word):
		raise ValueError("a word is at most 4096 actions 0..11")
	W = max(len(word), 1) if window is None else int(window)
	if W < 1:
		raise ValueError("window < 1")
	return _one_pass(kind, word, radius, min(W, max(len(word), 1)))


def shorten(kind: str, word, radius: int, window: int = None, passes: int = None) -> tuple:
	"""Passes until one does not reduce the length, or `passes` of them: shorten_model.shorten's loop."""
	word = tuple(int(a) for a in word)
	done = 0
	while passes is None or done < passes:
		new = one_pass(kind, word, radius, window).word
		done += 1
		shorter = len(new) < len(word)
		word = new
		if not shorter:
			break
	return word


# ---- the words: every one has exactly 4 096 moves ---------------------------------------------------------------------------------

def _pad(word: list, n: int, rng) -> list:
	"""`word` with effect-free pieces -- a move and its opposite, or a move four times -- put in at seeded places until it has n
	moves.  Every such piece is even, so n - len(word) has to be."""
	word = list(word)
	assert len(word) <= n and (n - len(word)) % 2 == 0
	while len(word) < n:
		a, at = int(rng.randint(0, 12)), int(rng.randint(0, len(word) + 1))
		word[at:at] = [a] * 4 if n - len(word) >= 4 and rng.randint(0, 2) else [a, rev(a)]
	return word


@functools.lru_cache(maxsize=None)
def collapse(depth: int, seed: int = 11) -> tuple:
	"""A word whose whole window (0, 4 096) lies exactly `depth` (0 or 4) moves from solved and is the ONLY cheapest way through
	it, so that one pass at radius 4 replaces the single edge (0, 4 096).

	A scramble with detours put into it (shorten_model.detour_word alone) cannot be that word: it still passes through the states
	along the scramble, and at every state g with dist(g) + dist(g -> X) = dist(X) the split there costs as little as the whole
	window; the DP then takes the largest i and the word falls apart into short edges.  So the word leaves solved by a move `a`
	that leads away from X, the state of a seeded scramble of `depth` moves, and arrives by a move `m` from a state further from
	solved than X; in between it goes 40 seeded moves R away from everything, spends its length there on detour_word's detours of
	nothing (an empty scramble inflated to just under what is left, then padded with effect-free pieces at seeded places), comes
	back by inverse(R) and takes a shortest word G for what remains:  a + R + detours + inverse(R) + G + m.  That no split ties is
	not argued here: tests/test_shorten_limits_cpu.py asserts it on the reference."""
	assert depth in (0, 4)
	rng = np.random.RandomState(seed)
	ball = plain_ball(4)
	if depth == 0:
		a = int(rng.randint(0, 12))
		m, G, X = rev(a), [], orc.SOLVED.astype(np.int8)
	else:
		while True:                                                    # a scramble at exactly `depth`, left and reached the long way round
			s = [int(v) for v in rng.randint(0, 12, depth)]
			X = effect(s)
			away = [a for a in range(12) if ball_model.depth(ball, effect([rev(a)] + s)) < 0]
			back = [m for m in range(12) if ball_model.depth(ball, effect(s + [rev(m)])) < 0]
			if ball_model.depth(ball, X) != depth or not away or not back:
				continue
			a, m = int(rng.choice(away)), int(rng.choice(back))
			rest = effect([rev(a)] + s + [rev(m)])                        # a G m = X
			G = inverse(ball_model.search(rest, ball).queue)             # the queue solves `rest`; its inverse reaches it
			# no state on the way a, a G[:1], .., a G lies on a shortest way to X (a state outside the ball is further than 4)
			sides = [(ball_model.depth(ball, effect([a] + G[:k])), ball_model.depth(ball, effect(G[k:] + [m]))) for k in range(len(G) + 1)]
			if all(near < 0 or far < 0 or near + far > depth for near, far in sides):
				break
	R = [int(v) for v in rng.randint(0, 12, 40)]
	room = LIMIT - 2 - 2 * len(R) - len(G)
	detours = _pad(detour_word(seed + 1, 0, room - 16), room, rng)       # detour_word stops at most 11 moves past its target
	word = [a] + R + detours + inverse(R) + G + [m]
	assert len(word) == LIMIT and (effect(word) == X).all()
	return tuple(word)


@functools.lru_cache(maxsize=None)
def nested(seed: int = 23) -> tuple:
	"""Blocks w + inverse(w) of seeded lengths 70-120 (s), 260-400 (m) and about 1 000 (b) between stretches of a 30-move
	scramble's detour word: held windows of those spans, in a word far outside the ball.  Some blocks follow one another with
	only a pair of commuting turns in between ([2, 0] or [0, 2]: one state, two shortest words).  At the end of such a pair, and
	of the block behind it, the start of the block in front ties with a nearer start: the ties lie a whole block apart."""
	rng = np.random.RandomState(seed)

	def block(lo: int, hi: int) -> list:
		w = [int(a) for a in rng.randint(0, 12, int(rng.randint(lo, hi + 1)) // 2)]
		return w + inverse(w)

	s, m, b = (70, 120), (260, 400), (980, 1020)
	layout = ["-", s, "-", m, [2, 0], s, "-", b, [0, 2], m, "-", s, [0, 2], s, [2, 0], m, "-"]
	parts = [block(*x) if isinstance(x, tuple) else x for x in layout]
	fixed = sum(len(x) for x in parts if x != "-")
	stretch = detour_word(seed + 1, 30, LIMIT - fixed - 16)
	stretch = _pad(stretch, LIMIT - fixed, rng)
	gaps = layout.count("-")
	cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(40, len(stretch) - 40), gaps - 1, replace=False)) + [len(stretch)]
	pieces = iter(stretch[lo:hi] for lo, hi in zip(cuts, cuts[1:]))
	word = [a for x in parts for a in (next(pieces) if x == "-" else x)]
	assert len(word) == LIMIT
	return tuple(word)


@functools.lru_cache(maxsize=None)
def incompressible(seed: int = 37) -> tuple:
	"""Any seeded word: with windows of one move nothing can be taken away."""
	return tuple(int(a) for a in np.random.RandomState(seed).randint(0, 12, LIMIT))
