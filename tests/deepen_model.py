"""
The depth-first probes past the symmetry ball (engines rk_sdeepen and rk_sdeepen_*) restated in NumPy on top of
tests/sym_model.py: the words and their ranks, DeviceSymBall.solve_beyond, and how DeviceSymBallSearch(deepen=E) goes on from
the newest complete level of a pool that is full.  A helper for tests/test_deepen_*.py, not a test module.

Words.  A word of `extra` moves behind the action `last` (-1: none) is a sequence of actions 0..11 in which no action is the
opposite turn (a ^ 1) of the one before it; "before the first" is `last`.  Words are ranked in lexicographic order of their
actions, rank 0 first: the rank is a number whose digit k counts the allowed actions below action k -- 11 per place, 12 in the
first place of a word with no last action.

solve_beyond.  A state whose orbit the ball holds gets sym_model.solve's answer.  Any other runs rounds e = 1..extra: EVERY
word of e moves is applied, and a word hits when the ball holds the representative of the moved state.  The first round with a
hit answers: the lowest word that hits, then sym_model.solve's descent from the moved state.

The frontier continuation.  The own pool is symsearch_model's, popped one node at a time, and a pop runs only while 12 more
states fit (len + 12 <= capacity); when one does not, the search is out of memory.  The frontier is the newest complete level of
that pool, in index order, each node with the action stored for it as its last move (none for the start).  Rounds e = 1..E: the
LOWEST FRONTIER NODE that has a word of e moves that hits, THEN ITS LOWEST WORD.  The queue is the path to the node, the word,
the descent.  Round e is tried for every node of the frontier before any word of e + 1 moves.

Membership is decided by the symmetry ball (sym_model.depth).  To look at millions of moved states, they are first compared, by a
64-bit mix of their bytes, with the raw states of the plain ball of the same radius (tests/ball_model.py) -- a state lies in the
plain ball exactly when the symmetry ball holds its representative, which tests/test_deepen_cpu.py checks again --; equal states
have equal mixes, so no hit is lost, and every candidate is then decided by sym_model.depth.  The LAST move of a word is not
carried out for every word: s . a lies in the plain ball exactly when s is a ball state moved by the opposite turn of a, so the
state before the last move is compared with those 12 sets; a candidate is then moved and decided like any other.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import c_oracle
from oracle import cube_oracle as orc
from tests import ball_model
from tests import sym_model

BLOCK = 1 << 21                                   # moved states held at once
_MIX = np.array([0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93, 0xFF51AFD7ED558CCD], np.uint64)

Continued = namedtuple("Continued", "result queue len level frontier deepened node rank states parents actions")


# ---- words and ranks ----------------------------------------------------------------------------------------------------------
def word_count(extra: int, last: int = -1) -> int:
	return (12 if last < 0 else 11) * 11 ** (extra - 1)


def word_of(rank: int, extra: int, last: int = -1) -> list:
	assert 0 <= rank < word_count(extra, last)
	out, prev = [], last
	for k in range(extra):
		digit, rank = divmod(rank, 11 ** (extra - 1 - k))
		prev = digit if prev < 0 else digit + (digit >= (prev ^ 1))
		out.append(int(prev))
	return out


def words_of(ranks: np.ndarray, extra: int, last: np.ndarray) -> np.ndarray:
	"""word_of for many: int64 (n, extra)"""
	rem, prev = np.array(ranks, np.int64), np.array(last, np.int64)
	out = np.empty((len(rem), extra), np.int64)
	for k in range(extra):
		digit, rem = np.divmod(rem, 11 ** (extra - 1 - k))
		out[:, k] = prev = np.where(prev < 0, digit, digit + (digit >= (prev ^ 1)))
	return out


def rank_of(word, last: int = -1) -> int:
	rank, prev = 0, last
	for a in word:
		assert 0 <= a < 12 and (prev < 0 or a != (prev ^ 1))
		rank = rank * 11 + (a if prev < 0 else a - (a > (prev ^ 1)))
		prev = a
	return rank


# ---- every word of a round, applied --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_mixes(radius: int) -> tuple:
	"""Per action a: the sorted mixes of the plain ball's states moved by a ^ 1 -- the states that a takes into the ball."""
	ball = ball_model.build(radius).states
	return tuple(np.unique(_mix(c_oracle.multi_rotate(ball, np.full(len(ball), a ^ 1, np.uint8)))) for a in range(12))


def _mix(states20: np.ndarray) -> np.ndarray:
	with np.errstate(over="ignore"):
		return (np.ascontiguousarray(states20, np.int8).view("<u4").astype(np.uint64) * _MIX).sum(axis=1, dtype=np.uint64)


def _one_more_move(states, prev, owner, rank):
	"""Every allowed action applied to every row, rows and actions in order: the ranks stay in lexicographic order per owner."""
	a = np.tile(np.arange(12), len(states))
	p = np.repeat(prev, 12)
	keep = (p < 0) | (a != (p ^ 1))
	a, p = a[keep], p[keep]
	digit = np.where(p < 0, a, a - (a > (p ^ 1)))
	moved = c_oracle.multi_rotate(np.repeat(states, 12, axis=0)[keep], a.astype(np.uint8))
	return moved, a, np.repeat(owner, 12)[keep], np.repeat(rank, 12)[keep] * 11 + digit


def _by_state(states20: np.ndarray, fn) -> np.ndarray:
	"""fn of every row, computed once per distinct state (the states on a small ball's surface repeat a great deal)."""
	keys = np.ascontiguousarray(states20, np.int8).view("V20").reshape(-1)
	uniq, back = np.unique(keys, return_inverse=True)
	return fn(uniq.view(np.int8).reshape(-1, 20))[back.reshape(-1)]


def lowest_hits(ball: sym_model.SymBall, states20: np.ndarray, last: np.ndarray, extra: int, first_only: bool = False) -> np.ndarray:
	"""int64 (n,): the lowest rank of a word of `extra` moves from each state that hits the ball, -1 when none does.  `first_only`:
	states behind the first one with a hit may be left at -1 (the states are taken in order, a block at a time)."""
	states20 = np.ascontiguousarray(states20, np.int8).reshape(-1, 20)
	n = len(states20)
	best = np.full(n, -1, np.int64)
	mixes = _plain_mixes(ball.radius)
	per = max(1, BLOCK // (12 * 11 ** (extra - 1)))
	for at in range(0, n, per):
		s, prev = states20[at:at + per], np.asarray(last[at:at + per], np.int64)
		owner, rank = np.arange(at, at + len(s)), np.zeros(len(s), np.int64)
		for _ in range(extra - 1):
			s, prev, owner, rank = _one_more_move(s, prev, owner, rank)
		mix = _mix(s)
		rows, acts = [], []
		for a in range(12):                                   # the last move: only where it may lead into the ball
			r = np.nonzero(((prev < 0) | (prev != (a ^ 1))) & np.isin(mix, mixes[a]))[0]
			rows.append(r)
			acts.append(np.full(len(r), a))
		rows, acts = np.concatenate(rows), np.concatenate(acts)
		if len(rows):
			moved = c_oracle.multi_rotate(s[rows], acts.astype(np.uint8))
			held = _by_state(moved, lambda u: sym_model.depth(ball, u) >= 0)
			rows, acts = rows[held], acts[held]
			p = prev[rows]
			lowest = np.full(n, np.iinfo(np.int64).max)
			np.minimum.at(lowest, owner[rows], rank[rows] * 11 + np.where(p < 0, acts, acts - (acts > (p ^ 1))))
			best[lowest < np.iinfo(np.int64).max] = lowest[lowest < np.iinfo(np.int64).max]
		cand = rows
		if first_only and len(cand):
			break
	return best


def solve_beyond(ball: sym_model.SymBall, states20: np.ndarray, extra: int, last=None):
	"""(lengths int64 (n,), actions int64 (n, extra + radius) padded with -1)"""
	x = np.ascontiguousarray(states20, np.int8).reshape(-1, 20)
	n = len(x)
	last = np.full(n, -1, np.int64) if last is None else np.asarray(last, np.int64)
	lengths, actions = np.full(n, -1, np.int64), np.full((n, extra + ball.radius), -1, np.int64)
	got, word = sym_model.solve(ball, x)
	lengths[:] = got
	actions[:, :ball.radius] = word
	todo = np.nonzero(lengths < 0)[0]
	for e in range(1, extra + 1):
		if not len(todo):
			break
		rank = lowest_hits(ball, x[todo], last[todo], e)
		hit = todo[rank >= 0]
		if len(hit):
			w = words_of(rank[rank >= 0], e, last[hit])
			moved = x[hit]
			for k in range(e):
				moved = c_oracle.multi_rotate(moved, w[:, k].astype(np.uint8))
			both = _by_state(moved, lambda u: np.concatenate([c[:, None] if c.ndim == 1 else c for c in sym_model.solve(ball, u)], axis=1))
			down, tail = both[:, 0], both[:, 1:]
			assert (down == ball.radius).all()                # a first hit lies on the ball's surface
			lengths[hit] = e + down
			actions[hit, :e] = w
			actions[hit, e:e + ball.radius] = tail
		todo = todo[rank < 0]
	return lengths, actions


# ---- from the newest complete level of a full pool ----------------------------------------------------------------------------
def pool_until_full(start20: np.ndarray, ball: sym_model.SymBall, capacity: int):
	"""(Result or None, keys, parents, actions, (lo, hi), level): symsearch_model's pool, popped while 12 more states fit.  A
	Result when the search meets the ball first -- then nothing is continued."""
	from tests import symsearch_model
	keys = [None, np.ascontiguousarray(start20, np.int8).reshape(20).tobytes()]
	parents, actions = [0, 0], [-1, -1]
	if sym_model.depth(ball, np.frombuffer(keys[1], np.int8)[None])[0] >= 0:
		return symsearch_model.search(start20, ball)[0], keys, parents, actions, (1, 1), 0
	index = {keys[1]: 1}
	lo, hi, level = 1, 1, 0
	while True:
		new_lo = len(keys)
		for p in range(lo, hi + 1):
			if len(keys) - 1 + 12 > capacity:
				return None, keys, parents, actions, (lo, hi), level
			kids = c_oracle.expand12(np.frombuffer(keys[p], np.int8)[None].copy())[0]
			held = sym_model.depth(ball, kids)
			for a in range(12):
				k = kids[a].tobytes()
				if k in index:
					continue
				if held[a] >= 0:
					return symsearch_model.search(start20, ball)[0], keys, parents, actions, (lo, hi), level
				keys.append(k); parents.append(p); actions.append(a)
				index[k] = len(keys) - 1
		lo, hi, level = new_lo, len(keys) - 1, level + 1
		assert hi >= lo


def continue_from_frontier(start20: np.ndarray, ball: sym_model.SymBall, capacity: int, extra: int) -> Continued:
	"""What DeviceSymBallSearch(ball, capacity=max_capacity=capacity, deepen=extra).search(start20) leaves behind."""
	met, keys, parents, actions, (lo, hi), level = pool_until_full(start20, ball, capacity)
	n = len(keys) - 1
	arrays = (np.frombuffer(b"".join(keys[1:]), np.int8).reshape(n, 20).copy(), np.array(parents[1:], np.int64), np.array(actions[1:], np.int64))
	if met is not None:
		return Continued(met.result, met.queue, met.len, met.depth, None, 0, None, None, met.states, met.parents, met.actions)
	frontier = np.arange(lo, hi + 1)
	states, last = arrays[0][frontier - 1], arrays[2][frontier - 1]
	for e in range(1, extra + 1):
		rank = lowest_hits(ball, states, last, e, first_only=True)
		with_hit = np.nonzero(rank >= 0)[0]
		if len(with_hit):
			k = int(with_hit[0])                              # the lowest frontier node that has a hit ...
			node, r = int(frontier[k]), int(rank[k])          # ... then its lowest word
			path, i = [], node
			while parents[i]:
				path.append(actions[i])
				i = parents[i]
			w = word_of(r, e, int(last[k]))
			down, tail = sym_model.solve(ball, ball_model.apply(states[k], w)[None])
			queue = path[::-1] + w + [int(a) for a in tail[0, :down[0]]]
			return Continued(True, queue, n, level, (lo, hi), e, node, r, *arrays)
	return Continued(False, [], n, level, (lo, hi), 0, None, None, *arrays)
