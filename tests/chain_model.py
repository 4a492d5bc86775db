"""
The subgroup chain (engine rk_chain_*, `DeviceChainSolver`) restated in NumPy and plain Python over the oracle's move table:
signatures, the four tables by a dictionary search over signatures, the table indices and the descent.  A helper for
tests/test_chain_*.py, not a test module; it shares no code with the library.

Faces are FBTDLR, action 2 f / 2 f + 1 the two directions of face f.  position = code // 3 (edges // 2), digit = code % 3 (% 2).
Everything below is read off the move table: which faces change an edge's digit or take a corner's digit off 0, the three slices (the edges
that neither face of an axis moves), the generators of each stage and the corner permutations C3 of the half-turn group.

    stage  generators, ascending by first action (cost)           signature
    1      the 12 quarter turns (1)                               edge digit BY POSITION, 12 bits
    2      faces that flip no edge: both turns (1); the           corner digit by position, 8 x 2 bits; the positions that hold
           others: the half turn 2f 2f (2)                        the edges of the slice of the axis that changes no digit
    3      faces that keep both digits 0: both turns (1);        the least sequence among P o h, h in C3, P = the position of
           others: half turns (2)                                 corner cubie 0..7; the positions that hold the edges of the
                                                                  slice of the axis that flips edges
    4      the six half turns (2)                                 P; for each slice the place, within the slice, of each of its edges

THE INDEX of a signature in a stage's table (this is what the engine is compared against byte for byte):
    1  sum over positions p = 0..10 of digit(p) << p                                                            2^11
    2  (sum over p = 0..6 of digit(p) 3^p) * 495 + ordinal of the position set among the 4-subsets of 0..11       3^7 * 495
    3  coset ordinal * 70 + ordinal of the set among the 4-subsets of 0..7, the positions outside stage 2's       420 * 70
       slice counted ascending
    4  ((ordinal of P in C3 * 24 + q_0) * 24 + q_1) * 24 + q_2, q_s the ordinal of slice s's places               96 * 24^3
Subsets are ordered by their largest element, then the next (itertools.combinations sorted by the reversed tuple); sequences
lexicographically (itertools.permutations); cosets and C3 by their least sequence.  Slices: 0 = the axis that changes no
digit, 1 = the axis that flips edges, 2 = the third.  Nothing here computes a rank by arithmetic: ordinals are looked up in
enumerations.
"""
import functools
import itertools

import numpy as np

from oracle import cube_oracle as orc

UNREACHED = 255
COUNTS = (2048, 1082565, 29400, 663552)
SIZES = (2048, 3 ** 7 * 495, 420 * 70, 96 * 24 ** 3)


# ---- read off the move table ------------------------------------------------------------------------------------------------
def _moved_edges(f):
	return {e for e in range(12) if orc.LUT[2 * f, 1, 2 * e] != 2 * e}


FLIPS = tuple(bool((orc.LUT[2 * f, 1, np.arange(24)] % 2 != np.arange(24) % 2).any()) for f in range(6))
# (a corner's digit 1 and 2 change places under every face that moves it; what some faces keep is the digit 0, the goal of stage 2)
TWISTS = tuple(bool((orc.LUT[2 * f, 0, 3 * np.arange(8)] % 3 != 0).any()) for f in range(6))


def _axes():
	"""The three pairs of opposite faces (no edge in common), as (slice 0's axis, slice 1's, slice 2's)."""
	pairs = [(f, g) for f in range(6) for g in range(f + 1, 6) if not _moved_edges(f) & _moved_edges(g)]
	assert len(pairs) == 3
	plain = [p for p in pairs if not FLIPS[p[0]] and not TWISTS[p[0]]]
	flip = [p for p in pairs if FLIPS[p[0]]]
	rest = [p for p in pairs if p not in plain + flip]
	assert len(plain) == len(flip) == len(rest) == 1
	for f, g in pairs:
		assert FLIPS[f] == FLIPS[g] and TWISTS[f] == TWISTS[g]
	return plain[0], flip[0], rest[0]


AXES = _axes()
SLICES = tuple(tuple(sorted(set(range(12)) - _moved_edges(f) - _moved_edges(g))) for f, g in AXES)
assert all(len(s) == 4 for s in SLICES) and sorted(sum(SLICES, ())) == list(range(12))
OUTSIDE0 = tuple(p for p in range(12) if p not in SLICES[0])               # stage 3 counts positions among these


def _generators(quarter):
	out = []
	for f in range(6):
		out += [(2 * f,), (2 * f + 1,)] if quarter(f) else [(2 * f, 2 * f)]
	return tuple(out)


GENERATORS = (
	_generators(lambda f: True),
	_generators(lambda f: not FLIPS[f]),
	_generators(lambda f: not FLIPS[f] and not TWISTS[f]),
	_generators(lambda f: False),
)


def move(states, action):
	"""int64 (n, 20) after one action (an int, or one per row)."""
	a = np.broadcast_to(np.asarray(action, np.int64).reshape(-1, 1), (len(states), 1))
	out = np.empty_like(states)
	out[:, :8] = orc.LUT[a, 0, states[:, :8]]
	out[:, 8:] = orc.LUT[a, 1, states[:, 8:]]
	return out


def apply_generator(states, gen):
	for a in gen:
		states = move(states, a)
	return states


SOLVED = orc.SOLVED.astype(np.int64).reshape(1, 20)


@functools.lru_cache(None)
def c3():
	"""The corner sequences P (position of cubie 0..7) of the half-turn group, sorted: a closure from solved."""
	seen = {tuple(range(8))}
	todo = [SOLVED]
	while todo:
		s = todo.pop()
		for gen in GENERATORS[3]:
			t = apply_generator(s, gen)
			key = tuple(int(v) for v in t[0, :8] // 3)
			if key not in seen:
				seen.add(key)
				todo.append(t)
	return np.array(sorted(seen), np.int64)


def _pack8(seq):
	"""sequences of eight values 0..7 as one number whose order is the lexicographic one"""
	out = np.zeros(seq.shape[:-1], np.int64)
	for i in range(8):
		out = out * 8 + seq[..., i]
	return out


def coset_least(P):
	"""int64 (n,): the least of the sequences P o h, h in C3, packed."""
	return _pack8(P[:, c3()]).min(axis=1)


# ---- signatures: one int64 per state ------------------------------------------------------------------------------------------
def _position_set(states, cubies):
	return (1 << (states[:, [8 + e for e in cubies]] // 2)).sum(axis=1)


def signature(stage, states):
	states = np.asarray(states, np.int64).reshape(-1, 20)
	c, e = states[:, :8], states[:, 8:]
	if stage == 0:
		return ((e % 2) << (e // 2)).sum(axis=1)
	if stage == 1:
		return ((c % 3) << (2 * (c // 3))).sum(axis=1) | _position_set(states, SLICES[0]) << 16
	if stage == 2:
		return coset_least(c // 3) << 12 | _position_set(states, SLICES[1])
	key = _pack8(c // 3)
	for s in SLICES:
		place = np.searchsorted(np.array(s), e[:, list(s)] // 2)                 # within the slice; meaningful in the half-turn group
		for i in range(4):
			key = key << 2 | (place[:, i] & 3)
	return key


# ---- ordinals by enumeration -------------------------------------------------------------------------------------------------
def _subset_ordinals(n):
	"""int64 (2^n,): the ordinal of a 4-subset of 0..n-1 given as a bit set, -1 elsewhere"""
	out = np.full(1 << n, -1, np.int64)
	for i, t in enumerate(sorted(itertools.combinations(range(n), 4), key=lambda t: t[::-1])):
		out[sum(1 << p for p in t)] = i
	return out


@functools.lru_cache(None)
def _ordinals():
	sub12, sub8 = _subset_ordinals(12), _subset_ordinals(8)
	places = np.full(256, -1, np.int64)
	for i, t in enumerate(itertools.permutations(range(4))):
		places[t[0] << 6 | t[1] << 4 | t[2] << 2 | t[3]] = i
	every = np.array(list(itertools.permutations(range(8))), np.int64)
	least = np.unique(coset_least(every))
	return sub12, sub8, places, least, _pack8(c3())


def coset_count():
	return len(_ordinals()[3])


def index(stage, sig):
	"""The table index of signatures (int64 array)."""
	sig = np.asarray(sig, np.int64)
	sub12, sub8, places, least, group = _ordinals()
	if stage == 0:
		return sig & 2047
	if stage == 1:
		ori = sum(((sig >> (2 * p)) & 3) * 3 ** p for p in range(7))
		return ori * 495 + sub12[sig >> 16]
	if stage == 2:
		at = sig & 4095
		narrow = sum(((at >> p) & 1) << i for i, p in enumerate(OUTSIDE0))
		return np.searchsorted(least, sig >> 12) * 70 + sub8[narrow]
	out = np.searchsorted(group, sig >> 24)
	for s in range(3):
		out = out * 24 + places[(sig >> (8 * (2 - s))) & 255]
	return out


# ---- the tables -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def search(stage):
	"""{signature: cost from the stage's goal}: level d + 1 takes the cost-1 children of level d and the cost-2 children of
	level d - 1 that no earlier level holds; one representative state per signature."""
	goal = int(signature(stage, SOLVED)[0])
	dist = {goal: 0}
	levels = [SOLVED]                                                          # representatives by level
	while len(levels[-1]) or (len(levels) > 1 and len(levels[-2])):
		d = len(levels)
		children = [apply_generator(levels[d - len(gen)], gen) for gen in GENERATORS[stage] if d - len(gen) >= 0]
		children = np.concatenate(children) if children else np.zeros((0, 20), np.int64)
		sigs = signature(stage, children)
		sigs, first = np.unique(sigs, return_index=True)
		fresh = []
		for i, s in zip(first.tolist(), sigs.tolist()):
			if s not in dist:
				dist[s] = d
				fresh.append(i)
		levels.append(children[fresh])
	return dist


@functools.lru_cache(None)
def table(stage):
	"""uint8 (SIZES[stage],): the cost of every index, 255 where no signature has it."""
	dist = search(stage)
	sigs = np.fromiter(dist.keys(), np.int64, len(dist))
	t = np.full(SIZES[stage], UNREACHED, np.uint8)
	at = index(stage, sigs)
	assert len(np.unique(at)) == len(at) and at.min() >= 0 and at.max() < SIZES[stage]
	t[at] = np.fromiter(dist.values(), np.int64, len(dist))
	return t


def max_depths():
	return tuple(int(table(s)[table(s) != UNREACHED].max()) for s in range(4))


def max_length():
	return sum(max_depths())


# ---- the descent ---------------------------------------------------------------------------------------------------------------
def solve(states20):
	"""(lengths (n,), actions (n, max_length) padded with -1, stage lengths (n, 4)) of legal states: per stage, at each step the
	lowest generator whose entry equals the current entry minus its cost."""
	states = np.asarray(states20, np.int64).reshape(-1, 20).copy()
	n, width = len(states), max_length()
	actions = np.full((n, width), -1, np.int64)
	at = np.zeros(n, np.int64)
	stage_lengths = np.zeros((n, 4), np.int64)
	for stage in range(4):
		t = table(stage).astype(np.int64)
		cur = t[index(stage, signature(stage, states))]
		assert (cur != UNREACHED).all()
		stage_lengths[:, stage] = cur
		live = np.nonzero(cur > 0)[0]
		gens = GENERATORS[stage]
		while len(live):
			pick = np.full(len(live), -1, np.int64)
			for g in range(len(gens) - 1, -1, -1):
				child = t[index(stage, signature(stage, apply_generator(states[live], gens[g])))]
				pick[child + len(gens[g]) == cur[live]] = g
			assert (pick >= 0).all()
			for g, gen in enumerate(gens):
				m = live[pick == g]
				if len(m):
					states[m] = apply_generator(states[m], gen)
					for a in gen:
						actions[m, at[m]] = a
						at[m] += 1
					cur[m] -= len(gen)
			live = live[cur[live] > 0]
	assert (states == SOLVED).all()
	return at, actions, stage_lengths
