"""
The cube group on 20-byte states (engine rk_group_*: apply, inverse, relative, is_legal) restated in plain NumPy over the oracle's
move table: what the library has to reproduce bit for bit.  A helper for tests/test_group_*.py, not a test module; it shares no code
with the library.

A move permutes all 24 sticker slots of a kind (corner slot 3 * pos + k, edge slot 2 * pos + k).  A state b reached from solved by a
word has the full action g_b = the product of the word's moves on the slots, and b[c] = g_b(home slot of c).
    apply(a, b)[c] = g_b(a[c])        inverse(b): apply(b, inverse(b)) = solved        relative(s, goal) = apply(inverse(goal), s)

The tables.  The library walks every cubie on its own over the 12 actions.  Here the full actions of WORDS seeded random words (0 to
40 moves) are computed whole, as 24-permutations, and read off: full[kind][p][g(stride p)][k] = g(stride p + k).  Every entry must
get the same value from every word that reaches it, and every entry must be reached.  inv[kind][p][v] is the slot stride p + k that
full sends to the primary slot of v's position.

The corner twist tau is not typed in either.  Every reachable state has sum_c tau(s[c]) = 0 mod 3 and tau is 0 on the home codes:
a homogeneous linear system over Z3 in the 16 other slots, one equation per word.  Its solutions must be a line {0, tau, -tau} (the
invariant is unique up to sign); tau is the one with tau(slot 1) = 1.  is_legal: codes in range, both position lists permutations
of equal parity, an even number of flipped edges, twists that add up to 0 mod 3.
"""
import functools

import numpy as np

from oracle import cube_oracle as orc

WORDS = 4096
STRIDE = (3, 2)
HOMES = (8, 12)
HOME = np.concatenate([3 * np.arange(8), 2 * np.arange(12)])


def word_actions(seed: int, n: int, longest: int = 40):
	"""(lengths (n,), actions (n, longest)) of n seeded words, lengths 0..longest in turn."""
	rng = np.random.RandomState(seed)
	return np.arange(n) % (longest + 1), rng.randint(0, 12, (n, longest))


def full_actions(lengths: np.ndarray, actions: np.ndarray) -> np.ndarray:
	"""int64 (n, 2, 24): the product of every word's moves on the corner slots and on the edge slots."""
	n = len(lengths)
	g = np.tile(np.arange(24), (n, 2, 1))
	for t in range(actions.shape[1]):
		live = lengths > t
		for kind in range(2):
			moved = orc.LUT[actions[:, t][:, None], kind, g[:, kind]]
			g[:, kind] = np.where(live[:, None], moved, g[:, kind])
	return g


def states_of(g: np.ndarray) -> np.ndarray:
	"""The 20-byte states of full actions: where every cubie's primary sticker went."""
	return np.concatenate([g[:, 0, 3 * np.arange(8)], g[:, 1, 2 * np.arange(12)]], axis=1).astype(np.int8)


def _solve_mod3(rows: np.ndarray) -> np.ndarray:
	"""A basis (k, m) of the null space over Z3 of the integer matrix `rows` (n, m)."""
	a = np.unique(rows % 3, axis=0).astype(np.int64)
	m = a.shape[1]
	pivots, r = [], 0
	for col in range(m):
		hit = np.nonzero(a[r:, col])[0]
		if len(hit) == 0:
			continue
		a[[r, r + hit[0]]] = a[[r + hit[0], r]]
		a[r] = a[r] * a[r, col] % 3                              # 1 and 2 are their own inverses mod 3
		for i in range(len(a)):
			if i != r and a[i, col]:
				a[i] = (a[i] - a[i, col] * a[r]) % 3
		pivots.append(col)
		r += 1
		if r == len(a):
			break
	free = [c for c in range(m) if c not in pivots]
	basis = np.zeros((len(free), m), np.int64)
	for k, f in enumerate(free):
		basis[k, f] = 1
		for i, p in enumerate(pivots):
			basis[k, p] = -a[i, f] % 3
	return basis


@functools.lru_cache(maxsize=None)
def tables():
	"""(full uint8 (2, 12, 24, 3), inv uint8 (2, 12, 24), tau uint8 (24,)) in the layout of rk_group_tables."""
	g = full_actions(*word_actions(77_001, WORDS))
	full = np.full((2, 12, 24, 3), -1, np.int64)
	for kind in range(2):
		n = STRIDE[kind]
		for p in range(HOMES[kind]):
			v = g[:, kind, n * p]
			for k in range(n):
				got = g[:, kind, n * p + k]
				for code in range(24):
					vals = np.unique(got[v == code])
					assert len(vals) == 1, (kind, p, code, k, vals)       # reached, and the same from every word
					full[kind, p, code, k] = vals[0]
	inv = np.zeros((2, 12, 24), np.int64)
	for kind in range(2):
		n = STRIDE[kind]
		for p in range(HOMES[kind]):
			for code in range(24):
				slots = full[kind, p, code, :n]
				assert sorted(slots) == list(range(code // n * n, code // n * n + n))     # a cubie's stickers fill one position
				inv[kind, p, code] = n * p + int(np.nonzero(slots == code // n * n)[0][0])
	assert (full[1, :, :, 0] == np.arange(24)).all() and (full[1, :, :, 1] == np.arange(24) ^ 1).all()    # g_b(2 p + k) = b[p] ^ k
	# tau: the null space of "the twists of a reachable state add up to 0", in the slots that are no home code
	unknown = [v for v in range(24) if v % 3]
	counts = np.zeros((len(g), 24), np.int64)
	np.add.at(counts, (np.arange(len(g))[:, None], g[:, 0, 3 * np.arange(8)]), 1)
	basis = _solve_mod3(counts[:, unknown])
	assert len(basis) == 1, len(basis)                                        # unique up to sign
	line = basis[0] * (1 if basis[0][unknown.index(1)] == 1 else 2) % 3
	assert line[unknown.index(1)] == 1
	tau = np.zeros(24, np.int64)
	tau[unknown] = line
	assert not (counts @ tau % 3).any()
	full[full < 0] = 0
	return full.astype(np.uint8), inv.astype(np.uint8), tau.astype(np.uint8)


def _rows(states) -> np.ndarray:
	return np.asarray(states, np.int64).reshape(-1, 20)


def full_action_of(states) -> np.ndarray:
	"""int64 (n, 2, 24): g_b of legal states b, from the tables."""
	b = _rows(states)
	full = tables()[0].astype(np.int64)
	g = np.zeros((len(b), 2, 24), np.int64)
	for kind in range(2):
		n = STRIDE[kind]
		for p in range(HOMES[kind]):
			for k in range(n):
				g[:, kind, n * p + k] = full[kind, p, b[:, 8 * kind + p], k]
	return g


def apply(states, effects) -> np.ndarray:
	"""apply(a, b)[c] = g_b(a[c]); `effects`: one state or one for each."""
	a, b = _rows(states), _rows(effects)
	if len(b) == 1:
		b = np.repeat(b, len(a), axis=0)
	g = full_action_of(b)
	out = np.empty((len(a), 20), np.int8)
	out[:, :8] = np.take_along_axis(g[:, 0], a[:, :8], axis=1)
	out[:, 8:] = np.take_along_axis(g[:, 1], a[:, 8:], axis=1)
	return out


def inverse(states) -> np.ndarray:
	"""The state whose full action is the inverse permutation of g_b."""
	g = full_action_of(states)
	back = np.argsort(g, axis=2)
	return states_of(back)


def relative(states, goals) -> np.ndarray:
	s, goal = _rows(states), _rows(goals)
	if len(goal) == 1:
		goal = np.repeat(goal, len(s), axis=0)
	return apply(inverse(goal), s)


def _odd(perm: np.ndarray) -> np.ndarray:
	"""(n,) bool: the parity of every row of (n, m) permutations, by counting inversions."""
	m = perm.shape[1]
	upper = np.triu(np.ones((m, m), bool), 1)
	return ((perm[:, :, None] > perm[:, None, :]) & upper).sum(axis=(1, 2)) % 2 == 1


def is_legal(states) -> np.ndarray:
	"""(n,) bool: reachable from solved.  Rows of any bytes (read as uint8)."""
	x = np.asarray(states, np.int8).reshape(-1, 20).view(np.uint8).astype(np.int64)
	tau = tables()[2].astype(np.int64)
	ok = (x < 24).all(axis=1)
	safe = np.where(x < 24, x, 0)
	cpos, epos = safe[:, :8] // 3, safe[:, 8:] // 2
	ok &= (np.sort(cpos, axis=1) == np.arange(8)).all(axis=1)
	ok &= (np.sort(epos, axis=1) == np.arange(12)).all(axis=1)
	ok &= _odd(cpos) == _odd(epos)
	ok &= (safe[:, 8:] % 2).sum(axis=1) % 2 == 0
	ok &= tau[safe[:, :8]].sum(axis=1) % 3 == 0
	return ok


def variants(state) -> np.ndarray:
	"""int8 (12, 20): corner 0 twisted by 0 / 1 / 2 in place, edge 0 flipped or not, edges 0 and 1 swapped or not; row 0 is `state`."""
	s = np.asarray(state, np.int8).reshape(20)
	out = []
	for twist in range(3):
		for flip in range(2):
			for swap in range(2):
				v = s.copy()
				v[0] = v[0] // 3 * 3 + (v[0] % 3 + twist) % 3
				v[8] ^= flip
				if swap:
					v[8], v[9] = v[9], v[8]
				out.append(v)
	return np.stack(out)
