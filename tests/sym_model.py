"""
The 48 whole-cube symmetries, canonical representatives and the symmetry-reduced goal ball of DeviceSymBall (engines rk_sym_* and
rk_symball_*) restated in plain Python / NumPy over the oracle's move table: what the library has to reproduce bit for bit.  A
helper for tests/test_sym_*.py, not a test module.

The symmetries.  The faces are F B T D L R = 2 * axis + side.  Symmetry s = 8 * p + m sends axis `ax` to PERMS[p][ax] and swaps
the two faces of (source) axis `ax` when bit `ax` of m is set; s = 0 is the identity.  A symmetry relabels the actions: a turn of
face f becomes a turn of the image face, in the same sense for a rotation and in the opposite sense for a reflection.  Nothing
else is assumed: which sense it is, which cubie goes where (src) and how a cubie's code is re-coded (M) come out of the move table
alone -- the relabelling w -> pi(w) of move sequences is an automorphism of the cube group, so the code v = W(home of c') that a
sequence W gives cubie c' determines the code pi(W)(home of c) of its image cubie c, and a breadth-first walk over the 12 moves
from the two home codes fills the 24 entries of M[c] and contradicts itself for every c that is not the image.  (The library
derives its tables the other way round, from the faces a cubie lies on.)
    conj_S(x)[c] = M[S][c][x[src[S][c]]]            conj_S(rotate(x, a)) = rotate(conj_S(x), pi_S(a))

canonical(x): the smallest conjugate, compared as the tuple of its five little-endian dwords, the lowest symmetry that gives it,
and 48 / (the number of symmetries that give it) = the size of x's orbit.

The ball of representatives.  Node 1 is the solved state.  A level's representatives are popped in index order, their children
taken in action order 0..11 and canonicalised; a representative the pool holds (an earlier child of the level included) is
skipped, every other is appended.  Level `radius` is stored and never expanded.  depth(x) is the level of canonical(x); solve(x)
descends: at every step the lowest action whose child is one level nearer.
"""
import functools
import itertools
from collections import namedtuple

import numpy as np

from oracle import cube_oracle as orc

N_SYM = 48
PERMS = tuple(itertools.permutations(range(3)))      # lexicographic: 012 021 102 120 201 210
HOME = np.concatenate([3 * np.arange(8), 2 * np.arange(12)])
KIND_OF = orc.KIND

SymBall = namedtuple("SymBall", "radius len level_start states covered index")


def face_map(s: int) -> list:
	p, m = PERMS[s // 8], s % 8
	return [2 * p[f // 2] + ((f % 2) ^ ((m >> (f // 2)) & 1)) for f in range(6)]


def _relabel(s: int, mirror: int) -> list:
	phi = face_map(s)
	return [2 * phi[a // 2] + ((a % 2) ^ mirror) for a in range(12)]


def _walk(pi, kind: int, v0: int, w0: int):
	"""The map M with M[v0] = w0 and M[lut[a][v]] = lut[pi[a]][M[v]], or None if two paths disagree."""
	lut = orc.LUT
	M = {v0: w0}
	todo = [v0]
	while todo:
		v = todo.pop()
		for a in range(12):
			v2, w2 = int(lut[a, kind, v]), int(lut[pi[a], kind, M[v]])
			if v2 not in M:
				M[v2] = w2
				todo.append(v2)
			elif M[v2] != w2:
				return None
	return [M[v] for v in range(24)] if len(M) == 24 else None


def _derive(pi):
	"""(src (20,), M (20, 24)) of the relabelling pi, or None if it is no symmetry of the cube."""
	src, maps = [None] * 20, [None] * 20
	for c_from in range(20):
		kind = int(KIND_OF[c_from])
		images = []
		for c in (range(8) if kind == 0 else range(8, 20)):
			M = _walk(pi, kind, int(HOME[c_from]), int(HOME[c]))
			if M is not None:
				images.append((c, M))
		if len(images) != 1 or src[images[0][0]] is not None:
			return None
		src[images[0][0]], maps[images[0][0]] = c_from, images[0][1]
	return src, maps


@functools.lru_cache(maxsize=None)
def tables():
	"""actions uint8 (48, 12), src uint8 (48, 20), M uint8 (48, 20, 24)."""
	act, src, M = np.zeros((N_SYM, 12), np.uint8), np.zeros((N_SYM, 20), np.uint8), np.zeros((N_SYM, 20, 24), np.uint8)
	for s in range(N_SYM):
		found = [(pi, d) for pi, d in ((pi, _derive(pi)) for pi in (_relabel(s, 0), _relabel(s, 1))) if d is not None]
		assert len(found) == 1, (s, len(found))
		act[s], src[s], M[s] = found[0][0], found[0][1][0], found[0][1][1]
	return act, src, M


def conjugate(states20: np.ndarray, s: int) -> np.ndarray:
	_, src, M = tables()
	x = np.asarray(states20, np.int8).reshape(-1, 20)
	return M[s][np.arange(20)[None, :], x[:, src[s]]].astype(np.int8)


def all_conjugates(states20: np.ndarray) -> np.ndarray:
	"""int8 (48, n, 20)"""
	_, src, M = tables()
	x = np.asarray(states20, np.int8).reshape(-1, 20)
	return M[np.arange(N_SYM)[:, None, None], np.arange(20)[None, None, :], x[:, src].transpose(1, 0, 2)].astype(np.int8)


def _keys(states20: np.ndarray) -> np.ndarray:
	"""(..., 5) uint32: the little-endian dwords"""
	return np.ascontiguousarray(states20, np.int8).view("<u4")


def canonical(states20: np.ndarray):
	"""(reps int8 (n, 20), syms int64 (n,), orbit sizes int64 (n,))"""
	conj = all_conjugates(states20)                       # (48, n, 20)
	n = conj.shape[1]
	if n == 0:
		return np.zeros((0, 20), np.int8), np.zeros(0, np.int64), np.zeros(0, np.int64)
	k = _keys(conj).astype(np.uint64)                     # (48, n, 5)
	best = np.zeros(n, np.int64)
	for s in range(1, N_SYM):                              # a strict improvement only: the lowest symmetry keeps a tie
		less = np.zeros(n, bool)
		tie = np.ones(n, bool)
		cur = k[best, np.arange(n)]
		for j in range(5):
			less |= tie & (k[s, :, j] < cur[:, j])
			tie &= k[s, :, j] == cur[:, j]
		best[less] = s
	reps = conj[best, np.arange(n)]
	same = (conj == reps[None]).all(axis=2).sum(axis=0)
	assert (48 % same == 0).all()
	return reps, best, 48 // same


def build(radius: int) -> SymBall:
	"""states (n, 20) int8 in index order (row i = node i + 1); covered[l] = the orbit sizes of level l added up"""
	keys = [None, orc.SOLVED.astype(np.int8).tobytes()]
	index = {keys[1]: 1}
	level_start, covered = [1, 2], [1]
	level = [1]
	for _ in range(radius):
		parents = np.frombuffer(b"".join(keys[p] for p in level), np.int8).reshape(-1, 20)
		reps, _, orbit = canonical(orc.expand12(parents))
		new, total = [], 0
		for r, o in zip(reps, orbit):
			k = r.tobytes()
			if k in index:
				continue
			keys.append(k)
			index[k] = len(keys) - 1
			new.append(len(keys) - 1)
			total += int(o)
		level = new
		level_start.append(len(keys))
		covered.append(total)
	n = len(keys) - 1
	return SymBall(radius, n, np.array(level_start, np.int64), np.frombuffer(b"".join(keys[1:]), np.int8).reshape(n, 20).copy(),
	               np.array(covered, np.int64), index)


def depth(ball: SymBall, states20: np.ndarray) -> np.ndarray:
	reps, _, _ = canonical(states20)
	nodes = np.array([ball.index.get(r.tobytes(), 0) for r in reps], np.int64)
	return np.where(nodes > 0, np.searchsorted(ball.level_start, nodes, side="right") - 1, -1)


def solve(ball: SymBall, states20: np.ndarray):
	"""(lengths int64 (n,), actions int64 (n, radius) padded with -1): the descent, the lowest action that gets nearer first"""
	x = np.array(np.asarray(states20, np.int8).reshape(-1, 20))
	n = len(x)
	d = depth(ball, x)
	lengths = d.copy()
	actions = np.full((n, ball.radius), -1, np.int64)
	for step in range(ball.radius):
		rows = np.nonzero(d > 0)[0]
		if not len(rows):
			break
		child_depth = depth(ball, orc.expand12(x[rows])).reshape(len(rows), 12)
		nearer = child_depth == (d[rows] - 1)[:, None]
		assert nearer.any(axis=1).all()
		a = nearer.argmax(axis=1)
		actions[rows, step] = a
		x[rows] = orc.multi_rotate(x[rows], a // 2, 1 - a % 2)
		d[rows] -= 1
	return lengths, actions
