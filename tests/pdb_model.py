"""
Pattern databases (engine rk_pdb_*, `DevicePatternDB`) restated in plain NumPy over the oracle's move table: the index of the
selected codes, its inverse, the table by level sweeps and the descent.  A helper for tests/test_pdb_*.py, not a test module; it
shares no code with the library.

A pattern selects kc corner cubies (0..7) and ke edge cubies (0..11), ascending.  With position = code // 3 (edges: // 2) and
digit = code % 3 (edges: % 2), over the selected cubies of a kind in order (N = 8 or 12):
    r = 0; for i: d_i = p_i - #{j < i : p_j < p_i}; r = r * (N - i) + d_i
    o = 0; for i: o = o * 3 + digit_i  (edges: * 2);  with all 8 corners the last corner's digit is left out
    index = ((r_c * O_c + o_c) * P(12, ke) + r_e) * 2^ke + o_e
Unranking all eight corners recovers the last digit from sum tau(code) = 0 mod 3; tau comes from tests/group_model.py, which
derives it from the oracle's move table as the one invariant of its kind.

`dictionary_bfs` is the yardstick of the model itself: a breadth-first search over tuples of codes that uses none of the ranking.
"""
import numpy as np

from oracle import cube_oracle as orc

UNREACHED = 255


def _falling(n: int, k: int) -> int:
	out = 1
	for i in range(k):
		out *= n - i
	return out


class Pattern:
	def __init__(self, corners=(), edges=()):
		self.corners, self.edges = tuple(sorted(corners)), tuple(sorted(edges))
		self.kc, self.ke = len(self.corners), len(self.edges)
		assert self.kc + self.ke >= 1 and self.ke <= 10
		assert all(0 <= c < 8 for c in self.corners) and all(0 <= e < 12 for e in self.edges)
		self.oc_digits = 7 if self.kc == 8 else self.kc
		self.Pc, self.Oc = _falling(8, self.kc), 3 ** self.oc_digits
		self.Pe, self.Oe = _falling(12, self.ke), 2 ** self.ke
		self.size = self.Pc * self.Oc * self.Pe * self.Oe
		self.columns = np.array(list(self.corners) + [8 + e for e in self.edges], np.intp)     # of a 20-byte row
		self.goal = np.array([3 * c for c in self.corners] + [2 * e for e in self.edges], np.int64)

	# -- codes: int64 (n, kc + ke), the selected corner codes then the selected edge codes --
	def select(self, states20) -> np.ndarray:
		return np.asarray(states20).reshape(-1, 20)[:, self.columns].astype(np.int64)

	def valid(self, codes) -> np.ndarray:
		"""bool (n,): every code in 0..23 and no two selected cubies of a kind on one position."""
		ok = ((codes >= 0) & (codes < 24)).all(axis=1)
		for part, stride in ((codes[:, :self.kc], 3), (codes[:, self.kc:], 2)):
			pos = part // stride
			for i in range(part.shape[1]):
				for j in range(i):
					ok &= pos[:, i] != pos[:, j]
		return ok

	def move(self, codes, action) -> np.ndarray:
		"""The codes after one action (an int, or one per row)."""
		a = np.broadcast_to(np.asarray(action, np.int64).reshape(-1, 1), (len(codes), 1))
		out = np.empty_like(codes)
		out[:, :self.kc] = orc.LUT[a, 0, codes[:, :self.kc]]
		out[:, self.kc:] = orc.LUT[a, 1, codes[:, self.kc:]]
		return out

	@staticmethod
	def _perm_rank(pos, N):
		r = np.zeros(len(pos), np.int64)
		for i in range(pos.shape[1]):
			d = pos[:, i] - (pos[:, :i] < pos[:, i:i + 1]).sum(axis=1)
			r = r * (N - i) + d
		return r

	def rank(self, codes) -> np.ndarray:
		codes = np.asarray(codes, np.int64)
		c, e = codes[:, :self.kc], codes[:, self.kc:]
		rc, re = self._perm_rank(c // 3, 8), self._perm_rank(e // 2, 12)
		oc = np.zeros(len(codes), np.int64)
		for i in range(self.oc_digits):
			oc = oc * 3 + c[:, i] % 3
		oe = np.zeros(len(codes), np.int64)
		for i in range(self.ke):
			oe = oe * 2 + e[:, i] % 2
		return ((rc * self.Oc + oc) * self.Pe + re) * self.Oe + oe

	@staticmethod
	def _perm_unrank(r, N, k):
		r = r.copy()
		digits = np.zeros((len(r), k), np.int64)
		for i in range(k - 1, -1, -1):
			r, digits[:, i] = np.divmod(r, N - i)
		free = np.ones((len(r), N), bool)
		pos = np.zeros((len(r), k), np.int64)
		rows = np.arange(len(r))
		for i in range(k):
			pos[:, i] = np.argmax(np.cumsum(free, axis=1) == (digits[:, i] + 1)[:, None], axis=1)      # the d-th free position
			free[rows, pos[:, i]] = False
		return pos

	def unrank(self, index) -> np.ndarray:
		x = np.asarray(index, np.int64).reshape(-1)
		x, oe = np.divmod(x, self.Oe)
		x, re = np.divmod(x, self.Pe)
		rc, oc = np.divmod(x, self.Oc)
		codes = np.zeros((len(x), self.kc + self.ke), np.int64)
		pc, pe = self._perm_unrank(rc, 8, self.kc), self._perm_unrank(re, 12, self.ke)
		for i in range(self.ke - 1, -1, -1):
			oe, bit = np.divmod(oe, 2)
			codes[:, self.kc + i] = 2 * pe[:, i] + bit
		for i in range(self.oc_digits - 1, -1, -1):
			oc, digit = np.divmod(oc, 3)
			codes[:, i] = 3 * pc[:, i] + digit
		if self.kc == 8:
			from tests import group_model
			tau = group_model.tables()[2].astype(np.int64)
			twist = tau[codes[:, :7]].sum(axis=1) % 3
			last = np.full(len(x), -1, np.int64)
			for k in range(3):
				cand = 3 * pc[:, 7] + k
				last = np.where((twist + tau[cand]) % 3 == 0, cand, last)
			assert (last >= 0).all()
			codes[:, 7] = last
		return codes

	# -- the table and the descent --
	def table(self):
		"""(uint8 (size,), level sizes): breadth-first distances from the goal by level sweeps."""
		t = np.full(self.size, UNREACHED, np.uint8)
		t[self.rank(self.goal[None])] = 0
		sizes = []
		for d in range(UNREACHED):
			at = np.nonzero(t == d)[0]
			if len(at) == 0:
				break
			sizes.append(len(at))
			codes = self.unrank(at)
			for a in range(12):
				child = self.rank(self.move(codes, a))
				t[child[t[child] == UNREACHED]] = d + 1
		return t, np.array(sizes, np.int64)

	def depth(self, table, states20) -> np.ndarray:
		codes = self.select(states20)
		ok = self.valid(codes)
		out = np.full(len(codes), -1, np.int64)
		out[ok] = table[self.rank(codes[ok])]
		return out

	def solve(self, table, states20, max_depth: int):
		"""(lengths (n,), actions (n, max_depth)) padded with -1: at each step the lowest action whose child's entry is one less."""
		codes = self.select(states20)
		ok = self.valid(codes)
		lengths = self.depth(table, states20)
		actions = np.full((len(codes), max_depth), -1, np.int64)
		codes = np.where(ok[:, None], codes, self.goal[None])
		cur = np.where(ok, lengths, 0)
		for t in range(max_depth):
			live = cur > 0
			if not live.any():
				break
			pick = np.full(len(codes), -1, np.int64)
			for a in range(11, -1, -1):
				nearer = table[self.rank(self.move(codes, a))].astype(np.int64) == cur - 1
				pick = np.where(live & nearer, a, pick)
			assert (pick[live] >= 0).all()
			actions[live, t] = pick[live]
			codes = np.where(live[:, None], self.move(codes, np.where(live, pick, 0)), codes)
			cur = cur - live
		return lengths, actions


def dictionary_bfs(pattern, limit=None) -> dict:
	"""tuple of the selected codes -> distance from the goal, moving the tuples through the oracle's table alone"""
	kind = np.array([0] * pattern.kc + [1] * pattern.ke)
	goal = tuple(int(v) for v in pattern.goal)
	dist, frontier, d = {goal: 0}, np.array([goal], np.int64), 0
	while len(frontier) and (limit is None or d < limit):
		d += 1
		fresh = []
		for a in range(12):
			for t in map(tuple, orc.LUT[a, kind[None, :], frontier].tolist()):
				if t not in dist:
					dist[t] = d
					fresh.append(t)
		frontier = np.array(fresh, np.int64).reshape(-1, len(goal))
	return dist
