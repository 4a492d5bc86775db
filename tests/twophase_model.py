"""
The two-phase search (engine rk_twophase_*, `DeviceTwoPhaseSolver`) restated in NumPy over the oracle's move table: the six
coordinates, their move tables, the four pruning tables, the move-pruning rule, the budget rule and the `tries` loop.  A helper for
tests/test_twophase_*.py, not a test module; it shares no code with the library.  Launch 1, the chain's answer, is the model of
tests/chain_model.py.  All states advance in lock-step, one child, pop or restart per state and trip, as the kernel's lanes do.

Coordinates (position = code // 3, edges // 2; all BY POSITION, ordinals looked up in enumerations):
    phase 1   twist, slice = divmod(the chain's stage-2 index, 495)       flip = the chain's stage-1 index
    phase 2   corners = the ordinal of P = (position of corner cubie 0..7) among the permutations, lexicographic
              edges   = the ordinal of (place of the i-th edge outside slice 0 among the positions outside slice 0)
              places  = the ordinal of (place of slice 0's i-th edge within slice 0)
Tables 1..4: twist * 495 + slice, flip * 495 + slice (the 12 quarter turns, cost 1), corners * 24 + places, edges * 24 + places
(the chain's stage-3 generators: F F' B B' cost 1, TT DD LL RR cost 2).
"""
import functools
import itertools

import numpy as np

from tests import chain_model as CM

COUNTS = (1082565, 1013760, 967680, 967680)
SIZES = (2187 * 495, 2048 * 495, 40320 * 24, 40320 * 24)
STACK = 72
GENERATORS = (CM.GENERATORS[0], CM.GENERATORS[2])                # phase 1: the 12 actions; phase 2: 8 generators
assert [g[0] for g in GENERATORS[1]] == [0, 1, 2, 3, 4, 6, 8, 10] and [len(g) for g in GENERATORS[1]] == [1, 1, 1, 1, 2, 2, 2, 2]
ROWS = (2187, 2048, 495, 40320, 40320, 24)
SEARCH, SOL1, DONE = 0, 1, 2
IMPROVED, BUDGET = 1, 2


@functools.lru_cache(None)
def _perm_ordinals(k):
	"""sorted packed sequences of 0..k-1 (base 8): the ordinal of a sequence is its place here"""
	return np.array([functools.reduce(lambda a, v: a * 8 + v, t, 0) for t in itertools.permutations(range(k))], np.int64)


def _pack(seq):
	out = np.zeros(len(seq), np.int64)
	for i in range(seq.shape[1]):
		out = out * 8 + seq[:, i]
	return out


def coordinate(which, states):
	states = np.asarray(states, np.int64).reshape(-1, 20)
	c, e = states[:, :8], states[:, 8:]
	if which in (0, 2):
		i1 = CM.index(1, CM.signature(1, states))
		return i1 // 495 if which == 0 else i1 % 495
	if which == 1:
		return CM.index(0, CM.signature(0, states))
	if which == 3:
		return np.searchsorted(_perm_ordinals(8), _pack(c // 3))
	if which == 4:
		return np.searchsorted(_perm_ordinals(8), _pack(np.searchsorted(np.array(CM.OUTSIDE0), e[:, list(CM.OUTSIDE0)] // 2)))
	return np.searchsorted(_perm_ordinals(4), _pack(np.searchsorted(np.array(CM.SLICES[0]), e[:, list(CM.SLICES[0])] // 2)))


def table_index(table, states):
	a, b = ((0, 2), (1, 2), (3, 5), (4, 5))[table]
	return coordinate(a, states) * (495 if table < 2 else 24) + coordinate(b, states)


@functools.lru_cache(None)
def move_table(which):
	"""int64 (ROWS[which], generators): the coordinate after each generator, from one representative state per value found by a
	closure from solved."""
	gens, size = GENERATORS[which >= 3], ROWS[which]
	reps, have = np.zeros((size, 20), np.int64), np.zeros(size, bool)
	level = CM.SOLVED
	v = coordinate(which, level)
	reps[v], have[v] = level, True
	while len(level):
		children = np.concatenate([CM.apply_generator(level, gen) for gen in gens])
		v, first = np.unique(coordinate(which, children), return_index=True)
		new = ~have[v]
		reps[v[new]], have[v[new]] = children[first[new]], True
		level = children[first[new]]
	assert have.all()
	return np.stack([coordinate(which, CM.apply_generator(reps, gen)) for gen in gens], axis=1)


@functools.lru_cache(None)
def table(t):
	"""uint8 (SIZES[t],): level d + 1 takes the cost-1 children of level d and the cost-2 children of level d - 1 that no earlier
	level holds."""
	a, b = ((0, 2), (1, 2), (3, 5), (4, 5))[t]
	K, gens = (495 if t < 2 else 24), GENERATORS[t >= 2]
	ma, mb = move_table(a), move_table(b)
	out = np.full(SIZES[t], 255, np.uint8)
	goal = table_index(t, CM.SOLVED)
	out[goal] = 0
	levels = [goal]
	while len(levels[-1]) or (len(levels) > 1 and len(levels[-2])):
		d = len(levels)
		kids = [ma[levels[d - len(gen)] // K, col] * K + mb[levels[d - len(gen)] % K, col] for col, gen in enumerate(gens) if d - len(gen) >= 0]
		kids = np.unique(np.concatenate(kids)) if kids else np.zeros(0, np.int64)
		kids = kids[out[kids] == 255]
		out[kids] = d
		levels.append(kids)
	return out


def deepest():
	return tuple(int(table(t).max()) for t in range(4))


# ---- the move-pruning rule -------------------------------------------------------------------------------------------------------
def allowed(phase, last, last2):
	"""the bit set of the actions that may follow `last` (255: none before) in `phase`"""
	mask = 0xFFF if phase == 1 else 0x55F
	if last != 255:
		mask &= ~(1 << (last ^ 1))
		if (last >> 1) & 1:
			mask &= ~(3 << (2 * ((last >> 1) - 1)))
		if last & 1 or last2 == last or (phase == 2 and last >= 4):
			mask &= ~(1 << last)
	return mask


@functools.lru_cache(None)
def _allowed_table():
	t = np.zeros((3, 256, 256), np.int64)
	for phase in (1, 2):
		for last in list(range(12)) + [255]:
			for last2 in list(range(12)) + [255]:
				t[phase, last, last2] = allowed(phase, last, last2)
	return t


_LOWEST = np.array([0] + [(m & -m).bit_length() - 1 for m in range(1, 4096)], np.int64)


# ---- the search -------------------------------------------------------------------------------------------------------------------
def solve(states20, tries, max_nodes):
	"""(lengths, actions (n, chain max_length) padded with -1, phase lengths (n, 2), reason, nodes) of LEGAL states."""
	states = np.asarray(states20, np.int64).reshape(-1, 20)
	n = len(states)
	L, out_act, stages = CM.solve(states)
	out_act = out_act.copy()
	mt = [move_table(w) for w in range(6)]
	pr = [table(t).astype(np.int64) for t in range(4)]
	allow = _allowed_table()
	z = lambda: np.zeros(n, np.int64)
	root = [coordinate(w, states) for w in range(3)]
	c = [r.copy() for r in root]
	D = np.maximum(pr[0][root[0] * 495 + root[2]], pr[1][root[1] * 495 + root[2]])
	best, bp1 = L.astype(np.int64).copy(), (stages[:, 0] + stages[:, 1]).astype(np.int64)
	phase, depth, cost, g, D2, p1, found, flags, nodes = z() + 1, z(), z(), z(), z(), z(), z(), z(), z()
	leaf, root2 = [z(), z(), z()], [z(), z(), z()]
	stack = np.zeros((n, STACK), np.int64)
	mode = np.where(D >= best, DONE, np.where(D == 0, SOL1, SEARCH))
	for w in range(3):
		leaf[w][:] = root[w]

	def set_c(i, src):
		for w in range(3):
			c[w][i] = src[w][i]

	def resume1(i):
		over = (found[i] == tries) | (D[i] >= best[i])
		mode[i[over]] = DONE
		i = i[~over]
		phase[i] = 1
		set_c(i, leaf)
		depth[i], cost[i], g[i], mode[i] = D[i], D[i], 12, SEARCH

	def write_row(q, entries):
		w = 0
		for e in range(entries):
			a = int(stack[q, e])
			out_act[q, w] = a
			w += 1
			if e >= p1[q] and a >= 4:
				out_act[q, w] = a
				w += 1
		out_act[q, w:] = -1
		assert w == best[q]

	while True:
		i = np.nonzero(mode == SOL1)[0]
		if len(i):
			found[i] += 1
			x = states[i].copy()
			for e in range(int(p1[i].max())):
				m = p1[i] > e
				x[m] = CM.move(x[m], stack[i[m], e])
			for w in range(3):
				root2[w][i] = coordinate(3 + w, x)
			h2 = np.maximum(pr[2][root2[0][i] * 24 + root2[2][i]], pr[3][root2[1][i] * 24 + root2[2][i]])
			solved = i[h2 == 0]
			for q in solved:
				best[q] = bp1[q] = p1[q]
				flags[q] |= IMPROVED
				write_row(q, int(p1[q]))
			mode[solved] = DONE
			resume1(i[(h2 != 0) & (p1[i] + h2 >= best[i])])
			go = (h2 != 0) & (p1[i] + h2 < best[i])
			j = i[go]
			phase[j] = 2
			set_c(j, root2)
			depth[j], cost[j], g[j], D2[j], mode[j] = 0, 0, 0, h2[go], SEARCH
		i = np.nonzero(mode == SEARCH)[0]
		if not len(i) and not (mode == SOL1).any():
			break
		if not len(i):
			continue
		two = phase[i] == 2
		base = np.where(two, p1[i], 0)
		last = np.where(depth[i] > 0, stack[i, np.maximum(base + depth[i] - 1, 0)], 255)
		last2 = np.where(depth[i] > 1, stack[i, np.maximum(base + depth[i] - 2, 0)], 255)
		mask = allow[phase[i], last, last2] & ~((1 << g[i]) - 1)
		has = mask != 0
		# the budget, before each child evaluation
		spent = has & (nodes[i] == max_nodes)
		flags[i[spent]] |= BUDGET
		mode[i[spent]] = DONE
		child = has & ~spent
		pop = ~has & (depth[i] > 0)
		over = ~has & (depth[i] == 0)
		# a bound is exhausted
		o2 = i[over & two]
		D2[o2] += 1
		back = p1[o2] + D2[o2] >= best[o2]
		resume1(o2[back])
		set_c(o2[~back], root2)
		g[o2[~back]] = 0
		o1 = i[over & ~two]
		D[o1] += 1
		end = D[o1] >= best[o1]
		mode[o1[end]] = DONE
		set_c(o1[~end], root)
		g[o1[~end]] = 0
		# a step through the move tables: a child, or a pop through the inverse generator
		s = child | pop
		j, two_j, child_j = i[s], two[s], child[s]
		if not len(j):
			continue
		a = np.where(child_j, _LOWEST[mask[s]], last[s])
		act = np.where(child_j, a, np.where(two_j & (a >= 4), a, a ^ 1))
		col = np.where(two_j & (act >= 4), 2 + act // 2, act)
		new = [np.where(two_j, mt[3 + w][np.where(two_j, c[w][j], 0), np.minimum(col, 7)], mt[w][np.where(two_j, 0, c[w][j]), col]) for w in range(3)]
		ca = np.where(two_j & (a >= 4), 2, 1)
		k = j[~child_j]
		for w in range(3):
			c[w][k] = new[w][~child_j]
		depth[k] -= 1
		cost[k] -= ca[~child_j]
		g[k] = a[~child_j] + 1
		k, a, ca, two_k = j[child_j], a[child_j], ca[child_j], two_j[child_j]
		new = [v[child_j] for v in new]
		nodes[k] += 1
		K = np.where(two_k, 24, 495)
		h = np.where(two_k, np.maximum(pr[2][np.where(two_k, new[0] * K + new[2], 0)], pr[3][np.where(two_k, new[1] * K + new[2], 0)]),
		             np.maximum(pr[0][np.where(two_k, 0, new[0] * K + new[2])], pr[1][np.where(two_k, 0, new[1] * K + new[2])]))
		fits = cost[k] + ca + h <= np.where(two_k, D2[k], D[k])
		g[k[~fits]] = a[~fits] + 1
		k, a, ca, two_k, h = k[fits], a[fits], ca[fits], two_k[fits], h[fits]
		stack[k, np.where(two_k, p1[k], 0) + depth[k]] = a
		for w in range(3):
			c[w][k] = new[w][fits]
		depth[k] += 1
		cost[k] += ca
		g[k] = 0
		s1 = k[~two_k & (cost[k] == D[k])]
		p1[s1] = D[s1]
		for w in range(3):
			leaf[w][s1] = c[w][s1]
		mode[s1] = SOL1
		won = k[two_k & (h == 0)]
		for q in won:
			best[q] = p1[q] + cost[q]
			bp1[q] = p1[q]
			flags[q] |= IMPROVED
			write_row(q, int(p1[q] + depth[q]))
		resume1(won)
	reason = np.where(flags & IMPROVED == 0, 2, np.where(flags & BUDGET != 0, 1, 0))
	return best, out_act, np.stack([bp1, best - bp1], axis=1), reason, nodes


# ---- brute force, independent of the tables above --------------------------------------------------------------------------------
def coset_key(states):
	"""what names a state's coset of the subgroup: edge digits, corner digits and slice 0's positions, all by position"""
	return list(zip(CM.signature(0, states).tolist(), CM.signature(1, states).tolist()))


@functools.lru_cache(None)
def coset_distances(depth=4):
	"""{coset key: quarter turns from the subgroup}, breadth-first to `depth`, one representative per coset"""
	dist = {coset_key(CM.SOLVED)[0]: 0}
	level = CM.SOLVED
	for d in range(1, depth + 1):
		children = np.concatenate([CM.move(level, a) for a in range(12)])
		fresh = []
		for i, k in enumerate(coset_key(children)):
			if k not in dist:
				dist[k] = d
				fresh.append(i)
		level = children[fresh]
	return dist


@functools.lru_cache(None)
def subgroup_states(max_cost=6):
	"""(states int64 (m, 20), cost (m,)): every state the phase-2 generators reach from solved at cost <= max_cost, with its exact
	cost, by levels over whole states"""
	seen = {tuple(CM.SOLVED[0].tolist()): 0}
	levels = [CM.SOLVED]
	for d in range(1, max_cost + 1):
		children = np.concatenate([CM.apply_generator(levels[d - len(gen)], gen) for gen in GENERATORS[1] if d - len(gen) >= 0])
		fresh = []
		for i, k in enumerate(map(tuple, children.tolist())):
			if k not in seen:
				seen[k] = d
				fresh.append(i)
		levels.append(children[fresh])
	return np.concatenate(levels), np.concatenate([np.full(len(l), d, np.int64) for d, l in enumerate(levels)])


def scrambles(seed, depths):
	"""one seeded scramble per entry of `depths`, int8 (n, 20)"""
	from oracle import cube_oracle as orc
	rs, want = np.random.RandomState(seed), np.asarray(depths)
	s = orc.repeat_state(orc.SOLVED, len(want))
	for d in range(int(want.max())):
		moved = orc.multi_rotate(s, rs.randint(0, 6, len(want)), rs.randint(0, 2, len(want)))
		s = np.where((want > d)[:, None], moved, s)
	return s.astype(np.int8)


def replay(states20, lengths, actions):
	"""the states after their queues, by the model's move"""
	s = np.asarray(states20, np.int64).reshape(-1, 20).copy()
	for t in range(actions.shape[1]):
		live = np.nonzero(lengths > t)[0]
		if len(live):
			s[live] = CM.move(s[live], actions[live, t])
	return s
