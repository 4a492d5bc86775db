"""
The two-phase search WITH A CAP on the phase-2 bound (rk_twophase_solve_capped, `DeviceTwoPhaseSolver(phase2_cap=C)`) restated in
NumPy: the search of tests/twophase_model.py with its two changed conditions -- a phase-1 solution whose phase-2 entry h2 is not 0
is left behind if p1 + h2 >= best OR h2 > C; after D2 += 1 phase 1 goes on if p1 + D2 >= best OR D2 > C -- and with the two counts
per state the engine reports: phase-1 solutions found, phase-2 searches entered.  Tables, coordinates, the move-pruning rule and
the helpers are tests/twophase_model.py's, which stays as it is; the loop is restated here because the conditions sit inside it.
A helper for tests/test_twophase_cap_*.py, not a test module; it shares no code with the library.
"""
import numpy as np

from tests import chain_model as CM
from tests import twophase_model as T
from tests.twophase_model import BUDGET, DONE, IMPROVED, SEARCH, SOL1

NO_CAP = 1 << 30                                                  # a bound no phase 2 reaches


def solve(states20, tries, max_nodes, cap=None, trace=None):
	"""(lengths, actions (n, chain max_length) padded with -1, phase lengths (n, 2), reason, nodes, counts (n, 2) = phase-1 solutions
	found and phase-2 searches entered) of LEGAL states; `cap` None: no cap.  `trace`, a dict, gets per state what only the cap's two
	conditions decided: "first_rejected" = the first phase-1 solution was left behind by h2 > C alone, "gave_up" = the phase-2
	searches left by D2 > C alone, "improved_after" = the state improved from a later phase-1 word after such a search."""
	C = NO_CAP if cap is None else int(cap)
	states = np.asarray(states20, np.int64).reshape(-1, 20)
	n = len(states)
	L, out_act, stages = CM.solve(states)
	out_act = out_act.copy()
	mt = [T.move_table(w) for w in range(6)]
	pr = [T.table(t).astype(np.int64) for t in range(4)]
	allow = T._allowed_table()
	z = lambda: np.zeros(n, np.int64)
	root = [T.coordinate(w, states) for w in range(3)]
	c = [r.copy() for r in root]
	D = np.maximum(pr[0][root[0] * 495 + root[2]], pr[1][root[1] * 495 + root[2]])
	best, bp1 = L.astype(np.int64).copy(), (stages[:, 0] + stages[:, 1]).astype(np.int64)
	phase, depth, cost, g, D2, p1, found, flags, nodes, entered = z() + 1, z(), z(), z(), z(), z(), z(), z(), z(), z()
	leaf, root2 = [z(), z(), z()], [z(), z(), z()]
	stack = np.zeros((n, T.STACK), np.int64)
	first_rejected, gave_up, improved_after, gave_up_at = np.zeros(n, bool), z(), np.zeros(n, bool), z() - 1
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
				root2[w][i] = T.coordinate(3 + w, x)
			h2 = np.maximum(pr[2][root2[0][i] * 24 + root2[2][i]], pr[3][root2[1][i] * 24 + root2[2][i]])
			solved = i[h2 == 0]
			for q in solved:
				best[q] = bp1[q] = p1[q]
				flags[q] |= IMPROVED
				write_row(q, int(p1[q]))
			mode[solved] = DONE
			left = (p1[i] + h2 >= best[i]) | (h2 > C)                    # the cap's first condition
			first_rejected[i[(h2 != 0) & (found[i] == 1) & (p1[i] + h2 < best[i]) & (h2 > C)]] = True
			resume1(i[(h2 != 0) & left])
			go = (h2 != 0) & ~left
			j = i[go]
			entered[j] += 1
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
		back = (p1[o2] + D2[o2] >= best[o2]) | (D2[o2] > C)               # the cap's second condition
		by_cap = o2[(p1[o2] + D2[o2] < best[o2]) & (D2[o2] > C)]
		gave_up[by_cap] += 1
		gave_up_at[by_cap] = found[by_cap]
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
		a = np.where(child_j, T._LOWEST[mask[s]], last[s])
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
			improved_after[q] |= 0 <= gave_up_at[q] < found[q]
			write_row(q, int(p1[q] + depth[q]))
		resume1(won)
	if trace is not None:
		trace.update(first_rejected=first_rejected, gave_up=gave_up, improved_after=improved_after)
	reason = np.where(flags & IMPROVED == 0, 2, np.where(flags & BUDGET != 0, 1, 0))
	return best, out_act, np.stack([bp1, best - bp1], axis=1), reason, nodes, np.stack([found, entered], axis=1)
