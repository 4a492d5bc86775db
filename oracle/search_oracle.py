"""
CPU oracle for the search loops -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (rules: see cube_oracle.py).

A plain-Python/NumPy restatement of the reference's batch weighted A* (librubiks/solving/agents.py:171-413) and MCTS
(agents.py:415-645), written for clarity, one explicit loop per step of the reference's vectorised code.  Built on
oracle/cube_oracle.py for the cube arithmetic.

Parity status: PINNED.  tests/test_search_oracle.py replays the traces that oracle/gen_golden.py captured from the
UNMODIFIED reference agents (driven by the exact-integer stub net below) and requires identical node arrays,
pop order and action queues.
"""
from __future__ import annotations

import heapq
from collections import deque

import numpy as np

from oracle import cube_oracle as orc


class StubNet:
	"""
	Exact heuristic used for traces: value = -(number of cubies not on their solved code), policy logits zero.
	Works on NumPy or torch one-hot batches; returns the same container type.  All numbers are small integers in
	float32, so CPU and GPU agree bit for bit.
	"""
	def __init__(self):
		self.solved_oh = orc.as_oh(orc.SOLVED)[0]
		self._dev = {}                       # device -> solved one-hot tensor (no copies inside a graph capture)

	def eval(self):
		return self

	def __call__(self, x, policy=True, value=True):
		import torch
		is_torch = isinstance(x, torch.Tensor)
		if is_torch:
			if x.device not in self._dev:
				self._dev[x.device] = torch.from_numpy(self.solved_oh).to(x.device)
			sol = self._dev[x.device]
			v = -(20 - (x.float() * sol).sum(dim=1, keepdim=True))
			p = torch.zeros(len(x), 12, device=x.device)
		else:
			v = -(20 - (x * self.solved_oh).sum(axis=1, keepdims=True)).astype(np.float32)
			p = np.zeros((len(x), 12), np.float32)
		out = ([p] if policy else []) + ([v] if value else [])
		return out if len(out) > 1 else out[0]


class PolicyStubNet(StubNet):
	"""
	StubNet with a non-uniform policy that is exact on any hardware (the twin of gen_golden.py's PolicyStubNet): every
	logit is 0 or -inf, 8 finite ones when corner 0 has an even code and 4 when odd, so the softmax is exactly 0, 1/8
	or 1/4 whether an implementation divides by the sum or multiplies by its reciprocal.
	"""
	def __init__(self):
		super().__init__()
		t = np.zeros((24, 12), np.float32)
		for c in range(24):
			banned = [(c + 3 * j) % 12 for j in range(4)] if c % 2 == 0 else [(c + j) % 12 for j in range(8)]
			t[c, banned] = -np.inf
		self.table = t
		self._tab_dev = {}

	def __call__(self, x, policy=True, value=True):
		import torch
		out = []
		if policy:
			if isinstance(x, torch.Tensor):
				if x.device not in self._tab_dev:
					self._tab_dev[x.device] = torch.from_numpy(self.table).to(x.device)
				out.append(self._tab_dev[x.device][x[:, :24].float().argmax(dim=1)])
			else:
				out.append(self.table[x[:, :24].argmax(axis=1)])
		if value:
			out.append(super().__call__(x, policy=False, value=True))
		return out if len(out) > 1 else out[0]


class NoisyStubNet(StubNet):
	"""
	StubNet plus exact integer "noise": value = -(cubies off their solved code) + ((one-hot . w) mod 7) - 3 with a fixed vector
	of small integers w, so every number is a small integer in float32 on any hardware.  The noise misleads the search, which
	then reaches the goal over roundabout paths -- what the graph completion and the breadth-first shortening of MCTS
	(agents.py:597-633) need to have something to shorten.  Test infrastructure only.
	"""
	def __init__(self, seed: int = 0):
		super().__init__()
		self.w = np.random.RandomState(seed).randint(0, 50, 480).astype(np.float32)
		self._w_dev = {}

	def __call__(self, x, policy=True, value=True):
		import torch
		out = []
		if policy:
			out.append(torch.zeros(len(x), 12, device=x.device) if isinstance(x, torch.Tensor) else np.zeros((len(x), 12), np.float32))
		if value:
			base = super().__call__(x, policy=False, value=True)
			if isinstance(x, torch.Tensor):
				if x.device not in self._w_dev:
					self._w_dev[x.device] = torch.from_numpy(self.w).to(x.device)
				noise = torch.remainder((x.float() * self._w_dev[x.device]).sum(dim=1, keepdim=True), 7.0) - 3.0
			else:
				noise = (np.mod((x * self.w).sum(axis=1, keepdims=True), 7.0) - 3.0).astype(np.float32)
			out.append(base + noise)
		return out if len(out) > 1 else out[0]


def _round_bf16(a: np.ndarray) -> np.ndarray:
	"""float32 array rounded to the nearest bfloat16 (ties to even), returned as float32.  No NaN expected; +-inf stay."""
	u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
	u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
	return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


class LookupNet(StubNet):
	"""
	A net whose outputs are ARBITRARY float32 (or bfloat16) bit patterns and still the same bits on NumPy, torch-CPU and torch-GPU
	for any batch shape: h = (one-hot . w) mod M with small integer weights w (a sum of twenty integers below 2^24, exact in float32
	in any order, as in NoisyStubNet) and k = number of cubies off their solved code (StubNet's -value, 0..20) select one entry of
	tables made once on the host, and a gather copies bits.
	  value  = value_table[h, k], where value_table[h, k] = float32(float32(noise[h] + stub_weight * (-k)) + offset) with
	           noise ~ N(0, scale^2): StubNet's value scaled by `stub_weight` keeps the search going somewhere, the noise misleads it
	           (states are rediscovered over shorter ways: both relaxation passes of A* run), `offset` > 0 makes A* costs negative;
	  logits = logit_table[h], shape (M, 12): normal rows of scale 0.01 .. 20, and every third row a NEAR TIE: a maximum of magnitude
	           0.01 .. 20 and one logit a gap of 1 ulp .. 2^-16 below it at a lower or a higher index (`near_ties` lists them).
	Planted after that, whole rows of the value table (so they reach the output whatever k): exact duplicates, pairs one ulp apart
	(`dtype`'s ulp), +0.0 and -0.0; with `special` also float32 denormals, +-1e30, +inf and -inf.  No NaN anywhere: heapq on NaN
	tuples has no defined order.  dtype "bfloat16": both tables are rounded to bfloat16 once on the host; torch outputs are then
	bfloat16 tensors, NumPy outputs float32 arrays holding the same numbers.
	Test infrastructure only.
	"""
	M = 4093
	GAPS = (0.0, 2.0 ** -26, 2.0 ** -24, 2.0 ** -23, 2.0 ** -22, 2.0 ** -21, 1.5 * 2.0 ** -21, 2.0 ** -20, 1.5 * 2.0 ** -20, 2.0 ** -19,
	        1.5 * 2.0 ** -19, 2.0 ** -18, 2.0 ** -17, 2.0 ** -16)          # 0.0 stands for "one ulp of the maximum"
	MAGNITUDES = (0.01, 0.3, 3.0, 20.0)

	def __init__(self, seed: int = 0, scale: float = 3.0, offset: float = 0.0, dtype: str = "float32", special: bool = False,
	             stub_weight: float = 0.5):
		super().__init__()
		if dtype not in ("float32", "bfloat16"):
			raise ValueError('dtype is "float32" or "bfloat16"')
		self.dtype, self.special = dtype, bool(special)
		M = self.M
		rng = np.random.RandomState(seed)
		self.w = rng.randint(0, M, 480).astype(np.float32)
		noise = (rng.standard_normal(M) * scale).astype(np.float32)
		stub = (np.float32(stub_weight) * -np.arange(21, dtype=np.float32)).astype(np.float32)
		vt = ((noise[:, None] + stub[None, :]).astype(np.float32) + np.float32(offset)).astype(np.float32)
		# logits
		row_scale = np.array(self.MAGNITUDES, np.float32)[rng.randint(0, 4, M)]
		lt = (rng.standard_normal((M, 12)) * row_scale[:, None]).astype(np.float32)
		lt[1::97, 3] = lt[1::97, 7]                                     # exact ties in ordinary rows
		lt[2::101, 5] = 0.0
		lt[2::101, 6] = -0.0
		self.near_ties = []                                             # (h, index of the maximum, index of the runner-up)
		for h in range(0, M, 3):
			mag = self.MAGNITUDES[rng.randint(4)] * (1 + rng.rand())
			m = np.float32(mag if rng.rand() < 0.5 else -mag)
			gap = self.GAPS[rng.randint(len(self.GAPS))]
			j, i = rng.choice(12, 2, replace=False)
			row = (m - np.float32(1) - np.abs(rng.standard_normal(12))).astype(np.float32)
			row[j] = m
			row[i] = np.nextafter(m, np.float32(-np.inf)) if gap == 0.0 else np.float32(np.float64(m) - gap)
			lt[h] = row
			self.near_ties.append((h, int(j), int(i)))
		if dtype == "bfloat16":
			vt, lt = _round_bf16(vt), _round_bf16(lt)
		# planted rows of the value table
		pick = rng.permutation(M)
		step = np.uint32(1 << 16 if dtype == "bfloat16" else 1)
		vt[pick[0:64]] = vt[pick[64:128]]                               # exact duplicates
		vt[pick[128:192]] = (vt[pick[192:256]].view(np.uint32) + step).view(np.float32)      # one ulp further from zero
		vt[pick[256:264]] = 0.0
		vt[pick[264:272]] = -0.0
		self.planted = {"duplicates": (pick[0:64], pick[64:128]), "ulp_pairs": (pick[128:192], pick[192:256]),
		                "plus_zero": pick[256:264], "minus_zero": pick[264:272]}
		if self.special:
			values = [1e-40, -1e-40, 1.4e-45, -1.4e-45, 1e30, -1e30, np.inf, -np.inf]
			for n, v in enumerate(values):
				vt[pick[272 + 4 * n:276 + 4 * n]] = np.float32(v)
			self.planted["special"] = (pick[272:272 + 4 * len(values)], np.repeat(np.array(values, np.float32), 4))
			if dtype == "bfloat16":
				vt = _round_bf16(vt)
		assert not np.isnan(vt).any() and not np.isnan(lt).any()
		self.value_table = np.ascontiguousarray(vt.reshape(-1))         # entry 21 h + k
		self.logit_table = np.ascontiguousarray(lt)
		self._tables_dev = {}                                           # device -> (w, value table, logit table, solved one-hot)

	def _tables(self, device):
		import torch
		if device not in self._tables_dev:
			dt = torch.bfloat16 if self.dtype == "bfloat16" else torch.float32
			self._tables_dev[device] = (torch.from_numpy(self.w).to(device), torch.from_numpy(self.value_table).to(device).to(dt),
			                            torch.from_numpy(self.logit_table).to(device).to(dt), torch.from_numpy(self.solved_oh).to(device))
		return self._tables_dev[device]

	def rows(self, x):
		"""(h, k) of every row of a one-hot batch, as integer arrays (NumPy) or tensors (torch)."""
		import torch
		if isinstance(x, torch.Tensor):
			w, _, _, sol = self._tables(x.device)
			xf = x.float()
			h = torch.remainder((xf * w).sum(dim=1), float(self.M)).long()
			k = (20 - (xf * sol).sum(dim=1)).long()
		else:
			x = np.asarray(x, np.float32)
			h = np.mod((x * self.w).sum(axis=1), np.float32(self.M)).astype(np.int64)
			k = (20 - (x * self.solved_oh).sum(axis=1)).astype(np.int64)
		return h, k

	def __call__(self, x, policy=True, value=True):
		import torch
		h, k = self.rows(x)
		out = []
		if isinstance(x, torch.Tensor):
			_, vt, lt, _ = self._tables(x.device)
			if policy:
				out.append(lt[h])
			if value:
				out.append(vt[21 * h + k].reshape(-1, 1))
		else:
			if policy:
				out.append(self.logit_table[h])
			if value:
				out.append(self.value_table[21 * h + k].reshape(-1, 1))
		return out if len(out) > 1 else out[0]


def adi_traindata_oracle(net, games: int, depth: int, alpha: float, method: str):
	"""
	`Train.ADI_traindata` (train.py:256-339) on the CPU oracle: scramble (:277), 12-child fan-out (:285), rewards
	(:294-296), value of every child + reward (:303, :313), targets (:315-324), loss weights (:329-332).
	Pinned by tests/test_search_oracle.py against tests/golden/adi_trace.npz (captured from the unmodified reference).
	Returns (one-hot states float32 (n,480), policy int64 (n,), value float32 (n,), loss weights float32 (n,)).
	"""
	states, oh_states = orc.sequence_scrambler(games, depth, method == "lapanfix")
	solved_scrambled = orc.multi_is_solved(states)
	sub = orc.expand12(states)
	solved_sub = orc.multi_is_solved(sub)
	rewards = np.where(solved_sub, 0.0 if method == "reward0" else 1.0, -1.0).astype(np.float32)
	values = np.asarray(net(orc.as_oh(sub), policy=False, value=True), dtype=np.float32).reshape(-1) + rewards
	values = values.reshape(-1, 12)
	policy = values.argmax(axis=1)
	value = values[np.arange(len(values)), policy].copy()
	if method == "lapanfix":
		value[solved_scrambled] = 0
	elif method == "schultzfix":
		value[np.arange(0, len(states), depth)] = 0
	w = np.tile(1 / np.arange(1, depth + 1), games)
	u = np.ones_like(w)
	lw = ((1 - alpha) * w / w.sum() + alpha * u / len(u)) * (w.sum() + len(u))
	return oh_states, policy.astype(np.int64), value.astype(np.float32), lw.astype(np.float32)


def _values(net, states: np.ndarray) -> np.ndarray:
	"""float32 value vector of the net for a batch of 20-byte states."""
	v = net(orc.as_oh(states), policy=False, value=True)
	return np.asarray(v, dtype=np.float32).reshape(-1)


# ----------------------------------------------------------------------------------------------------------------
class BFSOracle:
	"""agents.py:92-129: first-in-first-out search over the 12-move graph, bounded by the number of states seen (the reference's
	time limit is not restated: traces are captured with max_states alone)."""

	def __init__(self):
		self.states, self.action_queue = {}, deque()

	def __len__(self):
		return len(self.states)                                              # agents.py:128-129

	def search(self, start: np.ndarray, max_states: int) -> bool:
		self.states, self.action_queue = {}, deque()
		if orc.is_solved(start):
			return True
		self.states = {start.tobytes(): (None, None)}                        # agents.py:103
		queue = deque([start])
		while len(self) < max_states:                                        # agents.py:105
			state = queue.popleft()
			key = state.tobytes()
			for a in range(12):
				child = orc.rotate(state, a // 2, 1 - a % 2)
				ckey = child.tobytes()
				if ckey in self.states:
					continue
				if orc.is_solved(child):                                     # agents.py:113-118: walk the predecessors back to the start
					self.action_queue.appendleft(a)
					while self.states[key][0] is not None:
						self.action_queue.appendleft(self.states[key][1])
						key = self.states[key][0]
					return True
				self.states[ckey] = (key, a)
				queue.append(child)
		return False


# ----------------------------------------------------------------------------------------------------------------
class AStarOracle:
	"""agents.py:171-413.  Node arrays are 1-based like the reference's (index 0 unused)."""

	def __init__(self, net, lambda_: float, expansions: int):
		self.net, self.lambda_, self.expansions = net, lambda_, expansions

	def reset(self):
		self.index = {}                      # state bytes -> idx                     agents.py:201
		self.states = [None]                 # agents.py:202
		self.G = [np.nan]                    # float64 in the reference; whole numbers
		self.parents = [0]
		self.parent_actions = [0]
		self.open = []                       # heap of (cost, idx)                    agents.py:185
		self.pops = []                       # pop order of every iteration (for the traces)
		self.action_queue = deque()

	def __len__(self):
		return len(self.index)

	def _add(self, state, g, parent, action):
		idx = len(self.states)
		self.states.append(state.copy())
		self.G.append(float(g))
		self.parents.append(parent)
		self.parent_actions.append(action)
		self.index[state.tobytes()] = idx
		return idx

	def search(self, start: np.ndarray, max_states: int) -> bool:
		"""agents.py:220-252 with the deterministic budget (no time limit)."""
		self.reset()
		if orc.is_solved(start):
			return True
		self._add(np.asarray(start, np.int8), 0, 0, 0)
		heapq.heappush(self.open, (0, 1))
		while len(self) + self.expansions * 12 <= max_states:
			n_pop = min(len(self.open), self.expansions)
			popped = [heapq.heappop(self.open)[1] for _ in range(n_pop)]
			self.pops.append(np.array(popped, dtype=np.int64))
			if self.expand_batch(popped):
				i = self.index[orc.SOLVED.tobytes()]
				while i != 1:
					self.action_queue.appendleft(self.parent_actions[i])
					i = self.parents[i]
				return True
		return False

	def expand_batch(self, popped) -> bool:
		"""agents.py:254-331."""
		if not popped:
			return False
		parents_of = np.repeat(np.array(popped), 12)
		actions_of = np.tile(np.arange(12), len(popped))
		children = orc.expand12(np.array([self.states[i] for i in popped]))
		keys = [c.tobytes() for c in children]

		# first occurrence of every distinct state in batch order (np.unique(..., return_index=True), :291-295)
		first_pos = {}
		for pos, k in enumerate(keys):
			first_pos.setdefault(k, pos)
		first_unseen = [pos for pos, k in enumerate(keys) if first_pos[k] == pos and k not in self.index]
		first_seen = [pos for pos, k in enumerate(keys) if first_pos[k] == pos and k in self.index]
		seen_idx = [self.index[keys[pos]] for pos in first_seen]          # before the new ones are added

		# unseen: append in batch order (:299-313)
		new_idx = []
		for pos in first_unseen:
			p = int(parents_of[pos])
			new_idx.append(self._add(children[pos], self.G[p] + 1, p, int(actions_of[pos])))
		new_states = children[first_unseen]

		# cost and push (:315-317, :369-383): float64 lambda*G plus float32 heuristic
		if len(new_idx):
			H = -_values(self.net, new_states)
			if np.isnan(H).any():                                              # heapq has no order for it; the engines end the search (error 4)
				raise ValueError(f"A* oracle: the net returned NaN for {int(np.isnan(H).sum())} of {len(H)} new states")
			cost = self.lambda_ * np.array([self.G[i] for i in new_idx], dtype=np.float64) + H
			for c, i in zip(cost, new_idx):
				heapq.heappush(self.open, (c, i))

		# goal test on the new states only (:321-323); the reference returns before relaxing
		if len(new_idx) and orc.multi_is_solved(new_states).any():
			return True

		# relax the seen ones (:333-367): two passes, each evaluated in full before it is applied
		rel_parent = [int(parents_of[pos]) for pos in first_seen]
		rel_action = [int(actions_of[pos]) for pos in first_seen]
		new_way = [self.G[p] + 1 < self.G[s] for s, p in zip(seen_idx, rel_parent)]
		rhs = [self.G[p] + 1 for p in rel_parent]
		for s, p, a, hit, g in zip(seen_idx, rel_parent, rel_action, new_way, rhs):
			if hit:
				self.G[s], self.parent_actions[s], self.parents[s] = g, a, p
		shortcut = [self.G[s] + 1 < self.G[p] for s, p in zip(seen_idx, rel_parent)]
		rhs = [self.G[s] + 1 for s in seen_idx]
		for s, p, a, hit, g in zip(seen_idx, rel_parent, rel_action, shortcut, rhs):
			if hit:                                   # repeated p: the last assignment stays, as in NumPy
				self.G[p], self.parent_actions[p], self.parents[p] = g, a ^ 1, s
		return False

	# arrays in the layout of the golden traces
	def arrays(self):
		n = len(self)
		return (np.array(self.states[1:n + 1], dtype=np.int8), np.array(self.G[1:n + 1]),
		        np.array(self.parents[2:n + 1], dtype=np.int64), np.array(self.parent_actions[2:n + 1], dtype=np.int64))


# ----------------------------------------------------------------------------------------------------------------
class MCTSOracle:
	"""agents.py:415-645.  One tree; arrays 1-based like the reference's."""

	def __init__(self, net, c: float, search_graph: bool, nu: float = 100.0, priors=None):
		"""`priors`: optional callable(states (n, 20) int8, root: bool) -> (n, 12) priors of those states, used instead of the
		float32 softmax of the net's logits (`root`: the call is for the start state, whose softmax the reference takes on the
		net's device, agents.py:472; every other call stands for the host's, :551-552).  It lets a test feed the tree arithmetic
		the very P bits another implementation stored, whoever's exp made them."""
		self.net, self.c, self.search_graph, self.nu, self.priors = net, c, search_graph, nu, priors

	def reset(self, cap: int):
		self.index = {}
		self.states = np.zeros((cap + 1, 20), np.int8)
		self.neighbors = np.zeros((cap + 1, 12), np.int64)
		self.leaves = np.ones(cap + 1, bool)
		self.P = np.zeros((cap + 1, 12))
		self.V = np.zeros(cap + 1)
		self.N = np.zeros((cap + 1, 12), np.int64)
		self.W = np.zeros((cap + 1, 12))
		self.L = np.zeros((cap + 1, 12))
		self.action_queue = deque()
		self.sims = 0

	def __len__(self):
		return len(self.index)

	def _policy_value(self, states, root=False):
		import torch
		if self.priors is not None:
			p = np.asarray(self.priors(states, root), dtype=np.float64).reshape(len(states), 12)
			return p, _values(self.net, states).astype(np.float64)
		p, v = self.net(orc.as_oh(states))
		p = torch.as_tensor(np.asarray(p)).float().softmax(dim=1).numpy()       # float32 softmax, as agents.py:552
		return p.astype(np.float64), np.asarray(v, dtype=np.float32).reshape(-1).astype(np.float64)

	def search(self, start: np.ndarray, max_states: int, max_sims: int = None) -> bool:
		"""agents.py:461-494 with the deterministic budget (`max_sims` additionally bounds the number of simulations)."""
		self.reset(max_states + 12)
		self.index[start.tobytes()] = 1
		self.states[1] = start
		if orc.is_solved(start):
			return True
		p, v = self._policy_value(start[None], root=True)
		self.P[1], self.V[1] = p[0], v[0]
		path, actions = [1], []
		while len(self) + 12 <= max_states and (max_sims is None or self.sims < max_sims):
			leaf, action = self.expand_leaf(path, actions)
			if leaf != -1:
				self.action_queue = deque(actions + [action])
				if self.search_graph:
					self.complete_graph()
					self.shorten(leaf)
				return True
			path, actions = self.find_leaf()
		self.action_queue = deque(actions)
		return False

	def expand_leaf(self, path, actions):
		"""agents.py:496-573."""
		self.sims += 1
		leaf = path[-1]
		children = orc.expand12(self.states[leaf][None])
		keys = [c.tobytes() for c in children]
		unseen = [a for a, k in enumerate(keys) if k not in self.index]
		for a in unseen:                                                     # new indices in action order (:523-529)
			idx = len(self.index) + 1
			self.index[keys[a]] = idx
			self.states[idx] = children[a]
		child_idx = np.array([self.index[k] for k in keys])
		self.neighbors[leaf] = child_idx                                     # :534
		self.neighbors[child_idx, np.arange(12) ^ 1] = leaf                  # :535
		self.leaves[leaf] = False
		solved = np.flatnonzero(orc.multi_is_solved(children))               # :540-543, over ALL children
		solve_leaf, solve_action = (int(child_idx[solved[0]]), int(solved[0])) if solved.size else (-1, -1)

		new_idx = child_idx[unseen]
		p, v = self._policy_value(children[unseen])                          # :548-552 (the reference assumes >= 1 new)
		self.P[new_idx], self.V[new_idx] = p, v
		best = v.max()
		self.W[leaf] = self.V[self.neighbors[leaf]]                          # :560
		self.W[new_idx] = v[:, None]                                         # :561
		for node, a in zip(path[:-1], actions):                              # :562 max-backup
			self.W[node, a] = np.maximum(self.W[node, a], best)              # (of -0.0 and +0.0 either may come back)
		if actions:                                                          # :567-570
			for node, a in set(zip(path[:-1], actions)):                     # fancy `+=` counts a repeated pair once
				self.N[node, a] += 1
			for node, a in zip(path[:-1], actions):
				self.L[node, a] = 0
			for node, a in zip(path[1:], actions):
				self.L[node, a ^ 1] = 0
		return solve_leaf, solve_action

	def find_leaf(self):
		"""agents.py:575-595."""
		cur, path, actions = 1, [1], []
		while not self.leaves[cur]:
			sqrt_n = np.sqrt(self.N[cur].sum())
			U = self.c * self.P[cur] * sqrt_n / (1 + self.N[cur])
			Q = self.W[cur] - self.L[cur]
			a = int((U + Q).argmax())
			self.L[cur, a] += self.nu
			cur = int(self.neighbors[cur, a])
			self.L[cur, a ^ 1] += self.nu
			path.append(cur)
			actions.append(a)
		return path, actions

	def complete_graph(self):
		"""agents.py:597-611."""
		n = len(self)
		leaf_idx = np.flatnonzero(self.leaves[:n + 1])[1:]
		if not len(leaf_idx):
			return
		children = orc.expand12(self.states[leaf_idx])
		child_idx = np.array([self.index.get(c.tobytes(), 0) for c in children])
		rep = np.repeat(leaf_idx, 12)
		acts = np.tile(np.arange(12), len(leaf_idx))
		self.neighbors[rep, acts] = child_idx
		self.neighbors[child_idx, acts ^ 1] = rep
		self.neighbors[0] = 0

	def shorten(self, solved_index: int):
		"""Breadth-first search inside the explored graph (agents.py:613-633)."""
		if solved_index == 1:
			return
		self.action_queue = deque()
		came_from = {1: (None, None)}
		q = deque([1])
		while q:
			v = q.popleft()
			for a, n in enumerate(self.neighbors[v]):
				n = int(n)
				if not n or n in came_from:
					continue
				if n == solved_index:
					self.action_queue.appendleft(a)
					while came_from[v][0] is not None:
						self.action_queue.appendleft(came_from[v][1])
						v = came_from[v][0]
					return
				came_from[n] = (v, a)
				q.append(n)
