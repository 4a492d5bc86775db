"""
The three-call form of an A* iteration (rk_astar_expand / rk_astar_commit / rk_astar_next_pops) restated on the CPU oracle, and the
driver that steers it: what the engine has to reproduce bit for bit when the CALLER chooses the pop count and the values of every
iteration.  A helper for tests/test_astar_steps_*.py, not a test module.

Model.  `StepModel` is oracle.search_oracle.AStarOracle with a scripted net: one iteration pops min(n_expand, |open|) pairs, runs
the oracle's own expand_batch, and the values of the new states are the next scripted vector (by position, not by state).  The loop
guard is the engine's, `len + 12 * n_expand <= budget`.  On top of it the model restates the engine's open queue as far as a test can
see it from outside: the level capacities of queue_plan and the level a push goes to (the first whose capacity holds the new records
and everything live below it).

Dry run.  `dry(limit)` expands the first `limit` pairs of the open queue without changing anything and returns, for every pop count
n, how many new states n_expand = n would append (a prefix of one scan: new states are first occurrences in batch order), and their G.

Driver.  `run(geometry, bf16, engine)` picks the n_expand of every iteration so that the number of new records lands on the sizes at
which the engine's sort / merge / insert change their form (`targets`), with small pseudo-random pop counts in between and a return
to n_expand = N now and then, and one value pattern per iteration (`PATTERNS`).  Everything is seeded: the run of the CPU test is the
run the GPU test follows.  `engine`, if given, is called once per iteration with the model before and after its step.

What cannot be reached (the driver looks for it in every dry run and the CPU test names it): a popped node has its parent among its
twelve children, so an iteration appends at most 11 per node (12 for the root) -- K = 12 N only for N = 1, `Kpad - 1` never; and a
node with no or one unseen neighbour needs expanded nodes next to (nearly) all its neighbours, which a pool of 10^5 states out of
4.3 * 10^19 does not hold -- n_new = 0 and n_new = 1 do not occur.
"""
import heapq
from collections import namedtuple

import numpy as np

from oracle import cube_oracle as orc
from oracle.search_oracle import AStarOracle, _round_bf16

# librubiks_amd/csrc/rk_astar.hip
SMALL_CHUNK, SORT_CHUNK, MAX_NEW_RUNS, POP_LDS, QL = 256, 2048, 8, 6144, 12


def sort_geometry(N: int):
	"""(K, chunk, Kpad, form) of an engine with max_expansions N: astar_create_impl and new_chunk_of."""
	K = 12 * N
	chunk = SMALL_CHUNK if K <= SORT_CHUNK else SORT_CHUNK
	Kpad = -(-K // chunk) * chunk
	form = "runs of 256" if chunk == SMALL_CHUNK else ("chunks as they are" if Kpad <= MAX_NEW_RUNS * SORT_CHUNK else "merge passes")
	return K, chunk, Kpad, form


def queue_plan(N: int, capacity: int):
	"""Level capacities of the open queue (queue_plan, world = 1): 4 K, 16 K, ... records, at least 4096; the top level holds the pool."""
	C1, c, caps = capacity + 1, max(4 * 12 * N, 4096), []
	while True:
		top = c >= C1 or len(caps) == QL - 1
		caps.append(C1 if top else c)
		if top:
			return caps
		c *= 4


def targets(N: int):
	"""The new-record counts at which the commit path changes its form, for an engine with chunk c: 1, 127, 128, 129, c - 1, c, c + 1,
	2 c, 2 c + 1, every power of two from 128 to c and one above each, Kpad - 1, K, and 0.  -> (all of them, those within reach)."""
	K, c, Kpad, _ = sort_geometry(N)
	t = {0, 1, 127, 128, 129, c - 1, c, c + 1, 2 * c, 2 * c + 1, Kpad - 1, K}
	p = 128
	while p <= c:
		t |= {p, p + 1}
		p *= 2
	reach = {x for x in t if x <= 11 * N or (N == 1 and x == 12)}
	return sorted(t), sorted(reach)


class _Scripted:
	"""The net of the model: whatever the states, the next scripted vector."""
	def __init__(self):
		self.next = None

	def __call__(self, x, policy=True, value=True):
		assert self.next is not None and len(self.next) == len(x), "one scripted value per new state"
		v, self.next = self.next, None
		return np.asarray(v, np.float32).reshape(-1, 1)


class _Lowered(list):
	"""G as the oracle keeps it, counting the writes that lower an entry (the two relaxation passes)."""
	lowered = 0

	def __setitem__(self, i, v):
		if v < self[i]:
			self.lowered += 1
		list.__setitem__(self, i, v)


Step = namedtuple("Step", "n_expand popped n_new won solved n_states level")


class StepModel(AStarOracle):
	def __init__(self, lambda_: float, N: int, capacity: int):
		super().__init__(_Scripted(), lambda_, N)
		self.N, self.capacity, self.caps = N, capacity, queue_plan(N, capacity)

	def start(self, state: np.ndarray, budget: int):
		self.reset()
		self.G = _Lowered(self.G)
		self.budget = budget
		self._add(np.asarray(state, np.int8), 0, 0, 0)
		heapq.heappush(self.open, (0.0, 1))
		self.levels = [set() for _ in self.caps]
		self.levels[0].add(1)
		self.iterations, self.won, self.solved = 0, False, 0

	def runs(self, n_expand: int) -> bool:
		"""the engine's loop guard (agents.py:236 with the caller's pop count) and its stop flags"""
		return not self.won and bool(self.open) and len(self) + 12 * n_expand <= self.budget

	def next_pops(self, n_expand: int):
		return [i for _, i in heapq.nsmallest(n_expand, self.open)] if self.runs(n_expand) else []

	def dry(self, limit: int):
		"""-> (cum, G): cum[n] = new states of an iteration with n_expand = n (n = 0 .. min(limit, |open|)), G of the first cum[-1] of them"""
		head = heapq.nsmallest(limit, self.open)
		cum, G, batch = [0], [], set()
		if head:
			children = orc.expand12(np.array([self.states[i] for _, i in head]))
			for n, (_, p) in enumerate(head):
				for c in children[12 * n:12 * n + 12]:
					k = c.tobytes()
					if k not in self.index and k not in batch:
						batch.add(k)
						G.append(self.G[p] + 1)
				cum.append(len(G))
		return cum, np.array(G, np.float64)

	def step(self, n_expand: int, values) -> Step:
		if np.isnan(np.asarray(values, np.float32)).any():                    # before anything changes: heapq has no order for a NaN cost,
			raise ValueError("a NaN among the scripted values: the engine ends the search with error 4, the model has no answer")
		if not self.runs(n_expand):
			return Step(n_expand, [], 0, int(self.won), self.solved, len(self), -1)
		popped = [heapq.heappop(self.open)[1] for _ in range(min(len(self.open), n_expand))]
		for i in popped:
			next(s for s in self.levels if i in s).remove(i)
		n_before = len(self)
		self.net.next = values
		self.won = bool(self.expand_batch(popped))
		self.net.next = None
		n_new, level = len(self) - n_before, -1
		if self.won:
			self.solved = self.index[orc.SOLVED.tobytes()]
		if n_new:
			total = n_new
			for level, cap in enumerate(self.caps):
				total += len(self.levels[level])
				if total <= cap:
					break
			merged = set(range(n_before + 1, n_before + n_new + 1)).union(*self.levels[:level + 1])
			for s in self.levels[:level]:
				s.clear()
			self.levels[level] = merged
		self.iterations += 1
		return Step(n_expand, popped, n_new, int(self.won), self.solved, len(self), level)

	def open_sorted(self):
		"""the open queue in pop order: (costs as float64 with -0.0 folded into +0.0, as the engine's keys hold them; indices)"""
		cost = np.array([c for c, _ in self.open], np.float64) + 0.0
		idx = np.array([i for _, i in self.open], np.int64)
		order = np.lexsort((idx, cost))
		return cost[order], idx[order]

	def path(self, i: int):
		out = []
		while i != 1:
			out.append(self.parent_actions[i])
			i = self.parents[i]
		return out[::-1]


# ---- value patterns: float32 bit patterns built on the host, one value per new state in index order ---------------------------------
PATTERNS = ("equal", "alternate", "ascending", "descending", "blocks", "ulp_pairs", "zero_cross", "specials", "random_bits")


def _ordered(k: np.ndarray, bf16: bool) -> np.ndarray:
	"""integers -> floats, strictly monotone: k >= 0 is the k-th non-negative bit pattern, k < 0 the |k|-th negative one"""
	k = np.asarray(k, np.int64)
	mag = np.abs(k).astype(np.uint32)
	assert mag.max(initial=0) < (0x7F80 if bf16 else 0x7F800000)
	bits = (mag << np.uint32(16 if bf16 else 0)) | np.where(k < 0, np.uint32(0x80000000), np.uint32(0))
	return bits.astype(np.uint32).view(np.float32)


def make_values(pattern: str, G: np.ndarray, lambda_: float, rng: np.random.RandomState, bf16: bool) -> np.ndarray:
	"""float32 values of len(G) new states (for the bfloat16 leg: float32 numbers that bfloat16 holds exactly).  No NaN."""
	n = len(G)
	ulp = np.uint32(1 << 16 if bf16 else 1)
	rnd = lambda m: _round_bf16((rng.standard_normal(m) * 16).astype(np.float32)) if bf16 else (rng.standard_normal(m) * 16).astype(np.float32)
	if pattern == "equal":
		v = np.repeat(rnd(1), n)
	elif pattern == "alternate":
		v = rnd(2)[np.arange(n) % 2]
	elif pattern in ("ascending", "descending"):
		span = 0x7F7F if bf16 else 0x7F7FFFFF                                 # the largest finite magnitude, as a bit pattern
		stride = int(rng.randint(1, max(1, min(2 * (span - 1) // max(n, 1), 1 << 20)) + 1))
		k0 = -(stride * (n - 1) // 2)                                         # from below zero to above it
		v = _ordered(k0 + stride * np.arange(n), bf16)
		v = v[::-1].copy() if pattern == "descending" else v
	elif pattern == "blocks":
		edges = sorted({b + e for b in range(0, n + SORT_CHUNK, SORT_CHUNK) for e in (0, 64, 128, 256)})
		block = np.searchsorted(edges, np.arange(n), side="right")
		v = rnd(5)[rng.randint(0, 5, len(edges) + 1)][block]                 # few values: whole blocks repeat further on
	elif pattern == "ulp_pairs":
		x = np.repeat(rnd((n + 1) // 2), 2)[:n]
		v = (x.view(np.uint32) + np.where(np.arange(n) % 2 == 1, ulp, np.uint32(0))).view(np.float32)
	elif pattern == "zero_cross":
		base = (lambda_ * G).astype(np.float32)                             # cost = lambda G - value: zero, or one rounding away from it
		if bf16:
			base = _round_bf16(base)
		up = (base.view(np.uint32) + ulp).view(np.float32)
		down = np.where(base == 0, -up, (np.maximum(base.view(np.uint32), ulp) - ulp).view(np.float32))
		v = np.choose(rng.randint(0, 6, n), [base, up, down, np.zeros(n, np.float32), -np.zeros(n, np.float32), -base])
	elif pattern == "specials":
		palette = np.array([1e-40, -1e-40, 1.4e-45, -1.4e-45, 1e30, -1e30, np.inf, -np.inf, 1.0, -2.5, 0.0, -0.0], np.float32)
		v = palette[rng.randint(0, len(palette), n)]
	elif pattern == "random_bits":
		bits = rng.randint(0, 1 << 16, n).astype(np.uint32) << np.uint32(16)
		if not bf16:
			bits |= rng.randint(0, 1 << 16, n).astype(np.uint32)
		nan_exp = (bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)   # infinities and NaNs: take one exponent bit away
		v = np.where(nan_exp, bits & np.uint32(0xBFFFFFFF), bits).astype(np.uint32).view(np.float32)
	else:
		raise ValueError(pattern)
	v = np.ascontiguousarray(_round_bf16(v) if bf16 else v, np.float32)
	assert v.shape == (n,) and not np.isnan(v).any()
	return v


# ---- geometries and the driver -----------------------------------------------------------------------------------------------------------
Geometry = namedtuple("Geometry", "N capacity lambda_ depth seed min_iters iterations full_every why")

GEOMETRIES = [
	# level 0 holds 4096 records whatever the N below 86: the pushes of these two climb to the top level
	Geometry(1, 6000, 0.5, 14, 11, 470, 470, 0, "256-record single run, K = 12"),
	Geometry(3, 9000, 0.3, 14, 12, 300, 300, 4, "256-record single run, K = 36"),
	Geometry(21, 60_000, 0.5, 12, 13, 150, 400, 9, "K = 252: one run of 256"),
	Geometry(22, 60_000, 0.3, 12, 14, 150, 400, 9, "K = 264: two runs of 256"),
	Geometry(170, 200_000, 0.5, 12, 15, 100, 400, 12, "K = 2040, Kpad = 2048: eight runs of 256, the last form before the switch"),
	Geometry(171, 200_000, 0.3, 12, 16, 100, 400, 12, "K = 2052: chunk 2048, Kpad = 4096, two chunks as they are"),
	Geometry(1365, 400_000, 0.5, 12, 17, 60, 400, 8, "Kpad = 16 384: eight chunks, no merge pass"),
	Geometry(1366, 400_000, 0.3, 12, 18, 60, 400, 8, "Kpad = 18 432: nine chunks, k_merge_pass, one run into the insert"),
	Geometry(2048, 400_000, 0.5, 12, 19, 60, 400, 8, "three levels, levels * N = 6144: selection in one workgroup"),
	Geometry(2049, 400_000, 0.3, 12, 20, 60, 400, 8, "three levels, levels * N = 6147: k_pop_wide"),
]
MAX_FULL = 7                    # returns to n_expand = N in an engine with N >= 1365 (11 N new states each: the pool stays below 250 000)
FILLERS = (1, 2, 3, 4, 5, 7)    # pop counts between targets
# the one run that ends on the loop guard on purpose (budget GUARD_BUDGET), and goes on after rk_astar_set_budget
GUARD_CASE = Geometry(5, 9000, 0.5, 12, 21, 1, 80, 3, "ends on the loop guard")
GUARD_BUDGET = 700
# tests/test_astar_nonfinite_gpu.py: the smallest engines in which every form of the kernel that READS the values runs -- one
# k_records_sort<256> workgroup; several of them (a value at j >= 256 is read by a later workgroup); k_records_sort<2048> with
# k_merge_pass behind it (a value at j >= 2048).  The schedule is `run`'s; the test stops it at the iteration it poisons.
NAN_GEOMETRIES = [
	Geometry(4, 9000, 0.5, 14, 31, 1, 40, 3, "K = 48: one run of 256"),
	Geometry(30, 60_000, 0.3, 12, 32, 1, 40, 3, "K = 360: two runs of 256, the second workgroup reads j >= 256"),
	Geometry(1366, 400_000, 0.3, 12, 18, 1, 40, 8, "Kpad = 18 432: nine 2048-record chunks and k_merge_pass (GEOMETRIES[7])"),
]


def start_state(g: Geometry) -> np.ndarray:
	rng = np.random.RandomState(g.seed)
	s = orc.SOLVED
	for _ in range(g.depth):
		s = orc.rotate(s, int(rng.randint(6)), int(rng.randint(2)))
	return s


Record = namedtuple("Record", "it n_expand n_new pattern target step values")


def run(g: Geometry, bf16: bool, engine=None, budget: int = None, model=None, iterations: int = None):
	"""The schedule of geometry `g`, model (and `engine`) in lock-step.  engine.iteration(model, n_expand, values, pattern, target)
	has to call model.step(n_expand, values) itself, between its own expand and commit, and return the Step.
	`model`: go on with this one (a run that had stopped) for `iterations` more.
	-> (model, [Record])"""
	rng = np.random.RandomState(1000 * g.seed + int(bf16) + (0 if model is None else 500))
	m = model
	if m is None:
		m = StepModel(g.lambda_, g.N, g.capacity)
		m.start(start_state(g), g.capacity if budget is None else budget)
	_, reach = targets(g.N)
	left, log, fulls = set(reach), [], 0
	first_pattern = int(rng.randint(len(PATTERNS)))
	for it in range(g.iterations if iterations is None else iterations):
		target = None
		scan = g.N if it == 0 or not left else min(g.N, max(max(left) // 8 + 2, max(FILLERS)))
		full = (it == 0 and model is None) or (g.full_every and it % g.full_every == 0 and (g.N < 1365 or fulls < MAX_FULL))
		cum, G = m.dry(g.N if full else scan)
		if full:
			n_expand = g.N
			fulls += 1
		else:
			hits = [t for t in sorted(left) if t in cum[1:]]
			if hits:
				target = hits[int(rng.randint(len(hits)))]
				n_expand = cum.index(target, 1)
			else:
				n_expand = min(g.N, FILLERS[int(rng.randint(len(FILLERS)))])
				if log and log[-1].n_expand <= max(FILLERS) and rng.randint(3) == 0:
					n_expand = log[-1].n_expand                                   # the same pop count twice in a row
		n_new = cum[min(n_expand, len(cum) - 1)] if m.runs(n_expand) else 0
		if target is None and n_new in left:
			target = n_new
		left.discard(n_new)
		pattern = PATTERNS[(first_pattern + it) % len(PATTERNS)]
		values = make_values(pattern, G[:n_new], g.lambda_, rng, bf16)
		step = engine.iteration(m, n_expand, values, pattern, target) if engine is not None else m.step(n_expand, values)
		assert step.n_new == n_new, (g.N, it, n_expand, step.n_new, n_new)
		log.append(Record(it, n_expand, n_new, pattern, target, step, values))
		if step.won or not step.popped:
			break
		if left <= {0, 1} and it + 1 >= g.min_iters and fulls >= 3 and m.G.lowered and m.budget >= g.capacity and iterations is None:
			break                                                               # every size that occurs at all was seen, and a relaxation: enough
	return m, log


def coverage(g: Geometry, log):
	"""what the CPU test asserts and the summary lists"""
	_, reach = targets(g.N)
	hit = sorted({r.n_new for r in log} & set(reach))
	n_exp = [r.n_expand for r in log]
	return {"hit": hit, "missed": sorted(set(reach) - set(hit)), "distinct": len(set(n_exp)),
	        "changes": sum(a != b for a, b in zip(n_exp, n_exp[1:])), "repeats": sum(a == b for a, b in zip(n_exp, n_exp[1:])),
	        "patterns": sorted({r.pattern for r in log}), "iterations": len(log)}
