"""
The CPU half of "the hash-sharded A* on REAL-VALUED net outputs" (the GPU half: tests/test_sharded_real_valued_gpu.py).  The nets are
the LookupNet variants of tests/test_real_valued_oracle_cpu.VARIANTS: values of arbitrary float32 / bfloat16 bit patterns, the same bits
on the host and on the device, so every comparison is exact equality.
  * oracle/sharded_oracle.py at world = 1 IS AStarOracle on the fixture cases of tests/golden/real_trace.npz (AStarOracle is pinned to
    the unmodified reference there): states, G, parents, actions, every iteration's pops, the open queue as (cost bits, index) pairs;
  * at world 2 / 3 / 8 the protocol's properties (check_shards) hold on every case the GPU test uses;
  * the cases the GPU test uses are NOT WEAK: every float-sensitive situation of k_shard_decide, k_end<true> and the sharded push that
    the GPU comparison is there for really occurs in them -- asserted here on the oracle alone, so that a weak input fails on the CPU
    and not silently on the GPU.
CPU only.
"""
import numpy as np
import pytest

from oracle import cube_oracle as orc
from oracle.sharded_oracle import STOP_BUDGET, STOP_CAPACITY, STOP_WON, ShardedAStarOracle
from tests.test_real_valued_oracle_cpu import ASTAR_CASES, astar_oracle, load_trace, net_of, variant
from tests.test_sharded_oracle_cpu import check_shards

WORLDS = (2, 3, 8)
LAM_ULP = 2.0 ** 29          # lambda * G is exact and 2^29 times a value: the float64 sum keeps a value's float32 ulp as ITS last bit
# (seed, scramble depth, lambda, N, state budget) per variant: what tests/test_sharded_real_valued_gpu.py runs at every world size.
# N is 10 (one workgroup of k_shard_decide, most ranks pop 0 or 1), a value in 100..130, or 300 (k_shard_decide spans workgroups).
GPU_CASES = {
	"plain": [(102, 7, 0.3, 10, 20_000), (304, 9, 0.6, 120, 30_000), (109, 9, -0.0, 300, 30_000)],      # -0.0: test_a_cost_is_minus_zero_...
	"offset": [(106, 4, 2.5, 10, 10_000), (202, 12, LAM_ULP, 120, 25_000), (103, 9, 1.0, 300, 30_000)],
	"special": [(108, 10, 0.0, 10, 12_000), (107, 12, 0.2, 120, 30_000), (157, 9, 0.0, 300, 30_000)],
	"bf16": [(104, 11, 0.05, 10, 15_000), (105, 8, 0.3, 120, 20_000), (111, 13, 0.1, 300, 30_000)],
	"misleading": [(105, 10, 0.6, 10, 15_000), (12, 16, 0.02, 120, 30_000), (112, 14, 0.02, 300, 30_000)],
}
CAPACITY_CASE = ("offset", (42, 14, 0.2, 100, 10_000_000), 9_000)          # (variant, case, states a rank's pool holds)
# The wide pop (k_pop_wide and k_shard_heads write the candidates and the gather contribution instead of k_end<true>), derived in
# test_sharded_real_valued_gpu.test_wide_pop: (variant, world, (seed, depth, lambda, N), capacity, budgets)
WIDE_CASE = ("special", 8, (157, 9, 0.1, 1229), 480_000, (40_000, 110_000))
POP_LDS, QL = 6144, 12                                                     # rk_astar.hip


def queue_levels(N: int, world: int, capacity: int) -> list:
	"""rk_astar.hip:queue_plan -- the record capacities of the open queue's levels of one rank's engine."""
	inflow = 12 * N if world == 1 else -(-12 * N // world)
	c, caps = max(4 * inflow, 4096), []
	while True:
		top = c >= capacity + 1 or len(caps) == QL - 1
		caps.append(capacity + 1 if top else c)
		if top:
			return caps
		c *= 4


_RUNS = {}


class CountingOracle(ShardedAStarOracle):
	"""The oracle unchanged, with what the "not weak" conditions need to see: shortcut offers that hit (relaxation case 2 across
	ranks), nodes relaxed by case 1, and every rank's open-set size after every iteration."""

	def search(self, start, max_states, capacity=None):
		self.offer_hits, self.case1, self._open_after = 0, 0, []
		stop = super().search(start, max_states, capacity)
		self.open_sizes = np.array(self._open_after, np.int64).reshape(self.iterations, self.world)
		return stop

	def _apply_offers(self, rk, offers):
		# hits of offers whose child lives on ANOTHER rank than the parent: relaxation case 2 through the exchange
		self.offer_hits += sum(1 for p, g_new, _, crank, _ in offers if g_new < rk.G[p] and crank != rk.rank)
		ShardedAStarOracle._apply_offers(rk, offers)
		self._g_after_offers = rk.G[:]

	def _insert_push(self, rk, offers, records):
		n_new = super()._insert_push(rk, offers, records)      # the base's own step, in its own order; it applies the offers first
		self.case1 += sum(1 for a, b in zip(self._g_after_offers, rk.G) if a != b)      # G changed after the offers: case 1
		self._open_after.append(len(rk.open))
		return n_new


def start_of(case):
	np.random.seed(case[0])
	return orc.scramble(case[1], True)[0]


def sharded_oracle(name: str, world: int, case, capacity=None) -> CountingOracle:
	"""The oracle's search of a case, made once per process (the GPU tests compare the engines with the same object)."""
	key = (name, world, case, capacity)
	if key not in _RUNS:
		seed, depth, lam, N, budget = case
		o = CountingOracle(variant(name), lam, N, world)
		o.search(start_of(case), budget, capacity)
		_RUNS[key] = o
	return _RUNS[key]


def all_cases():
	return [(name, case) for name in GPU_CASES for case in GPU_CASES[name]]


# ---- what a search's published candidates hold -------------------------------------------------------------------------------------
def ordered(x: np.ndarray) -> np.ndarray:
	"""float64 (no -0.0, no NaN) -> int64 that orders like the numbers and counts float64 steps: neighbours differ by one."""
	i = np.ascontiguousarray(x, np.float64).view(np.int64)
	return np.where(i < 0, -(i & np.int64(0x7FFFFFFFFFFFFFFF)), i)


TINY32 = 1.1754944e-38
BIG32 = float(np.float32(1e30))


def facts(o: ShardedAStarOracle) -> dict:
	"""Which of the situations the GPU comparison is there for occur among the candidate costs the ranks of this search publish."""
	W, N = o.world, o.N
	f = dict(dup_cross=False, straddle=False, signs_zero=False, inf_short=False, neg_inf=False, denormal=False, plus_big=False, minus_big=False,
	         min_gap=None, max_pop=max((len(p) for it in o.pops for p in it), default=0))
	assert len(o.cand_costs) == o.iterations + 1
	for it, per_rank in enumerate(o.cand_costs):
		cost = np.concatenate(per_rank)
		if not len(cost):
			continue
		rank = np.concatenate([np.full(len(c), r) for r, c in enumerate(per_rank)])
		pos = np.concatenate([np.arange(len(c)) for c in per_rank])
		order = np.lexsort((pos, rank, cost))
		cost, rank = cost[order], rank[order]
		f["signs_zero"] |= bool((cost < 0).any() and (cost > 0).any() and (cost == 0).any())
		f["inf_short"] |= any(len(c) < N and np.isposinf(c).any() for c in per_rank)
		f["neg_inf"] |= bool(np.isneginf(cost).any())
		f["denormal"] |= bool(((np.abs(cost) < TINY32) & (cost != 0)).any())
		f["plus_big"] |= bool((cost == BIG32).any())
		f["minus_big"] |= bool((cost == -BIG32).any())
		# groups of bit-equal costs, the ranks they sit on
		u, first = np.unique(cost, return_index=True)
		last = np.append(first[1:], len(cost)) - 1
		lo, hi = rank[first], rank[last]                                     # within a group the ranks ascend
		f["dup_cross"] |= bool((lo != hi).any())
		if it < o.iterations and len(cost) > N and cost[N - 1] == cost[N]:      # the N-th place cuts a group of equal costs ...
			g = np.searchsorted(u, cost[N])
			f["straddle"] |= bool(lo[g] != hi[g])                            # ... that sits on more than one rank: the rank rule decides a pop
		fin = np.isfinite(u)
		if fin.sum() > 1:
			k = ordered(u[fin]).astype(np.uint64)
			gap = k[1:] - k[:-1]                                             # float64 steps between neighbouring distinct costs (mod 2^64: exact)
			l, h = lo[fin], hi[fin]
			cross = ~((l[1:] == h[1:]) & (l[:-1] == h[:-1]) & (l[1:] == l[:-1]))   # the two groups are not on one and the same rank
			if cross.any():
				m = int(gap[cross].min())
				f["min_gap"] = m if f["min_gap"] is None else min(f["min_gap"], m)
	return f


# ---- the pin at world 1 ------------------------------------------------------------------------------------------------------------
def bits(costs) -> np.ndarray:
	return np.array([float(c) for c in costs], np.float64).view(np.uint64)


@pytest.mark.parametrize("tag", ASTAR_CASES)
def test_world1_is_the_single_queue_oracle_on_real_values(tag):
	"""ShardedAStarOracle at world 1 against AStarOracle (pinned to the unmodified reference by tests/golden/real_trace.npz) on the
	fixture's own nets, starts and budgets: every array, every iteration's pops, the open queue with its costs compared as bits."""
	t = load_trace()
	_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
	ref, ref_solved, ref_queue = astar_oracle(tag)
	o = ShardedAStarOracle(net_of(t, tag), float(t[f"{tag}_lambda"]), expansions, 1)
	stop = o.search(t[f"{tag}_start"], max_states)
	assert (stop == STOP_WON) == ref_solved and (ref_solved or stop == STOP_BUDGET)
	rs, rG, rp, ra = ref.arrays()
	states, G, parents, prank, pact = o.arrays(0)
	assert states.shape == rs.shape and (states == rs).all() and (G == rG).all()
	assert (parents[1:] == rp).all() and (pact[1:] == ra).all() and not prank.any()
	assert len(o.pops) == len(ref.pops) and all(list(a[0]) == [int(i) for i in b] for a, b in zip(o.pops, ref.pops))
	assert list(o.action_queue) == list(ref.action_queue)
	got = o.open_queue(0)
	assert [i for _, i in got] == [int(i) for _, i in ref_queue]
	assert (bits(c for c, _ in got) == bits(c for c, _ in ref_queue)).all()
	# what the one rank publishes is what it pops: the first min(N, |open|) costs of the queue, + 0.0
	assert len(o.cand_costs) == o.iterations + 1 and all(len(c) == 1 and c[0].dtype == np.float64 for c in o.cand_costs)
	assert all(len(c[0]) == len(p[0]) for c, p in zip(o.cand_costs, o.pops))
	last = o.cand_costs[-1][0]
	assert (last.view(np.uint64) == bits(c for c, _ in got[:len(last)])).all()


# ---- the protocol's properties on the GPU cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_protocol_properties_on_the_gpu_cases(name, world):
	for case in GPU_CASES[name]:
		o = sharded_oracle(name, world, case)
		seen = check_shards(o, start_of(case))
		N, budget = case[3], case[4]
		assert len(seen) == o.total_states <= budget, (name, case)
		assert all(sum(len(p) for p in it) <= N for it in o.pops) and all(sum(c) <= 12 * N for c in o.new_counts)
		if o.stop == STOP_WON:
			s = start_of(case)
			for a in o.action_queue:
				s = orc.rotate(s, a // 2, 1 - a % 2)
			assert orc.is_solved(s), (name, case)
		else:
			assert o.stop == STOP_BUDGET and o.total_states + 12 * N > budget, (name, case)


@pytest.mark.parametrize("world", WORLDS)
def test_protocol_properties_on_the_capacity_and_the_wide_case(world):
	name, case, capacity = CAPACITY_CASE
	check_shards(sharded_oracle(name, world, case, capacity), start_of(case))
	name, w, case, capacity, budgets = WIDE_CASE
	if w == world:
		check_shards(sharded_oracle(name, w, case + (budgets[0],)), start_of(case))


def test_the_case_set_has_the_shapes_the_issue_asks_for():
	for name, cases in GPU_CASES.items():
		assert 2 <= len(cases) <= 3 and all(c[4] <= 40_000 for c in cases), name
	Ns = {c[3] for _, c in all_cases()}
	assert 10 in Ns and 300 in Ns and any(100 <= n <= 130 for n in Ns) and all(n == 10 or n == 300 or 100 <= n <= 130 for n in Ns)


def test_the_wide_case_is_wide_and_fills_two_queue_levels():
	"""pop_is_wide: levels * N > POP_LDS.  N is the smallest that is wide with this world's and capacity's levels; with the larger
	budget a rank's open set outgrows level 0 early enough that several iterations select their candidates from two levels."""
	name, world, case, capacity, budgets = WIDE_CASE
	caps = queue_levels(case[3], world, capacity)
	assert len(caps) * case[3] > POP_LDS >= len(caps) * (case[3] - 1) and len(queue_levels(case[3] - 1, world, capacity)) == len(caps)
	assert all(len(queue_levels(c[3], w, c[4])) * c[3] <= POP_LDS for _, c in all_cases() for w in WORLDS)      # everybody else: one workgroup
	small, large = (sharded_oracle(name, world, case + (b,)) for b in budgets)
	assert small.stop == large.stop == STOP_BUDGET and small.iterations >= 4
	# an open set larger than level 0 cannot lie in level 0 alone, and the next push goes to level 0 again
	grown = np.flatnonzero(large.open_sizes.max(axis=1) > caps[0])
	assert len(grown) and large.iterations - 1 - grown[0] >= 2 and not (small.open_sizes > caps[0]).any()
	f = facts(large)
	assert f["inf_short"] and f["neg_inf"] and f["dup_cross"] and f["straddle"]


def test_select_pops_tells_an_open_node_at_plus_infinity_from_the_padding():
	"""The host statement of k_shard_decide's rule (librubiks_amd.solving.sharded.select_pops) with the candidate counts: a node whose
	cost is +inf is popped when it is among the n cheapest; without the counts every +inf is padding, as before."""
	from librubiks_amd.solving.sharded import select_pops
	inf = np.inf
	heads = np.array([[1.0, inf, inf, inf], [-inf, 2.0, inf, inf], [inf, inf, inf, inf]])
	assert select_pops(heads, 4).tolist() == [1, 2, 0]
	assert select_pops(heads, 4, [2, 3, 0]).tolist() == [2, 2, 0]          # rank 0's +inf is a node; the lower rank wins the tie at +inf
	assert select_pops(heads, 6, [2, 3, 1]).tolist() == [2, 3, 1]
	assert select_pops(heads, 5, [1, 4, 1]).tolist() == [1, 4, 0]          # position breaks the tie inside a rank, rank before that
	assert select_pops(heads, 2, [2, 3, 1]).tolist() == [1, 1, 0]


# ---- the inputs are not weak --------------------------------------------------------------------------------------------------------
def _facts(world):
	return {(name, case): facts(sharded_oracle(name, world, case)) for name, case in all_cases()}


@pytest.mark.parametrize("world", WORLDS)
def test_equal_costs_on_two_ranks_decide_a_pop(world):
	"""Some iteration holds two bit-equal candidate costs on different ranks, and in one the global N-th place cuts such a group:
	who pops is decided by `r < d.rank ? o[mid] <= x : o[mid] < x` alone.  At every world size, with float32 and with bfloat16 values."""
	fs = _facts(world)
	assert any(f["dup_cross"] for f in fs.values())
	assert any(f["straddle"] for (name, _), f in fs.items() if name != "bf16")
	assert any(f["straddle"] for (name, _), f in fs.items() if name == "bf16")


@pytest.mark.parametrize("world", WORLDS)
def test_candidates_of_both_signs_and_a_zero_meet(world):
	assert any(f["signs_zero"] for f in _facts(world).values())


@pytest.mark.parametrize("world", WORLDS)
def test_a_cost_is_minus_zero_before_it_is_normalised(world):
	"""sortable_key's `c + 0.0`: lambda * G + (-value) is -0.0 only when BOTH terms are, and lambda * G is +0.0 or positive for
	every lambda >= +0.0.  The `plain` case with lambda = -0.0 (costs are -value, about 0.5 k - noise: a zero is among the cheapest) makes -0.0 * G = -0.0 for every node but the root, so a node whose
	value is +0.0 has the raw cost (-0.0) + (-0.0) = -0.0 and one whose value is -0.0 has (-0.0) + (+0.0) = +0.0: an engine that
	dropped the normalisation would publish -0.0 bits and pop the former before the latter whatever their indices, where the oracle
	(heapq: -0.0 == 0.0, then the index; cost + 0.0 published) has +0.0 bits and index order.  Asserted: nodes of both kinds were
	popped (so they were candidates) by ranks of this search, and in one iteration one rank popped both kinds."""
	case = next(c for c in GPU_CASES["plain"] if c[2] == 0 and np.signbit(c[2]))
	o = sharded_oracle("plain", world, case)
	net = variant("plain")
	raw_minus = raw_plus = together = 0
	for per_rank in o.pops:
		for r, popped in enumerate(per_rank):
			popped = [i for i in popped if o.ranks[r].G[i] > 0]               # (the root's cost is the constant 0.0)
			if not popped:
				continue
			v = np.asarray(net(orc.as_oh(np.array([o.ranks[r].states[i] for i in popped])), policy=False), np.float32).reshape(-1)
			G = np.array([o.ranks[r].G[i] for i in popped], np.float64)
			raw = np.float64(case[2]) * G + (-v).astype(np.float64)              # cost_record's sum, before sortable_key
			zero = raw == 0
			raw_minus += int((zero & np.signbit(raw)).sum())
			raw_plus += int((zero & ~np.signbit(raw)).sum())
			together += bool((zero & np.signbit(raw)).any() and (zero & ~np.signbit(raw)).any())
	print("world", world, "popped nodes with raw cost -0.0:", raw_minus, "+0.0:", raw_plus, "both in one rank's pops:", together)
	assert raw_minus >= 1 and raw_plus >= 1 and together >= 1
	assert any((c == 0).any() for per_rank in o.cand_costs for c in per_rank)


def test_the_counting_oracle_is_the_oracle():
	"""The GPU tests compare the engines with CountingOracle objects: they must be ShardedAStarOracle's searches, array for array."""
	name, case = "misleading", GPU_CASES["misleading"][1]
	seed, depth, lam, N, budget = case
	for world in (1, 3):
		a = sharded_oracle(name, world, case)
		b = ShardedAStarOracle(variant(name), lam, N, world)
		assert b.search(start_of(case), budget) == a.stop and (world == 1 or a.offer_hits > 0)
		assert a.pops == b.pops and a.new_counts == b.new_counts and list(a.action_queue) == list(b.action_queue)
		for r in range(world):
			assert all((x == y).all() for x, y in zip(a.arrays(r), b.arrays(r))) and a.open_queue(r) == b.open_queue(r)
			assert all((x[r].view(np.uint64) == y[r].view(np.uint64)).all() for x, y in zip(a.cand_costs, b.cand_costs))


@pytest.mark.parametrize("world", WORLDS)
def test_special_values_reach_the_gather(world):
	"""`special`: a real +inf on a rank that publishes fewer than N candidates (so it sits next to the +inf padding), and -inf, a
	float32 denormal, +1e30 and -1e30 among the candidates."""
	fs = [f for (name, _), f in _facts(world).items() if name == "special"]
	for what in ("inf_short", "neg_inf", "denormal", "plus_big", "minus_big"):
		assert any(f[what] for f in fs), what


@pytest.mark.parametrize("world", WORLDS)
def test_costs_one_float64_ulp_apart_on_two_ranks(world):
	"""The smallest gap between two distinct candidate costs on different ranks of one iteration, in float64 steps.  The tables plant
	values one FLOAT32 ulp apart, 2^29 float64 steps at lambda = 0; the cases with lambda = 2^29 bring that down to the last bit of the
	float64 cost: lambda * G is exact there and about 2^29 times a value, so the sum 2^29 G + (-value) rounds the value to the cost's
	own last bits and neighbouring costs are ONE float64 ulp apart.  Smallest gap seen: 1 ulp at world 2, 3 and 8."""
	gaps = [f["min_gap"] for f in _facts(world).values() if f["min_gap"] is not None]
	print("smallest cross-rank gap in float64 ulps per case:", gaps)
	assert min(gaps) == 1


@pytest.mark.parametrize("world", WORLDS)
def test_relaxation_crossed_the_ranks(world):
	"""`misleading`: shortcut offers hit on their parents' owners (relaxation case 2 through the exchange); case 1 ran too."""
	runs = [sharded_oracle(name, world, case) for name, case in all_cases() if name == "misleading"]
	assert sum(o.offer_hits for o in runs) >= 1
	assert sum(sharded_oracle(name, world, case).case1 for name, case in all_cases()) >= 1


@pytest.mark.parametrize("world", WORLDS)
def test_searches_end_all_three_ways(world):
	stops = {sharded_oracle(name, world, case).stop for name, case in all_cases()}
	assert stops == {STOP_WON, STOP_BUDGET}
	name, case, capacity = CAPACITY_CASE
	o = sharded_oracle(name, world, case, capacity)
	assert o.stop == STOP_CAPACITY and o.iterations > 1
	assert max(len(rk) for rk in o.ranks) + 12 * case[3] > capacity and all(len(rk) <= capacity for rk in o.ranks)


def test_a_rank_pops_more_than_one_workgroup_of_k_shard_decide():
	"""k_shard_decide handles 256 / world candidates per workgroup: 85 at world 3, 32 at world 8 (128 at world 2)."""
	for world, per_group in ((2, 128), (3, 85), (8, 32)):
		assert max(f["max_pop"] for f in _facts(world).values()) > per_group, world
