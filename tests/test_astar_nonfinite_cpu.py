"""
Why the A* engines REFUSE a NaN value (engine error 4, include/rubiks_hip.h "NON-FINITE VALUES") instead of ordering it: the written
proof, on the host alone.

The sharded engine publishes every rank's candidate costs as float64, sorted by KEY (sortable_key: a total order on bits, a NaN with
the sign bit set below -inf, one without it above +inf), and k_shard_decide ranks them across the ranks with FLOATING-POINT compares.
`decide_counts` restates that kernel's rule -- the binary search with its two compare forms, the `grank < N` cut, the +inf padding
behind a rank's candidates -- and this file asserts
  * that the restatement IS the specification (librubiks_amd.solving.sharded.select_pops) on NaN-free lists: ties across ranks, real
    -inf and +inf candidates beside the padding, empty ranks;
  * that with NaN candidates at either end of a rank's list the ranks together pop MORE than N nodes -- the bound the budget and
    capacity stops and the fixed net batch rest on.  So the engine must stop before this arithmetic runs, which it does;
  * that neither oracle nor the steps model gives a NaN to heapq: they raise ValueError.
"""
import numpy as np
import pytest

from librubiks_amd.solving.sharded import select_pops
from oracle import cube_oracle as orc
from oracle.search_oracle import AStarOracle, StubNet
from oracle.sharded_oracle import ShardedAStarOracle
from tests import astar_steps_model as sm

POS_NAN = np.uint64(0x7FF8000000000000).view(np.float64)      # cost of a NEGATIVE NaN value (cost = lambda G + (-value)): key above +inf
NEG_NAN = np.uint64(0xFFF8000000000000).view(np.float64)      # cost of a positive NaN value, what the GPU's own arithmetic produces: key below -inf


def decide_counts(heads: np.ndarray, counts, N: int) -> np.ndarray:
	"""k_shard_decide (librubiks_amd/csrc/rk_astar.hip): candidate i of rank `me` has the global rank i + sum over the other ranks r of
	the lower bound of its cost x in r's list -- `o[mid] <= x` for r < me (they win ties), `o[mid] < x` for r > me -- over r's
	counts[r] candidates (slot 4 of its contribution; +inf padding lies behind them); it is popped when that rank is below N."""
	W = heads.shape[0]
	pops = np.zeros(W, np.int64)
	for me in range(W):
		for i in range(int(counts[me])):
			x, grank = float(heads[me, i]), i
			for r in range(W):
				if r == me:
					continue
				o, lo, hi = heads[r], 0, int(counts[r])
				while lo < hi:
					mid = (lo + hi) >> 1
					if (float(o[mid]) <= x) if r < me else (float(o[mid]) < x):
						lo = mid + 1
					else:
						hi = mid
				grank += lo
			pops[me] += grank < N
	return pops


def padded(lists, N: int):
	"""(world, N) heads as the all-gather holds them and the candidate counts"""
	heads = np.full((len(lists), N), np.inf)
	for r, l in enumerate(lists):
		heads[r, :len(l)] = l
	return heads, np.array([len(l) for l in lists], np.int64)


def clean_lists(rng, world: int, N: int):
	"""NaN-free candidate lists in key order = ascending: few distinct values (ties inside a rank and across ranks), now and then a real
	-inf or +inf candidate (a net may return +-inf), short and empty ranks."""
	lists = []
	for r in range(world):
		n = int(rng.choice([0, 1, N // 2, N, N]))
		pool = np.array([-np.inf, -2.5, -1.0, 0.0, 0.5, 0.5, 1.0, 3.0, 7.25, np.inf]) if rng.randint(3) else rng.standard_normal(16).round(1)
		lists.append(np.sort(pool[rng.randint(0, len(pool), min(n, N))]))
	return lists


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("N", [1, 4, 64])
def test_restated_rank_rule_equals_select_pops_without_nan(world, N):
	rng = np.random.RandomState(100 * world + N)
	seen_inf = seen_tie = seen_empty = 0
	for _ in range(120 if N < 64 else 40):
		lists = clean_lists(rng, world, N)
		heads, counts = padded(lists, N)
		want = select_pops(heads, N, counts)
		got = decide_counts(heads, counts, N)
		assert got.tolist() == want.tolist(), (lists, got, want)
		assert got.sum() == min(N, counts.sum())
		seen_inf += any(np.isinf(l).any() for l in lists)
		seen_empty += any(len(l) == 0 for l in lists)
		seen_tie += len(np.unique(np.concatenate(lists))) < counts.sum()
	assert seen_inf and seen_tie and seen_empty


def test_the_issue_example_pops_five_of_four():
	"""world 2, N 4: by key the global top four are the NaN, 1, 2, 3 -- rank 0 pops one node and rank 1 three.  The kernel's rule:
	the NaN compares false against everything, so rank 1 never counts it and pops all four of its own: five pops."""
	heads, counts = padded([[NEG_NAN, 9.0, 9.1, 9.2], [1.0, 2.0, 3.0, 4.0]], 4)
	got = decide_counts(heads, counts, 4)
	assert got.tolist() == [1, 4] and got.sum() == 5 > 4


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("N", [4, 64])
@pytest.mark.parametrize("end", ["front", "back"])
def test_nan_candidates_break_the_bound_of_n_pops(world, N, end):
	"""k = 1..3 NaNs on one rank, where the key order puts them -- a cost NaN with the sign bit at the FRONT of the list, one without
	it at the BACK (behind the rank's finite candidates, in front of the padding) -- while the other ranks together hold at least N
	cheaper finite candidates: the finite candidates are ranked among themselves as if the NaNs were not there (N pops), and every NaN
	candidate is popped too, its rank being its own position.  N + k pops."""
	rng = np.random.RandomState(7 * world + N + (end == "back"))
	for trial in range(40):
		k = int(rng.randint(1, 4))
		p = int(rng.randint(world))
		lists = []
		for r in range(world):
			if r == p:
				finite = np.sort(100.0 + rng.standard_normal(int(rng.randint(0, N - k + 1))).round(2))      # dearer than everything elsewhere
				lists.append(np.concatenate([np.full(k, NEG_NAN), finite]) if end == "front" else np.concatenate([finite, np.full(k, POS_NAN)]))
			else:
				lists.append(np.sort(rng.standard_normal(N).round(1)))
		heads, counts = padded(lists, N)
		got = decide_counts(heads, counts, N)
		assert got.sum() == N + k > N, (trial, p, k, got)
		assert got[p] == k                                                    # the NaNs themselves; by key the front ones belong to the top N, the back ones do not
		# the same lists with the NaNs taken out: the rule holds its bound again
		clean = [l[~np.isnan(l)] for l in lists]
		h2, c2 = padded(clean, N)
		assert decide_counts(h2, c2, N).tolist() == select_pops(h2, N, c2).tolist() and decide_counts(h2, c2, N).sum() == N


class NanNet(StubNet):
	"""StubNet whose value of the `at`-th state of every batch is a NaN"""
	def __init__(self, at: int = 0):
		super().__init__()
		self.at = at

	def __call__(self, x, policy=True, value=True):
		v = np.array(super().__call__(x, policy=False, value=True), np.float32)
		v[min(self.at, len(v) - 1)] = np.nan
		return v


def test_oracles_and_the_steps_model_refuse_nan():
	np.random.seed(7)
	start, _, _ = orc.scramble(6, True)
	with pytest.raises(ValueError, match="NaN"):
		AStarOracle(NanNet(3), 0.5, 10).search(start, 5_000)
	for world in (1, 3):
		with pytest.raises(ValueError, match="NaN"):
			ShardedAStarOracle(NanNet(0), 0.5, 10, world).search(start, 5_000)
	assert AStarOracle(StubNet(), 0.5, 10).search(start, 5_000) in (True, False)        # the same search with numbers runs
	g = sm.NAN_GEOMETRIES[0]
	m = sm.StepModel(g.lambda_, g.N, g.capacity)
	m.start(sm.start_state(g), g.capacity)
	m.step(g.N, np.zeros(12, np.float32))
	before = (len(m), sorted(m.open), m.iterations)
	cum, _ = m.dry(g.N)
	for bits in (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF):
		v = np.zeros(cum[-1], np.float32)
		v[-1] = np.uint32(bits).view(np.float32)
		with pytest.raises(ValueError, match="NaN"):
			m.step(g.N, v)
		assert (len(m), sorted(m.open), m.iterations) == before                  # refused before anything changed
	for inf in (np.inf, -np.inf):                                             # infinities stay legal
		v = np.zeros(m.dry(g.N)[0][-1], np.float32)
		v[0] = inf
		assert m.step(g.N, v).n_new == len(v)


def test_nan_geometries_reach_every_value_reading_form():
	"""One run of 256; a second workgroup of k_records_sort<256>; k_records_sort<2048> with k_merge_pass."""
	forms = [sm.sort_geometry(g.N) for g in sm.NAN_GEOMETRIES]
	assert [f[1] for f in forms] == [256, 256, 2048] and forms[0][2] == 256 and forms[1][2] == 512 and forms[2][3] == "merge passes"
