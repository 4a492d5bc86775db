"""
The hash-sharded A* (rk_astar.hip section "Hash-sharded search", librubiks_amd/solving/sharded.py) against its oracle on REAL-VALUED
net outputs, bit for bit.  The nets are LookupNets (tests/test_real_valued_oracle_cpu.VARIANTS): arbitrary float32 / bfloat16 bit
patterns -- both signs, duplicates, pairs one ulp apart, zeros of both signs, with `special` denormals, +-1e30 and infinities -- that are
the same bits on the host and on the device.  tests/test_sharded_real_valued_cpu.py pins the oracle at world 1 and asserts, on the
oracle alone, that the cases below really hold what they are for (equal costs on two ranks at the N-th place, a real +inf next to the
padding, costs one float64 ulp apart, offers across ranks, more pops than one workgroup of k_shard_decide handles, ...).
  * world 2 / 3 / 8, all ranks' engines in one process (tests/test_sharded_gpu._simulate_ranks): every all-gather contribution -- the
    candidate costs as uint64, +inf behind them --, every rank's pops in every iteration, the new-state counts, the stop decision, the
    winner and the action queue, every shard array and the final open queue with its cost bits;
  * the pool-capacity stop, and the wide pop (k_pop_wide + k_shard_heads) the same way;
  * the Python driver ShardedAStar at world 1, eager and as a replayed hipGraph, on the fixture cases of tests/golden/real_trace.npz
    (the unmodified reference's searches), the bfloat16 one included.
"""
import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.sharded import ShardedAStar
from oracle.sharded_oracle import STOP_BUDGET, STOP_CAPACITY
from tests.test_real_valued_oracle_cpu import ASTAR_CASES, astar_oracle, load_trace, net_of, variant
from tests.test_real_valued_search_gpu import _check_astar
from tests.test_sharded_gpu import _simulate_ranks
from tests.test_sharded_oracle_cpu import check_shards
from tests.test_sharded_real_valued_cpu import CAPACITY_CASE, GPU_CASES, POP_LDS, WIDE_CASE, WORLDS, queue_levels, sharded_oracle, start_of

pytestmark = pytest.mark.gpu


def _run(name, world, case, capacity, oracle_capacity=None):
	seed, depth, lam, N, budget = case
	o = sharded_oracle(name, world, case, oracle_capacity)
	start = start_of(case)
	stop, queue, shards, total, iters = _simulate_ranks(world, start, lam, N, budget, capacity=capacity, oracle=o, net=variant(name),
	                                                    values_bf16=name == "bf16")
	assert total == o.total_states and stop == o.stop and iters == o.iterations
	print(name, world, case, "stop", stop, "states", total, "iterations", iters)
	return o, start, shards


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name,k", [(name, k) for name in GPU_CASES for k in range(len(GPU_CASES[name]))])
def test_simulated_ranks_equal_the_oracle_on_real_values(name, k, world):
	"""Everything _simulate_ranks compares with an oracle (see there), on keys a few ulps apart, on both sides of zero and at the
	edges of float64; then the protocol's properties on the ENGINES' arrays (every parent link, also across ranks, a move of the cube)."""
	case = GPU_CASES[name][k]
	o, start, shards = _run(name, world, case, capacity=case[4])
	check_shards(o, start, arrays=lambda r: shards[r])


@pytest.mark.parametrize("world", WORLDS)
def test_pool_capacity_stop_on_real_values(world):
	name, case, capacity = CAPACITY_CASE
	o, _, shards = _run(name, world, case, capacity=capacity, oracle_capacity=capacity)
	assert o.stop == STOP_CAPACITY and all(len(s[0]) <= capacity for s in shards)


@pytest.mark.parametrize("budget", WIDE_CASE[4])
def test_wide_pop(budget):
	"""
	The wide pop: with pop_is_wide(d) -- d.q.levels * d.N > POP_LDS = 6144 records -- k_end<true> writes only the eight header doubles
	of the all-gather contribution; k_pop_wide selects the candidates as a grid from global memory and k_shard_heads turns their
	keys into the published doubles.  The queue's depth is queue_plan's: level capacities max(4 * ceil(12 N / world), 4096) * 4^j
	until one holds capacity + 1 records, at most 12 levels.  So the smallest N that is wide at all is 513, with 12 levels, which no
	pool has (the largest capacity the engine accepts, 0x3FFFFFF0 states, gives 10 levels: N >= 615 and some 90 GB per rank).  With
	memory a test may use: 5 levels need capacity >= 64 * level 0, and level 0 is smallest on the most ranks -- world 8,
	N = 1229 (5 * 1229 = 6145): level 0 = 4 * ceil(14748 / 8) = 7376 records, capacity 480 000 > 64 * 7376 = 472 064 states per rank
	(about 40 MB each).  N = 1228 is not wide at this depth, and 4 levels would need N >= 1537.
	Budget 40 000: the wide pop runs in every one of the six iterations, but no rank's open set outgrows level 0, so the selection
	merges nothing.  Budget 110 000 is the smallest round budget at which a rank's open set passes 7376 records (level 0 spills into
	level 1) early enough for two further iterations to select from TWO levels (asserted on the oracle in the CPU file); its oracle
	takes about two seconds.
	"""
	name, world, (seed, depth, lam, N), capacity, _ = WIDE_CASE
	levels = len(queue_levels(N, world, capacity))
	assert levels * N > POP_LDS >= levels * (N - 1)
	o, start, shards = _run(name, world, (seed, depth, lam, N, budget), capacity=capacity)
	assert o.stop == STOP_BUDGET
	check_shards(o, start, arrays=lambda r: shards[r])


# ---- the Python driver at world 1 ---------------------------------------------------------------------------------------------------
class _Pool:
	"""A ShardedAStar's one shard with the attributes _check_astar reads from an AStar."""

	def __init__(self, agent: ShardedAStar):
		self.states, self.G, self.parents, self.parent_actions = agent.local_arrays()
		self.action_queue, self.n = agent.action_queue, len(agent)
		lib = _ffi.lib()
		n_open = int(lib.rk_astar_open_size(agent._h))
		costs, idx = np.zeros(n_open, np.float64), np.zeros(n_open, np.int64)
		got = lib.rk_astar_export_open(agent._h, costs.ctypes.data, idx.ctypes.data, n_open, _ffi.stream_ptr())
		assert got == n_open
		self.open_queue = list(zip(costs.tolist(), idx.tolist()))

	def __len__(self):
		return self.n


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("tag", ASTAR_CASES)
def test_driver_world1_on_the_fixture_cases(tag, graph):
	"""ShardedAStar without a process group -- records, bucketing, insert in arrival order, offers, rk_astar_shard_push_rows with the
	values in the net's own dtype -- on the searches the unmodified reference ran: pool, action queue and the whole open queue as
	(cost bits, index) pairs, eager and with the captured iteration (twice: the second search replays the kept graph)."""
	t = load_trace()
	_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
	ref, ref_solved, _ = astar_oracle(tag)
	net = net_of(t, tag)
	kw = dict(use_hipgraph=True, poll=3) if graph else {}
	agent = ShardedAStar(net, float(t[f"{tag}_lambda"]), expansions, capacity=max_states + 16, **kw)
	for again in range(2 if graph else 1):
		solved = agent.search(t[f"{tag}_start"], None, max_states)
		if graph:
			assert agent.graph_error is None and agent.captures == 1
		_check_astar(_Pool(agent), ref, ref_solved, solved, (tag, graph, again))
		assert agent.iterations == len(ref.pops) and agent.total_states == len(ref)
	if bool(t[f"{tag}_net"][3]):                                   # the values really went in as bfloat16
		assert net(torch.zeros(2, 480, device="cuda"), policy=False).dtype == torch.bfloat16
