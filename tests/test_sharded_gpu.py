"""
GPU tests of the hash-sharded A* (librubiks_amd/solving/sharded.py, rk_astar_shard_*).
  * world = 1 (no process group): the sharded code path -- records, bucketing, insert in arrival order, shortcut
    offers -- must reproduce the reference traces and the single-GPU engine exactly;
  * world = 2 and 3: several ranks share the one GPU of the test box and exchange through gloo (host-staged):
    every rank reports the same verdict and a valid action queue, every stored state sits on its owner rank exactly
    once, G is consistent along parent links inside a shard, results are deterministic.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import AStar
from librubiks_amd.solving.sharded import ShardedAStar
from oracle import cube_oracle as orc
from oracle.search_oracle import AStarOracle, NoisyStubNet, StubNet

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", ["a", "b", "d", "e", "f"])
def test_world1_reproduces_reference_traces(golden, tag):
	"""e, f: the reference's traces with the misleading NoisyStubNet (relaxation cases 1 and 2 really happen): the sharded engine's
	offers -- case 2 deferred to the next exchange, last hit per parent wins -- must give the reference's arrays."""
	t = golden["astar_trace"]
	_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
	agent = ShardedAStar(NoisyStubNet() if tag in ("e", "f") else StubNet(), float(t[f"{tag}_lambda"]), expansions, capacity=max_states + 16)
	solved = agent.search(t[f"{tag}_start"], None, max_states)
	n = int(t[f"{tag}_n"])
	assert solved == bool(t[f"{tag}_solved"]) and len(agent) == n
	states, G, parents, pact = agent.local_arrays()
	assert (states[1:] == t[f"{tag}_states"]).all() and (G[1:] == t[f"{tag}_G"]).all()
	assert (parents[2:] == t[f"{tag}_parents"]).all() and (pact[2:] == t[f"{tag}_parent_actions"]).all()
	assert list(agent.action_queue) == t[f"{tag}_action_queue"].tolist()


@pytest.mark.parametrize("seed,depth,lam,n,budget", [(103, 9, 1.0, 128, 30_000), (104, 6, 0.05, 1000, 40_000), (107, 12, 0.2, 400, 120_000)])
def test_world1_equals_oracle(seed, depth, lam, n, budget):
	np.random.seed(seed)
	start, _, _ = orc.scramble(depth, True)
	ref = AStarOracle(StubNet(), lam, n)
	ref_solved = ref.search(start, budget)
	agent = ShardedAStar(StubNet(), lam, n, capacity=budget + 16)
	assert agent.search(start, None, budget) == ref_solved
	states, G, parents, pact = agent.local_arrays()
	rs, rG, rp, ra = ref.arrays()
	assert (states[1:] == rs).all() and (G[1:] == rG).all() and (parents[2:] == rp).all() and (pact[2:] == ra).all()
	assert list(agent.action_queue) == list(ref.action_queue)


def _simulate_ranks(world, start, lam, N, budget, capacity, oracle=None, net=None, values_bf16=False, short_rows=None, inspect=None,
                    short_tail=float("-inf")):
	"""
	All `world` ranks of a sharded search in ONE process on one GPU: one engine per rank, the two collectives done by hand
	(all-gather = stack the contributions, all-to-all = transpose the send blocks).  Checks on the way that every rank takes
	the same stop decision and that the device's global top-N selection equals the host statement of the rule.
	With `oracle` (a ShardedAStarOracle that has run the same search on the CPU) every iteration's pops and new-state counts
	of every rank, and at the end every rank's whole shard -- states, G, parents, parent ranks, actions, open queue -- are
	compared with it BIT FOR BIT (VERDICT r3 #1b) -- and every all-gather contribution: the candidate costs a rank publishes are the
	oracle's float64 costs bit for bit, +inf behind them.
	`values_bf16`: the net returns bfloat16 values; the engines are told so (rk_astar_set_values_dtype) and read the tensor as it is.
	`short_rows`: every push promises values for this many rows only and hands over a view of that length at the front of a larger
	tensor whose tail is `short_tail`: -inf (a value no net row holds) or a NaN (which would end the search with error 4 if it were
	read); `inspect(rank, handle, new states of the last iteration)` runs before the engines go away.
	"""
	import ctypes as C
	from librubiks_amd.solving.sharded import net_rows, select_pops
	lib, st = _ffi.lib(), _ffi.stream_ptr
	hs, sends, mines = [], [], []
	for r in range(world):
		h = C.c_void_p()
		_ffi.check(lib.rk_astar_create_sharded(C.byref(h), capacity, N, r, world))
		_ffi.check(lib.rk_astar_set_values_dtype(h, _ffi.OH_BF16 if values_bf16 else _ffi.OH_F32))
		send = torch.zeros((world, int(lib.rk_astar_shard_block_bytes(h))), dtype=torch.uint8, device="cuda")
		mine = torch.zeros(int(lib.rk_astar_shard_gather_len(h)), dtype=torch.float64, device="cuda")
		_ffi.check(lib.rk_astar_shard_bind(h, mine.data_ptr()))
		_ffi.check(lib.rk_astar_shard_reset(h, start.ctypes.data, lam, send.data_ptr(), st()))
		hs.append(h); sends.append(send); mines.append(mine)
	oh = torch.zeros((12 * N, 480), device="cuda")        # 12 N rows whatever the world size: all ranks together pop N nodes
	net = net or StubNet()
	dec = (C.c_longlong * 8)()
	n_new = (C.c_int * 1)()
	pops = np.zeros(N, np.int64)
	iters, news = 0, []
	while True:
		gathered = torch.stack(mines).contiguous()
		heads = gathered.cpu().numpy()
		if oracle is not None:
			# what every rank publishes -- also in the gather that takes the stop decision: its n_r candidate costs, then +inf up to N
			assert iters < len(oracle.cand_costs), "the device goes on where the oracle stopped"
			for r in range(world):
				n_r, cost = int(heads[r, 4]), oracle.cand_costs[iters][r]
				assert heads[r, 4] == len(cost) <= N, (iters, r, heads[r, 4], len(cost))
				assert (heads[r, 8:8 + n_r].view(np.uint64) == cost.view(np.uint64)).all(), (iters, r)
				assert np.isposinf(heads[r, 8 + n_r:]).all() and heads.shape[1] == 8 + N, (iters, r)
		decisions = []
		for r in range(world):
			_ffi.check(lib.rk_astar_shard_select(hs[r], gathered.data_ptr(), 1e10, float(budget), sends[r].data_ptr(), st()))
			_ffi.check(lib.rk_astar_shard_decision(hs[r], dec, st()))
			decisions.append(list(dec))
		stop = decisions[0][0]
		assert all(d[:4] == decisions[0][:4] for d in decisions)          # same stop, winner and total everywhere
		if stop:
			break
		want = select_pops(heads[:, 8:], N, heads[:, 4])                  # (slot 4: the candidates of a row; an open node may cost +inf)
		assert [d[4] for d in decisions] == want.tolist(), (iters, [d[4] for d in decisions], want)
		if oracle is not None:
			assert iters < len(oracle.pops), "the device goes on where the oracle stopped"
			for r in range(world):
				got = lib.rk_astar_next_pops(hs[r], pops.ctypes.data, N, st())
				assert pops[:got].tolist() == oracle.pops[iters][r], (iters, r)   # the very nodes, in pop order
		recvs = [torch.stack([sends[src][r] for src in range(world)]).contiguous() for r in range(world)]
		news = []
		for r in range(world):
			_ffi.check(lib.rk_astar_shard_insert(hs[r], recvs[r].data_ptr(), sends[r].data_ptr(), oh.data_ptr(), _ffi.OH_F32, st()))
			_ffi.check(lib.rk_astar_shard_new_count(hs[r], n_new, st()))
			torch.cuda.synchronize()
			assert 0 <= n_new[0] <= 12 * N, (iters, r, n_new[0])            # a rank never appends more than 12 N states
			news.append(n_new[0])
			values = net(oh, policy=False, value=True).reshape(-1).contiguous()
			assert values.dtype == (torch.bfloat16 if values_bf16 else torch.float32) and values.is_cuda     # bfloat16 goes in unconverted
			# what the driver does: values promised for a fixed number of rows (the rank's expected share + 6 sigma + 64), which also
			# sizes this iteration's sort / insert launches (shard_push_impl); the whole-batch entry on every third iteration
			if short_rows is not None:
				# (the tail covers the sort's whole rounded-up geometry: whatever the engine reads stays inside this allocation)
				padded = torch.full((short_rows + 4096,), short_tail, dtype=values.dtype, device="cuda")
				padded[:short_rows] = values[:short_rows]
				_ffi.check(lib.rk_astar_shard_push_rows(hs[r], padded[:short_rows].data_ptr(), short_rows, recvs[r].data_ptr(), sends[r].data_ptr(), st()))
			elif iters % 3 == 2:
				_ffi.check(lib.rk_astar_shard_push(hs[r], values.data_ptr(), recvs[r].data_ptr(), sends[r].data_ptr(), st()))
			else:
				_ffi.check(lib.rk_astar_shard_push_rows(hs[r], values.data_ptr(), net_rows(12 * N, world), recvs[r].data_ptr(), sends[r].data_ptr(), st()))
			torch.cuda.synchronize()
		assert sum(news) <= 12 * N                                          # ... and all ranks together no more than 12 N either
		if oracle is not None:
			assert news == oracle.new_counts[iters], (iters, news, oracle.new_counts[iters])
		iters += 1
		assert iters < 100_000
	queue = None
	if stop == 1:
		rank, idx = decisions[0][1], decisions[0][2]
		root_owner = lib.rk_shard_owner(start.ctypes.data, world)
		hop, queue = (C.c_longlong * 3)(), []
		while not (rank == root_owner and idx == 1):
			_ffi.check(lib.rk_astar_shard_parent(hs[rank], idx, hop, st()))
			queue.insert(0, int(hop[2]))
			rank, idx = int(hop[0]), int(hop[1])
			assert len(queue) < 1000
	else:
		recvs = [torch.stack([sends[src][r] for src in range(world)]).contiguous() for r in range(world)]
		for r in range(world):
			_ffi.check(lib.rk_astar_shard_flush(hs[r], recvs[r].data_ptr(), st()))
	shards = []
	for r in range(world):
		n = decisions[r][6]
		states, G = np.zeros((n, 20), np.int8), np.zeros(n)
		parents, prank, pact = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
		if n:
			_ffi.check(lib.rk_astar_export(hs[r], 1, n, states.ctypes.data, G.ctypes.data, parents.ctypes.data, pact.ctypes.data, st()))
			_ffi.check(lib.rk_astar_shard_export_ranks(hs[r], 1, n, prank.ctypes.data, st()))
		shards.append((states, G, parents, prank, pact))
		if oracle is not None:
			os_, oG, op, orank, oa = oracle.arrays(r)
			assert n == len(os_), (r, n, len(os_))
			assert (states == os_).all() and (G == oG).all(), r
			assert (parents == op).all() and (prank == orank).all() and (pact == oa).all(), r
			n_open = int(lib.rk_astar_open_size(hs[r]))
			costs, idx = np.zeros(n_open), np.zeros(n_open, np.int64)
			got = lib.rk_astar_export_open(hs[r], costs.ctypes.data, idx.ctypes.data, n_open, st())
			assert list(zip(costs[:got].tolist(), idx[:got].tolist())) == [(c, i) for c, i in oracle.open_queue(r)], r
			want_costs = np.array([float(c) for c, _ in oracle.open_queue(r)], np.float64)
			assert got == n_open == len(want_costs) and (costs.view(np.uint64) == want_costs.view(np.uint64)).all(), r     # bits: a -0.0 the engine kept would show
		if inspect is not None:
			inspect(r, hs[r], news[r] if news else 0)
		lib.rk_astar_destroy(hs[r])
	if oracle is not None:
		assert iters == oracle.iterations and stop == oracle.stop
		if stop == 1:
			assert (decisions[0][1], decisions[0][2]) == oracle.winner and queue == list(oracle.action_queue)
	return stop, queue, shards, decisions[0][3], iters


@pytest.mark.parametrize("world", [2, 3, 8])
def test_ranks_simulated_in_one_process(world):
	lib = _ffi.lib()
	for seed, depth, lam, N, budget in [(7, 6, 0.5, 10, 30_000), (19, 7, 0.1, 300, 60_000), (405, 8, 0.5, 30, 40_000)]:
		np.random.seed(seed)
		start, _, _ = orc.scramble(depth, True)
		stop, queue, shards, total, iters = _simulate_ranks(world, start, lam, N, budget, capacity=budget)
		stop2, queue2, shards2, total2, iters2 = _simulate_ranks(world, start, lam, N, budget, capacity=budget)
		assert (stop, queue, total, iters) == (stop2, queue2, total2, iters2)          # deterministic
		assert all((a[k] == b[k]).all() for a, b in zip(shards, shards2) for k in range(5))
		if stop == 1:
			s = start
			for a in queue:
				s = orc.rotate(s, a // 2, 1 - a % 2)
			assert orc.is_solved(s)
		else:
			assert stop == 2 and total + 12 * N > budget >= total          # the reference's guard (agents.py:236), whatever the world size
		seen = set()
		for r, (states, G, _, _, _) in enumerate(shards):
			owners = np.array([lib.rk_shard_owner(np.ascontiguousarray(x).ctypes.data, world) for x in states[:: max(1, len(states) // 300)]])
			assert (owners == r).all()
			keys = {x.tobytes() for x in states}
			assert len(keys) == len(states) and not (keys & seen)
			seen |= keys
		assert len(seen) == total and start.tobytes() in seen


@pytest.mark.parametrize("world", [2, 3, 8])
def test_ranks_simulated_equal_the_sharded_oracle(world):
	"""VERDICT r3 #1b / "What's missing" 4: the world > 1 engines against the CPU restatement of the protocol
	(oracle/sharded_oracle.py, pinned at world = 1 to the reference's traces): every iteration's pops of every rank, the new
	states per rank, the stop decision, and at the end every rank's states, G, parents, parent RANKS, actions and open queue,
	bit for bit; then the cross-rank walk of the parent links on the engines' arrays (every link a real move of the cube)."""
	from oracle.sharded_oracle import ShardedAStarOracle
	from tests.test_sharded_oracle_cpu import check_shards
	for seed, depth, lam, N, budget in [(7, 6, 0.5, 10, 30_000), (19, 7, 0.1, 300, 60_000), (405, 8, 0.5, 30, 40_000), (107, 12, 0.2, 400, 120_000)]:
		np.random.seed(seed)
		start, _, _ = orc.scramble(depth, True)
		o = ShardedAStarOracle(StubNet(), lam, N, world)
		o.search(start, budget)
		stop, queue, shards, total, iters = _simulate_ranks(world, start, lam, N, budget, capacity=budget, oracle=o)
		assert total == o.total_states
		check_shards(o, start, arrays=lambda r: shards[r])
	# a misleading heuristic: dozens of shortcut offers cross the ranks, several on one parent in one exchange (last hit wins)
	for seed, depth, lam, N, budget in [(11, 14, 0.05, 50, 60_000), (12, 16, 0.02, 200, 40_000)]:
		np.random.seed(seed)
		start, _, _ = orc.scramble(depth, True)
		o = ShardedAStarOracle(NoisyStubNet(), lam, N, world)
		o.search(start, budget)
		stop, queue, shards, total, iters = _simulate_ranks(world, start, lam, N, budget, capacity=budget, oracle=o, net=NoisyStubNet())
		assert total == o.total_states
	# the capacity stop is the oracle's too
	np.random.seed(42)
	start, _, _ = orc.scramble(14, True)
	o = ShardedAStarOracle(StubNet(), 0.2, 100, world)
	assert o.search(start, 10_000_000, capacity=9_000) == 3
	assert _simulate_ranks(world, start, 0.2, 100, 10_000_000, capacity=9_000, oracle=o)[0] == 3


def test_configs4_full_workload_on_8_simulated_ranks():
	"""VERDICT r3 #1c: BASELINE.json configs[4] at its own workload -- a depth-20 scramble, lambda 0.16, N = 700
	(configs/main_eval.ini:8-9), a budget of 2 M states -- on 8 ranks' engines in one process, every iteration and every
	shard compared bit for bit with the CPU oracle of the protocol, which replays the whole budget."""
	import time
	from oracle.sharded_oracle import ShardedAStarOracle
	from tests.test_sharded_oracle_cpu import check_shards
	world, N, lam, budget = 8, 700, 0.16, 2_000_000
	np.random.seed(0)
	start, _, _ = orc.scramble(20, True)
	t0 = time.perf_counter()
	o = ShardedAStarOracle(StubNet(), lam, N, world)
	o.search(start, budget)
	t1 = time.perf_counter()
	stop, queue, shards, total, iters = _simulate_ranks(world, start, lam, N, budget, capacity=420_000, oracle=o)
	t2 = time.perf_counter()
	print(f"configs[4] workload: stop {stop}, {total} states in {iters} iterations on {world} ranks; oracle {t1 - t0:.1f} s, engines with per-iteration checks {t2 - t1:.1f} s")
	assert total == o.total_states and (stop == 1 or (stop == 2 and total + 12 * N > budget >= total))
	assert iters > 200 and min(len(s[0]) for s in shards) > 0.8 * total / world          # a real search, evenly sharded
	check_shards(o, start, arrays=lambda r: shards[r])
	if stop == 1:
		s = start
		for a in queue:
			s = orc.rotate(s, a // 2, 1 - a % 2)
		assert orc.is_solved(s)


def test_pool_capacity_stops_every_rank_together():
	"""A budget larger than what the per-rank pools hold must end the search on all ranks at once (no rank left in a
	collective): stop reason 3, decided from the all-gathered pool sizes."""
	np.random.seed(42)
	start, _, _ = orc.scramble(14, True)
	stop, queue, shards, total, iters = _simulate_ranks(3, start, 0.2, 100, budget=10_000_000, capacity=9_000)
	assert stop == 3 and queue is None and iters > 1
	assert max(len(s[0]) for s in shards) + 12 * 100 > 9_000 and all(len(s[0]) <= 9_000 for s in shards)
	agent = ShardedAStar(StubNet(), 0.2, 100, capacity=9_000)                 # the agent reports it too (world = 1)
	assert agent.search(start, None, 10_000_000) is False and agent.stop_reason == "capacity"


def test_short_net_batch_reads_no_value_beyond_its_rows():
	"""A push that promises fewer rows than the iteration has new states (rk_astar_shard_push_rows): the sort geometry is `rows`
	rounded UP to a whole chunk, yet the states beyond `rows` are padding in the sort, the insert and the end -- no value past
	values[rows - 1] reaches a cost record -- and the engine reports ERR_NET_ROWS (status word 6 = 3), on which all ranks stop.
	The values tensor is a view at the front of a larger one whose tail holds -inf, a cost of +inf that nothing else produces
	(StubNet's values are small integers): the read, if it happened, would stay inside the allocation and show in the open queue."""
	import ctypes as C
	lib, world, N, rows = _ffi.lib(), 2, 300, 64
	np.random.seed(19)
	start, _, _ = orc.scramble(9, True)
	seen = []

	def inspect(r, h, n_new):
		status = (C.c_longlong * 8)()
		_ffi.check(lib.rk_astar_status(h, status, _ffi.stream_ptr()))
		n_open = int(lib.rk_astar_open_size(h))
		costs, idx = np.zeros(n_open + 1), np.zeros(n_open + 1, np.int64)
		got = lib.rk_astar_export_open(h, costs.ctypes.data, idx.ctypes.data, n_open + 1, _ffi.stream_ptr())
		seen.append((r, n_new, int(status[6]), got, costs[:got].copy()))

	stop, queue, shards, total, iters = _simulate_ranks(world, start, 0.5, N, 60_000, capacity=60_000, short_rows=rows, inspect=inspect)
	assert stop == 6 and queue is None and 2 <= iters <= 4, (stop, iters)           # the first iteration with more than 64 new states on a rank
	assert len(seen) == world and any(n_new > rows for _, n_new, _, _, _ in seen)
	for r, n_new, err, n_open, costs in seen:
		assert err == (3 if n_new > rows else 0), (r, n_new, err)
		assert n_open > 0 and np.isfinite(costs).all(), (r, "a value from beyond the promised rows became a cost")
		assert (costs == np.round(costs * 2) / 2).all(), r                          # lambda G + small integers, nothing else


def _free_port():
	with socket.socket() as s:
		s.bind(("127.0.0.1", 0))
		return s.getsockname()[1]


def _rank_main(rank, world, port, out_dir, cases):
	import torch.distributed as dist
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
	dist.init_process_group("gloo", rank=rank, world_size=world)
	try:
		torch.cuda.set_device(0)
		for ci, (seed, depth, lam, n, budget) in enumerate(cases):
			np.random.seed(seed)
			start, _, _ = orc.scramble(depth, True)
			agent = ShardedAStar(StubNet(), lam, n, capacity=budget)
			solved = agent.search(start, None, budget)
			states, G, parents, pact = agent.local_arrays()
			np.savez(os.path.join(out_dir, f"c{ci}_r{rank}.npz"), solved=solved, queue=np.array(agent.action_queue, dtype=np.int64),
			         states=states[1:], G=G[1:], parents=parents[1:], pact=pact[1:], prank=agent.local_parent_ranks()[1:],
			         n=len(agent), total=agent.total_states, iters=agent.iterations, start=start)
	finally:
		dist.destroy_process_group()


CASES = [(7, 6, 0.5, 10, 30_000), (19, 7, 0.1, 300, 60_000), (402, 6, 1.0, 50, 30_000), (404, 5, 0.2, 200, 40_000), (405, 8, 0.5, 30, 40_000)]


@pytest.mark.parametrize("world", [2, 3])
def test_multi_rank_on_one_gpu(world, tmp_path):
	for attempt in range(2):                      # run twice: results must be deterministic
		d = tmp_path / f"run{attempt}"
		d.mkdir()
		mp.spawn(_rank_main, args=(world, _free_port(), str(d), CASES), nprocs=world, join=True)
	lib = _ffi.lib()
	n_solved = 0
	for ci, (seed, depth, lam, n, budget) in enumerate(CASES):
		runs = [[np.load(tmp_path / f"run{a}" / f"c{ci}_r{r}.npz") for r in range(world)] for a in range(2)]
		first = runs[0]
		start = first[0]["start"]
		# same verdict and action queue on every rank, both runs
		for run in runs:
			for z in run:
				assert bool(z["solved"]) == bool(first[0]["solved"]) and z["queue"].tolist() == first[0]["queue"].tolist()
				assert int(z["total"]) == int(first[0]["total"])
		for r in range(world):
			assert (runs[0][r]["states"] == runs[1][r]["states"]).all() and (runs[0][r]["G"] == runs[1][r]["G"]).all()
		# the real driver -- separate processes, collectives over gloo, the net in two pieces -- against the protocol's CPU oracle:
		# every rank's shard bit for bit, the iteration count and the action queue (VERDICT r3 #1b)
		from oracle.sharded_oracle import ShardedAStarOracle
		o = ShardedAStarOracle(StubNet(), lam, n, world)
		stop = o.search(start, budget)
		assert (stop == 1) == bool(first[0]["solved"]) and int(first[0]["iters"]) == o.iterations
		assert first[0]["queue"].tolist() == list(o.action_queue)
		for r in range(world):
			os_, oG, op, orank, oa = o.arrays(r)
			z = first[r]
			assert (z["states"] == os_).all() and (z["G"] == oG).all() and (z["parents"] == op).all(), (ci, r)
			assert (z["prank"] == orank).all() and (z["pact"] == oa).all(), (ci, r)
		# the action queue solves the cube
		if first[0]["solved"]:
			n_solved += 1
			s = start
			for a in first[0]["queue"]:
				s = orc.rotate(s, a // 2, 1 - a % 2)
			assert orc.is_solved(s)
			# never worse than what the oracle's single-queue search finds under the same budget, if it finds one
			ref = AStarOracle(StubNet(), lam, n)
			if ref.search(start, budget):
				assert len(first[0]["queue"]) <= len(ref.action_queue) + 2
		# every state lives on its owner rank, exactly once overall; G is the length of a real path bound
		seen = set()
		total = 0
		for r in range(world):
			st = first[r]["states"]
			total += len(st)
			assert len(st) == int(first[r]["n"])
			owners = np.array([lib.rk_shard_owner(np.ascontiguousarray(x).ctypes.data, world) for x in st[:: max(1, len(st) // 500)]])
			assert (owners == r).all()
			keys = {x.tobytes() for x in st}
			assert len(keys) == len(st) and not (keys & seen)
			seen |= keys
		assert total == int(first[0]["total"]) and start.tobytes() in seen
		assert total <= budget
	assert n_solved >= 3


def _rank_fc_small(rank, world, port, out_dir, fused):
	import torch.distributed as dist
	from benchmarks.nets import FcSmall
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
	dist.init_process_group("gloo", rank=rank, world_size=world)
	try:
		torch.cuda.set_device(0)
		net = FcSmall(seed=4).cuda().eval()
		np.random.seed(77)
		start, _, _ = orc.scramble(12, True)
		agent = ShardedAStar(net, 0.2, 100, capacity=60_000, fused_first_layer=fused)
		solved = agent.search(start, None, 40_000)
		states, G, parents, pact = agent.local_arrays()
		np.savez(os.path.join(out_dir, f"fc_r{rank}.npz"), solved=solved, queue=np.array(agent.action_queue, dtype=np.int64), states=states[1:],
		         n=len(agent), total=agent.total_states, iters=agent.iterations, rows_max=agent.net_rows_max, rows_total=agent.net_rows_total, start=start)
	finally:
		dist.destroy_process_group()


@pytest.mark.parametrize("fused", [False, "folded"])
def test_net_batch_is_bounded_by_12n_not_by_the_world(tmp_path, fused):
	"""VERDICT r2 #2 / ADVICE r2: with a real net (random-init fc_small) at 2 ranks the rows pushed through the net per iteration
	never exceed 12 N, and on average stay near a rank's share 12 N / world instead of world * 12 N."""
	world, N = 2, 100
	mp.spawn(_rank_fc_small, args=(world, _free_port(), str(tmp_path), fused), nprocs=world, join=True)
	z = [np.load(tmp_path / f"fc_r{r}.npz") for r in range(world)]
	assert bool(z[0]["solved"]) == bool(z[1]["solved"]) and z[0]["queue"].tolist() == z[1]["queue"].tolist()
	assert int(z[0]["iters"]) == int(z[1]["iters"]) > 3
	seen = set()
	for r in range(world):
		assert 0 < int(z[r]["rows_max"]) <= 12 * N
		assert int(z[r]["rows_total"]) <= 0.8 * 12 * N * int(z[r]["iters"])       # near 12 N / world + rounding, far from 12 N
		keys = {x.tobytes() for x in z[r]["states"]}
		assert len(keys) == len(z[r]["states"]) == int(z[r]["n"]) and not (keys & seen)
		seen |= keys
	assert len(seen) == int(z[0]["total"])
	if z[0]["solved"]:
		s = z[0]["start"]
		for a in z[0]["queue"]:
			s = orc.rotate(s, a // 2, 1 - a % 2)
		assert orc.is_solved(s)


def _rank_capacity(rank, world, port, out_dir):
	import torch.distributed as dist
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
	dist.init_process_group("gloo", rank=rank, world_size=world)
	try:
		torch.cuda.set_device(0)
		np.random.seed(42)
		start, _, _ = orc.scramble(14, True)
		agent = ShardedAStar(StubNet(), 0.2, 100, capacity=9_000, poll=2)
		solved = agent.search(start, None, 10_000_000)                        # budget far beyond world * capacity
		np.savez(os.path.join(out_dir, f"cap_r{rank}.npz"), solved=solved, reason=agent.stop_reason, n=len(agent), iters=agent.iterations)
	finally:
		dist.destroy_process_group()


def test_multi_rank_capacity_stop_gloo(tmp_path):
	"""with capacity < budget no rank may run into ECAPACITY while its peers wait in a collective."""
	mp.spawn(_rank_capacity, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
	z = [np.load(tmp_path / f"cap_r{r}.npz") for r in range(2)]
	assert all(str(x["reason"]) == "capacity" and not bool(x["solved"]) for x in z)
	assert int(z[0]["iters"]) == int(z[1]["iters"]) > 1 and all(int(x["n"]) <= 9_000 for x in z)


def _nccl_world1(rank, port, out_path, case):
	"""One rank, nccl backend, collectives forced: the RCCL transport (device tensors, variable-size all_to_all_single,
	all_gather_into_tensor, broadcast) carries a whole search."""
	import torch.distributed as dist
	torch.cuda.set_device(0)
	# one rank: a file store needs no port (a port found free by the parent can be taken again before the child binds it)
	dist.init_process_group("nccl", init_method=f"file://{out_path}.rendezvous", rank=0, world_size=1, device_id=torch.device("cuda", 0))
	try:
		seed, depth, lam, n, budget = case
		np.random.seed(seed)
		start, _, _ = orc.scramble(depth, True)
		agent = ShardedAStar(StubNet(), lam, n, capacity=budget + 16, force_collectives=True)
		assert agent.tp.backend == "nccl" and agent.tp.on_device and not agent.tp.shortcut
		solved = agent.search(start, None, budget)
		states, G, parents, pact = agent.local_arrays()
		np.savez(out_path, solved=solved, states=states[1:], G=G[1:], parents=parents[2:], pact=pact[2:], queue=np.array(agent.action_queue, dtype=np.int64))
	finally:
		dist.destroy_process_group()


def test_rccl_transport_world1(tmp_path):
	case = (19, 7, 0.1, 300, 60_000)
	out = str(tmp_path / "nccl.npz")
	mp.spawn(_nccl_world1, args=(_free_port(), out, case), nprocs=1, join=True)
	z = np.load(out)
	seed, depth, lam, n, budget = case
	np.random.seed(seed)
	start, _, _ = orc.scramble(depth, True)
	ref = AStarOracle(StubNet(), lam, n)
	assert ref.search(start, budget) == bool(z["solved"])
	rs, rG, rp, ra = ref.arrays()
	assert (z["states"] == rs).all() and (z["G"] == rG).all() and (z["parents"] == rp).all() and (z["pact"] == ra).all()
	assert z["queue"].tolist() == list(ref.action_queue)


def _rank_partitioned_mcts(rank, world, port, out_dir):
	import torch.distributed as dist
	from librubiks_amd.solving.sharded import PartitionedMCTS
	from oracle.search_oracle import PolicyStubNet
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
	dist.init_process_group("gloo", rank=rank, world_size=world)
	try:
		torch.cuda.set_device(0)
		agent = PartitionedMCTS(PolicyStubNet(), 1.5, len(_MCTS_STARTS()), capacity=2500)
		solved = agent.search(_MCTS_STARTS(), max_states=2500, max_sims=400)
		np.savez(os.path.join(out_dir, f"pm_r{rank}.npz"), solved=solved, states=agent.states, sims=agent.sims, mine=agent.mine,
		         queues=np.array([list(agent.action_queue_of(t)) + [-1] * (64 - len(agent.action_queue_of(t))) for t in range(agent.n_trees)]))
	finally:
		dist.destroy_process_group()


def _MCTS_STARTS():
	out = []
	for i in range(7):                                                       # an odd number: the ranks get 4 and 3 trees
		np.random.seed(300 + i)
		out.append(orc.scramble(4 + i % 3, True)[0])
	return np.array(out)


def test_partitioned_mcts_gloo(tmp_path):
	"""configs[3] at N > 1: trees partitioned over ranks, no collective in the loop; every rank ends with the whole batch's
	results, and they equal one MCTSBatch over all trees (each tree is the reference's search of its start state alone)."""
	from librubiks_amd.solving.agents import MCTSBatch
	from oracle.search_oracle import PolicyStubNet
	mp.spawn(_rank_partitioned_mcts, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
	z = [np.load(tmp_path / f"pm_r{r}.npz") for r in range(2)]
	assert z[0]["mine"].tolist() == [0, 2, 4, 6] and z[1]["mine"].tolist() == [1, 3, 5]
	for k in ("solved", "states", "sims", "queues"):
		assert (z[0][k] == z[1][k]).all()
	starts = _MCTS_STARTS()
	one = MCTSBatch(PolicyStubNet(), 1.5, len(starts), capacity=2500)
	solved = one.search(starts, max_states=2500, max_sims=400)
	assert (solved == z[0]["solved"]).all() and 2 <= solved.sum() < len(starts)      # solved and unsolved trees both covered
	assert (one.status[:, 2] == z[0]["states"]).all()
	for t in range(len(starts)):
		q = [a for a in z[0]["queues"][t] if a >= 0]
		assert q == list(one.action_queue_of(t) if solved[t] else [])
		if solved[t]:
			s = starts[t]
			for a in q:
				s = orc.rotate(s, a // 2, 1 - a % 2)
			assert orc.is_solved(s)


def test_sharded_world1_with_fused_first_layer():
	"""ShardedAStar hands the net the new nodes' 20-byte states (RK_OH_STATES through rk_astar_shard_insert): at world 1
	it is the single-GPU engine with the same option, node for node (same fixed batch shape, so the same net numbers)."""
	from benchmarks.nets import FcSmall
	net = FcSmall(seed=4).cuda().eval()
	np.random.seed(77)
	start, _, _ = orc.scramble(10, True)
	one = AStar(net, 0.2, 50, fused_first_layer=True)
	many = ShardedAStar(net, 0.2, 50, capacity=30_000, fused_first_layer=True)
	a, b = one.search(start, None, 20_000), many.search(start, None, 20_000)
	assert a == b and len(one) == len(many)
	states, G, parents, pact = many.local_arrays()
	n = len(one)
	assert (states[1:n + 1] == one.states[1:n + 1]).all() and (G[1:n + 1] == one.G[1:n + 1]).all()
	if a:
		assert list(one.action_queue) == list(many.action_queue)


def _rk_comm_world1(rank, out_path, case):
	"""One rank over the C ABI's own RCCL layer (rk_comm_*): no torch.distributed anywhere in this process."""
	from librubiks_amd.solving.sharded import RcclTransport
	torch.cuda.set_device(0)
	seed, depth, lam, n, budget = case
	np.random.seed(seed)
	start, _, _ = orc.scramble(depth, True)
	tp = RcclTransport(RcclTransport.unique_id(), 0, 1)
	agent = ShardedAStar(StubNet(), lam, n, capacity=budget + 16, transport=tp)
	assert not agent.tp.shortcut and agent.tp.on_device
	solved = agent.search(start, None, budget)
	states, G, parents, pact = agent.local_arrays()
	# the raw transfers, checked on known bytes: all-gather and all-to-all of one rank are copies, broadcast leaves the buffer alone
	a = torch.arange(40, dtype=torch.float64, device="cuda")
	assert torch.equal(tp.all_gather(a)[0], a)
	s, r = torch.randint(0, 255, (1, 4096), dtype=torch.uint8, device="cuda"), torch.zeros((1, 4096), dtype=torch.uint8, device="cuda")
	assert torch.equal(tp.all_to_all(s, r), s)
	assert tp.broadcast_vec(np.array([3, 5, 7]), 0).tolist() == [3, 5, 7]
	np.savez(out_path, solved=solved, states=states[1:], G=G[1:], parents=parents[2:], pact=pact[2:], queue=np.array(agent.action_queue, dtype=np.int64),
	         collectives=tp.collectives, iters=agent.iterations)


def test_rk_comm_transport_world1(tmp_path):
	"""the hash-sharded search driven through rk_comm_* (RCCL behind the C ABI) instead of torch.distributed --
	the route a ctypes-only caller takes to configs[4].  One rank on the one-GPU box: the collectives really run (all-gather,
	grouped send/recv, broadcast on device buffers) and the search equals the oracle's, array by array."""
	case = (19, 7, 0.1, 300, 60_000)
	out = str(tmp_path / "rkcomm.npz")
	mp.spawn(_rk_comm_world1, args=(out, case), nprocs=1, join=True)
	z = np.load(out)
	seed, depth, lam, n, budget = case
	np.random.seed(seed)
	start, _, _ = orc.scramble(depth, True)
	ref = AStarOracle(StubNet(), lam, n)
	assert ref.search(start, budget) == bool(z["solved"])
	rs, rG, rp, ra = ref.arrays()
	assert (z["states"] == rs).all() and (z["G"] == rG).all() and (z["parents"] == rp).all() and (z["pact"] == ra).all()
	assert z["queue"].tolist() == list(ref.action_queue)
	assert int(z["collectives"]) >= 2 * int(z["iters"])                        # two collectives per iteration went through RCCL


# ------------------------------------------------------------------------------------------------- round 5: the iteration is host-free and capturable
@pytest.mark.parametrize("tag", ["a", "b", "d", "e", "f"])
def test_world1_captured_iteration_reproduces_reference_traces(golden, tag):
	"""the sharded iteration -- gather, select, exchange, insert, net, push -- replayed as ONE hipGraph launch
	(world 1: the collectives short-circuit) gives the reference's traces bit for bit; the graph is kept from search to search."""
	t = golden["astar_trace"]
	_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
	agent = ShardedAStar(NoisyStubNet() if tag in ("e", "f") else StubNet(), float(t[f"{tag}_lambda"]), expansions, capacity=max_states + 16,
	                     use_hipgraph=True, poll=3)
	for again in range(2):
		solved = agent.search(t[f"{tag}_start"], None, max_states)
		assert agent.graph_error is None and agent.captures == 1                     # captured once, replayed by the second search
		assert agent.host_launches >= agent.iterations - 1                           # one launch per iteration (the first one ran eagerly, before the capture)
		n = int(t[f"{tag}_n"])
		assert solved == bool(t[f"{tag}_solved"]) and len(agent) == n
		states, G, parents, pact = agent.local_arrays()
		assert (states[1:] == t[f"{tag}_states"]).all() and (G[1:] == t[f"{tag}_G"]).all()
		assert (parents[2:] == t[f"{tag}_parents"]).all() and (pact[2:] == t[f"{tag}_parent_actions"]).all()
		assert list(agent.action_queue) == t[f"{tag}_action_queue"].tolist()


def _captured_collectives_world1(rank, port, out_path, tags, how):
	"""One rank, collectives FORCED and on the device (torch's nccl = RCCL, or rk_comm): the captured iteration contains the
	all-gather and the all-to-all themselves."""
	import json
	import torch.distributed as dist
	from librubiks_amd.solving.sharded import RcclTransport
	from tests.conftest import GOLDEN
	torch.cuda.set_device(0)
	t = dict(np.load(os.path.join(GOLDEN, "astar_trace.npz")))
	if how == "nccl":
		dist.init_process_group("nccl", init_method=f"file://{out_path}.rendezvous", rank=0, world_size=1, device_id=torch.device("cuda", 0))
	out = {}
	try:
		for tag in tags:
			_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
			kw = {"force_collectives": True} if how == "nccl" else {"transport": RcclTransport(RcclTransport.unique_id(), 0, 1)}
			agent = ShardedAStar(NoisyStubNet() if tag in ("e", "f") else StubNet(), float(t[f"{tag}_lambda"]), expansions, capacity=max_states + 16,
			                     use_hipgraph=True, poll=4, **kw)
			assert agent.tp.on_device and not agent.tp.shortcut
			solved = agent.search(t[f"{tag}_start"], None, max_states)
			states, G, parents, pact = agent.local_arrays()
			ok = (solved == bool(t[f"{tag}_solved"]) and len(agent) == int(t[f"{tag}_n"]) and (states[1:] == t[f"{tag}_states"]).all()
			      and (G[1:] == t[f"{tag}_G"]).all() and (parents[2:] == t[f"{tag}_parents"]).all() and (pact[2:] == t[f"{tag}_parent_actions"]).all()
			      and list(agent.action_queue) == t[f"{tag}_action_queue"].tolist())
			out[tag] = {"equal": bool(ok), "graph_error": agent.graph_error, "captures": agent.captures, "launches": agent.host_launches,
			            "iterations": agent.iterations, "collectives": agent.tp.collectives}
			del agent
	finally:
		if how == "nccl":
			dist.destroy_process_group()
	with open(out_path, "w") as f:
		json.dump(out, f)


@pytest.mark.parametrize("how", ["nccl", "rk_comm"])
def test_captured_iteration_with_device_collectives_world1(tmp_path, how):
	"""VERDICT r4 #2 "done": with the collectives forced at world 1 over RCCL (torch's nccl backend; the C ABI's rk_comm) the
	captured loop gives the reference traces a / b / d / e / f bit for bit, with at most one host launch per iteration.  A stack
	that cannot capture a collective must say so (graph_error) and still give the traces, eagerly."""
	import json
	out = str(tmp_path / "cap.json")
	mp.spawn(_captured_collectives_world1, args=(_free_port(), out, ["a", "b", "d", "e", "f"], how), nprocs=1, join=True)
	z = json.load(open(out))
	print(how, z)
	for tag, r in z.items():
		assert r["equal"], (tag, r)
		if r["graph_error"] is None:
			assert r["captures"] == 1 and r["launches"] >= r["iterations"] - 1


def _rank_row_shortfall(rank, world, port, out_dir):
	import torch.distributed as dist
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
	dist.init_process_group("gloo", rank=rank, world_size=world)
	try:
		torch.cuda.set_device(0)
		np.random.seed(19)
		start, _, _ = orc.scramble(7, True)
		agent = ShardedAStar(StubNet(), 0.1, 300, capacity=60_000, poll=3)
		agent.rows_override = 64                                             # far below a rank's share of 3 600 children: the shortfall happens at once
		solved = agent.search(start, None, 60_000)
		states, G, parents, pact = agent.local_arrays()
		np.savez(os.path.join(out_dir, f"sf_r{rank}.npz"), solved=solved, states=states[1:], G=G[1:], parents=parents[1:], pact=pact[1:],
		         prank=agent.local_parent_ranks()[1:], iters=agent.iterations, repeated=agent.repeated, full=agent.full_rows, rows=agent.net_rows_max,
		         queue=np.array(agent.action_queue, dtype=np.int64), start=start)
	finally:
		dist.destroy_process_group()


def test_row_shortfall_repeats_the_search_with_the_full_batch(tmp_path):
	"""The net runs on a fixed number of rows; an iteration that brings a rank more new states than that is detected ON THE DEVICE
	(rk_astar_shard_push_rows: error 3 in the all-gather), every rank stops together, and the driver repeats the search with
	12 N rows.  Forced here with 64 rows: both ranks repeat exactly once and end with the protocol oracle's shards."""
	from oracle.sharded_oracle import ShardedAStarOracle
	world = 2
	mp.spawn(_rank_row_shortfall, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
	z = [np.load(tmp_path / f"sf_r{r}.npz") for r in range(world)]
	assert all(int(x["repeated"]) == 1 and bool(x["full"]) and int(x["rows"]) == 3600 for x in z)
	o = ShardedAStarOracle(StubNet(), 0.1, 300, world)
	stop = o.search(z[0]["start"], 60_000)
	assert (stop == 1) == bool(z[0]["solved"]) and int(z[0]["iters"]) == o.iterations and z[0]["queue"].tolist() == list(o.action_queue)
	for r in range(world):
		os_, oG, op, orank, oa = o.arrays(r)
		assert (z[r]["states"] == os_).all() and (z[r]["G"] == oG).all() and (z[r]["parents"] == op).all()
		assert (z[r]["prank"] == orank).all() and (z[r]["pact"] == oa).all()


def test_device_clock_ends_a_search_on_time():
	"""The time limit is decided on the device (rank 0's constant-rate clock, started at the reset): a search that runs for
	T seconds without a limit stops with reason "time" shortly after a limit of T / 4, without the host writing anything per
	iteration (eager and captured alike)."""
	import time
	for use_graph in (False, True):
		agent = ShardedAStar(StubNet(), 0.05, 20, capacity=4_000_000, poll=8, use_hipgraph=use_graph)
		found = False
		for seed in range(5, 12):
			np.random.seed(seed)
			start, _, _ = orc.scramble(20, True)
			agent.search(start, None, 50_000)                                     # engine, buffers, capture
			torch.cuda.synchronize()
			t0 = time.perf_counter()
			agent.search(start, None, 4_000_000)
			T = time.perf_counter() - t0
			if agent.stop_reason != "budget" or T < 0.2:
				continue                                                          # solved, or too quick to cut short: another scramble
			found = True
			t0 = time.perf_counter()
			solved = agent.search(start, T / 4, 4_000_000)
			dt = time.perf_counter() - t0
			assert not solved and agent.stop_reason == "time" and T / 4 <= dt < 0.75 * T, (use_graph, agent.stop_reason, T, dt)
			assert agent.total_states < 4_000_000 - 12 * 20
			break
		assert found


@pytest.mark.parametrize("fused", [False, "folded"])
def test_captured_iteration_with_a_real_net_equals_the_eager_one(fused):
	"""The replayed graph holds the net's GEMMs as well as the engine's kernels: with a random-init fc_small (float32, and bfloat16 with
	the first layer fused + folded) the captured search visits the very states of the eager one -- same fixed batch shape, so the same
	net numbers -- and the second search on the kept graph does too."""
	from benchmarks.nets import FcSmall
	net = FcSmall(seed=4).cuda().eval()
	if fused:
		net = net.to(torch.bfloat16)
	np.random.seed(77)
	start, _, _ = orc.scramble(11, True)
	eager = ShardedAStar(net, 0.2, 60, capacity=40_000, fused_first_layer=fused, poll=2)
	graph = ShardedAStar(net, 0.2, 60, capacity=40_000, fused_first_layer=fused, poll=5, use_hipgraph=True)
	a = eager.search(start, None, 25_000)
	es, eG, ep, ea = eager.local_arrays()
	for again in range(2):
		b = graph.search(start, None, 25_000)
		assert graph.graph_error is None and graph.captures == 1
		assert a == b and len(eager) == len(graph) and eager.iterations == graph.iterations
		gs, gG, gp, ga = graph.local_arrays()
		assert (es == gs).all() and (eG == gG).all() and (ep == gp).all() and (ea == ga).all()
		if a:
			assert list(eager.action_queue) == list(graph.action_queue)
