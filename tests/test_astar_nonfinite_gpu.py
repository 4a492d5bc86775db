"""
A NaN among the net's values ends an A* search with engine error 4 -- the single engine (rk_astar_*), one search of a batch
(rk_astarb_*) and every rank of a sharded search (rk_astar_shard_*) -- and +-inf stay ordinary values (include/rubiks_hip.h,
"NON-FINITE VALUES").  tests/test_astar_nonfinite_cpu.py shows on the host why an order for NaN would not do.

Single engine: the driver of tests/test_astar_steps_gpu.py (engine and CPU model in lock-step, equal after every iteration) runs
astar_steps_model.NAN_GEOMETRIES up to the first iteration with enough new states, and there the test swaps ONE value:
  * for a NaN bit pattern -- either sign, quiet and signalling, float32 and bfloat16 -- at the first covered record, the last one,
    the first record of a later sort chunk and the last record of a chunk: the commit must report done = 1, error = 4, no win, and
    nothing pops again whatever pop count is asked for or budget is set;
  * for +inf and for -inf at the same place: not refused, engine and model stay equal (the infinity control);
  * for nothing, with a tail of NaN behind the n_new values: never read.
The same handle runs all of these, reset in between, and at the end a whole model run with the pool, the paths and the open queue
compared: a reset after a refusal leaves nothing behind.
Then the agents: AStar, AStarBatch (the other searches of the batch end bit for bit as without the poisoned one) and the sharded
engines as simulated ranks and as ShardedAStar.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import AStar, AStarBatch
from librubiks_amd.solving.sharded import ShardedAStar
from oracle import cube_oracle as orc
from oracle.search_oracle import AStarOracle, StubNet
from oracle.sharded_oracle import ShardedAStarOracle
from tests import astar_steps_model as sm
from tests.test_astar_steps_gpu import Engine
from tests.test_real_valued_oracle_cpu import variant
from tests.test_real_valued_search_gpu import _check_astar
from tests.test_sharded_gpu import _free_port, _simulate_ranks

pytestmark = pytest.mark.gpu

ERR_NONFINITE = 4
F32_NANS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF)      # +quiet (what the GPU's arithmetic produces), -quiet, signalling, all ones
BF16_NANS = (0x7FC0, 0xFFC0, 0x7F81)
POSITIONS = ("first", "last", "chunk_first", "chunk_last")


class Refused(Exception):
	"""ends astar_steps_model.run at the poisoned iteration (the model has no answer beyond it)"""


class NanEngine(Engine):
	"""tests/test_astar_steps_gpu.Engine that changes one value of the first iteration (after the root's) with more than `min_new` new states."""
	plan = None                # (kind, position, payload): "nan" (payload: bit pattern), "inf" (payload: the value), "beyond"
	min_new = 0
	hit = None                 # (iteration, n_new, j) of the changed value
	tail = 0                   # NaNs behind the values of the next upload

	def restart(self):
		g = self.g
		start = np.ascontiguousarray(sm.start_state(g))
		_ffi.check(self.lib.rk_astar_reset(self.h, start.ctypes.data, g.lambda_, None))
		_ffi.check(self.lib.rk_astar_set_budget(self.h, g.capacity, None))
		self.it, self.n_exp, self.hit, self.tail = 0, g.N, None, 0
		st = self.status()
		assert st[0] == 0 and st[6] == 0 and st[2] == 1, ("after the reset", st)

	def where_j(self, position, n_new):
		chunk = sm.sort_geometry(self.g.N)[1]
		return {"first": 0, "last": n_new - 1, "chunk_first": chunk, "chunk_last": chunk - 1}[position]

	def upload(self, values):
		if not self.tail:
			return super().upload(values)
		# the n_new values at the front of a larger tensor whose tail is NaN: the whole padded sort geometry and more
		nan = np.uint32(0x7FC00000).view(np.float32)
		return super().upload(np.concatenate([values, np.full(self.tail, nan, np.float32)]))

	def iteration(self, m, n_expand, values, pattern, target):
		n_new = len(values)
		if self.plan is None or self.hit is not None or self.it < 1 or n_new <= self.min_new:
			self.tail = 0
			return super().iteration(m, n_expand, values, pattern, target)
		kind, position, payload = self.plan
		j = self.where_j(position, n_new) if kind != "beyond" else n_new
		self.hit = (self.it, n_new, j)
		if kind == "inf":
			values = values.copy()
			values[j] = payload
			assert np.isinf(values).any()                                       # the commit in question holds an infinity
			return super().iteration(m, n_expand, values, pattern, target)
		if kind == "beyond":
			self.tail = sm.sort_geometry(self.g.N)[2] + 2048
			step = super().iteration(m, n_expand, values, pattern, target)
			self.tail = 0
			return step
		# a NaN: the model takes the clean values (the pool it builds is what the engine's pool must be), the engine the poisoned ones
		lib, h, at = self.lib, self.h, self.where(n_expand, n_new, pattern) + f", NaN {payload:#x} at j = {j} ({position})"
		_ffi.check(lib.rk_astar_expand(h, n_expand, self.info, None))
		step = m.step(n_expand, values)
		assert list(self.info) == [len(step.popped), step.n_new, step.won, step.solved, step.n_states] and not step.won, (at, list(self.info))
		bad = values.copy()
		bad.view(np.uint32)[j] = np.uint32(payload << 16 if self.bf16 else payload)
		assert np.isnan(bad[j]) and np.isnan(bad).sum() == 1
		with pytest.raises(ValueError):
			m.step(n_expand, bad)                                               # the model refuses it too
		dev = self.upload(bad)
		_ffi.check(lib.rk_astar_commit(h, dev.data_ptr(), None))
		st = self.status()
		assert st[0] == 1 and st[6] == ERR_NONFINITE and st[1] == 0 and st[7] == 0, (at, "done, error 4, no win, nothing to pop", st)
		assert st[2] == len(m) and lib.rk_astar_size(h) == len(m), (at, "the pool of the refused iteration stays as it was appended", st)
		assert self.next_pops() == [], at
		for n in (n_expand, 1 if n_expand != 1 else self.g.N, self.g.N):        # the pending list, and a selection made again (k_pop_select_only)
			_ffi.check(lib.rk_astar_expand(h, n, self.info, None))
			assert list(self.info)[:2] == [0, 0] and self.info[4] == len(m), (at, "expand after the refusal", n, list(self.info))
			assert lib.rk_astar_commit(h, None, None) == -4, (at, "nothing pending")
		_ffi.check(lib.rk_astar_set_budget(h, self.g.capacity, None))           # a budget does not revive it
		st = self.status()
		assert st[0] == 1 and st[6] == ERR_NONFINITE and st[7] == 0, (at, "after rk_astar_set_budget", st)
		raise Refused(at)


GEOMS = [(gi, bf16) for gi in range(len(sm.NAN_GEOMETRIES)) for bf16 in (False, True)]
SINGLE = [(gi, bf16, p) for gi, bf16 in GEOMS for p in (POSITIONS[:2] if gi == 0 else POSITIONS)]


def _engine(gi, bf16, chunked):
	g = sm.NAN_GEOMETRIES[gi]
	e = NanEngine(g, bf16, g.capacity)
	e.min_new = sm.sort_geometry(g.N)[1] if chunked else 1       # more than one chunk of new records, so that "last" lies in a later one
	return g, e


@pytest.mark.parametrize("gi,bf16,position", SINGLE, ids=[f"N{sm.NAN_GEOMETRIES[gi].N}-{'bf16' if b else 'f32'}-{p}" for gi, b, p in SINGLE])
def test_single_engine_refuses_nan_and_takes_infinities(gi, bf16, position):
	g, e = _engine(gi, bf16, gi > 0)
	K, chunk, Kpad, form = sm.sort_geometry(g.N)
	try:
		for bits in BF16_NANS if bf16 else F32_NANS:
			e.restart()
			e.plan = ("nan", position, bits)
			with pytest.raises(Refused):
				sm.run(g, bf16, engine=e)
			it, n_new, j = e.hit
			assert 0 <= j < n_new and (gi == 0 or n_new > chunk)
			print(f"N = {g.N} ({form}, chunk {chunk}) {'bf16' if bf16 else 'f32'}: NaN {bits:#x} refused at iteration {it}, n_new {n_new}, "
			      f"record {j} ({position}: chunk {j // chunk} of {-(-n_new // chunk)}, slot {j % chunk})")
		for inf in (np.inf, -np.inf):                                      # the infinity control: same place, not refused, equal to the model
			e.restart()
			e.plan = ("inf", position, np.float32(inf))
			m, log = sm.run(g, bf16, engine=e, iterations=it + 4)
			assert e.hit == (it, n_new, j) and len(log) == it + 4 and e.status()[6] == 0
			e.check_open(m, f"after the {inf} control")
	finally:
		e.close()


@pytest.mark.parametrize("gi,bf16", GEOMS, ids=[f"N{sm.NAN_GEOMETRIES[gi].N}-{'bf16' if b else 'f32'}" for gi, b in GEOMS])
def test_nan_beyond_the_new_states_is_not_read_and_a_reset_forgets_a_refusal(gi, bf16):
	g, e = _engine(gi, bf16, gi > 0)
	try:
		e.restart()
		e.plan = ("beyond", None, None)                                    # values[n_new ...] = NaN: never read, nothing stops
		m, log = sm.run(g, bf16, engine=e, iterations=12)
		it, n_new, j = e.hit
		assert j == n_new and len(log) == 12 and e.status()[6] == 0
		e.check_open(m, "after the NaN tail")
		e.restart()
		e.plan = ("nan", "last", (BF16_NANS if bf16 else F32_NANS)[0])
		with pytest.raises(Refused):
			sm.run(g, bf16, engine=e)
		e.restart()                                                        # ... and the same handle runs the whole schedule, as a fresh one
		e.plan = None
		m, log = sm.run(g, bf16, engine=e)
		assert len(log) >= 7
		e.check_end(m, g.seed)
		print(f"N = {g.N} {'bf16' if bf16 else 'f32'}: NaN tail behind {n_new} values at iteration {it} not read; after a refusal and a reset "
		      f"{len(log)} iterations, {len(m)} states equal to the model")
	finally:
		e.close()


# ---- the agents --------------------------------------------------------------------------------------------------------------
class Planted:
	"""`net` with the value of ONE state replaced (by its one-hot row, wherever it turns up in a batch); NumPy and torch alike."""
	def __init__(self, net, state, value=float("nan")):
		self.net, self.value, self.on = net, value, True
		self.row = orc.as_oh(np.asarray(state, np.int8)[None])[0].astype(np.float32)
		self._dev = None

	def eval(self):
		return self

	def __call__(self, x, policy=True, value=True):
		out = self.net(x, policy=policy, value=value)
		if value and self.on:
			v = out[-1] if isinstance(out, (list, tuple)) else out
			if isinstance(x, torch.Tensor):
				if self._dev is None:
					self._dev = torch.from_numpy(self.row).to(x.device)
				v[(x.float() == self._dev).all(dim=1)] = self.value
			else:
				v[(np.asarray(x, np.float32) == self.row).all(axis=1)] = self.value
		return out


@pytest.mark.parametrize("exact", [False, True], ids=["padded", "exact"])
def test_astar_agent_raises_and_searches_again(exact):
	seed, depth, lam, n, budget = 102, 7, 0.3, 17, 20_000
	np.random.seed(seed)
	start, _, _ = orc.scramble(depth, True)
	clean = variant("plain")
	ref = AStarOracle(clean, lam, n)
	ref_solved = ref.search(start, budget)
	assert len(ref) > 2_000
	net = Planted(clean, ref.states[len(ref) // 2])
	agent = AStar(net, lam, n, exact_batch=exact)
	with pytest.raises(_ffi.RubiksHipError, match="NaN among the net's values"):
		agent.search(start, None, budget)
	assert 1 < len(agent) < len(ref)                                       # it stopped where the value was read, not at the budget
	net.on = False
	solved = agent.search(start, None, budget)
	_check_astar(agent, ref, ref_solved, solved, "the same agent after the refusal")
	fresh = AStar(clean, lam, n, exact_batch=exact)
	assert fresh.search(start, None, budget) == solved and len(fresh) == len(agent)
	assert (fresh.states == agent.states).all() and (fresh.G == agent.G).all() and (fresh.parents == agent.parents).all()
	assert fresh.open_queue == agent.open_queue


S, BN, BLAM = 4, 10, 0.3


def _batch_inputs():
	starts = []
	for i in range(S):
		np.random.seed(600 + i)
		starts.append(orc.scramble(13 + i, True)[0])
	return np.ascontiguousarray(np.array(starts, np.int8)), np.array([2500, 3000, 3500, 4000], np.int64)


class _Batch:
	def __init__(self, starts, budgets):
		self.lib, self.h = _ffi.lib(), C.c_void_p()
		_ffi.check(self.lib.rk_astarb_create(C.byref(self.h), S, int(budgets.max()), BN))
		_ffi.check(self.lib.rk_astarb_reset(self.h, starts.ctypes.data, budgets.ctypes.data, BLAM, None))
		self.oh = torch.zeros((S * 12 * BN, 480), device="cuda")

	def status(self):
		st = np.zeros((S, 7), np.int64)
		_ffi.check(self.lib.rk_astarb_status(self.h, st.ctypes.data, None))
		return st

	def expand(self, net):
		_ffi.check(self.lib.rk_astarb_step_expand(self.h, self.oh.data_ptr(), _ffi.OH_F32, None))
		return net(self.oh, policy=False, value=True).reshape(-1).float().contiguous()

	def commit(self, values):
		_ffi.check(self.lib.rk_astarb_step_commit(self.h, values.data_ptr(), None))
		torch.cuda.synchronize()

	def pool(self, s, n):
		states, G, par, act = np.zeros((n, 20), np.int8), np.zeros(n), np.zeros(n, np.int64), np.zeros(n, np.int64)
		_ffi.check(self.lib.rk_astarb_export(self.h, s, 1, n, states.ctypes.data, G.ctypes.data, par.ctypes.data, act.ctypes.data, None))
		return states.tobytes(), G.tobytes(), par.tobytes(), act.tobytes()

	def close(self):
		self.lib.rk_astarb_destroy(self.h)


@pytest.mark.parametrize("bits", [0x7FC00000, 0xFFC00000])
def test_batch_poisoned_search_ends_alone(bits):
	"""Four searches through the C API, twice: in one batch search 1 gets a NaN at its LAST covered value in iteration 3.  That search
	reports done / error 4 with that commit; the other three have, after every later iteration until they end, the status row and the
	pool (states, G, parents, actions) of the clean batch, bit for bit.  (The batch has no export of a search's open queue; its
	length is a status word, and every later pop, new state and G follows from its content.)"""
	starts, budgets = _batch_inputs()
	net, poisoned, others = variant("plain"), 1, [0, 2, 3]
	a, b = _Batch(starts, budgets), _Batch(starts, budgets)
	try:
		for it in range(200):
			before = a.status()
			va, vb = a.expand(net), b.expand(net)
			if it == 3:
				n_new = int(a.status()[poisoned, 2] - before[poisoned, 2])
				assert 0 < n_new <= 12 * BN and not before[:, 0].any()           # every search is still running when one is poisoned
				host = va.cpu().numpy()                                              # (bits set on the host: the payload arrives as it is)
				host.view(np.uint32)[poisoned * 12 * BN + n_new - 1] = bits
				va = torch.from_numpy(host).cuda()
			a.commit(va)
			b.commit(vb)
			sa, sb = a.status(), b.status()
			if it == 3:
				at_refusal = int(sa[poisoned, 2])
			if it >= 3:
				assert sa[poisoned, 0] == 1 and sa[poisoned, 6] == ERR_NONFINITE and sa[poisoned, 1] == 0, (it, sa[poisoned])
				assert sa[poisoned, 3] == 4 and sa[poisoned, 2] == at_refusal, (it, "the refused search neither pops nor grows", sa[poisoned])
			assert (sa[others] == sb[others]).all() and not sb[:, 6].any(), (it, sa, sb)
			if it >= 3:
				for s in others:
					assert a.pool(s, int(sa[s, 2])) == b.pool(s, int(sb[s, 2])), (it, s)
			if sb[others, 0].all():
				break
		assert it > 10 and sb[others, 0].all(), (it, sb)
		# the handle after a reset: the clean batch's first iterations again
		_ffi.check(a.lib.rk_astarb_reset(a.h, starts.ctypes.data, budgets.ctypes.data, BLAM, None))
		_ffi.check(b.lib.rk_astarb_reset(b.h, starts.ctypes.data, budgets.ctypes.data, BLAM, None))
		for it in range(8):
			a.commit(a.expand(net))
			b.commit(b.expand(net))
			sa, sb = a.status(), b.status()
			assert (sa == sb).all() and not sa[:, 6].any(), (it, sa, sb)
		assert all(a.pool(s, int(sa[s, 2])) == b.pool(s, int(sb[s, 2])) for s in range(S))
	finally:
		a.close()
		b.close()


def test_batch_agent_names_the_search():
	starts, budgets = _batch_inputs()
	clean = variant("plain")
	refs = [AStarOracle(clean, BLAM, BN) for _ in range(S)]
	for i, r in enumerate(refs):
		r.search(starts[i], int(budgets[i]))
	mine = next(k for k in range(len(refs[2]) // 2, len(refs[2])) if all(refs[2].states[k].tobytes() not in refs[i].index for i in (0, 1, 3)))
	agent = AStarBatch(Planted(clean, refs[2].states[mine]), BLAM, BN, S, capacity=int(budgets.max()))
	with pytest.raises(_ffi.RubiksHipError, match=r"searches \[2\] ended with 4: NaN among the net's values"):
		agent.search(starts, max_states=budgets, poll=2)
	agent.net.on = False
	solved = agent.search(starts, max_states=budgets, poll=2)
	for i, r in enumerate(refs):
		states, G, parents, pact = agent.arrays_of(i)
		rs, rG, rp, ra = r.arrays()
		assert bool(solved[i]) == bool(r.action_queue) and (states[1:] == rs).all() and (G[1:] == rG).all() and (parents[2:] == rp).all(), i


# ---- sharded -----------------------------------------------------------------------------------------------------------------
class _Recorder(StubNet):
	"""StubNet that keeps the states of every batch (the CPU oracle calls it once per rank with new states, in rank order)"""
	def __init__(self):
		super().__init__()
		self.batches = []

	def __call__(self, x, policy=True, value=True):
		self.batches.append(np.array(x))
		return super().__call__(x, policy=policy, value=value)


def _planted_in_iteration(world, start, lam, N, budget, iteration):
	"""-> (rank, one-hot row) of the LAST new state of iteration `iteration` on the rank with most of them, from a clean oracle run"""
	rec = _Recorder()
	o = ShardedAStarOracle(rec, lam, N, world)
	o.search(start, budget)
	assert o.iterations > iteration + 3
	calls = [(it, r) for it, row in enumerate(o.new_counts) for r, c in enumerate(row) if c]
	assert len(calls) == len(rec.batches)
	rank = int(np.argmax(o.new_counts[iteration]))
	batch = rec.batches[calls.index((iteration, rank))]
	assert len(batch) == o.new_counts[iteration][rank] > 1
	return rank, batch[-1]


class _PlantedRow(Planted):
	def __init__(self, net, row, value):
		self.net, self.value, self.on, self.row, self._dev = net, value, True, np.asarray(row, np.float32), None


SHARDED = [(2, 4), (3, 4), (2, 64), (3, 64)]


@pytest.mark.parametrize("world,N", SHARDED)
def test_sharded_ranks_stop_together_in_the_iteration_of_the_nan(world, N):
	np.random.seed(19)
	start, _, _ = orc.scramble(9, True)
	lam, budget = 0.5, 30_000
	rank, row = _planted_in_iteration(world, start, lam, N, budget, 2)
	lib, seen = _ffi.lib(), []

	def inspect(r, h, n_new):
		dec, status = (C.c_longlong * 8)(), (C.c_longlong * 8)()
		_ffi.check(lib.rk_astar_shard_decision(h, dec, None))
		_ffi.check(lib.rk_astar_status(h, status, None))
		seen.append((r, list(dec), int(status[6]), int(lib.rk_astar_size(h)), n_new))

	stop, queue, shards, total, iters = _simulate_ranks(world, start, lam, N, budget, capacity=budget, net=_PlantedRow(StubNet(), row, float("nan")), inspect=inspect)
	assert stop == 6 and queue is None and iters == 3, (stop, iters)       # iterations 0, 1, 2 ran; the decision behind the poisoned push stops
	assert len(seen) == world
	for r, dec, err, size, n_new in seen:
		assert dec[0] == 6 and dec[7] == ERR_NONFINITE and dec[4] == 0 and dec[5] == 3, (r, dec)    # D_STOP, D_ERROR, D_NPOP, D_ITERS
		assert err == (ERR_NONFINITE if r == rank else 0), (r, err)
		assert size == dec[6] == len(shards[r][0]), (r, "no pool grew after the decision", size, dec[6])
	assert sum(dec[6] for _, dec, _, _, _ in seen) == seen[0][1][3] == total
	# the infinity control: the same state worth +inf (a cost of -inf, popped first) is an ordinary search, equal to the oracle throughout
	o = ShardedAStarOracle(_PlantedRow(StubNet(), row, float("inf")), lam, N, world)
	o.search(start, budget)
	assert any(np.isneginf(c).any() for per_rank in o.cand_costs for c in per_rank)
	_simulate_ranks(world, start, lam, N, budget, capacity=budget, oracle=o, net=_PlantedRow(StubNet(), row, float("inf")))


def test_short_net_batch_with_a_nan_beyond_its_rows_still_reports_the_rows():
	"""tests/test_sharded_gpu.test_short_net_batch_reads_no_value_beyond_its_rows with a NaN tail: the values behind `rows` are not read,
	so the error is ERR_NET_ROWS (3) as before, never 4 -- and again on a second run of the same engines' worth."""
	lib, world, N, rows = _ffi.lib(), 2, 300, 64
	np.random.seed(19)
	start, _, _ = orc.scramble(9, True)
	for attempt in range(2):
		seen = []

		def inspect(r, h, n_new):
			status = (C.c_longlong * 8)()
			_ffi.check(lib.rk_astar_status(h, status, None))
			n_open = int(lib.rk_astar_open_size(h))
			costs = np.zeros(n_open + 1)
			got = lib.rk_astar_export_open(h, costs.ctypes.data, None, n_open + 1, None)
			seen.append((r, n_new, int(status[6]), costs[:got].copy()))

		stop, queue, shards, total, iters = _simulate_ranks(world, start, 0.5, N, 60_000, capacity=60_000, short_rows=rows, inspect=inspect,
		                                                    short_tail=float("nan"))
		assert stop == 6 and 2 <= iters <= 4 and any(n_new > rows for _, n_new, _, _ in seen)
		for r, n_new, err, costs in seen:
			assert err == (3 if n_new > rows else 0), (attempt, r, n_new, err)
			assert len(costs) and np.isfinite(costs).all(), (attempt, r)


def test_sharded_agent_raises_world1():
	np.random.seed(19)
	start, _, _ = orc.scramble(9, True)
	_, row = _planted_in_iteration(1, start, 0.5, 4, 30_000, 2)
	net = _PlantedRow(StubNet(), row, float("nan"))
	agent = ShardedAStar(net, 0.5, 4, capacity=30_000)
	with pytest.raises(_ffi.RubiksHipError, match="4: NaN among the net's values"):
		agent.search(start, None, 30_000)
	assert agent.stop_reason == "engine error" and agent.iterations == 3
	net.on = False
	o = ShardedAStarOracle(StubNet(), 0.5, 4, 1)
	assert agent.search(start, None, 30_000) == (o.search(start, 30_000) == 1) and list(agent.action_queue) == list(o.action_queue)


def _rank_nan(rank, world, port, out_dir, row):
	import torch.distributed as dist
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
	dist.init_process_group("gloo", rank=rank, world_size=world)
	try:
		torch.cuda.set_device(0)
		np.random.seed(19)
		start, _, _ = orc.scramble(9, True)
		agent = ShardedAStar(_PlantedRow(StubNet(), row, float("nan")), 0.5, 4, capacity=30_000)
		try:
			agent.search(start, None, 30_000)
			text = ""
		except _ffi.RubiksHipError as e:
			text = str(e)
		np.savez(os.path.join(out_dir, f"nan_r{rank}.npz"), text=text, iters=agent.iterations, reason=agent.stop_reason)
	finally:
		dist.destroy_process_group()


def test_sharded_agent_raises_on_every_rank(tmp_path):
	world = 2
	np.random.seed(19)
	start, _, _ = orc.scramble(9, True)
	rank, row = _planted_in_iteration(world, start, 0.5, 4, 30_000, 2)
	mp.spawn(_rank_nan, args=(world, _free_port(), str(tmp_path), row), nprocs=world, join=True)
	z = [np.load(tmp_path / f"nan_r{r}.npz") for r in range(world)]
	for r in range(world):
		assert f"rank {r}:" in str(z[r]["text"]) and "4: NaN among the net's values" in str(z[r]["text"]), (r, str(z[r]["text"]))
		assert int(z[r]["iters"]) == 3 and str(z[r]["reason"]) == "engine error"
