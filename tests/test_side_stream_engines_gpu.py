"""
Search engines on a torch side stream behind a gate (tests/side_stream.py).

  * pattern A for the frontier engines -- DeviceBFS, DeviceBiBFS, DeviceBallSearch, DeviceSymBallSearch -- on one 7-move scramble, driven
    entry by entry: reset, run, a grow, run again, status, export and path, each enqueue-only call behind a gate that is still closed
    when the last of them returns, each synchronising call (reset, grow) behind a gate that is closed when it starts.  The engine holds a
    decoy search of another scramble when the gated reset arrives.
  * pattern B, then A, for DeviceBallSearchBatch's and DeviceSymBallSearchBatch's engines (5 slots, then a second reset of two slots
    while the others rest), for rk_beamb_create and for rk_astar_create, each followed by its agent's search on a side stream: the
    null stream is gated, `create` has no stream argument, and its own null-stream initialisation must be COMPLETE when it returns --
    otherwise the test stops and never runs the engine.
  * DeviceEGVM, GreedyBatch, DeviceBeamSearch (with and without the radius-3 ball), DeviceBeamSearchBatch and
    DeviceSymBallSearchBatch(deepen=4) through their agents inside torch.cuda.stream(s), the gate before the search, against the models
    and traces of the engines' own GPU tests.
  * eager AStar, AStarBatch and MCTSBatch behind a GatedNet that re-arms a 2 ms gate at every forward, against the reference's traces and the oracle.
  * pattern C: two OhLinear handles on two side streams; a beam search and a symmetry-ball search on one ball on two streams.

Everything is compared bit for bit with the same calls on the default stream by a second engine, whose behaviour the engines' own GPU
tests pin against the models.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.oh_linear import BACKWARD_MIN_ROWS, OhLinear
from librubiks_amd.solving import _engine as eng
from librubiks_amd.solving.agents import (DeviceBallSearch, DeviceBFS, DeviceBiBFS, DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch)
from tests import oh_linear_ref as R
from tests import side_stream as S

pytestmark = pytest.mark.gpu

RADIUS = 4
CAP_GROWN = 131072
BUDGET = 30_000                        # the plain BFS stops at its budget; the others meet long before


@functools.lru_cache(maxsize=None)
def _ball(kind):
	ball = (DeviceGoalBall if kind == "goal" else DeviceSymBall)(RADIUS).build()
	torch.cuda.synchronize()
	return ball


def _root(seed) -> np.ndarray:
	"""a scramble of 7 moves that lies 7 moves from solved (so every engine has work to do and the ball searches meet at depth 3)"""
	for k in range(50):                # further than radius + 1 = 5 moves, and odd like the scramble: 7
		r = S.scrambles(1, 7, 7000 + 50 * seed + k)
		if int(_ball("sym").child_depths(r)[0][0]) == -1:
			return np.ascontiguousarray(r[0])
	raise AssertionError("no deep scramble found")


# name -> (agent, ball, pops, first capacity): two iterations fit the first pool, the search needs more nodes than it holds
ENGINES = {
	"bfs": (DeviceBFS, None, 256, 8192),                     # stops at its budget
	"bibfs": (DeviceBiBFS, None, 64, 2048),                  # three levels of both sides are 2 390 nodes
	"ballsearch": (DeviceBallSearch, "goal", 16, 512),       # meets at depth 3: 1 195 nodes
	"symballsearch": (DeviceSymBallSearch, "sym", 16, 512),
}


def _drive(name, root, decoy_root=None, s=None):
	"""reset, two iterations, a grow, the rest, status, export and path; on the default stream, or (`s`) behind gates on a side stream
	with the engine holding a search of `decoy_root`.  -> everything the host read"""
	cls, ball, pops, CAP = ENGINES[name]
	K = 12 * pops
	agent = cls(_ball(ball), pops=pops, capacity=CAP) if ball else cls(pops=pops, capacity=CAP)
	h = agent._engine(CAP)
	e = agent._entry
	words = agent._status_words
	first = (CAP - agent._first_nodes) // K
	assert first >= 1

	def gate(blocking):
		if s is None:
			return None
		ev = S.gate(s)
		if blocking:
			S.held(ev)
		return ev

	def held(ev):
		if ev is not None:
			S.held(ev)

	def go():
		gate(True)
		_ffi.check(e("reset")(h, root.ctypes.data, BUDGET, _ffi.stream_ptr()))
		ev = gate(False)
		_ffi.check(e("run")(h, first, _ffi.stream_ptr()))
		held(ev)
		st1 = S.status_words(e("status"), h, words)
		gate(True)
		_ffi.check(e("grow")(h, CAP_GROWN, _ffi.stream_ptr()))
		ev = gate(False)
		_ffi.check(e("run")(h, min(32, (CAP_GROWN - st1[2]) // K), _ffi.stream_ptr()))
		held(ev)
		st2 = S.status_words(e("status"), h, words)
		cols = eng.export_frontier(e("export"), (h,), st2[2], agent._first_nodes, name == "bibfs")
		path = list(eng.read_path(e("path"), h)) if st2[1] else None
		return st1, st2, cols, path

	if s is None:
		out = go()
	else:
		_ffi.check(e("reset")(h, decoy_root.ctypes.data, BUDGET, _ffi.stream_ptr()))
		_ffi.check(e("run")(h, first, _ffi.stream_ptr()))
		torch.cuda.synchronize()
		s.wait_stream(torch.cuda.default_stream())
		with torch.cuda.stream(s):
			out = go()
			s.synchronize()
	agent._free()
	return out


@pytest.mark.parametrize("name", list(ENGINES))
def test_frontier_engine_behind_gates(name):
	root, decoy = _root(0), _root(1)
	assert not (root == decoy).all()
	want = _drive(name, root)
	got = _drive(name, root, decoy, S.side_stream())
	st1, st2, cols, path = want
	assert st1[6] == 0 and st2[6] == 0 and not st1[0] and st2[0], (st1, st2)      # no error; not done in the first pool; done in the grown one
	assert st2[2] > ENGINES[name][3]                                                     # which the search needed
	if name != "bfs":
		assert st2[1] and len(path) == 7
	assert got[0] == st1 and got[1] == st2 and got[3] == path
	for a, b in zip(got[2], cols):
		assert a.dtype == b.dtype and (a == b).all()
	other = _drive(name, decoy)
	assert not (other[2][0][1] == cols[0][1]).all()                              # the decoy search is another search


# ---------------------------------------------------------------------------------------------------------------- pattern B
def _null_stream_gated_create(create, *args):
	"""Pattern B, steps 1 to 3: the gate on the NULL stream, `create`, and the gate must be complete when create returns -- its own
	null-stream initialisation was finished, not merely queued.  -> the handle; on failure nothing of the engine is ever run."""
	S.sleep_rate()
	torch.cuda.synchronize()
	ev = S.gate(torch.cuda.default_stream())
	h = C.c_void_p()
	_ffi.check(getattr(_ffi.lib(), create)(C.byref(h), *args))
	done = ev.query()
	torch.cuda.synchronize()
	if not done:                                      # (never run, only freed, now that the null stream has drained)
		getattr(_ffi.lib(), create.replace("_create", "_destroy"))(h)
	assert done, f"{create} returned while the null stream was still busy: its initialisation was only queued"
	return h


def _adopt(agent, h, destroy):
	"""the agent owns the engine that pattern B made (what Owner._create would have left)"""
	agent._h, agent._destroy = h, destroy


BATCH = {"bsearchb": ("rk_bsearchb", "goal"), "ssearchb": ("rk_ssearchb", "sym")}
SLOTS = 5
SLOT_CAP = 16384


def _batch_drive(prefix, h, roots, decoys, s=None):
	"""all five slots reset and run to the end, then slots 1 and 3 reset again while the others rest; -> what the host read"""
	lib = _ffi.lib()
	e = lambda name: getattr(lib, f"{prefix}_{name}")
	budgets = np.full(SLOTS, BUDGET, np.int64)

	def gate(blocking):
		if s is None:
			return None
		ev = S.gate(s)
		if blocking:
			S.held(ev)
		return ev

	def reset(slots, rows):
		slots = np.asarray(slots, np.int32)
		rows = np.ascontiguousarray(rows)
		gate(True)
		_ffi.check(e("reset")(h, len(slots), slots.ctypes.data, rows.ctypes.data, budgets.ctypes.data, _ffi.stream_ptr()))

	def run():
		ev = gate(False)
		_ffi.check(e("run")(h, 12, _ffi.stream_ptr()))
		if ev is not None:
			S.held(ev)
		st = (C.c_longlong * (SLOTS * 10))()
		_ffi.check(e("status")(h, st, _ffi.stream_ptr()))
		paths = np.full((SLOTS, 1 + 16), -7, np.int32)
		_ffi.check(e("paths")(h, paths.ctypes.data, 16, _ffi.stream_ptr()))
		for row in paths:                             # (behind a queue's last action the row holds whatever the engine's buffer held)
			row[1 + max(int(row[0]), 0):] = -7
		return np.array(st, np.int64).reshape(SLOTS, 10), paths

	def go():
		reset(range(SLOTS), roots)
		st1, p1 = run()
		reset([3, 1], decoys[:2])
		st2, p2 = run()
		n = int(st2[2, 2])
		cols = eng.export_frontier(e("export"), (h, 2), n)
		return st1, p1, st2, p2, cols

	if s is None:
		return go()
	sl = np.arange(SLOTS, dtype=np.int32)                 # a decoy search of every slot on the default stream: the gated resets find stale pools
	rows = np.ascontiguousarray(decoys)
	_ffi.check(e("reset")(h, SLOTS, sl.ctypes.data, rows.ctypes.data, budgets.ctypes.data, _ffi.stream_ptr()))
	_ffi.check(e("run")(h, 3, _ffi.stream_ptr()))
	torch.cuda.synchronize()
	s.wait_stream(torch.cuda.default_stream())
	with torch.cuda.stream(s):
		out = go()
		s.synchronize()
	return out


@pytest.mark.parametrize("name", list(BATCH))
def test_batch_ball_search_create_then_side_stream(name):
	prefix, kind = BATCH[name]
	ball = _ball(kind)
	roots = np.stack([_root(10 + i) for i in range(SLOTS)])
	decoys = np.stack([_root(20 + i) for i in range(SLOTS)])
	lib = _ffi.lib()
	ref = C.c_void_p()
	_ffi.check(getattr(lib, f"{prefix}_create")(C.byref(ref), ball._h, SLOTS, SLOT_CAP, 64))
	h = _null_stream_gated_create(f"{prefix}_create", ball._h, SLOTS, SLOT_CAP, 64)       # pattern B: only a complete create is ever run
	try:
		want = _batch_drive(prefix, ref, roots, decoys)
		got = _batch_drive(prefix, h, roots, decoys, S.side_stream())
		st1, p1, st2, p2, cols = want
		assert (st1[:, 0] == 1).all() and (st1[:, 1] == 1).all() and (st1[:, 6] == 0).all(), st1      # all met, no error
		assert (p1[:, 0] == 7).all() and (p2[:, 0] == 7).all()
		assert (st2[[0, 2, 4]] == st1[[0, 2, 4]]).all() and (p2[[0, 2, 4]] == p1[[0, 2, 4]]).all()     # the resting slots stayed
		assert not (p2[[1, 3]] == p1[[1, 3]]).all()
		for a, b in zip(got[:4], want[:4]):
			assert (a == b).all()
		for a, b in zip(got[4], cols):
			assert (a == b).all()
	finally:
		torch.cuda.synchronize()
		getattr(lib, f"{prefix}_destroy")(h)
		getattr(lib, f"{prefix}_destroy")(ref)


# ---------------------------------------------------------------------------------------------------------------- pattern C
def test_two_first_layer_handles_on_two_streams():
	"""a forward of one handle and a backward of another, interleaved by one host thread on two side streams, each behind its own gate:
	each equals its solo run on the default stream"""
	H, n = 192, 2 * BACKWARD_MIN_ROWS + 1
	torch.manual_seed(5)
	lin_a = torch.nn.Linear(480, H).cuda().requires_grad_(False)
	lin_b = torch.nn.Linear(480, H).cuda().requires_grad_(False)
	fwd, bwd = OhLinear(lin_a, "gather"), OhLinear(lin_b, "gather")
	xa = torch.from_numpy(R.random_states(n, 1)).cuda()
	xb = torch.from_numpy(R.random_states(n, 2)).cuda()
	dy = torch.randint(-8, 9, (n, H), generator=torch.Generator().manual_seed(3)).float().cuda()

	def backward(states, grad, dw, db):
		_ffi.check(_ffi.lib().rk_ohl_backward(bwd._h, states.data_ptr(), grad.data_ptr(), n, dw.data_ptr(), db.data_ptr(), _ffi.stream_ptr()))
	want_y = fwd(xa)
	want_w, want_b = torch.empty((H, 480), device="cuda"), torch.empty(H, device="cuda")
	backward(xb, dy, want_w, want_b)
	abuf, bbuf = xb.clone(), xa.clone()                                          # each starts as the other's states
	y, dw, db = S.sentinel((n, H), torch.float32), S.sentinel((H, 480), torch.float32), S.sentinel((H,), torch.float32)
	torch.cuda.synchronize()
	s1, s2 = S.side_stream(), S.side_stream()
	assert s1.cuda_stream != s2.cuda_stream
	ev1, ev2 = S.gate(s1), S.gate(s2)
	with torch.cuda.stream(s1):
		abuf.copy_(xa, non_blocking=True)
	with torch.cuda.stream(s2):
		bbuf.copy_(xb, non_blocking=True)
	with torch.cuda.stream(s1):
		fwd(abuf, out=y)
	with torch.cuda.stream(s2):
		backward(bbuf, dy, dw, db)
	S.held(ev1)
	S.held(ev2)
	torch.cuda.synchronize()
	assert S.same_bits(y, want_y) and S.same_bits(dw, want_w) and S.same_bits(db, want_b)


# ------------------------------------------------------------------------------------- agents inside torch.cuda.stream(s)
def _on_side_stream(search, warm, first_blocking):
	"""`warm()` (a decoy search: captures the kept steps, fills the side stream's allocator, leaves a stale search in the engine), then
	the gate, then `search()`, all inside torch.cuda.stream(s).  The engines' resets synchronise: the gate is closed when the first
	of `first_blocking` starts.  -> what search returned"""
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		if warm is not None:
			warm()
			s.synchronize()
		ev = S.gate(s)
		with S.watch(first_blocking, lambda: ev, before=True, once=True) as notes:
			out = search()
		s.synchronize()
	S.all_held(notes)
	return out


def _entries_of(*prefixes) -> list:
	"""every stream-taking entry of an engine: the gate is closed when the search makes its first call of any of them"""
	return [n for n, (_, args) in _ffi.SIGNATURES.items() if n.startswith(prefixes) and not n.endswith(("_create", "_destroy")) and len(args) > 1]


def test_device_egvm_agent():
	from librubiks_amd.solving.agents import DeviceEGVM
	from tests import test_egvm_device_gpu as E
	t = E._load("egvm_trace.npz")
	tag = "late_solve"
	seed, max_states, net, eps, workers, depth = E._case(t, tag)
	agent = DeviceEGVM(net, eps, workers, depth, poll=4)

	def search():
		np.random.seed(seed)
		return agent.search(t[f"{tag}_start"], time_limit=None, max_states=max_states)
	solved = _on_side_stream(search, lambda: agent.search(t["noisy_budget_start"], time_limit=None, max_states=max_states), ["rk_egvm_reset"])
	E._check(t, tag, agent, solved)
	assert agent.rounds == int(t[f"{tag}_rounds"])


def test_greedy_batch_agent():
	from librubiks_amd.solving.agents import GreedyBatch
	from tests import test_greedy_batch_gpu as G
	agent = GreedyBatch(G.net_of("noisy"), "value", 5, poll=3)
	want = G.wanted("value", "noisy", 200)[0][:5]
	got = _on_side_stream(lambda: G.play(agent, G.STARTS[:5], 200), lambda: agent.search(G.STARTS[5:10], time_limit=None, max_states=200),
	                      ["rk_greedy_reset"])
	assert got == want


@pytest.mark.parametrize("with_ball", [False, True])
def test_device_beam_search_agent(with_ball):
	from librubiks_amd.solving.agents import DeviceBeamSearch
	from tests import beam_model as bm
	from tests import test_beam_gpu as Bt
	if with_ball:
		case = ("noisy", 22, 572, 6)
		assert case in bm.BALL_CASES
		ref, start = bm.ball_reference(case), bm.start_of(572, 6)
		agent = DeviceBeamSearch(Bt._device_net("noisy"), 22, 12, ball=DeviceSymBall(bm.BALL_RADIUS).build())
	else:
		case = bm.Case("noisy", 22, True, 12, 561, 4)
		assert case in bm.SOLVING_CASES
		ref, start = bm.reference(case), bm.start_of(561, 4)
		agent = Bt._agent(case)
	solved = _on_side_stream(lambda: agent.search(start, None, None), lambda: agent.search(bm.start_of(999, 7), None, None), ["rk_beam_reset"])
	Bt._same(agent, solved, ref, case)


def test_beam_batch_create_then_agent_on_side_stream():
	"""pattern B for rk_beamb_create, then the agent on a side stream: 7 starts through 5 slots, so two slots are reset again while
	the others rest"""
	from librubiks_amd.solving.agents import DeviceBeamSearchBatch
	from tests import beam_batch_groups as gg
	from tests import test_beam_batch_gpu as Bb
	width, depth, slots, n = 22, 12, 5, 7
	b = DeviceBeamSearchBatch(Bb._device_net("noisy"), width, searches=slots, max_depth=depth)
	h = _null_stream_gated_create("rk_beamb_create", None, slots, width, depth, 1)
	_adopt(b, h, "rk_beamb_destroy")
	starts = gg.starts_of(n)
	refs = [gg.alone("noisy", width, depth, True, k) for k in range(n)]
	solved = _on_side_stream(lambda: b.search(starts, keep_arrays=True), lambda: b.search(gg.starts_of(slots, first=10)), _entries_of("rk_beamb_"))
	assert b._h is h                                  # the searches ran the engine that pattern B made
	Bb._all_same(b, solved, refs, starts, "side stream")


def test_symsearch_batch_deepen_agent():
	"""DeviceSymBallSearchBatch(deepen=4): 9 states through 5 slots (refills while the others rest, full pools that go on by probes)"""
	from tests import test_symsearch_batch_deepen_gpu as D
	states = D._states().copy()
	ref = D._batch(5, 16)
	want = D.Run(ref, ref.search(states.copy()), len(states))
	b = D._batch(5, 16)
	got_solved = _on_side_stream(lambda: b.search(states.copy()), lambda: b.search(states[::-1].copy()), _entries_of("rk_ssearchb_", "rk_sdeepenb_"))
	got = D.Run(b, got_solved, len(states))
	assert (got.solved == want.solved).all() and (got.status == want.status).all() and (got.lengths == want.lengths).all()
	assert got.queues == want.queues and (got.deepened == want.deepened).all() and want.deepened.any()


# ------------------------------------------------------------------------------------- eager searches behind a GatedNet
def _eager(search, net, commits, warm=None):
	"""an eager search inside torch.cuda.stream(s) (it starts with host reads, so a gate before it would only be waited for): the
	net's own short gate before every forward, still closed when the first `commits` entry after that forward has been enqueued"""
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		net.net(torch.zeros((24, 480), device="cuda"), policy=False)      # the stub's own first call copies its table to the device and waits
		s.synchronize()
		if warm is not None:                          # a decoy search: loads every kernel of the step and fills the stream's allocator
			warm()
			s.synchronize()
			net.calls = 0
		with S.watch(commits, net.fresh_gate()) as notes:
			out = search()
		s.synchronize()
	S.all_held(notes)
	assert len(notes) >= net.calls - 1 > 0                # (a forward whose commit the search never issued has no note)
	return out


def test_eager_astar_create_then_search(golden):
	"""pattern B for rk_astar_create (it clears three arrays of look-back words through the null stream; a scan on another stream
	would spin on stale words), then the eager search on a side stream against the reference's trace"""
	from librubiks_amd.solving.agents import AStar
	from oracle.search_oracle import StubNet
	from tests import test_astar_gpu as A
	t, tag = golden["astar_trace"], "a"
	_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
	net = S.GatedNet(StubNet())
	agent = AStar(net, float(t[f"{tag}_lambda"]), expansions, use_hipgraph=False)
	cap = max(int(min(max_states, agent.capacity or agent.default_capacity)), 12 * expansions + 2)
	_adopt(agent, _null_stream_gated_create("rk_astar_create", cap, expansions), "rk_astar_destroy")
	agent._h_cap, agent._h_expansions = cap, expansions
	h = agent._h
	solved = _eager(lambda: agent.search(t[f"{tag}_start"], time_limit=None, max_states=max_states), net, ["rk_astar_step_commit"])
	assert agent._h is h and solved == bool(t[f"{tag}_solved"]) and net.calls >= agent.iterations > 1
	A._check_against(agent, t[f"{tag}_states"], t[f"{tag}_G"], t[f"{tag}_parents"], t[f"{tag}_parent_actions"], t[f"{tag}_action_queue"])


def test_eager_astar_batch(golden):
	from librubiks_amd.solving.agents import AStarBatch
	from oracle.search_oracle import StubNet
	t, tag = golden["astar_trace"], "a"
	_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
	net = S.GatedNet(StubNet())
	agent = AStarBatch(net, float(t[f"{tag}_lambda"]), expansions, 1, capacity=max_states)
	solved = _eager(lambda: agent.search(t[f"{tag}_start"][None], max_states=max_states, use_graph=False, poll=1), net,
	                ["rk_astarb_step_commit"])
	n = int(t[f"{tag}_n"])
	assert bool(solved[0]) == bool(t[f"{tag}_solved"]) and int(agent.status[0, 2]) == n and int(agent.status[0, 3]) == len(t[f"{tag}_pop_lens"])
	states, G, parents, pact = agent.arrays_of(0)
	assert (states[1:] == t[f"{tag}_states"]).all() and (G[1:] == t[f"{tag}_G"]).all()
	assert (parents[2:] == t[f"{tag}_parents"]).all() and (pact[2:] == t[f"{tag}_parent_actions"]).all()
	assert list(agent.action_queue_of(0)) == t[f"{tag}_action_queue"].tolist()


def test_eager_mcts_batch():
	"""MCTSBatch(use_graph=False) with the priors in the backup kernel: between a forward and its backup the step only enqueues, and
	with poll=32 most iterations never wait.  Four trees of tests/test_mcts_gpu.py's batch case, each against the oracle run alone."""
	from librubiks_amd.solving.agents import MCTSBatch
	from oracle import cube_oracle as orc
	from oracle.search_oracle import MCTSOracle, StubNet
	from tests import test_mcts_gpu as M
	T, c = 4, 5.0
	starts, budgets = [], []
	for i in range(T):
		np.random.seed(200 + i)
		starts.append(orc.scramble(2 + i % 5, True)[0])
		budgets.append(600 + 250 * i)
	starts = np.array(starts)
	net = S.GatedNet(StubNet())
	agent = MCTSBatch(net, c, T, capacity=4000)
	assert agent.priors == "kernel"
	solved = _eager(lambda: agent.search(starts, max_states=np.array(budgets), use_graph=False, poll=32), net,
	                ["rk_mcts_set_root_pv", "rk_mcts_backup_select_logits", "rk_mcts_backup_select"],
	                warm=lambda: agent.search(starts[::-1].copy(), max_states=np.array(budgets), use_graph=False, poll=32))
	assert net.calls == agent.simulations + 1 > 32                       # the root's forward, then one per simulation; more than one poll
	n_solved = 0
	for i in range(T):
		ref = MCTSOracle(StubNet(), c, False)
		ref_solved = ref.search(starts[i], budgets[i])
		assert bool(solved[i]) == ref_solved, i
		assert list(agent.action_queue_of(i)) == list(ref.action_queue), i
		M._same_tree(agent.tree_arrays(i), ref)
		assert int(agent.status[i, 3]) == ref.sims
		n_solved += ref_solved
	assert n_solved > 0


# ------------------------------------------------------------------------------------- pattern C, engines on one ball
def test_beam_and_symball_search_share_a_ball_on_two_streams():
	"""a DeviceBeamSearch and a DeviceSymBallSearch attached to the same DeviceSymBall: the frontier engine's iterations wait behind a
	gate on one stream while the beam search runs on another; each equals its solo run"""
	from librubiks_amd.solving.agents import DeviceBeamSearch
	from tests import beam_model as bm
	from tests import test_beam_gpu as Bt
	ball = DeviceSymBall(bm.BALL_RADIUS).build()
	case = ("noisy", 22, 572, 6)
	ref, start = bm.ball_reference(case), bm.start_of(572, 6)
	beam = DeviceBeamSearch(Bt._device_net("noisy"), 22, 12, ball=ball)
	root = _root(2)
	solo = DeviceSymBallSearch(ball, pops=16, capacity=65536)
	assert solo.search(root, None, 1 << 30)
	n_solo, queue_solo, cols_solo = len(solo), list(solo.action_queue), solo.arrays()
	front = DeviceSymBallSearch(ball, pops=16, capacity=65536)
	h, e = front._engine(65536), front._entry
	torch.cuda.synchronize()
	s1, s2 = S.side_stream(), S.side_stream()
	with torch.cuda.stream(s1):
		beam.search(bm.start_of(999, 7), None, None)      # warm: the kept step is captured
		s1.synchronize()
	with torch.cuda.stream(s2):
		_ffi.check(e("reset")(h, root.ctypes.data, 1 << 30, _ffi.stream_ptr()))
		ev = S.gate(s2)
		_ffi.check(e("run")(h, 64, _ffi.stream_ptr()))
		S.held(ev)
	with torch.cuda.stream(s1):
		solved = beam.search(start, None, None)
	with torch.cuda.stream(s2):
		st = S.status_words(e("status"), h, front._status_words)
		cols = eng.export_frontier(e("export"), (h,), st[2], 1)
		path = list(eng.read_path(e("path"), h))
	torch.cuda.synchronize()
	Bt._same(beam, solved, ref, case)
	assert st[0] and st[1] and st[6] == 0 and st[2] == n_solo and path == queue_solo
	for a, b in zip(cols, cols_solo):
		assert (a[1:] == b).all()
	front._free()
