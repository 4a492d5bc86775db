"""
Every search engine against its oracle on REAL-VALUED net outputs, bit for bit.  The nets are LookupNets (oracle/search_oracle.py):
their values and logits are arbitrary float32 (or bfloat16) bit patterns -- negative and positive, duplicates, pairs one ulp apart,
zeros of both signs, with `special` denormals, +-1e30 and infinities -- yet the same bits on the host and on the device for any batch
shape, so every comparison below is exact equality, the float arrays included.  tests/test_real_valued_oracle_cpu.py pins the oracles
to the unmodified reference on the same nets (tests/golden/real_trace.npz) and checks that the inputs are not weak.
  * AStar / AStarBatch against AStarOracle: pool, pop order, action queue and the whole open queue as (cost, index) pairs -- the
    float64 cost lambda * G + (-value), its order-preserving key on both sides of zero, and every sort and merge path on keys that
    are a few ulps apart (256-record runs, 2048-record chunks, merge passes, the multi-level rank merge);
  * MCTS / MCTSBatch against MCTSOracle, which takes P through its hook the way the engine's `priors` mode defines it, so the
    tree arithmetic (U + Q on real W, the max-backup) is compared whoever's exp made P;
  * GreedyBatch against the restatement of its rule -- first maximum of the logits, handed back when a float32 gap to the maximum
    lies in (0, 2^-20) -- and the host agents, on logit tables with gaps on both sides of that constant;
  * DeviceEGVM against the host EGVM.
"""
import numpy as np
import pytest
import torch

from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import AStar, AStarBatch, DeviceEGVM, EGVM, GreedyBatch, MCTS, MCTSBatch
from oracle import cube_oracle as orc
from oracle.search_oracle import AStarOracle, LookupNet, MCTSOracle
from tests.test_greedy_batch_gpu import STARTS, host_search, move, value_step
from tests.test_mcts_gpu import _same_tree
from tests.test_real_valued_oracle_cpu import ASTAR_CASES, MCTS_CASES, VARIANTS, astar_oracle, load_trace, net_of, variant  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- A* ---------------------------------------------------------------------------------------------------------------------
def _check_astar(agent: AStar, ref: AStarOracle, ref_solved: bool, solved: bool, what):
	assert solved == ref_solved, what
	states, G, parents, pact = ref.arrays()
	n = len(states)
	assert len(agent) == n, what
	assert (agent.states[1:n + 1] == states).all(), what
	assert (agent.G[1:n + 1] == G).all() and agent.G.dtype == np.float64, what
	assert (agent.parents[2:n + 1] == parents).all(), what
	assert (agent.parent_actions[2:n + 1] == pact).all(), what
	assert list(agent.action_queue) == list(ref.action_queue), what
	if not ref_solved:                                        # the whole open queue as (cost, index) pairs in pop order, costs bit for bit
		want = sorted(ref.open)
		got = agent.open_queue
		assert [i for _, i in got] == [int(i) for _, i in want], what
		got_c, want_c = np.array([c for c, _ in got], np.float64), np.array([float(c) for c, _ in want], np.float64)
		assert (got_c.view(np.uint64) == want_c.view(np.uint64)).all(), what           # (no -0.0 on either side: c + 0.0 and heapq's 0.0 + H)


@pytest.mark.parametrize("tag", ASTAR_CASES)
def test_astar_fixture_cases(tag):
	"""The cases the unmodified reference ran (the oracle equals it: test_real_valued_oracle_cpu), eager with the pop order recorded,
	eager as it runs in production, and as a replayed hipGraph."""
	t = load_trace()
	_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
	ref, ref_solved, _ = astar_oracle(tag)
	start, lam = t[f"{tag}_start"], float(t[f"{tag}_lambda"])
	bf16 = bool(t[f"{tag}_net"][3])
	net = net_of(t, tag)
	for mode in ("pops", "eager", "graph", "exact"):
		agent = AStar(net, lam, expansions, use_hipgraph=mode == "graph", exact_batch=mode == "exact")
		agent.record_pops = mode == "pops"
		solved = agent.search(start, None, max_states)
		_check_astar(agent, ref, ref_solved, solved, (tag, mode))
		if mode == "pops":
			assert [len(p) for p in agent.pops] == [len(p) for p in ref.pops]
			assert (np.concatenate(agent.pops) == np.concatenate(ref.pops)).all()
		if bf16:                                               # the values really went in as bfloat16
			assert net(torch.zeros(2, 480, device="cuda"), policy=False).dtype == torch.bfloat16


@pytest.mark.parametrize("seed,depth,lam,n,budget,net", [
	# the grid of test_astar_gpu.test_against_oracle -- K = 12 N decides how the new records are sorted and merged: runs of 256, up to
	# eight 2048-record chunks, chunks merged into one run first (N = 1500, N = 10 000) -- on real keys
	(101, 5, 0.0, 3, 4_000, "special"), (102, 7, 0.3, 17, 20_000, "plain"), (103, 9, 1.0, 128, 30_000, "offset"),
	(104, 6, 0.05, 1000, 40_000, "bf16"), (105, 10, 0.6, 50, 25_000, "misleading"), (106, 4, 2.5, 7, 10_000, "offset"),
	(107, 12, 0.2, 400, 120_000, "special"), (108, 11, 0.15, 1500, 150_000, "offset"), (109, 13, 0.1, 10_000, 400_000, "plain"),
	(110, 12, 0.0, 1500, 150_000, "special"), (111, 13, 0.1, 10_000, 400_000, "bf16"), (112, 14, 0.02, 200, 60_000, "misleading"),
])
def test_astar_against_oracle(seed, depth, lam, n, budget, net):
	np.random.seed(seed)
	start, _, _ = orc.scramble(depth, True)
	ref = AStarOracle(variant(net), lam, n)
	ref_solved = ref.search(start, budget)
	cost = np.array([float(c) for c, _ in ref.open])
	print(seed, net, "solved", ref_solved, "n", len(ref), "open", len(cost), "negative", float((cost < 0).mean()) if len(cost) else None,
	      "distinct", len(np.unique(cost)))
	for mode in ("eager", "graph") + (("exact",) if n >= 1000 else ()):
		agent = AStar(variant(net), lam, n, use_hipgraph=mode == "graph", exact_batch=mode == "exact")
		solved = agent.search(start, None, budget)
		_check_astar(agent, ref, ref_solved, solved, (seed, mode))


def test_astar_grid_inputs_are_not_weak():
	"""Of the grid above (the oracle alone, small cases): negative and non-negative costs in one queue, and relaxed nodes."""
	np.random.seed(101)
	start, _, _ = orc.scramble(5, True)
	ref = AStarOracle(variant("special"), 0.0, 3)
	assert not ref.search(start, 4_000)
	cost = np.array([float(c) for c, _ in ref.open])
	assert (cost < 0).mean() >= 0.25 and (cost >= 0).mean() >= 0.25 and 2_000 < len(np.unique(cost)) < len(cost)
	np.random.seed(112)
	start, _, _ = orc.scramble(14, True)
	ref = AStarOracle(variant("misleading"), 0.02, 200)
	ref.search(start, 60_000)
	G, par = np.array(ref.G), np.array(ref.parents)
	assert (G[2:] != G[par[2:]] + 1).sum() >= 20


@pytest.mark.parametrize("use_graph,n,exact,net", [(False, 10, False, "offset"), (True, 10, False, "special"), (False, 200, False, "bf16"),
                                                   (True, 200, False, "offset"), (False, 10, True, "misleading"), (False, 200, True, "special"),
                                                   (False, 1000, True, "offset")])
def test_astar_batch_equals_oracle_per_search(use_graph, n, exact, net):
	"""Ten searches with mixed depths and budgets in one engine -- the padded batch, the compacted one (`exact_batch`) and the replayed
	graph: each equals the oracle run alone."""
	S, lam = 10, 0.3
	starts, budgets = [], []
	for i in range(S):
		np.random.seed(500 + i)
		starts.append(orc.scramble(3 + i % 6, True)[0])
		budgets.append(3000 + 2500 * i)
	starts = np.array(starts)
	starts[4] = orc.SOLVED
	agent = AStarBatch(variant(net), lam, n, S, capacity=max(budgets))
	solved = agent.search(starts, max_states=np.array(budgets), use_graph=use_graph, poll=4, exact_batch=exact)
	n_solved = 0
	for i in range(S):
		ref = AStarOracle(variant(net), lam, n)
		ref_solved = ref.search(starts[i], budgets[i])
		assert bool(solved[i]) == ref_solved, i
		assert list(agent.action_queue_of(i)) == list(ref.action_queue), i
		if i != 4:
			states, G, parents, pact = agent.arrays_of(i)
			rs, rG, rp, ra = ref.arrays()
			assert (states[1:] == rs).all() and (G[1:] == rG).all() and (parents[2:] == rp).all() and (pact[2:] == ra).all(), i
			assert int(agent.status[i, 3]) == len(ref.pops), i
		n_solved += ref_solved
	assert 1 <= n_solved <= S


# ---- MCTS -------------------------------------------------------------------------------------------------------------------
def engine_priors(net, mode: str):
	"""MCTSOracle's hook: the priors of a batch of states as the engine's `priors` mode defines them -- "torch" and "kernel": the
	float32 softmax on the device; "reference": the root's on the device (ref:agents.py:472), everybody else's on the host in the
	logits' dtype (`p.cpu().softmax(dim=1)`, ref:agents.py:551-552)."""
	def hook(states, root):
		logits = net(torch.from_numpy(orc.as_oh(np.asarray(states, np.int8).reshape(-1, 20))).cuda(), value=False)
		if root or mode != "reference":
			return logits.float().softmax(dim=1).double().cpu().numpy()
		return agents._host_softmax(logits.cpu()).double().numpy()
	return hook


@pytest.mark.parametrize("priors,graph", [("reference", False), ("torch", False), ("kernel", False), ("torch", True), ("kernel", True)])
@pytest.mark.parametrize("tag", MCTS_CASES)
def test_mcts_fixture_cases(tag, priors, graph):
	t = load_trace()
	_, _, search_graph, max_states = (int(x) for x in t[f"{tag}_params"])
	net, c, start = net_of(t, tag), float(t[f"{tag}_c"]), t[f"{tag}_start"]
	ref = MCTSOracle(net, c, bool(search_graph), priors=engine_priors(net, priors))
	ref_solved = ref.search(start, max_states)
	agent = MCTS(net, c, bool(search_graph), use_hipgraph=graph, priors=priors)
	solved = agent.search(start, None, max_states)
	n = len(ref)
	print(tag, priors, graph, "solved", ref_solved, "n", n, "sims", ref.sims, "distinct W", len(np.unique(ref.W[1:n + 1])), "max N", int(ref.N.max()))
	assert solved == ref_solved and len(agent) == n
	_same_tree(agent._export(), ref)
	assert int(agent._batch.status[0, 3]) == ref.sims
	assert list(agent.action_queue) == list(ref.action_queue)
	# the tree is the reference's too wherever the priors are: same states in the same order as the fixture when P agrees to the bit
	if (ref.P[1:n + 1].astype(np.float32) == t[f"{tag}_P"]).all():
		assert n == int(t[f"{tag}_n"]) and ref.sims == int(t[f"{tag}_sims"]) and list(ref.action_queue) == t[f"{tag}_action_queue"].tolist()


@pytest.mark.parametrize("priors,use_graph,dtype,search_graph", [
	("kernel", False, "float32", False), ("kernel", True, "float32", True), ("torch", True, "float32", False), ("reference", False, "float32", True),
	("kernel", True, "bfloat16", False), ("torch", False, "bfloat16", True), ("reference", False, "bfloat16", False)])
def test_mcts_batch_equals_oracle_per_tree(priors, use_graph, dtype, search_graph):
	"""12 trees with different depths and budgets in one engine; each equals the oracle run alone -- the whole tree, the simulation
	count and the action queue."""
	T, c = 12, 1.0
	net = LookupNet(seed=41, dtype=dtype)
	starts, budgets = [], []
	for i in range(T):
		np.random.seed(200 + i)
		starts.append(orc.scramble(2 + i % 5, True)[0])
		budgets.append(600 + 250 * i)
	starts = np.array(starts)
	starts[7] = orc.SOLVED
	agent = MCTSBatch(net, c, T, capacity=4000, priors=priors, search_graph=search_graph)
	solved = agent.search(starts, max_states=np.array(budgets), use_graph=use_graph, poll=32)
	distinct = 0
	for i in range(T):
		ref = MCTSOracle(net, c, search_graph, priors=engine_priors(net, priors))
		ref_solved = ref.search(starts[i], budgets[i])
		assert bool(solved[i]) == ref_solved, i
		assert list(agent.action_queue_of(i)) == list(ref.action_queue), i
		if i != 7:
			_same_tree(agent.tree_arrays(i), ref)
			assert int(agent.status[i, 3]) == ref.sims
			distinct = max(distinct, len(np.unique(ref.W[1:len(ref) + 1])))
	assert solved[7] and distinct > (200 if dtype == "bfloat16" else 1000)        # (bfloat16 has 256 numbers per binade: a few hundred in all)


# ---- GreedyBatch ------------------------------------------------------------------------------------------------------------
TIE_GAP = np.float32(2.0 ** -20)


def restated_policy_game(net, state, max_states: int):
	"""Agent.search's loop around the ENGINE's policy rule, in float32 as the kernel states it: the action is the first maximum m of
	the logits; with gap_k = fl32(m - x_k), a game with some gap that is neither 0 nor >= 2^-20 is not moved but handed back (status
	3).  -> (status, action queue, the smallest positive gap met at every step, the hand-back's included)."""
	queue, met = [], []
	if orc.is_solved(state):
		return 1, queue, met
	solved = False
	while not solved and len(queue) < max_states:
		logits = np.asarray(net(orc.as_oh(state), value=False), np.float32).reshape(12)
		a = int(logits.argmax())                               # first maximum (no NaN in these tables)
		gaps = (logits[a] - logits).astype(np.float32)
		met.append(float(gaps[gaps > 0].min()) if (gaps > 0).any() else np.inf)
		if not ((gaps == 0) | (gaps >= TIE_GAP)).all():
			return 3, queue, met
		state = move(state, a)
		solved = orc.is_solved(state)
		queue.append(a)
	return (1 if solved else 2), queue, met


def restated_value_game(net, state, max_states: int):
	queue = []
	if orc.is_solved(state):
		return 1, queue
	solved = False
	while not solved and len(queue) < max_states:
		a, state, solved = value_step(net, state)
		queue.append(a)
	return (1 if solved else 2), queue


def greedy_starts() -> np.ndarray:
	rng = np.random.RandomState(17)
	out = [s for s in STARTS]
	for _ in range(106):
		s = orc.SOLVED.copy()
		for a in rng.randint(0, 12, rng.randint(1, 26)):
			s = move(s, int(a))
		out.append(s)
	return np.array(out, dtype=np.int8)


def _played(agent, starts, budget):
	agent.search(starts, time_limit=None, max_states=budget)
	return [(int(agent.status[i]), [int(a) for a in agent.action_queue_of(i)]) for i in range(len(starts))]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_greedy_policy_hands_back_exactly_the_near_ties(dtype):
	net = LookupNet(seed=51, dtype=dtype)
	starts, budget = greedy_starts(), 12
	want = [restated_policy_game(net, s, budget) for s in starts]
	agent = GreedyBatch(net, "policy", len(starts), poll=5)
	got = _played(agent, starts, budget)
	handed = [i for i, (st, _, _) in enumerate(want) if st == 3]
	for i, (g, w) in enumerate(zip(got, want)):
		print(dtype, i, "engine", g, "restated", w[:2], "gaps", ["%.3g" % x for x in w[2]])
	assert agent.handed_back.tolist() == handed                             # the same SET of games, exactly
	assert got == [(st, q) for st, q, _ in want]                            # ... each after the same moves; everybody else move for move
	for i, s in enumerate(starts):
		if i not in handed:
			assert got[i] == host_search(net, "policy", s, budget), i        # PolicySearch: argmax(softmax(logits)) on the host
	if dtype == "float32":
		# the inputs reach both sides of the constant: gaps just above it are played through -- by games that end handed back later and
		# by games that never are --, gaps just below it are handed back
		near_above = [i for i, (_, _, met) in enumerate(want) if any(2.0 ** -20 <= x < 2.0 ** -18 for x in met)]
		assert any(i in handed for i in near_above) and any(i not in handed for i in near_above)
		assert any(2.0 ** -22 <= want[i][2][-1] < 2.0 ** -20 for i in handed) and any(want[i][2][-1] < 2.0 ** -23 for i in handed)
		assert any(st == 2 and len(q) == budget for st, q, _ in want) and 10 <= len(handed) <= len(starts) - 10
		# a gap of one ulp occurs at small and at large magnitudes, at a lower and at a higher index than the maximum
		lt = net.logit_table
		lower = [lt[h, j] - lt[h, i] for h, j, i in net.near_ties if i < j and 0 < lt[h, j] - lt[h, i] < 2.0 ** -20]
		higher = [lt[h, j] - lt[h, i] for h, j, i in net.near_ties if i > j and 0 < lt[h, j] - lt[h, i] < 2.0 ** -20]
		assert len(lower) > 50 and len(higher) > 50
	else:
		assert len(handed) == 0                                              # bfloat16 numbers of these sizes are 0 or >= 2^-16 apart


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_greedy_value_equals_restatement_and_host(dtype):
	net = LookupNet(seed=52, dtype=dtype, special=dtype == "float32")
	starts, budget = greedy_starts()[:64], 15
	want = [restated_value_game(net, s, budget) for s in starts]
	agent = GreedyBatch(net, "value", 64, poll=4)
	got = _played(agent, starts, budget)
	for i, (g, w) in enumerate(zip(got, want)):
		print(dtype, i, "engine", g, "restated", w)
	assert got == want and len(agent.handed_back) == 0
	assert got == [host_search(net, "value", s, budget) for s in starts]
	assert any(st == 1 and len(q) > 1 for st, q in want) and any(st == 2 for st, q in want)


# ---- DeviceEGVM -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poll", [1, 3, 1000])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_device_egvm_equals_host_egvm(dtype, poll):
	"""Whole searches on real-valued outputs: the action queue, len(agent) and the state of the global NumPy generator afterwards are the
	host EGVM's (itself pinned to the reference by tests/golden/egvm_trace.npz), whatever the number of rounds between two polls."""
	net = LookupNet(seed=61, dtype=dtype, special=dtype == "float32")
	cases = [(1, 3, 0.3, 24, 6, 24 * 6 * 8), (2, 9, 0.5, 16, 8, 16 * 8 * 10), (3, 14, 0.0, 10, 12, 10 * 12 * 6), (4, 6, 1.0, 8, 5, 8 * 5 * 7),
	         (5, 2, 0.4, 32, 4, 32 * 4 * 20)]
	ends = set()
	for seed, depth, eps, workers, wdepth, budget in cases:
		np.random.seed(seed)
		start = orc.scramble(depth, True)[0]
		host = EGVM(net, eps, workers, wdepth)
		np.random.seed(1000 + seed)
		host_solved = host.search(start, time_limit=None, max_states=budget)
		host_state = np.random.get_state()
		dev = DeviceEGVM(net, eps, workers, wdepth, poll=poll)
		np.random.seed(1000 + seed)
		dev_solved = dev.search(start, time_limit=None, max_states=budget)
		dev_state = np.random.get_state()
		print(dtype, poll, seed, "host", host_solved, len(host), list(host.action_queue), "device", dev_solved, len(dev), list(dev.action_queue))
		assert dev_solved == host_solved and len(dev) == len(host)
		assert list(dev.action_queue) == [int(a) for a in host.action_queue]
		assert dev_state[0] == host_state[0] and (dev_state[1] == host_state[1]).all() and dev_state[2:] == host_state[2:]
		ends.add(bool(host_solved))
	assert ends == {True, False}
