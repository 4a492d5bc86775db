"""
Pins the search oracle (oracle/search_oracle.py) to the UNMODIFIED reference on REAL-VALUED net outputs: tests/golden/real_trace.npz
(tools/gen_golden_real.py) holds searches of the reference's AStar and MCTS driven by a torch twin of LookupNet, whose values and
logits are arbitrary float32 bit patterns that are nevertheless the same on any hardware.  AStarOracle must reproduce every array, the
pop order and the open queue left at the end -- float64 costs included, bit for bit -- and MCTSOracle, fed the P the reference stored,
the whole tree.  The second half checks that the inputs exercise what they are for (negative costs, relaxation, repeated and distinct
costs, infinities, denormals, zeros of both signs, real W), so that a weak input fails here and not silently on the GPU.  CPU only.
"""
import hashlib
import os

import numpy as np
import pytest

from oracle import cube_oracle as orc
from oracle.search_oracle import AStarOracle, LookupNet, MCTSOracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ASTAR_CASES = ["a_solve17", "a_offset1000", "a_special128", "a_bf16_3", "a_budget128", "a_solve3"]
MCTS_CASES = ["m_half", "m_one_graph", "m_five", "m_five_graph"]
_CACHE = {}
# the LookupNets of the searches that have no fixture (tests/test_real_valued_search_gpu.py, tests/test_sharded_real_valued_*.py)
VARIANTS = {
	"plain": dict(),                                           # costs positive, a misleading heuristic: both relaxation passes run
	"offset": dict(offset=9.0),                                # costs on both sides of zero
	"special": dict(offset=9.0, special=True),                 # ... and denormals, +-1e30, +-inf
	"bf16": dict(dtype="bfloat16", offset=9.0),                # bfloat16 outputs: the engine widens them itself
	"misleading": dict(scale=6.0, stub_weight=0.25),           # noise far above the signal, as NoisyStubNet's
}
_NETS = {}


def variant(name: str, seed: int = 30) -> LookupNet:
	if (name, seed) not in _NETS:
		_NETS[name, seed] = LookupNet(seed=seed, **VARIANTS[name])
	return _NETS[name, seed]


def load_trace() -> dict:
	if "trace" not in _CACHE:
		with np.load(os.path.join(GOLDEN, "real_trace.npz")) as z:
			_CACHE["trace"] = {k: z[k] for k in z.files}
	return _CACHE["trace"]


def net_of(t: dict, tag: str, **over) -> LookupNet:
	"""The LookupNet of a fixture case ({tag}_net: seed, scale, offset, bfloat16 tables, special, stub_weight)."""
	seed, scale, offset, bf16, special, stub_weight = (float(x) for x in t[f"{tag}_net"])
	kw = dict(seed=int(seed), scale=scale, offset=offset, dtype="bfloat16" if bf16 else "float32", special=bool(special), stub_weight=stub_weight)
	kw.update(over)
	return LookupNet(**kw)


def same(t: dict, key: str, a: np.ndarray) -> bool:
	"""`a` against the fixture's array `key`, stored in full or as SHA-256, shape and prefix; bit for bit (floats by their bytes)."""
	if key in t:
		want = t[key]
		a = np.ascontiguousarray(a, dtype=want.dtype)
		return a.shape == want.shape and a.tobytes() == want.tobytes()
	prefix = t[f"{key}_prefix"]
	a = np.ascontiguousarray(a, dtype=prefix.dtype)
	return (list(a.shape) == t[f"{key}_shape"].tolist() and a[:len(prefix)].tobytes() == prefix.tobytes()
	        and hashlib.sha256(a.tobytes()).hexdigest() == str(t[f"{key}_sha256"]))


def astar_oracle(tag: str):
	"""The oracle's search of an A* fixture case, made once -> (oracle, solved, open queue sorted as (cost, index) tuples)."""
	if tag not in _CACHE:
		t = load_trace()
		_, _, expansions, max_states = (int(x) for x in t[f"{tag}_params"])
		agent = AStarOracle(net_of(t, tag), float(t[f"{tag}_lambda"]), expansions)
		solved = agent.search(t[f"{tag}_start"], max_states)
		_CACHE[tag] = (agent, solved, sorted(agent.open))
	return _CACHE[tag]


def recorded_priors(t: dict, tag: str):
	"""The hook that hands MCTSOracle the P the reference stored: a search asks for the priors of its states in index order (the
	root, then every expansion's new states), so the rows of {tag}_P are handed out in order; `states` are compared afterwards."""
	P, given = t[f"{tag}_P"], [0]

	def in_order(batch, root):
		lo = given[0]
		assert root == (lo == 0)
		given[0] = lo + len(batch)
		return P[lo:lo + len(batch)]
	return in_order


def _apply(state, queue):
	for a in queue:
		state = orc.rotate(state, a // 2, 1 - a % 2)
	return state


# ---- the oracle against the reference ------------------------------------------------------------------------------------------
def test_fixture_holds_the_cases():
	t = load_trace()
	assert {k[:-len("_params")] for k in t if k.endswith("_params")} == set(ASTAR_CASES) | set(MCTS_CASES)
	lam = {float(t[f"{g}_lambda"]) for g in ASTAR_CASES}
	N = {int(t[f"{g}_params"][2]) for g in ASTAR_CASES}
	assert lam == {0.0, 0.05, 0.3, 1.0} and N == {3, 17, 128, 1000}
	assert any(t[f"{g}_net"][2] > 0 for g in ASTAR_CASES) and any(t[f"{g}_net"][3] for g in ASTAR_CASES) and any(t[f"{g}_net"][4] for g in ASTAR_CASES)
	assert {float(t[f"{g}_c"]) for g in MCTS_CASES} == {0.5, 1.0, 5.0} and {int(t[f"{g}_params"][2]) for g in MCTS_CASES} == {0, 1}


@pytest.mark.parametrize("tag", ASTAR_CASES)
def test_astar_oracle_reproduces_reference(tag):
	t = load_trace()
	seed, depth, _, _ = (int(x) for x in t[f"{tag}_params"])
	np.random.seed(seed)
	assert (orc.scramble(depth, True)[0] == t[f"{tag}_start"]).all()
	agent, solved, queue = astar_oracle(tag)
	assert solved == bool(t[f"{tag}_solved"]) and len(agent) == int(t[f"{tag}_n"])
	states, G, parents, pact = agent.arrays()
	assert same(t, f"{tag}_states", states)
	assert same(t, f"{tag}_G", G)
	assert same(t, f"{tag}_parents", parents)
	assert same(t, f"{tag}_parent_actions", pact)
	assert list(agent.action_queue) == t[f"{tag}_action_queue"].tolist()
	assert [len(p) for p in agent.pops] == t[f"{tag}_pop_lens"].tolist()
	assert same(t, f"{tag}_pops", np.concatenate(agent.pops))
	assert same(t, f"{tag}_open_idx", np.array([i for _, i in queue], np.int64))
	assert same(t, f"{tag}_open_cost", np.array([float(c) for c, _ in queue], np.float64))       # float64 costs, by their bytes
	if solved:
		assert orc.is_solved(_apply(t[f"{tag}_start"], agent.action_queue))


@pytest.mark.parametrize("tag", MCTS_CASES)
def test_mcts_oracle_reproduces_reference(tag):
	t = load_trace()
	seed, depth, search_graph, max_states = (int(x) for x in t[f"{tag}_params"])
	np.random.seed(seed)
	start = orc.scramble(depth, True)[0]
	assert (start == t[f"{tag}_start"]).all()
	agent = MCTSOracle(net_of(t, tag), float(t[f"{tag}_c"]), bool(search_graph), priors=recorded_priors(t, tag))
	solved = agent.search(start, max_states)
	n = len(agent)
	assert solved == bool(t[f"{tag}_solved"]) and n == int(t[f"{tag}_n"]) and agent.sims == int(t[f"{tag}_sims"])
	assert same(t, f"{tag}_states", agent.states[1:n + 1])
	assert same(t, f"{tag}_neighbors", agent.neighbors[1:n + 1])
	assert same(t, f"{tag}_leaves", agent.leaves[1:n + 1])
	assert same(t, f"{tag}_N", agent.N[1:n + 1])
	for name in ("P", "V", "W", "L"):
		a = getattr(agent, name)[1:n + 1]
		assert (a.astype(np.float32).astype(np.float64) == a).all(), name     # float32 numbers, as the fixture stores them
		assert same(t, f"{tag}_{name}", a + 0.0 if name == "W" else a), name      # (W: zeros as +0.0, see tools/gen_golden_real.py)
	assert list(agent.action_queue) == t[f"{tag}_action_queue"].tolist()
	if solved:
		assert orc.is_solved(_apply(start, agent.action_queue))
	# the default priors (float32 softmax on this host) agree with the reference's up to the exp of the day: not bit for bit by
	# contract, which is why the hook exists -- but closely
	own = MCTSOracle(net_of(t, tag), float(t[f"{tag}_c"]), bool(search_graph))
	p, _ = own._policy_value(agent.states[1:n + 1])
	assert np.abs(p - agent.P[1:n + 1]).max() < 1e-6


# ---- the net ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(seed=1), dict(seed=2, offset=14.0, special=True), dict(seed=4, dtype="bfloat16"), dict(seed=5, dtype="bfloat16", special=True)])
def test_lookup_net_is_the_same_on_numpy_and_torch_for_any_batch_shape(kw):
	import torch
	net = LookupNet(**kw)
	rng = np.random.RandomState(3)
	states = [orc.SOLVED.copy()]
	s = orc.SOLVED.copy()
	for a in rng.randint(0, 12, 700):
		s = orc.rotate(s, int(a) // 2, 1 - int(a) % 2)
		states.append(s)
	oh = orc.as_oh(np.array(states))
	p, v = net(oh)
	assert p.dtype == v.dtype == np.float32 and p.shape == (701, 12) and v.shape == (701, 1)
	want_dtype = torch.bfloat16 if net.dtype == "bfloat16" else torch.float32
	for lo, hi in ((0, 701), (0, 1), (5, 6), (100, 163), (699, 701)):
		for x in (torch.from_numpy(oh[lo:hi]), torch.from_numpy(oh[lo:hi]).to(torch.bfloat16)):
			tp, tv = net(x)
			assert tp.dtype == tv.dtype == want_dtype
			assert (tp.float().numpy().view(np.uint32) == p[lo:hi].view(np.uint32)).all()
			assert (tv.float().numpy().view(np.uint32) == v[lo:hi].view(np.uint32)).all()
			assert (net(x, policy=False).float().numpy().view(np.uint32) == v[lo:hi].view(np.uint32)).all()
			assert (net(x, value=False).float().numpy().view(np.uint32) == p[lo:hi].view(np.uint32)).all()
	if net.dtype == "bfloat16":                       # every table entry is a bfloat16 number
		assert not (net.value_table.view(np.uint32) & 0xFFFF).any() and not (net.logit_table.view(np.uint32) & 0xFFFF).any()


def test_lookup_net_tables_hold_what_they_promise():
	net = LookupNet(seed=3, special=True)
	vt = net.value_table.reshape(net.M, 21)
	a, b = net.planted["duplicates"]
	assert (vt[a].view(np.uint32) == vt[b].view(np.uint32)).all()
	a, b = net.planted["ulp_pairs"]
	assert (np.abs(vt[a].view(np.int32) - vt[b].view(np.int32)) == 1).all() and (vt[a] != vt[b]).all()
	assert (vt[net.planted["plus_zero"]] == 0).all() and not np.signbit(vt[net.planted["plus_zero"]]).any()
	assert (vt[net.planted["minus_zero"]] == 0).all() and np.signbit(vt[net.planted["minus_zero"]]).all()
	rows, values = net.planted["special"]
	assert (vt[rows] == values[:, None]).all()
	tiny = np.float32(1.1754944e-38)
	assert ((np.abs(values) < tiny) & (values != 0)).sum() == 16 and np.isposinf(values).sum() == 4 and np.isneginf(values).sum() == 4
	assert (np.abs(values) == np.float32(1e30)).sum() == 8
	assert not np.isnan(vt).any() and not np.isnan(net.logit_table).any()
	assert not np.isinf(LookupNet(seed=3).value_table).any()
	# near ties of the logit table: gaps from one ulp to 2^-16 on both sides of 2^-20, maxima of magnitude 0.01 .. 40, runner-up
	# at lower and at higher indices
	lt = net.logit_table
	gaps, mags, lower = [], [], 0
	for h, j, i in net.near_ties:
		assert lt[h].argmax() in (j, i) and lt[h, j] == lt[h].max()
		gaps.append(float(np.float32(lt[h, j]) - np.float32(lt[h, i])))
		mags.append(abs(float(lt[h, j])))
		lower += i < j
	gaps, mags = np.array(gaps), np.array(mags)
	for lo, hi in ((2.0 ** -30, 2.0 ** -24), (2.0 ** -24, 2.0 ** -22), (2.0 ** -22, 2.0 ** -20), (2.0 ** -20, 2.0 ** -18), (2.0 ** -18, 2.0 ** -15)):
		assert ((gaps >= lo) & (gaps < hi)).sum() >= 20, (lo, hi)
	assert (gaps == 0).any() and (gaps == 2.0 ** -20).any()
	assert mags.min() < 0.02 and mags.max() > 20 and 0.3 < lower / len(gaps) < 0.7


# ---- the inputs exercise what they are for ------------------------------------------------------------------------------------------
def _costs(tag):
	_, _, queue = astar_oracle(tag)
	return np.array([float(c) for c, _ in queue]), np.array([i for _, i in queue])


def test_negative_and_non_negative_costs_meet_in_one_queue():
	ok = 0
	for tag in ASTAR_CASES:
		cost, _ = _costs(tag)
		ok += bool(len(cost) and (cost < 0).mean() >= 0.25 and (cost >= 0).any())
	assert ok >= 1


def test_relaxation_ran():
	ran = 0
	for tag in ASTAR_CASES:
		agent, _, _ = astar_oracle(tag)
		G, par = np.array(agent.G), np.array(agent.parents)
		ran += bool((G[2:] != G[par[2:]] + 1).any())
	assert ran >= 1
	assert sum(int(load_trace()[f"{tag}_relaxed"]) > 0 for tag in ASTAR_CASES) >= 2       # ... and in the reference


@pytest.mark.parametrize("tag", ASTAR_CASES)
def test_costs_repeat_and_differ(tag):
	cost, _ = _costs(tag)
	distinct = len(np.unique(cost))
	assert 1 < distinct < len(cost)
	assert distinct >= 300                                   # real keys, not a handful of integers


def test_searches_end_both_ways():
	t = load_trace()
	assert sum(bool(t[f"{g}_solved"]) and len(t[f"{g}_action_queue"]) >= 4 for g in ASTAR_CASES) >= 2
	on_budget = [g for g in ASTAR_CASES if not bool(t[f"{g}_solved"]) and int(t[f"{g}_n"]) + 12 * int(t[f"{g}_params"][2]) > int(t[f"{g}_params"][3])]
	assert len(on_budget) >= 1


def test_special_case_queue_holds_the_edge_values():
	t = load_trace()
	tag = next(g for g in ASTAR_CASES if t[f"{g}_net"][4])
	agent, _, _ = astar_oracle(tag)
	cost, idx = _costs(tag)
	assert np.isposinf(cost).any()
	assert ((np.abs(cost) < 1.1754944e-38) & (cost != 0)).any()           # a float32 denormal, widened
	zero = idx[cost == 0]
	assert len(zero) and not np.signbit(cost[cost == 0]).any()                                            # the cost is +0.0 whatever the value's sign
	values = agent.net(orc.as_oh(np.array([agent.states[i] for i in zero])), policy=False).reshape(-1)
	assert (values == 0).all() and np.signbit(values).any() and (~np.signbit(values)).any()
	assert (np.abs(cost) == float(np.float32(1e30))).any()


def test_mcts_trees_hold_real_numbers():
	t = load_trace()
	rich = 0
	for tag in MCTS_CASES:
		_, _, search_graph, max_states = (int(x) for x in t[f"{tag}_params"])
		agent = MCTSOracle(net_of(t, tag), float(t[f"{tag}_c"]), bool(search_graph), priors=recorded_priors(t, tag))
		agent.search(t[f"{tag}_start"], max_states)
		n = len(agent)
		rich += len(np.unique(agent.W[1:n + 1])) > 2000 and agent.N[1:n + 1].max() > 100
	assert rich >= 2
