"""
Fixtures of A* and MCTS on REAL-VALUED net outputs -- TEST INFRASTRUCTURE, run on a CPU machine that has the unmodified reference checked
out (REFERENCE=path; default: a `reference` directory beside the repository).  No test imports this file; the tests read only what it
writes.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_real.py

It drives the reference's `AStar.search` (agents.py:171-413) and `MCTS.search` (agents.py:415-645) in the 20-byte representation under a
state budget alone, with `TwinNet` below: a torch net that returns the numbers of oracle/search_oracle.py's LookupNet -- arbitrary
float32 bit patterns looked up from tables, the same on any hardware and for any batch shape -- by arithmetic of its own (float64
products, integer remainder, two-dimensional indexing; LookupNet sums float32 products and takes a float remainder).  main() checks the
two against each other on every state a search stored.  Data only goes to tests/golden/real_trace.npz.

Per case (tag a_* for A*, m_* for MCTS):
  {tag}_net            LookupNet's arguments [seed, scale, offset, bfloat16 tables (0/1), special (0/1), stub_weight]
  {tag}_params         A*: [seed, scramble depth, expansions, max_states]; MCTS: [seed, scramble depth, search_graph, max_states]
  {tag}_lambda / _c    lambda / c
  {tag}_start, _solved, _n, _action_queue
  A*:   _states, _G, _parents, _parent_actions (rows 1..n, parents from row 2, as astar_trace.npz), _pops, _pop_lens, _relaxed (G
        entries lowered by relax_seen_states), _open_cost, _open_idx (the open queue left at the end, sorted as (cost, index) tuples)
  MCTS: _sims, _states, _neighbors, _leaves, _P (float32: the float32 softmax the reference stored, in full), _V, _N, _W, _L
        (float32: every entry is a float32 value or a multiple of nu, checked here; zeros of W are stored as +0.0, because the sign
        of np.maximum(-0.0, +0.0) in the max-backup, agents.py:562, is the NumPy build's choice)
An array of more than LIMIT bytes is stored as {key}_sha256 (of its C-order bytes), {key}_shape and {key}_prefix (its first PREFIX
rows) instead -- never P, which the CPU test feeds to the oracle.
"""
import hashlib
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden", "real_trace.npz")
LIMIT, PREFIX = 24 * 1024, 256

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore", category=DeprecationWarning)

from librubiks import cube  # noqa: E402
from librubiks.solving import agents  # noqa: E402
from oracle import cube_oracle as orc  # noqa: E402
from oracle.search_oracle import LookupNet  # noqa: E402

#: tag -> (seed, scramble depth, lambda, expansions, max_states, LookupNet arguments)
ASTAR = {
	"a_solve17": (102, 7, 0.3, 17, 20_000, dict(seed=1)),
	"a_offset1000": (104, 6, 0.05, 1000, 40_000, dict(seed=2, offset=14.0)),
	"a_special128": (108, 11, 0.0, 128, 30_000, dict(seed=3, offset=12.0, special=True)),
	"a_bf16_3": (101, 5, 1.0, 3, 4_000, dict(seed=4, dtype="bfloat16")),
	"a_budget128": (107, 12, 0.3, 128, 30_000, dict(seed=5)),
	"a_solve3": (115, 6, 1.0, 3, 10_000, dict(seed=6, scale=1.0, stub_weight=1.0)),
}
#: tag -> (seed, scramble depth, c, search_graph, max_states, LookupNet arguments)
MCTS = {
	"m_half": (23, 12, 0.5, False, 3_000, dict(seed=11)),
	"m_one_graph": (40, 4, 1.0, True, 3_000, dict(seed=12)),
	"m_five": (7, 6, 5.0, False, 1_200, dict(seed=13)),
	"m_five_graph": (42, 3, 5.0, True, 3_000, dict(seed=12)),
}


def net_args(kw) -> np.ndarray:
	return np.array([kw.get("seed", 0), kw.get("scale", 3.0), kw.get("offset", 0.0), float(kw.get("dtype", "float32") == "bfloat16"),
	                 float(kw.get("special", False)), kw.get("stub_weight", 0.5)], np.float64)


class TwinNet:
	"""LookupNet's numbers for torch one-hot batches, float32 out (a bfloat16 table holds bfloat16 numbers widened), by its own arithmetic."""
	def __init__(self, net: LookupNet):
		self.M = net.M
		self.w = torch.from_numpy(net.w.astype(np.float64))
		self.sol = torch.from_numpy(np.asarray(net.solved_oh, np.float64))
		self.values = torch.from_numpy(net.value_table.reshape(net.M, 21).copy())
		self.logits = torch.from_numpy(net.logit_table.copy())

	def eval(self):
		return self

	def __call__(self, x, policy=True, value=True):
		xd = x.double()
		h = (xd @ self.w).round().long() % self.M
		k = 20 - (xd @ self.sol).round().long()
		out = ([self.logits[h]] if policy else []) + ([self.values[h, k].unsqueeze(1)] if value else [])
		return out if len(out) > 1 else out[0]


def put(out: dict, key: str, a: np.ndarray, full: bool = False):
	a = np.ascontiguousarray(a)
	if full or a.nbytes <= LIMIT:
		out[key] = a
	else:
		out[f"{key}_sha256"] = np.array(hashlib.sha256(a.tobytes()).hexdigest())
		out[f"{key}_shape"] = np.array(a.shape, np.int64)
		out[f"{key}_prefix"] = a[:PREFIX].copy()


def save_npz(path: str, arrays: dict):
	"""An .npz like np.savez_compressed's, with fixed member timestamps: the same arrays give the same bytes."""
	import zipfile
	with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
		for key, a in arrays.items():
			info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
			info.compress_type = zipfile.ZIP_DEFLATED
			with z.open(info, "w", force_zip64=True) as f:
				np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def start_of(seed: int, depth: int) -> np.ndarray:
	np.random.seed(seed)
	state, _, _ = cube.scramble(depth, True)
	return state


def check_twin(net: LookupNet, twin: TwinNet, states: np.ndarray):
	p, v = twin(cube.as_oh(states))
	p2, v2 = net(orc.as_oh(states))
	assert (p.numpy().view(np.uint32) == p2.view(np.uint32)).all() and (v.numpy().view(np.uint32) == v2.view(np.uint32)).all()


def astar_case(out, tag, seed, depth, lam, expansions, max_states, kw):
	net = LookupNet(**kw)
	twin = TwinNet(net)
	state = start_of(seed, depth)
	agent = agents.AStar(twin, lambda_=lam, expansions=expansions)
	relax = [0]
	inner_relax = agent.relax_seen_states

	def counted_relax(*a, **k):
		m = len(agent) + 1                         # rows beyond hold whatever np.empty found
		before = agent.G[1:m].copy()
		r = inner_relax(*a, **k)
		relax[0] += int((agent.G[1:m] != before).sum())
		return r
	agent.relax_seen_states = counted_relax
	pops = []
	inner = agent.expand_batch
	agent.expand_batch = lambda idcs: (pops.append(np.array(idcs)), inner(idcs))[1]
	solved = bool(agent.search(state, time_limit=None, max_states=max_states))
	n = len(agent)
	check_twin(net, twin, agent.states[1:n + 1])
	queue = sorted(agent.open_queue)
	out[f"{tag}_net"] = net_args(kw)
	out[f"{tag}_params"] = np.array([seed, depth, expansions, max_states], np.int64)
	out[f"{tag}_lambda"] = np.array(float(lam))
	out[f"{tag}_start"] = np.asarray(state, np.int8)
	out[f"{tag}_solved"] = np.array(solved)
	out[f"{tag}_n"] = np.array(n, np.int64)
	out[f"{tag}_action_queue"] = np.array([int(a) for a in agent.action_queue], np.int64)
	out[f"{tag}_relaxed"] = np.array(relax[0], np.int64)
	out[f"{tag}_pop_lens"] = np.array([len(p) for p in pops], np.int64)
	put(out, f"{tag}_states", agent.states[1:n + 1].astype(np.int8))
	put(out, f"{tag}_G", agent.G[1:n + 1].astype(np.float64))
	put(out, f"{tag}_parents", agent.parents[2:n + 1].astype(np.int64))
	put(out, f"{tag}_parent_actions", agent.parent_actions[2:n + 1].astype(np.int64))
	put(out, f"{tag}_pops", np.concatenate(pops).astype(np.int64))
	put(out, f"{tag}_open_cost", np.array([float(c) for c, _ in queue], np.float64))
	put(out, f"{tag}_open_idx", np.array([int(i) for _, i in queue], np.int64))
	cost = np.array([float(c) for c, _ in queue])
	print(f"astar {tag}: solved={solved} n={n} iters={len(pops)} queue={len(agent.action_queue)} relaxed={relax[0]} open={len(cost)} "
	      f"negative={float((cost < 0).mean()) if len(cost) else 0:.3f} distinct={len(np.unique(cost))}", flush=True)


def mcts_case(out, tag, seed, depth, c, search_graph, max_states, kw):
	net = LookupNet(**kw)
	twin = TwinNet(net)
	state = start_of(seed, depth)
	agent = agents.MCTS(twin, c=c, search_graph=search_graph)
	sims = [0]
	inner = agent.expand_leaf

	def counted(v, a):
		sims[0] += 1
		return inner(v, a)
	agent.expand_leaf = counted
	solved = bool(agent.search(state, time_limit=None, max_states=max_states))
	n = len(agent)
	check_twin(net, twin, agent.states[1:n + 1])
	out[f"{tag}_net"] = net_args(kw)
	out[f"{tag}_params"] = np.array([seed, depth, int(search_graph), max_states], np.int64)
	out[f"{tag}_c"] = np.array(float(c))
	out[f"{tag}_start"] = np.asarray(state, np.int8)
	out[f"{tag}_solved"] = np.array(solved)
	out[f"{tag}_n"] = np.array(n, np.int64)
	out[f"{tag}_sims"] = np.array(sims[0], np.int64)
	out[f"{tag}_action_queue"] = np.array([int(a) for a in agent.action_queue], np.int64)
	put(out, f"{tag}_states", agent.states[1:n + 1].astype(np.int8))
	put(out, f"{tag}_neighbors", agent.neighbors[1:n + 1].astype(np.int32))
	put(out, f"{tag}_leaves", agent.leaves[1:n + 1].copy())
	put(out, f"{tag}_N", agent.N[1:n + 1].astype(np.int32))
	for name in ("P", "V", "W", "L"):
		a = getattr(agent, name)[1:n + 1]
		assert (a.astype(np.float32).astype(np.float64) == a).all(), name
		if name == "W":
			a = a + 0.0                        # -0.0 -> +0.0: which of the two np.maximum(-0.0, +0.0) returns (:562) is not defined
		put(out, f"{tag}_{name}", a.astype(np.float32), full=name == "P")
	W = agent.W[1:n + 1]
	print(f"mcts {tag}: solved={solved} n={n} sims={sims[0]} queue={len(agent.action_queue)} distinct W={len(np.unique(W))} "
	      f"max N={int(agent.N[1:n + 1].max())}", flush=True)


def main():
	torch.set_num_threads(1)
	cube.set_is2024(True)
	out = {}
	for tag, (seed, depth, lam, expansions, max_states, kw) in ASTAR.items():
		astar_case(out, tag, seed, depth, lam, expansions, max_states, kw)
	for tag, (seed, depth, c, search_graph, max_states, kw) in MCTS.items():
		mcts_case(out, tag, seed, depth, c, search_graph, max_states, kw)
	save_npz(OUT, out)
	print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
	main()
