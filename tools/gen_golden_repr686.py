"""
Fixtures of the 6x8x6 representation -- TEST INFRASTRUCTURE, run on a CPU machine that has the unmodified reference checked out
(default /root/reference, or REFERENCE=path).  No test imports this file; the tests read only what it writes.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_repr686.py

It drives the reference under `cube.set_is2024(False)` with the exact stub nets of tests/repr686_nets.py and writes data only:

  tests/golden/repr686_cube.npz     paired walks: the same actions applied in both representations (depth 0, the 12 single
                                    moves, random depths 1..30) -> 20-byte states and the 6x8x6 states as (n, 48) colours
  tests/golden/repr686_search.npz   AStar (nodes, G, parents, parent actions, action queue, pops per iteration), MCTS (states,
                                    neighbors, leaves, N, W, L, V, P, action queue), EGVM / ValueSearch action
                                    queues, and Train.ADI_traindata for the four reward methods

6x8x6 node arrays are stored as (n, 48) int8 colour indices plus the SHA-256 of the full (n, 6, 8, 6) int8 array.
"""
import hashlib
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = os.environ.get("REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.filterwarnings("ignore", category=DeprecationWarning)

from librubiks import cube  # noqa: E402
from librubiks.solving import agents  # noqa: E402
from repr686_nets import StubNet686, NoisyStubNet686, PolicyStubNet686  # noqa: E402


def sha(a: np.ndarray) -> str:
	return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def colours(states686: np.ndarray) -> np.ndarray:
	s = np.asarray(states686).reshape(-1, 48, 6)
	assert (s.sum(axis=2) == 1).all()
	return s.argmax(axis=2).astype(np.int8)


def walk(is2024: bool, actions: np.ndarray) -> np.ndarray:
	"""(games, depth) actions (-1 = none) -> the state of every game after its moves, in one representation."""
	cube.set_is2024(is2024)
	s = cube.repeat_state(cube.get_solved(), len(actions))
	for d in range(actions.shape[1]):
		live = actions[:, d] >= 0
		if live.any():
			f, dr = cube.indices_to_actions(actions[live, d])
			s[live] = cube.multi_rotate(s[live], f, dr)
	return s


def cube_fixture():
	rng = np.random.RandomState(686)
	games = 13 + 200
	depth = 30
	acts = np.full((games, depth), -1, np.int64)
	for a in range(12):
		acts[1 + a, 0] = a
	lens = rng.randint(1, 31, games - 13)
	for g, n in enumerate(lens):
		acts[13 + g, :n] = rng.randint(0, 12, n)
	s20 = walk(True, acts)
	s686 = walk(False, acts)
	cube.set_is2024(True)
	out = dict(actions=acts.astype(np.int8), states20=s20.astype(np.int8), colours686=colours(s686), sha686=np.array(sha(s686.astype(np.int8))))
	np.savez_compressed(os.path.join(OUT, "repr686_cube.npz"), **out)
	print(f"cube: {games} walks")


def astar(out):
	cases = {
		"a": dict(seed=7, depth=5, lambda_=0.5, expansions=10, max_states=3_000, net="plain"),
		"b": dict(seed=11, depth=9, lambda_=0.05, expansions=50, max_states=3_000, net="noisy"),
		"c": dict(seed=5, depth=6, lambda_=0.2, expansions=20, max_states=2_000, net="noisy"),
	}
	for tag, c in cases.items():
		cube.set_is2024(False)
		np.random.seed(c["seed"])
		state, _, _ = cube.scramble(c["depth"], True)
		net = NoisyStubNet686(1) if c["net"] == "noisy" else StubNet686()
		agent = agents.AStar(net, lambda_=c["lambda_"], expansions=c["expansions"])
		relax = [0]
		inner_relax = agent.relax_seen_states
		def counted_relax(*a, inner_relax=inner_relax, relax=relax, agent=agent, **k):
			before = agent.G.copy()
			r = inner_relax(*a, **k)
			relax[0] += int((agent.G[:len(before)] != before).sum())
			return r
		agent.relax_seen_states = counted_relax
		pops = []
		inner = agent.expand_batch
		agent.expand_batch = lambda idcs, inner=inner, pops=pops: (pops.append(np.array(idcs)), inner(idcs))[1]
		solved = agent.search(state, time_limit=None, max_states=c["max_states"])
		n = len(agent)
		p = f"astar_{tag}_"
		out[p + "params"] = np.array([c["seed"], c["depth"], c["expansions"], c["max_states"], int(c["net"] == "noisy")])
		out[p + "lambda"] = np.array(c["lambda_"])
		out[p + "start"] = state.astype(np.int8)
		out[p + "solved"] = np.array(solved)
		out[p + "n"] = np.array(n)
		out[p + "states"] = colours(agent.states[1:n + 1])
		out[p + "states_sha"] = np.array(sha(agent.states[1:n + 1].astype(np.int8)))
		out[p + "G"] = agent.G[1:n + 1].copy()
		out[p + "parents"] = agent.parents[2:n + 1].astype(np.int64)
		out[p + "parent_actions"] = agent.parent_actions[2:n + 1].astype(np.int64)
		out[p + "action_queue"] = np.array(list(agent.action_queue), dtype=np.int64)
		out[p + "pop_lens"] = np.array([len(q) for q in pops])
		out[p + "pops"] = np.concatenate(pops).astype(np.int64) if pops else np.zeros(0, np.int64)
		out[p + "relaxed"] = np.array(relax[0])
		print(f"astar {tag}: solved={solved} n={n} iterations={len(pops)} queue={len(agent.action_queue)} relaxed={relax[0]}")


def mcts(out):
	cases = {
		"a": dict(seed=7, depth=4, c=0.6, search_graph=False, max_states=2_500, net="plain"),
		"b": dict(seed=31, depth=3, c=5.0, search_graph=True, max_states=2_500, net="policy"),
	}
	for tag, c in cases.items():
		cube.set_is2024(False)
		np.random.seed(c["seed"])
		state, _, _ = cube.scramble(c["depth"], True)
		agent = agents.MCTS(PolicyStubNet686() if c["net"] == "policy" else StubNet686(), c=c["c"], search_graph=c["search_graph"])
		solved = agent.search(state, time_limit=None, max_states=c["max_states"])
		n = len(agent)
		p = f"mcts_{tag}_"
		out[p + "params"] = np.array([c["seed"], c["depth"], int(c["search_graph"]), c["max_states"], int(c["net"] == "policy")])
		out[p + "c"] = np.array(c["c"])
		out[p + "start"] = state.astype(np.int8)
		out[p + "solved"] = np.array(solved)
		out[p + "n"] = np.array(n)
		out[p + "states"] = colours(agent.states[1:n + 1])
		out[p + "states_sha"] = np.array(sha(agent.states[1:n + 1].astype(np.int8)))
		out[p + "neighbors"] = agent.neighbors[1:n + 1].astype(np.int32)
		out[p + "leaves"] = agent.leaves[1:n + 1].copy()
		out[p + "N"] = agent.N[1:n + 1].astype(np.int32)
		out[p + "W"] = agent.W[1:n + 1].astype(np.float32)
		out[p + "L"] = agent.L[1:n + 1].astype(np.float32)
		out[p + "V"] = agent.V[1:n + 1].astype(np.float32)
		out[p + "P"] = agent.P[1:n + 1].astype(np.float32)
		out[p + "action_queue"] = np.array(list(agent.action_queue), dtype=np.int64)
		assert (agent.W[1:n + 1] == out[p + "W"]).all() and (agent.P[1:n + 1] == out[p + "P"]).all()
		print(f"mcts {tag}: solved={solved} n={n} queue={len(agent.action_queue)}")


def greedy(out):
	cases = {
		"egvm": dict(seed=41, depth=5, max_states=4_000, agent=lambda: agents.EGVM(NoisyStubNet686(2), epsilon=0.3, workers=20, depth=8)),
		"egvm_policy": dict(seed=42, depth=4, max_states=3_000, agent=lambda: agents.EGVM(PolicyStubNet686(), epsilon=0.5, workers=16, depth=6)),
		# the one-step agents count their moves only when they stop (ref:agents.py:23-37), so max_states does not bound them: scrambles
		# they solve, under a time limit that is never reached
		"value": dict(seed=43, depth=2, max_states=40, agent=lambda: agents.ValueSearch(StubNet686())),
		"value_3": dict(seed=46, depth=3, max_states=40, agent=lambda: agents.ValueSearch(StubNet686())),
	}
	for tag, c in cases.items():
		cube.set_is2024(False)
		np.random.seed(c["seed"])
		state, _, _ = cube.scramble(c["depth"], True)
		agent = c["agent"]()
		solved = agent.search(state, time_limit=None if "egvm" in tag else 30, max_states=c["max_states"])
		assert solved or "egvm" in tag, tag
		p = f"{tag}_"
		out[p + "params"] = np.array([c["seed"], c["depth"], c["max_states"]])
		out[p + "start"] = state.astype(np.int8)
		out[p + "solved"] = np.array(solved)
		out[p + "len"] = np.array(len(agent))
		out[p + "action_queue"] = np.array([int(a) for a in agent.action_queue], dtype=np.int64)
		out[p + "rng_after"] = np.array(np.random.randint(0, 2 ** 31 - 1))          # the draws of the search, pinned
		print(f"{tag}: solved={solved} len={len(agent)} queue={len(agent.action_queue)}")


def adi(out):
	from librubiks import train as ref_train
	from librubiks.utils.ticktock import TickTock
	cases = {
		"lapanfix": dict(seed=12, games=37, depth=9, alpha=0.3, ff=3),
		"paper": dict(seed=12, games=37, depth=9, alpha=0.3, ff=3),
		"schultzfix": dict(seed=13, games=20, depth=11, alpha=0.0, ff=1),
		"reward0": dict(seed=14, games=50, depth=6, alpha=1.0, ff=4),
	}
	for method, c in cases.items():
		cube.set_is2024(False)
		me = types.SimpleNamespace(rollout_games=c["games"], rollout_depth=c["depth"], reward_method=method,
		                           adi_ff_batches=c["ff"], tt=TickTock(), with_analysis=False)
		me._get_adi_ff_slices = types.MethodType(ref_train.Train._get_adi_ff_slices, me)
		np.random.seed(c["seed"])
		oh, policy, value, lw = ref_train.Train.ADI_traindata(me, NoisyStubNet686(4), c["alpha"])
		oh = oh.cpu().numpy()
		p = f"adi_{method}_"
		out[p + "params"] = np.array([c["seed"], c["games"], c["depth"], c["ff"]])
		out[p + "alpha"] = np.array(c["alpha"])
		out[p + "oh_sha256"] = np.array(sha(oh.astype(np.float32)))
		out[p + "colours"] = colours(oh)
		out[p + "policy"] = policy.numpy().astype(np.int64)
		out[p + "value"] = value.numpy().astype(np.float32)
		out[p + "loss_weights"] = lw.numpy().astype(np.float32)
		print(f"adi {method}: n={len(oh)} values {float(value.min())}..{float(value.max())}")


def main():
	torch.set_num_threads(4)
	cube_fixture()
	out = {}
	astar(out)
	mcts(out)
	greedy(out)
	adi(out)
	cube.set_is2024(True)
	np.savez_compressed(os.path.join(OUT, "repr686_search.npz"), **out)
	for f in ("repr686_cube.npz", "repr686_search.npz"):
		print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
	main()
