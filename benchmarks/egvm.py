"""
Epsilon-greedy value search on one MI355X: DeviceEGVM (engine rk_egvm_*) against the host agent `agents.EGVM` (the baseline).

    python benchmarks/egvm.py [--rounds 100] [--repeats 3] [--poll 8] [--out profiles/r07_egvm.json]

Both agents search from the same seeded 30-move scramble with max_states = rounds x workers x depth, seeded alike, so they walk
the same rounds (with the exact stub net the same states; a real net in bfloat16 may break a near-tie differently, see
DeviceEGVM).  Nets: the exact stub heuristic as one kernel (benchmarks/nets.py FastStub: the engine and the host loop with a net
that costs nothing) and fc_small in bfloat16 (random weights).  Parameters: the shipping ones of librubiks_amd/wire.py
(epsilon 0.375, 10 workers, depth 50) and 100 workers at the same depth.  One JSON line per (net, workers), and all of them in
--out: seconds per round and states per second of both agents (best of --repeats, after a warm-up search that loads the kernels
and, for DeviceEGVM, captures its two hipGraphs), and their ratio.

    python benchmarks/egvm.py --one-search          one DeviceEGVM search (fc_small bf16, wire parameters) after a warm-up, nothing
                                                    else: the process to put under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from librubiks_amd import cube  # noqa: E402
from librubiks_amd.solving.agents import EGVM, DeviceEGVM  # noqa: E402
from benchmarks.nets import FastStub, FcSmall  # noqa: E402

EPSILON, DEPTH = 0.375, 50


def scramble(seed: int, depth: int = 30) -> np.ndarray:
	rng = np.random.RandomState(seed)
	s = cube.get_solved()
	for a in rng.randint(0, 12, depth):
		s = cube.rotate(s, *cube.action_space[a])
	return s


class CastInput:
	"""A low-precision net for the host `EGVM`, which hands every net a float32 one-hot: the cast is part of the baseline's time."""
	def __init__(self, net, dtype):
		self.net, self.dtype = net, dtype

	def eval(self):
		return self

	def __call__(self, x, policy=True, value=True):
		return self.net(x.to(self.dtype), policy=policy, value=value)


def timed(agent, start, max_states: int, repeats: int, seed: int):
	"""-> (best seconds of a search, solved, len(agent), rounds walked) after one warm-up search."""
	np.random.seed(seed)
	agent.search(start, max_states=max_states)
	best = None
	for _ in range(repeats):
		np.random.seed(seed)
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		solved = agent.search(start, max_states=max_states)
		torch.cuda.synchronize()
		dt = time.perf_counter() - t0
		best = dt if best is None else min(best, dt)
	per_round = agent.workers * agent.depth
	return best, bool(solved), len(agent), -(-len(agent) // per_round)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--rounds", type=int, default=100)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--poll", type=int, default=8)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--workers", type=int, nargs="+", default=[10, 100])
	ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_egvm.json"))
	ap.add_argument("--one-search", action="store_true")
	args = ap.parse_args()
	start = scramble(args.seed)
	if args.one_search:
		agent = DeviceEGVM(FcSmall().cuda().eval().to(torch.bfloat16), EPSILON, 10, DEPTH, poll=args.poll)
		for _ in range(2):                                   # the first captures, the second is the one to look at
			np.random.seed(args.seed)
			agent.search(start, max_states=args.rounds * 10 * DEPTH)
		torch.cuda.synchronize()
		print(json.dumps({"one_search": True, "rounds": agent.rounds, "len": len(agent)}))
		return
	nets = {"stub": FastStub(), "fc_small_bf16": FcSmall().cuda().eval().to(torch.bfloat16)}
	rows = []
	for name, net in nets.items():
		for workers in args.workers:
			max_states = args.rounds * workers * DEPTH
			row = {"net": name, "epsilon": EPSILON, "workers": workers, "depth": DEPTH, "scramble_depth": 30, "max_states": max_states,
			       "poll": args.poll}
			host_net = CastInput(net, torch.bfloat16) if name.endswith("bf16") else net
			for key, agent in (("host", EGVM(host_net, EPSILON, workers, DEPTH)), ("device", DeviceEGVM(net, EPSILON, workers, DEPTH, poll=args.poll))):
				s, solved, n, rounds = timed(agent, start, max_states, args.repeats, args.seed)
				row.update({f"{key}_s": round(s, 6), f"{key}_solved": solved, f"{key}_len": n, f"{key}_rounds": rounds,
				            f"{key}_s_per_round": round(s / max(rounds, 1), 6), f"{key}_states_per_s": round(n / s)})
			row["device_over_host_states_per_s"] = round(row["device_states_per_s"] / max(row["host_states_per_s"], 1), 2)
			rows.append(row)
			print(json.dumps(row), flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, "w") as f:
		json.dump({"benchmark": "benchmarks/egvm.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
		f.write("\n")


if __name__ == "__main__":
	main()
