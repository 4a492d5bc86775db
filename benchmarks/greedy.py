"""
The one-step agents under the Evaluator on one MI355X: games one after the other (`PolicySearch` / `ValueSearch`, the host loops)
against all games in lock-step on the device (`GreedyBatch`, engine rk_greedy_*).

    python benchmarks/greedy.py [--games 100] [--depths 2 4 8 25] [--max-states 30] [--repeats 2] [--out profiles/r08_greedy.json]

In one process, for both modes and two nets -- the exact stub heuristic as one kernel (benchmarks/nets.py FastStub: the loop with a
net that costs nothing) and fc_small in bfloat16 (random weights) -- it plays

    Evaluator(games, depths, max_states=S).eval(agent, batched=False)      and      .eval(agent, batched=True)

under the same seed, with all games in one group (batch_games = games x depths: a group costs games x max_states bytes), checks that
`res` and `states` are equal where the net is exact, and writes one JSON record per case: games and moves played, seconds (best of
--repeats after one warm-up of each leg; a batched eval includes making its engine and capturing its graph), moves per second,
microseconds per move (sequential) and per lock-step move of all games (batched), graph captures and the ratio.  The host agents
hand every net a float32 one-hot, so the sequential leg of the bfloat16 net runs behind a cast (part of its time, as in
benchmarks/egvm.py); the engine writes the bfloat16 one-hot itself.

    python benchmarks/greedy.py --one-search [--mode value]      two GreedyBatch searches (fc_small bf16, games x depths games),
                                                                   nothing else: the process to put under rocprofv3 --kernel-trace --stats
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
from librubiks_amd.solving.agents import GreedyBatch, PolicySearch, ValueSearch  # noqa: E402
from librubiks_amd.solving.evaluation import Evaluator  # noqa: E402
from benchmarks.egvm import CastInput  # noqa: E402
from benchmarks.nets import FastStub, FcSmall  # noqa: E402


class KeepingEvaluator(Evaluator):
	"""Remembers the batch engines it makes, for their counters."""
	def _batch_agent(self, agent, n):
		b = super()._batch_agent(agent, n)
		self.engines = getattr(self, "engines", []) + [b]
		return b


def timed(ev, agent, batched: bool, seed: int, repeats: int):
	best = None
	for i in range(repeats + 1):                                 # the first one warms up and is not timed
		ev.engines = []
		np.random.seed(seed)
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		res, states, _ = ev.eval(agent, batched=batched)
		torch.cuda.synchronize()
		dt = time.perf_counter() - t0
		if i and (best is None or dt < best):
			best = dt
	return best, res, states


def scrambles(n: int, depths, seed: int) -> np.ndarray:
	np.random.seed(seed)
	return np.array([cube.scramble(int(d), True)[0] for d in depths for _ in range(n)], dtype=np.int8)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--games", type=int, default=100)
	ap.add_argument("--depths", type=int, nargs="+", default=[2, 4, 8, 25])
	ap.add_argument("--max-states", type=int, default=30)
	ap.add_argument("--repeats", type=int, default=2)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--mode", default="value")
	ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_greedy.json"))
	ap.add_argument("--one-search", action="store_true")
	args = ap.parse_args()
	total = args.games * len(args.depths)
	if args.one_search:
		agent = GreedyBatch(FcSmall().cuda().eval().to(torch.bfloat16), args.mode, total)
		starts = scrambles(args.games, args.depths, args.seed)
		for _ in range(2):                                       # the first captures, the second is the one to look at
			agent.search(starts, max_states=args.max_states)
		torch.cuda.synchronize()
		print(json.dumps({"one_search": True, "mode": args.mode, "games": total, "launched": agent.launched, "moves": len(agent)}))
		return
	fc = FcSmall().cuda().eval().to(torch.bfloat16)
	nets = {"stub": (FastStub(), None), "fc_small_bf16": (fc, CastInput(fc, torch.bfloat16))}
	rows = []
	for name, (net, host_net) in nets.items():
		for mode, cls in (("policy", PolicySearch), ("value", ValueSearch)):
			ev = KeepingEvaluator(args.games, args.depths, max_states=args.max_states, batch_games=total)
			row = {"net": name, "mode": mode, "games": total, "depths": args.depths, "max_states": args.max_states}
			s_seq, res_s, states_s = timed(ev, cls(host_net or net), False, args.seed, args.repeats)
			s_bat, res_b, states_b = timed(ev, cls(net), True, args.seed, args.repeats)
			launched = sum(b.launched for b in ev.engines)
			moves_s, moves_b = int(states_s.sum()), int(states_b.sum())
			row.update({
				"sequential_s": round(s_seq, 6), "sequential_moves": moves_s, "sequential_solved": int((res_s != -1).sum()),
				"sequential_moves_per_s": round(moves_s / s_seq), "sequential_us_per_move": round(1e6 * s_seq / max(moves_s, 1), 2),
				"batched_s": round(s_bat, 6), "batched_moves": moves_b, "batched_solved": int((res_b != -1).sum()),
				"batched_moves_per_s": round(moves_b / s_bat), "lock_step_moves": launched,
				"batched_us_per_lock_step_move": round(1e6 * s_bat / max(launched, 1), 2),
				"graph_captures": sum(b.captures for b in ev.engines), "replayed": ev.replayed,
				"same_results": bool((res_s == res_b).all() and (states_s == states_b).all()),
				"batched_over_sequential": round(s_seq / s_bat, 2)})
			if name == "stub":
				assert row["same_results"], row                  # the stub is exact: the games are the same move for move
			rows.append(row)
			print(json.dumps(row), flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, "w") as f:
		json.dump({"benchmark": "benchmarks/greedy.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
		f.write("\n")


if __name__ == "__main__":
	main()
