"""
Searches that go on past a full pool, many at once: DeviceSymBallSearchBatch(deepen=8) against the unchanged
DeviceSymBallSearch(deepen=8) run one search after the other, on one MI355X and the radius-10 symmetry ball, in one process.

    python benchmarks/symball_search_batch_deepen.py [--per-length 256] [--lengths 16 18] [--searches 16 64 256] [--pops 2048]
                                                     [--out profiles/r18_symball_batch_deepen.json]

  starts      per optimal length L, --per-length starts: seeded L-move scrambles whose shortest solution has L moves, found by the
              batch with ample pools (benchmarks/symball_search_batch.py: pick_sets).  `mixed` is all of them, interleaved.
  pools       held one level short, as benchmarks/symball_deepen.py holds them: capacity = the own levels that an ample search
              completes, less the last, plus half of that one -- 58 126 states at length 16 and 5 094 742 at length 18 on the
              radius-10 ball --, so the newest complete level is one earlier and two rounds are needed.  The mixed set runs in pools
              of its longest length.
  sequential  every set through one DeviceSymBallSearch(capacity = max_capacity = that, deepen=8): seconds, searches_per_s,
              probes and probes_per_s.
  batch       the same through DeviceSymBallSearchBatch(capacity = that, deepen=8) at every --searches: the same columns, the
              lock-step iterations, and ratio_to_sequential = sequential seconds / batch seconds.
Equal lengths are asserted throughout.  No ratio is promised; settings slower than the sequential run are listed as they come.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch, DeviceSymBallSearchBatch  # noqa: E402
from benchmarks.symball_search_batch import pick_sets  # noqa: E402

LEVELS = DeviceGoalBall.LEVELS                  # states at distance 0..8 of ANY state


def short_capacity(ball: DeviceSymBall, length: int) -> int:
	"""The pool of benchmarks/symball_deepen.py for a start of optimal length `length`: an ample search completes the own levels
	0 .. length - radius - 1; this holds them less the last, and half of that one."""
	depth = length - ball.radius - 1
	return sum(LEVELS[:depth]) + LEVELS[depth] // 2


def sequential_row(ball, name: str, starts: np.ndarray, capacity: int, pops: int, lengths: np.ndarray) -> dict:
	agent = DeviceSymBallSearch(ball, pops=pops, capacity=capacity, max_capacity=capacity, deepen=8)
	agent.search(starts[0])                                  # warm-up: the pool, the kernels
	probes, deepened = 0, []
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	for s, want in zip(starts, lengths):
		assert agent.search(s) and len(agent.action_queue) == want
		probes += agent.probes
		deepened.append(agent.deepened)
	dt = time.perf_counter() - t0
	return {"set": name, "n": len(starts), "engine": type(agent).__name__, "pops": pops, "capacity": capacity, "seconds": round(dt, 6),
	        "searches_per_s": round(len(starts) / dt, 2), "probes": probes, "probes_per_s": round(probes / dt),
	        "deepened": {str(e): deepened.count(e) for e in sorted(set(deepened))}}


def batch_row(ball, name: str, starts: np.ndarray, capacity: int, pops: int, searches: int, lengths: np.ndarray, seq: dict) -> dict:
	b = DeviceSymBallSearchBatch(ball, searches=searches, pops=pops, capacity=capacity, deepen=8)
	b.search(starts[:searches])                              # warm-up: the engine, the kernels
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	solved = b.search(starts)
	dt = time.perf_counter() - t0
	assert solved.all() and (b.lengths == lengths).all()
	rounds = b.deepened.tolist()
	return {"set": name, "n": len(starts), "engine": type(b).__name__, "searches": searches, "pops": pops, "capacity_per_slot": capacity,
	        "seconds": round(dt, 6), "searches_per_s": round(len(starts) / dt, 2), "probes": b.probes, "probes_per_s": round(b.probes / dt),
	        "lockstep_iterations": b.lockstep_iterations, "deepened": {str(e): rounds.count(e) for e in sorted(set(rounds))},
	        "ratio_to_sequential": round(seq["seconds"] / dt, 2)}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--radius", type=int, default=10)
	ap.add_argument("--lengths", type=int, nargs="+", default=[16, 18])
	ap.add_argument("--per-length", type=int, default=256)
	ap.add_argument("--searches", type=int, nargs="+", default=[16, 64, 256])
	ap.add_argument("--pops", type=int, default=2_048)
	ap.add_argument("--pick-capacity", type=int, default=12_000_000, help="states per slot while the starts are selected: ample for length 18")
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--out", default=os.path.join("profiles", "r18_symball_batch_deepen.json"))
	args = ap.parse_args()
	ball = DeviceSymBall(args.radius).build()
	picked = pick_sets(ball, sorted(args.lengths), args.per_length, args.seed, args.pick_capacity)
	sets = {str(L): (s, np.full(len(s), L), short_capacity(ball, L)) for L, s in picked.items()}
	most = max(len(s) for s in picked.values())
	mixed = [(s[j], L) for j in range(most) for L, s in picked.items() if j < len(s)]
	sets["mixed"] = (np.stack([s for s, _ in mixed]), np.array([L for _, L in mixed]), short_capacity(ball, max(args.lengths)))
	doc = {"benchmark": "benchmarks/symball_search_batch_deepen.py", "device": torch.cuda.get_device_name(0), "radius": args.radius, "orbits": len(ball),
	       "deepen": 8, "sets": {k: len(v[0]) for k, v in sets.items()}, "capacity": {k: v[2] for k, v in sets.items()}, "sequential": [], "batch": []}

	def save():
		with open(args.out, "w") as f:                       # after every row: a later row that runs out of time loses nothing
			json.dump(doc, f, indent=1)
			f.write("\n")
	for name, (starts, lengths, capacity) in sets.items():
		seq = sequential_row(ball, name, starts, capacity, args.pops, lengths)
		doc["sequential"].append(seq)
		print(json.dumps(seq), flush=True)
		save()
		for searches in args.searches:
			doc["batch"].append(batch_row(ball, name, starts, capacity, args.pops, searches, lengths, seq))
			print(json.dumps(doc["batch"][-1]), flush=True)
			save()
	doc["slower_than_sequential"] = [[r["set"], r["searches"], r["ratio_to_sequential"]] for r in doc["batch"] if r["ratio_to_sequential"] < 1.0]
	save()


if __name__ == "__main__":
	main()
