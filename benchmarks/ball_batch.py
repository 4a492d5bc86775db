"""
Many shortest-solution searches on one MI355X: DeviceBallSearchBatch (engine rk_bsearchb_*) against the unchanged DeviceBallSearch
run one search after the other, on the radius-8 ball, everything in one process.

    python benchmarks/ball_batch.py [--per-length 256] [--lengths 10 12 14] [--searches 16 64 256] [--pops 512 2048 16384]
                                    [--out profiles/r11_ball_batch.json]

  starts      per optimal length L, --per-length starts: seeded L-move scrambles (benchmarks/bfs.py: scramble) whose shortest
              solution has L moves.  The lengths are found by the batch itself and every one is checked in the run: the sequential
              engine must find the same length from the same start.  `mixed` is all of them, the lengths interleaved.
  sequential  every set through one DeviceBallSearch (its default pops), search after search: seconds (best of --repeats passes
              after a warm-up search), searches_per_s, iterations, states stored.
  batch       every set through DeviceBallSearchBatch for every (searches, pops): seconds (best of --repeats calls after a warm-up
              call, which makes the engine), searches_per_s, lock-step iterations, us_per_lockstep_iteration, states_per_s (states
              stored by all searches per second), hbm_fraction and speedup = sequential seconds / batch seconds.
hbm_fraction is benchmarks/bfs.py's traffic model -- per child 20/12 + 8 + 4 + 4 + 4 + 4 + 4 + 1 + 1 bytes and 29 per new state,
per second over 8 TB/s -- and leaves out the look-up in the ball (one or more 64-byte lines per child) as it leaves out probe chains.
`favoured_pops_at_64` is the pops with the most searches per second on the mixed set at 64 searches: the default of the class.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd.solving.agents import DeviceBallSearch, DeviceBallSearchBatch, DeviceGoalBall  # noqa: E402
from benchmarks.bfs import HBM_PEAK, scramble  # noqa: E402


def pick_sets(ball, lengths, per_length: int, seed: int, capacity: int) -> dict:
	"""{L: (per_length, 20) starts of optimal length L}, fewer if 3 x per_length scrambles of L moves do not hold as many."""
	b = DeviceBallSearchBatch(ball, searches=256, capacity=capacity)
	sets = {}
	for L in lengths:
		cand = np.stack([scramble(seed + 1_000 * L + j, L) for j in range(3 * per_length)])
		assert b.search(cand).all()
		sets[L] = cand[b.lengths == L][:per_length]
		print(json.dumps({"length": L, "candidates": len(cand), "of_that_length": int((b.lengths == L).sum()), "taken": len(sets[L])}), flush=True)
	return sets


def traffic(popped: int, stored: int, n: int) -> float:
	"""Bytes by benchmarks/bfs.py's model: `popped` nodes with 12 children each, `stored` - n new states."""
	children = 12 * popped
	return children * (20 / 12 + 8 + 4 + 4 + 4 + 4 + 4 + 1 + 1) + (stored - n) * (20 + 4 + 1 + 4)


def sequential_row(agent, name: str, starts: np.ndarray, repeats: int):
	agent.search(starts[0])                                  # warm-up: the pool, the kernels
	best, lengths = None, None
	for _ in range(repeats):
		got, iterations, stored, popped = [], 0, 0, 0
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		for s in starts:
			ok = agent.search(s)
			got.append(len(agent.action_queue) if ok else -1)
			iterations += agent.iterations; stored += len(agent); popped += agent.popped
		dt = time.perf_counter() - t0
		best, lengths = (dt if best is None else min(best, dt)), np.array(got)
	n = len(starts)
	return {"set": name, "n": n, "engine": "DeviceBallSearch", "pops": agent.pops, "seconds": round(best, 6), "searches_per_s": round(n / best, 1),
	        "iterations": iterations, "us_per_iteration": round(1e6 * best / max(iterations, 1), 2), "states_stored": stored,
	        "states_per_s": round(stored / best), "hbm_fraction": round(traffic(popped, stored, n) / best / HBM_PEAK, 5)}, lengths


def batch_row(b, name: str, starts: np.ndarray, repeats: int, seq: dict, lengths: np.ndarray):
	assert (b.search(starts) == (lengths >= 0)).all() and (b.lengths == lengths).all()          # warm-up, and the same answers
	best = None
	for _ in range(repeats):
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		b.search(starts)
		dt = time.perf_counter() - t0
		best = dt if best is None else min(best, dt)
	n, stored, its = len(starts), int(b.sizes.sum()), b.lockstep_iterations
	return {"set": name, "n": n, "engine": "DeviceBallSearchBatch", "searches": b.searches, "pops": b.pops, "seconds": round(best, 6),
	        "searches_per_s": round(n / best, 1), "lockstep_iterations": its, "us_per_lockstep_iteration": round(1e6 * best / max(its, 1), 2),
	        "states_stored": stored, "states_per_s": round(stored / best),
	        "hbm_fraction": round(traffic(int(b.popped.sum()), stored, n) / best / HBM_PEAK, 5),
	        "speedup_over_sequential": round(seq["seconds"] / best, 2)}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--radius", type=int, default=8)
	ap.add_argument("--lengths", type=int, nargs="+", default=[10, 12, 14])
	ap.add_argument("--per-length", type=int, default=256)
	ap.add_argument("--searches", type=int, nargs="+", default=[16, 64, 256])
	ap.add_argument("--pops", type=int, nargs="+", default=[512, 2_048, 16_384])
	ap.add_argument("--capacity", type=int, default=2_000_000, help="states per slot of the batch")
	ap.add_argument("--repeats", type=int, default=2)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	ball = DeviceGoalBall(args.radius).build()
	sets = {str(L): s for L, s in pick_sets(ball, sorted(args.lengths), args.per_length, args.seed, args.capacity).items()}
	most = max(len(s) for s in sets.values())
	sets["mixed"] = np.stack([s[j] for j in range(most) for s in sets.values() if j < len(s)])
	doc = {"benchmark": "benchmarks/ball_batch.py", "device": torch.cuda.get_device_name(0), "radius": args.radius, "repeats": args.repeats,
	       "capacity_per_slot": args.capacity, "sets": {k: len(v) for k, v in sets.items()}, "sequential": [], "batch": []}
	agent = DeviceBallSearch(ball)
	seq = {}
	for name, starts in sets.items():
		seq[name] = sequential_row(agent, name, starts, args.repeats)
		doc["sequential"].append(seq[name][0])
		print(json.dumps(seq[name][0]), flush=True)
	del agent
	for searches in args.searches:
		for pops in args.pops:
			b = DeviceBallSearchBatch(ball, searches=searches, pops=pops, capacity=args.capacity)
			for name, starts in sets.items():
				doc["batch"].append(batch_row(b, name, starts, args.repeats, *seq[name]))
				print(json.dumps(doc["batch"][-1]), flush=True)
			del b
	at64 = [r for r in doc["batch"] if r["set"] == "mixed" and r["searches"] == 64]
	if at64:
		doc["favoured_pops_at_64"] = max(at64, key=lambda r: r["searches_per_s"])["pops"]
	doc["batch_never_slower"] = all(r["speedup_over_sequential"] >= 1.0 for r in doc["batch"])
	if args.out:
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")


if __name__ == "__main__":
	main()
