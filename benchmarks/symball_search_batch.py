"""
Many shortest-solution searches that end at the symmetry ball on one MI355X: DeviceSymBallSearchBatch (engine rk_ssearchb_*) against
the unchanged DeviceSymBallSearch run one search after the other, on the radius-10 symmetry ball, and beside the unchanged
DeviceBallSearchBatch on the radius-8 plain ball where its pools fit; everything in one process.

    python benchmarks/symball_search_batch.py [--per-length 256] [--lengths 12 14 16] [--searches 16 64 256] [--pops 512 2048 16384]
                                              [--out profiles/r16_symball_search_batch.json]

  starts      per optimal length L, --per-length starts: seeded L-move scrambles (benchmarks/bfs.py: scramble) whose shortest
              solution has L moves.  The lengths are found by the batch itself and every one is checked in the run: the sequential
              engine must find the same length from the same start.  `mixed` is all of them, the lengths interleaved.
  sequential  every set through one DeviceSymBallSearch (its default pops), search after search: seconds (best of --repeats passes
              after a warm-up search), searches_per_s, iterations, states stored.
  batch       every set through DeviceSymBallSearchBatch for every (searches, pops): seconds (best of --repeats calls after a warm-up
              call, which makes the engine), searches_per_s, lock-step iterations, us_per_lockstep_iteration, states_per_s (states
              stored by all searches per second) and speedup = sequential seconds / batch seconds.
  plain       the sets of lengths up to --plain-max-length through DeviceBallSearchBatch at --plain-searches slots on the plain ball
              of radius --plain-radius: a search of length 16 stores 49 M states there, 64 such pools do not fit; same columns, and
              sym_over_plain = plain seconds / the symmetry batch's seconds at the same slots and pops.
Equal lengths are asserted throughout.  `favoured_pops_at_64` is the pops with the most searches per second on the mixed set at 64
searches; `slower_than_sequential` lists the settings (set, searches, pops) with a speed-up below 1.  No threshold is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd.solving.agents import (DeviceBallSearchBatch, DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch,  # noqa: E402
                                          DeviceSymBallSearchBatch)
from benchmarks.bfs import scramble  # noqa: E402


def pick_sets(ball, lengths, per_length: int, seed: int, capacity: int) -> dict:
	"""{L: (per_length, 20) starts of optimal length L}, fewer if 8 x per_length scrambles of L moves do not hold as many (about a fifth of the 14- and 16-move scrambles are that far away)."""
	b = DeviceSymBallSearchBatch(ball, searches=256, capacity=capacity)
	sets = {}
	for L in lengths:
		cand = np.stack([scramble(seed + 1_000 * L + j, L) for j in range(8 * per_length)])
		assert b.search(cand).all()
		sets[L] = cand[b.lengths == L][:per_length]
		print(json.dumps({"length": L, "candidates": len(cand), "of_that_length": int((b.lengths == L).sum()), "taken": len(sets[L])}), flush=True)
	return sets


def sequential_row(agent, name: str, starts: np.ndarray, repeats: int):
	agent.search(starts[0])                                  # warm-up: the pool, the kernels
	best, lengths = None, None
	for _ in range(repeats):
		got, iterations, stored = [], 0, 0
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		for s in starts:
			ok = agent.search(s)
			got.append(len(agent.action_queue) if ok else -1)
			iterations += agent.iterations; stored += len(agent)
		dt = time.perf_counter() - t0
		best, lengths = (dt if best is None else min(best, dt)), np.array(got)
	n = len(starts)
	return {"set": name, "n": n, "engine": type(agent).__name__, "pops": agent.pops, "seconds": round(best, 6), "searches_per_s": round(n / best, 1),
	        "iterations": iterations, "us_per_iteration": round(1e6 * best / max(iterations, 1), 2), "states_stored": stored,
	        "states_per_s": round(stored / best)}, lengths


def batch_row(b, name: str, starts: np.ndarray, repeats: int, seq: dict, lengths: np.ndarray):
	assert (b.search(starts) == (lengths >= 0)).all() and (b.lengths == lengths).all()          # warm-up, and the same answers
	best = None
	for _ in range(repeats):
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		b.search(starts)
		dt = time.perf_counter() - t0
		best = dt if best is None else min(best, dt)
	assert (b.lengths == lengths).all() and not b.capacity_exhausted.any()
	n, stored, its = len(starts), int(b.sizes.sum()), b.lockstep_iterations
	return {"set": name, "n": n, "engine": type(b).__name__, "searches": b.searches, "pops": b.pops, "seconds": round(best, 6),
	        "searches_per_s": round(n / best, 1), "lockstep_iterations": its, "us_per_lockstep_iteration": round(1e6 * best / max(its, 1), 2),
	        "states_stored": stored, "states_per_s": round(stored / best), "speedup_over_sequential": round(seq["seconds"] / best, 2)}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--radius", type=int, default=10)
	ap.add_argument("--lengths", type=int, nargs="+", default=[12, 14, 16])
	ap.add_argument("--per-length", type=int, default=256)
	ap.add_argument("--searches", type=int, nargs="+", default=[16, 64, 256])
	ap.add_argument("--pops", type=int, nargs="+", default=[512, 2_048, 16_384])
	ap.add_argument("--capacity", type=int, default=1_250_000, help="states per slot of the symmetry batch: six own levels and 12 x 16 384 children")
	ap.add_argument("--plain-radius", type=int, default=8)
	ap.add_argument("--plain-searches", type=int, default=64)
	ap.add_argument("--plain-max-length", type=int, default=14)
	ap.add_argument("--plain-capacity", type=int, default=2_000_000, help="states per slot of the plain batch")
	ap.add_argument("--repeats", type=int, default=2)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	t0 = time.perf_counter()
	ball = DeviceSymBall(args.radius).build()
	torch.cuda.synchronize()
	build_s = time.perf_counter() - t0
	picked = pick_sets(ball, sorted(args.lengths), args.per_length, args.seed, args.capacity)
	sets = {str(L): s for L, s in picked.items()}
	most = max(len(s) for s in sets.values())
	sets["mixed"] = np.stack([s[j] for j in range(most) for s in picked.values() if j < len(s)])
	doc = {"benchmark": "benchmarks/symball_search_batch.py", "device": torch.cuda.get_device_name(0), "radius": args.radius, "orbits": len(ball),
	       "ball_build_seconds": round(build_s, 3), "repeats": args.repeats, "capacity_per_slot": args.capacity,
	       "sets": {k: len(v) for k, v in sets.items()}, "sequential": [], "batch": [], "plain_batch": []}
	agent = DeviceSymBallSearch(ball)
	seq = {}
	for name, starts in sets.items():
		seq[name] = sequential_row(agent, name, starts, args.repeats)
		doc["sequential"].append(seq[name][0])
		print(json.dumps(seq[name][0]), flush=True)
	del agent
	for searches in args.searches:
		for pops in args.pops:
			b = DeviceSymBallSearchBatch(ball, searches=searches, pops=pops, capacity=args.capacity)
			for name, starts in sets.items():
				doc["batch"].append(batch_row(b, name, starts, args.repeats, *seq[name]))
				print(json.dumps(doc["batch"][-1]), flush=True)
			del b
	# the plain batch on the plain ball, where its pools fit
	plain_ball = DeviceGoalBall(args.plain_radius).build()
	fits = [str(L) for L in sorted(args.lengths) if L <= args.plain_max_length]
	doc["plain_radius"], doc["plain_capacity_per_slot"], doc["plain_sets"] = args.plain_radius, args.plain_capacity, fits
	for pops in args.pops:
		b = DeviceBallSearchBatch(plain_ball, searches=args.plain_searches, pops=pops, capacity=args.plain_capacity)
		for name in fits:
			row = batch_row(b, name, sets[name], args.repeats, *seq[name])
			same = [r for r in doc["batch"] if (r["set"], r["searches"], r["pops"]) == (name, args.plain_searches, pops)]
			if same:
				row["sym_over_plain"] = round(row["seconds"] / same[0]["seconds"], 2)
			doc["plain_batch"].append(row)
			print(json.dumps(row), flush=True)
		del b
	at64 = [r for r in doc["batch"] if r["set"] == "mixed" and r["searches"] == 64]
	if at64:
		doc["favoured_pops_at_64"] = max(at64, key=lambda r: r["searches_per_s"])["pops"]
	doc["slower_than_sequential"] = [[r["set"], r["searches"], r["pops"], r["speedup_over_sequential"]] for r in doc["batch"]
	                                 if r["speedup_over_sequential"] < 1.0]
	doc["batch_never_slower"] = not doc["slower_than_sequential"]
	if args.out:
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")


if __name__ == "__main__":
	main()
