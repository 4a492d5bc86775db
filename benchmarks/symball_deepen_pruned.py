"""
The probes past the symmetry ball with and without pruning by pattern databases, on one MI355X, everything in one process.

    python benchmarks/symball_deepen_pruned.py [--batch 1000000] [--skip small searches] [--out profiles/r28_deepen_pruned.json]

The bound is all eight corners and the two disjoint six-edge sets of benchmarks/pattern_db.py (edges 0..5 and 6..11).  Every
workload runs unpruned, then pruned, in turn, after a warm-up of both on a small slice; equal lengths and equal action queues are
asserted, and a row reports the words issued, the ball look-ups made, their ratio, the wall time of each run (host clock around a
call that ends in a device read) and the ratio pruned / unpruned.  No threshold is set: a ratio above 1 is reported as it is.

  batches_r10   benchmarks/symball_deepen.py's batches: DeviceSymBall(10).solve_beyond(extra=3) on --batch seeded scrambles of 11,
                12 and 13 moves.
  batches_r8    the same scrambles on DeviceSymBall(8) with extra=5: the small ball, where the cut reaches further up the word.
  searches      DeviceSymBallSearch(ball10, max_capacity=20 M, deepen=8) on the 23- and 24-move prefixes of seed 0's scramble
                (optimal length 19 and 20 in profiles/r17_symball_deepen.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import cube  # noqa: E402
from librubiks_amd.solving.agents import DevicePatternBound, DevicePatternDB, DeviceSymBall, DeviceSymBallSearch  # noqa: E402
from benchmarks.bibfs import scramble_prefixes, solves  # noqa: E402
from benchmarks.symball_deepen import scrambles  # noqa: E402


def timed(call):
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	out = call()
	torch.cuda.synchronize()
	return out, time.perf_counter() - t0


def compared(row: dict, plain, s_plain: float, pruned, s_pruned: float) -> dict:
	"""`row` with the counts (probes, lookups) and seconds of both runs"""
	row.update({"probes": plain[0], "lookups_unpruned": plain[1], "lookups_pruned": pruned[1], "lookups_over_probes": round(pruned[1] / max(plain[0], 1), 5),
	            "lookups_saved": round(1.0 - pruned[1] / max(plain[0], 1), 5), "unpruned_s": round(s_plain, 4), "pruned_s": round(s_pruned, 4),
	            "ratio_pruned_over_unpruned_s": round(s_pruned / s_plain, 3), "equal_answers": True})
	assert plain[0] == pruned[0] and plain[0] == plain[1] and pruned[1] <= pruned[0], (plain, pruned)
	print(json.dumps(row), flush=True)
	return row


def batches(ball: DeviceSymBall, bound: DevicePatternBound, extra: int, args) -> list:
	rows = []
	for moves in (11, 12, 13):
		states = scrambles(args.batch, moves, 100 + moves).cpu().numpy()
		ball.solve_beyond(states[:1024], extra)                              # both kernels loaded, every round's shapes seen
		ball.solve_beyond(states[:1024], extra, prune=bound)
		(len_a, act_a), s_plain = timed(lambda: ball.solve_beyond(states, extra))
		plain = (ball.probes, ball.lookups)
		(len_b, act_b), s_pruned = timed(lambda: ball.solve_beyond(states, extra, prune=bound))
		pruned = (ball.probes, ball.lookups)
		assert (len_a == len_b).all() and (act_a == act_b).all()
		rows.append(compared({"radius": ball.radius, "extra": extra, "scramble_moves": moves, "states": args.batch, "unanswered": int((len_a < 0).sum()),
		                      "beyond_the_ball": int((len_a > ball.radius).sum())}, plain, s_plain, pruned, s_pruned))
	return rows


def searches(ball: DeviceSymBall, bound: DevicePatternBound, args) -> list:
	rows = []
	agents = [DeviceSymBallSearch(ball, pops=args.pops, capacity=args.far_capacity, max_capacity=args.far_capacity, deepen=8, prune=p) for p in (None, bound)]
	prefixes = list(scramble_prefixes(args.seed))
	for agent in agents:
		agent.search(prefixes[17], time_limit=args.time_limit)               # a shorter start: the pool made, the kernels loaded
	for k in (23, 24):
		start = prefixes[k - 1]
		runs = []
		for agent in agents:
			ok, s = timed(lambda: agent.search(start, time_limit=args.time_limit))
			assert ok and solves(start, agent.action_queue)
			runs.append((list(agent.action_queue), agent.deepened, (agent.probes, agent.lookups), s))
		assert runs[0][:2] == runs[1][:2]
		rows.append(compared({"radius": ball.radius, "scramble_moves": k, "seed": args.seed, "capacity": args.far_capacity, "length": len(runs[0][0]),
		                      "deepened": runs[0][1]}, runs[0][2], runs[0][3], runs[1][2], runs[1][3]))
	return rows


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--pops", type=int, default=16_384)
	ap.add_argument("--seed", type=int, default=0)
	ap.add_argument("--far-capacity", type=int, default=20_000_000)
	ap.add_argument("--batch", type=int, default=1_000_000)
	ap.add_argument("--time-limit", type=float, default=120.0)
	ap.add_argument("--skip", nargs="*", default=[], choices=["batches", "small", "searches"])
	ap.add_argument("--out", default=os.path.join("profiles", "r28_deepen_pruned.json"))
	args = ap.parse_args()
	cube.set_is2024(True)
	t0 = time.perf_counter()
	dbs = [DevicePatternDB.corners(), DevicePatternDB(edges=range(6)), DevicePatternDB(edges=range(6, 12))]
	bound = DevicePatternBound(dbs)
	doc = {"device": torch.cuda.get_device_name(0), "databases": ["corners", "six edges 0..5", "six edges 6..11"], "database_bytes": sum(len(db) for db in dbs),
	       "databases_build_s": round(time.perf_counter() - t0, 3), "pops": args.pops}
	print(json.dumps(doc), flush=True)

	def save():
		with open(args.out, "w") as f:                           # after every part: a later part that runs out of time loses nothing
			json.dump(doc, f, indent=1)
			f.write("\n")

	if "small" not in args.skip:
		ball8 = DeviceSymBall(8, pops=args.pops).build()
		doc["batches_r8"] = batches(ball8, bound, 5, args)
		save()
		del ball8
	ball = DeviceSymBall(10, pops=args.pops).build()
	if "batches" not in args.skip:
		doc["batches_r10"] = batches(ball, bound, 3, args)
		save()
	if "searches" not in args.skip:
		doc["searches"] = searches(ball, bound, args)
		save()


if __name__ == "__main__":
	main()
