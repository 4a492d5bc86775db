"""
Two-sided breadth-first search on one MI355X: DeviceBiBFS (engine rk_bibfs_*), with the one-sided DeviceBFS beside it where one
side still reaches.

    python benchmarks/bibfs.py [--lengths 8 10 12 14 16] [--pops 16384] [--repeats 3] [--out profiles/r09_bibfs.json]

Starts of known optimal length: seeded 40-move scrambles are cut to their prefixes (every prefix of a scramble is a start), the
prefixes are searched with DeviceBiBFS in rising order, and for every wanted length L the first prefix whose shortest solution
has exactly L moves is kept (the next seed is taken while a length is missing).  For each L, in one process:
  bibfs_s         seconds per DeviceBiBFS search (best of --repeats after a warm-up search) on the agent that made the selection:
                  its pool has grown to `capacity` by then, and every search clears the table of that capacity (4 GB at 256 M
                  states), which is most of the time at the short lengths; a fresh agent with the default pool is untimed here,
                  len (states stored on both sides together), depths (f, b), iterations, popped, us_per_iteration, states_per_s
  bfs_s           for L <= --bfs-max-length: seconds per DeviceBFS search from the same start (same pops, same protocol of warm-up
                  and repeats), its len and iterations, and ratio_bfs_over_bibfs = bfs_s / bibfs_s
Every search is checked: the queue has L moves and solves the start.  The rows go to stdout as JSON lines and, with --out, into one
JSON document.  --one-search L runs the selection and two searches of that length and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import cube  # noqa: E402
from librubiks_amd.solving.agents import DeviceBFS, DeviceBiBFS  # noqa: E402


def scramble_prefixes(seed: int, depth: int = 40) -> list:
	rng = np.random.RandomState(seed)
	s, out = cube.get_solved(), []
	for a in rng.randint(0, 12, depth):
		s = cube.rotate(s, *cube.action_space[a])
		out.append(s.copy())
	return out


def solves(start: np.ndarray, queue) -> bool:
	s = start
	for a in queue:
		s = cube.rotate(s, *cube.action_space[a])
	return bool(cube.is_solved(s))


def pick_starts(agent, lengths, seed: int, time_limit: float) -> dict:
	"""{L: (seed, prefix length, start)}: the first prefix of optimal length L, for every wanted L."""
	found, top = {}, max(lengths)
	while len(found) < len(lengths) and seed < 10_000:
		for k, start in enumerate(scramble_prefixes(seed), 1):
			if k < min(set(lengths) - set(found)):
				continue                                   # a k-move prefix has no solution longer than k
			if not agent.search(start, time_limit=time_limit):
				break
			L = len(agent.action_queue)
			if L in lengths and L not in found:
				found[L] = (seed, k, start)
			if L > top or len(found) == len(lengths):
				break                                      # longer prefixes only get deeper (and dearer)
		seed += 1
	return found


def timed(agent, start, repeats: int, **limits):
	agent.search(start, **limits)                          # warm-up: allocates (and grows) the pool, loads the kernels
	best = None
	for _ in range(repeats):
		t0 = time.perf_counter()
		ok = agent.search(start, **limits)
		dt = time.perf_counter() - t0
		best = dt if best is None else min(best, dt)
	return ok, best


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--lengths", type=int, nargs="+", default=[8, 10, 12, 14, 16])
	ap.add_argument("--pops", type=int, default=16_384)
	ap.add_argument("--poll", type=int, default=8)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--bfs-max-length", type=int, default=8)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--time-limit", type=float, default=60.0)
	ap.add_argument("--out", default=None)
	ap.add_argument("--one-search", type=int, default=None)
	args = ap.parse_args()
	lengths = sorted(set(args.lengths if args.one_search is None else [args.one_search]))
	two = DeviceBiBFS(pops=args.pops, poll=args.poll)
	starts = pick_starts(two, lengths, args.seed, args.time_limit)
	if args.one_search is not None:
		_, _, start = starts[args.one_search]
		for _ in range(2):
			assert two.search(start, time_limit=args.time_limit) and len(two.action_queue) == args.one_search
		return
	rows = []
	for L in lengths:
		if L not in starts:
			rows.append({"length": L, "error": "no prefix of this optimal length found"})
			print(json.dumps(rows[-1]), flush=True)
			continue
		seed, k, start = starts[L]
		ok, best = timed(two, start, args.repeats, time_limit=args.time_limit)
		assert ok and len(two.action_queue) == L and solves(start, two.action_queue)
		row = {
			"length": L, "seed": seed, "scramble_moves": k, "pops": args.pops, "bibfs_s": round(best, 6), "len": len(two),
			"depths": list(two.depths), "iterations": two.iterations, "popped": two.popped, "grown_in_warmup": two.grown,
			"us_per_iteration": round(1e6 * best / max(two.iterations, 1), 2), "states_per_s": round(len(two) / best),
			"capacity": two._h_cap,
		}
		if L <= args.bfs_max_length:
			one = DeviceBFS(pops=args.pops, poll=args.poll)
			ok, best1 = timed(one, start, args.repeats, max_states=2 ** 31 - 1)
			assert ok and len(one.action_queue) == L and solves(start, one.action_queue)
			row.update({"bfs_s": round(best1, 6), "bfs_len": len(one), "bfs_iterations": one.iterations,
			            "ratio_bfs_over_bibfs": round(best1 / best, 2)})
			del one
		rows.append(row)
		print(json.dumps(row), flush=True)
	if args.out:
		import torch
		doc = {"benchmark": "benchmarks/bibfs.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "rows": rows}
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")


if __name__ == "__main__":
	main()
