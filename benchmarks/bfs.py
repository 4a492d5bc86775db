"""
Breadth-first search on one MI355X: DeviceBFS (engine rk_bfs_*) against the host agent `agents.BFS`.

    python benchmarks/bfs.py [--depths 6 7 8] [--pops 16384] [--repeats 3] [--host-max-depth 6]

Full searches from the start of a seeded 40-move scramble with max_states = the number of states within distance d (quarter-turn
metric), so every search returns False with exactly the balls of radius d stored.  One JSON line per depth:
  device_s (best of --repeats, pool sized up front: no growth inside the timed search), states_per_s, children_per_s,
  us_per_iteration, pops (P), iterations, len, len_ok (len == the ball's size), host_s (agents.BFS, depths <= --host-max-depth),
  bytes_per_child (the kernels' global traffic by the model below) and hbm_fraction (that traffic per second over 8 TB/s).
Traffic model per child (parent-major, so a parent's 20 bytes are shared by its 12 children): the parent read 20/12, the
table compare-and-swap 8 (read and write of 4), the slot 4 + 4, the table word 4, the prefix 4 + 4, the first-occurrence flag
1 + 1, and per NEW state its 20-byte row, parent 4, action 1 and the table write 4.  Probe chains past the first slot and
the look-back words are left out; the CAS is counted as a read plus a write although atomics execute at the memory side.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import cube  # noqa: E402
from librubiks_amd.solving.agents import BFS, DeviceBFS  # noqa: E402

LEVELS = [1, 12, 114, 1_068, 10_011, 93_840, 878_880, 8_221_632, 76_843_595]
HBM_PEAK = 8.0e12


def scramble(seed: int, depth: int = 40) -> np.ndarray:
	rng = np.random.RandomState(seed)
	s = cube.get_solved()
	for a in rng.randint(0, 12, depth):
		s = cube.rotate(s, *cube.action_space[a])
	return s


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--depths", type=int, nargs="+", default=[6, 7, 8])
	ap.add_argument("--pops", type=int, default=16_384)
	ap.add_argument("--poll", type=int, default=8)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--host-max-depth", type=int, default=6)
	ap.add_argument("--seed", type=int, default=2024)
	args = ap.parse_args()
	start = scramble(args.seed)
	for depth in args.depths:
		budget = sum(LEVELS[:depth + 1])
		agent = DeviceBFS(pops=args.pops, capacity=budget + 12 * args.pops * (args.poll + 1), poll=args.poll)
		agent.search(start, max_states=budget)              # warm-up: allocates the pool, loads the kernels
		best = None
		for _ in range(args.repeats):
			t0 = time.perf_counter()
			solved = agent.search(start, max_states=budget)
			dt = time.perf_counter() - t0
			best = dt if best is None else min(best, dt)
		children = 12 * agent.popped
		new_per_child = (len(agent) - 1) / max(children, 1)
		bpc = 20 / 12 + 8 + 4 + 4 + 4 + 4 + 4 + 1 + 1 + new_per_child * (20 + 4 + 1 + 4)
		row = {
			"depth": depth, "max_states": budget, "solved": bool(solved), "len": len(agent), "len_ok": len(agent) == budget,
			"grown": agent.grown, "pops": args.pops, "iterations": agent.iterations, "popped": agent.popped, "children": children,
			"device_s": round(best, 6), "states_per_s": round(len(agent) / best), "children_per_s": round(children / best),
			"us_per_iteration": round(1e6 * best / max(agent.iterations, 1), 2), "new_per_child": round(new_per_child, 4),
			"bytes_per_child": round(bpc, 2), "hbm_fraction": round(bpc * children / best / HBM_PEAK, 4),
		}
		if depth <= args.host_max_depth:
			host = BFS()
			t0 = time.perf_counter()
			host.search(start, max_states=budget)
			row["host_s"] = round(time.perf_counter() - t0, 4)
			row["host_len"] = len(host)
			row["speedup_vs_host"] = round(row["host_s"] / best, 1)
		print(json.dumps(row), flush=True)


if __name__ == "__main__":
	main()
