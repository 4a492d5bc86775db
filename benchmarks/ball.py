"""
The goal ball on one MI355X: DeviceGoalBall (engine rk_ball_*) and DeviceBallSearch (engine rk_bsearch_*), everything in one process.

    python benchmarks/ball.py [--radii 6 7 8] [--queries 1000000 16000000] [--lengths 8 10 12 14 16] [--out profiles/r10_ball.json]

  build     per radius: seconds for a fresh ball (best of --repeats; allocation, the clearing of the table and the level checks
            included; a radius-1 ball is built first so that the kernels are loaded), states_per_s, iterations, us_per_iteration --
            and DeviceBFS to the same radius as benchmarks/bfs.py runs it (pool sized up front, warm-up search, best of --repeats).
  queries   `depth` and `solve` of the ball of the largest radius through the C entries on device tensors, timed with device events
            (one warm-up, best of 5): n queries drawn uniformly from the ball's own nodes, and n scrambles of 30 random moves
            (outside; the count that is inside after all is reported).  Two traffic models per query, both stated in the row:
            `requested` -- the bytes the threads ask for: 20 (query) + 4 per probed table word + 20 per compared row + the
            answer (4; solve: + radius, + 5 per step of the walk) -- with probes counted as 1 for a hit and 1 / (1 - load) for a
            miss (linear probing, every occupied word met costs a compare); `lines64` -- every random access moves a 64-byte line:
            a table word one line, a 20-byte row 1.25 lines (rows are 20 bytes apart, a quarter of them straddle two lines), a
            parent / action pair two lines.  hbm_fraction = lines64 bytes per second over 8 TB/s.
  searches  starts of optimal length L picked as benchmarks/bibfs.py picks them; DeviceBallSearch on the ball of the largest radius
            and the unchanged DeviceBiBFS from the same start: ms (best of --repeats after a warm-up search), states stored, iterations.
--queries-only skips the builds' repeats and the searches (for a kernel trace).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import _ffi, cube, gpu  # noqa: E402
from librubiks_amd.solving.agents import DeviceBallSearch, DeviceBFS, DeviceBiBFS, DeviceGoalBall  # noqa: E402
from benchmarks.bibfs import pick_starts, solves, timed  # noqa: E402
from benchmarks.bfs import scramble  # noqa: E402

LEVELS = DeviceGoalBall.LEVELS
HBM_PEAK = 8.0e12


def build_rows(radii, pops, repeats, seed):
	DeviceGoalBall(1, pops=pops).build()                       # loads the kernels
	rows = []
	for radius in radii:
		best = None
		for _ in range(repeats):
			ball = DeviceGoalBall(radius, pops=pops)
			torch.cuda.synchronize()
			t0 = time.perf_counter()
			ball.build()
			dt = time.perf_counter() - t0
			best = dt if best is None else min(best, dt)
			n, iterations = len(ball), ball.iterations
			del ball
		budget = sum(LEVELS[:radius + 1])
		one = DeviceBFS(pops=pops, capacity=budget + 12 * pops * 9, poll=8)
		start = scramble(seed)
		_, bfs_s = timed(one, start, repeats, max_states=budget)
		rows.append({"radius": radius, "pops": pops, "states": n, "build_s": round(best, 6), "states_per_s": round(n / best),
		             "iterations": iterations, "us_per_iteration": round(1e6 * best / max(iterations, 1), 2),
		             "bfs_s": round(bfs_s, 6), "bfs_len": len(one), "bfs_iterations": one.iterations,
		             "bfs_states_per_s": round(len(one) / bfs_s), "ratio_build_over_bfs": round(best / bfs_s, 2)})
		del one
		print(json.dumps(rows[-1]), flush=True)
	return rows


def device_ms(call, repeats: int = 5) -> float:
	call()
	torch.cuda.synchronize()
	best = None
	for _ in range(repeats):
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		call()
		b.record()
		torch.cuda.synchronize()
		ms = a.elapsed_time(b)
		best = ms if best is None else min(best, ms)
	return best


def query_rows(ball, sizes, seed):
	lib, radius = _ffi.lib(), ball.radius
	n_ball = len(ball)
	status = (C.c_longlong * 16)()
	_ffi.check(lib.rk_ball_status(ball._h, status))
	load = n_ball / (1 << (2 * n_ball + 2 - 1).bit_length())   # table slots: the power of two >= 2 C + 2
	pool = np.zeros((n_ball, 20), np.int8)
	_ffi.check(lib.rk_ball_export(ball._h, 1, n_ball, pool.ctypes.data, None, None, _ffi.stream_ptr()))
	mean_depth = sum(l * n for l, n in enumerate(LEVELS[:radius + 1])) / n_ball
	rng = np.random.RandomState(seed)
	rows = []
	for n in sizes:
		inside = torch.from_numpy(pool[rng.randint(0, n_ball, n)]).to(gpu)
		outside = torch.from_numpy(cube.repeat_state(cube.get_solved(), n)).to(gpu)
		g = torch.Generator(device=gpu).manual_seed(seed)
		for _ in range(30):
			outside = cube.device.multi_rotate(outside, torch.randint(0, 12, (n,), device=gpu, generator=g, dtype=torch.uint8))
		depth = torch.empty(n, dtype=torch.int32, device=gpu)
		acts = torch.empty((n, max(radius, 1)), dtype=torch.int8, device=gpu)
		for name, q in (("inside", inside), ("outside", outside)):
			stream = _ffi.stream_ptr()
			ms_d = device_ms(lambda: _ffi.check(lib.rk_ball_depth(ball._h, q.data_ptr(), n, depth.data_ptr(), stream)))
			found = int((depth >= 0).sum())
			ms_s = device_ms(lambda: _ffi.check(lib.rk_ball_solve(ball._h, q.data_ptr(), n, depth.data_ptr(), acts.data_ptr(), stream)))
			hit = name == "inside"
			probes = 1.0 if hit else 1.0 / (1.0 - load)
			compares = 1.0 if hit else probes - 1.0
			walk = mean_depth if hit else 0.0
			req_d = 20 + 4 * probes + 20 * compares + 4
			lin_d = 20 + 64 * probes + 80 * compares + 4
			req_s, lin_s = req_d + radius + 5 * walk, lin_d + radius + 128 * walk
			rows.append({"queries": n, "from": name, "radius": radius, "found": found, "table_load": round(load, 3),
			             "depth_ms": round(ms_d, 4), "depth_queries_per_s": round(n / ms_d * 1e3),
			             "depth_bytes_requested": round(req_d, 1), "depth_bytes_lines64": round(lin_d, 1),
			             "depth_hbm_fraction": round(lin_d * n / (ms_d * 1e-3) / HBM_PEAK, 4),
			             "solve_ms": round(ms_s, 4), "solve_queries_per_s": round(n / ms_s * 1e3),
			             "solve_bytes_requested": round(req_s, 1), "solve_bytes_lines64": round(lin_s, 1),
			             "solve_hbm_fraction": round(lin_s * n / (ms_s * 1e-3) / HBM_PEAK, 4)})
			print(json.dumps(rows[-1]), flush=True)
		del inside, outside
	return rows


def search_rows(ball, lengths, pops, repeats, seed, time_limit):
	two = DeviceBiBFS(pops=pops)
	starts = pick_starts(two, lengths, seed, time_limit)
	agent = DeviceBallSearch(ball, pops=pops)
	rows = []
	for L in lengths:
		if L not in starts:
			rows.append({"length": L, "error": "no prefix of this optimal length found"})
			continue
		s, k, start = starts[L]
		ok, best = timed(agent, start, repeats, time_limit=time_limit)
		assert ok and len(agent.action_queue) == L and solves(start, agent.action_queue)
		row = {"length": L, "seed": s, "scramble_moves": k, "radius": ball.radius, "pops": pops, "ball_search_ms": round(1e3 * best, 4),
		       "ball_search_len": len(agent), "ball_search_iterations": agent.iterations, "ball_search_depth": agent.depth,
		       "meeting_depth": agent.meeting_depth}
		ok, best2 = timed(two, start, repeats, time_limit=time_limit)
		assert ok and len(two.action_queue) == L
		row.update({"bibfs_ms": round(1e3 * best2, 4), "bibfs_len": len(two), "bibfs_iterations": two.iterations,
		            "bibfs_capacity": two._h_cap, "ratio_bibfs_over_ball_search": round(best2 / best, 2)})
		rows.append(row)
		print(json.dumps(row), flush=True)
	return rows


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--radii", type=int, nargs="+", default=[6, 7, 8])
	ap.add_argument("--queries", type=int, nargs="+", default=[1_000_000, 16_000_000])
	ap.add_argument("--lengths", type=int, nargs="+", default=[8, 10, 12, 14, 16])
	ap.add_argument("--pops", type=int, default=16_384)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--time-limit", type=float, default=60.0)
	ap.add_argument("--queries-only", action="store_true")
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	doc = {"benchmark": "benchmarks/ball.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
	if not args.queries_only:
		doc["build"] = build_rows(sorted(args.radii), args.pops, args.repeats, args.seed)
	ball = DeviceGoalBall(max(args.radii), pops=args.pops).build()
	doc["queries"] = query_rows(ball, args.queries, args.seed)
	if not args.queries_only:
		doc["searches"] = search_rows(ball, sorted(set(args.lengths)), args.pops, args.repeats, args.seed, args.time_limit)
	if args.out:
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")


if __name__ == "__main__":
	main()
