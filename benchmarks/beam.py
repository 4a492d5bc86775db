"""
DeviceBeamSearch (engine rk_beam_*) on one MI355X, everything in one process.

    python benchmarks/beam.py [--widths 256 4096 65536] [--games 100] [--depths 14 20 30] [--radii 8 10] [--out profiles/r20_beam.json]

Nets: the stub heuristic (a forward that costs nothing) and fc_small in bfloat16 with the first layer fused and the BatchNorm
layers folded (random weights: the search is as long as it gets, the solutions say nothing about a trained net).
  depth rows    per (net, width): microseconds per depth split into the net forward and the engine's launches by device events
                (eager, --timed-depths depths after a warm-up on a depth-30 scramble that does not stop), the same depth replayed
                from the kept hipGraph, and the children per second that gives (12 x width rows per depth, an upper bound on states)
  search rows   per (net, ball, scramble depth): --games seeded scrambles through DeviceBeamSearch(width = --search-width) with
                ball None / DeviceSymBall(r) for r in --radii: share solved, mean length of the solutions, mean seconds, states
                explored; beside the unchanged AStar at N = 100 on the same starts (budget --astar-states)
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
from librubiks_amd import cube, _ffi  # noqa: E402
from librubiks_amd.solving import _engine as eng  # noqa: E402
from librubiks_amd.solving.agents import AStar, DeviceBeamSearch, DeviceSymBall  # noqa: E402
from benchmarks.nets import FastStub, FcSmall  # noqa: E402


def scramble(seed: int, depth: int) -> np.ndarray:
	rng = np.random.RandomState(seed)
	s = cube.get_solved()
	for a in rng.randint(0, 12, depth):
		s = cube.rotate(s, *cube.action_space[a])
	return s


def solves(start, queue) -> bool:
	for a in queue:
		start = cube.rotate(start, *cube.action_space[a])
	return bool(cube.is_solved(start))


def depth_split(net, fused, width: int, depths: int, poll: int) -> dict:
	"""us per depth: net forward and engine launches apart (eager, device events), and the whole depth replayed from the kept graph"""
	start = scramble(77, 30)
	agent = DeviceBeamSearch(net, width, max_depth=4 * depths + 8, poll=poll, fused_first_layer=fused)
	agent.search(start, None, None)                            # makes the engine, the batch and the graph; warms every shape
	h, batch, graph = agent._h, agent._batch[1], agent._graph_cache[1]
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	_ffi.check(lib.rk_beam_reset(h, start.ctypes.data, _ffi.INT64_MAX, stream))
	marks = [eng.events(3) for _ in range(depths)]
	with torch.no_grad():
		for m in marks:
			m[0].record()
			values, code = eng.engine_values(eng.sliced_value_forward(agent._forward, batch))
			m[1].record()
			_ffi.check(lib.rk_beam_step(h, values.data_ptr(), code, stream))
			m[2].record()
	torch.cuda.synchronize()
	net_us = [1e3 * m[0].elapsed_time(m[1]) for m in marks[2:]]
	eng_us = [1e3 * m[1].elapsed_time(m[2]) for m in marks[2:]]
	a, b = eng.events(2)
	a.record()
	for _ in range(depths):
		graph.replay()
	b.record()
	torch.cuda.synchronize()
	st = agent._poll(h)
	replay_us = 1e3 * a.elapsed_time(b) / depths
	return {"width": width, "rows_per_depth": 12 * width, "timed_depths": depths, "still_running": st[0] == 0,
	        "net_us_per_depth": round(float(np.mean(net_us)), 2), "engine_us_per_depth": round(float(np.mean(eng_us)), 2),
	        "engine_us_min": round(float(np.min(eng_us)), 2), "graph_us_per_depth": round(replay_us, 2),
	        "children_per_s_graph": round(12 * width / (replay_us * 1e-6))}


def play(agent, starts, **limits) -> dict:
	solved, lengths, seconds, states = 0, [], [], []
	for s in starts:
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		won = agent.search(s, **limits)
		torch.cuda.synchronize()
		seconds.append(time.perf_counter() - t0)
		states.append(len(agent))
		if won:
			assert solves(s, agent.action_queue)
			solved += 1
			lengths.append(len(agent.action_queue))
	return {"share_solved": round(solved / len(starts), 4), "mean_length": round(float(np.mean(lengths)), 2) if lengths else None,
	        "mean_s": round(float(np.mean(seconds)), 6), "mean_states": round(float(np.mean(states)), 1),
	        "states_per_s": round(float(np.sum(states) / np.sum(seconds)))}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--widths", type=int, nargs="+", default=[256, 4096, 65536])
	ap.add_argument("--search-width", type=int, default=4096)
	ap.add_argument("--max-depth", type=int, default=64)
	ap.add_argument("--games", type=int, default=100)
	ap.add_argument("--depths", type=int, nargs="+", default=[14, 20, 30])
	ap.add_argument("--radii", type=int, nargs="+", default=[8, 10])
	ap.add_argument("--timed-depths", type=int, default=24)
	ap.add_argument("--poll", type=int, default=8)
	ap.add_argument("--astar-states", type=int, default=200_000)
	ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_beam.json"))
	args = ap.parse_args()
	nets = {"stub": (FastStub(), False), "fc_small_bf16_fused_folded": (FcSmall().cuda().eval().to(torch.bfloat16), "folded")}
	doc = {"benchmark": "benchmarks/beam.py", "device": torch.cuda.get_device_name(0), "poll": args.poll, "depth_rows": [], "search_rows": []}
	for name, (net, fused) in nets.items():
		for width in args.widths:
			row = {"net": name, **depth_split(net, fused, width, args.timed_depths, args.poll)}
			doc["depth_rows"].append(row)
			print(json.dumps(row), flush=True)
	balls = {None: None}
	for r in args.radii:
		balls[r] = DeviceSymBall(r).build()
	for name, (net, fused) in nets.items():
		for depth in args.depths:
			starts = [scramble(1000 * depth + g, depth) for g in range(args.games)]
			for r, ball in balls.items():
				agent = DeviceBeamSearch(net, args.search_width, args.max_depth, ball=ball, poll=args.poll, fused_first_layer=fused)
				agent.search(starts[0], None, None)                # the capture is not timed
				row = {"net": name, "agent": "DeviceBeamSearch", "width": args.search_width, "max_depth": args.max_depth, "ball_radius": r,
				       "scramble_depth": depth, "games": args.games, **play(agent, starts)}
				doc["search_rows"].append(row)
				print(json.dumps(row), flush=True)
			astar = AStar(net, 0.2, 100, fused_first_layer=fused)
			astar.search(starts[0], None, args.astar_states)
			row = {"net": name, "agent": "AStar", "lambda": 0.2, "expansions": 100, "max_states": args.astar_states, "scramble_depth": depth,
			       "games": args.games, **play(astar, starts, time_limit=None, max_states=args.astar_states)}
			doc["search_rows"].append(row)
			print(json.dumps(row), flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, "w") as f:
		json.dump(doc, f, indent=1)
		f.write("\n")


if __name__ == "__main__":
	main()
