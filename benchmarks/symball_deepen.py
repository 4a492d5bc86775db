"""
Depth-first probes past the symmetry ball, on one MI355X and the radius-10 DeviceSymBall, everything in one process.

    python benchmarks/symball_deepen.py [--radius 10] [--pops 16384] [--batch 1000000] [--time-limit 120] [--out profiles/r17_symball_deepen.json]

  probe_rate   one full-cap launch of rk_sdeepen (2^28 probes: words of 4 moves from 40-move scrambles, none of which hits, so no
               rank is skipped): seconds and probes per second, by HIP events.  Beside it the parent commit's read-only look-up
               on the same number of states, rk_symball_depth (k_sb_depth: load, canonical form, probe -- the probe launch of a
               search, k_ss_probe, is that plus the fan-out move, and cannot be launched alone), and the ratio of the two rates.
  searches     optimal length 16 and 18 (starts selected as benchmarks/symball_search.py selects them): the unchanged
               DeviceSymBallSearch against deepen=8 with the pool held one level short -- capacity = max_capacity = the own levels
               that were complete plus half of the next, so the newest complete level is one earlier and two rounds are needed;
               equal lengths asserted.  Then prefixes of 22..28 moves of seeded scrambles with deepen=8, the pool at --far-capacity
               states and a time limit of --time-limit seconds each, until a start 20 quarter turns from solved is met: the
               length found, or not reached.
  batches      DeviceSymBall.solve_beyond(extra=3) on --batch seeded scrambles of 11, 12 and 13 moves: states per second and the
               share answered by the ball and by rounds 1, 2 and 3.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import _ffi, cube, gpu  # noqa: E402
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch  # noqa: E402
from benchmarks.bibfs import pick_starts, scramble_prefixes, solves  # noqa: E402
from benchmarks.symball_search import Selector  # noqa: E402

LEVELS = DeviceGoalBall.LEVELS                  # states at distance 0..8 of ANY state: the graph looks the same from every vertex


def scrambles(n: int, moves: int, seed: int) -> torch.Tensor:
	"""(n, 20) int8 on the device: `moves` seeded random quarter turns from solved."""
	g = torch.Generator(device="cpu").manual_seed(seed)
	states = torch.from_numpy(np.repeat(np.asarray(cube.cube._solved2024, np.int8)[None], n, axis=0)).to(gpu)
	for _ in range(moves):
		a = torch.randint(0, 12, (n,), generator=g, dtype=torch.uint8).to(gpu)
		_ffi.check(_ffi.lib().rk_multi_rotate(_ffi.REPR_2024, states.data_ptr(), a.data_ptr(), states.data_ptr(), n, _ffi.stream_ptr()))
	return states


def event_seconds(launch) -> float:
	t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	t0.record()
	launch()
	t1.record()
	torch.cuda.synchronize()
	return t0.elapsed_time(t1) / 1e3


def probe_rate(ball: DeviceSymBall) -> dict:
	lib, cap, extra = _ffi.lib(), int(_ffi.lib().rk_sdeepen_max_probes()), 4
	words = 12 * 11 ** (extra - 1)
	n = cap // words
	states = scrambles(n, 40, 1)
	best = torch.full((n,), -1, dtype=torch.int32, device=gpu)
	deepen = lambda cnt: _ffi.check(lib.rk_sdeepen(ball._h, states.data_ptr(), None, cnt, extra, 0, words, best.data_ptr(), _ffi.stream_ptr()))
	deepen(64)                                               # loads the kernel
	s_new = min(event_seconds(lambda: deepen(n)) for _ in range(2))
	hits = int((best != -1).sum())
	m = 1 << 24                                              # the parent commit's look-up, a wave per state
	q = scrambles(m, 40, 2)
	out = torch.empty(m, dtype=torch.int32, device=gpu)
	depth = lambda: _ffi.check(lib.rk_symball_depth(ball._h, q.data_ptr(), m, out.data_ptr(), _ffi.stream_ptr()))
	depth()
	s_old = min(event_seconds(depth) for _ in range(2))
	return {"extra": extra, "states": n, "words_per_state": words, "probes": n * words, "cap": cap, "hits": hits, "launch_s": round(s_new, 4),
	        "probes_per_s": round(n * words / s_new), "depth_states": m, "depth_launch_s": round(s_old, 5), "depth_probes_per_s": round(m / s_old),
	        "ratio_deepen_over_depth": round((n * words / s_new) / (m / s_old), 3)}


def timed_search(agent, start, **limits):
	t0 = time.perf_counter()
	ok = agent.search(start, **limits)
	return ok, time.perf_counter() - t0


def searches(ball: DeviceSymBall, args) -> list:
	rows = []
	sym = DeviceSymBallSearch(ball, pops=args.pops)
	starts = pick_starts(Selector(sym, args.select_states), args.lengths, args.seed, args.time_limit)
	for L in args.lengths:
		seed, k, start = starts[L]
		sym.search(start)                                    # warm-up: grows the pool
		ok, s_pool = timed_search(sym, start)
		assert ok and len(sym.action_queue) == L and solves(start, sym.action_queue)
		short = sum(LEVELS[:sym.depth]) + LEVELS[sym.depth] // 2      # levels 0 .. depth - 1 and half of level `depth`
		deep = DeviceSymBallSearch(ball, pops=args.pops, capacity=short, max_capacity=short, deepen=8)
		deep.search(start)
		ok, s_deep = timed_search(deep, start)
		assert ok and len(deep.action_queue) == L and solves(start, deep.action_queue), (L, len(deep.action_queue))
		rows.append({"length": L, "seed": seed, "scramble_moves": k, "pool_ms": round(1e3 * s_pool, 3), "pool_states": len(sym), "pool_levels": sym.depth,
		             "deepen_ms": round(1e3 * s_deep, 3), "deepen_capacity": short, "deepen_states": len(deep), "deepen_levels": deep.depth,
		             "deepened": deep.deepened, "probes": deep.probes, "ratio_deepen_over_pool_ms": round(s_deep / s_pool, 3), "equal_lengths": True})
		print(json.dumps(rows[-1]), flush=True)
		del deep
	# beyond the pool: prefixes of 22 .. 28 moves of seeded scrambles, seed after seed, until one lies 20 quarter turns from solved
	# (a seed's later prefixes are left out once one is that far or not reached) or --far-seconds are spent
	far = DeviceSymBallSearch(ball, pops=args.pops, capacity=args.far_capacity, max_capacity=args.far_capacity, deepen=8)
	spent, seen = 0.0, set()
	for seed in range(args.seed, args.seed + 16):
		for k, start in enumerate(scramble_prefixes(seed), 1):
			if k < 22 or k > 28:
				continue
			ok, s = timed_search(far, start, time_limit=args.time_limit)
			spent += s
			length = len(far.action_queue) if ok else None
			if ok and far.deepened == 0 and length in seen:
				continue                                         # (the pool sufficed, as for a start already listed)
			seen.add(length)
			rows.append({"scramble_moves": k, "seed": seed, "time_limit_s": args.time_limit, "reached": bool(ok), "length": length,
			             "solves": bool(ok and solves(start, far.action_queue)), "seconds": round(s, 3), "pool_states": len(far), "pool_levels": far.depth,
			             "deepened": far.deepened, "probes": far.probes, "capacity": args.far_capacity})
			print(json.dumps(rows[-1]), flush=True)
			if not ok or length >= 20:
				break
		if 20 in seen or spent > args.far_seconds:
			break
	return rows


def batches(ball: DeviceSymBall, args) -> list:
	rows = []
	for moves in (11, 12, 13):
		states = scrambles(args.batch, moves, 100 + moves).cpu().numpy()
		ball.solve_beyond(states[:1024], 3)
		t0 = time.perf_counter()
		lengths, _ = ball.solve_beyond(states, 3)
		s = time.perf_counter() - t0
		share = {"ball": round(float(((lengths >= 0) & (lengths <= ball.radius)).mean()), 5)}
		share.update({f"round_{e}": round(float((lengths == ball.radius + e).mean()), 5) for e in (1, 2, 3)})
		rows.append({"scramble_moves": moves, "states": args.batch, "seconds": round(s, 3), "states_per_s": round(args.batch / s),
		             "unanswered": int((lengths < 0).sum()), "share": share})
		print(json.dumps(rows[-1]), flush=True)
	return rows


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--radius", type=int, default=10)
	ap.add_argument("--pops", type=int, default=16_384)
	ap.add_argument("--lengths", type=int, nargs="+", default=[16, 18])
	ap.add_argument("--seed", type=int, default=0)
	ap.add_argument("--select-states", type=int, default=80_000_000)
	ap.add_argument("--far-capacity", type=int, default=20_000_000)
	ap.add_argument("--far-seconds", type=float, default=360.0)
	ap.add_argument("--batch", type=int, default=1_000_000)
	ap.add_argument("--time-limit", type=float, default=120.0)
	ap.add_argument("--skip", nargs="*", default=[], choices=["rate", "searches", "batches"])
	ap.add_argument("--out", default=os.path.join("profiles", "r17_symball_deepen.json"))
	args = ap.parse_args()
	cube.set_is2024(True)
	t0 = time.perf_counter()
	ball = DeviceSymBall(args.radius, pops=args.pops).build()
	doc = {"device": torch.cuda.get_device_name(0), "radius": args.radius, "orbits": len(ball), "build_s": round(time.perf_counter() - t0, 3), "pops": args.pops}
	print(json.dumps(doc), flush=True)
	def save():
		with open(args.out, "w") as f:                       # after every part: a later part that runs out of time loses nothing
			json.dump(doc, f, indent=1)
			f.write("\n")

	if "rate" not in args.skip:
		doc["probe_rate"] = probe_rate(ball)
		print(json.dumps(doc["probe_rate"]), flush=True)
		save()
	if "batches" not in args.skip:
		doc["batches"] = batches(ball, args)
		save()
	if "searches" not in args.skip:
		doc["searches"] = searches(ball, args)
		save()


if __name__ == "__main__":
	main()
