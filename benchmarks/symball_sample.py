"""
Unranking the symmetry ball on one MI355X: DeviceSymBall.state_at / child_depths / adi.ball_traindata (engines
rk_symball_state_at, rk_symball_child_depths) beside the unchanged rk_symball_depth on the same states in the same process.

    python benchmarks/symball_sample.py [--radius 10] [--depths 6 8 10] [--ranks 16777216] [--repeats 5] [--rows 1048576]
                                        [--out profiles/r22_symball_sample.json]

  index        the orbit index's build: wall clock of the first state_at (one sample: four launches and one read for the index, then
               the sample), once per process, and the same call again beside it
  state_at     2^24 uniform ranks at each depth, device events around the launch, best of `repeats`: states/s, and the share of the
               8 TB/s HBM peak by this traffic model per sample: 4 B depth + 8 B rank in, 20 B state out, 256 B of orbit bytes,
               20 B of the representative and log2(tiles of the level) x 8 B of prefix words (upper bound: the first steps of the
               bisection hit the same few lines for every sample and come from cache)
  child_depths on those states: states/s; 20 B in, 13 B out, thirteen probes of (4 B table word + 20 B stored state) at least
  depth        the yardstick: rk_symball_depth on the same states, the same way; 20 B in, 4 B out, one probe
  traindata    adi.ball_traindata rows/s by the wall clock (host draws, sample, one-hot, targets, copies of the targets to the host)
Every row carries its ratio to `depth`.  Nothing here asserts a rate.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import _ffi, cube  # noqa: E402
from librubiks_amd.adi import ball_traindata  # noqa: E402
from librubiks_amd.solving.agents import DeviceSymBall  # noqa: E402

HBM_PEAK = 8.0e12


def best_ms(launch, repeats: int) -> float:
	start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	launch()                                                             # warm-up
	torch.cuda.synchronize()
	best = math.inf
	for _ in range(repeats):
		start.record()
		launch()
		stop.record()
		stop.synchronize()
		best = min(best, start.elapsed_time(stop))
	return best


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--radius", type=int, default=10)
	ap.add_argument("--depths", type=int, nargs="+", default=[6, 8, 10])
	ap.add_argument("--ranks", type=int, default=1 << 24)
	ap.add_argument("--repeats", type=int, default=5)
	ap.add_argument("--rows", type=int, default=1 << 20)
	ap.add_argument("--out", default=os.path.join("profiles", "r22_symball_sample.json"))
	args = ap.parse_args()
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	t0 = time.perf_counter()
	ball = DeviceSymBall(args.radius).build()
	torch.cuda.synchronize()
	build_s = time.perf_counter() - t0
	t0 = time.perf_counter()
	ball.state_at(0, [0])
	index_s = time.perf_counter() - t0
	t0 = time.perf_counter()
	ball.state_at(0, [0])
	one_sample_s = time.perf_counter() - t0
	doc = {"benchmark": "benchmarks/symball_sample.py", "device": torch.cuda.get_device_name(0), "radius": args.radius, "orbits": len(ball),
	       "states_covered": [int(c) for c in ball.states_covered], "ball_build_s": round(build_s, 4),
	       "index": {"build_s_first_call": round(index_s, 4), "same_call_again_s": round(one_sample_s, 5), "bytes": ball.index_bytes},
	       "ranks": args.ranks, "repeats": args.repeats, "rows": []}
	n = args.ranks
	rng = np.random.default_rng(22)
	err = torch.empty(1, dtype=torch.int32, device="cuda")
	for d in args.depths:
		if d > args.radius:
			continue
		covered = int(ball.states_covered[d])
		d_t = torch.full((n,), d, dtype=torch.int32, device="cuda")
		r_t = torch.from_numpy(rng.integers(0, covered, n, dtype=np.int64)).cuda()
		states = torch.empty((n, 20), dtype=torch.int8, device="cuda")
		depth32 = torch.empty(n, dtype=torch.int32, device="cuda")
		own = torch.empty(n, dtype=torch.int8, device="cuda")
		kids = torch.empty((n, 12), dtype=torch.int8, device="cuda")
		at_ms = best_ms(lambda: _ffi.check(lib.rk_symball_state_at(ball._h, d_t.data_ptr(), r_t.data_ptr(), n, states.data_ptr(), err.data_ptr(), stream)),
		                args.repeats)
		assert int(err.item()) == 0
		depth_ms = best_ms(lambda: _ffi.check(lib.rk_symball_depth(ball._h, states.data_ptr(), n, depth32.data_ptr(), stream)), args.repeats)
		assert bool((depth32 == d).all())
		kids_ms = best_ms(lambda: _ffi.check(lib.rk_symball_child_depths(ball._h, states.data_ptr(), n, own.data_ptr(), kids.data_ptr(), err.data_ptr(),
		                                                                   stream)), args.repeats)
		assert int(err.item()) == 0 and bool((own == d).all())
		level_tiles = max(1, (int(ball.level_start[d + 1]) - int(ball.level_start[d])) // 256)
		at_bytes = 4 + 8 + 20 + 256 + 20 + 8 * math.ceil(math.log2(level_tiles + 1))
		row = {"depth": d, "states_at_depth": covered,
		       "state_at": {"ms": round(at_ms, 4), "states_per_s": round(n / (at_ms * 1e-3)), "bytes_per_state_model": at_bytes,
		                    "hbm_fraction": round(at_bytes * n / (at_ms * 1e-3) / HBM_PEAK, 5), "ratio_to_depth": round(depth_ms / at_ms, 4)},
		       "child_depths": {"ms": round(kids_ms, 4), "states_per_s": round(n / (kids_ms * 1e-3)), "bytes_per_state_model": 33 + 13 * 24,
		                        "hbm_fraction": round((33 + 13 * 24) * n / (kids_ms * 1e-3) / HBM_PEAK, 5), "ratio_to_depth": round(depth_ms / kids_ms, 4)},
		       "depth": {"ms": round(depth_ms, 4), "states_per_s": round(n / (depth_ms * 1e-3)), "bytes_per_state_model": 48,
		                 "hbm_fraction": round(48 * n / (depth_ms * 1e-3) / HBM_PEAK, 5)}}
		doc["rows"].append(row)
		print(json.dumps(row))
	best = math.inf
	for _ in range(args.repeats):
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		ball_traindata(ball, args.rows, None, rng)
		torch.cuda.synchronize()
		best = min(best, time.perf_counter() - t0)
	doc["traindata"] = {"rows": args.rows, "depths": "uniform over the ball", "s": round(best, 5), "rows_per_s": round(args.rows / best)}
	print(json.dumps(doc["traindata"]))
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, "w") as f:
		json.dump(doc, f, indent=1)
	print("wrote", args.out, "| representation:", "20-byte" if cube.get_is2024() else "6x8x6")


if __name__ == "__main__":
	main()
