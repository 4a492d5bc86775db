"""
The subgroup chain on one MI355X (engine rk_chain_*, `DeviceChainSolver`), everything in one process:

    python benchmarks/chain_solve.py [--rows 1048576 16777216] [--repeats 5] [--shorten-rows 10000] [--out profiles/r27_chain.json]

  * the wall time of making the solver (the four tables are built on the host and uploaded), the coset counts and stage depths;
  * rk_chain_solve on seeded 40-move scrambles beside the unchanged rk_pdb_solve of the all-corners database on the same rows --
    both are dependent byte-read descents --: device events around one launch, best of `repeats` after a warm-up launch;
    states/s and the ratio of the two times;
  * the mean and the greatest length, overall and per stage;
  * the mean length of `shorten-rows` of the solutions after one pass and after the converged passes of DeviceSymBall(8).shorten.
Nothing here asserts a rate.
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
from librubiks_amd.solving.agents import DeviceChainSolver, DevicePatternDB, DeviceSymBall  # noqa: E402


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


def scrambles(n: int, depth: int, seed: int) -> torch.Tensor:
	"""n states `depth` seeded random moves from solved, moved on the device"""
	g = torch.Generator(device="cuda").manual_seed(seed)
	s = torch.from_numpy(np.repeat(cube.get_solved()[None], n, axis=0)).cuda()
	for _ in range(depth):
		cube.device.multi_rotate(s, torch.randint(0, 12, (n,), generator=g, device="cuda", dtype=torch.uint8), out=s)
	return s


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1 << 24])
	ap.add_argument("--repeats", type=int, default=5)
	ap.add_argument("--shorten-rows", type=int, default=10_000)
	ap.add_argument("--out", default=os.path.join("profiles", "r27_chain.json"))
	args = ap.parse_args()
	_ffi.require_gpu()
	lib = _ffi.lib()
	DeviceChainSolver()                                                  # the first use: code objects loaded
	t0 = time.perf_counter()
	solver = DeviceChainSolver()
	torch.cuda.synchronize()
	doc = {"benchmark": "benchmarks/chain_solve.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
	       "create_wall_s": round(time.perf_counter() - t0, 4), "coset_counts": list(solver.coset_counts),
	       "stage_depths": list(solver.stage_depths), "max_length": solver.max_length, "queries": [], "lengths": [], "shorten": None}
	print(json.dumps({k: doc[k] for k in ("create_wall_s", "coset_counts", "stage_depths", "max_length")}))
	corners = DevicePatternDB.corners().build()
	for n in args.rows:
		s = scrambles(n, 40, 2701)
		st, S = _ffi.stream_ptr(), s.data_ptr()
		lengths = torch.empty(n, dtype=torch.int32, device="cuda")
		stages = torch.empty((n, 4), dtype=torch.int32, device="cuda")
		err = torch.zeros(1, dtype=torch.int32, device="cuda")
		actions = torch.empty((n, max(solver.max_length, corners.max_depth)), dtype=torch.int8, device="cuda")
		pdb_ms = best_ms(lambda: _ffi.check(lib.rk_pdb_solve(corners._h, S, n, lengths.data_ptr(), actions.data_ptr(), err.data_ptr(), st)), args.repeats)
		assert int(err.item()) == 0
		chain_ms = best_ms(lambda: _ffi.check(lib.rk_chain_solve(solver._h, S, n, lengths.data_ptr(), actions.data_ptr(), stages.data_ptr(),
		                                                         err.data_ptr(), st)), args.repeats)
		assert int(err.item()) == -1 and int(lengths.min()) >= 0
		for entry, ms in (("rk_pdb_solve (all corners)", pdb_ms), ("rk_chain_solve", chain_ms)):
			row = {"entry": entry, "rows": n, "ms": round(ms, 4), "rows_per_s": round(n / (ms * 1e-3)), "time_over_pdb_solve": round(ms / pdb_ms, 3)}
			doc["queries"].append(row)
			print(json.dumps(row))
		row = {"rows": n, "mean_length": round(float(lengths.double().mean()), 4), "max_length": int(lengths.max()),
		       "mean_stage_lengths": [round(float(v), 4) for v in stages.double().mean(dim=0)], "max_stage_lengths": stages.max(dim=0).values.tolist()}
		doc["lengths"].append(row)
		print(json.dumps(row))
		if doc["shorten"] is None and args.shorten_rows:
			k = min(args.shorten_rows, n)
			h_len, h_act = lengths[:k].cpu().numpy(), actions[:k, :solver.max_length].cpu().numpy()
			queues = [h_act[i, :h_len[i]] for i in range(k)]
			ball = DeviceSymBall(8).build()
			t0 = time.perf_counter()
			once = ball.shorten(queues, passes=1)
			t1 = time.perf_counter()
			done = ball.shorten(queues)
			t2 = time.perf_counter()
			doc["shorten"] = {"ball": "DeviceSymBall(8)", "queues": k, "mean_length": round(float(h_len.mean()), 4),
			                  "mean_after_one_pass": round(float(np.mean([len(q) for q in once])), 4), "one_pass_wall_s": round(t1 - t0, 3),
			                  "mean_converged": round(float(np.mean([len(q) for q in done])), 4), "max_converged": int(max(len(q) for q in done)),
			                  "converged_wall_s": round(t2 - t1, 3)}
			print(json.dumps(doc["shorten"]))
			del ball
		del s, lengths, stages, actions
	os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
	with open(args.out, "w") as f:
		json.dump(doc, f, indent=1)
		f.write("\n")
	print("wrote", args.out)


if __name__ == "__main__":
	main()
