"""
Pattern databases on one MI355X (engine rk_pdb_*, `DevicePatternDB`), everything in one process:

    python benchmarks/pattern_db.py [--rows 1048576 16777216] [--repeats 5] [--out profiles/r25_pdb.json]

  * build time by the wall clock (the build synchronises) for the cross, all eight corners, six edges and seven edges, with the
    level sizes;
  * rk_pdb_depth and rk_pdb_solve of the cross and of the corners on seeded 40-move scrambles: device events around one launch, best
    of `repeats` after a warm-up launch; states/s; the share of the 8 TB/s HBM peak by this traffic model per query: 20 B of the row
    read, 4 B written, one 64-byte line of the table (solve is given the same model: its further lines and its action row are not
    counted, so its share is a lower bound of what it moves); and the ratio of its time to the unchanged rk_symball_depth (radius 6)
    and rk_group_legal on the same rows in the same run;
  * the histogram of `lower_bound` over the corners and two disjoint six-edge sets on those scrambles.
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
from librubiks_amd.solving.agents import DevicePatternDB, DeviceSymBall  # noqa: E402

HBM_PEAK = 8.0e12
BYTES_PER_QUERY = 20 + 4 + 64


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


def timed_build(name: str, db: DevicePatternDB) -> dict:
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	db.build()
	torch.cuda.synchronize()
	row = {"pattern": name, "corners": list(db.corner_cubies), "edges": list(db.edge_cubies), "entries": db.size,
	       "build_wall_s": round(time.perf_counter() - t0, 4), "levels": db.levels, "level_sizes": db.level_sizes.tolist()}
	print(json.dumps(row))
	return row


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1 << 24])
	ap.add_argument("--repeats", type=int, default=5)
	ap.add_argument("--out", default=os.path.join("profiles", "r25_pdb.json"))
	args = ap.parse_args()
	_ffi.require_gpu()
	lib = _ffi.lib()
	doc = {"benchmark": "benchmarks/pattern_db.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK,
	       "traffic_model": "per query 20 B read + 4 B written + one 64-byte line of the table", "builds": [], "queries": [], "lower_bound": []}
	DevicePatternDB(corners=(0,)).build()                                # the first launch of every kernel: code objects loaded
	dbs = {"cross": DevicePatternDB.cross("D"), "corners": DevicePatternDB.corners(), "six edges 0..5": DevicePatternDB(edges=range(6)),
	       "six edges 6..11": DevicePatternDB(edges=range(6, 12)), "seven edges 0..6": DevicePatternDB(edges=range(7))}
	for name, db in dbs.items():
		doc["builds"].append(timed_build(name, db))
	dbs.pop("seven edges 0..6")._free()                                  # 511 MB given back before the query buffers are made
	ball = DeviceSymBall(6).build()
	for n in args.rows:
		s = scrambles(n, 40, 2501)
		st, S = _ffi.stream_ptr(), s.data_ptr()
		depth = torch.empty(n, dtype=torch.int32, device="cuda")
		flags = torch.empty(n, dtype=torch.uint8, device="cuda")
		err = torch.zeros(1, dtype=torch.int32, device="cuda")
		yards = {"rk_symball_depth": best_ms(lambda: _ffi.check(lib.rk_symball_depth(ball._h, S, n, depth.data_ptr(), st)), args.repeats),
		         "rk_group_legal": best_ms(lambda: _ffi.check(lib.rk_group_legal(S, n, flags.data_ptr(), None, st)), args.repeats)}
		for name, ms in yards.items():
			row = {"entry": name, "rows": n, "ms": round(ms, 4), "rows_per_s": round(n / (ms * 1e-3))}
			doc["queries"].append(row)
			print(json.dumps(row))
		for name in ("cross", "corners"):
			db = dbs[name]
			actions = torch.empty((n, db.max_depth), dtype=torch.int8, device="cuda")
			entries = (("rk_pdb_depth", lambda: _ffi.check(lib.rk_pdb_depth(db._h, S, n, depth.data_ptr(), st))),
			           ("rk_pdb_solve", lambda: _ffi.check(lib.rk_pdb_solve(db._h, S, n, depth.data_ptr(), actions.data_ptr(), err.data_ptr(), st))))
			for entry, launch in entries:
				ms = best_ms(launch, args.repeats)
				row = {"entry": entry, "pattern": name, "rows": n, "ms": round(ms, 4), "rows_per_s": round(n / (ms * 1e-3)),
				       "share_of_hbm_peak": round(n * BYTES_PER_QUERY / (ms * 1e-3) / HBM_PEAK, 4),
				       "time_over_symball_depth": round(ms / yards["rk_symball_depth"], 4), "time_over_group_legal": round(ms / yards["rk_group_legal"], 3)}
				doc["queries"].append(row)
				print(json.dumps(row))
			assert int(err.item()) == 0
			del actions
		low = DevicePatternDB.lower_bound(s, [dbs["corners"], dbs["six edges 0..5"], dbs["six edges 6..11"]])
		hist = torch.bincount(low.to(torch.int64)).tolist()
		row = {"rows": n, "databases": ["corners", "six edges 0..5", "six edges 6..11"], "histogram": hist,
		       "mean": round(float(low.double().mean()), 4)}
		doc["lower_bound"].append(row)
		print(json.dumps(row))
		del s, depth, flags
	os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
	with open(args.out, "w") as f:
		json.dump(doc, f, indent=1)
		f.write("\n")
	print("wrote", args.out)


if __name__ == "__main__":
	main()
