"""
The cube group's entries on one MI355X: rk_group_apply / inverse / relative / legal beside rk_sym_conjugate -- the same 20 B in and
20 B out, a thread per state -- on the same seeded scramble rows in one process.

    python benchmarks/group.py [--rows 1048576 16777216] [--repeats 5] [--out profiles/r24_group.json]

Per entry and row count: device events around one launch, best of `repeats` after a warm-up launch; rows/s; the share of the 8 TB/s
HBM peak by this traffic model per row: every operand row read once (20 B; the second operand of apply / relative another 20 B, or
nothing when it is one row for all), the output written once (20 B; legal: 1 B of flags), tables and statistics not counted; and the
ratio to rk_sym_conjugate's time on those rows.  Nothing here asserts a rate.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import _ffi, cube  # noqa: E402

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
	ap.add_argument("--out", default=os.path.join("profiles", "r24_group.json"))
	args = ap.parse_args()
	_ffi.require_gpu()
	lib = _ffi.lib()
	doc = {"benchmark": "benchmarks/group.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK,
	       "traffic_model": "operand rows 20 B each (a one-for-all second operand: 0), output 20 B (legal: 1 B)", "rows": []}
	for n in args.rows:
		a, b = scrambles(n, 30, 2401), scrambles(n, 30, 2402)
		out = torch.empty((n, 20), dtype=torch.int8, device="cuda")
		flags = torch.empty(n, dtype=torch.uint8, device="cuda")
		stats = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")
		st = _ffi.stream_ptr()
		A, B, O = a.data_ptr(), b.data_ptr(), out.data_ptr()
		entries = (
			("rk_sym_conjugate", 40, lambda: _ffi.check(lib.rk_sym_conjugate(A, n, 17, O, st))),
			("rk_group_apply", 60, lambda: _ffi.check(lib.rk_group_apply(A, n, B, n, O, st))),
			("rk_group_apply (one effect)", 40, lambda: _ffi.check(lib.rk_group_apply(A, n, B, 1, O, st))),
			("rk_group_inverse", 40, lambda: _ffi.check(lib.rk_group_inverse(A, n, O, st))),
			("rk_group_relative", 60, lambda: _ffi.check(lib.rk_group_relative(A, n, B, n, O, st))),
			("rk_group_relative (one goal)", 40, lambda: _ffi.check(lib.rk_group_relative(A, n, B, 1, O, st))),
			("rk_group_legal", 21, lambda: _ffi.check(lib.rk_group_legal(A, n, flags.data_ptr(), stats.data_ptr(), st))),
		)
		yard = None
		for name, per_row, launch in entries:
			ms = best_ms(launch, args.repeats)
			yard = ms if yard is None else yard
			row = {"entry": name, "rows": n, "ms": round(ms, 4), "rows_per_s": round(n / (ms * 1e-3)), "bytes_per_row": per_row,
			       "share_of_hbm_peak": round(n * per_row / (ms * 1e-3) / HBM_PEAK, 4), "time_over_sym_conjugate": round(ms / yard, 3)}
			doc["rows"].append(row)
			print(json.dumps(row))
		assert stats.tolist()[0] == 0                                    # scrambles are legal
		del a, b, out, flags
	os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
	with open(args.out, "w") as f:
		json.dump(doc, f, indent=1)
		f.write("\n")
	print("wrote", args.out)


if __name__ == "__main__":
	main()
