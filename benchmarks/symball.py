"""
The symmetry-reduced goal ball on one MI355X: DeviceSymBall (engine rk_symball_*) beside the plain DeviceGoalBall (engine
rk_ball_*), and canonicalisation alone (rk_sym_canonical), everything in one process.

    python benchmarks/symball.py [--radii 8 9 10] [--plain-radius 8] [--queries 1000000 16000000] [--out profiles/r13_symball.json]

  build      per radius: seconds for a fresh DeviceSymBall (allocation, the clearing of the table and the level checks included; a
             radius-1 ball is built first so that the kernels are loaded), orbits stored, orbits per level, the orbit sizes of
             every level added up (`states_covered`; equal to the plain ball's level sizes through level 8, or the row says so),
             capacity, table slots and bytes (20 per pool row + 4 per table slot) -- and the plain ball of --plain-radius the same
             way (20 + 4 + 1 per pool row + 4 per table slot).  Every row says which engine it is.
  depth      n queries through the C entries on device tensors, timed with device events (one warm-up, best of 5), on the plain
             ball and on every sym ball that was built: `inside` = drawn uniformly from the PLAIN ball's nodes (every one lies in
             every ball here), `outside` = 30 random moves from solved.
  canonical  rk_sym_canonical alone on the `outside` states: states per second, and the share of the 8 TB/s HBM peak that its
             20 bytes in + 22 bytes out per state amount to (it is bound by LDS reads and the wave reduction, not by HBM).
A radius whose build fails (no device memory, capacity) is recorded with its error and skipped.
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
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall  # noqa: E402
from benchmarks.ball import device_ms  # noqa: E402

HBM_PEAK = 8.0e12


def timed_build(ball):
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	ball.build()
	torch.cuda.synchronize()
	return time.perf_counter() - t0


def sym_row(radius: int, pops: int):
	ball = DeviceSymBall(radius, pops=pops)
	try:
		dt = timed_build(ball)
	except _ffi.RubiksHipError as e:
		return None, {"engine": "rk_symball (DeviceSymBall)", "radius": radius, "pops": pops, "error": str(e)}
	status = (C.c_longlong * 32)()
	_ffi.check(_ffi.lib().rk_symball_status(ball._h, status))
	covered = ball.states_covered.tolist()
	known = list(DeviceSymBall.LEVELS[:radius + 1])
	n = len(ball)
	return ball, {"engine": "rk_symball (DeviceSymBall)", "radius": radius, "pops": pops, "orbits": n,
	              "orbits_per_level": np.diff(ball.level_start).tolist(), "states_covered": covered,
	              "states_covered_total": int(sum(covered)), "covered_equals_known_levels_0_to_8": covered[:len(known)] == known,
	              "capacity": int(status[4]), "table_slots": int(status[5]), "bytes": 20 * (int(status[4]) + 1) + 4 * int(status[5]),
	              "bytes_per_orbit": round((20 * (int(status[4]) + 1) + 4 * int(status[5])) / n, 2),
	              "build_s": round(dt, 4), "iterations": ball.iterations, "orbits_per_s": round(n / dt),
	              "states_covered_per_s": round(sum(covered) / dt)}


def plain_row(radius: int, pops: int):
	ball = DeviceGoalBall(radius, pops=pops)
	dt = timed_build(ball)
	n = len(ball)
	slots = 1 << (2 * n + 2 - 1).bit_length()
	return ball, {"engine": "rk_ball (DeviceGoalBall)", "radius": radius, "pops": pops, "states": n, "table_slots": slots,
	              "bytes": 25 * (n + 1) + 4 * slots, "bytes_per_state": round((25 * (n + 1) + 4 * slots) / n, 2),
	              "build_s": round(dt, 4), "iterations": ball.iterations, "states_per_s": round(n / dt)}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--radii", type=int, nargs="+", default=[8, 9, 10])
	ap.add_argument("--plain-radius", type=int, default=8)
	ap.add_argument("--queries", type=int, nargs="+", default=[1_000_000, 16_000_000])
	ap.add_argument("--pops", type=int, default=16_384)
	ap.add_argument("--seed", type=int, default=0)
	ap.add_argument("--out", default=os.path.join("profiles", "r13_symball.json"))
	args = ap.parse_args()
	_ffi.require_gpu()
	lib = _ffi.lib()
	DeviceSymBall(1, pops=args.pops).build()                   # loads the kernels
	DeviceGoalBall(1, pops=args.pops).build()
	result = {"device": torch.cuda.get_device_name(0), "build": [], "depth": [], "canonical": []}

	def save():
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			json.dump(result, f, indent=1)

	plain, row = plain_row(args.plain_radius, args.pops)
	result["build"].append(row)
	print(json.dumps(row), flush=True)
	n_plain = len(plain)
	pool = np.zeros((n_plain, 20), np.int8)
	_ffi.check(lib.rk_ball_export(plain._h, 1, n_plain, pool.ctypes.data, None, None, _ffi.stream_ptr()))
	rng = np.random.RandomState(args.seed)
	batches = {}
	for n in args.queries:
		inside = torch.from_numpy(pool[rng.randint(0, n_plain, n)]).to(gpu)
		outside = torch.from_numpy(cube.repeat_state(cube.get_solved(), n)).to(gpu)
		g = torch.Generator(device=gpu).manual_seed(args.seed)
		for _ in range(30):
			outside = cube.device.multi_rotate(outside, torch.randint(0, 12, (n,), device=gpu, generator=g, dtype=torch.uint8))
		batches[n] = {"inside": inside, "outside": outside}
	del pool

	def depth_rows(engine, entry, handle, radius):
		for n, parts in batches.items():
			out = torch.empty(n, dtype=torch.int32, device=gpu)
			for name, q in parts.items():
				stream = _ffi.stream_ptr()
				ms = device_ms(lambda: _ffi.check(entry(handle, q.data_ptr(), n, out.data_ptr(), stream)))
				row = {"engine": engine, "radius": radius, "queries": n, "from": name, "found": int((out >= 0).sum()),
				       "depth_ms": round(ms, 4), "queries_per_s": round(n / ms * 1e3)}
				result["depth"].append(row)
				print(json.dumps(row), flush=True)

	depth_rows("rk_ball (DeviceGoalBall)", lib.rk_ball_depth, plain._h, args.plain_radius)
	del plain
	torch.cuda.empty_cache()
	save()
	for n, parts in batches.items():
		q = parts["outside"]
		rep = torch.empty((n, 20), dtype=torch.int8, device=gpu)
		sym = torch.empty(n, dtype=torch.uint8, device=gpu)
		orbit = torch.empty(n, dtype=torch.uint8, device=gpu)
		stream = _ffi.stream_ptr()
		ms = device_ms(lambda: _ffi.check(lib.rk_sym_canonical(q.data_ptr(), n, rep.data_ptr(), sym.data_ptr(), orbit.data_ptr(), stream)))
		row = {"engine": "rk_sym_canonical", "states": n, "ms": round(ms, 4), "states_per_s": round(n / ms * 1e3),
		       "bytes_per_state": 42, "hbm_fraction": round(42 * n / (ms * 1e-3) / HBM_PEAK, 5),
		       "full_orbits": int((orbit == 48).sum())}
		result["canonical"].append(row)
		print(json.dumps(row), flush=True)
		del rep, sym, orbit
	save()
	for radius in args.radii:
		ball, row = sym_row(radius, args.pops)
		result["build"].append(row)
		print(json.dumps(row), flush=True)
		save()
		if ball is None:
			continue
		depth_rows("rk_symball (DeviceSymBall)", lib.rk_symball_depth, ball._h, radius)
		del ball
		torch.cuda.empty_cache()
		save()
	print(f"wrote {args.out}")


if __name__ == "__main__":
	main()
