"""
Shortening action queues against the symmetry ball on one MI355X: DeviceSymBall.shorten (engine rk_sshorten) beside
DeviceGoalBall.shorten (rk_bshorten), everything in one process.

    python benchmarks/symball_shorten.py [--paths 10000] [--shapes 30:200 20:50] [--out profiles/r15_symball_shorten.json]

  input     benchmarks/ball_shorten.py's: per shape depth:L, seeded scrambles of `depth` random moves, each inflated to about L moves
            by seeded detours that leave its effect as it was.
  cases     DeviceGoalBall(8) at window 8, DeviceSymBall(8) at window 8, DeviceSymBall(10) at windows 10, 12 and None (every window).
  one pass  the C entry on device tensors, cut into calls as the method cuts them (shorten_scratch_bytes), timed with device events
            (one warm-up, best of --repeats): pairs = the windows (i, j) of the batch, min(W, L - i) per start i; pairs_per_s.
  split     the device time of the three kernels of one pass (windows, dp, emit) from the profiler's kernel records, summed by name;
            null when the profiler gives none.
  lengths   the mean length before, after one pass and at the fixed point (the method, by the wall clock, with its passes).
  resident  the device memory a built ball keeps: free memory before the build minus free memory after it.
  check     the radius-8 lengths of the two balls after one pass are equal queue for queue (asserted: they follow from d(i, j)
            alone).  The fixed points of a narrow window start their later passes from words that may differ, so they are compared
            and the queues whose lengths differ are counted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import _ffi, gpu  # noqa: E402
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall  # noqa: E402
from benchmarks.ball_shorten import inflated, wall  # noqa: E402


def built(make):
	"""(the ball, built; the bytes it keeps resident)"""
	torch.cuda.synchronize()
	torch.cuda.empty_cache()
	free0 = torch.cuda.mem_get_info()[0]
	ball = make().build()
	torch.cuda.synchronize()
	return ball, free0 - torch.cuda.mem_get_info()[0]


def window_pairs(L: int, window) -> int:
	"""The windows (i, j) of a queue of L moves with j - i <= window: min(window, L - i) per start i."""
	W = L if window is None else min(window, L)
	return W * (L - W) + W * (W + 1) // 2


def prepared(ball, words, window):
	"""One pass over `words` through the C entry, in the method's chunks: a callable that launches it, and the calls' error words."""
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	entry = getattr(lib, ball._shorten_entry)
	longest = max(len(w) for w in words)
	w = longest if window is None else min(window, longest)
	step = max(1, ball.shorten_scratch_bytes // (longest * w + 2 * (longest + 1)))
	calls = []
	for at in range(0, len(words), step):
		part = words[at:at + step]
		n, max_len = len(part), max(len(x) for x in part)
		wc = max_len if window is None else min(window, max_len)
		acts = np.full((n, max_len), -1, np.int8)
		for r, x in enumerate(part):
			acts[r, :len(x)] = x
		need = lib.rk_bshorten_scratch_bytes(n, max_len, wc)
		t = dict(acts=torch.from_numpy(acts).to(gpu), lens=torch.tensor([len(x) for x in part], dtype=torch.int32, device=gpu),
		         out=torch.empty((n, max_len), dtype=torch.int8, device=gpu), out_len=torch.empty(n, dtype=torch.int32, device=gpu),
		         err=torch.empty(1, dtype=torch.int32, device=gpu))
		calls.append((t, n, max_len, wc, need))
	scratch = torch.empty(max(c[4] for c in calls), dtype=torch.uint8, device=gpu)

	def run():
		for t, n, max_len, wc, need in calls:
			_ffi.check(entry(ball._h, t["acts"].data_ptr(), t["lens"].data_ptr(), n, max_len, wc, t["out"].data_ptr(), t["out_len"].data_ptr(),
			                 t["err"].data_ptr(), scratch.data_ptr(), need, stream))
	return run, calls


def device_pass_ms(run, repeats: int) -> float:
	run()
	torch.cuda.synchronize()
	best = None
	for _ in range(repeats):
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		run()
		b.record()
		torch.cuda.synchronize()
		ms = a.elapsed_time(b)
		best = ms if best is None else min(best, ms)
	return best


def kernel_split_ms(run):
	"""{windows, dp, emit: ms} of one pass, from the profiler's kernel records; None when it gives none."""
	try:
		from torch.profiler import ProfilerActivity, profile
		with profile(activities=[ProfilerActivity.CUDA]) as prof:
			run()
			torch.cuda.synchronize()
		split = {"windows": 0.0, "dp": 0.0, "emit": 0.0}
		seen = 0
		for ev in prof.events():
			for key in split:
				if f"_{key}" in ev.name and ("k_shorten_" in ev.name or "k_ss_" in ev.name):
					split[key] += (ev.device_time if hasattr(ev, "device_time") else ev.cuda_time) / 1e3
					seen += 1
		return {k: round(v, 4) for k, v in split.items()} if seen else None
	except Exception:                                                    # no profiler in this build: the split is left out
		return None


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--paths", type=int, default=10_000)
	ap.add_argument("--shapes", nargs="+", default=["30:200", "20:50"])
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--radii", type=int, nargs=2, default=[8, 10], help="the radius both balls are compared at, and the deep symmetry ball's")
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	r_both, r_deep = args.radii
	plain, plain_bytes = built(lambda: DeviceGoalBall(r_both))
	sym, sym_bytes = built(lambda: DeviceSymBall(r_both))
	t0 = time.perf_counter()
	deep, deep_bytes = built(lambda: DeviceSymBall(r_deep))
	deep_build_s = time.perf_counter() - t0
	cases = [("DeviceGoalBall", plain, r_both, 8, plain_bytes), ("DeviceSymBall", sym, r_both, 8, sym_bytes),
	         ("DeviceSymBall", deep, r_deep, 10, deep_bytes), ("DeviceSymBall", deep, r_deep, 12, deep_bytes),
	         ("DeviceSymBall", deep, r_deep, None, deep_bytes)]
	doc = {"benchmark": "benchmarks/symball_shorten.py", "device": torch.cuda.get_device_name(0), "paths": args.paths, "repeats": args.repeats,
	       "scratch_cap_bytes": sym.shorten_scratch_bytes, "orbits": {str(r_both): len(sym), str(r_deep): len(deep)},
	       "deep_build_wall_s": round(deep_build_s, 3), "rows": [], "radius_%d_window_8" % r_both: []}
	for ball in (plain, sym, deep):
		ball.shorten([[0, 1, 0, 1]])                                     # loads the kernels
	for shape in args.shapes:
		depth, target = (int(x) for x in shape.split(":"))
		rng = np.random.RandomState(args.seed + depth)
		words = [inflated(rng, depth, target) for _ in range(args.paths)]
		lengths = {}
		for name, ball, radius, window, resident in cases:
			pairs = sum(window_pairs(len(w), window) for w in words)
			run, calls = prepared(ball, words, window)
			ms = device_pass_ms(run, args.repeats)
			assert all(int(c[0]["err"].item()) == 0 for c in calls)
			split = kernel_split_ms(run)
			one, one_s = wall(lambda: ball.shorten(words, window=window, passes=1))
			full, full_s = wall(lambda: ball.shorten(words, window=window))
			lengths[(name, radius, window)] = ([len(x) for x in one], [len(x) for x in full])
			row = {"ball": name, "radius": radius, "window": window, "scramble_depth": depth, "target_length": target, "paths": args.paths,
			       "pairs": pairs, "calls_per_pass": len(calls), "pass_device_ms": round(ms, 4), "pairs_per_s": round(pairs / ms * 1e3),
			       "kernel_ms": split, "pass_method_wall_s": round(one_s, 4), "fixed_point_wall_s": round(full_s, 4),
			       "mean_length_before": round(float(np.mean([len(w) for w in words])), 2),
			       "mean_length_after_one_pass": round(float(np.mean([len(w) for w in one])), 2),
			       "mean_length_after": round(float(np.mean([len(w) for w in full])), 2), "resident_bytes": int(resident)}
			doc["rows"].append(row)
			print(json.dumps(row), flush=True)
		# One pass: the lengths follow from d(i, j) alone, which the two balls share -- equal queue for queue.  Further passes start
		# from words that may differ where a window has several shortest words, so with a narrow window the two fixed points need
		# not be equal queue for queue (both are locally optimal): the queues that differ are counted, not refused.
		(p_one, p_full), (s_one, s_full) = lengths[("DeviceGoalBall", r_both, 8)], lengths[("DeviceSymBall", r_both, 8)]
		assert p_one == s_one
		doc["radius_%d_window_8" % r_both].append({"scramble_depth": depth, "one_pass_lengths_equal": True,
		                                           "fixed_point_queues_that_differ": sum(a != b for a, b in zip(p_full, s_full)),
		                                           "fixed_point_moves_in_all": [sum(p_full), sum(s_full)]})
		print(json.dumps(doc["radius_%d_window_8" % r_both][-1]), flush=True)
	if args.out:
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")


if __name__ == "__main__":
	main()
