"""
Shortening action queues against the goal ball on one MI355X: DeviceGoalBall.shorten (engine rk_bshorten_*), everything in one process.

    python benchmarks/ball_shorten.py [--radius 8] [--paths 1000 10000] [--shapes 20:50 30:200] [--out profiles/r12_ball_shorten.json]

  input     per shape depth:L, seeded scrambles of `depth` random moves, each inflated to about L moves by seeded detours that leave
            its effect as it was: a random word of 2-6 moves followed by its inverse, inserted at a random place, or a move written
            as the three opposite turns.
  one pass  rk_bshorten on device tensors, cut into calls as the method cuts them (shorten_scratch_bytes), timed with device events
            (one warm-up, best of --repeats): pairs = the windows (i, j) of the batch, L (L + 1) / 2 per queue with the full window;
            pairs_per_s; and the method's own single pass by the wall clock (padding, copies and the host's loop included).
  traffic   benchmarks/ball.py's two models for one probe of a window, without the 20-byte query (the state is composed in
            registers) and with a one-byte answer: `requested` = 4 per probed table word + 20 per compared row + 1, `lines64` = 64
            per table word + 80 per compared row + 1; probes = 1 for a hit, 1 / (1 - load) for a miss, weighted by the share of the
            windows that the ball holds (measured on the comparison's sample).  hbm_fraction = lines64 bytes per second over 8 TB/s.
  fixed     the method to the fixed point by the wall clock: passes, mean length before and after.
  compare   the only way to the same window depths without the engine: the host advances every start of a window by one move per
            step with cube.multi_rotate, collects the states and asks DeviceGoalBall.depth -- on the first --compare-paths queues,
            by the wall clock, checked against the lengths a pass computes from them (the whole queue's window).  ratio = seconds
            per pair of that over seconds per pair of the method's single pass on the whole batch.
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
from librubiks_amd.solving.agents import DeviceGoalBall  # noqa: E402

HBM_PEAK = 8.0e12


def inflated(rng, depth: int, target: int) -> np.ndarray:
	word = [int(a) for a in rng.randint(0, 12, depth)]
	while len(word) < target:
		at = int(rng.randint(0, len(word) + 1))
		if rng.randint(0, 2) or not word:
			w = [int(a) for a in rng.randint(0, 12, int(rng.randint(2, 7)))]
			word[at:at] = w + [a ^ 1 for a in reversed(w)]           # cube.rev_action: the two turns of a face are a, a ^ 1
		else:
			at = min(at, len(word) - 1)
			word[at:at + 1] = [word[at] ^ 1] * 3
	return np.array(word, np.int64)


def device_pass_ms(ball, words, repeats: int) -> float:
	"""One pass over `words` with the full window through the C entry, in the method's chunks; the device's time alone."""
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	longest = max(len(w) for w in words)
	step = max(1, ball.shorten_scratch_bytes // (longest * longest + 2 * (longest + 1)))
	calls = []
	for at in range(0, len(words), step):
		part = words[at:at + step]
		n, max_len = len(part), max(len(w) for w in part)
		acts = np.full((n, max_len), -1, np.int8)
		for r, w in enumerate(part):
			acts[r, :len(w)] = w
		need = lib.rk_bshorten_scratch_bytes(n, max_len, max_len)
		t = dict(acts=torch.from_numpy(acts).to(gpu), lens=torch.tensor([len(w) for w in part], dtype=torch.int32, device=gpu),
		         out=torch.empty((n, max_len), dtype=torch.int8, device=gpu), out_len=torch.empty(n, dtype=torch.int32, device=gpu),
		         err=torch.empty(1, dtype=torch.int32, device=gpu))
		calls.append((t, n, max_len, need))
	scratch = torch.empty(max(c[3] for c in calls), dtype=torch.uint8, device=gpu)

	def run():
		for t, n, max_len, need in calls:
			_ffi.check(lib.rk_bshorten(ball._h, t["acts"].data_ptr(), t["lens"].data_ptr(), n, max_len, max_len, t["out"].data_ptr(),
			                           t["out_len"].data_ptr(), t["err"].data_ptr(), scratch.data_ptr(), need, stream))
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
	assert all(int(c[0]["err"].item()) == 0 for c in calls)
	return best, len(calls)


def wall(call):
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	out = call()
	torch.cuda.synchronize()
	return out, time.perf_counter() - t0


def window_depths_by_host(ball, words):
	"""d(i, j) of every window of every word, the way the public surface allowed before the engine: list of (L, L) arrays, row i,
	column j - i - 1, -9 where there is no window."""
	longest = max(len(w) for w in words)
	start_of = np.concatenate([[0], np.cumsum([len(w) for w in words])])
	owner = np.repeat(np.arange(len(words)), [len(w) for w in words])
	pos = np.concatenate([np.arange(len(w)) for w in words])                    # i of every start
	flat = np.concatenate(words)
	length = np.array([len(w) for w in words])[owner]
	states = cube.repeat_state(cube.get_solved(), len(flat))
	depths = [np.full((len(w), len(w)), -9, np.int64) for w in words]
	for k in range(1, longest + 1):
		live = np.nonzero(pos + k <= length)[0]
		act = flat[start_of[owner[live]] + pos[live] + k - 1]
		states[live] = cube.multi_rotate(states[live], act // 2, 1 - act % 2)
		d = ball.depth(states[live])
		for q in np.unique(owner[live]):
			sel = owner[live] == q
			depths[q][pos[live][sel], k - 1] = d[sel]
	return depths


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--radius", type=int, default=8)
	ap.add_argument("--paths", type=int, nargs="+", default=[1_000, 10_000])
	ap.add_argument("--shapes", nargs="+", default=["20:50", "30:200"])
	ap.add_argument("--compare-paths", type=int, default=100)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	ball = DeviceGoalBall(args.radius).build()
	n_ball = len(ball)
	load = n_ball / (1 << (2 * n_ball + 2 - 1).bit_length())
	doc = {"benchmark": "benchmarks/ball_shorten.py", "device": torch.cuda.get_device_name(0), "radius": args.radius,
	       "ball_states": n_ball, "table_load": round(load, 3), "repeats": args.repeats,
	       "scratch_cap_bytes": ball.shorten_scratch_bytes, "rows": []}
	ball.shorten([[0, 1, 0, 1]])                                 # loads the kernels
	for shape in args.shapes:
		depth, target = (int(x) for x in shape.split(":"))
		for n in args.paths:
			rng = np.random.RandomState(args.seed + depth)
			words = [inflated(rng, depth, target) for _ in range(n)]
			pairs = sum(len(w) * (len(w) + 1) // 2 for w in words)
			ms, calls = device_pass_ms(ball, words, args.repeats)
			one, one_s = wall(lambda: ball.shorten(words, passes=1))
			full, full_s = wall(lambda: ball.shorten(words))
			cur, passes = words, 0
			while True:                                                  # again one pass at a time, to count the passes
				new = ball.shorten(cur, passes=1)
				passes += 1
				if sum(map(len, new)) == sum(map(len, cur)):
					break
				cur = new
			assert all((x == y).all() for x, y in zip(full, new))
			# the comparison, on a sample
			m = min(args.compare_paths, n)
			sample = words[:m]
			sample_pairs = sum(len(w) * (len(w) + 1) // 2 for w in sample)
			depths, cmp_s = wall(lambda: window_depths_by_host(ball, sample))
			held = sum(int((d >= 0).sum()) for d in depths)
			whole = [int(d[0, len(w) - 1]) for d, w in zip(depths, sample)]      # the whole queue's window: -1 or the optimum
			got = [len(x) for x in one[:m]]
			assert all(g == w for g, w in zip(got, whole) if w >= 0)
			hit = held / sample_pairs
			probes = hit * 1.0 + (1.0 - hit) / (1.0 - load)
			compares = hit * 1.0 + (1.0 - hit) * (1.0 / (1.0 - load) - 1.0)
			req, lin = 4 * probes + 20 * compares + 1, 64 * probes + 80 * compares + 1
			row = {"scramble_depth": depth, "target_length": target, "paths": n, "pairs": pairs, "calls_per_pass": calls,
			       "pass_device_ms": round(ms, 4), "pairs_per_s": round(pairs / ms * 1e3),
			       "windows_held_share": round(hit, 4), "bytes_per_probe_requested": round(req, 1), "bytes_per_probe_lines64": round(lin, 1),
			       "hbm_fraction": round(lin * pairs / (ms * 1e-3) / HBM_PEAK, 4),
			       "pass_method_wall_s": round(one_s, 4), "pass_method_pairs_per_s": round(pairs / one_s),
			       "fixed_point_wall_s": round(full_s, 4), "passes": passes,
			       "mean_length_before": round(float(np.mean([len(w) for w in words])), 2),
			       "mean_length_after_one_pass": round(float(np.mean([len(w) for w in one])), 2),
			       "mean_length_after": round(float(np.mean([len(w) for w in full])), 2),
			       "compare_paths": m, "compare_pairs": sample_pairs, "compare_wall_s": round(cmp_s, 4),
			       "compare_pairs_per_s": round(sample_pairs / cmp_s),
			       "ratio_compare_over_method_per_pair": round((cmp_s / sample_pairs) / (one_s / pairs), 2)}
			doc["rows"].append(row)
			print(json.dumps(row), flush=True)
	if args.out:
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")


if __name__ == "__main__":
	main()
