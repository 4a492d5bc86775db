"""
The cap on the two-phase search's phase-2 bound on one MI355X (rk_twophase_solve_capped, `DeviceTwoPhaseSolver(phase2_cap=C)`),
everything in one process:

    python benchmarks/two_phase_cap.py [--sweep-rows 65536] [--big-rows 1048576] [--caps 8 10 12 14 16 18 20 24] [--out profiles/r32_two_phase_cap.json]

On the rows of benchmarks/two_phase.py (seeded 40-move scrambles): at `--sweep-rows` rows every cap and "none" at every
`--max-nodes`; at `--big-rows` rows "none" and the two best caps of the sweep (lowest mean length at the greatest budget) at the
least and the greatest budget.  A capped setting runs with tries = 2^31 - 1, "none" with tries = 8.  The columns are two_phase.py's
-- device events, the time as a ratio to the chain's on the same rows, mean and greatest length, mean phase lengths, the shares
of reasons 0 / 1 / 2, nodes per state and nodes/s -- and the mean phase-1 solutions found and phase-2 searches entered.  A call
longer than `--long-ms` is repeated `--long-repeats` times, not `--repeats`.  Then, on `--exact-rows` states at the exact depth 10,
the mean excess over that depth without a cap and with the best one.  What the cap buys is read against the "none" rows of the
SAME run.  The file is written after every setting.  Nothing here asserts a rate or a length.  Run it under a time limit
(`timeout -k 10 900 python benchmarks/two_phase_cap.py`): in profiles/r32_two_phase_cap.json a call takes up to 1.8 s at 64 K rows and
23 s at 1 M rows, and the whole run took 5.5 minutes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd import _ffi  # noqa: E402
from librubiks_amd.solving.agents import DeviceChainSolver, DeviceSymBall, DeviceTwoPhaseSolver  # noqa: E402
from benchmarks.chain_solve import best_ms, scrambles  # noqa: E402

MOST_TRIES = (1 << 31) - 1


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--sweep-rows", type=int, default=1 << 16)
	ap.add_argument("--big-rows", type=int, default=1 << 20)
	ap.add_argument("--caps", type=int, nargs="+", default=[8, 10, 12, 14, 16, 18, 20, 24])
	ap.add_argument("--max-nodes", type=int, nargs="+", default=[1 << 16, 1 << 18, 1 << 20])
	ap.add_argument("--repeats", type=int, default=5)
	ap.add_argument("--long-repeats", type=int, default=2)
	ap.add_argument("--long-ms", type=float, default=1000.0)
	ap.add_argument("--exact-rows", type=int, default=10_000)
	ap.add_argument("--out", default=os.path.join("profiles", "r32_two_phase_cap.json"))
	args = ap.parse_args()
	_ffi.require_gpu()
	lib = _ffi.lib()
	chain = DeviceChainSolver()
	solver = DeviceTwoPhaseSolver(chain=chain)
	doc = {"benchmark": "benchmarks/two_phase_cap.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
	       "long_repeats": args.long_repeats, "long_ms": args.long_ms, "tries": {"none": 8, "capped": MOST_TRIES}, "chain": [],
	       "settings": [], "best_caps": None, "exact_depth_10": None}

	def save():
		os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")

	st = _ffi.stream_ptr()

	def run(n, settings):
		"""the chain, then every (cap or None, max_nodes) of `settings` on the n rows; -> their rows of the table"""
		s = scrambles(n, 40, 2701)
		lengths = torch.empty(n, dtype=torch.int32, device="cuda")
		actions = torch.full((n, solver.max_length), -1, dtype=torch.int8, device="cuda")
		phases = torch.empty((n, 2), dtype=torch.int32, device="cuda")
		reason = torch.empty(n, dtype=torch.int32, device="cuda")
		nodes = torch.empty(n, dtype=torch.int64, device="cuda")
		counts = torch.empty((n, 2), dtype=torch.int32, device="cuda")
		err = torch.zeros(1, dtype=torch.int32, device="cuda")
		chain_ms = best_ms(lambda: _ffi.check(lib.rk_chain_solve(chain._h, s.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(), None,
		                                                         err.data_ptr(), st)), args.repeats)
		chain_lengths = lengths.clone()
		row = {"entry": "rk_chain_solve", "rows": n, "ms": round(chain_ms, 4), "mean_length": round(float(lengths.double().mean()), 4),
		       "max_length": int(lengths.max())}
		doc["chain"].append(row)
		print(json.dumps(row), flush=True)
		fill_ms = best_ms(lambda: actions.fill_(-1), args.repeats)
		out = []
		for cap, max_nodes in settings:
			tries = 8 if cap is None else MOST_TRIES

			def launch():
				actions.fill_(-1)
				_ffi.check(lib.rk_twophase_solve_capped(solver._h, chain._h, s.data_ptr(), n, tries, max_nodes, cap or 0, lengths.data_ptr(),
				                                        actions.data_ptr(), phases.data_ptr(), reason.data_ptr(), nodes.data_ptr(), counts.data_ptr(),
				                                        err.data_ptr(), st))
			t0 = time.perf_counter()
			launch()                                                      # best_ms warms up once more; this call sizes the repeats
			torch.cuda.synchronize()
			repeats = args.long_repeats if (time.perf_counter() - t0) * 1e3 > args.long_ms else args.repeats
			ms = best_ms(launch, repeats) - fill_ms
			assert int(err.item()) == -1 and int(lengths.min()) >= 0 and bool((lengths <= chain_lengths).all())
			total_nodes = int(nodes.sum())
			shares = [round(float((reason == r).double().mean()), 4) for r in range(3)]
			row = {"rows": n, "phase2_cap": cap, "tries": tries, "max_nodes": max_nodes, "repeats": repeats, "ms": round(ms, 3),
			       "rows_per_s": round(n / (ms * 1e-3)), "time_over_chain": round(ms / chain_ms, 1), "search_launch_ms": round(ms - chain_ms, 3),
			       "mean_length": round(float(lengths.double().mean()), 4), "max_length": int(lengths.max()),
			       "mean_phase_lengths": [round(float(v), 4) for v in phases.double().mean(dim=0)], "reason_shares": shares,
			       "mean_nodes": round(total_nodes / n, 1), "max_nodes_seen": int(nodes.max()),
			       "nodes_per_s": round(total_nodes / ((ms - chain_ms) * 1e-3)),
			       "mean_found": round(float(counts[:, 0].double().mean()), 2), "mean_entered": round(float(counts[:, 1].double().mean()), 2)}
			doc["settings"].append(row)
			out.append(row)
			print(json.dumps(row), flush=True)
			save()
		return out

	caps = list(args.caps) + [None]
	sweep = run(args.sweep_rows, [(cap, m) for m in args.max_nodes for cap in caps])
	top = max(args.max_nodes)
	ranked = sorted((r for r in sweep if r["max_nodes"] == top and r["phase2_cap"] is not None), key=lambda r: r["mean_length"])
	best = [r["phase2_cap"] for r in ranked[:2]]
	doc["best_caps"] = {"by": f"mean length at {args.sweep_rows} rows and max_nodes {top}", "caps": best}
	save()
	if args.big_rows:
		ends = sorted({min(args.max_nodes), top})
		run(args.big_rows, [(cap, m) for m in ends for cap in [None] + best])
	if args.exact_rows:
		ball = DeviceSymBall(10).build()
		states = ball.sample(args.exact_rows, depth=10, rng=np.random.default_rng(2901))[0]
		del ball
		doc["exact_depth_10"] = []
		for cap, max_nodes in ((None, 1 << 16), (best[0], 1 << 16), (None, 1 << 20), (best[0], 1 << 20)):
			made = DeviceTwoPhaseSolver(chain=chain, tries=8 if cap is None else None, max_nodes=max_nodes, phase2_cap=cap)
			lengths = np.asarray(made.solve(states)[0], np.int64)
			row = {"states": len(lengths), "exact_depth": 10, "phase2_cap": cap, "tries": made.tries, "max_nodes": max_nodes,
			       "mean_excess": round(float(lengths.mean()) - 10, 4), "max_length": int(lengths.max())}
			doc["exact_depth_10"].append(row)
			print(json.dumps(row), flush=True)
			save()
	save()
	print("wrote", args.out)


if __name__ == "__main__":
	main()
