"""
The two-phase search on one MI355X (engine rk_twophase_*, `DeviceTwoPhaseSolver`), everything in one process:

    python benchmarks/two_phase.py [--rows 65536 1048576] [--tries 1 8 64] [--max-nodes 65536 1048576] [--out profiles/r29_two_phase.json]

On seeded 40-move scrambles (the rows of benchmarks/chain_solve.py): the unchanged rk_chain_solve, then rk_twophase_solve at every
(tries, max_nodes), device events, best of `--repeats`: states/s, the time as a ratio to the chain's on the same rows, the search
launch alone (the difference of the two, both measured), mean and greatest length and mean phase lengths beside the chain's, the
shares of reasons 0 / 1 / 2, mean and greatest nodes per state and nodes/s, the mean length after `DeviceSymBall(8).shorten` on
`--shorten-rows` of the queues of one setting.  Then, on `--exact-rows` states at the exact depth 10 (`DeviceSymBall(10).sample`),
the mean excess over that depth.  A setting whose answer equals the chain's on more than half the rows, or whose time exceeds 100x
the chain's, is listed under "findings".  The file is written after every section, so a run that is cut short leaves what it had.
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
from librubiks_amd import _ffi  # noqa: E402
from librubiks_amd.solving.agents import DeviceChainSolver, DeviceSymBall, DeviceTwoPhaseSolver  # noqa: E402
from benchmarks.chain_solve import best_ms, scrambles  # noqa: E402


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--rows", type=int, nargs="+", default=[1 << 16, 1 << 20])
	ap.add_argument("--tries", type=int, nargs="+", default=[1, 8, 64])
	ap.add_argument("--max-nodes", type=int, nargs="+", default=[1 << 16, 1 << 20])
	ap.add_argument("--repeats", type=int, default=5)
	ap.add_argument("--shorten-rows", type=int, default=10_000)
	ap.add_argument("--shorten-setting", type=int, nargs=2, default=[8, 1 << 16], help="tries and max_nodes of the queues that are shortened")
	ap.add_argument("--exact-rows", type=int, default=10_000)
	ap.add_argument("--out", default=os.path.join("profiles", "r29_two_phase.json"))
	args = ap.parse_args()
	_ffi.require_gpu()
	lib = _ffi.lib()
	chain = DeviceChainSolver()
	DeviceTwoPhaseSolver(chain=chain)                                     # the first use: code objects loaded
	t0 = time.perf_counter()
	solver = DeviceTwoPhaseSolver(chain=chain)
	torch.cuda.synchronize()
	doc = {"benchmark": "benchmarks/two_phase.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
	       "create_wall_s": round(time.perf_counter() - t0, 4), "table_counts": list(solver.table_counts),
	       "table_depths": list(solver.table_depths), "grid_rows": solver.grid_rows, "chain": [], "settings": [], "findings": [],
	       "shorten": None, "exact_depth_10": None}

	def save():
		os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")

	print(json.dumps({k: doc[k] for k in ("create_wall_s", "table_counts", "table_depths")}), flush=True)
	st = _ffi.stream_ptr()
	for n in args.rows:
		s = scrambles(n, 40, 2701)
		lengths = torch.empty(n, dtype=torch.int32, device="cuda")
		actions = torch.full((n, solver.max_length), -1, dtype=torch.int8, device="cuda")
		phases = torch.empty((n, 2), dtype=torch.int32, device="cuda")
		reason = torch.empty(n, dtype=torch.int32, device="cuda")
		nodes = torch.empty(n, dtype=torch.int64, device="cuda")
		err = torch.zeros(1, dtype=torch.int32, device="cuda")
		chain_ms = best_ms(lambda: _ffi.check(lib.rk_chain_solve(chain._h, s.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(), None,
		                                                         err.data_ptr(), st)), args.repeats)
		chain_lengths = lengths.clone()
		row = {"entry": "rk_chain_solve", "rows": n, "ms": round(chain_ms, 4), "rows_per_s": round(n / (chain_ms * 1e-3)),
		       "mean_length": round(float(lengths.double().mean()), 4), "max_length": int(lengths.max())}
		doc["chain"].append(row)
		print(json.dumps(row), flush=True)
		for max_nodes in args.max_nodes:
			for tries in args.tries:
				def launch():
					actions.fill_(-1)
					_ffi.check(lib.rk_twophase_solve(solver._h, chain._h, s.data_ptr(), n, tries, max_nodes, lengths.data_ptr(), actions.data_ptr(),
					                                 phases.data_ptr(), reason.data_ptr(), nodes.data_ptr(), err.data_ptr(), st))
				fill_ms = best_ms(lambda: actions.fill_(-1), args.repeats)
				ms = best_ms(launch, args.repeats) - fill_ms
				assert int(err.item()) == -1 and int(lengths.min()) >= 0 and bool((lengths <= chain_lengths).all())
				total_nodes = int(nodes.sum())
				shares = [round(float((reason == r).double().mean()), 4) for r in range(3)]
				row = {"rows": n, "tries": tries, "max_nodes": max_nodes, "ms": round(ms, 3), "rows_per_s": round(n / (ms * 1e-3)),
				       "time_over_chain": round(ms / chain_ms, 1), "search_launch_ms": round(ms - chain_ms, 3),
				       "mean_length": round(float(lengths.double().mean()), 4), "max_length": int(lengths.max()),
				       "mean_phase_lengths": [round(float(v), 4) for v in phases.double().mean(dim=0)], "reason_shares": shares,
				       "mean_nodes": round(total_nodes / n, 1), "max_nodes_seen": int(nodes.max()),
				       "nodes_per_s": round(total_nodes / ((ms - chain_ms) * 1e-3))}
				doc["settings"].append(row)
				print(json.dumps(row), flush=True)
				if shares[2] > 0.5:
					doc["findings"].append(f"rows={n} tries={tries} max_nodes={max_nodes}: {shares[2]:.1%} of the rows still hold the chain's answer")
				if ms > 100 * chain_ms:
					doc["findings"].append(f"rows={n} tries={tries} max_nodes={max_nodes}: {ms / chain_ms:.0f}x the chain's time")
				if doc["shorten"] is None and args.shorten_rows and [tries, max_nodes] == list(args.shorten_setting):
					k = min(args.shorten_rows, n)
					h_len, h_act = lengths[:k].cpu().numpy(), actions[:k].cpu().numpy()
					ball = DeviceSymBall(8).build()
					done = ball.shorten([h_act[i, :h_len[i]] for i in range(k)])
					doc["shorten"] = {"ball": "DeviceSymBall(8)", "queues": k, "tries": tries, "max_nodes": max_nodes,
					                  "mean_length": round(float(h_len.mean()), 4), "mean_converged": round(float(np.mean([len(q) for q in done])), 4)}
					print(json.dumps(doc["shorten"]), flush=True)
					del ball
				save()
		del s, lengths, actions, phases, reason, nodes
	if args.exact_rows:
		ball = DeviceSymBall(10).build()
		states = ball.sample(args.exact_rows, depth=10, rng=np.random.default_rng(2901))[0]
		del ball
		doc["exact_depth_10"] = []
		for tries, max_nodes in ((1, 1 << 16), (8, 1 << 16), (8, 1 << 20)):
			got = DeviceTwoPhaseSolver(chain=chain, tries=tries, max_nodes=max_nodes).solve(states, details=True)
			lengths = np.asarray(got[0].cpu() if isinstance(got[0], torch.Tensor) else got[0], np.int64)
			row = {"states": len(lengths), "exact_depth": 10, "tries": tries, "max_nodes": max_nodes,
			       "mean_excess": round(float(lengths.mean()) - 10, 4), "max_length": int(lengths.max())}
			doc["exact_depth_10"].append(row)
			print(json.dumps(row), flush=True)
			save()
	save()
	print("wrote", args.out)


if __name__ == "__main__":
	main()
