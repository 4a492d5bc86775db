"""
Shortest solutions that end at the symmetry ball, on one MI355X: DeviceSymBallSearch (engine rk_ssearch_*) on the radius-10
DeviceSymBall against the unchanged DeviceBallSearch on the plain radius-8 DeviceGoalBall and the unchanged DeviceBiBFS, everything
in one process.

    python benchmarks/symball_search.py [--lengths 12 14 16 18] [--pops 16384] [--repeats 3] [--out profiles/r14_symball_search.json]

Starts of optimal length L are prefixes of seeded 40-move scrambles, selected as benchmarks/ball.py selects them
(benchmarks/bibfs.py: pick_starts) -- with the new agent as the exact solver, since it is the only one of the three that reaches
18 moves; a prefix that needs more than --select-states own states is passed over.  Per length:
  sym_*     DeviceSymBallSearch: ms per search (best of --repeats after a warm-up search that grows the pool), states stored,
            iterations, us per iteration, complete own levels, the meeting depth
  ball_*    DeviceBallSearch on the plain ball where its own pool fits: it needs L - 8 - 1 complete levels and a part of the next,
            by counting 9.3 x as many states per level as the search above; `ball_fits: false` with the count otherwise
  bibfs_*   DeviceBiBFS where both sides fit its pool
  equal_lengths   every agent that ran found L moves, and its queue solves the start
--one-search L builds the ball, selects the start and runs two searches of that length with the new agent and nothing else: the
process to put under `rocprofv3 --kernel-trace --stats`, whose kernel_stats give the probe launch's share; --stats-csv reads that
file back into the document (`probe_share`: k_ss_probe's time over all rk_ssearch launches', `probe_share_of_iteration`: over the five
launches of an iteration).
"""
import argparse
import csv
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from librubiks_amd.solving.agents import DeviceBallSearch, DeviceBiBFS, DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch  # noqa: E402
from benchmarks.bibfs import pick_starts, solves, timed  # noqa: E402

GROWTH = 9.3                                    # states of a level over the level before it, far from both ends
LEVELS = DeviceGoalBall.LEVELS


class Selector:
	"""pick_starts' view of an agent: a search with a state budget, so that a prefix beyond the wanted lengths is given up."""

	def __init__(self, agent, max_states: int):
		self.agent, self.max_states = agent, max_states

	def search(self, start, time_limit=None):
		return self.agent.search(start, time_limit=time_limit, max_states=self.max_states)

	@property
	def action_queue(self):
		return self.agent.action_queue


def own_states(own_levels: int) -> float:
	"""States within `own_levels` moves of a start far from solved, by counting (the ball's own level sizes, then x 9.3)."""
	return sum(LEVELS[l] if l < len(LEVELS) else LEVELS[-1] * GROWTH ** (l - len(LEVELS) + 1) for l in range(own_levels + 1))


#: the launches of rk_ssearch: its own kernels (k_ss_*) and the frontier pool's, which every breadth-first engine shares
SEARCH_KERNELS = ("k_ss_", "k_fr_scan", "k_fr_append", "k_fr_rehash", "k_srch_end")
#: of these, the launches outside an iteration (an iteration is probe, expand, scan, append, end)
NOT_ITERATION = ("k_ss_root", "k_ss_walk", "k_fr_rehash")


def kernel_shares(path: str) -> dict:
	"""rocprofv3's kernel_stats.csv: time per kernel of the search, and the probe launch's share of it."""
	rows = {}
	with open(path) as f:
		for r in csv.DictReader(f):
			name = r["Name"].split("(")[0]
			if any(k in name for k in SEARCH_KERNELS):
				rows[name] = {"calls": int(r["Calls"]), "total_ns": int(r["TotalDurationNs"]), "average_ns": float(r["AverageNs"])}
	total = sum(r["total_ns"] for r in rows.values())
	iteration = sum(r["total_ns"] for n, r in rows.items() if not any(k in n for k in NOT_ITERATION))
	probe = sum(r["total_ns"] for n, r in rows.items() if "k_ss_probe" in n)
	return {"kernels": rows, "search_kernels_ns": total, "probe_share": round(probe / total, 4) if total else None,
	        "iteration_kernels_ns": iteration, "probe_share_of_iteration": round(probe / iteration, 4) if iteration else None}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--lengths", type=int, nargs="+", default=[12, 14, 16, 18])
	ap.add_argument("--sym-radius", type=int, default=10)
	ap.add_argument("--ball-radius", type=int, default=8)
	ap.add_argument("--pops", type=int, default=16_384)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--seed", type=int, default=2024)
	ap.add_argument("--time-limit", type=float, default=60.0)
	ap.add_argument("--select-states", type=int, default=200_000_000)
	ap.add_argument("--one-search", type=int, default=None)
	ap.add_argument("--stats-csv", default=None)
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	lengths = sorted(set(args.lengths if args.one_search is None else [args.one_search]))
	t0 = time.perf_counter()
	sball = DeviceSymBall(args.sym_radius, pops=args.pops).build()
	torch.cuda.synchronize()
	sym_build_s = time.perf_counter() - t0
	sym = DeviceSymBallSearch(sball, pops=args.pops)
	starts = pick_starts(Selector(sym, args.select_states), lengths, args.seed, args.time_limit)
	if args.one_search is not None:
		_, _, start = starts[args.one_search]
		for _ in range(2):
			assert sym.search(start, time_limit=args.time_limit) and len(sym.action_queue) == args.one_search
		return
	pball = DeviceGoalBall(args.ball_radius, pops=args.pops).build()
	plain, two = DeviceBallSearch(pball, pops=args.pops), DeviceBiBFS(pops=args.pops)
	doc = {"benchmark": "benchmarks/symball_search.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "pops": args.pops,
	       "sym_ball": {"radius": sball.radius, "orbits": len(sball), "build_s": round(sym_build_s, 4)},
	       "plain_ball": {"radius": pball.radius, "states": len(pball)}, "rows": []}
	for L in lengths:
		if L not in starts:
			doc["rows"].append({"length": L, "error": "no prefix of this optimal length found"})
			print(json.dumps(doc["rows"][-1]), flush=True)
			continue
		seed, k, start = starts[L]
		ok, best = timed(sym, start, args.repeats, time_limit=args.time_limit)
		equal = ok and len(sym.action_queue) == L and solves(start, sym.action_queue)
		row = {"length": L, "seed": seed, "scramble_moves": k, "sym_ms": round(1e3 * best, 4), "sym_len": len(sym), "sym_iterations": sym.iterations,
		       "sym_us_per_iteration": round(1e6 * best / max(sym.iterations, 1), 2), "sym_states_per_s": round(len(sym) / best),
		       "sym_depth": sym.depth, "sym_meeting_depth": sym.meeting_depth, "sym_capacity": sym._h_cap}
		# the plain ball: L - radius - 1 complete own levels and a part of the next one
		need = own_states(L - pball.radius)
		row["ball_fits"] = L <= pball.radius or need <= plain.max_capacity
		if row["ball_fits"]:
			ok, best1 = timed(plain, start, args.repeats, time_limit=args.time_limit)
			equal = equal and ok and len(plain.action_queue) == L and solves(start, plain.action_queue)
			row.update({"ball_ms": round(1e3 * best1, 4), "ball_len": len(plain), "ball_iterations": plain.iterations,
			            "ball_us_per_iteration": round(1e6 * best1 / max(plain.iterations, 1), 2), "ball_states_per_s": round(len(plain) / best1),
			            "ball_depth": plain.depth, "ratio_ball_over_sym_ms": round(best1 / best, 3),
			            "ratio_ball_over_sym_states": round(len(plain) / len(sym), 2)})
		else:
			row["ball_states_needed_by_counting"] = round(need)
		# the two-sided search: ceil(L / 2) levels on one side, the rest on the other
		need2 = own_states((L + 1) // 2) + own_states(L // 2)
		row["bibfs_fits"] = need2 <= two.max_capacity
		if row["bibfs_fits"]:
			ok, best2 = timed(two, start, args.repeats, time_limit=args.time_limit)
			equal = equal and ok and len(two.action_queue) == L and solves(start, two.action_queue)
			row.update({"bibfs_ms": round(1e3 * best2, 4), "bibfs_len": len(two), "bibfs_iterations": two.iterations,
			            "ratio_bibfs_over_sym_ms": round(best2 / best, 3)})
		else:
			row["bibfs_states_needed_by_counting"] = round(need2)
		row["equal_lengths"] = bool(equal)
		doc["rows"].append(row)
		print(json.dumps(row), flush=True)
	if args.stats_csv:
		doc["kernel_trace"] = kernel_shares(args.stats_csv)
	if args.out:
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")


if __name__ == "__main__":
	main()
