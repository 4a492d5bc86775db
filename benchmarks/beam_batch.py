"""
DeviceBeamSearchBatch (engine rk_beamb_*) beside the unchanged DeviceBeamSearch on one MI355X, everything in one process.

    python benchmarks/beam_batch.py [--games 256] [--depth 20] [--widths 256 4096] [--slots 16 64 256] [--radius 10]
                                    [--out profiles/r21_beam_batch.json]

--games seeded scrambles of --depth moves, on the stub heuristic (a forward that costs nothing) and on fc_small in bfloat16 with the
first layer fused and the BatchNorm layers folded (random weights), to DeviceSymBall(--radius) and without a ball.  Per (net, ball,
width): DeviceBeamSearch plays the scrambles one after the other -- the yardstick --, then DeviceBeamSearchBatch plays them with each
of --slots slots (capped by searches * width <= 2^16; a cap that repeats a setting is skipped).  Recorded: searches per second,
microseconds per lock-step depth, children per second (12 x width per depth a search ran) and the speed-up over the sequential
run.  On the stub net `lengths` and `status` must equal the sequential ones state by state (asserted); with fc_small a near-tie may
resolve differently in another batch shape, so there the number of states that differ is recorded.  `slower_than_sequential`
lists every setting where the batch lost.  The file is rewritten after every row, so a run that is cut short keeps what it measured.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from librubiks_amd.solving.agents import DeviceBeamSearch, DeviceBeamSearchBatch, DeviceSymBall  # noqa: E402
from benchmarks.beam import scramble, solves  # noqa: E402
from benchmarks.nets import FastStub, FcSmall  # noqa: E402


def sequential(agent, starts) -> dict:
	status, lengths, depths = [], [], []
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	for s in starts:
		won = agent.search(s, None, None)
		status.append(agent.status)
		lengths.append(len(agent.action_queue) if won else -1)
		depths.append(agent.depth)
	torch.cuda.synchronize()
	return {"seconds": time.perf_counter() - t0, "status": np.array(status), "lengths": np.array(lengths), "depths": np.array(depths)}


def batched(b, starts) -> dict:
	torch.cuda.synchronize()
	t0 = time.perf_counter()
	b.search(starts)
	torch.cuda.synchronize()
	return {"seconds": time.perf_counter() - t0, "status": b.status[:, 0].copy(), "lengths": b.lengths.copy(), "depths": b.depths.copy(),
	        "lockstep_depths": b.lockstep_depths}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--games", type=int, default=256)
	ap.add_argument("--depth", type=int, default=20)
	ap.add_argument("--widths", type=int, nargs="+", default=[256, 4096])
	ap.add_argument("--slots", type=int, nargs="+", default=[16, 64, 256])
	ap.add_argument("--radius", type=int, default=10)
	ap.add_argument("--max-depth", type=int, default=64)
	ap.add_argument("--poll", type=int, default=8)
	ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_beam_batch.json"))
	args = ap.parse_args()
	nets = {"stub": (FastStub(), False), "fc_small_bf16_fused_folded": (FcSmall().cuda().eval().to(torch.bfloat16), "folded")}
	starts = np.array([scramble(1000 * args.depth + g, args.depth) for g in range(args.games)], np.int8)
	doc = {"benchmark": "benchmarks/beam_batch.py", "device": torch.cuda.get_device_name(0), "games": args.games, "scramble_depth": args.depth,
	       "max_depth": args.max_depth, "poll": args.poll, "rows": [], "slower_than_sequential": [], "complete": False}

	def save():
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			json.dump(doc, f, indent=1)
			f.write("\n")

	for radius in (args.radius, None):
		ball = DeviceSymBall(radius).build() if radius is not None else None
		for name, (net, fused) in nets.items():
			for width in args.widths:
				common = {"max_depth": args.max_depth, "ball": ball, "poll": args.poll, "fused_first_layer": fused}
				agent = DeviceBeamSearch(net, width, **common)
				agent.search(starts[0], None, None)                    # the capture is not timed
				seq = sequential(agent, starts)
				for i in np.nonzero(seq["lengths"] >= 0)[0][:4]:
					agent.search(starts[i], None, None)
					assert solves(starts[i], agent.action_queue)
				del agent
				children = 12 * width * int(seq["depths"].sum())
				row = {"net": name, "ball_radius": radius, "width": width, "agent": "DeviceBeamSearch", "seconds": round(seq["seconds"], 4),
				       "searches_per_s": round(args.games / seq["seconds"], 1), "share_solved": round(float((seq["lengths"] >= 0).mean()), 4),
				       "depths_run": int(seq["depths"].sum()), "us_per_depth": round(1e6 * seq["seconds"] / max(int(seq["depths"].sum()), 1), 2),
				       "children_per_s": round(children / seq["seconds"])}
				doc["rows"].append(row)
				print(json.dumps(row), flush=True)
				save()
				tried = set()
				for slots in args.slots:
					slots = max(1, min(slots, DeviceBeamSearchBatch.MAX_BEAMS // width, args.games))
					if slots in tried:
						continue
					tried.add(slots)
					b = DeviceBeamSearchBatch(net, width, searches=slots, **common)
					b.search(starts[:1])                               # the capture is not timed
					got = batched(b, starts)
					differ = int(((got["status"] != seq["status"]) | (got["lengths"] != seq["lengths"])).sum())
					if name == "stub":
						assert differ == 0, (name, radius, width, slots, differ)
					for i in np.nonzero(got["lengths"] >= 0)[0][:4]:
						assert solves(starts[i], b.action_queue_of(i))
					children = 12 * width * int(got["depths"].sum())
					row = {"net": name, "ball_radius": radius, "width": width, "agent": "DeviceBeamSearchBatch", "searches": slots,
					       "seconds": round(got["seconds"], 4), "searches_per_s": round(args.games / got["seconds"], 1),
					       "share_solved": round(float((got["lengths"] >= 0).mean()), 4), "lockstep_depths": int(got["lockstep_depths"]),
					       "us_per_lockstep_depth": round(1e6 * got["seconds"] / max(int(got["lockstep_depths"]), 1), 2),
					       "children_per_s": round(children / got["seconds"]), "states_that_differ_from_sequential": differ,
					       "speedup_over_sequential": round(seq["seconds"] / got["seconds"], 3)}
					doc["rows"].append(row)
					if row["speedup_over_sequential"] < 1:
						doc["slower_than_sequential"].append({k: row[k] for k in ("net", "ball_radius", "width", "searches", "speedup_over_sequential")})
					print(json.dumps(row), flush=True)
					save()
					del b
	doc["complete"] = True
	save()


if __name__ == "__main__":
	main()
