"""
ADI data generation with exact values inside the symmetry ball (`adi_traindata(..., ball=DeviceSymBall(R))`, engine
rk_symball_child_values) beside the unchanged `ball=None` path, on one MI355X at the reference's training size
(configs/main_train.ini:4-5: 7 500 games x depth 30 -> 2.7 M children per rollout) with the random-init fc_small net in bfloat16,
first layer fused with the ELU + BatchNorm epilogue, other BatchNorm layers folded.  One process: rollouts without a ball, with
DeviceSymBall(8) and with DeviceSymBall(10), the three taking turns rep by rep on the same seeds, each call timed by a host clock
around work that ends in a device synchronise.  Per ball also:
  * the share of the children the ball answered, by the number of moves of the scramble behind the parent state (lapanfix: state j of
    a game is j moves from solved, j = 0 .. depth - 1), and overall -- the rest are the net's rows;
  * the new entry's device time alone (its four launches on kept buffers), by device events over `--entry-reps` calls.
No ratio is promised: where the ball path is slower, the record says so ("ball_vs_none" > 1).

    python benchmarks/adi_ball.py --out profiles/r19_adi_ball.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.nets import FcSmall  # noqa: E402
from librubiks_amd import _ffi, cube  # noqa: E402
from librubiks_amd.adi import adi_traindata  # noqa: E402
from librubiks_amd.solving.agents import DeviceSymBall  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=7500)
ap.add_argument("--depth", type=int, default=30)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--entry-reps", type=int, default=20)
ap.add_argument("--radii", type=int, nargs="*", default=[8, 10])
ap.add_argument("--ff", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

_ffi.require_gpu()
METHOD, MODE = "lapanfix", "folded"
net = FcSmall().cuda().eval().to(torch.bfloat16)
balls = {None: None}
build_s = {}
for r in args.radii:
	t0 = time.perf_counter()
	balls[r] = DeviceSymBall(r).build()
	torch.cuda.synchronize()
	build_s[r] = time.perf_counter() - t0


def rollout(ball, games, seed):
	np.random.seed(seed)
	t0 = time.perf_counter()
	out = adi_traindata(net, games, args.depth, 0.5, METHOD, ff_batches=args.ff, fused_first_layer=MODE, ball=ball)
	torch.cuda.synchronize()
	return time.perf_counter() - t0, out


for ball in balls.values():                                              # warm-up: every shape's first launches, the fused net's set-up
	rollout(ball, 200, 0)
	rollout(ball, args.games, 0)
times = {r: [] for r in balls}
for rep in range(args.reps):                                             # the three take turns on the same seed
	for r, ball in balls.items():
		t, out = rollout(ball, args.games, 100 + rep)
		times[r].append(t)
		del out

# the children of one rollout (seed 100), for the shares and the entry's own time
np.random.seed(100)
faces = np.random.randint(0, 6, (args.depth, args.games))
dirs = np.random.randint(0, 2, (args.depth, args.games))
acts = torch.from_numpy((2 * faces + (1 - dirs)).astype(np.uint8)).cuda()
sub = cube.device.rollout_fanout(acts, True)[2]
m12 = len(sub)
lib = _ffi.lib()
rows_out = []
for r in args.radii:
	ball = balls[r]
	_, depths, rows, _ = cube.device.ball_child_values(ball, sub, 1.0)
	inside = (depths >= 0).reshape(args.games, args.depth, 12).float()
	by_depth = inside.mean(dim=(0, 2)).cpu().tolist()
	count = len(rows)
	values = torch.empty(m12, dtype=torch.float32, device="cuda")
	d8 = torch.empty(m12, dtype=torch.int8, device="cuda")
	idx = torch.empty(m12, dtype=torch.int32, device="cuda")
	outside = torch.empty((m12, 20), dtype=torch.int8, device="cuda")
	cnt = torch.empty(1, dtype=torch.int32, device="cuda")
	scratch = torch.empty(int(lib.rk_symball_child_values_scratch_bytes(m12)), dtype=torch.uint8, device="cuda")
	call = lambda: _ffi.check(lib.rk_symball_child_values(ball._h, sub.data_ptr(), m12, 1.0, d8.data_ptr(), values.data_ptr(), idx.data_ptr(),
	                                                      outside.data_ptr(), cnt.data_ptr(), scratch.data_ptr(), scratch.numel(), _ffi.stream_ptr()))
	for _ in range(3):
		call()
	start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	start.record()
	for _ in range(args.entry_reps):
		call()
	end.record()
	torch.cuda.synchronize()
	best, base = min(times[r]), min(times[None])
	rows_out.append({"radius": r, "orbits": len(ball), "build_seconds_with_create": build_s[r], "seconds_best": best, "seconds_all": times[r],
	                 "ball_vs_none": best / base, "slower_than_none": best > base, "children_answered_share": 1 - count / m12,
	                 "net_rows": count, "net_rows_none": m12, "share_by_scramble_moves": by_depth,
	                 "entry_device_seconds": start.elapsed_time(end) / 1e3 / args.entry_reps, "entry_reps": args.entry_reps})
rec = {"bench": "adi_ball", "device": torch.cuda.get_device_name(0), "games": args.games, "depth": args.depth, "children": m12,
       "net": "fc_small random init bf16", "mode": "first layer fused with ELU + BatchNorm epilogue, other BatchNorm layers folded",
       "method": METHOD, "ff_batches": args.ff, "reps": args.reps,
       "none": {"seconds_best": min(times[None]), "seconds_all": times[None]}, "balls": rows_out}
text = json.dumps(rec)
if args.out:
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, "w") as f:
		f.write(text + "\n")
print(text, flush=True)
