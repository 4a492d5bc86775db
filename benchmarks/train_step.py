"""
Training from 20-byte states against training from one-hot rows, fc_small float32 (benchmarks.nets.FcSmall), one process, device events,
best of 5 after one warm-up, at batch sizes 1 000 / 10 000 / 225 000 (the last is one whole rollout of 7 500 games x depth 30):

  * `rk_ohl_backward` alone (dW and db of the first layer from states and dY);
  * the first layer forward + backward as torch runs it (`as_oh` + F.linear + autograd) and as `StateLinear` runs it;
  * one whole optimizer step (forward, both losses, backward, RMSprop) with `net(as_oh(states))` and with `train_on_states(net)(states)`;
  * peak allocated memory of that step both ways.

Traffic model of `rk_ohl_backward` (what has to cross HBM once, nothing counted twice for cache misses): n rows x (4 H bytes of dY + 20 bytes of
states), the partial slices written and read once (2 x splits x 480 x H x 4) and dW + db written (480 H x 4 + 4 H).  `hbm_share` is that over
the time over HBM_PEAK (8 TB/s, the MI355X's specified peak).

    python benchmarks/train_step.py > profiles/r23_train_step.json
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
SIZES = (1_000, 10_000, 225_000)
H = 4096


def best_of(fn, reps=5):
	fn()
	torch.cuda.synchronize()
	best = float("inf")
	for _ in range(reps):
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		fn()
		b.record()
		b.synchronize()
		best = min(best, a.elapsed_time(b))
	return best


def main():
	from benchmarks.nets import FcSmall
	from librubiks_amd import _ffi, cube
	from librubiks_amd.oh_linear import StateLinear, backward_rows, train_on_states
	rec = {"unit": "ms, best of 5, device events", "net": "fc_small float32, random init", "hbm_peak_bytes_per_s": HBM_PEAK, "sizes": {}}
	pc, vc = torch.nn.CrossEntropyLoss(reduction="none"), torch.nn.MSELoss(reduction="none")
	for n in SIZES:
		g = torch.Generator().manual_seed(n)
		# seeded codes 0 .. 23 per cubie (the layer is a table lookup per cubie: well-scrambled cubes spread over the bins the same way)
		states = torch.randint(0, 24, (n, 20), generator=g).to(torch.int8).cuda()
		dy = torch.randn((n, H), generator=g).cuda()
		pt = torch.randint(0, 12, (n,), generator=g).cuda()
		vt, lw = torch.randn(n, generator=g).cuda(), torch.rand(n, generator=g).cuda()
		out = {}

		net = FcSmall().cuda().train()
		lin = net.shared_net[0]
		first = StateLinear(lin)
		dw, db = torch.empty((H, 480), device="cuda"), torch.empty(H, device="cuda")
		lib, eng = _ffi.lib(), first._engine

		def bwd():
			_ffi.check(lib.rk_ohl_backward(eng._h, states.data_ptr(), dy.data_ptr(), n, dw.data_ptr(), db.data_ptr(), _ffi.stream_ptr()))
		ms = best_of(bwd)
		rows = backward_rows(n, H)
		splits = -(-n // rows)
		total = n * (4 * H + 20) + 2 * splits * 480 * H * 4 + 480 * H * 4 + 4 * H
		out["rk_ohl_backward"] = {"ms": ms, "rows_per_workgroup": rows, "splits": splits, "model_bytes": total, "model_bytes_per_row": total / n,
		                          "hbm_share": total / (ms * 1e-3) / HBM_PEAK}

		def layer_torch():
			lin.weight.grad = lin.bias.grad = None
			torch.nn.functional.linear(cube.device.as_oh(states), lin.weight, lin.bias).backward(dy)

		def layer_states():
			lin.weight.grad = lin.bias.grad = None
			first(states).backward(dy)
		out["first_layer_fwd_bwd"] = {"as_oh + F.linear": best_of(layer_torch), "StateLinear": best_of(layer_states)}

		opt = torch.optim.RMSprop(net.parameters(), lr=1e-5)
		from_states = train_on_states(net)

		def step(fwd, data):
			opt.zero_grad()
			pp, vp = fwd(data(), policy=True, value=True)
			loss = torch.mean(pc(pp, pt) * lw + vc(vp.squeeze(), vt) * lw)
			loss.backward()
			opt.step()
		ways = {"onehot": lambda: step(net, lambda: cube.device.as_oh(states)), "states": lambda: step(from_states, lambda: states)}
		out["optimizer_step"], out["peak_allocated_bytes"] = {}, {}
		for name, fn in ways.items():
			out["optimizer_step"][name] = best_of(fn)
			torch.cuda.synchronize()
			torch.cuda.reset_peak_memory_stats()
			base = torch.cuda.memory_allocated()
			fn()
			torch.cuda.synchronize()
			out["peak_allocated_bytes"][name] = {"peak": torch.cuda.max_memory_allocated(), "before_the_step": base}
		rec["sizes"][str(n)] = out
		del net, opt, from_states, first, dy
		torch.cuda.empty_cache()
	print(json.dumps(rec, indent=1))


if __name__ == "__main__":
	main()
