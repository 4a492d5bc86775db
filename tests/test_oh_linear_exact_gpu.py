"""
The fused net ends -- k_ohl_gather, k_ohl_mfma, k_ohl_mfma_direct and k_tail_linear (librubiks_amd/csrc/rk_oh_linear.hip) -- against a
float64 reference built on the device by indexing (tests/oh_linear_ref.py), at bounds derived from the number formats:

  * gather route, float32, no epilogue: 21 u mag (twenty sequential float32 adds), with and without a bias, from float32 and from
    bfloat16 weights;
  * every bfloat16 output (both MFMA forms, `route="mfma"`, the gather route's bfloat16 output): HALF a bfloat16 ulp, 2^-8, plus the
    float32 sum's error -- nearest-even rounding, which a truncating kernel misses on a quarter of its outputs;
  * the float32 epilogue on its own, fed the gather route's own float32 sums: 16 u of the product, which tells expm1 from exp - 1;
  * a NaN in the bias or in a selected weight is a NaN behind every (route, activation, affine) combination and nothing else is;
  * rk_tail_linear with and without a bias and on the activations' boundary inputs (zeros, denormals, -100, the largest bfloat16, the
    infinities, a NaN);
  * `fuse_first_linear(..., epilogue=True, fold_batchnorm=True)` on a net whose first and last layers have no bias.

tests/test_oh_linear_ref_cpu.py proves that these bounds accept a faithful emulation of every route and reject the subtly wrong ones.
Shapes: H = 64 is one column tile, at H = 192 the direct form's last column group holds two live waves and two dead ones; n = 1, 31, 32,
33 around a row tile, the 480 cover rows (every (cubie, code) pair), 769 = the first batch `route="mfma"` gives to the tiled form, with a
ragged last pass.  Row 0 of every batch but the cover rows holds codes 23 and 0 alternating: the ends of a 24-wide slice for a single row.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import cube
from librubiks_amd.oh_linear import OhLinear, TailLinear, batchnorm_affine, fuse_first_linear
from tests import oh_linear_ref as R
from tests.helpers import random_walk

pytestmark = pytest.mark.gpu

SEED = 11
HS = (64, 192)
NS = (1, 31, 32, 33, 480, 769)
CASES = [(a, aff) for a in (None, "elu", "elu0.7", "relu") for aff in (False, True)]


@functools.lru_cache(maxsize=None)
def _pool() -> torch.Tensor:
	"""781 rows: the edge row, the 480 cover rows, 300 scrambled cubes"""
	edge = np.array([[23 if i % 2 == 0 else 0 for i in range(20)]], dtype=np.int8)
	return torch.from_numpy(np.concatenate([edge, R.cover_states(SEED), random_walk(300, 15, seed=SEED)])).cuda()


def _rows(n):
	"""the slice of the pool a batch of n rows is (the cover rows on their own at n = 480)"""
	return slice(1, 481) if n == 480 else slice(0, n)


@functools.lru_cache(maxsize=None)
def _layer(H, dtype, bias=True, seed=SEED):
	torch.manual_seed(seed + H)
	lin = torch.nn.Linear(480, H, bias=bias)
	torch.nn.init.xavier_uniform_(lin.weight)
	if bias:
		torch.nn.init.uniform_(lin.bias, -0.5, 0.5)
	return lin.cuda().to(dtype).requires_grad_(False)


@functools.lru_cache(maxsize=None)
def _bn(H, seed=3):
	"""an eval-mode BatchNorm1d with statistics worth applying and gammas of both signs; -> (module, scale, shift)"""
	g = torch.Generator().manual_seed(seed)
	bn = torch.nn.BatchNorm1d(H)
	with torch.no_grad():
		bn.running_mean.copy_(torch.randn(H, generator=g) * 0.3)
		bn.running_var.copy_(torch.rand(H, generator=g) * 1.5 + 0.25)
		bn.weight.copy_((torch.rand(H, generator=g) + 0.5) * torch.where(torch.rand(H, generator=g) < 0.25, -1.0, 1.0))
		bn.bias.copy_(torch.randn(H, generator=g) * 0.2)
	bn = bn.cuda().eval()
	return (bn,) + tuple(batchnorm_affine(bn))


@functools.lru_cache(maxsize=None)
def _reference(H, dtype, bias, route):
	"""(x, mag) in float64 for the whole pool, on the values `route` sums from the layer _layer(H, dtype, bias); computed once, never written"""
	lin = _layer(H, dtype, bias)
	return R.first_layer64(_pool(), R.route_weight(lin.weight, route), lin.bias)


def _epilogues(layer, H):
	"""every (activation, affine) combination set on `layer` in turn: -> (label, keyword arguments of the reference helpers)"""
	bn, scale, shift = _bn(H)
	for name, affine in CASES:
		act, alpha = R.ACTS[name]
		layer.set_epilogue(R.module_of(name), bn if affine else None)
		yield f"{name} affine={affine}", dict(act=act, alpha=alpha, scale=scale if affine else None, shift=shift if affine else None)
	layer.set_epilogue(None, None)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("H", HS)
def test_gather_f32_against_float64(H, bias):
	"""The exact route without an epilogue: within 21 u mag of the float64 sum, with a bias and with `bias=None` (k_ohl_bias writes zeros)."""
	lin = _layer(H, torch.float32, bias)
	x, mag = _reference(H, torch.float32, bias, "gather")
	layer = OhLinear(lin, route="gather")
	for n in NS:
		y = layer(_pool()[_rows(n)].contiguous())
		assert y.dtype == torch.float32 and y.shape == (n, H)
		R.assert_f32_preactivation(y, x[_rows(n)], mag[_rows(n)], what=f"gather f32 n={n} H={H} bias={bias}")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("H", HS)
def test_gather_from_bf16_weights_into_a_float32_output(H, bias):
	"""A bfloat16 layer on the gather route with a float32 `out=`: the same 21 u mag bound, on the bfloat16 weight and bias values."""
	lin = _layer(H, torch.bfloat16, bias)
	x, mag = _reference(H, torch.bfloat16, bias, "gather")
	layer = OhLinear(lin, route="gather")
	for n in NS:
		states = _pool()[_rows(n)].contiguous()
		out = torch.full((len(states) + 2, H), 7.0, dtype=torch.float32, device="cuda")
		layer(states, out=out[:len(states)], route="gather")
		assert (out[len(states):] == 7.0).all()
		R.assert_f32_preactivation(out[:len(states)], x[_rows(n)], mag[_rows(n)], what=f"gather bf16->f32 n={n} H={H} bias={bias}")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("route", ["mfma_direct", "mfma_tiled", "mfma"])
def test_mfma_routes_against_float64(route, H, bias):
	"""Both MFMA forms and the automatic choice, every epilogue, every batch size: half a bfloat16 ulp of the float64 reference plus the
	float32 sum's error.  Guard rows behind the output stay untouched."""
	lin = _layer(H, torch.bfloat16, bias)
	x, mag = _reference(H, torch.bfloat16, bias, "mfma")
	layer = OhLinear(lin, route="mfma")
	worst = 0.0
	for label, kw in _epilogues(layer, H):
		for n in NS:
			states = _pool()[_rows(n)].contiguous()
			out = torch.full((len(states) + 2, H), 7.0, dtype=torch.bfloat16, device="cuda")
			layer(states, out=out[:len(states)], route=route)
			assert (out[len(states):] == 7.0).all(), (route, label, n)
			worst = max(worst, R.assert_bf16_output(out[:len(states)], x[_rows(n)], mag[_rows(n)], **kw, what=f"{route} {label} n={n} H={H} bias={bias}"))
	print(f"largest |diff| / bound: {worst:.3f}")


@pytest.mark.parametrize("route", ["mfma_direct", "mfma_tiled"])
def test_mfma_routes_round_float32_weights_to_nearest_even(route):
	"""A float32 layer on the MFMA route: k_ohl_prepare rounds the weights to bfloat16 (nearest even), the bias stays float32."""
	H = 192
	lin = _layer(H, torch.float32, True)
	x, mag = _reference(H, torch.float32, True, "mfma")
	layer = OhLinear(lin, route="mfma")
	for label, kw in _epilogues(layer, H):
		y = layer(_pool(), route=route)
		assert y.dtype == torch.bfloat16
		R.assert_bf16_output(y, x, mag, **kw, what=f"{route} from f32 weights, {label}")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("H", HS)
def test_gather_bf16_output_with_epilogue(H, bias):
	"""The gather route from bfloat16 weights with its bfloat16 output and every epilogue: the bfloat16 bound."""
	lin = _layer(H, torch.bfloat16, bias)
	x, mag = _reference(H, torch.bfloat16, bias, "gather")
	layer = OhLinear(lin, route="gather")
	for label, kw in _epilogues(layer, H):
		for n in NS:
			y = layer(_pool()[_rows(n)].contiguous())
			assert y.dtype == torch.bfloat16
			R.assert_bf16_output(y, x[_rows(n)], mag[_rows(n)], **kw, what=f"gather bf16 {label} n={n} H={H} bias={bias}")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("H", HS)
def test_gather_f32_epilogue_on_its_own(H, bias):
	"""The float32 epilogue, isolated from the sum: the layer without an epilogue gives x32 (the same float32 adds in the same order:
	checked here bit for bit), the layer with one must give scale * act(x32) + shift within 16 u of the product and 2 u of the result.
	The pool holds well over 100 pre-activations in (-0.1, -1e-3), where exp(x) - 1 is 1e-4 off and expm1 is not."""
	lin = _layer(H, torch.float32, bias)
	pool = _pool()
	x32 = OhLinear(lin, route="gather")(pool)
	acc = (lin.bias if bias else torch.zeros(H, device="cuda")).expand(len(pool), H).clone()
	idx = pool.long() + 24 * torch.arange(20, device="cuda")
	wt = lin.weight.t().contiguous()
	for i in range(20):
		acc = acc + wt[idx[:, i]]
	assert torch.equal(x32, acc)
	assert R.elu_teeth(x32) >= 100, R.elu_teeth(x32)
	layer = OhLinear(lin, route="gather")
	worst = 0.0
	for label, kw in _epilogues(layer, H):
		worst = max(worst, R.assert_f32_epilogue(layer(pool), x32, **kw, what=f"f32 epilogue {label} H={H} bias={bias}"))
		for n in NS:
			y = layer(pool[_rows(n)].contiguous())
			R.assert_f32_epilogue(y, x32[_rows(n)], **kw, what=f"f32 epilogue {label} n={n} H={H} bias={bias}")
	print(f"largest |diff| / bound: {worst:.3f}")


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("route", ["gather_f32", "gather_bf16", "mfma_direct", "mfma_tiled", "mfma"])
def test_nan_survives_every_epilogue(route, H):
	"""VERDICT r2 #9, behind the epilogue too: a NaN in bias[:4] and one NaN weight (output 9, cubie 3 at code 23) that only some rows
	select.  The output is NaN exactly where the float64 reference is -- the gather routes meet the weight only in the rows that select
	it, the matrix product multiplies it with the one-hot's zeros in every row (0 * NaN = NaN, as torch's dense layer does) -- and no
	other output is NaN or infinite, whatever the activation and with or without the affine map."""
	dtype = torch.float32 if route == "gather_f32" else torch.bfloat16
	lin = copy.deepcopy(_layer(H, dtype, True))
	lin.bias[:4] = float("nan")
	lin.weight[9, 24 * 3 + 23] = float("nan")
	pool = _pool()
	picked = pool[:, 3] == 23
	assert picked.any() and not picked.all()
	kernel_route = "gather" if route.startswith("gather") else route
	x, mag = R.first_layer64(pool, R.route_weight(lin.weight, kernel_route), lin.bias)
	assert torch.isnan(x[:, :4]).all() and torch.equal(torch.isnan(x[:, 9]), picked) and not torch.isnan(x[:, 10:]).any()
	if kernel_route != "gather":
		x[:, 9] = float("nan")
	layer = OhLinear(lin, route=kernel_route)
	x32 = OhLinear(lin, route="gather")(pool) if route == "gather_f32" else None
	for label, kw in _epilogues(layer, H):
		for n in (len(pool), 33):
			y = layer(pool[:n].contiguous(), route=kernel_route)
			ref = R.epilogue64(x[:n], **kw)
			assert torch.equal(torch.isnan(y), torch.isnan(ref)), (route, label, n)
			assert not torch.isinf(y).any() and torch.isnan(y[:, :4]).all() and not torch.isnan(y[:, 10:]).any(), (route, label, n)
			if route == "gather_f32":
				R.assert_f32_preactivation(x32[:n], x[:n], mag[:n])
				R.assert_f32_epilogue(y, x32[:n], **kw, what=f"NaN {route} {label} n={n}")
			else:
				R.assert_bf16_output(y, x[:n], mag[:n], **kw, what=f"NaN {route} {label} n={n}")


@pytest.mark.parametrize("n,H", [(3072, 4096), (66_000, 64)])
def test_mfma_tiled_three_tiles_per_wave_against_float64(n, H):
	"""The tiled form with three 32-row tiles per wave and pass.  rk_ohl_forward's planner takes it where it costs fewer tiles on the busiest
	SIMD than two: 3 072 x 4 096 (64 column tiles: 8 row groups of 384 rows against 6 of 512 on 512 slots), and 66 000 x 64 -- one column
	tile, 512 row groups wanted; two tiles: quantum 256, ceil(66 000 / 256) = 258 groups of 256 rows, ceil(258 / 256) = 2 workgroups per
	slot x 1 pass x 2 tiles = 4; three tiles: quantum 384, ceil(66 000 / 384) = 172 groups of 384 rows, 1 x 1 x 3 = 3 < 4.  (Any n in
	65 537 .. 98 304 does at H = 64.)  The last group is ragged (66 000 = 171 x 384 + 336).  ELU + affine epilogue, float64 reference
	by indexing, one torch expression per cubie.  (The library does not say which form it took: whoever changes the planner recomputes
	this; a comment at the planner points here.)"""
	lin = _layer(H, torch.bfloat16, True)
	states = torch.from_numpy(np.concatenate([R.cover_states(SEED), R.random_states(n - 480, seed=n)])).cuda()
	x, mag = R.first_layer64(states, lin.weight, lin.bias)
	layer = OhLinear(lin, route="mfma")
	bn, scale, shift = _bn(H)
	for label, kw in (("no epilogue", {}), ("elu0.7 affine", dict(act="elu", alpha=0.7, scale=scale, shift=shift))):
		layer.set_epilogue(R.module_of("elu0.7") if kw else None, bn if kw else None)
		out = torch.full((n + 2, H), 7.0, dtype=torch.bfloat16, device="cuda")
		layer(states, out=out[:n], route="mfma_tiled")
		assert (out[n:] == 7.0).all()
		print(f"{label}: largest |diff| / bound: {R.assert_bf16_output(out[:n], x, mag, **kw, what=f'tiled {n} x {H} {label}'):.3f}")


def _tail_input(K, rows=37):
	"""`rows` x K bfloat16: rows 0 .. 15 (one workgroup's block) carry one boundary value each among ordinary values, the rest is ordinary.
	-> (x, {name: row})"""
	g = torch.Generator(device="cuda").manual_seed(K)
	x = (torch.randn(rows, K, device="cuda", generator=g) * 1.5).to(torch.bfloat16)
	edges = {"+0": 0.0, "-0": -0.0, "-2^-20": -2.0 ** -20, "-2^-126": -2.0 ** -126, "-100": -100.0,
	         "bf16 max": float(torch.finfo(torch.bfloat16).max), "+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"),
	         "-2^-130": -2.0 ** -130}
	where = {}
	for r, (name, v) in enumerate(edges.items()):
		x[r, (5 + 37 * r) % K] = v
		where[name] = r
	x[10, :] = 0.0                                                       # all zeros but one -inf: ELU gives -alpha there and nothing else counts
	x[10, 77] = float("-inf")
	where["only -inf"] = 10
	x[11, 3::7] = -0.0                                                   # several boundary values in one row
	x[11, 1], x[11, K - 1], x[11, K // 2] = -100.0, float("-inf"), -2.0 ** -126
	assert x[1, (5 + 37) % K].view(torch.int16) == -32768                # the -0 is a -0
	return x, where


@pytest.mark.parametrize("M", [1, 13])
@pytest.mark.parametrize("K", [512, 1024, 2048])
def test_tail_linear_edges_and_no_bias(K, M):
	"""rk_tail_linear with and without a bias on a block of boundary inputs: +-0, -2^-20, the smallest normal and a denormal, -100, the
	largest bfloat16, +-inf and a NaN, each among ordinary values.  Against float64 on torch's own activation in float32 rounded to
	bfloat16 (as test_tail_linear_is_activation_plus_linear builds it), at that test's bound.  An infinite activation times a weight is
	that infinity in the reference and in the kernel; -inf under ELU is the finite -alpha; a row holding a NaN is NaN in all M outputs,
	with and without an activation; every other output is finite exactly where the reference is."""
	x, where = _tail_input(K)
	for bias in (True, False):
		torch.manual_seed(K + M)
		lin = torch.nn.Linear(K, M, bias=bias).cuda().to(torch.bfloat16).requires_grad_(False)
		W = lin.weight.double()
		b = lin.bias.double() if bias else torch.zeros(M, dtype=torch.float64, device="cuda")
		assert (W != 0).all()
		for name in (None, "elu", "elu0.7", "relu"):
			module = R.module_of(name)
			tail = TailLinear(module, lin)
			assert (tail.bias is None) == (not bias)
			y = tail(x)
			assert y.shape == (len(x), M) and y.dtype == torch.bfloat16
			a = (module(x.float()) if module is not None else x.float()).to(torch.bfloat16).double()
			ref = a @ W.t() + b
			mag = a.abs() @ W.abs().t() + b.abs()
			what = f"tail K={K} M={M} bias={bias} act={name}"
			R.assert_tail(y, ref, mag, what=what)
			assert torch.isnan(y[where["nan"]]).all(), what
			assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.isfinite(y), torch.isfinite(ref)), what
			finite_rows = torch.isfinite(a).all(dim=1)
			assert torch.isfinite(y[finite_rows]).all(), what
			# the rows that are not: a NaN or a +inf passes every activation, a -inf only where there is none (ELU: -alpha, ReLU: 0)
			lost = torch.isnan(x).any(dim=1) | (x == float("inf")).any(dim=1)
			if name is None:
				lost = lost | (x == float("-inf")).any(dim=1)
			assert torch.equal(~finite_rows, lost) and lost[where["nan"]] and lost[where["+inf"]] and bool(lost[where["-inf"]]) == (name is None), what
			if name in ("elu", "elu0.7"):
				alpha = R.ACTS[name][1]
				r = where["only -inf"]
				assert torch.isfinite(y[where["-inf"]]).all() and torch.isfinite(y[11]).all(), what
				want = torch.tensor(-alpha, dtype=torch.bfloat16).double() * W[:, 77] + b
				# an exact product, one float32 add (2^-24) and the rounding to bfloat16 (2^-8)
				assert ((y[r].double() - want).abs() <= (2.0 ** -8 + 2.0 ** -22) * want.abs() + 1e-30).all(), what
			if name == "relu":
				assert torch.equal(y[where["only -inf"]].double(), b.to(torch.bfloat16).double()), what


class _NoBiasNet(torch.nn.Module):
	"""A net of the reference's shape (model.py:117-141) whose first and last Linear layers have no bias: 480 -> 64 shared, heads
	64 -> 512 -> 12 / 1, ELU + BatchNorm1d behind every layer but the last."""
	def __init__(self, seed):
		super().__init__()
		torch.manual_seed(seed)
		nn = torch.nn
		self.shared_net = nn.Sequential(nn.Linear(480, 64, bias=False), nn.ELU(), nn.BatchNorm1d(64))
		self.policy_net = nn.Sequential(nn.Linear(64, 512), nn.ELU(), nn.BatchNorm1d(512), nn.Linear(512, 12, bias=False))
		self.value_net = nn.Sequential(nn.Linear(64, 512), nn.ELU(), nn.BatchNorm1d(512), nn.Linear(512, 1, bias=False))
		g = torch.Generator().manual_seed(seed)
		for m in self.modules():
			if isinstance(m, nn.Linear):
				nn.init.xavier_uniform_(m.weight)
			if isinstance(m, nn.BatchNorm1d):
				with torch.no_grad():
					m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
					m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.25)
					m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
					m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)

	def forward(self, x, policy=True, value=True):
		x = self.shared_net(x)
		out = ([self.policy_net(x)] if policy else []) + ([self.value_net(x)] if value else [])
		return out if len(out) > 1 else out[0]


def test_fused_folded_net_without_biases():
	"""fuse_first_linear(net, epilogue=True, fold_batchnorm=True) on a bfloat16 net whose first and last Linear layers have bias=False: the
	first layer runs with a zero bias and its epilogue, the heads end in TailLinear (folding gives the last layers the bias the BatchNorm's
	shift becomes).  Against the plain net in float64 on the same bfloat16 parameters, at the bfloat16 tolerance of
	test_fused_net_with_epilogue_and_folded_batchnorm."""
	net = _NoBiasNet(seed=7).cuda().eval().to(torch.bfloat16)
	assert net.shared_net[0].bias is None and net.policy_net[-1].bias is None and net.value_net[-1].bias is None
	fused = fuse_first_linear(net, epilogue=True, fold_batchnorm=True)
	assert isinstance(fused.merged_heads[-1], TailLinear) and fused.merged_heads[-1].out_features == 13
	assert isinstance(fused.modules[1][-1], TailLinear) and isinstance(fused.modules[2][-1], TailLinear)
	assert not any(isinstance(m, torch.nn.BatchNorm1d) for seq in fused.modules for m in seq)
	states = _pool()
	with torch.no_grad():
		want_p, want_v = copy.deepcopy(net).double()(cube.device.as_oh(states).double())
		tol = dict(rtol=0.06, atol=0.06 * float(want_v.abs().max()))
		for n in (len(states), 1):
			for kw in ({}, {"policy": False}, {"value": False}):
				got = fused(states[:n].contiguous(), **kw)
				got = got if isinstance(got, list) else [got]
				want = ([want_p[:n]] if kw.get("policy", True) else []) + ([want_v[:n]] if kw.get("value", True) else [])
				assert len(got) == len(want)
				for g, w in zip(got, want):
					assert g.shape == w.shape and g.dtype == torch.bfloat16
					assert torch.allclose(g.double(), w, **tol), (n, kw, float((g.double() - w).abs().max()))
