"""
The bounds of tests/oh_linear_ref.py have teeth (no GPU, no HIP call): every route of the fused first layer is EMULATED here in torch
float32 on the CPU -- sequential float32 adds in the kernel's order, expm1 in float32, `.to(torch.bfloat16)` as the nearest-even
rounding -- and must pass its assert helper with no element left out; each subtly wrong variant of the emulation (a kernel bug that
the older tolerances let through) must be rejected by the SAME helper.  tests/test_oh_linear_exact_gpu.py then holds the kernels to
these helpers.
"""
import numpy as np
import pytest
import torch

from tests import oh_linear_ref as R
from tests.helpers import random_walk

SEED = 11               # layer / state seed: gives well over 100 pre-activations in (-0.1, -1e-3) at both widths (asserted below)


def _states():
	return torch.from_numpy(np.concatenate([R.cover_states(SEED), random_walk(300, 15, seed=SEED)]))


def _layer(H, seed=SEED):
	torch.manual_seed(seed)
	lin = torch.nn.Linear(480, H)
	torch.nn.init.xavier_uniform_(lin.weight)
	torch.nn.init.uniform_(lin.bias, -0.5, 0.5)
	return lin.weight.detach().clone(), lin.bias.detach().clone()


def _affine(H, seed=3):
	"""scale and shift as batchnorm_affine returns them (float32), of both signs"""
	g = torch.Generator().manual_seed(seed)
	scale = (torch.rand(H, generator=g) + 0.5) * torch.where(torch.rand(H, generator=g) < 0.25, -1.0, 1.0)
	return scale.float(), (torch.randn(H, generator=g) * 0.3).float()


def _sum32(states, w32, b32, wrong_row=None):
	"""((b + w_0) + w_1) + ... + w_19 in float32, the gather kernel's order.  wrong_row = cubie: its code 23 reads row 22 (mutant)."""
	wt = w32.t().contiguous()
	codes = states.long().clone()
	if wrong_row is not None:
		codes[:, wrong_row] = torch.where(codes[:, wrong_row] == 23, torch.full_like(codes[:, wrong_row], 22), codes[:, wrong_row])
	idx = codes + 24 * torch.arange(20)
	acc = b32.expand(len(states), wt.shape[1]).clone()
	for i in range(20):
		acc = acc + wt[idx[:, i]]
	return acc


def _epilogue32(x, act, alpha, scale, shift, exp_minus_one=False, nan_to_zero=False):
	"""The kernel's epilogue in float32: ELU through expm1 (exp_minus_one: exp(x) - 1, the cancelling form), a multiply and an add.
	nan_to_zero: the select `x > 0 ? x : alpha e(min(x, 0))`, which sends a NaN to alpha * 0 (ReLU: 0)."""
	a = x
	if act == "elu":
		neg = torch.where(x < 0, x, torch.zeros_like(x))
		e = torch.exp(neg) - 1.0 if exp_minus_one else torch.expm1(neg)
		a = torch.where(x > 0, x, alpha * e) if nan_to_zero else torch.where(~(x <= 0), x, alpha * e)
	elif act == "relu":
		a = torch.where(x > 0, x, torch.zeros_like(x)) if nan_to_zero else torch.where(x < 0, torch.zeros_like(x), x)
	if scale is not None:
		a = a * scale
		a = a + shift
	return a


def _truncate_bf16(y32):
	return (y32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)         # exact: the low 16 bits are gone already


def _rejected(fn, *args, **kw):
	with pytest.raises(AssertionError, match="out of bound"):
		fn(*args, **kw)


CASES = [(a, aff) for a in (None, "elu", "elu0.7", "relu") for aff in (False, True)]


@pytest.mark.parametrize("H", [64, 192])
def test_faithful_emulations_pass_and_mutants_are_rejected(H):
	states = _states()
	assert len(states) == 780
	w, b = _layer(H)
	scale_shift = _affine(H)

	# ---- the float32 sum (gather route, no epilogue), with and without bias
	x, mag = R.first_layer64(states, w, b)
	x32 = _sum32(states, w, b)
	R.assert_f32_preactivation(x32, x, mag)
	x0, mag0 = R.first_layer64(states, w, None)
	R.assert_f32_preactivation(_sum32(states, w, torch.zeros(H)), x0, mag0)
	assert torch.equal(x0 + b.double(), x) or (x0 + b.double() - x).abs().max() < 1e-15
	_rejected(R.assert_f32_preactivation, _sum32(states, w, b, wrong_row=7), x, mag)         # code 23 of cubie 7 reads row 22
	dropped = b.clone()
	dropped[-32:] = 0.0
	_rejected(R.assert_f32_preactivation, _sum32(states, w, dropped), x, mag)                # the bias dropped for the last 32 columns
	_rejected(R.assert_f32_preactivation, x32, x0, mag0)                                     # ... or added where the layer has none

	# ---- the float32 epilogue on its own
	teeth = R.elu_teeth(x32)
	assert teeth >= 100, teeth                                                                # the ELU cases below can tell expm1 from exp - 1
	for name, affine in CASES:
		act, alpha = R.ACTS[name]
		scale, shift = scale_shift if affine else (None, None)
		kw = dict(act=act, alpha=alpha, scale=scale, shift=shift)
		R.assert_f32_epilogue(_epilogue32(x32, act, alpha, scale, shift), x32, **kw, what=f"{name} {affine}")
		if act == "elu":
			_rejected(R.assert_f32_epilogue, _epilogue32(x32, act, alpha, scale, shift, exp_minus_one=True), x32, **kw)
		if affine:                                                                            # scale and shift 32 columns off in the last tile
			s2, t2 = scale.clone(), shift.clone()
			s2[-32:], t2[-32:] = scale[-64:-32], shift[-64:-32]
			_rejected(R.assert_f32_epilogue, _epilogue32(x32, act, alpha, s2, t2), x32, **kw)

	# ---- bfloat16 outputs: the MFMA route (weights rounded to bfloat16) and the gather route with a bfloat16 output
	for route, wr in (("mfma", R.route_weight(w, "mfma")), ("gather", w)):
		xr, magr = R.first_layer64(states, wr, b)
		s32 = _sum32(states, wr, b)
		for name, affine in CASES:
			act, alpha = R.ACTS[name]
			scale, shift = scale_shift if affine else (None, None)
			kw = dict(act=act, alpha=alpha, scale=scale, shift=shift)
			what = f"{route} {name} {affine}"
			y32 = _epilogue32(s32, act, alpha, scale, shift, exp_minus_one=route == "mfma")  # the fast form, which T_exp pays for
			R.assert_bf16_output(y32.to(torch.bfloat16), xr, magr, **kw, what=what)
			R.assert_bf16_output(_epilogue32(s32, act, alpha, scale, shift).to(torch.bfloat16), xr, magr, **kw, what=what)
			_rejected(R.assert_bf16_output, _truncate_bf16(y32), xr, magr, **kw)              # truncation instead of nearest even
			wrong = _epilogue32(_sum32(states, wr, b, wrong_row=19), act, alpha, scale, shift)
			_rejected(R.assert_bf16_output, wrong.to(torch.bfloat16), xr, magr, **kw)
			nobias = _epilogue32(_sum32(states, wr, dropped), act, alpha, scale, shift)
			_rejected(R.assert_bf16_output, nobias.to(torch.bfloat16), xr, magr, **kw)
			if affine:
				s2, t2 = scale.clone(), shift.clone()
				s2[-32:], t2[-32:] = scale[-64:-32], shift[-64:-32]
				_rejected(R.assert_bf16_output, _epilogue32(s32, act, alpha, s2, t2).to(torch.bfloat16), xr, magr, **kw)
		if route == "mfma":                                                                   # the layer's own float32 weights are NOT what this route sums
			xf, magf = R.first_layer64(states, w, b)
			_rejected(R.assert_f32_preactivation, s32, xf, magf)


@pytest.mark.parametrize("H", [64, 192])
def test_a_nan_mapped_to_zero_is_rejected(H):
	"""A NaN in bias[:4] and one NaN weight that only some rows select: the faithful epilogue keeps them (and passes, NaN for NaN), the
	select that maps a NaN to alpha * 0 is rejected -- in float32 and behind the bfloat16 rounding, with and without the affine map."""
	states = _states()
	w, b = _layer(H)
	b[:4] = float("nan")
	w[9, 24 * 3 + 23] = float("nan")                                                          # cubie 3, code 23
	picked = states[:, 3] == 23
	assert picked.any() and not picked.all()
	x, mag = R.first_layer64(states, w, b)
	assert torch.isnan(x[:, :4]).all() and torch.equal(torch.isnan(x[:, 9]), picked) and not torch.isnan(x[:, 10:]).any()
	x32 = _sum32(states, w, b)
	R.assert_f32_preactivation(x32, x, mag)
	scale_shift = _affine(H)
	for name, affine in CASES:
		act, alpha = R.ACTS[name]
		scale, shift = scale_shift if affine else (None, None)
		kw = dict(act=act, alpha=alpha, scale=scale, shift=shift)
		good = _epilogue32(x32, act, alpha, scale, shift)
		assert torch.equal(torch.isnan(good), torch.isnan(R.epilogue64(x, **kw)))
		R.assert_f32_epilogue(good, x32, **kw)
		R.assert_bf16_output(good.to(torch.bfloat16), x, mag, **kw)
		if act is not None:
			lost = _epilogue32(x32, act, alpha, scale, shift, nan_to_zero=True)
			assert not torch.isnan(lost).any()
			_rejected(R.assert_f32_epilogue, lost, x32, **kw)
			_rejected(R.assert_bf16_output, lost.to(torch.bfloat16), x, mag, **kw)
	# and the other way round: a NaN the reference does not have
	fine_w, fine_b = _layer(H)
	xf, magf = R.first_layer64(states, fine_w, fine_b)
	_rejected(R.assert_f32_preactivation, x32, xf, magf)


def test_an_infinity_must_be_the_same_infinity():
	"""Where the reference is infinite every bound is infinite too (2^-8 |ref|, an infinite mag) and inf <= inf would accept anything:
	each helper takes only the same infinity there, and a finite value, the other infinity or a NaN is rejected -- alone and among
	thousands of good elements.  An emulated tail (float32 products and sums, nearest-even bfloat16) with a +inf and a -inf row passes;
	the same tail with the sign of one row's activations flipped (a wrong-signed infinity, which `isfinite` cannot see) does not.  The
	ratio a helper returns is a number, never a NaN."""
	inf, nan = float("inf"), float("nan")
	ref = torch.tensor([[inf, inf, -inf, 1.0]], dtype=torch.float64)
	mag = torch.tensor([[inf, inf, inf, 2.0]], dtype=torch.float64)
	good = torch.tensor([[inf, inf, -inf, 1.0]]).to(torch.bfloat16)
	assert R.assert_tail(good, ref, mag) == 0.0
	for col, v in ((0, 5.0), (0, -inf), (0, nan), (1, 3.0e38), (2, inf), (2, -3.0e38), (3, inf), (3, nan)):
		y = good.clone()
		y[0, col] = v
		_rejected(R.assert_tail, y, ref, mag)
	_rejected(R.assert_tail, torch.tensor([[5.0, -inf, inf, 1.0]]).to(torch.bfloat16), ref, mag)
	_rejected(R.assert_tail, good, ref, torch.full_like(mag, inf))                            # an infinite bound on a finite element binds nothing

	# the first layer's helpers: an infinite weight in one row's selection
	states = _states()
	w, b = _layer(64)
	w[5, 24 * 2 + 7] = inf                                                                    # output 5, cubie 2 at code 7
	w[6, 24 * 2 + 7] = -inf
	picked = states[:, 2] == 7
	assert picked.any() and not picked.all()
	x, mag = R.first_layer64(states, w, b)
	assert (x[picked, 5] == inf).all() and (x[picked, 6] == -inf).all() and torch.isfinite(x[~picked]).all()
	x32 = _sum32(states, w, b)
	r = R.assert_f32_preactivation(x32, x, mag)
	assert r == r and r <= 1.0
	row = int(picked.nonzero()[0])
	for col, v in ((5, 1.0), (5, -inf), (5, nan), (6, inf), (6, -3.0e38)):
		y = x32.clone()
		y[row, col] = v
		_rejected(R.assert_f32_preactivation, y, x, mag)
	# behind an epilogue: +inf pre-activations in a column of positive and one of negative scale (-inf behind the affine map)
	scale, shift = _affine(64)
	cols = (int((scale > 0).nonzero()[0]), int((scale < 0).nonzero()[0]))
	w, b = _layer(64)
	w[cols, 24 * 2 + 7] = inf
	x, mag = R.first_layer64(states, w, b)
	x32 = _sum32(states, w, b)
	for name, affine in CASES:
		act, alpha = R.ACTS[name]
		sc, sh = (scale, shift) if affine else (None, None)
		kw = dict(act=act, alpha=alpha, scale=sc, shift=sh)
		y = _epilogue32(x32, act, alpha, sc, sh)
		want = R.epilogue64(x, **kw)
		assert (want[picked][:, cols[0]] == inf).all() and (want[picked][:, cols[1]] == (-inf if affine else inf)).all()
		for helper, out, args in ((R.assert_f32_epilogue, y, (x32,)), (R.assert_bf16_output, y.to(torch.bfloat16), (x, mag))):
			r = helper(out, *args, **kw)
			assert r == r and r <= 1.0, (name, affine, r)
			for col in cols:
				for v in (0.0, 1.0e30, nan, -float(out[row, col])):                           # finite, a NaN, the other infinity
					wrong = out.clone()
					wrong[row, col] = v
					_rejected(helper, wrong, *args, **kw)

	# a tail: activation, 512 -> 13, with a +inf row and a -inf row among ordinary ones
	g = torch.Generator().manual_seed(5)
	a = (torch.randn(16, 512, generator=g) * 1.5).to(torch.bfloat16)
	a[6, 41], a[7, 78] = inf, -inf
	W = (torch.randn(13, 512, generator=g) * 0.05).to(torch.bfloat16)
	bias = (torch.randn(13, generator=g) * 0.1).to(torch.bfloat16)
	assert (W != 0).all()
	ref = a.double() @ W.double().t() + bias.double()
	mag = a.double().abs() @ W.double().abs().t() + bias.double().abs()
	assert torch.isinf(ref[6:8]).all() and torch.isfinite(ref[:6]).all() and torch.isfinite(ref[8:]).all()
	y = (a.float() @ W.float().t() + bias.float()).to(torch.bfloat16)
	r = R.assert_tail(y, ref, mag)
	assert r == r and r <= 1.0
	for r_ in (6, 7):
		flipped = a.clone()
		flipped[r_] = -flipped[r_]                                                            # an activation sign error on that row
		wrong = (flipped.float() @ W.float().t() + bias.float()).to(torch.bfloat16)
		assert torch.equal(torch.isfinite(wrong), torch.isfinite(ref))                        # ... which a finiteness check lets through
		_rejected(R.assert_tail, wrong, ref, mag)
		wrong = y.clone()
		wrong[r_, 3] = 0.25                                                                   # one finite output on an infinite row
		_rejected(R.assert_tail, wrong, ref, mag)


def test_cover_states_select_every_pair():
	rows = R.cover_states(SEED)
	assert rows.shape == (480, 20) and rows.dtype == np.int8 and rows.min() == 0 and rows.max() == 23
	assert (rows[np.arange(480), np.arange(480) // 24] == np.arange(480) % 24).all()
	hit = np.zeros((20, 24), dtype=bool)
	hit[np.arange(480) // 24, np.arange(480) % 24] = True
	assert hit.all()
	assert (R.cover_states(SEED) == rows).all() and (R.cover_states(SEED + 1) != rows).any()


def test_reference_is_the_one_hot_layer_and_torchs_activations():
	"""first_layer64 against the dense one-hot product in float64, epilogue64 against torch's own modules in float64 (eval-mode BatchNorm1d
	through batchnorm_affine), the edge values of the activations included."""
	from librubiks_amd.oh_linear import batchnorm_affine
	states = _states()[::7]
	w, b = _layer(64)
	oh = torch.zeros(len(states), 480, dtype=torch.float64)
	oh[torch.arange(len(states))[:, None], states.long() + 24 * torch.arange(20)] = 1.0
	x, mag = R.first_layer64(states, w, b)
	assert torch.allclose(x, oh @ w.double().t() + b.double(), rtol=0, atol=1e-14)
	assert torch.allclose(mag, oh @ w.double().abs().t() + b.double().abs(), rtol=0, atol=1e-14)
	bn = torch.nn.BatchNorm1d(64).double()
	with torch.no_grad():
		bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0); bn.weight.normal_(); bn.bias.normal_()
	bn.eval()
	scale, shift = batchnorm_affine(bn)
	with torch.no_grad():
		for name in (None, "elu", "elu0.7", "relu"):
			act, alpha = R.ACTS[name]
			m = R.module_of(name)
			want = bn(m(x) if m is not None else x)
			assert torch.allclose(R.epilogue64(x, act, alpha, scale, shift), want, rtol=1e-6, atol=1e-6)       # (scale, shift are float32)
			assert torch.equal(R.act64(x, act, alpha), m(x) if m is not None else x)
	edge = torch.tensor([0.0, -0.0, -2.0 ** -20, -2.0 ** -126, -100.0, float("inf"), float("-inf"), float("nan"), 3.0], dtype=torch.float64)
	e = R.act64(edge, "elu", 0.7)
	assert e[0] == 0 and e[1] == 0 and e[2] == 0.7 * np.expm1(-2.0 ** -20) and e[4] == 0.7 * np.expm1(-100.0) and e[5] == float("inf")
	assert e[6] == -0.7 and torch.isnan(e[7]) and e[8] == 3.0 and not torch.isnan(e[:7]).any()
	r = R.act64(edge, "relu")
	assert torch.equal(r[:7], torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, float("inf"), 0.0], dtype=torch.float64)) and torch.isnan(r[7]) and r[8] == 3.0
