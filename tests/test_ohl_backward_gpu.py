"""
rk_ohl_backward and rk_ohl_set_weights (librubiks_amd/csrc/rk_oh_linear.hip) on the device, against the float64 reference of
tests/ohl_backward_ref.py built there by index_add.

  * integer-valued dY in [-8, 8] with n <= 2^15: every partial sum is an integer below 2^24, so ANY summation order is exact and dW, db must
    equal the float64 reference bit for bit.  n = 1, 2, 63, 64, 65, the 480 cover rows (every (cubie, code) bin hit), 4 097, and one row
    more than two full row ranges of a workgroup (2 * BACKWARD_MIN_ROWS + 1: three workgroups per column tile, the last with a single row,
    which is also the one-row tail behind the groups of four); H = 64 (one column tile), 192, 512;
  * real-valued dY within the derived bound count u magW / n u magB; the largest error / bound ratio is printed;
  * overwrite (outputs prefilled with NaN), codes out of range, a single NaN / infinity, +inf and -inf in one bin, bitwise reproducibility
    across calls and handles, n = 0, the argument checks (outputs untouched), and rk_ohl_set_weights against a fresh handle on all routes.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.oh_linear import BACKWARD_MIN_ROWS, OhLinear, backward_rows
from tests import oh_linear_ref as R
from tests import ohl_backward_ref as B

pytestmark = pytest.mark.gpu

SEED = 23
HS = (64, 192, 512)
TWO_RANGES = 2 * BACKWARD_MIN_ROWS + 1
NS = (1, 2, 63, 64, 65, 480, 4097, TWO_RANGES)


@functools.lru_cache(maxsize=None)
def _engine(H, seed=SEED):
	torch.manual_seed(seed + H)
	lin = torch.nn.Linear(480, H).cuda().requires_grad_(False)
	return OhLinear(lin, "gather")


@functools.lru_cache(maxsize=None)
def _states(n) -> torch.Tensor:
	if n == 480:
		return torch.from_numpy(R.cover_states(SEED)).cuda()
	return torch.from_numpy(R.random_states(n, SEED + n)).cuda()


@functools.lru_cache(maxsize=None)
def _dy(n, H, kind) -> torch.Tensor:
	g = torch.Generator().manual_seed(SEED + 7 * n + H)
	if kind == "int":
		return torch.randint(-8, 9, (n, H), generator=g).float().cuda()
	return torch.randn((n, H), generator=g, dtype=torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def _reference(n, H, kind):
	"""first_layer_grad64 of (_states(n), _dy(n, H, kind)): computed once, never written"""
	return B.first_layer_grad64(_states(n), _dy(n, H, kind))


def _backward(eng, states, dy, dw=None, db=None, fill=float("nan"), bias=True):
	"""one rk_ohl_backward into outputs prefilled with `fill` -> (dw, db)"""
	H = eng.out_features
	if dw is None:
		dw = torch.full((H, 480), fill, dtype=torch.float32, device="cuda")
	if db is None and bias:
		db = torch.full((H,), fill, dtype=torch.float32, device="cuda")
	_ffi.check(_ffi.lib().rk_ohl_backward(eng._h, states.data_ptr(), dy.data_ptr(), len(dy), dw.data_ptr(), db.data_ptr() if db is not None else None,
	                                      _ffi.stream_ptr()))
	return dw, db


def _bits(t):
	return t.contiguous().view(torch.int32)


def test_row_range_constant():
	"""the shapes below rely on it: no row range shorter than BACKWARD_MIN_ROWS, so TWO_RANGES rows are three ranges at every H here"""
	for H in HS:
		assert backward_rows(1, H) == BACKWARD_MIN_ROWS and backward_rows(TWO_RANGES, H) == BACKWARD_MIN_ROWS
		assert backward_rows(4097, H) >= BACKWARD_MIN_ROWS
	assert backward_rows(20000, 512) > BACKWARD_MIN_ROWS                     # 32 row ranges of 628 rows: the other arm of the plan
	assert backward_rows(20000, 512) % 4 == 0 and 32 * backward_rows(20000, 512) >= 20000 > 31 * backward_rows(20000, 512)


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_exact_on_integers(n, H):
	dW, dB, _, _, count = _reference(n, H, "int")
	dw, db = _backward(_engine(H), _states(n), _dy(n, H, "int"))
	assert float(dW.abs().max()) < 2 ** 24
	assert torch.equal(_bits(dw), _bits(dW.float())), int((dw.double() != dW).sum())
	assert torch.equal(_bits(db), _bits(dB.float()))
	if n == 480:
		assert int(count.min()) >= 1
	# a column no row selects is +0.0 (all bits zero), whatever the buffer held
	empty = (count == 0)
	assert int(_bits(dw)[:, empty].abs().max() if bool(empty.any()) else 0) == 0


def test_all_rows_the_same_state():
	n, H = 4097, 192
	row = _states(480)[100:101]
	states = row.expand(n, 20).contiguous()
	dy = _dy(n, H, "int")
	dw, db = _backward(_engine(H), states, dy)
	total = dy.double().sum(0)
	cols = (B.codes_of(row)[0] + 24 * torch.arange(20, device="cuda"))
	want = torch.zeros((H, 480), dtype=torch.float64, device="cuda")
	want[:, cols] = total[:, None]
	assert torch.equal(_bits(dw), _bits(want.float())) and torch.equal(_bits(db), _bits(total.float()))
	mask = torch.ones(480, dtype=torch.bool, device="cuda")
	mask[cols] = False
	assert int(mask.sum()) == 460 and int(_bits(dw)[:, mask].abs().max()) == 0        # exactly +0.0


@pytest.mark.parametrize("fill", [float("nan"), 7.5])
def test_outputs_are_overwritten(fill):
	n, H = 65, 64
	dW, dB, _, _, _ = _reference(n, H, "int")
	dw, db = _backward(_engine(H), _states(n), _dy(n, H, "int"), fill=fill)
	assert not bool(torch.isnan(dw).any()) and not bool(torch.isnan(db).any())
	assert torch.equal(_bits(dw), _bits(dW.float())) and torch.equal(_bits(db), _bits(dB.float()))
	dw2, none = _backward(_engine(H), _states(n), _dy(n, H, "int"), bias=False)        # db is nullable
	assert none is None and torch.equal(_bits(dw2), _bits(dw))


def test_codes_out_of_range_count_as_23():
	n, H = 260, 64
	st = R.random_states(n, SEED).astype(np.int16)
	rs = np.random.RandomState(SEED)
	hit = rs.rand(n, 20) < 0.3
	st[hit] = rs.randint(24, 256, size=int(hit.sum()))                      # bytes 24 .. 127 and, as int8, -128 .. -1
	st[0, :6] = [24, 127, 128, 255, 23, 100]
	states = torch.from_numpy(st.astype(np.uint8).view(np.int8)).cuda()
	assert bool((states < 0).any()) and bool((states >= 24).any())
	clamped = B.codes_of(states).to(torch.int8)
	assert int(clamped.max()) == 23 and int(clamped.min()) >= 0
	dy = _dy(n, H, "int")
	eng = _engine(H)
	dw, db = _backward(eng, states, dy)
	dW, dB, _, _, _ = B.first_layer_grad64(clamped, dy)
	assert torch.equal(_bits(dw), _bits(dW.float())) and torch.equal(_bits(db), _bits(dB.float()))
	dw_c, _ = _backward(eng, clamped.contiguous(), dy)
	assert torch.equal(_bits(dw), _bits(dw_c))
	# and that is the forward's reading of the same bytes: its output on the raw states is first_layer64 on the clamped codes
	lin = torch.nn.Linear(480, H).cuda().requires_grad_(False)
	x, mag = R.first_layer64(clamped, lin.weight, lin.bias)
	R.assert_f32_preactivation(OhLinear(lin, "gather")(states), x, mag)


@pytest.mark.parametrize("n,H", [(65, 64), (4097, 192), (20000, 512)])
def test_real_valued_within_the_derived_bound(n, H):
	ref = _reference(n, H, "real")
	dw, db = _backward(_engine(H), _states(n), _dy(n, H, "real"))
	ratio = B.assert_grad(dw, db, ref, f"n = {n}, H = {H}")
	print(f"rk_ohl_backward n = {n}, H = {H}: largest |error| / bound = {ratio:.4f}")
	assert ratio <= 1.0
	# reproducible: a second call and a second handle of the same H give the same bits
	dw2, db2 = _backward(_engine(H), _states(n), _dy(n, H, "real"))
	dw3, db3 = _backward(_engine(H, seed=SEED + 1), _states(n), _dy(n, H, "real"))
	for a, b in ((dw2, db2), (dw3, db3)):
		assert torch.equal(_bits(a), _bits(dw)) and torch.equal(_bits(b), _bits(db))


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_a_single_nonfinite_reaches_its_21_outputs_and_nothing_else(value):
	n, H, r, h = TWO_RANGES, 192, 300, 77
	states = _states(n)
	dy = _dy(n, H, "real").clone()
	dy[r, h] = value
	dw, db = _backward(_engine(H), states, dy)
	hitW = torch.zeros((H, 480), dtype=torch.bool, device="cuda")
	hitW[h, B.codes_of(states[r]) + 24 * torch.arange(20, device="cuda")] = True
	hitB = torch.zeros(H, dtype=torch.bool, device="cuda")
	hitB[h] = True
	same = (lambda t: torch.isnan(t)) if value != value else (lambda t: t == value)
	assert torch.equal(same(dw), hitW) and torch.equal(same(db), hitB)
	assert bool(torch.isfinite(dw[~hitW]).all()) and bool(torch.isfinite(db[~hitB]).all())
	B.assert_grad(dw, db, B.first_layer_grad64(states, dy))


def test_opposite_infinities_in_one_bin_are_nan():
	n, H, h = 65, 64, 5
	states = _states(n).clone()
	states[40] = states[3]
	dy = _dy(n, H, "real").clone()
	dy[3, h], dy[40, h] = float("inf"), float("-inf")
	dw, db = _backward(_engine(H), states, dy)
	ref = B.first_layer_grad64(states, dy)
	assert int(torch.isnan(ref[0]).sum()) == 20 and bool(torch.isnan(ref[1][h]))
	assert torch.equal(torch.isnan(dw), torch.isnan(ref[0])) and torch.equal(torch.isnan(db), torch.isnan(ref[1]))
	B.assert_grad(dw, db, ref)


def test_no_rows_writes_zeros():
	H = 192
	dw, db = _backward(_engine(H), torch.empty((0, 20), dtype=torch.int8, device="cuda"), torch.empty((0, H), device="cuda"))
	assert int(_bits(dw).abs().max()) == 0 and int(_bits(db).abs().max()) == 0


def test_arguments_are_checked_before_any_launch():
	n, H = 65, 64
	lib, eng, states, dy = _ffi.lib(), _engine(H), _states(n), _dy(n, H, "int")
	# the outputs lie INSIDE larger tensors prefilled with a sentinel: a launch on a shifted pointer would still write sentinel cells
	big_w = torch.full((H * 480 + 64,), 7.5, dtype=torch.float32, device="cuda")
	big_b = torch.full((H + 64,), 7.5, dtype=torch.float32, device="cuda")
	big_y = torch.cat([dy.reshape(-1), torch.zeros(64, device="cuda")])
	pw, pb, py, st = big_w.data_ptr() + 64, big_b.data_ptr() + 64, big_y.data_ptr(), _ffi.stream_ptr()
	assert pw % 16 == 0 and py % 16 == 0
	bad = [
		(None, states.data_ptr(), py, pw, "null handle"),
		(eng._h, None, py, pw, "null pointer"),
		(eng._h, states.data_ptr(), None, pw, "null pointer"),
		(eng._h, states.data_ptr(), py, None, "null pointer"),
		(eng._h, states.data_ptr(), py + 4, pw, "aligned"),
		(eng._h, states.data_ptr(), py + 8, pw, "aligned"),
		(eng._h, states.data_ptr(), py, pw + 4, "aligned"),
		(eng._h, states.data_ptr(), py, pw + 8, "aligned"),
	]
	for hh, s, y, w, msg in bad:
		assert lib.rk_ohl_backward(hh, s, y, n, w, pb, st) == -1, msg
		assert msg.encode() in lib.rk_last_error(), (msg, lib.rk_last_error())
	torch.cuda.synchronize()
	assert bool((big_w == 7.5).all()) and bool((big_b == 7.5).all())
	assert lib.rk_ohl_set_weights(None, dy.data_ptr(), _ffi.OH_F32, None, st) == -1
	assert lib.rk_ohl_set_weights(eng._h, None, _ffi.OH_F32, None, st) == -1
	assert lib.rk_ohl_set_weights(eng._h, dy.data_ptr(), _ffi.OH_F16, None, st) == -1
	# the same outputs, properly addressed: written
	assert lib.rk_ohl_backward(eng._h, states.data_ptr(), py, n, pw, pb, st) == 0
	dW, dB, _, _, _ = _reference(n, H, "int")
	assert torch.equal(big_w[16:16 + H * 480].reshape(H, 480), dW.float()) and torch.equal(big_b[16:16 + H], dB.float())
	assert bool((big_w[:16] == 7.5).all()) and bool((big_w[16 + H * 480:] == 7.5).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("epilogue", [False, True])
def test_set_weights_equals_a_fresh_handle(dtype, epilogue):
	H = 192
	g = torch.Generator().manual_seed(SEED)

	def layer():
		lin = torch.nn.Linear(480, H)
		with torch.no_grad():
			lin.weight.copy_(torch.randn((H, 480), generator=g) * 0.1)
			lin.bias.copy_(torch.randn(H, generator=g) * 0.3)
		return lin.cuda().to(dtype).requires_grad_(False)
	old, new = layer(), layer()
	scale = (torch.rand(H, generator=g) + 0.5).cuda()
	shift = torch.randn(H, generator=g).cuda()
	refreshed, fresh = OhLinear(old), OhLinear(new)
	for e in (refreshed, fresh):
		if epilogue:
			_ffi.check(_ffi.lib().rk_ohl_set_epilogue(e._h, _ffi.OHL_ACT_ELU, 1.0, scale.data_ptr(), shift.data_ptr(), _ffi.stream_ptr()))
	code = _ffi.OH_F32 if dtype == torch.float32 else _ffi.OH_BF16
	_ffi.check(_ffi.lib().rk_ohl_set_weights(refreshed._h, new.weight.data_ptr(), code, new.bias.data_ptr(), _ffi.stream_ptr()))
	for n in (65, 1000):
		states = _states(n)
		for route in ("gather", "mfma_direct", "mfma_tiled"):
			a, b = refreshed(states, route=route), fresh(states, route=route)
			assert a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
			                                          b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), (n, route)
			assert not torch.equal(a, OhLinear(old)(states, route=route))            # and the weights did change
