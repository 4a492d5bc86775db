"""
tests/ohl_backward_ref.py on the CPU: the derived bound (count u magW per element of dW, n u magB for db) accepts float32 emulations of the
sum in two different orders -- rows ascending, and four row ranges summed on their own and then added up, the shape of rk_ohl_backward --
and rejects five kernels that are each wrong in one small way.  No device, no library: plain torch.
"""
import numpy as np
import pytest
import torch

from tests import oh_linear_ref as R
from tests import ohl_backward_ref as B

N, H, SEED = 301, 64, 5


def _inputs():
	"""301 rows: cover rows (every bin hit), a few codes out of range (24, 100, 127, -1, -128), seeded normal dY"""
	st = np.concatenate([R.cover_states(SEED)[:281], R.random_states(20, SEED + 1)])
	st[3, 4], st[17, 0], st[50, 19], st[99, 7], st[200, 11] = 24, 100, 127, -1, -128
	dy = torch.randn((N, H), generator=torch.Generator().manual_seed(SEED), dtype=torch.float32)
	return torch.from_numpy(st), dy


def _emulate(states, dy, splits=1, clamp=True, db_bins=24):
	"""float32, the kernel's shape: per row range the bins' sums over ascending rows from +0.0, the ranges added in ascending order;
	db = the sum of cubie 0's first `db_bins` bins, ascending.  clamp=False drops codes >= 24 instead of counting them as 23."""
	n, Hh = dy.shape
	raw = states.long() & 0xFF
	idx = B.codes_of(states) + 24 * torch.arange(20)
	bounds = np.linspace(0, n, splits + 1).astype(int)
	total = None
	for s in range(splits):
		acc = torch.zeros((480, Hh), dtype=torch.float32)
		for r in range(bounds[s], bounds[s + 1]):
			cols = idx[r] if clamp else idx[r][raw[r] < 24]
			acc[cols] = acc[cols] + dy[r]                                # 20 different cubies: 20 different columns
		total = acc if total is None else total + acc
	db = total[0].clone()
	for v in range(1, db_bins):
		db = db + total[v]
	return total.t().contiguous(), db


def test_bound_accepts_two_summation_orders():
	st, dy = _inputs()
	ref = B.first_layer_grad64(st, dy)
	assert int(ref[4].min()) > 0 and int(ref[4].sum()) == 20 * N            # every bin hit; every row in one bin per cubie
	one = _emulate(st, dy, splits=1)
	four = _emulate(st, dy, splits=4)
	assert not torch.equal(one[0], four[0])                                 # the orders do differ in their roundings
	r1, r4 = B.assert_grad(*one, ref), B.assert_grad(*four, ref)
	assert 0 < r1 < 1 and 0 < r4 < 1


def test_bound_is_exact_on_integers_and_zero_on_empty_bins():
	st, dy = _inputs()
	st = st[:40]
	dyi = torch.randint(-8, 9, (40, H), generator=torch.Generator().manual_seed(1)).float()
	ref = B.first_layer_grad64(st, dyi)
	dw, db = _emulate(st, dyi, splits=4)
	assert torch.equal(dw.double(), ref[0]) and torch.equal(db.double(), ref[1])
	assert int((ref[4] == 0).sum()) > 0
	B.assert_grad(dw, db, ref)
	dw[:, int((ref[4] == 0).nonzero()[0])] = 1e-30                          # an empty bin must be exactly zero
	with pytest.raises(AssertionError):
		B.assert_grad(dw, db, ref)


def test_bound_rejects_last_row_dropped():
	st, dy = _inputs()
	with pytest.raises(AssertionError, match="dW"):
		B.assert_grad(*_emulate(st[:-1], dy[:-1], splits=4), B.first_layer_grad64(st, dy))


def test_bound_rejects_one_cubie_shifted_by_a_bin():
	st, dy = _inputs()
	off = st.clone()
	off[:, 7] = (B.codes_of(st)[:, 7] + 1) % 24
	with pytest.raises(AssertionError, match="dW"):
		B.assert_grad(*_emulate(off, dy, splits=4), B.first_layer_grad64(st, dy))


def test_bound_rejects_codes_out_of_range_dropped():
	st, dy = _inputs()
	with pytest.raises(AssertionError, match="dW"):
		B.assert_grad(*_emulate(st, dy, splits=4, clamp=False), B.first_layer_grad64(st, dy))


def test_bound_rejects_accumulating_into_stale_output():
	st, dy = _inputs()
	dw, db = _emulate(st, dy, splits=4)
	stale = torch.full_like(dw, 2.0 ** -10)
	with pytest.raises(AssertionError, match="dW"):
		B.assert_grad(dw + stale, db, B.first_layer_grad64(st, dy))
	# (db's bound, n u magB = 301 * 2^-24 * ~240, is about 4e-3: what is left in a gradient buffer is a gradient, of the order of 1)
	with pytest.raises(AssertionError, match="db"):
		B.assert_grad(dw, db + 0.5, B.first_layer_grad64(st, dy))


def test_bound_rejects_db_with_a_bin_missing():
	st, dy = _inputs()
	with pytest.raises(AssertionError, match="db"):
		B.assert_grad(*_emulate(st, dy, splits=4, db_bins=23), B.first_layer_grad64(st, dy))


def test_nonfinite_follow_the_reference():
	st, dy = _inputs()
	dy[5, 3], dy[6, 9], dy[7, 11], dy[8, 11] = float("nan"), float("inf"), float("inf"), float("-inf")
	st[8] = st[7]                                                           # +inf and -inf in the same 20 bins: NaN
	ref = B.first_layer_grad64(st, dy)
	assert int(torch.isnan(ref[0]).sum()) == 40 and int(torch.isinf(ref[0]).sum()) == 20
	assert torch.isnan(ref[1]).nonzero().flatten().tolist() == [3, 11] and torch.isinf(ref[1]).nonzero().flatten().tolist() == [9]
	dw, db = _emulate(st, dy, splits=4)
	B.assert_grad(dw, db, ref)
	dw[3, int(B.codes_of(st)[5, 0])] = 0.0                                  # a NaN lost
	with pytest.raises(AssertionError):
		B.assert_grad(dw, db, ref)
