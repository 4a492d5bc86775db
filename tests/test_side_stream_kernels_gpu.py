"""
The symmetry kernels and the 6x8x6 kernels on a torch side stream behind a gate (tests/side_stream.py, pattern A) at 257 and 1000
states: rk_sym_canonical, rk_sym_conjugate, rk_as_correct686, rk_oh686_from2024 (float32 and bfloat16), rk_686_to2024 and the 6x8x6
fan-out with flags and statistics.  The states arrive BEHIND the gate over other legal states, the outputs start as sentinel bytes,
and everything is compared bit for bit with the same call on the default stream (which tests/test_sym_gpu.py and
tests/test_repr686_kernels_gpu.py pin against the models).
"""
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from tests import side_stream as S

pytestmark = pytest.mark.gpu

NS = (257, 1000)


@functools.lru_cache(maxsize=None)
def _states(n, seed=0) -> torch.Tensor:
	"""legal 20-byte states 0 .. 9 moves deep (symmetric ones near solved among them), on the device"""
	return torch.from_numpy(S.mixed_depths(n, 9, 77 + n + seed)).cuda()


def _decoy(n) -> torch.Tensor:
	d = _states(n, seed=1).clone()
	assert not torch.equal(d, _states(n))
	return d


def _gated(true: torch.Tensor, buf: torch.Tensor, enqueue, before=None):
	"""pattern A, steps 2 to 4: on a side stream the gate, the true inputs over the decoy, `enqueue`, the gate still closed, then wait"""
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		ev = S.gate(s)
		buf.copy_(true, non_blocking=True)
		if before is not None:
			before()
		enqueue()
		S.held(ev)
		s.synchronize()


def _canonical(q, rep, sym, orbit):
	_ffi.check(_ffi.lib().rk_sym_canonical(q.data_ptr(), len(q), rep.data_ptr(), sym.data_ptr(), orbit.data_ptr(), _ffi.stream_ptr()))


def _conjugate(q, k, out):
	_ffi.check(_ffi.lib().rk_sym_conjugate(q.data_ptr(), len(q), k, out.data_ptr(), _ffi.stream_ptr()))


@pytest.mark.parametrize("n", NS)
def test_sym_canonical(n):
	true, buf = _states(n), _decoy(n)
	want = [torch.empty((n, 20), dtype=torch.int8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")]
	_canonical(true, *want)
	got = [S.sentinel(w.shape, w.dtype) for w in want]
	_gated(true, buf, lambda: _canonical(buf, *got))
	for a, b in zip(got, want):
		assert S.same_bits(a, b)
	assert int(want[2].min()) < 48 and int(want[1].max()) > 0            # symmetric states and other symmetries than the identity occur


@pytest.mark.parametrize("n", NS)
def test_sym_conjugate(n):
	true, buf = _states(n), _decoy(n)
	for k in (0, 17, 47):
		want = torch.empty((n, 20), dtype=torch.int8, device="cuda")
		_conjugate(true, k, want)
		got = S.sentinel((n, 20), torch.int8)
		buf.copy_(_decoy(n))
		_gated(true, buf, lambda: _conjugate(buf, k, got))
		assert S.same_bits(got, want), k
		assert (k == 0) == torch.equal(want, true)


@pytest.mark.parametrize("dtype", [torch.int8, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", NS)
def test_to686_and_back(n, dtype):
	"""rk_oh686_from2024 into int8 states, float32 and bfloat16 one-hot rows; rk_686_to2024 on the int8 form with its statistics"""
	true, buf = _states(n), _decoy(n)
	want = cube.device.to686(true, dtype)
	got = S.sentinel(want.shape, dtype)
	_gated(true, buf, lambda: cube.device.to686(buf, dtype, out=got))
	assert S.same_bits(got, want)
	if dtype != torch.int8:
		return
	true6, buf6 = want, cube.device.to686(_decoy(n))
	bad = true6.clone()
	bad[n // 2, 0, 0] = 0                                                # one row that is no legal state: written as -1 bytes and counted
	stats_w = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")
	want20 = cube.device.from686(bad, stats=stats_w)
	assert stats_w.tolist() == [1, n // 2] and torch.equal(want20[:n // 2], true[:n // 2])
	stats = torch.tensor([5, 3], dtype=torch.int64, device="cuda")       # a decoy's counts; the initial pair arrives behind the gate
	init = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")
	got20 = S.sentinel((n, 20), torch.int8)
	_gated(bad, buf6, lambda: cube.device.from686(buf6, out=got20, stats=stats), before=lambda: stats.copy_(init, non_blocking=True))
	assert S.same_bits(got20, want20) and stats.tolist() == [1, n // 2]


@pytest.mark.parametrize("n", NS)
def test_as_correct686(n):
	true6, buf6 = cube.device.to686(_states(n)), cube.device.to686(_decoy(n))
	want = torch.empty((n, 6, 8), dtype=torch.float32, device="cuda")
	_ffi.check(_ffi.lib().rk_as_correct686(true6.data_ptr(), want.data_ptr(), n, _ffi.stream_ptr()))
	got = S.sentinel((n, 6, 8), torch.float32)
	_gated(true6, buf6, lambda: _ffi.check(_ffi.lib().rk_as_correct686(buf6.data_ptr(), got.data_ptr(), n, _ffi.stream_ptr())))
	assert S.same_bits(got, want)
	assert set(np.unique(want.cpu().numpy()).tolist()) == {-1.0, 1.0}


@pytest.mark.parametrize("n", NS)
def test_fanout686_with_flags_and_statistics(n):
	states = _states(n).clone()
	near = cube.device.multi_rotate(torch.from_numpy(S.orc.repeat_state(S.orc.SOLVED, 2)).cuda(), torch.tensor([3, 8], dtype=torch.uint8, device="cuda"))
	states[5], states[n - 1] = near[0], near[1]                          # two parents one move from solved
	true6, buf6 = cube.device.to686(states), cube.device.to686(_decoy(n))
	cube.set_is2024(False)
	try:
		stats_w = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")
		want_ch, want_fl = cube.device.expand12(true6, stats=stats_w)
		assert int(want_fl.sum()) == stats_w[0].item() >= 2
		ch, fl = S.sentinel(want_ch.shape, torch.int8), S.sentinel(want_fl.shape, torch.uint8)
		stats = torch.tensor([5, 3], dtype=torch.int64, device="cuda")
		init = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")
		_gated(true6, buf6, lambda: cube.device.expand12(buf6, ch, fl, stats=stats), before=lambda: stats.copy_(init, non_blocking=True))
		assert S.same_bits(ch, want_ch) and S.same_bits(fl, want_fl) and stats.tolist() == stats_w.tolist()
		ch2 = S.sentinel(want_ch.shape, torch.int8)
		buf6.copy_(cube.device.to686(_decoy(n)))
		_gated(true6, buf6, lambda: cube.device.expand12(buf6, ch2, want_flags=False))
		assert S.same_bits(ch2, want_ch)
	finally:
		cube.set_is2024(True)
