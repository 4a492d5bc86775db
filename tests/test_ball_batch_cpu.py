"""
DeviceBallSearchBatch without a GPU: its arguments are checked before anything is launched, the Evaluator batches exactly
`DeviceBallSearch` (not a subclass), the rk_bsearchb_* entries are declared, bound and exported alike, and the library refuses
bad engine arguments before it touches a device.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceBallSearch, DeviceBallSearchBatch, DeviceGoalBall
from librubiks_amd.solving.evaluation import Evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_ENTRIES = ["rk_bsearchb_create", "rk_bsearchb_destroy", "rk_bsearchb_reset", "rk_bsearchb_run", "rk_bsearchb_status",
                 "rk_bsearchb_paths", "rk_bsearchb_export"]


@pytest.mark.parametrize("kw", [dict(searches=0), dict(searches=1025), dict(searches=True), dict(searches=2.5),
                                dict(pops=0), dict(pops=-3), dict(pops=1.5), dict(pops=(1 << 22) + 1), dict(pops=True),
                                dict(capacity=1), dict(capacity=2.5), dict(capacity=1 << 31), dict(capacity=True),
                                dict(poll=0), dict(poll=True)])
def test_bad_arguments_are_refused_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceBallSearchBatch(DeviceGoalBall(2), **kw)


def test_good_arguments_and_a_non_ball():
	ball = DeviceGoalBall(3, pops=5)
	b = DeviceBallSearchBatch(ball, searches=5, pops=7, capacity=1_000, poll=3)
	assert b.ball is ball and (b.searches, b.pops, b.capacity, b.poll) == (5, 7, 1_000, 3)
	assert b._h is None and len(b) == 0 and b.on_poll is None and not ball.built
	assert b.status.shape == (0, 10) and b.lengths.shape == (0,) and b.meeting_depths.shape == (0,)
	assert b.capacity_exhausted.dtype == bool and b.capacity_exhausted.shape == (0,)
	assert str(b) == "Breadth-first searches to a goal ball x5 (device, radius=3, pops=7)"
	d = DeviceBallSearchBatch(ball)
	assert (d.searches, d.capacity, d.poll) == (64, None, 8) and 1 <= d.pops <= DeviceBallSearchBatch.MAX_POPS
	assert DeviceBallSearchBatch(ball, searches=1).searches == 1 and DeviceBallSearchBatch(ball, searches=1024).searches == 1024
	for bad in (3, None, DeviceBallSearch(ball)):
		with pytest.raises(TypeError):
			DeviceBallSearchBatch(bad)
	with pytest.raises(ValueError):
		b.arrays(0)
	# the shape of the input is checked before the device is asked for
	with pytest.raises(ValueError):
		b.search(np.zeros((3, 19), np.int8))
	with pytest.raises(ValueError):
		b.search(np.zeros((3, 20), np.int8), max_states=[5, 5])
	assert not ball.built


def test_evaluator_batches_exactly_the_ball_search():
	class Sub(DeviceBallSearch):
		pass
	ball = DeviceGoalBall(2)
	assert Evaluator.can_batch(DeviceBallSearch(ball))
	assert not Evaluator.can_batch(Sub(ball))
	assert not Evaluator.can_batch(DeviceBallSearchBatch(ball)) and not Evaluator.can_batch(ball)
	assert not ball.built
	b = Evaluator(4, [3], max_states=500)._batch_agent(DeviceBallSearch(ball, pops=7, poll=3), 4)
	assert type(b) is DeviceBallSearchBatch and b.ball is ball
	assert (b.searches, b.pops, b.poll, b.capacity) == (4, 7, 3, 500 + 12 * 7) and not ball.built


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	lib = _ffi.lib()
	assert set(re.findall(r"\b(rk_bsearchb_[a-z0-9_]+)\s*\(", text)) == set(BATCH_ENTRIES)
	assert {s for s in _ffi.SIGNATURES if s.startswith("rk_bsearchb_")} == set(BATCH_ENTRIES)
	assert {s for s in exported if s.startswith("rk_bsearchb_")} == set(BATCH_ENTRIES)
	for name in BATCH_ENTRIES:
		assert getattr(lib, name) is not None


def test_library_refuses_bad_engine_arguments():
	lib = _ffi.lib()
	ball, h = C.c_void_p(), C.c_void_p()
	buf = np.zeros(64, np.int64)
	_ffi.check(lib.rk_ball_create(C.byref(ball), 2, 16))
	try:
		for n_slots, cap, pops in ((0, 1000, 16), (1025, 1000, 16), (-1, 1000, 16), (4, 1, 16), (4, 0x3FFFFFF1, 16), (4, 1000, 0),
		                           (4, 1000, (1 << 22) + 1)):
			assert lib.rk_bsearchb_create(C.byref(h), ball, n_slots, cap, pops) == -1 and h.value is None     # RK_EINVAL
		assert lib.rk_bsearchb_create(C.byref(h), None, 4, 1000, 16) == -1 and h.value is None
		assert lib.rk_bsearchb_create(None, ball, 4, 1000, 16) == -1
	finally:
		assert lib.rk_ball_destroy(ball) == 0
	assert lib.rk_bsearchb_reset(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None) != 0
	assert lib.rk_bsearchb_run(None, 1, None) != 0
	assert lib.rk_bsearchb_status(None, buf.ctypes.data, None) != 0
	assert lib.rk_bsearchb_paths(None, buf.ctypes.data, 8, None) != 0
	assert lib.rk_bsearchb_export(None, 0, 1, 1, None, buf.ctypes.data, None, None) != 0
	assert lib.rk_bsearchb_destroy(None) == 0
