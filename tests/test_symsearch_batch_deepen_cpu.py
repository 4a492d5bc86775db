"""
DeviceSymBallSearchBatch(deepen=E) without a GPU: the argument, the new result fields, and the new entries' null checks.
  * `deepen` is checked as `DeviceSymBallSearch` checks it, before any engine exists; the plain batch does not take it;
  * `deepened` and `probes` exist before any call and after a call with no states;
  * the entries rk_sdeepenb_* are in the header, the binding and the library, and refuse a null engine.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceBallSearchBatch, DeviceSymBall, DeviceSymBallSearchBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_sdeepenb_set", "rk_sdeepenb_frontiers", "rk_sdeepenb_probe", "rk_sdeepenb_keys", "rk_sdeepenb_paths"]


@pytest.mark.parametrize("bad", (-1, 9, 2.5, True))
def test_deepen_is_checked_before_any_engine_exists(bad):
	ball = DeviceSymBall(2)
	with pytest.raises(ValueError, match="deepen must be an integer in 0..8"):
		DeviceSymBallSearchBatch(ball, deepen=bad)
	assert ball._h is None and not ball.built


def test_the_plain_batch_does_not_take_the_argument():
	with pytest.raises(TypeError):
		DeviceBallSearchBatch(DeviceGoalBall(2), deepen=1)


def test_result_fields_before_a_call_and_after_one_without_states():
	ball = DeviceSymBall(2)
	assert DeviceSymBallSearchBatch(ball).deepen == 0
	for deepen in (0, 8):
		b = DeviceSymBallSearchBatch(ball, searches=3, pops=7, deepen=deepen)
		assert b.deepen == deepen
		for _ in range(2):
			assert b.deepened.shape == (0,) and b.deepened.dtype == np.int64 and b.probes == 0 and type(b.probes) is int
			solved = b.search(np.zeros((0, 20), np.int8))
			assert solved.shape == (0,) and solved.dtype == bool
		assert b._h is None and ball._h is None and not ball.built


def test_entries_in_header_binding_and_library_and_null_engines():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	assert set(re.findall(r"\b(rk_sdeepenb_[a-z0-9_]+)\s*\(", text)) == set(ENTRIES)
	assert {s for s in _ffi.SIGNATURES if s.startswith("rk_sdeepenb_")} == set(ENTRIES)
	assert {s for s in exported if s.startswith("rk_sdeepenb_")} == set(ENTRIES)
	lib = _ffi.lib()
	buf = np.zeros(64, np.int64)
	calls = (("set", (None, 1)), ("frontiers", (None, buf.ctypes.data, None)), ("probe", (None, 1, buf.ctypes.data, None)),
	         ("keys", (None, buf.ctypes.data, None)),
	         ("paths", (None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 8, None)))
	for name, args in calls:
		assert getattr(lib, "rk_sdeepenb_" + name)(*args) == -1, name
		assert lib.rk_last_error().startswith(b"rk_sdeepenb_" + name.encode()), lib.rk_last_error()
