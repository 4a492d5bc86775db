"""
DeviceSymBallSearchBatch without a GPU: the rk_ssearchb_* entries are declared, bound and exported alike, each with the argument
list of its rk_bsearchb_* twin; the library refuses bad engine arguments, an unbuilt ball and null handles before it touches a
device; the constructor checks its arguments before anything is launched; the Evaluator batches exactly `DeviceSymBallSearch`
(not a subclass); and a call that has nothing to run, or that finds no device, makes nothing.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import (DeviceBallSearchBatch, DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch,
                                          DeviceSymBallSearchBatch)
from librubiks_amd.solving.evaluation import Evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_ssearchb_create", "rk_ssearchb_destroy", "rk_ssearchb_reset", "rk_ssearchb_run", "rk_ssearchb_status",
           "rk_ssearchb_paths", "rk_ssearchb_export"]


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	lib = _ffi.lib()
	assert set(re.findall(r"\b(rk_ssearchb_[a-z0-9_]+)\s*\(", text)) == set(ENTRIES)
	assert {s for s in _ffi.SIGNATURES if s.startswith("rk_ssearchb_")} == set(ENTRIES)
	assert {s for s in exported if s.startswith("rk_ssearchb_")} == set(ENTRIES)
	for name in ENTRIES:
		assert getattr(lib, name) is not None
		# entry for entry the argument list of rk_bsearchb_*
		assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES[name.replace("rk_ssearchb_", "rk_bsearchb_")]
	# the header's argument lists, with the ball's type exchanged
	decl = lambda prefix: {m.group(1): re.sub(r"\s+", " ", m.group(2)) for m in re.finditer(r"\b%s_([a-z]+)\s*\(([^)]*)\)" % prefix, text)}
	sym, plain = decl("rk_ssearchb"), decl("rk_bsearchb")
	assert set(sym) == set(plain) == {n.split("_")[-1] for n in ENTRIES}
	for name, args in sym.items():
		assert args.replace("rk_ssearchb_t", "rk_bsearchb_t").replace("rk_symball_t", "rk_ball_t") == plain[name], name


def test_create_refuses_bad_arguments_and_an_unbuilt_ball():
	lib = _ffi.lib()
	ball, h = C.c_void_p(), C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(ball), 2, 16, 0))          # created, not built: allocates nothing, needs no device
	try:
		# rk_bsearchb_create's limits, checked before the ball is looked at: slots 1..1024, capacity 2..0x3FFFFFF0, pops 1..2^22
		for n_slots, cap, pops in ((0, 1000, 16), (1025, 1000, 16), (-1, 1000, 16), (4, 1, 16), (4, 0x3FFFFFF1, 16), (4, 1000, 0),
		                           (4, 1000, (1 << 22) + 1)):
			assert lib.rk_ssearchb_create(C.byref(h), ball, n_slots, cap, pops) == -1 and h.value is None     # RK_EINVAL
		assert lib.rk_ssearchb_create(C.byref(h), None, 4, 1000, 16) == -1 and h.value is None
		assert lib.rk_ssearchb_create(None, ball, 4, 1000, 16) == -1
		# the limits themselves pass the range checks and reach the ball: RK_ESTATE, nothing is made, nothing is attached
		for n_slots, cap, pops in ((4, 1000, 16), (1, 2, 1), (1024, 0x3FFFFFF0, 1 << 22)):
			assert lib.rk_ssearchb_create(C.byref(h), ball, n_slots, cap, pops) == -4 and h.value is None
			assert b"rk_ssearchb_create: build the ball first" in lib.rk_last_error()
	finally:
		assert lib.rk_symball_destroy(ball) == 0                           # no batch holds it


def test_null_handles_get_the_plain_batch_codes():
	lib = _ffi.lib()
	buf = np.zeros(64, np.int64)
	calls = (("reset", (None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None)), ("run", (None, 1, None)),
	         ("status", (None, buf.ctypes.data, None)), ("paths", (None, buf.ctypes.data, 8, None)),
	         ("export", (None, 0, 1, 1, None, buf.ctypes.data, None, None)), ("destroy", (None,)))
	for name, args in calls:
		got = getattr(lib, "rk_ssearchb_" + name)(*args)
		text = lib.rk_last_error()
		assert got == getattr(lib, "rk_bsearchb_" + name)(*args), name
		assert got == (0 if name == "destroy" else -1), name
		if name != "destroy":
			assert text.startswith(b"rk_ssearchb_" + name.encode()), text


@pytest.mark.parametrize("kw", [dict(searches=0), dict(searches=1025), dict(searches=True), dict(searches=2.5),
                                dict(pops=0), dict(pops=-3), dict(pops=1.5), dict(pops=(1 << 22) + 1), dict(pops=True),
                                dict(capacity=1), dict(capacity=2.5), dict(capacity=1 << 31), dict(capacity=True),
                                dict(poll=0), dict(poll=True)])
def test_bad_arguments_are_refused_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceSymBallSearchBatch(DeviceSymBall(2), **kw)


def test_constructor():
	ball = DeviceSymBall(3, pops=5)
	b = DeviceSymBallSearchBatch(ball, searches=5, pops=7, capacity=1_000, poll=3)
	assert b.ball is ball and (b.searches, b.pops, b.capacity, b.poll) == (5, 7, 1_000, 3)
	assert b._h is None and len(b) == 0 and b.on_poll is None and b.lockstep_iterations == 0 and not ball.built
	assert b.status.shape == (0, 10) and b.lengths.shape == (0,) and b.meeting_depths.shape == (0,) and b.meeting_nodes.shape == (0,)
	for name in ("sizes", "iterations", "popped", "stops", "depths"):
		assert getattr(b, name).shape == (0,)
	assert b.capacity_exhausted.dtype == bool and b.capacity_exhausted.shape == (0,)
	assert str(b) == "Breadth-first searches to a symmetry-reduced goal ball x5 (device, radius=3, pops=7)"
	d = DeviceSymBallSearchBatch(ball)
	assert (d.searches, d.pops, d.capacity, d.poll) == (64, 2_048, None, 8)
	assert (DeviceSymBallSearchBatch.MAX_SEARCHES, DeviceSymBallSearchBatch.MAX_POPS, DeviceSymBallSearchBatch.MAX_CAPACITY) == (
		DeviceBallSearchBatch.MAX_SEARCHES, DeviceBallSearchBatch.MAX_POPS, DeviceBallSearchBatch.MAX_CAPACITY)
	assert DeviceSymBallSearchBatch(ball, searches=1).searches == 1 and DeviceSymBallSearchBatch(ball, searches=1024).searches == 1024
	for wrong in (3, None, DeviceGoalBall(3), DeviceSymBallSearch(ball)):
		with pytest.raises(TypeError):
			DeviceSymBallSearchBatch(wrong)
	with pytest.raises(TypeError):
		DeviceBallSearchBatch(ball)                                        # the plain batch keeps refusing a symmetry ball
	assert not isinstance(b, DeviceBallSearchBatch) and not isinstance(DeviceBallSearchBatch(DeviceGoalBall(2)), DeviceSymBallSearchBatch)
	with pytest.raises(ValueError):
		b.arrays(0)
	# the shape of the input is checked before the device is asked for
	with pytest.raises(ValueError):
		b.search(np.zeros((3, 19), np.int8))
	with pytest.raises(ValueError):
		b.search(np.zeros((3, 20), np.int8), max_states=[5, 5])
	assert b._h is None and not ball.built


def test_evaluator_batches_exactly_the_symmetry_search():
	class Sub(DeviceSymBallSearch):
		pass
	ball = DeviceSymBall(2)
	assert Evaluator.can_batch(DeviceSymBallSearch(ball))
	assert not Evaluator.can_batch(Sub(ball))
	assert not Evaluator.can_batch(DeviceSymBallSearchBatch(ball)) and not Evaluator.can_batch(ball)
	b = Evaluator(4, [3], max_states=500)._batch_agent(DeviceSymBallSearch(ball, pops=7, poll=3), 4)
	assert type(b) is DeviceSymBallSearchBatch and b.ball is ball
	assert (b.searches, b.pops, b.poll, b.capacity) == (4, 7, 3, 500 + 12 * 7)      # the capacity rule used for DeviceBallSearch
	assert not ball.built


def test_nothing_to_run_touches_no_device(monkeypatch):
	ball = DeviceSymBall(2)
	b = DeviceSymBallSearchBatch(ball, searches=3, pops=7)
	solved = b.search(np.zeros((0, 20), np.int8), keep_arrays=True)
	assert solved.shape == (0,) and solved.dtype == bool and b._h is None and ball._h is None and not ball.built
	assert b.lengths.shape == (0,) and b.status.shape == (0, 10) and b.meeting_depths.shape == (0,) and b.meeting_nodes.shape == (0,)
	assert b.lockstep_iterations == 0 and len(b) == 0
	with pytest.raises(IndexError):
		b.action_queue_of(0)
	# 6x8x6 states are checked (and converted) by a launch of their own before the engine is asked for: without a device that is where
	# the call ends, with nothing made; with one an illegal state is a ValueError there (tests/test_symsearch_batch_gpu.py: test_edges)
	monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a machine that has a device: as if it had none)
	monkeypatch.setattr(_ffi, "_gpu_seen", False)
	cube.set_is2024(False)
	solved_686 = np.asarray(cube.get_solved())
	bad = np.stack([solved_686, np.zeros((6, 8, 6), np.int8), solved_686])
	with pytest.raises(_ffi.RubiksHipError):
		b.search(bad)
	assert b._h is None and ball._h is None and not ball.built and b.status.shape == (0, 10)
	cube.set_is2024(True)
	with pytest.raises(_ffi.RubiksHipError):
		b.search(np.zeros((2, 20), np.int8))
	assert b._h is None and ball._h is None and not ball.built
