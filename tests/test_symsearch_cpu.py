"""
DeviceSymBallSearch without a GPU: the plain-Python model of its protocol (tests/symsearch_model.py) against the model of the
plain search (tests/ball_model.py) on a plain ball of the same radius -- the own pool, the depth, the meeting and the length of
the queue are equal, only the ball's half of the queue may differ --; the rk_ssearch_* entries are declared, bound and exported
alike; null handles, bad capacities and pops and an unbuilt ball are refused; the constructor checks its arguments; and a search
without a device raises.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceBallSearch, DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch
from tests import ball_model
from tests import sym_model
from tests import symsearch_model as model

orc = ball_model.orc
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_ssearch_create", "rk_ssearch_destroy", "rk_ssearch_reset", "rk_ssearch_run", "rk_ssearch_status", "rk_ssearch_grow",
           "rk_ssearch_size", "rk_ssearch_export", "rk_ssearch_path"]
RADIUS = 3
#: 20-move scrambles whose prefixes of 1..8 moves lie, at radius 3, inside the ball (1..3 moves) and at own depths 0..4; seed 4's
#: prefix of 4 moves meets in the first child of the first pop, seed 33's prefixes of 6..8 moves have two meeting children in one batch
SEEDS = (0, 4, 33)


def starts() -> list:
	"""[(seed, moves, 20-byte start)]: every prefix of 1..8 moves of the three scrambles."""
	out = []
	for seed in SEEDS:
		acts = np.random.RandomState(seed).randint(0, 12, 20)
		out += [(seed, n, ball_model.apply(orc.SOLVED, acts[:n])) for n in range(1, 9)]
	return out


@functools.lru_cache(maxsize=None)
def sym_ball(radius: int = RADIUS):
	return sym_model.build(radius)


@functools.lru_cache(maxsize=None)
def modelled(seed: int, moves: int):
	"""(Result, popped) of the model for a start of `starts()`."""
	start = next(s for sd, n, s in starts() if (sd, n) == (seed, moves))
	return model.search(start, sym_ball())


def test_model_equals_the_plain_model_on_a_plain_ball():
	plain = ball_model.build(RADIUS)
	depths = set()
	for seed, moves, start in starts():
		got, popped = modelled(seed, moves)
		want = ball_model.search(start, plain)
		assert got.result is True and want.result is True
		assert (got.len, got.depth, got.meeting_depth) == (want.len, want.depth, want.meeting_depth), (seed, moves)
		assert (got.meeting == want.meeting).all()
		assert (got.states == want.states).all() and (got.parents == want.parents).all() and (got.actions == want.actions).all()
		assert len(got.queue) == len(want.queue) <= moves
		assert orc.is_solved(ball_model.apply(start, got.queue)) and orc.is_solved(ball_model.apply(start, want.queue))
		inside = ball_model.depth(plain, start) >= 0
		assert inside == (popped == 0)
		depths.add("inside" if inside else got.depth)
		# the own half is the same path; the meeting is the start moved along it
		own = len(got.queue) - got.meeting_depth
		assert got.queue[:own] == want.queue[:own] and (ball_model.apply(start, got.queue[:own]) == got.meeting).all()
	assert depths == {"inside", 0, 1, 2, 3, 4}
	# what the GPU test relies on: a meeting in the very first child, and two meeting children in one batch at own depth >= 2
	first, popped = modelled(4, 4)
	assert first.len == 1 and popped == 1 and first.depth == 0 and len(first.queue) == 4
	assert modelled(33, 6)[0].depth == 2 and model.meetings_in_batch(starts()[16 + 5][2], sym_ball(), 5) == 2


def test_model_budget():
	seed, moves, start = starts()[6]
	full, _ = modelled(seed, moves)
	plain = ball_model.build(RADIUS)
	for budget in (1, 13, full.len // 2, full.len - 12):         # (the pop that meets is the last one: it starts above len - 12)
		got, _ = model.search(start, sym_ball(), max_states=budget)
		want = ball_model.search(start, plain, max_states=budget)
		assert got.result is False and want.result is False and got.len == want.len and got.depth == want.depth
		assert (got.states == want.states).all() and got.meeting is None and got.queue == []
	assert model.search(start, sym_ball(), max_states=full.len)[0].result is True


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	lib = _ffi.lib()
	assert set(re.findall(r"\b(rk_ssearch_[a-z0-9_]+)\s*\(", text)) == set(ENTRIES)
	assert {s for s in _ffi.SIGNATURES if s.startswith("rk_ssearch_")} == set(ENTRIES)
	assert {s for s in exported if s.startswith("rk_ssearch_")} == set(ENTRIES)
	for name in ENTRIES:
		assert getattr(lib, name) is not None
		# entry for entry the argument list of rk_bsearch_*
		assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES[name.replace("rk_ssearch_", "rk_bsearch_")]


def test_library_refuses_bad_engine_arguments():
	lib = _ffi.lib()
	buf = np.zeros(32, np.int64)
	h, s = C.c_void_p(), C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(h), 2, 16, 0))         # created, not built: allocates nothing, needs no device
	try:
		# rk_bsearch_create's codes for a null argument, a capacity outside 2..0x3FFFFFF0 and pops outside 1..2^22
		assert lib.rk_ssearch_create(C.byref(s), None, 1000, 16) == -1 and s.value is None
		assert lib.rk_ssearch_create(C.byref(s), h, 1, 16) == -1 and s.value is None
		assert lib.rk_ssearch_create(C.byref(s), h, 0x3FFFFFF1, 16) == -1 and s.value is None
		assert lib.rk_ssearch_create(C.byref(s), h, 1000, 0) == -1 and s.value is None
		assert lib.rk_ssearch_create(C.byref(s), h, 1000, (1 << 22) + 1) == -1 and s.value is None
		assert lib.rk_ssearch_create(None, h, 1000, 16) == -1
		# a ball that is not built: RK_ESTATE, nothing is made, nothing is attached
		assert lib.rk_ssearch_create(C.byref(s), h, 1000, 16) == -4 and s.value is None
		assert b"build the ball first" in lib.rk_last_error()
	finally:
		assert lib.rk_symball_destroy(h) == 0
	start = model.scramble(1, 3)
	assert lib.rk_ssearch_reset(None, start.ctypes.data, 100, None) != 0
	assert lib.rk_ssearch_run(None, 1, None) != 0
	assert lib.rk_ssearch_status(None, buf.ctypes.data, None) != 0
	assert lib.rk_ssearch_grow(None, 1000, None) != 0
	assert lib.rk_ssearch_export(None, 1, 1, None, buf.ctypes.data, None, None) != 0
	assert lib.rk_ssearch_path(None, buf.ctypes.data, 16, None) < 0
	assert lib.rk_ssearch_size(None) == 0
	assert lib.rk_ssearch_destroy(None) == 0
	# the same codes as the plain engine's entries
	for name, args in (("reset", (None, start.ctypes.data, 100, None)), ("run", (None, 1, None)), ("status", (None, buf.ctypes.data, None)),
	                   ("grow", (None, 1000, None)), ("export", (None, 1, 1, None, buf.ctypes.data, None, None)),
	                   ("path", (None, buf.ctypes.data, 16, None)), ("size", (None,)), ("destroy", (None,))):
		assert getattr(lib, "rk_ssearch_" + name)(*args) == getattr(lib, "rk_bsearch_" + name)(*args), name


@pytest.mark.parametrize("kw", [dict(pops=0), dict(pops=-3), dict(pops=1.5), dict(pops=(1 << 22) + 1), dict(pops=True),
                                dict(capacity=1), dict(capacity=0), dict(capacity=2.5), dict(capacity=1 << 31),
                                dict(max_capacity=1), dict(poll=0)])
def test_bad_search_arguments_are_refused_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceSymBallSearch(DeviceSymBall(2), **kw)


def test_constructor():
	ball = DeviceSymBall(3, pops=5)
	a = DeviceSymBallSearch(ball, pops=7, capacity=1_000, max_capacity=5_000, poll=3)
	assert a.ball is ball and (a.pops, a.capacity, a.max_capacity, a.poll) == (7, 1_000, 5_000, 3)
	assert len(a) == 0 and a._h is None and a.depth == 0 and a.iterations == 0 and a.popped == 0 and a.grown == 0
	assert a.meeting is None and a.meeting_node is None and a.meeting_depth is None and a.capacity_exhausted is False
	assert str(a) == "Breadth-first search to a symmetry-reduced goal ball (device, radius=3, pops=7)"
	d = DeviceSymBallSearch(ball)
	assert (d.pops, d.capacity, d.poll) == (16_384, None, 8) and d.max_capacity == DeviceBallSearch.max_capacity
	for wrong in (3, None, DeviceGoalBall(3)):
		with pytest.raises(TypeError):
			DeviceSymBallSearch(wrong)
	with pytest.raises(TypeError):
		DeviceBallSearch(ball)                                   # the plain search keeps refusing a symmetry ball
	assert not isinstance(a, DeviceBallSearch) and not isinstance(DeviceBallSearch(DeviceGoalBall(2)), DeviceSymBallSearch)


def test_search_without_a_gpu_raises(monkeypatch):
	monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a machine that has a device: as if it had none)
	monkeypatch.setattr(_ffi, "_gpu_seen", False)
	ball = DeviceSymBall(2)
	agent = DeviceSymBallSearch(ball, pops=7)
	with pytest.raises(_ffi.RubiksHipError):
		agent.search(model.scramble(1, 1), max_states=100)
	assert agent._h is None and len(agent) == 0 and ball._h is None and not ball.built
