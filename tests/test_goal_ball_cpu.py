"""
DeviceGoalBall and DeviceBallSearch without a GPU: arguments are checked before anything is launched, the rk_ball_* and
rk_bsearch_* entries are declared, bound and exported alike, null handles are refused, a search without a device raises, and the
plain-Python model of the two protocols (tests/ball_model.py) that the GPU tests compare against has the level sizes of the
quarter-turn Cayley graph and finds solutions as short as the two-sided model (tests/bibfs_model.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceBallSearch, DeviceGoalBall
from tests import ball_model as model
from tests import bibfs_model
from tests.test_bibfs_device_gpu import LEVELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALL_ENTRIES = ["rk_ball_create", "rk_ball_destroy", "rk_ball_build", "rk_ball_status", "rk_ball_export", "rk_ball_depth",
                "rk_ball_solve"]
SEARCH_ENTRIES = ["rk_bsearch_create", "rk_bsearch_destroy", "rk_bsearch_reset", "rk_bsearch_run", "rk_bsearch_status",
                  "rk_bsearch_grow", "rk_bsearch_size", "rk_bsearch_export", "rk_bsearch_path"]

_balls = {}


def _ball(radius: int):
	if radius not in _balls:
		_balls[radius] = model.build(radius)
	return _balls[radius]


@pytest.mark.parametrize("kw", [dict(radius=-1), dict(radius=9), dict(radius=True), dict(radius=2.5),
                                dict(radius=2, pops=0), dict(radius=2, pops=1.5), dict(radius=2, pops=(1 << 22) + 1),
                                dict(radius=2, pops=True)])
def test_bad_ball_arguments_are_refused_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceGoalBall(**kw)


@pytest.mark.parametrize("kw", [dict(pops=0), dict(pops=-3), dict(pops=1.5), dict(pops=(1 << 22) + 1), dict(pops=True),
                                dict(capacity=1), dict(capacity=0), dict(capacity=2.5), dict(capacity=1 << 31),
                                dict(max_capacity=1), dict(poll=0)])
def test_bad_search_arguments_are_refused_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceBallSearch(DeviceGoalBall(2), **kw)


def test_good_arguments():
	ball = DeviceGoalBall(3, pops=5)
	assert (ball.radius, ball.pops, ball._h, ball.built) == (3, 5, None, False)
	assert DeviceGoalBall(0).radius == 0 and DeviceGoalBall(8).pops == 16_384
	assert DeviceGoalBall.LEVELS[:8] == tuple(LEVELS) and sum(DeviceGoalBall.LEVELS[:8]) == 9_205_558
	assert str(ball) == "Goal ball (device, radius=3)"
	a = DeviceBallSearch(ball, pops=7, capacity=1_000, max_capacity=5_000, poll=3)
	assert a.ball is ball and (a.pops, a.capacity, a.max_capacity, a.poll) == (7, 1_000, 5_000, 3)
	assert len(a) == 0 and a._h is None and a.depth == 0 and a.meeting is None and a.meeting_depth is None
	assert str(a) == "Breadth-first search to a goal ball (device, radius=3, pops=7)"
	assert DeviceBallSearch(ball).max_capacity == DeviceBallSearch.max_capacity and DeviceBallSearch(ball).pops == 16_384
	with pytest.raises(TypeError):
		DeviceBallSearch(3)


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	lib = _ffi.lib()
	for prefix, entries in (("rk_ball_", BALL_ENTRIES), ("rk_bsearch_", SEARCH_ENTRIES)):
		assert set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)) == set(entries)
		assert {s for s in _ffi.SIGNATURES if s.startswith(prefix)} == set(entries)
		assert {s for s in exported if s.startswith(prefix)} == set(entries)
		for name in entries:
			assert getattr(lib, name) is not None


def test_library_refuses_bad_engine_arguments():
	lib = _ffi.lib()
	h = C.c_void_p()
	for radius, pops in ((-1, 16), (9, 16), (2, 0), (2, (1 << 22) + 1)):
		assert lib.rk_ball_create(C.byref(h), radius, pops) == -1 and h.value is None
	assert lib.rk_ball_create(None, 2, 16) == -1
	buf = np.zeros(32, np.int64)
	assert lib.rk_ball_build(None, 8, None) == -1
	assert lib.rk_ball_status(None, buf.ctypes.data) == -1
	assert lib.rk_ball_export(None, 1, 1, None, buf.ctypes.data, None, None) == -1
	assert lib.rk_ball_depth(None, buf.ctypes.data, 1, buf.ctypes.data, None) == -1
	assert lib.rk_ball_solve(None, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, None) == -1
	assert lib.rk_ball_destroy(None) == 0
	# a ball that is created but not built allocates nothing, needs no device, and refuses every use
	_ffi.check(lib.rk_ball_create(C.byref(h), 2, 16))
	try:
		assert lib.rk_ball_build(h, 0, None) == -1
		_ffi.check(lib.rk_ball_status(h, buf.ctypes.data))
		assert buf[:6].tolist() == [0, 0, 0, 2, 127, 0] and not buf[6:16].any()
		assert lib.rk_ball_export(h, 1, 1, None, buf.ctypes.data, None, None) == -4                  # RK_ESTATE: not built
		assert lib.rk_ball_depth(h, buf.ctypes.data, 1, buf.ctypes.data, None) == -4
		assert lib.rk_ball_solve(h, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, None) == -4
		s = C.c_void_p()
		assert lib.rk_bsearch_create(C.byref(s), None, 1000, 16) == -1 and s.value is None
		assert lib.rk_bsearch_create(C.byref(s), h, 1, 16) == -1 and s.value is None
		assert lib.rk_bsearch_create(C.byref(s), h, 0x3FFFFFF1, 16) == -1 and s.value is None
		assert lib.rk_bsearch_create(C.byref(s), h, 1000, 0) == -1 and s.value is None
		assert lib.rk_bsearch_create(None, h, 1000, 16) == -1
	finally:
		assert lib.rk_ball_destroy(h) == 0
	start = model.scramble(1, 3)
	assert lib.rk_bsearch_reset(None, start.ctypes.data, 100, None) != 0
	assert lib.rk_bsearch_run(None, 1, None) != 0
	assert lib.rk_bsearch_status(None, buf.ctypes.data, None) != 0
	assert lib.rk_bsearch_grow(None, 1000, None) != 0
	assert lib.rk_bsearch_export(None, 1, 1, None, buf.ctypes.data, None, None) != 0
	assert lib.rk_bsearch_path(None, buf.ctypes.data, 16, None) < 0
	assert lib.rk_bsearch_size(None) == 0
	assert lib.rk_bsearch_destroy(None) == 0


def test_search_without_a_gpu_raises(monkeypatch):
	monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a machine that has a device: as if it had none)
	monkeypatch.setattr(_ffi, "_gpu_seen", False)
	ball = DeviceGoalBall(2)
	agent = DeviceBallSearch(ball, pops=7)
	with pytest.raises(_ffi.RubiksHipError):
		agent.search(model.scramble(1, 1), max_states=100)
	assert agent._h is None and len(agent) == 0
	for use in (ball.build, lambda: len(ball), lambda: ball.level_start, lambda: ball.depth(model.scramble(1, 1)[None]),
	            lambda: ball.solve(model.scramble(1, 1)[None]), ball.arrays):
		with pytest.raises(_ffi.RubiksHipError):
			use()
	assert ball._h is None and not ball.built


@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4])
def test_model_ball_has_the_level_sizes_of_the_graph(radius):
	ball = _ball(radius)
	assert np.diff(ball.level_start).tolist() == LEVELS[:radius + 1]
	assert ball.len == sum(LEVELS[:radius + 1]) == len(ball.states) == len(ball.index) and ball.level_start[0] == 1
	assert (ball.states[0] == model.orc.SOLVED).all() and ball.parents[0] == 0 and ball.actions[0] == -1
	assert len({s.tobytes() for s in ball.states}) == ball.len
	# a child follows its parent, lies one level further out, and is its parent moved by its action
	for node in range(2, ball.len + 1, max(1, ball.len // 500)):
		p, a = int(ball.parents[node - 1]), int(ball.actions[node - 1])
		assert p < node and model.depth_of(ball, p) + 1 == model.depth_of(ball, node)
		assert (model.apply(ball.states[p - 1], [a]) == ball.states[node - 1]).all()
		queue = model.solve(ball, ball.states[node - 1])
		assert len(queue) == model.depth(ball, ball.states[node - 1]) == model.depth_of(ball, node)
		assert model.orc.is_solved(model.apply(ball.states[node - 1], queue))
	assert model.depth(ball, model.scramble(20_000, 20)) == -1 and model.solve(ball, model.scramble(20_000, 20)) is None


@pytest.mark.parametrize("radius", [0, 2, 4])
@pytest.mark.parametrize("moves", [1, 2, 3, 4, 5, 6, 7])
def test_model_search_is_as_short_as_the_two_sided_model(radius, moves):
	ball = _ball(radius)
	for seed in (0, 1):
		start = model.scramble(1000 * moves + seed, moves)
		want = bibfs_model.search(start)
		m = model.search(start, ball)
		assert m.result and len(m.queue) == len(want.queue) <= moves
		assert model.orc.is_solved(model.apply(start, m.queue))
		assert m.len == len(m.states) == len(m.parents) == len(m.actions) and (m.states[0] == start).all()
		inside = model.depth(ball, start)
		if inside >= 0:                                          # the ball holds the start: its path, nothing popped
			assert m.len == 1 and m.depth == 0 and m.meeting_depth == inside == len(m.queue) and (m.meeting == start).all()
		else:
			assert m.meeting_depth == radius and len(m.queue) == m.depth + 1 + radius
			assert (m.meeting == model.apply(start, m.queue[:m.depth + 1])).all()
			assert not any(s.tobytes() in ball.index for s in m.states)


def test_model_budget_and_pool_order():
	ball = _ball(2)
	start = model.scramble(7000, 7)
	full = model.search(start, ball)
	assert full.result and full.parents[0] == 0 and full.actions[0] == -1
	assert (full.parents[1:] < np.arange(2, full.len + 1)).all()
	for i in range(1, full.len, max(1, full.len // 300)):
		p, a = int(full.parents[i]), int(full.actions[i])
		assert (model.apply(full.states[p - 1], [a]) == full.states[i]).all()
	# a budget of one state stops before the first pop; one below the full size stops short with a prefix of the pool
	first = model.search(start, ball, max_states=1)
	assert not first.result and first.len == 1 and first.meeting is None and first.meeting_depth is None
	cut = model.search(start, ball, max_states=full.len // 2)
	assert not cut.result and cut.queue == [] and full.len // 2 <= cut.len < full.len // 2 + 12
	assert (cut.states == full.states[:cut.len]).all() and (cut.parents == full.parents[:cut.len]).all()
	# a start the ball holds needs no pop, so no budget refuses it
	inside = model.search(model.scramble(1, 2), ball, max_states=1)
	assert inside.result and inside.len == 1
