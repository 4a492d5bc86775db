"""
Shortening action queues against the goal ball, without a GPU: the plain-Python model (tests/shorten_model.py) that the GPU tests
compare against, on balls of radius 0-4 --
  * the result reaches the same state from a scrambled start and is no longer than the word;
  * shortening is idempotent, and a single pass gives a fixed point back unchanged;
  * at the fixed point every window of at most W moves whose state the ball holds has as many moves as that state's depth
    (checked by brute force over all windows, with depths looked up independently of the pass);
  * constructed cases: a word and its inverse, four equal turns, three equal turns, a ball path, a window inside the ball;
-- and the rk_bshorten_* entries: declared, bound and exported alike, arguments refused before anything is launched.
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
from librubiks_amd.solving.agents import DeviceGoalBall
from tests import ball_model
from tests import shorten_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_bshorten_scratch_bytes", "rk_bshorten"]
RADII = (0, 1, 2, 3, 4)
# (seed, scramble depth, inflated length, window): windows below, at and above the word's length
WORDS = [(0, 3, 12, None), (1, 6, 20, None), (2, 10, 40, 8), (3, 8, 30, 2), (4, 5, 25, 1), (5, 12, 70, 64), (6, 4, 16, 100)]


@functools.lru_cache(maxsize=None)
def _ball(radius: int):
	return ball_model.build(radius)


@functools.lru_cache(maxsize=None)
def _case(radius: int, k: int):
	seed, depth, target, window = WORDS[k]
	word = model.detour_word(seed, depth, target)
	return word, window, model.shorten(_ball(radius), word, window)


def _assert_locally_optimal(ball, word, window):
	W = max(len(word), 1) if window is None else window
	depths = model.window_depths(ball, word, W)
	assert all(d == j - i for (i, j), d in depths.items()), [(ij, d) for ij, d in depths.items() if d != ij[1] - ij[0]][:5]
	if ball.radius >= 1:
		assert all((i, i + 1) in depths for i in range(len(word)))


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("k", range(len(WORDS)))
def test_result_reaches_the_same_state_and_is_no_longer(radius, k):
	word, window, got = _case(radius, k)
	assert len(got) <= len(word) and all(0 <= a < 12 for a in got)
	start = ball_model.scramble(900 + k, 25)
	assert (ball_model.apply(start, got) == ball_model.apply(start, word)).all()


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("k", range(len(WORDS)))
def test_idempotent_and_a_fixed_point_of_one_pass(radius, k):
	word, window, got = _case(radius, k)
	assert model.shorten(_ball(radius), got, window) == got
	assert model.one_pass(_ball(radius), got, window) == got


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("k", range(len(WORDS)))
def test_fixed_point_is_locally_optimal_by_brute_force(radius, k):
	word, window, got = _case(radius, k)
	_assert_locally_optimal(_ball(radius), got, window)


def test_window_one_changes_nothing_and_passes_are_counted():
	word = model.detour_word(11, 6, 30)
	for radius in (0, 2):
		assert model.shorten(_ball(radius), word, 1) == word
	ball = _ball(2)
	assert model.shorten(ball, word, passes=0) == word
	one, full = model.one_pass(ball, word), model.shorten(ball, word)
	assert model.shorten(ball, word, passes=1) == one and len(full) <= len(one) < len(word)
	# a narrow window needs several passes: every pass cancels the innermost pair of w + inverse(w)
	w = [0, 2, 4, 6, 8]
	nested = w + model.inverse(w)
	assert [len(model.shorten(_ball(0), nested, 2, passes=p)) for p in range(7)] == [10, 8, 6, 4, 2, 0, 0]
	assert model.shorten(_ball(0), nested, 2) == []
	for bad in ([12], [-1], [0, 3, 12, 1]):
		with pytest.raises(ValueError):
			model.one_pass(ball, bad)
	with pytest.raises(ValueError):
		model.one_pass(ball, [0], 0)


@pytest.mark.parametrize("radius", RADII)
def test_constructed_cases(radius):
	ball = _ball(radius)
	assert model.shorten(ball, []) == []
	w = [int(a) for a in np.random.RandomState(5).randint(0, 12, 9)]
	assert model.shorten(ball, w + model.inverse(w)) == []                 # an identity loop, at any radius
	for a in range(12):
		assert model.shorten(ball, [a] * 4) == []
		assert model.shorten(ball, [a] * 3) == ([model.rev(a)] if radius >= 1 else [a] * 3)
		assert model.shorten(ball, [a]) == [a]
	# a ball path -- an optimal word of at most `radius` moves -- comes back unchanged, towards solved and away from it
	for node in range(1, ball.len + 1, max(1, ball.len // 40)):
		path = ball_model.ball_path(ball, node)
		assert model.shorten(ball, path) == path
		assert model.shorten(ball, model.ball_word(ball, node)) == model.ball_word(ball, node)
	# a word of at most W moves whose end state the ball holds comes out with that state's depth
	for seed in range(40):
		word = model.detour_word(100 + seed, seed % (radius + 1), 10 + seed % 7)      # a scramble inside the ball, with detours
		d = ball_model.depth(ball, ball_model.apply(model.orc.SOLVED, word))
		assert 0 <= d <= seed % (radius + 1)
		assert len(model.shorten(ball, word)) == d
		assert len(model.one_pass(ball, word, len(word))) == d            # the whole word is one window: one pass is enough


def test_radius_zero_removes_exactly_the_identity_loops():
	ball = _ball(0)
	word = model.detour_word(21, 8, 40)
	got = model.shorten(ball, word)
	start = ball_model.scramble(77, 20)
	assert (ball_model.apply(start, got) == ball_model.apply(start, word)).all() and len(got) < len(word)
	# no window of the result is the identity, and every move of the result is a move of the word, in order
	assert not model.window_depths(ball, got, len(got))
	it = iter(word)
	assert all(a in it for a in got)
	# a word without an identity loop stays as it is
	assert model.shorten(ball, [0, 2, 0, 2, 5, 7]) == [0, 2, 0, 2, 5, 7]


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	assert set(re.findall(r"\b(rk_bshorten[a-z0-9_]*)\s*\(", text)) == set(ENTRIES)
	assert {s for s in _ffi.SIGNATURES if s.startswith("rk_bshorten")} == set(ENTRIES)
	assert {s for s in exported if s.startswith("rk_bshorten")} == set(ENTRIES)
	for name in ENTRIES:
		assert getattr(_ffi.lib(), name) is not None


def test_library_refuses_bad_arguments_before_any_launch():
	lib = _ffi.lib()
	assert lib.rk_bshorten_scratch_bytes(3, 10, 4) == 3 * 10 * 4 + 8 + 3 * 11 * 2      # d(i, j) bytes rounded up to 16, then pred
	assert lib.rk_bshorten_scratch_bytes(0, 10, 4) == 0
	assert lib.rk_bshorten_scratch_bytes(1, 4096, 4096) == 4096 * 4096 + 4097 * 2
	for n, max_len, window in ((1, 0, 1), (1, 4097, 1), (1, 10, 0), (1, 10, 11), (1, 10, -1), ((1 << 30) // 10 + 1, 10, 1)):
		assert lib.rk_bshorten_scratch_bytes(n, max_len, window) == -1
	buf = np.zeros(64, np.int64)
	p = buf.ctypes.data
	assert lib.rk_bshorten(None, p, p, 1, 8, 8, p + 64, p, p, p, 1 << 20, None) == -1 and b"null ball" in lib.rk_last_error()
	h = C.c_void_p()
	_ffi.check(lib.rk_ball_create(C.byref(h), 2, 16))
	try:
		assert lib.rk_bshorten(h, p, p, 1, 8, 8, p + 64, p, p, p, 1 << 20, None) == -4          # RK_ESTATE: not built
		assert b"build the ball first" in lib.rk_last_error()
	finally:
		assert lib.rk_ball_destroy(h) == 0


@pytest.mark.parametrize("kw", [dict(window=0), dict(window=-2), dict(window=1.5), dict(window=True), dict(passes=-1), dict(passes=0.5)])
def test_method_refuses_bad_arguments_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceGoalBall(2).shorten([[0, 1]], **kw)


def test_method_refuses_bad_queues_and_needs_a_gpu(monkeypatch):
	ball = DeviceGoalBall(2)
	for bad in ([[12]], [[0, -1, 3]], [[1, 2], [3, 40]], [[0] * 4097]):
		with pytest.raises(ValueError):
			ball.shorten(bad)
	assert ball._h is None and not ball.built
	monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a machine that has a device: as if it had none)
	monkeypatch.setattr(_ffi, "_gpu_seen", False)
	with pytest.raises(_ffi.RubiksHipError):
		ball.shorten([[0, 1]])
