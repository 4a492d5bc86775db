"""
DeviceSymBall.shorten (engine rk_sshorten) on the GPU, against the plain-Python model (tests/symshorten_model.py) bit for bit:
  * symmetry balls of radius 0, 1, 3 and 4; one mixed batch per call (symshorten_model.mixed_batch: the queues of 0, 1, 2, 63, 64,
    65, 129 and 300 moves of tests/test_ball_shorten_gpu.py and four whose replaced segment has several shortest words); windows
    1 (nothing changes), 2, 8, 64 and None;
  * one pass of rk_sshorten called directly -- rows, padding, lengths and the error word -- equals one pass of the model, and the
    fixed point of the method equals the model's and is returned unchanged by a further call;
  * a reversed and duplicated batch gives the same result per queue; a batch forced through several scratch chunks equals the
    unchunked result;
  * against code that already ships: DeviceGoalBall(5).shorten gives the same lengths queue for queue, and the same states;
  * the bytes do not depend on the ball's `pops`;
  * misuse: an unbuilt ball, null pointers, output == input, window 0, max_len 4097, misaligned and too little scratch; an
    action 12 passed to the entry is reported and its queue comes back as it was -- and the ball still answers afterwards;
  * a DeviceSymBallSearch attached to the same ball gives the same result before and after: the ball is only read;
  * the 6x8x6 mode changes nothing: the method takes no states.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch
from tests import ball_model
from tests import sym_model
from tests import symshorten_model as model

pytestmark = pytest.mark.gpu

RADII = (0, 1, 3, 4)
WINDOWS = (1, 2, 8, 64, None)

_device_balls = {}


def _ball(radius: int) -> DeviceSymBall:
	"""One device ball per radius for the whole module (it is read-only once built)."""
	if radius not in _device_balls:
		_device_balls[radius] = DeviceSymBall(radius).build()
	return _device_balls[radius]


@functools.lru_cache(maxsize=None)
def _model_ball(radius: int):
	return sym_model.build(radius)


@functools.lru_cache(maxsize=None)
def _words() -> tuple:
	return model.mixed_batch()


@functools.lru_cache(maxsize=None)
def _want(radius: int, window, passes) -> tuple:
	return tuple(tuple(model.shorten(_model_ball(radius), w, window, passes)) for w in _words())


def _lists(arrays) -> list:
	assert all(isinstance(a, np.ndarray) and a.dtype == np.int64 and a.ndim == 1 for a in arrays)
	return [a.tolist() for a in arrays]


def _one_pass_direct(ball: DeviceSymBall, words, window, max_len=None):
	"""rk_sshorten called directly: (rows (n, max_len) int8, lengths (n,) int32, error word)."""
	lib = _ffi.lib()
	n = len(words)
	max_len = max_len or max(len(w) for w in words)
	window = max_len if window is None else min(window, max_len)
	acts = np.full((n, max_len), -1, np.int8)
	for r, w in enumerate(words):
		acts[r, :len(w)] = w
	lens = torch.tensor([len(w) for w in words], dtype=torch.int32, device="cuda")
	d_acts = torch.from_numpy(acts).cuda()
	out = torch.full((n, max_len), 77, dtype=torch.int8, device="cuda")
	out_len = torch.full((n,), -5, dtype=torch.int32, device="cuda")
	err = torch.full((1,), 9, dtype=torch.int32, device="cuda")
	need = lib.rk_bshorten_scratch_bytes(n, max_len, window)                # one size and layout for both balls
	assert need > 0
	scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
	_ffi.check(lib.rk_sshorten(ball._h, d_acts.data_ptr(), lens.data_ptr(), n, max_len, window, out.data_ptr(), out_len.data_ptr(),
	                           err.data_ptr(), scratch.data_ptr(), need, _ffi.stream_ptr()))
	assert (d_acts.cpu().numpy() == acts).all()                          # the input is only read
	return out.cpu().numpy(), out_len.cpu().numpy(), int(err.item())


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("radius", RADII)
def test_one_pass_of_the_entry_equals_one_pass_of_the_model(radius, window):
	words = _words()
	assert [len(w) for w in words[:8]] == list(model.LENGTHS)
	want = _want(radius, window, 1)
	rows, lengths, err = _one_pass_direct(_ball(radius), words, window)
	assert err == 0 and lengths.tolist() == [len(w) for w in want]
	for r, w in enumerate(want):
		assert rows[r, :len(w)].tolist() == list(w) and (rows[r, len(w):] == -1).all()
	if window == 1:
		assert [list(w) for w in want] == [list(w) for w in words]
	# the method's single pass is the same pass
	assert _lists(_ball(radius).shorten(words, window=window, passes=1)) == [list(w) for w in want]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("radius", RADII)
def test_fixed_point_equals_the_model(radius, window):
	words = _words()
	want = _want(radius, window, None)
	got = _lists(_ball(radius).shorten(words, window=window))
	assert got == [list(w) for w in want]
	assert all(len(g) <= len(w) for g, w in zip(got, words))
	if window != 1:
		assert sum(map(len, got)) < sum(map(len, words))
	# a further call returns it unchanged, and the state from a scrambled start is the word's
	assert _lists(_ball(radius).shorten(got, window=window)) == got
	start = ball_model.scramble(321, 25)
	for g, w in zip(got, words):
		assert (ball_model.apply(start, g) == ball_model.apply(start, w)).all()


@pytest.mark.parametrize("radius", (0, 4))
def test_order_and_duplicates_do_not_matter(radius):
	words = list(_words())
	want = [list(w) for w in _want(radius, None, None)]
	batch = words[::-1] + words + [words[7], words[3]]
	got = _lists(_ball(radius).shorten(batch))
	assert got == want[::-1] + want + [want[7], want[3]]
	assert _lists(_ball(radius).shorten([])) == [] and _lists(_ball(radius).shorten([[], ()])) == [[], []]
	assert _lists(_ball(radius).shorten(words, passes=0)) == [list(w) for w in words]


@pytest.mark.parametrize("cap,window", [(1, None), (10_000, None), (1, 8), (10_000, 8)])
def test_a_batch_cut_into_scratch_chunks_equals_the_whole(monkeypatch, cap, window):
	"""A queue of 300 moves needs 90 602 bytes of scratch with every window and 3 002 with windows of 8: each cap cuts the first
	pass over the non-empty queues into several calls, none of which (but a call of a single queue) gets more than the cap."""
	ball = _ball(3)
	words = list(_words()) * 2
	busy = sum(1 for w in words if len(w))
	want = [list(w) for w in _want(3, window, None)] * 2
	lib = _ffi.lib()
	real, calls = lib.rk_sshorten, []
	monkeypatch.setattr(lib, "rk_sshorten", lambda *a: calls.append((a[3], a[10])) or real(*a))
	assert DeviceSymBall.shorten_scratch_bytes == 256 << 20
	assert _lists(ball.shorten(words, window=window)) == want
	whole = list(calls)
	assert whole[0][0] == busy and whole[0][1] <= 256 << 20                # one call for the first pass
	del calls[:]
	monkeypatch.setattr(ball, "shorten_scratch_bytes", cap, raising=False)
	assert _lists(ball.shorten(words, window=window)) == want
	assert len(calls) > len(whole) and calls[0][0] < busy
	assert all(n == 1 or scratch <= cap + 15 for n, scratch in calls)       # (+ 15: the d(i, j) bytes of a call are rounded up to 16)
	if cap == 1:
		assert max(n for n, _ in calls) == 1


def _apply_all(words) -> np.ndarray:
	"""The solved state after every word, by cube.multi_rotate: one call per position, over the words that reach it."""
	states = np.stack([cube.get_solved()] * len(words))
	for t in range(max(len(w) for w in words)):
		rows = [r for r, w in enumerate(words) if len(w) > t]
		acts = np.array([words[r][t] for r in rows], np.int64)
		states[rows] = cube.multi_rotate(states[rows], acts // 2, 1 - acts % 2)
	return states


def test_lengths_and_states_equal_the_plain_balls_at_radius_five():
	sball, pball = DeviceSymBall(5), DeviceGoalBall(5)
	words = [model.detour_word(200 + s, s % 21, 40 + s % 50) for s in range(64)]
	before = _apply_all(words)
	shortened = 0
	for window in (8, None):
		got, plain = _lists(sball.shorten(words, window=window)), _lists(pball.shorten(words, window=window))
		assert [len(g) for g in got] == [len(p) for p in plain]
		assert (_apply_all(got) == _apply_all(plain)).all() and (_apply_all(got) == before).all()
		shortened += sum(len(g) < len(w) for g, w in zip(got, words))
	assert shortened >= 64


def test_the_bytes_do_not_depend_on_pops():
	words = _words()
	a, b = DeviceSymBall(4, pops=7), DeviceSymBall(4, pops=4096)
	assert (a.arrays() == b.arrays()).all()
	for window in (8, None):
		one = _one_pass_direct(a, words, window)
		two = _one_pass_direct(b, words, window)
		assert (one[0] == two[0]).all() and (one[1] == two[1]).all() and one[2] == two[2] == 0
		assert _lists(a.shorten(words, window=window)) == _lists(b.shorten(words, window=window)) == [list(w) for w in _want(4, window, None)]


def test_misuse_is_refused_and_the_ball_still_answers():
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	ball = _ball(3)
	known = np.stack([ball_model.scramble(5, 2), ball_model.scramble(20_000, 20)])

	def still_answers():
		assert ball.depth(known).tolist() == [2, -1]

	for bad in ([[0, 12, 3]], [[1], [2, -1]], [[0] * 4097]):
		with pytest.raises(ValueError):
			ball.shorten(bad)
		still_answers()
	# the entry itself: the bad action indexes no table, is reported in the error word, and its queue comes back as it is
	words = [[0, 0, 0, 0, 5], [3, 12, 2, 2, 2, 2], [4, 5, 7], [1, -1, 0, 0, 0]]
	rows, lengths, err = _one_pass_direct(ball, words, None)
	assert err == -1 and lengths.tolist() == [1, 6, 1, 5]
	assert rows.tolist() == [[5, -1, -1, -1, -1, -1], [3, 12, 2, 2, 2, 2], [7, -1, -1, -1, -1, -1], [1, -1, 0, 0, 0, -1]]
	still_answers()
	rows, lengths, err = _one_pass_direct(ball, words[::2], None, max_len=9)   # and the next call's error word is clear again
	assert err == 0 and lengths.tolist() == [1, 1] and rows[:, 0].tolist() == [5, 7] and (rows[:, 1:] == -1).all()
	# an unbuilt ball, null pointers and sizes out of range
	acts = torch.zeros((1, 8), dtype=torch.int8, device="cuda")          # a queue of eight actions 0: two identity loops
	lens = torch.tensor([8], dtype=torch.int32, device="cuda")
	rows, n_out, word = torch.zeros((1, 8), dtype=torch.int8, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
	scratch = torch.zeros(1 << 10, dtype=torch.uint8, device="cuda")
	good = [ball._h, acts.data_ptr(), lens.data_ptr(), 1, 8, 8, rows.data_ptr(), n_out.data_ptr(), word.data_ptr(), scratch.data_ptr(), 1 << 10, stream]

	def call(**kw):
		names = ("h", "actions", "len", "n", "max_len", "window", "out", "out_len", "error", "scratch", "scratch_bytes", "stream")
		return lib.rk_sshorten(*[kw.get(name, v) for name, v in zip(names, good)])

	h = C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(h), 1, 8, 0))
	try:
		assert call(h=h) == -4 and b"rk_sshorten: build the ball first" in lib.rk_last_error()      # RK_ESTATE
	finally:
		assert lib.rk_symball_destroy(h) == 0
	assert call(h=None) == -1 and b"rk_sshorten: null ball" in lib.rk_last_error()
	still_answers()
	for name in ("actions", "len", "out", "out_len", "error", "scratch"):
		assert call(**{name: None}) == -1 and b"null pointer" in lib.rk_last_error()
		still_answers()
	for max_len, window in ((8, 0), (4097, 8), (8, 9), (0, 1)):
		assert call(max_len=max_len, window=window) == -1
		still_answers()
	assert call(scratch_bytes=63) == -1 and b"scratch" in lib.rk_last_error()
	assert call(out=acts.data_ptr()) == -1                                 # the output may not be the input
	assert call(scratch=scratch.data_ptr() + 4) == -1 and call(len=lens.data_ptr() + 1) == -1         # misaligned
	torch.cuda.synchronize()
	assert (n_out.item(), word.item()) == (1, 1)                           # nothing was launched by a refused call
	assert call(n=0, actions=None, len=None, out=None, out_len=None, scratch=None, scratch_bytes=0) == 0   # no queues: nothing to do
	_ffi.check(call())
	torch.cuda.synchronize()
	assert (n_out.item(), word.item()) == (0, 0) and (rows == -1).all().item()
	still_answers()


def test_a_search_attached_to_the_ball_is_undisturbed():
	ball = _ball(4)
	agent = DeviceSymBallSearch(ball, pops=64)
	start = ball_model.scramble(7003, 7)
	assert agent.search(start.copy())
	before = (list(agent.action_queue), len(agent))
	depth_before = ball.depth(np.stack([ball_model.scramble(s, 6) for s in range(50)]))
	arrays_before = ball.arrays().copy()
	got = _lists(ball.shorten(_words()))
	assert got == [list(w) for w in _want(4, None, None)]
	assert agent.search(start.copy())
	assert (list(agent.action_queue), len(agent)) == before
	assert (ball.depth(np.stack([ball_model.scramble(s, 6) for s in range(50)])) == depth_before).all()
	ball._cache = {}
	assert (ball.arrays() == arrays_before).all()
	# the search's solution is a shortest one: nothing to take away
	assert _lists(ball.shorten([before[0]])) == [before[0]]


def test_the_6x8x6_mode_gives_the_same_queues():
	ball = _ball(4)
	want = [list(w) for w in _want(4, 8, None)]
	assert _lists(ball.shorten(_words(), window=8)) == want
	try:
		cube.set_is2024(False)
		assert _lists(ball.shorten(_words(), window=8)) == want
	finally:
		cube.set_is2024(True)
