"""
DeviceGoalBall.shorten (engine rk_bshorten) and DeviceSymBall.shorten (engine rk_sshorten) on the GPU, each against its plain-Python
model (tests/shorten_model.py, tests/symshorten_model.py) bit for bit.  What both kinds of ball promise is stated once (tests/ball_kinds.py
names what differs); what the symmetry ball alone has is in tests/test_symball_shorten_gpu.py.
Both kinds:
  * balls of radius 0, 1, 3 and 4 (plain: 11 206 states); one mixed batch per call with queues of 0, 1, 2, 63, 64, 65, 129 and 300
    moves (the edges of a wave's 64-move chunk and a queue of several chunks) and, for the symmetry ball, four whose replaced
    segment has several shortest words (symshorten_model.mixed_batch); windows 1 (nothing changes), 2, 8, 64 and None;
  * one pass of the entry called directly -- rows, padding, lengths and the error word -- equals one pass of the model, and the
    fixed point of the method equals the model's and is returned unchanged by a further call: one body each in tests/ball_kinds.py,
    run here for the plain ball and in tests/test_symball_shorten_gpu.py for the symmetry ball;
  * a reversed and duplicated batch gives the same result per queue; a batch forced through several scratch chunks equals the
    unchunked result;
  * misuse: actions outside 0..11 (the method raises; the entry reports them, indexes no table and gives the queue back), an
    unbuilt ball, null pointers, output == input, window 0, max_len 4097, misaligned and too little scratch -- and the ball still
    answers afterwards;
  * a search (DeviceBallSearch, DeviceSymBallSearch) attached to the same ball gives the same result before and after: the ball
    is only read.
The plain ball alone:
  * the constructed cases of tests/test_ball_shorten_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from tests import ball_kinds
from tests import ball_model
from tests import shorten_model
from tests.ball_kinds import IDS, KINDS, PLAIN, device_ball, lists, model_ball, one_pass_direct, want_words, words

pytestmark = pytest.mark.gpu

RADII = (0, 1, 3, 4)
WINDOWS = (1, 2, 8, 64, None)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("radius", RADII)
def test_one_pass_of_the_entry_equals_one_pass_of_the_model(radius, window):
	ball_kinds.one_pass_of_the_entry_equals_one_pass_of_the_model(PLAIN, radius, window)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("radius", RADII)
def test_fixed_point_equals_the_model(radius, window):
	ball_kinds.fixed_point_equals_the_model(PLAIN, radius, window)


# ---- both kinds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", (0, 4))
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_order_and_duplicates_do_not_matter(kind, radius):
	ball = device_ball(kind, radius)
	batch = list(words(kind))
	want = [list(w) for w in want_words(kind, radius, None, None)]
	got = lists(ball.shorten(batch[::-1] + batch + [batch[7], batch[3]]))
	assert got == want[::-1] + want + [want[7], want[3]]
	assert lists(ball.shorten([])) == [] and lists(ball.shorten([[], ()])) == [[], []]
	assert lists(ball.shorten(batch, passes=0)) == [list(w) for w in batch]


@pytest.mark.parametrize("kind,cap,window", [pytest.param(k, cap, window, id=f"{k.name}-{cap}-{window}") for k in KINDS for cap, window in k.scratch_caps])
def test_a_batch_cut_into_scratch_chunks_equals_the_whole(monkeypatch, kind, cap, window):
	"""A queue of 300 moves needs 90 602 bytes of scratch with every window and 3 002 with windows of 8: each cap cuts the first
	pass over the non-empty queues (14 of the plain batch taken twice) into several calls, none of which (but a call of a single
	queue) gets more than the cap."""
	ball = device_ball(kind, 3)
	batch = list(words(kind)) * 2
	busy = sum(1 for w in batch if len(w))
	assert busy == 2 * (7 + kind.extra_words)
	want = [list(w) for w in want_words(kind, 3, window, None)] * 2
	lib = _ffi.lib()
	real, calls = getattr(lib, kind.shorten_entry), []
	monkeypatch.setattr(lib, kind.shorten_entry, lambda *a: calls.append((a[3], a[10])) or real(*a))
	assert kind.ball.shorten_scratch_bytes == 256 << 20
	assert lists(ball.shorten(batch, window=window)) == want
	whole = list(calls)
	assert whole[0][0] == busy and whole[0][1] <= 256 << 20              # one call for the first pass
	del calls[:]
	monkeypatch.setattr(ball, "shorten_scratch_bytes", cap, raising=False)
	assert lists(ball.shorten(batch, window=window)) == want
	assert len(calls) > len(whole) and calls[0][0] < busy
	assert all(n == 1 or scratch <= cap + kind.scratch_slack for n, scratch in calls)
	if kind is PLAIN or cap == 1:                                        # (the symmetry suite never asked this of its cap of 10 000)
		assert (max(n for n, _ in calls) == 1) == (cap == 1)


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_misuse_is_refused_and_the_ball_still_answers(kind):
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	entry = getattr(lib, kind.shorten_entry)
	ball = device_ball(kind, 3)
	known = np.stack([ball_model.scramble(5, 2), ball_model.scramble(20_000, 20)])

	def still_answers():
		assert ball.depth(known).tolist() == [2, -1]

	for bad in ([[0, 12, 3]], [[1], [2, -1]], [[0] * 4097]):
		with pytest.raises(ValueError):
			ball.shorten(bad)
		still_answers()
	# the entry itself: the bad action indexes no table, is reported in the error word, and its queue comes back as it is
	bad = [[0, 0, 0, 0, 5], [3, 12, 2, 2, 2, 2], [4, 5, 7], [1, -1, 0, 0, 0]]
	rows, lengths, err = one_pass_direct(kind, ball, bad, None)
	assert err == -1 and lengths.tolist() == [1, 6, 1, 5]
	assert rows.tolist() == [[5, -1, -1, -1, -1, -1], [3, 12, 2, 2, 2, 2], [7, -1, -1, -1, -1, -1], [1, -1, 0, 0, 0, -1]]
	still_answers()
	rows, lengths, err = one_pass_direct(kind, ball, bad[::2], None, max_len=9)   # and the next call's error word is clear again
	assert err == 0 and lengths.tolist() == [1, 1] and rows[:, 0].tolist() == [5, 7] and (rows[:, 1:] == -1).all()
	# an unbuilt ball, null pointers and sizes out of range
	acts = torch.zeros((1, 8), dtype=torch.int8, device="cuda")          # a queue of eight actions 0: two identity loops
	lens = torch.tensor([8], dtype=torch.int32, device="cuda")
	rows, n_out, word = torch.zeros((1, 8), dtype=torch.int8, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
	scratch = torch.zeros(1 << 10, dtype=torch.uint8, device="cuda")
	good = [ball._h, acts.data_ptr(), lens.data_ptr(), 1, 8, 8, rows.data_ptr(), n_out.data_ptr(), word.data_ptr(), scratch.data_ptr(), 1 << 10, stream]

	def call(**kw):
		names = ("h", "actions", "len", "n", "max_len", "window", "out", "out_len", "error", "scratch", "scratch_bytes", "stream")
		return entry(*[kw.get(name, v) for name, v in zip(names, good)])

	prefix, create_args = kind.ball_create
	h = C.c_void_p()
	_ffi.check(getattr(lib, prefix + "_create")(C.byref(h), *create_args))
	try:
		assert call(h=h) == -4 and f"{kind.shorten_entry}: build the ball first".encode() in lib.rk_last_error()      # RK_ESTATE
	finally:
		assert getattr(lib, prefix + "_destroy")(h) == 0
	assert call(h=None) == -1 and f"{kind.shorten_entry}: null ball".encode() in lib.rk_last_error()
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


def _ball_arrays(ball) -> list:
	"""The ball's arrays as a list: the plain ball gives several, the symmetry ball one."""
	arrays = ball.arrays()
	return [arrays.copy()] if isinstance(arrays, np.ndarray) else [a.copy() for a in arrays]


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_a_search_attached_to_the_ball_is_undisturbed(kind):
	ball = device_ball(kind, 4)
	agent = kind.search(ball, pops=64)
	start = ball_model.scramble(7003, 7)
	assert agent.search(start.copy())
	before = (list(agent.action_queue), len(agent))
	if kind is PLAIN:
		before += (agent.depth, agent.meeting_depth, [a.copy() for a in agent.arrays()])
	depth_before = ball.depth(np.stack([ball_model.scramble(s, 6) for s in range(50)]))
	arrays_before = _ball_arrays(ball)
	got = lists(ball.shorten(words(kind)))
	assert got == [list(w) for w in want_words(kind, 4, None, None)]
	assert agent.search(start.copy())
	assert (list(agent.action_queue), len(agent)) == before[:2]
	if kind is PLAIN:
		assert (agent.depth, agent.meeting_depth) == before[2:4] and all((x == y).all() for x, y in zip(agent.arrays(), before[4]))
	assert (ball.depth(np.stack([ball_model.scramble(s, 6) for s in range(50)])) == depth_before).all()
	ball._cache = {}
	assert all((x == y).all() for x, y in zip(_ball_arrays(ball), arrays_before))
	# the search's solution is a shortest one: nothing to take away
	assert lists(ball.shorten([before[0]])) == [before[0]]


# ---- the plain ball alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", RADII)
def test_constructed_cases(radius):
	model = shorten_model
	ball, mball = device_ball(PLAIN, radius), model_ball(PLAIN, radius)
	w = [int(a) for a in np.random.RandomState(5).randint(0, 12, 9)]
	batch, want = [w + model.inverse(w)], [[]]
	for a in range(12):
		batch += [[a] * 4, [a] * 3, [a]]
		want += [[], [model.rev(a)] if radius >= 1 else [a] * 3, [a]]
	for node in range(1, mball.len + 1, max(1, mball.len // 40)):          # ball paths: optimal words, unchanged
		for path in (ball_model.ball_path(mball, node), model.ball_word(mball, node)):
			batch.append(path)
			want.append(path)
	assert lists(ball.shorten(batch)) == want
	# a word of at most W moves whose end state the ball holds comes out with that state's depth, after one pass
	queues = [model.detour_word(100 + seed, seed % (radius + 1), 10 + seed % 7) for seed in range(40)]
	depths = ball.depth(np.stack([ball_model.apply(model.orc.SOLVED, x) for x in queues])).tolist()
	assert all(0 <= d <= seed % (radius + 1) for seed, d in enumerate(depths))
	assert [len(g) for g in ball.shorten(queues, passes=1)] == depths
	assert lists(ball.shorten(queues)) == [model.shorten(mball, x) for x in queues]
