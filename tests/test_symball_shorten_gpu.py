"""
DeviceSymBall.shorten (engine rk_sshorten) on the GPU, against the plain-Python model (tests/symshorten_model.py) bit for bit:
  * symmetry balls of radius 0, 1, 3 and 4; one mixed batch per call (symshorten_model.mixed_batch: the queues of 0, 1, 2, 63, 64,
    65, 129 and 300 moves of tests/test_ball_shorten_gpu.py and four whose replaced segment has several shortest words); windows
    1 (nothing changes), 2, 8, 64 and None;
  * one pass of rk_sshorten called directly -- rows, padding, lengths and the error word -- equals one pass of the model, and the
    fixed point of the method equals the model's and is returned unchanged by a further call (the bodies, in tests/ball_kinds.py,
    are the plain ball's too);
  * against code that already ships: DeviceGoalBall(5).shorten gives the same lengths queue for queue, and the same states;
  * the bytes do not depend on the ball's `pops`;
  * the 6x8x6 mode changes nothing: the method takes no states.
The reversed and duplicated batch, the scratch chunks, misuse and the attached DeviceSymBallSearch are what this ball shares with
the plain one: tests/test_ball_shorten_gpu.py runs them for both.
"""
import numpy as np
import pytest

from librubiks_amd import cube
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall
from tests import ball_kinds
from tests import symshorten_model as model
from tests.ball_kinds import SYM, device_ball, lists, one_pass_direct, want_words, words

pytestmark = pytest.mark.gpu

RADII = (0, 1, 3, 4)
WINDOWS = (1, 2, 8, 64, None)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("radius", RADII)
def test_one_pass_of_the_entry_equals_one_pass_of_the_model(radius, window):
	ball_kinds.one_pass_of_the_entry_equals_one_pass_of_the_model(SYM, radius, window)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("radius", RADII)
def test_fixed_point_equals_the_model(radius, window):
	ball_kinds.fixed_point_equals_the_model(SYM, radius, window)


def _apply_all(queues) -> np.ndarray:
	"""The solved state after every word, by cube.multi_rotate: one call per position, over the words that reach it."""
	states = np.stack([cube.get_solved()] * len(queues))
	for t in range(max(len(w) for w in queues)):
		rows = [r for r, w in enumerate(queues) if len(w) > t]
		acts = np.array([queues[r][t] for r in rows], np.int64)
		states[rows] = cube.multi_rotate(states[rows], acts // 2, 1 - acts % 2)
	return states


def test_lengths_and_states_equal_the_plain_balls_at_radius_five():
	sball, pball = DeviceSymBall(5), DeviceGoalBall(5)
	queues = [model.detour_word(200 + s, s % 21, 40 + s % 50) for s in range(64)]
	before = _apply_all(queues)
	shortened = 0
	for window in (8, None):
		got, plain = lists(sball.shorten(queues, window=window)), lists(pball.shorten(queues, window=window))
		assert [len(g) for g in got] == [len(p) for p in plain]
		assert (_apply_all(got) == _apply_all(plain)).all() and (_apply_all(got) == before).all()
		shortened += sum(len(g) < len(w) for g, w in zip(got, queues))
	assert shortened >= 64


def test_the_bytes_do_not_depend_on_pops():
	batch = words(SYM)
	a, b = DeviceSymBall(4, pops=7), DeviceSymBall(4, pops=4096)
	assert (a.arrays() == b.arrays()).all()
	for window in (8, None):
		one = one_pass_direct(SYM, a, batch, window)
		two = one_pass_direct(SYM, b, batch, window)
		assert (one[0] == two[0]).all() and (one[1] == two[1]).all() and one[2] == two[2] == 0
		assert lists(a.shorten(batch, window=window)) == lists(b.shorten(batch, window=window)) == [list(w) for w in want_words(SYM, 4, window, None)]


def test_the_6x8x6_mode_gives_the_same_queues():
	ball = device_ball(SYM, 4)
	want = [list(w) for w in want_words(SYM, 4, 8, None)]
	assert lists(ball.shorten(words(SYM), window=8)) == want
	try:
		cube.set_is2024(False)
		assert lists(ball.shorten(words(SYM), window=8)) == want
	finally:
		cube.set_is2024(True)
