"""
Shortening action queues against the symmetry ball, without a GPU: the plain-Python model (tests/symshorten_model.py) that the
GPU tests compare DeviceSymBall.shorten with, against the plain ball's model (tests/shorten_model.py) at radii 0, 1, 3 and 4 over
the words of tests/test_ball_shorten_gpu.py and four words whose replaced segment has several shortest words
(symshorten_model.mixed_batch) --
  * the lengths after one pass and at the fixed point are the plain ball's, queue for queue (conjugation keeps the distance);
  * every output has the effect of its input on the solved state;
  * the inputs do exercise it: at radius 4 at least three words get shorter in one pass, and at least one replaced segment gets
    another word than the plain ball's (the inverse of the descent is not the stored word);
-- and the method's argument checks that come before any device is touched.
"""
import functools

import numpy as np
import pytest

from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall
from oracle import cube_oracle as orc
from tests import ball_model
from tests import shorten_model
from tests import sym_model
from tests import symshorten_model as model

RADII = (0, 1, 3, 4)


@functools.lru_cache(maxsize=None)
def _words() -> tuple:
	return model.mixed_batch()


@functools.lru_cache(maxsize=None)
def _sym_ball(radius: int):
	return sym_model.build(radius)


@functools.lru_cache(maxsize=None)
def _plain_ball(radius: int):
	return ball_model.build(radius)


def _effect(word) -> np.ndarray:
	x = orc.SOLVED.astype(np.int8)[None]
	for a in word:
		x = orc.multi_rotate(x, np.array([a // 2]), np.array([1 - a % 2]))
	return x[0]


@pytest.mark.parametrize("radius", RADII)
def test_lengths_are_the_plain_balls_and_the_effect_is_kept(radius):
	words = _words()
	assert [len(w) for w in words[:8]] == list(model.LENGTHS)
	assert list(words[:8]) == [tuple(shorten_model.detour_word(40 + k, min(n, 20), n)[:n]) for k, n in enumerate(model.LENGTHS)]
	sball, pball = _sym_ball(radius), _plain_ball(radius)
	shorter, differ = 0, 0
	for w in words:
		replaced = []
		one = model.one_pass(sball, w, replaced=replaced)
		full = model.shorten(sball, w)
		assert len(one) == len(shorten_model.one_pass(pball, w))
		assert len(full) == len(shorten_model.shorten(pball, w))
		assert len(full) <= len(one) <= len(w) and all(0 <= a < 12 for a in one + full)
		assert (_effect(one) == _effect(w)).all() and (_effect(full) == _effect(w)).all()
		assert model.one_pass(sball, full) == full                          # a fixed point of the pass
		shorter += len(one) < len(w)
		for segment, new in replaced:                                       # the plain ball's word for the same net effect
			node = pball.index[np.ascontiguousarray(_effect(segment), np.int8).tobytes()]
			plain = shorten_model.ball_word(pball, node)
			assert len(plain) == len(new) and (_effect(plain) == _effect(new)).all()
			differ += plain != new
	if radius == 4:
		assert shorter >= 3
		assert differ >= 1                                                  # the inverse of the descent is exercised as a word of its own


def test_narrow_windows_agree_too():
	sball, pball = _sym_ball(3), _plain_ball(3)
	for w in _words()[:7] + _words()[8:]:
		for window in (1, 2, 8):
			got = model.shorten(sball, w, window)
			assert len(got) == len(shorten_model.shorten(pball, w, window)) and (_effect(got) == _effect(w)).all()
			if window == 1:
				assert got == list(w)


@pytest.mark.parametrize("bad,kw", [([[0, 12, 3]], {}), ([[0] * 4097], {}), ([[0, 1]], dict(window=0)), ([[0, 1]], dict(passes=-1))])
def test_method_refuses_bad_arguments_before_any_device_is_touched(bad, kw):
	ball = DeviceSymBall(2)
	with pytest.raises(ValueError):
		ball.shorten(bad, **kw)
	assert ball._h is None and not ball.built


def test_the_method_is_one_for_both_balls():
	assert DeviceSymBall.shorten is DeviceGoalBall.shorten
	assert DeviceSymBall.MAX_QUEUE == DeviceGoalBall.MAX_QUEUE == 4096
	assert DeviceSymBall.shorten_scratch_bytes == DeviceGoalBall.shorten_scratch_bytes == 256 << 20
	assert (DeviceGoalBall._shorten_entry, DeviceSymBall._shorten_entry) == ("rk_bshorten", "rk_sshorten")
