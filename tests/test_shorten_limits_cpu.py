"""
The fast reference of tests/shorten_long_ref.py pinned to the two plain-Python models, and its 4 096-move words proven to take
the shortening engines where their code changes form -- all of it without a GPU, on the reference alone:
  * one pass of the fast reference equals shorten_model.one_pass and symshorten_model.one_pass word for word on the whole mixed
    batch of each kind (the words of tests/ball_kinds.py), radii 0, 1, 3 and 4, windows 1, 2, 8, 64 and None; its d(i, j) are the
    models', its fixed point is the models';
  * `collapse`: 4 096 moves whose one replaced edge at radius 4 is (0, 4 096, 4) -- the DP's key holds k - 1 = 4 095, the emit
    composes a span of 64 chunks -- and the empty word at radius 0;
  * `nested`: replaced edges of a span in (64, 128], in (256, 512] and above 512 (the emit's chunk loop, two to sixteen trips);
    a j whose tied minima lie more than 256 apart (the winner and a loser in different trips of a DP thread's loop) and one whose
    ties lie more than 64 and less than 256 apart (different waves), both on the path that the emit follows;
  * `incompressible` with windows of one move: cost[L] = 4 096, the uint16 cost at the limit, and the word unchanged.
tests/test_shorten_limits_gpu.py runs the engines on these words.

Measured here (one CPU core): a pass of the reference over 4 096 moves with every window takes 3.3 s (radius 4; 1.5 s at radius
0), nearly all of it the 4 096 table look-ups; the pins take 0.3 s (plain) to 1.3 s (sym: the model canonicalises every window)
per case, the depth-table test 1.2 s and 1.8 s, the long-word tests 5.6 s (collapse), 4.5 s (nested), 2.3 s (radius 0) and 0.04 s
-- 25 s for the file.
"""
import functools

import numpy as np
import pytest

from tests import ball_model
from tests import shorten_long_ref as ref
from tests import shorten_model
from tests import symshorten_model

RADII = (0, 1, 3, 4)
WINDOWS = (1, 2, 8, 64, None)


@functools.lru_cache(maxsize=None)
def _words(kind: str) -> tuple:
	"""The mixed batch of the kind: what ball_kinds.words gives the GPU suites."""
	batch = symshorten_model.mixed_batch()
	return batch[:8] if kind == "plain" else batch


def _model(kind: str, radius: int):
	return (shorten_model, ref.plain_ball(radius)) if kind == "plain" else (symshorten_model, ref.sym_ball(radius))


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_one_pass_of_the_fast_reference_is_one_pass_of_the_model(kind, radius):
	model, ball = _model(kind, radius)
	assert [len(w) for w in _words(kind)[:8]] == list(symshorten_model.LENGTHS)
	shorter = 0
	for window in WINDOWS:
		for w in _words(kind):
			got = ref.one_pass(kind, w, radius, window)
			want = model.one_pass(ball, w, window)
			assert list(got.word) == want and got.cost == len(want)
			assert all(0 <= d < j - i <= (window or len(w)) for i, j, d in got.replaced)
			assert len(w) - got.cost == sum(j - i - d for i, j, d in got.replaced)
			shorter += got.cost < len(w)
	assert shorter >= (0 if radius == 0 else 3)


@pytest.mark.parametrize("radius", (0, 4))
def test_the_depth_table_and_the_fixed_point_are_the_models(radius):
	w = _words("plain")[7]
	for window in (8, len(w)):
		want = shorten_model.window_depths(ref.plain_ball(radius), w, window)
		table = ref.window_depths(w, radius, window)
		assert table.shape == (len(w), window) and table.dtype == np.int8
		held = {(j - k, j): int(table[j - 1, k - 1]) for j in range(1, len(w) + 1) for k in range(1, min(window, j) + 1) if table[j - 1, k - 1] >= 0}
		assert held == want
		assert all(table[j - 1, k - 1] == -1 for j in range(1, window) for k in range(j + 1, window + 1))    # no window starts before 0
	for kind in ref.KINDS:
		model, ball = _model(kind, radius)
		for window in (8, None):
			for word in _words(kind):
				assert list(ref.shorten(kind, word, radius, window)) == model.shorten(ball, word, window)
				assert list(ref.shorten(kind, word, radius, window, passes=1)) == model.one_pass(ball, word, window)


def test_misuse_is_refused_as_the_models_refuse_it():
	for bad, kw in (([0, 12], {}), ([0] * 4097, {}), ([0, 1], dict(window=0))):
		with pytest.raises(ValueError):
			ref.one_pass("plain", bad, 1, **kw)
	assert ref.one_pass("sym", [], 3).word == () and ref.one_pass("plain", [5], 0).word == (5,)


# ---- the long words: conditions on the reference alone, met by the seeds in tests/shorten_long_ref.py -------------------------------

def _well_formed(word):
	assert len(word) == ref.LIMIT == shorten_model.MAX_LEN and all(isinstance(a, int) and 0 <= a < 12 for a in word)


def test_collapse_is_one_edge_over_the_whole_queue():
	word = ref.collapse(4)
	_well_formed(word)
	assert ball_model.depth(ref.plain_ball(4), ref.effect(word)) == 4
	for kind in ref.KINDS:
		one = ref.one_pass(kind, word, 4, None)
		assert one.replaced == ((0, 4096, 4),) and one.cost == 4 and len(one.word) == 4
		assert int(one.pred[4096]) == 0                                    # j - i - 1 = 4 095: the low field of the DP's key is full
		assert (ref.effect(one.word) == ref.effect(word)).all()
		assert ref.shorten(kind, word, 4, None) == one.word
	# windows of 8 leave a long word behind: the engines' second and later passes have work
	assert 1000 < ref.one_pass("plain", word, 4, 8).cost < 4096


def test_collapse_of_nothing_is_the_empty_word_at_radius_zero():
	word = ref.collapse(0)
	_well_formed(word)
	assert ref.collapse(0) != ref.collapse(4)
	for kind in ref.KINDS:
		one = ref.one_pass(kind, word, 0, None)
		assert one.replaced == ((0, 4096, 0),) and one.word == () and one.cost == 0


def test_nested_has_the_long_edges_and_the_distant_ties():
	word = ref.nested()
	_well_formed(word)
	assert ball_model.depth(ref.plain_ball(4), ref.effect(word)) == -1      # far outside the ball
	plain, sym = ref.one_pass("plain", word, 4, None), ref.one_pass("sym", word, 4, None)
	assert plain.replaced == sym.replaced and plain.cost == sym.cost and (plain.pred == sym.pred).all()
	spans = [j - i for i, j, _ in plain.replaced]
	assert any(64 < s <= 128 for s in spans) and any(256 < s <= 512 for s in spans) and any(s > 512 for s in spans)
	assert 4 < plain.cost < 4096 and len(plain.replaced) > 3
	spread = dict(plain.tie_spread)
	assert plain.ties == len(spread)
	assert any(s > 256 for s in spread.values())                           # another trip of a thread's loop
	assert any(64 < s < 256 for s in spread.values())                      # another wave
	# such ties are on the path that is taken: the pred they decide is read by the emit
	assert {j for j in spread if spread[j] > 256} & {j for _, j, _ in _edges(plain)}
	assert {j for j in spread if 64 < spread[j] < 256} & {j for _, j, _ in _edges(plain)}
	assert (ref.effect(plain.word) == ref.effect(word)).all() and (ref.effect(sym.word) == ref.effect(word)).all()
	# the prefix of 4 095 moves that the GPU test takes keeps the long edges
	prefix = ref.one_pass("plain", word[:4095], 4, None)
	assert any(s > 512 for s in (j - i for i, j, _ in prefix.replaced))


def _edges(one: ref.Pass) -> list:
	"""Every edge (i, j, None) of a pass' path, copied ones included."""
	out, j = [], len(one.pred) - 1
	while j > 0:
		out.append((int(one.pred[j]), j, None))
		j = int(one.pred[j])
	return out


def test_incompressible_costs_every_move():
	word = ref.incompressible()
	_well_formed(word)
	for kind in ref.KINDS:
		one = ref.one_pass(kind, word, 3, 1)
		assert one.cost == 4096 and one.word == word and one.replaced == () and one.ties == 0
		assert ref.shorten(kind, word, 3, 1) == word
