"""
The paired inputs of tests/repr686_pairs.py are not weak (CPU only): the pool's rows are all different cubes, both forms of every
pool row draw the same picture, the pairing replays the unmodified reference's recorded walks (tests/golden/repr686_cube.npz,
tools/gen_golden_repr686.py), and the slot tables behind the row edits agree with the 20-byte codes.
"""
import os

import numpy as np

from oracle import cube_oracle as orc
from tests import repr686_pairs as pairs
from tests.test_repr686_cpu import as_states

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_pool_rows_are_distinct_legal_and_paired():
	s20, s686 = pairs.pool()
	assert s20.shape == (pairs.POOL, 20) and s686.shape == (pairs.POOL, 6, 8, 6) and s20.dtype == s686.dtype == np.int8
	assert len({r.tobytes() for r in s20}) == pairs.POOL
	assert len({r.tobytes() for r in s686}) == pairs.POOL
	assert not orc.multi_is_solved(s20).any() and not orc.multi_is_solved686(s686).any()
	flat = s686.reshape(pairs.POOL, 48, 6)
	assert ((flat == 0) | (flat == 1)).all() and (flat.sum(axis=2) == 1).all()
	assert (np.stack([np.bincount(c, minlength=6) for c in pairs.colours(s686)]) == 8).all()
	for i in range(pairs.POOL):
		assert (orc.as633(s20[i]) == orc.as633_686(s686[i])).all(), i


def test_gather_draws_neighbouring_rows_apart():
	idx, s20, s686 = pairs.gather(70_001, 5)
	p20, p686 = pairs.pool()
	assert idx.min() == 0 and idx.max() == pairs.POOL - 1 and len(np.unique(idx)) == pairs.POOL
	assert (s20 == p20[idx]).all() and (s686 == p686[idx]).all() and s20.flags.writeable and s686.flags.writeable
	assert (idx[1:] != idx[:-1]).mean() > 0.999
	again = pairs.gather(70_001, 5)
	assert (again[0] == idx).all() and (pairs.gather(70_001, 6)[0] != idx).any()


def test_pairing_replays_the_reference_walks():
	"""The fixture records the moves of every walk (`actions`, -1 = none), so the replay is possible: the same two oracle functions
	that build the pool, given those moves, must land on the reference's own states in both forms."""
	with np.load(os.path.join(GOLDEN, "repr686_cube.npz")) as z:
		actions, want20, want686 = z["actions"], z["states20"], as_states(z["colours686"])
	assert actions.shape == (len(want20), 30) and (actions >= 0).sum(axis=1).max() == 30
	s20, s686 = pairs.walk_pairs(actions)
	assert (s20 == want20).all() and (s686 == want686).all()


def test_slot_tables_agree_with_the_20_byte_codes():
	"""At every position the cubie that the 20-byte code names shows its colours on that position's slots, in the orientation the
	code gives (as `orc.as633` rolls them) -- so the tables edit the cubie they say they edit."""
	assert sorted(np.r_[pairs.CORNER_SLOTS.ravel(), pairs.EDGE_SLOTS.ravel()].tolist()) == list(range(48))
	assert (pairs.CORNER_SLOTS // 8 == pairs.CORNER_COLOURS).all() and (pairs.EDGE_SLOTS // 8 == pairs.EDGE_COLOURS).all()
	s20, s686 = pairs.pool()
	col = pairs.colours(s686)
	for i in range(0, pairs.POOL, 7):
		for c in range(8):
			pos, ori = divmod(int(s20[i, c]), 3)
			ori = -ori if pos in (0, 2, 5, 7) else ori
			assert (col[i, pairs.CORNER_SLOTS[pos]] == np.roll(pairs.CORNER_COLOURS[c], ori)).all(), (i, c)
		for e in range(12):
			pos, ori = divmod(int(s20[i, 8 + e]), 2)
			assert (col[i, pairs.EDGE_SLOTS[pos]] == np.roll(pairs.EDGE_COLOURS[e], ori)).all(), (i, e)


def test_row_edits_do_what_their_names_say():
	_, s686 = pairs.pool()
	base = s686[11]
	bcol = pairs.colours(base)[0]
	for kind in pairs.ILLEGAL_KINDS:
		bad = pairs.make_illegal(base, kind)
		assert bad.shape == (6, 8, 6) and bad.dtype == np.int8 and (bad != base).any(), kind
		assert (base == s686[11]).all()                                     # out of place
	onehot = lambda s: ((s == 0) | (s == 1)).all() and (s.reshape(48, 6).sum(axis=1) == 1).all()
	assert [bool(onehot(pairs.make_illegal(base, k))) for k in pairs.ILLEGAL_KINDS] == [True, False, False, True, False, False, True, True]
	assert pairs.make_illegal(base, "one_is_2").max() == 2 and pairs.make_illegal(base, "one_is_minus1").min() == -1
	twice = pairs.colours(pairs.make_illegal(base, "edge_twice"))[0]
	assert (twice[pairs.EDGE_SLOTS[2]] == bcol[pairs.EDGE_SLOTS[9]]).all() and (np.delete(twice, pairs.EDGE_SLOTS[2]) == np.delete(bcol, pairs.EDGE_SLOTS[2])).all()
	opp = pairs.colours(pairs.make_illegal(base, "opposite_faces_edge"))[0]
	assert not any(set(opp[pairs.EDGE_SLOTS[6]]) == set(e) for e in pairs.EDGE_COLOURS)
	for pos in range(12):
		f = pairs.colours(pairs.flip_edge(base, pos))[0]
		assert (f[pairs.EDGE_SLOTS[pos]] == bcol[pairs.EDGE_SLOTS[pos]][::-1]).all() and (f != bcol).sum() == 2
	for pos in range(8):
		t = pairs.colours(pairs.twist_corner(base, pos))[0]
		assert (t[pairs.CORNER_SLOTS[pos]] == np.roll(bcol[pairs.CORNER_SLOTS[pos]], 1)).all() and (t != bcol).sum() == 3


def test_flipped_and_twisted_rows_pair_with_one_changed_byte():
	"""`flipped20` / `twisted20` change one byte of the 20-byte row and draw the picture of the edited 6x8x6 row."""
	s20, s686 = pairs.pool()
	for i in range(0, pairs.POOL, 101):
		for pos in range(12):
			t = pairs.flipped20(s20[i], pos)
			assert (t != s20[i]).sum() == 1 and (orc.as633(t) == orc.as633_686(pairs.flip_edge(s686[i], pos))).all(), (i, pos)
		for pos in range(8):
			t = pairs.twisted20(s20[i], pos)
			assert (t != s20[i]).sum() == 1 and (t // 3 == s20[i] // 3)[:8].all(), (i, pos)
			assert (orc.as633(t) == orc.as633_686(pairs.twist_corner(s686[i], pos))).all(), (i, pos)
