"""
Paired inputs for the 6x8x6 kernel tests -- TEST INFRASTRUCTURE, pure NumPy, no kernel anywhere.

"The same cube in both forms" is the oracle walking both representations with the same draws: from `orc.SOLVED` and
`orc.SOLVED686`, `orc.multi_rotate` and `orc.multi_rotate686` with the same (faces, dirs) for DEPTH moves.  `pool()` holds POOL such
pairs; `gather(n, seed)` draws n of them with `rng.randint(0, POOL, n)`, so that neighbouring rows of a large input differ.
tests/test_repr686_pairs_cpu.py asserts that these inputs are not weak.

The slot tables and the row edits below (illegal rows for `from686`, an edge flipped / a corner twisted in place) come from the
oracle's sticker maps alone.
"""
import functools

import numpy as np

from oracle import cube_oracle as orc

POOL = 4099
DEPTH = 25
SEED = 686


def walk_pairs(actions: np.ndarray):
	"""(games, depth) action indices, -1 = no move -> (states20 (games, 20), states686 (games, 6, 8, 6)) after each game's moves."""
	actions = np.asarray(actions).astype(np.int64)
	games = len(actions)
	s20 = orc.repeat_state(orc.SOLVED, games)
	s686 = orc.repeat_state(orc.SOLVED686, games)
	for d in range(actions.shape[1]):
		live = actions[:, d] >= 0
		if live.any():
			faces, dirs = orc.indices_to_actions(actions[live, d])
			s20[live] = orc.multi_rotate(s20[live], faces, dirs)
			s686[live] = orc.multi_rotate686(s686[live], faces, dirs)
	return s20, s686


@functools.lru_cache(maxsize=None)
def pool():
	"""(states20 (POOL, 20), states686 (POOL, 6, 8, 6)) int8, read-only: POOL paired walks of DEPTH moves."""
	rng = np.random.RandomState(SEED)
	s20, s686 = walk_pairs(rng.randint(0, 12, (POOL, DEPTH)))
	s20, s686 = np.ascontiguousarray(s20, dtype=np.int8), np.ascontiguousarray(s686, dtype=np.int8)
	s20.flags.writeable = False
	s686.flags.writeable = False
	return s20, s686


def gather(n: int, seed: int):
	"""n pool rows drawn with replacement: (indices (n,), states20 (n, 20), states686 (n, 6, 8, 6)), fresh writable arrays."""
	idx = np.random.RandomState(seed).randint(0, POOL, n)
	s20, s686 = pool()
	return idx, s20[idx], s686[idx]


# ---------------------------------------------------------------------------------------------------------------------------
# Where each cubie position shows its stickers: slot = 8 face + ring position.  `orc.as633_686` puts ring position
# (j + _RING_SHIFT[face]) % 8 of a face at flat index _RING_TO_33[j] of its 3x3 picture; the sticker maps name picture cells.
# ---------------------------------------------------------------------------------------------------------------------------
def _slot(face: int, row: int, col: int) -> int:
	j = int(np.nonzero(orc._RING_TO_33 == 3 * row + col)[0][0])
	return 8 * face + (j + int(orc._RING_SHIFT[face])) % 8


#: CORNER_SLOTS[pos] / EDGE_SLOTS[pos]: the slots of corner position 0..7 / edge position 0..11, in the sticker maps' order
CORNER_SLOTS = np.array([[_slot(*s) for s in c] for c in orc._CORNER_STICKERS])
EDGE_SLOTS = np.array([[_slot(*s) for s in e] for e in orc._EDGE_STICKERS])
#: the colours a cubie carries = the faces of its home position, same order
CORNER_COLOURS = np.array([[s[0] for s in c] for c in orc._CORNER_STICKERS])
EDGE_COLOURS = np.array([[s[0] for s in e] for e in orc._EDGE_STICKERS])


def colours(states686: np.ndarray) -> np.ndarray:
	"""(n, 6, 8, 6) one-hot states -> (n, 48) colour of every slot."""
	return np.asarray(states686).reshape(-1, 48, 6).argmax(axis=2)


def _paint(row: np.ndarray, slot: int, colour: int):
	row[slot] = 0
	row[slot, colour] = 1


#: the kinds of row that `from686` must refuse; the first four are those of tests/test_repr686_cube_gpu.py
ILLEGAL_KINDS = ("other_colour", "empty_slot", "two_ones", "corner_mirrored", "one_is_2", "one_is_minus1", "opposite_faces_edge",
                 "edge_twice")


def make_illegal(state686: np.ndarray, kind: str) -> np.ndarray:
	"""A copy of one legal (6, 8, 6) state made illegal in the way `kind` names."""
	row = np.array(state686, dtype=np.int8).reshape(48, 6)
	col = row.argmax(axis=1)
	if kind == "other_colour":                     # one slot shows another colour (that colour then shows nine times)
		row[5] = np.roll(row[5], 1)
	elif kind == "empty_slot":
		row[3] = 0
	elif kind == "two_ones":
		row[7, (col[7] + 1) % 6] = 1
	elif kind == "corner_mirrored":                # two stickers of one corner swapped: its mirror image, which no cubie is
		a, b = CORNER_SLOTS[0, 0], CORNER_SLOTS[0, 1]
		_paint(row, a, col[b])
		_paint(row, b, col[a])
	elif kind == "one_is_2":
		row[20, col[20]] = 2
	elif kind == "one_is_minus1":
		row[41, col[41]] = -1
	elif kind == "opposite_faces_edge":            # F and B colours on one edge: each slot a clean one-hot, but no such cubie
		_paint(row, EDGE_SLOTS[6, 0], 0)
		_paint(row, EDGE_SLOTS[6, 1], 1)
	elif kind == "edge_twice":                     # edge position 2 shows what position 9 shows: one cubie twice, one missing
		_paint(row, EDGE_SLOTS[2, 0], col[EDGE_SLOTS[9, 0]])
		_paint(row, EDGE_SLOTS[2, 1], col[EDGE_SLOTS[9, 1]])
	else:
		raise KeyError(kind)
	return row.reshape(6, 8, 6)


def flip_edge(state686: np.ndarray, pos: int) -> np.ndarray:
	"""The edge at position `pos` flipped in place: every cubie still shows once (not a reachable cube, but well formed)."""
	row = np.array(state686, dtype=np.int8).reshape(48, 6)
	a, b = EDGE_SLOTS[pos]
	row[[a, b]] = row[[b, a]]
	return row.reshape(6, 8, 6)


def twist_corner(state686: np.ndarray, pos: int) -> np.ndarray:
	"""The corner at position `pos` twisted in place by a third of a turn (its three colours cycle through its three slots)."""
	row = np.array(state686, dtype=np.int8).reshape(48, 6)
	a, b, c = CORNER_SLOTS[pos]
	row[[a, b, c]] = row[[c, a, b]]
	return row.reshape(6, 8, 6)


def flipped20(state20: np.ndarray, pos: int) -> np.ndarray:
	"""The 20-byte row of `flip_edge`: the byte of the edge cubie at position `pos` changes orientation, nothing else changes."""
	out = np.array(state20, dtype=np.int8)
	out[8 + int(np.nonzero(out[8:] // 2 == pos)[0][0])] ^= 1
	return out


def twisted20(state20: np.ndarray, pos: int) -> np.ndarray:
	"""The 20-byte row of `twist_corner`: the byte of the corner cubie at position `pos` goes to the next orientation (the previous
	one at the positions whose winding `orc.as633` mirrors), nothing else changes."""
	out = np.array(state20, dtype=np.int8)
	c = int(np.nonzero(out[:8] // 3 == pos)[0][0])
	out[c] = 3 * pos + (out[c] % 3 + (2 if pos in (0, 2, 5, 7) else 1)) % 3
	return out
