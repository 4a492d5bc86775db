"""
The symmetry kernels (rk_sym_*) and DeviceSymBall (engine rk_symball_*) on the GPU:
  * `cube.canonical` on all 11 206 states of the plain radius-4 ball plus 1 000 seeded 20-move scrambles (12 206: no multiple of
    64 or 256) against the model (tests/sym_model.py) for representatives, symmetries and orbit sizes, on n = 0 and n = 1, and
    `cube.conjugate` for every symmetry on 257 states, in both representations;
  * `DeviceSymBall(4)` with pops 1 / 7 / 4096 against the model, bit for bit, and equal across the three;
  * `DeviceSymBall(5).depth` against the engine that already ships: every state of `DeviceGoalBall(6)` (983 926 states);
  * `solve` on every state of the plain radius-4 ball: the plain ball's depths, the model's descent, and every row solves;
  * a capacity that is too small: a refusal and a usable process; the C entries' argument checks.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall
from tests import ball_model
from tests import sym_model as model
from tests.bibfs_model import scramble

pytestmark = pytest.mark.gpu

orc = model.orc
REPRS = ("2024", "686")
POPS = (1, 7, 4096)
LEVELS = list(DeviceSymBall.LEVELS)


@functools.lru_cache(maxsize=None)
def _plain4():
	"""The plain radius-4 ball of the model: 11 206 states in index order, and their depths."""
	ball = ball_model.build(4)
	assert ball.len == 11_206
	return ball.states, np.searchsorted(ball.level_start, np.arange(1, ball.len + 1), side="right") - 1


@functools.lru_cache(maxsize=None)
def _far(n: int = 1000) -> np.ndarray:
	return np.stack([scramble(20_000 + s, 20) for s in range(n)])


@functools.lru_cache(maxsize=None)
def _queries() -> np.ndarray:
	q = np.concatenate([_plain4()[0], _far()])
	assert len(q) == 12_206 and len(q) % 64 and len(q) % 256
	return q


@functools.lru_cache(maxsize=None)
def _model_canonical():
	return model.canonical(_queries())


@functools.lru_cache(maxsize=None)
def _model_ball(radius: int):
	return model.build(radius)


@functools.lru_cache(maxsize=None)
def _sym4() -> DeviceSymBall:
	return DeviceSymBall(4).build()


def _in_repr(states20: np.ndarray) -> np.ndarray:
	return states20 if cube.get_is2024() else cube.as686(states20).reshape(len(states20), 6, 8, 6)


def _apply_rows(states20: np.ndarray, actions: np.ndarray) -> np.ndarray:
	"""Row i of `actions` (padded with -1) applied to state i, with the oracle's moves."""
	out = np.array(states20, np.int8)
	for k in range(actions.shape[1]):
		rows = np.nonzero(actions[:, k] >= 0)[0]
		if len(rows):
			a = actions[rows, k]
			out[rows] = orc.multi_rotate(out[rows], a // 2, 1 - a % 2)
	return out


@pytest.mark.parametrize("rep", REPRS)
def test_canonical_against_the_model(rep):
	want_reps, want_syms, want_orbit = _model_canonical()
	cube.set_is2024(rep == "2024")
	reps, syms, orbit = cube.canonical(_in_repr(_queries()))
	assert reps.dtype == np.int8 and syms.dtype == np.int64 and orbit.dtype == np.int64
	assert reps.shape == _in_repr(want_reps).shape and (reps == _in_repr(want_reps)).all()
	assert (syms == want_syms).all() and (orbit == want_orbit).all()
	assert set(np.unique(orbit).tolist()) <= {1, 2, 3, 4, 6, 8, 12, 16, 24, 48} and orbit[0] == 1 and (orbit[11_206:] == 48).sum() > 900
	one = cube.canonical(_in_repr(_queries()[500:501]))
	assert (one[0] == _in_repr(want_reps[500:501])).all() and one[1].tolist() == [want_syms[500]] and one[2].tolist() == [want_orbit[500]]
	none = cube.canonical(_in_repr(_queries()[:0]))
	assert none[0].shape == _in_repr(want_reps[:0]).shape and none[1].shape == (0,) and none[2].shape == (0,)
	with pytest.raises(ValueError):
		cube.canonical(np.zeros((3, 19), np.int8))


@pytest.mark.parametrize("rep", REPRS)
def test_conjugate_against_the_model(rep):
	x = _queries()[11_206 - 129:11_206 + 128]
	assert len(x) == 257
	cube.set_is2024(rep == "2024")
	given = _in_repr(x)
	for s in range(48):
		got = cube.conjugate(given, s)
		assert got.dtype == np.int8 and (got == _in_repr(model.conjugate(x, s))).all(), s
	assert (cube.conjugate(given, 0) == given).all()
	assert cube.conjugate(given[:0], 7).shape == given[:0].shape and (cube.conjugate(given[:1], 7) == _in_repr(model.conjugate(x[:1], 7))).all()


def test_ball_against_the_model_and_independent_of_pops():
	want = _model_ball(4)
	assert want.covered.tolist() == LEVELS[:5]
	orbits = np.diff(want.level_start).tolist()
	runs = []
	for pops in POPS:
		ball = DeviceSymBall(4, pops=pops)
		assert len(ball) == want.len and ball.built
		assert ball.level_start.dtype == np.int64 and ball.level_start.tolist() == want.level_start.tolist()
		assert ball.states_covered.dtype == np.int64 and ball.states_covered.tolist() == want.covered.tolist()
		states = ball.arrays()
		assert states.dtype == np.int8 and states.shape == (want.len, 20) and (states == want.states).all()
		assert ball.iterations == sum(-(-n // pops) for n in orbits[:4])         # no batch crosses a level boundary
		assert [ball.depth_of_node(n) for n in (1, 2, 3, 8, 33, 251)] == [0, 1, 2, 3, 4, 4]
		runs.append((len(ball), ball.level_start, ball.states_covered, states))
	for other in runs[1:]:
		assert other[0] == runs[0][0]
		for x, y in zip(other[1:], runs[0][1:]):
			assert (x == y).all()
	cube.set_is2024(False)
	assert (DeviceSymBall(4, pops=7).arrays() == cube.as686(want.states)).all()
	cube.set_is2024(True)
	zero = DeviceSymBall(0)
	assert len(zero) == 1 and zero.level_start.tolist() == [1, 2] and zero.iterations == 0 and zero.states_covered.tolist() == [1]
	assert zero.depth(np.stack([orc.SOLVED, scramble(1, 1)])).tolist() == [0, -1]
	assert zero.build() is zero


def test_depth_against_the_plain_ball():
	plain = DeviceGoalBall(6)
	states, _, _ = plain.arrays()
	assert len(states) == 983_926
	want = np.searchsorted(plain.level_start, np.arange(1, len(states) + 1), side="right") - 1
	ball = DeviceSymBall(5)
	depths = ball.depth(states)
	assert depths.dtype == np.int64 and depths.shape == want.shape
	assert (depths == np.where(want <= 5, want, -1)).all()
	assert (ball.depth(_far()) == -1).all()
	assert ball.states_covered.tolist() == LEVELS[:6]
	# one representative per orbit: as many nodes per level as the plain ball's level has distinct canonical forms
	inside = states[:plain.level_start[6] - 1]
	reps, _, orbit = cube.canonical(inside)
	keys = np.ascontiguousarray(reps).view("V20").ravel()
	for level in range(6):
		lo, hi = plain.level_start[level] - 1, plain.level_start[level + 1] - 1
		distinct = np.unique(keys[lo:hi])
		assert len(distinct) == ball.level_start[level + 1] - ball.level_start[level], level
		mine = np.ascontiguousarray(ball.arrays()[ball.level_start[level] - 1:ball.level_start[level + 1] - 1]).view("V20").ravel()
		assert (np.sort(mine) == distinct).all()
	assert len(ball) == len(np.unique(keys))
	# the orbit sizes of the distinct representatives add up to the plain ball's states
	_, first = np.unique(keys, return_index=True)
	assert orbit[first].sum() == len(inside) == sum(LEVELS[:6])


@pytest.mark.parametrize("rep", REPRS)
def test_solve(rep):
	states, depths = _plain4()
	ball, want = _sym4(), _model_ball(4)
	cube.set_is2024(rep == "2024")
	lengths, actions = ball.solve(_in_repr(states))
	assert lengths.dtype == np.int64 and actions.dtype == np.int64 and actions.shape == (len(states), 4)
	assert (lengths == depths).all() and (ball.depth(_in_repr(states)) == depths).all()
	assert ((actions >= 0).sum(axis=1) == lengths).all() and (actions[np.arange(4)[None] >= lengths[:, None]] == -1).all()
	want_lengths, want_actions = model.solve(want, states)
	assert (lengths == want_lengths).all() and (actions == want_actions).all()
	assert orc.multi_is_solved(_apply_rows(states, actions)).all()
	outside = _far(16)
	lengths, actions = ball.solve(_in_repr(outside))
	assert (lengths == -1).all() and (actions == -1).all() and actions.shape == (16, 4)
	mixed = np.concatenate([outside[:2], states[[0, 5, 11_205]]])
	lengths, actions = ball.solve(_in_repr(mixed))
	assert lengths.tolist() == [-1, -1, 0, 1, 4] and (actions[:3] == -1).all() and (actions[4] >= 0).all()
	none = ball.solve(_in_repr(states[:0]))
	assert none[0].shape == (0,) and none[1].shape == (0, 4)
	with pytest.raises(ValueError):
		ball.depth(np.zeros((3, 19), np.int8))
	if rep == "686":
		with pytest.raises(ValueError):
			ball.solve(np.zeros((1, 6, 8, 6), np.int8))


def test_too_small_a_capacity_is_refused_and_the_process_goes_on():
	small = DeviceSymBall(4, pops=4096, capacity=100)
	with pytest.raises(_ffi.RubiksHipError, match="capacity"):
		small.build()
	assert not small.built
	with pytest.raises(_ffi.RubiksHipError, match="capacity"):              # asked again: refused again, nothing kept
		len(small)
	exact = DeviceSymBall(4, pops=7, capacity=251 + 12)                      # room for the orbits and for one more pop whatever it finds
	assert len(exact) == 251 and exact.capacity == 263 and (exact.arrays() == _model_ball(4).states).all()
	assert (exact.depth(_plain4()[0]) == _plain4()[1]).all()                 # and the device still answers
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	h = C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(h), 2, 8, 0))
	try:
		queries = torch.from_numpy(np.stack([orc.SOLVED, scramble(5, 5)]).astype(np.int8)).to("cuda")
		out = torch.full((2,), 7, dtype=torch.int32, device="cuda")
		acts = torch.full((2, 2), 7, dtype=torch.int8, device="cuda")
		err = torch.full((1,), 7, dtype=torch.int32, device="cuda")
		buf = np.zeros(20, np.int8)
		assert lib.rk_symball_depth(h, queries.data_ptr(), 2, out.data_ptr(), stream) == -4          # RK_ESTATE: not built
		_ffi.check(lib.rk_symball_build(h, 8, stream))
		_ffi.check(lib.rk_symball_build(h, 8, stream))                                               # built: nothing to do
		status = (C.c_longlong * 32)()
		_ffi.check(lib.rk_symball_status(h, status))
		assert list(status[:4]) == [1, 7, 2, 2] and list(status[6:10]) == [1, 2, 3, 8] and list(status[18:21]) == [1, 12, 114]
		assert lib.rk_symball_depth(h, None, 2, out.data_ptr(), stream) == -1                        # RK_EINVAL: null pointers
		assert lib.rk_symball_depth(h, queries.data_ptr(), 2, None, stream) == -1
		assert lib.rk_symball_depth(h, queries.data_ptr() + 1, 1, out.data_ptr(), stream) == -1      # misaligned
		assert lib.rk_symball_solve(h, queries.data_ptr(), 2, out.data_ptr(), None, err.data_ptr(), stream) == -1
		assert lib.rk_symball_solve(h, queries.data_ptr(), 2, out.data_ptr(), acts.data_ptr(), None, stream) == -1
		assert lib.rk_symball_depth(h, None, 0, None, stream) == 0                                   # no queries: nothing to do
		_ffi.check(lib.rk_symball_solve(h, queries.data_ptr(), 2, out.data_ptr(), acts.data_ptr(), err.data_ptr(), stream))
		assert out.tolist() == [0, -1] and acts.tolist() == [[-1, -1], [-1, -1]] and err.tolist() == [0]
		assert lib.rk_symball_export(h, 1, 8, buf.ctypes.data, stream) == -1                         # rows outside the pool
		assert lib.rk_symball_export(h, 1, 1, None, stream) == -1
		_ffi.check(lib.rk_symball_export(h, 1, 1, buf.ctypes.data, stream))
		assert (buf == orc.SOLVED).all()
		assert lib.rk_sym_canonical(queries.data_ptr() + 1, 1, None, None, None, stream) == -1       # misaligned
		sym = torch.full((2,), 99, dtype=torch.uint8, device="cuda")
		_ffi.check(lib.rk_sym_canonical(queries.data_ptr(), 2, None, sym.data_ptr(), None, stream))  # any output may be NULL
		assert sym.tolist() == [0, int(model.canonical(scramble(5, 5)[None])[1][0])]
	finally:
		assert lib.rk_symball_destroy(h) == 0
