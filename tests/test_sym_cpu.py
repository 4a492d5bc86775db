"""
The 48 symmetries and DeviceSymBall without a GPU: the library's compile-time tables (rk_sym_tables) against the model's, which
are derived another way (tests/sym_model.py); the relabellings are 48 distinct permutations of the actions; every symmetry keeps
the solved state; conjugation commutes with every move under the relabelling, checked with the oracle's moves on seeded
scrambles; the symmetries are closed under composition; arguments are refused before anything is launched; and the model's
radius-4 ball of representatives covers exactly the level sizes of the quarter-turn Cayley graph.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall
from tests import sym_model as model
from tests.bibfs_model import scramble

orc = model.orc


def _scrambles(n: int = 200, moves: int = 20) -> np.ndarray:
	return np.stack([scramble(50_000 + i, moves) for i in range(n)])


def test_library_tables_equal_the_model():
	act, src, m = cube.sym_tables()
	want_act, want_src, want_m = model.tables()
	assert act.shape == (48, 12) and src.shape == (48, 20) and m.shape == (48, 20, 24)
	assert (act == want_act).all() and (src == want_src).all() and (m == want_m).all()
	assert cube.sym_actions().dtype == np.int64 and (cube.sym_actions() == want_act).all()
	# symmetry 0 is the identity, and the documented order: s = 8 p + m acts on the faces as the model's face_map says
	assert act[0].tolist() == list(range(12)) and src[0].tolist() == list(range(20)) and (m[0] == np.arange(24)).all()
	for s in range(48):
		assert (act[s] // 2).tolist() == [model.face_map(s)[a // 2] for a in range(12)]
	lib = _ffi.lib()
	assert lib.rk_sym_tables(None, None, None) == -1
	only = np.zeros((48, 12), np.uint8)
	assert lib.rk_sym_tables(only.ctypes.data, None, None) == 0 and (only == want_act).all()


def test_relabellings_are_distinct_permutations():
	act, src, m = model.tables()
	assert all(sorted(row) == list(range(12)) for row in act.tolist())
	assert len({tuple(row) for row in act.tolist()}) == 48
	assert all(sorted(row) == list(range(20)) for row in src.tolist())
	assert (np.sort(m, axis=2) == np.arange(24)).all()                        # every code map is a bijection
	# a relabelling maps inverse moves to inverse moves
	assert (act[:, np.arange(12) ^ 1] == act ^ 1).all()


def test_every_symmetry_keeps_solved():
	for s in range(48):
		assert (model.conjugate(orc.SOLVED, s)[0] == orc.SOLVED).all()


def test_conjugation_commutes_with_every_move():
	act, _, _ = model.tables()
	x = _scrambles()
	for s in range(48):
		cx = model.conjugate(x, s)
		for a in range(12):
			b = int(act[s, a])
			moved = orc.multi_rotate(x, np.full(len(x), a // 2), np.full(len(x), 1 - a % 2))
			want = orc.multi_rotate(cx, np.full(len(x), b // 2), np.full(len(x), 1 - b % 2))
			assert (model.conjugate(moved, s) == want).all(), (s, a)


def test_symmetries_are_closed_under_composition():
	x = _scrambles(8)
	conj = model.all_conjugates(x)                                             # (48, n, 20)
	keys = {conj[s].tobytes(): s for s in range(48)}
	assert len(keys) == 48                                                     # 48 distinct maps on these states
	table = np.zeros((48, 48), np.int64)
	for s in range(48):
		for t in range(48):
			table[s, t] = keys[model.conjugate(conj[t], s).tobytes()]           # KeyError: not closed
	assert all(sorted(row) == list(range(48)) for row in table.tolist())       # a group: every row a permutation
	assert (table[0] == np.arange(48)).all() and (table[:, 0] == np.arange(48)).all()
	# canonical forms do not depend on which member of the orbit is asked, and the orbit size is the number of distinct conjugates
	reps, syms, orbit = model.canonical(x)
	for s in (1, 17, 47):
		again, _, orbit2 = model.canonical(conj[s])
		assert (again == reps).all() and (orbit2 == orbit).all()
	assert (model.conjugate(x[:1], int(syms[0])) == reps[:1]).all()
	sym_states = np.stack([orc.SOLVED, orc.rotate(orc.SOLVED, 0, 1)])
	assert model.canonical(sym_states)[2].tolist() == [1, 12]


@pytest.mark.parametrize("kw", [dict(radius=-1), dict(radius=11), dict(radius=True), dict(radius=2.5),
                                dict(radius=2, pops=0), dict(radius=2, pops=1.5), dict(radius=2, pops=(1 << 22) + 1),
                                dict(radius=2, pops=True), dict(radius=2, capacity=0), dict(radius=2, capacity=-5),
                                dict(radius=2, capacity=2.5), dict(radius=2, capacity=True), dict(radius=2, capacity=1 << 31)])
def test_bad_arguments_are_refused_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceSymBall(**kw)


def test_good_arguments_and_library_checks():
	ball = DeviceSymBall(3, pops=5, capacity=100)
	assert (ball.radius, ball.pops, ball.capacity, ball._h, ball.built, ball.iterations) == (3, 5, 100, None, False, 0)
	assert DeviceSymBall(10).pops == 16_384 and DeviceSymBall(10).capacity is None and DeviceSymBall.MAX_RADIUS == 10
	assert DeviceSymBall.LEVELS == DeviceGoalBall.LEVELS
	assert str(ball) == "Symmetry-reduced goal ball (device, radius=3)"
	with pytest.raises(ValueError):
		cube.conjugate(np.zeros((1, 20), np.int8), 48)
	with pytest.raises(ValueError):
		cube.conjugate(np.zeros((1, 20), np.int8), True)
	lib = _ffi.lib()
	h = C.c_void_p()
	for radius, pops, cap in ((-1, 16, 0), (11, 16, 0), (2, 0, 0), (2, (1 << 22) + 1, 0), (2, 16, 0x3FFFFFF1)):
		assert lib.rk_symball_create(C.byref(h), radius, pops, cap) == -1 and h.value is None
	assert lib.rk_symball_create(None, 2, 16, 0) == -1
	buf = np.zeros(32, np.int64)
	assert lib.rk_symball_build(None, 8, None) == -1
	assert lib.rk_symball_status(None, buf.ctypes.data) == -1
	assert lib.rk_symball_export(None, 1, 1, buf.ctypes.data, None) == -1
	assert lib.rk_symball_depth(None, buf.ctypes.data, 1, buf.ctypes.data, None) == -1
	assert lib.rk_symball_solve(None, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None) == -1
	assert lib.rk_symball_destroy(None) == 0
	assert lib.rk_sym_canonical(None, 1, None, None, None, None) == -1
	assert lib.rk_sym_canonical(None, 0, None, None, None, None) == 0
	assert lib.rk_sym_conjugate(buf.ctypes.data, 1, 48, buf.ctypes.data, None) == -1 and b"symmetry" in lib.rk_last_error()
	assert lib.rk_sym_conjugate(buf.ctypes.data, 1, -1, buf.ctypes.data, None) == -1
	assert lib.rk_sym_conjugate(buf.ctypes.data, 1, 3, None, None) == -1
	# a ball that is created but not built allocates nothing, needs no device, and refuses every use
	_ffi.check(lib.rk_symball_create(C.byref(h), 4, 16, 0))
	try:
		assert lib.rk_symball_build(h, 0, None) == -1
		_ffi.check(lib.rk_symball_status(h, buf.ctypes.data))
		want_capacity = sum(-(-n * 102 // 4800) + 64 for n in DeviceSymBall.LEVELS[:5])
		assert buf[:6].tolist() == [0, 0, 0, 4, want_capacity, 2048] and not buf[6:].any()
		assert lib.rk_symball_export(h, 1, 1, buf.ctypes.data, None) == -4                           # RK_ESTATE: not built
		assert lib.rk_symball_depth(h, buf.ctypes.data, 1, buf.ctypes.data, None) == -4
		assert lib.rk_symball_solve(h, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None) == -4
	finally:
		assert lib.rk_symball_destroy(h) == 0


def test_without_a_gpu_everything_raises(monkeypatch):
	monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a machine that has a device: as if it had none)
	monkeypatch.setattr(_ffi, "_gpu_seen", False)
	ball = DeviceSymBall(2)
	one = scramble(1, 1)[None]
	for use in (ball.build, lambda: len(ball), lambda: ball.level_start, lambda: ball.states_covered, lambda: ball.depth(one),
	            lambda: ball.solve(one), ball.arrays, lambda: cube.canonical(one), lambda: cube.conjugate(one, 5)):
		with pytest.raises(_ffi.RubiksHipError):
			use()
	assert ball._h is None and not ball.built


def test_model_ball_covers_the_levels_of_the_graph():
	ball = model.build(4)
	assert ball.covered.tolist() == list(DeviceSymBall.LEVELS[:5]) == [1, 12, 114, 1_068, 10_011]
	assert np.diff(ball.level_start).tolist() == [1, 1, 5, 25, 219] and ball.len == 251 == len(ball.states) == len(ball.index)
	reps, syms, _ = model.canonical(ball.states)
	assert (reps == ball.states).all() and (syms == 0).all()                  # every stored state is its own representative
	# depth and the descent on states of known distance: 1..4-move scrambles lie inside, and every solution solves
	x = np.stack([scramble(1000 * d + s, d) for d in (1, 2, 3, 4) for s in range(6)])
	lengths, actions = model.solve(ball, x)
	assert (lengths == model.depth(ball, x)).all() and (lengths >= 0).all() and (lengths <= np.repeat([1, 2, 3, 4], 6)).all()
	for state, n, row in zip(x, lengths, actions):
		for a in row[:n]:
			state = orc.rotate(state, a // 2, 1 - a % 2)
		assert orc.is_solved(state) and (row[n:] == -1).all()
	assert model.depth(ball, scramble(20_000, 20)[None]).tolist() == [-1]
