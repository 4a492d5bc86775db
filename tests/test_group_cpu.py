"""
The cube group on 20-byte states without a GPU: the library's compile-time tables (rk_group_tables) against the model's, which are
read off whole random words (tests/group_model.py); the rk_group_ entry set in the header, the binding and the library; every
argument check before a launch; and the model itself against ground truth that uses none of its tables -- the oracle's moves along
seeded words of 0..40 moves: composition is concatenation, the inverse is the reversed word of opposite turns, every scramble is
legal, legality is closed under the moves, and of the 12 variants of a legal state exactly one is legal.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from tests import group_model as model

orc = model.orc
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rk_group_tables", "rk_group_apply", "rk_group_inverse", "rk_group_relative", "rk_group_legal"}
N = 615                                                                  # 15 words of every length 0..40


def _along(states: np.ndarray, lengths: np.ndarray, actions: np.ndarray) -> np.ndarray:
	"""Every state moved along its own word, with the oracle's multi_rotate."""
	s = np.array(states, np.int8)
	for t in range(actions.shape[1]):
		live = lengths > t
		moved = orc.multi_rotate(s, actions[:, t] // 2, 1 - actions[:, t] % 2)
		s = np.where(live[:, None], moved, s)
	return s


def _scr(lengths, actions) -> np.ndarray:
	return _along(orc.repeat_state(orc.SOLVED, len(lengths)), lengths, actions)


def _words(seed: int, flip: bool = False):
	lengths, actions = model.word_actions(seed, N)
	return (lengths[::-1].copy() if flip else lengths), actions


def _reversed(lengths, actions):
	"""Every word reversed, every turn the opposite one."""
	out = np.zeros_like(actions)
	for i, n in enumerate(lengths):
		out[i, :n] = actions[i, :n][::-1] ^ 1
	return lengths, out


def test_library_tables_equal_the_model():
	full, inv, tau = cube.group_tables()
	want_full, want_inv, want_tau = model.tables()
	assert full.shape == (2, 12, 24, 3) and inv.shape == (2, 12, 24) and tau.shape == (24,)
	assert full.tobytes() == want_full.tobytes() and inv.tobytes() == want_inv.tobytes() and tau.tobytes() == want_tau.tobytes()
	assert not tau[::3].any() and sorted(set(tau.tolist())) == [0, 1, 2]    # zero on the home codes
	lib = _ffi.lib()
	assert lib.rk_group_tables(None, None, None) == -1 and b"rk_group_tables" in lib.rk_last_error()
	only = np.zeros(24, np.uint8)
	assert lib.rk_group_tables(None, None, only.ctypes.data) == 0 and (only == want_tau).all()


def test_entry_set():
	text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rubiks_hip.h")).read(), flags=re.S)
	assert {s for s in re.findall(r"\b(rk_[a-z0-9_]+)\s*\(", text) if s.startswith("rk_group_")} == ENTRIES
	assert {s for s in _ffi.SIGNATURES if s.startswith("rk_group_")} == ENTRIES
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	assert {s for s in exported if s.startswith("rk_group_")} == ENTRIES
	assert int(re.search(r"#define\s+RK_GROUP_GRID\s+(\d+)", text).group(1)) * 256 == cube.device.GROUP_PASS_ROWS


def test_arguments_are_refused_before_any_launch():
	lib = _ffi.lib()
	a, b, c = 0x10000, 0x20000, 0x30000                                  # never dereferenced: every call below returns before a launch
	big = (1 << 31)

	def refused(rc, name, word):
		assert rc == -1 and lib.rk_last_error().startswith(name.encode() + b": ") and word in lib.rk_last_error(), (rc, lib.rk_last_error())
	for name in ("rk_group_apply", "rk_group_relative"):
		f = getattr(lib, name)
		refused(f(None, 5, b, 5, c, None), name, b"null pointer")
		refused(f(a, 5, None, 5, c, None), name, b"null pointer")
		refused(f(a, 5, b, 5, None, None), name, b"null pointer")
		refused(f(a + 2, 5, b, 5, c, None), name, b"aligned")
		refused(f(a, 5, b + 1, 5, c, None), name, b"aligned")
		refused(f(a, 5, b, 5, c + 3, None), name, b"aligned")
		refused(f(a, big, b, big, c, None), name, b"states in one launch")
		for m in (0, 2, 4, 6):
			refused(f(a, 5, b, m, c, None), name, b"second operands")
		refused(f(a, 0, b, 2, c, None), name, b"second operands")
		refused(f(a, 5, b, 5, a + 20, None), name, b"overlaps")          # shifted by a row
		refused(f(a, 5, b, 5, b - 40, None), name, b"overlaps")
		refused(f(a, 5, b, 1, b, None), name, b"overlaps")               # the one row every thread reads
		refused(f(a, 5, a + 80, 1, a + 60, None), name, b"overlaps")
		assert f(None, 0, None, 0, None, None) == 0 and f(a, 0, b, 1, c, None) == 0
	f, name = lib.rk_group_inverse, "rk_group_inverse"
	refused(f(None, 5, c, None), name, b"null pointer")
	refused(f(a, 5, None, None), name, b"null pointer")
	refused(f(a + 1, 5, c, None), name, b"aligned")
	refused(f(a, 5, c + 2, None), name, b"aligned")
	refused(f(a, big, c, None), name, b"states in one launch")
	refused(f(a, 5, a + 4, None), name, b"overlaps")
	assert f(None, 0, None, None) == 0
	f, name = lib.rk_group_legal, "rk_group_legal"
	refused(f(None, 5, b, c, None), name, b"null pointer")
	refused(f(a, 5, None, None, None), name, b"null pointer")
	refused(f(a + 2, 5, b, c, None), name, b"aligned")
	refused(f(a, 5, b, c + 4, None), name, b"8-byte")
	refused(f(a, big, b, c, None), name, b"states in one launch")
	refused(f(a, 5, a + 99, c, None), name, b"overlap")
	assert f(None, 0, None, None, None) == 0


def test_without_a_gpu_everything_raises(monkeypatch):
	import torch
	monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a machine that has a device: as if it had none)
	monkeypatch.setattr(_ffi, "_gpu_seen", False)
	s = orc.SOLVED[None]
	for use in (lambda: cube.apply_state(s, s), lambda: cube.inverse(s), lambda: cube.relative(s, s), lambda: cube.is_legal(s)):
		with pytest.raises(_ffi.RubiksHipError):
			use()


def test_model_apply_is_concatenation():
	(la, aa), (lb, ab) = _words(11), _words(12, flip=True)
	a, b = _scr(la, aa), _scr(lb, ab)
	assert (model.apply(a, b) == _along(a, lb, ab)).all()
	assert (model.apply(a, b[7:8]) == _along(a, np.repeat(lb[7:8], N), np.repeat(ab[7:8], N, axis=0))).all()     # one effect for all
	assert (model.apply(a, orc.SOLVED) == a).all() and (model.apply(orc.repeat_state(orc.SOLVED, N), b) == b).all()
	for m in range(12):
		assert (model.apply(a, orc.rotate(orc.SOLVED, m // 2, 1 - m % 2)) == orc.multi_rotate(a, np.full(N, m // 2), np.full(N, 1 - m % 2))).all()


def test_model_inverse_is_the_reversed_word():
	la, aa = _words(13)
	a = _scr(la, aa)
	inv = model.inverse(a)
	assert (inv == _scr(*_reversed(la, aa))).all()
	solved = orc.repeat_state(orc.SOLVED, N)
	assert (model.apply(a, inv) == solved).all() and (model.apply(inv, a) == solved).all() and (model.inverse(inv) == a).all()


def test_model_relative():
	(la, aa), (lb, ab) = _words(14), _words(15, flip=True)
	goal = _scr(la, aa)
	s = _along(goal, lb, ab)                                               # the goal moved along a word: seen from the goal, the word's state
	assert (model.relative(s, goal) == _scr(lb, ab)).all()
	assert (model.relative(goal, goal) == orc.SOLVED).all()
	other = _scr(lb, ab)
	for m in range(12):
		f, d = np.full(N, m // 2), np.full(N, 1 - m % 2)
		assert (model.relative(orc.multi_rotate(other, f, d), goal) == orc.multi_rotate(model.relative(other, goal), f, d)).all()
		assert (model.relative(orc.multi_rotate(other, f, d), goal[3]) == orc.multi_rotate(model.relative(other, goal[3]), f, d)).all()


def test_model_legality():
	la, aa = _words(16)
	a = _scr(la, aa)
	assert model.is_legal(a).all() and model.is_legal(orc.SOLVED).all()
	var = np.concatenate([model.variants(s) for s in a[::5]])              # 123 states x 12
	legal = model.is_legal(var).reshape(-1, 12)
	assert legal[:, 0].all() and legal.sum(axis=1).tolist() == [1] * len(legal)
	for m in range(12):                                                    # closed under the moves, for legal and illegal states alike
		moved = orc.multi_rotate(var, np.full(len(var), m // 2), np.full(len(var), 1 - m % 2))
		assert (model.is_legal(moved) == legal.reshape(-1)).all()
	bad = np.repeat(a[40:41], 8, axis=0)
	for row, (at, code) in enumerate(((0, 24), (7, 127), (8, -1), (19, -128), (3, 31), (12, 24))):
		bad[row, at] = code
	bad[6, 1] = bad[6, 0]                                                  # a repeated corner position (and code)
	bad[7, 9] = bad[7, 8] ^ 1                                              # a repeated edge position
	assert not model.is_legal(bad).any()
