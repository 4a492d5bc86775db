"""
DeviceEGVM without a GPU: arguments are checked before anything is launched, the rk_egvm_* entries are declared, bound and
exported alike (include/rubiks_hip.h, librubiks_amd/_ffi.py, librubiks_hip.so), and the draw schedule -- the host's half of the
agent -- makes the reference's calls in the reference's order (ref:librubiks/solving/agents.py:694, :698) and leaves the global
NumPy generator where the reference leaves it.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceEGVM, EGVM, egvm_draw_rounds, egvm_rewind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_egvm_create", "rk_egvm_destroy", "rk_egvm_reset", "rk_egvm_set_draws", "rk_egvm_net_in", "rk_egvm_step",
           "rk_egvm_round_end", "rk_egvm_status", "rk_egvm_records"]


class Net:
	def eval(self):
		return self


@pytest.mark.parametrize("kw", [dict(workers=0), dict(workers=-2), dict(workers=1.5), dict(workers=True), dict(workers=(1 << 16) + 1),
                                dict(depth=0), dict(depth=2.0), dict(depth=(1 << 12) + 1), dict(workers=1 << 16, depth=1 << 7),
                                dict(poll=0), dict(poll=False), dict(poll=(1 << 12) + 1), dict(workers=1 << 10, depth=1 << 10, poll=1 << 9),
                                dict(epsilon=-0.1), dict(epsilon=1.5), dict(epsilon="0.3"), dict(epsilon=None), dict(epsilon=float("nan")),
                                dict(fused_first_layer="sometimes")])
def test_bad_arguments_are_refused_before_any_launch(kw):
	args = dict(epsilon=0.3, workers=10, depth=50)
	args.update(kw)
	with pytest.raises(ValueError):
		DeviceEGVM(Net(), **args)


def test_good_arguments():
	a = DeviceEGVM(Net(), epsilon=0.375, workers=10, depth=50, poll=3)
	assert (a.epsilon, a.workers, a.depth, a.poll) == (0.375, 10, 50, 3)
	assert len(a) == 0 and a._h is None and a.captures == 0 and not a.action_queue
	assert "device" in str(a) and str(a) != str(EGVM(Net(), 0.375, 10, 50))
	assert DeviceEGVM(Net(), 0, 1, 1).poll == 4 and DeviceEGVM(Net(), 1, np.int64(3), np.int32(2)).workers == 3
	seen = []
	b = DeviceEGVM.from_saved("folder", True, epsilon=0.3, workers=10, depth=50, loader=lambda loc, best: (seen.append((loc, best)), Net())[1])
	assert isinstance(b.net, Net) and (b.epsilon, b.workers, b.depth) == (0.3, 10, 50) and seen == [("folder", True)]


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	declared = set(re.findall(r"\b(rk_egvm_[a-z0-9_]+)\s*\(", text))
	assert declared == set(ENTRIES)
	assert set(ENTRIES) <= set(_ffi.SIGNATURES)
	assert {n for n in _ffi.SIGNATURES if n.startswith("rk_egvm_")} == set(ENTRIES)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	assert set(ENTRIES) <= exported
	lib = _ffi.lib()
	for name in ENTRIES:
		assert getattr(lib, name) is not None


def test_library_refuses_bad_engine_arguments():
	lib = _ffi.lib()
	h = C.c_void_p()
	for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (-1, 5, 1), ((1 << 16) + 1, 1, 1), (1, (1 << 12) + 1, 1), (1, 1, (1 << 12) + 1),
	            (1 << 16, 1 << 7, 1), (1 << 10, 1 << 10, 1 << 9)):
		assert lib.rk_egvm_create(C.byref(h), *bad) == -1 and h.value is None, bad
	assert lib.rk_egvm_create(None, 5, 5, 1) == -1
	root = np.zeros(20, np.int8)
	ptr, rows = C.c_void_p(), C.c_size_t()
	assert lib.rk_egvm_reset(None, root.ctypes.data, 100, None) != 0
	assert lib.rk_egvm_set_draws(None, root.ctypes.data, 1, None) != 0
	assert lib.rk_egvm_net_in(None, 0, 0, C.byref(ptr), C.byref(rows)) != 0
	assert lib.rk_egvm_step(None, 16, 0, None) != 0
	assert lib.rk_egvm_round_end(None, 16, 0, None) != 0
	assert lib.rk_egvm_status(None, root.ctypes.data, None) != 0
	assert lib.rk_egvm_records(None, 0, 1, root.ctypes.data, None) != 0
	assert lib.rk_egvm_destroy(None) == 0


def reference_draws(eps, W, D, rounds, end):
	"""What the reference draws (ref:agents.py:692-698, the loop of :665 around it) in a search of `rounds` full rounds, or one that
	ends by a solve after `end[1]` moves of round `end[0]`: the two calls of every depth, written out.  -> the (round, depth, W)
	table of actions (-1: follow the policy) of the depths that were drawn (-2 elsewhere)."""
	table = np.full((rounds, D, W), -2, np.int64)
	for r in range(rounds):
		for d in range(D):
			use_random = np.random.choice(2, W, p=[1 - eps, eps]).astype(bool)
			actions = np.full(W, -1)
			actions[use_random] = np.random.randint(0, 12, use_random.sum())
			table[r, d] = actions
			if end is not None and end == (r, d + 1):
				return table
	return table


@pytest.mark.parametrize("eps, W, D, rounds, end, poll", [
	(0.375, 10, 50, 3, None, 4), (0.375, 10, 50, 5, (4, 50), 2), (0.3, 20, 8, 7, (2, 1), 4), (0.5, 16, 6, 6, (5, 3), 4), (0.5, 16, 6, 6, (0, 2), 1),
	(0.0, 8, 10, 4, (3, 10), 3), (0.0, 8, 10, 4, None, 1), (1.0, 16, 6, 5, (1, 4), 5), (1.0, 3, 4, 2, None, 8), (0.6, 1, 50, 5, (3, 17), 2),
	(0.9, 7, 1, 9, (8, 1), 4), (0.25, 1, 1, 3, None, 2)])
def test_draw_schedule_is_the_references(eps, W, D, rounds, end, poll):
	"""The agent draws bursts of `poll` whole rounds ahead of the device, never beyond the rounds the budget allows, and rewinds
	when the search ends inside a round: the table the device gets and the generator afterwards are the reference's."""
	seed = 1234 + 7 * W + D
	np.random.seed(seed)
	want = reference_draws(eps, W, D, rounds, end)
	want_next = np.random.randint(0, 2 ** 31 - 1)
	np.random.seed(seed)
	got = np.full((rounds, D, W), -2, np.int64)
	drawn = 0
	while drawn < rounds:
		n = min(poll, rounds - drawn)                           # `rounds` stands for max_states // (W * D)
		table, before = egvm_draw_rounds(eps, W, D, n)
		assert table.dtype == np.int8 and table.shape == (n, D, W) and len(before) == n and table.flags.c_contiguous
		assert table.min() >= -1 and table.max() <= 11
		if end is not None and drawn <= end[0] < drawn + n:     # the device reports a solve in this burst
			k = end[0] - drawn
			got[drawn:drawn + k] = table[:k]
			again = egvm_rewind(before[k], eps, W, end[1])
			assert again.shape == (end[1], W) and (again == table[k, :end[1]]).all()
			got[end[0], :end[1]] = again
			break
		got[drawn:drawn + n] = table
		drawn += n
	assert (got == want).all()
	assert np.random.randint(0, 2 ** 31 - 1) == want_next
	if eps == 0.0:
		assert (got[got > -2] == -1).all()
	if eps == 1.0:
		assert (got[got > -2] >= 0).all()
