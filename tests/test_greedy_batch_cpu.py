"""
GreedyBatch without a GPU: arguments are checked before anything is launched, the rk_greedy_* entries are declared, bound and
exported alike (include/rubiks_hip.h, librubiks_amd/_ffi.py, librubiks_hip.so), the library refuses bad arguments, and the
Evaluator offers the lock-step form for exactly the one-step agents that draw nothing while they play.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import GreedyBatch
from librubiks_amd.solving.evaluation import Evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_greedy_create", "rk_greedy_destroy", "rk_greedy_net_in", "rk_greedy_reset", "rk_greedy_step", "rk_greedy_status",
           "rk_greedy_export"]


class Net:
	def eval(self):
		return self


@pytest.mark.parametrize("kw", [dict(mode="sampled"), dict(mode=None), dict(mode=0), dict(mode=True), dict(mode="Policy"),
                                dict(games=0), dict(games=-3), dict(games=2.0), dict(games=True), dict(games="4"), dict(games=(1 << 16) + 1),
                                dict(poll=0), dict(poll=False), dict(poll=1.5), dict(poll=(1 << 12) + 1), dict(fused_first_layer="sometimes")])
def test_bad_arguments_are_refused_before_any_launch(kw):
	args = dict(mode="policy", games=8)
	args.update(kw)
	with pytest.raises(ValueError):
		GreedyBatch(Net(), **args)


@pytest.mark.parametrize("max_states", [None, 0, -1, 2.5, True, "7", (1 << 30) // 8 + 1])
def test_bad_budgets_are_refused_before_any_launch(max_states):
	"""`search` checks its budget before it asks for a device (on a machine without one, the device is what it would miss next)."""
	a = GreedyBatch(Net(), "value", 8)
	with pytest.raises(ValueError, match="max_states"):
		a.search(np.zeros((1, 20), np.int8), max_states=max_states)
	assert a._h is None and a.captures == 0


def test_good_arguments():
	a = GreedyBatch(Net(), "value", 5, poll=3)
	assert (a.mode, a.games, a.poll) == ("value", 5, 3)
	assert len(a) == 0 and a._h is None and a.captures == 0 and a.on_poll is None
	assert a.status.shape == a.steps.shape == a.handed_back.shape == (0,)
	b = GreedyBatch(Net(), "policy", np.int64(1 << 16), np.int32(1 << 12))
	assert (b.mode, b.games, b.poll) == ("policy", 1 << 16, 1 << 12) and GreedyBatch(Net(), "policy", 1).poll == 8
	assert "policy" in str(b) and "value" in str(a) and str(a) != str(agents.ValueSearch(Net()))
	assert "max_states" in GreedyBatch.__doc__ and "sample_policy" in GreedyBatch.__doc__ and "RandomSearch" in GreedyBatch.__doc__


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	declared = set(re.findall(r"\b(rk_greedy_[a-z0-9_]+)\s*\(", text))
	assert declared == set(ENTRIES)
	assert {n for n in _ffi.SIGNATURES if n.startswith("rk_greedy_")} == set(ENTRIES)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	assert set(ENTRIES) <= exported
	assert {s for s in exported if s.startswith("rk_greedy_")} == set(ENTRIES)
	lib = _ffi.lib()
	for name in ENTRIES:
		assert getattr(lib, name) is not None


def test_library_refuses_bad_engine_arguments():
	lib = _ffi.lib()
	h = C.c_void_p()
	for bad in ((0, 5, 0), (-1, 5, 1), ((1 << 16) + 1, 1, 0), (5, 0, 0), (5, -7, 1), (5, 5, 2), (5, 5, -1), (1 << 16, (1 << 14) + 1, 0),
	            (3, (1 << 30) // 3 + 1, 1)):
		assert lib.rk_greedy_create(C.byref(h), *bad) == -1 and h.value is None, bad
		assert b"rk_greedy_create" in lib.rk_last_error()
	assert lib.rk_greedy_create(None, 5, 5, 0) == -1
	root = np.zeros(20, np.int8)
	buf = np.zeros(8, np.int64)
	ptr, rows = C.c_void_p(), C.c_size_t()
	assert lib.rk_greedy_net_in(None, 0, C.byref(ptr), C.byref(rows)) != 0
	assert lib.rk_greedy_reset(None, root.ctypes.data, 1, 10, None) != 0
	assert lib.rk_greedy_step(None, 16, 0, None) != 0
	assert lib.rk_greedy_status(None, buf.ctypes.data, None) != 0
	assert lib.rk_greedy_export(None, buf.ctypes.data, buf.ctypes.data, None, None) != 0
	assert lib.rk_greedy_destroy(None) == 0


class Sub(agents.ValueSearch):
	pass


class SubPolicy(agents.PolicySearch):
	pass


def test_evaluator_offers_lock_step_to_the_agents_that_draw_nothing():
	net = Net()
	assert Evaluator.can_batch(agents.ValueSearch(net))
	assert Evaluator.can_batch(agents.PolicySearch(net)) and Evaluator.can_batch(agents.PolicySearch(net, sample_policy=False))
	assert not Evaluator.can_batch(agents.PolicySearch(net, sample_policy=True))
	assert not Evaluator.can_batch(agents.RandomSearch())
	assert not Evaluator.can_batch(agents.EGVM(net, 0.3, 4, 4))
	assert not Evaluator.can_batch(agents.DeviceEGVM(net, 0.3, 4, 4))
	assert not Evaluator.can_batch(agents.BFS())
	assert not Evaluator.can_batch(Sub(net)) and not Evaluator.can_batch(SubPolicy(net))
	assert not Evaluator.can_batch(GreedyBatch(net, "value", 4))
	ev = Evaluator(3, [2, 4], max_states=50)
	assert ev.replayed == 0
	b = ev._batch_agent(agents.ValueSearch(net), 6)
	assert isinstance(b, GreedyBatch) and (b.mode, b.games, b.net) == ("value", 6, net)
	b = ev._batch_agent(agents.PolicySearch(net), 2)
	assert isinstance(b, GreedyBatch) and (b.mode, b.games, b.net) == ("policy", 2, net)
