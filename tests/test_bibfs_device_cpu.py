"""
DeviceBiBFS without a GPU: arguments are checked before anything is launched, the rk_bibfs_* entries are declared, bound and
exported alike, null handles are refused, a search without a device raises, and the plain-Python model of the protocol
(tests/bibfs_model.py) that the GPU tests compare against finds solutions as short as a one-sided breadth-first search.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceBiBFS
from tests import bibfs_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_bibfs_create", "rk_bibfs_destroy", "rk_bibfs_reset", "rk_bibfs_run", "rk_bibfs_status", "rk_bibfs_grow",
           "rk_bibfs_size", "rk_bibfs_export", "rk_bibfs_path"]


@pytest.mark.parametrize("kw", [dict(pops=0), dict(pops=-3), dict(pops=1.5), dict(pops=(1 << 22) + 1), dict(pops=True),
                                dict(capacity=1), dict(capacity=0), dict(capacity=2.5), dict(capacity=1 << 31),
                                dict(max_capacity=1), dict(poll=0)])
def test_bad_arguments_are_refused_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceBiBFS(**kw)


def test_good_arguments():
	a = DeviceBiBFS(pops=7, capacity=1_000, max_capacity=5_000, poll=3)
	assert (a.pops, a.capacity, a.max_capacity, a.poll) == (7, 1_000, 5_000, 3)
	assert len(a) == 0 and a._h is None and a.depths == (0, 0) and a.meeting is None
	assert str(a) == "Two-sided breadth-first search (device, pops=7)"
	assert DeviceBiBFS().max_capacity == DeviceBiBFS.max_capacity and DeviceBiBFS().pops == 16_384


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	declared = set(re.findall(r"\b(rk_bibfs_[a-z0-9_]+)\s*\(", text))
	assert declared == set(ENTRIES)
	assert {s for s in _ffi.SIGNATURES if s.startswith("rk_bibfs_")} == set(ENTRIES)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	assert {s for s in exported if s.startswith("rk_bibfs_")} == set(ENTRIES)
	lib = _ffi.lib()
	for name in ENTRIES:
		assert getattr(lib, name) is not None


def test_library_refuses_bad_engine_arguments():
	lib = _ffi.lib()
	h = C.c_void_p()
	assert lib.rk_bibfs_create(C.byref(h), 1, 16) != 0 and h.value is None
	assert lib.rk_bibfs_create(C.byref(h), 0x3FFFFFF1, 16) != 0 and h.value is None
	assert lib.rk_bibfs_create(C.byref(h), 1000, 0) != 0 and h.value is None
	assert lib.rk_bibfs_create(C.byref(h), 1000, (1 << 22) + 1) != 0 and h.value is None
	assert lib.rk_bibfs_create(None, 1000, 16) != 0
	buf = np.zeros(32, np.int64)
	start = model.scramble(1, 3)
	assert lib.rk_bibfs_reset(None, start.ctypes.data, 100, None) != 0
	assert lib.rk_bibfs_run(None, 1, None) != 0
	assert lib.rk_bibfs_status(None, buf.ctypes.data, None) != 0
	assert lib.rk_bibfs_grow(None, 1000, None) != 0
	assert lib.rk_bibfs_export(None, 1, 1, None, buf.ctypes.data, None, None, None) != 0
	assert lib.rk_bibfs_path(None, buf.ctypes.data, 16, None) < 0
	assert lib.rk_bibfs_size(None) == 0
	assert lib.rk_bibfs_destroy(None) == 0


def test_search_without_a_gpu_raises(monkeypatch):
	monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (on a machine that has a device: as if it had none)
	monkeypatch.setattr(_ffi, "_gpu_seen", False)
	agent = DeviceBiBFS(pops=7)
	with pytest.raises(_ffi.RubiksHipError):
		agent.search(model.scramble(1, 1), max_states=100)
	assert agent._h is None and len(agent) == 0


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_model_is_as_short_as_a_one_sided_search(depth):
	for seed in (0, 1, 2):
		start = model.scramble(100 * depth + seed, depth)
		want = model.one_sided_length(start, limit=depth)
		m = model.search(start)
		if want == 0:
			assert m.result and m.queue == [] and m.len == 0
			continue
		assert m.result and len(m.queue) == want <= depth and want % 2 == depth % 2
		assert model.orc.is_solved(model.apply(start, m.queue))
		assert m.depths == (want // 2, (want + 1) // 2 - 1)                          # S grows first: f = b or f = b + 1
		assert m.len == len(m.states) == len(m.parents) == len(m.actions) == len(m.sides)
		assert len({s.tobytes() for s in m.states}) == m.len                        # no state twice, on either side
		assert (m.meeting == model.apply(start, m.queue[:(want + 1) // 2])).all()      # the meeting lies on the solution


def test_model_budget_and_pool_order():
	start = model.scramble(7, 5)
	full = model.search(start)
	assert full.result
	# nodes 1 and 2, then levels alternate S, G, S, ...; a child follows its parent
	assert (full.states[0] == start).all() and (full.states[1] == model.orc.SOLVED).all()
	assert full.sides[:2].tolist() == [0, 1] and full.parents[:2].tolist() == [0, 0] and full.actions[:2].tolist() == [-1, -1]
	assert (full.parents[2:] < np.arange(3, full.len + 1)).all()
	assert (full.sides[full.parents[2:] - 1] == full.sides[2:]).all()
	for i in range(2, full.len):
		p, a = int(full.parents[i]), int(full.actions[i])
		assert (model.apply(full.states[p - 1], [a]) == full.states[i]).all()
	# a budget below two states stops before the first pop; one below the full size stops short with a prefix of the pool
	assert model.search(start, max_states=2).len == 2 and not model.search(start, max_states=2).result
	cut = model.search(start, max_states=full.len // 2)
	assert not cut.result and cut.queue == [] and cut.meeting is None
	assert full.len // 2 <= cut.len < full.len // 2 + 12
	assert (cut.states == full.states[:cut.len]).all() and (cut.parents == full.parents[:cut.len]).all()
