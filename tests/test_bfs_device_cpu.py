"""
DeviceBFS without a GPU: arguments are checked before anything is launched, and the rk_bfs_* entries are declared, bound and
exported alike (include/rubiks_hip.h, librubiks_amd/_ffi.py, librubiks_hip.so).
"""
import os
import re
import subprocess

import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceBFS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_bfs_create", "rk_bfs_destroy", "rk_bfs_reset", "rk_bfs_set_budget", "rk_bfs_run", "rk_bfs_status", "rk_bfs_grow",
           "rk_bfs_size", "rk_bfs_export", "rk_bfs_path"]


@pytest.mark.parametrize("kw", [dict(pops=0), dict(pops=-3), dict(pops=1.5), dict(pops=(1 << 22) + 1), dict(pops=True),
                                dict(capacity=1), dict(capacity=0), dict(capacity=2.5), dict(capacity=1 << 31),
                                dict(max_capacity=1), dict(poll=0)])
def test_bad_arguments_are_refused_before_any_launch(kw):
	with pytest.raises(ValueError):
		DeviceBFS(**kw)


def test_good_arguments():
	a = DeviceBFS(pops=7, capacity=1_000, max_capacity=5_000, poll=3)
	assert (a.pops, a.capacity, a.max_capacity, a.poll) == (7, 1_000, 5_000, 3)
	assert len(a) == 0 and a._h is None and "Breadth-first search" in str(a)
	assert DeviceBFS().max_capacity == DeviceBFS.max_capacity


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	declared = set(re.findall(r"\b(rk_bfs_[a-z0-9_]+)\s*\(", text))
	assert declared == set(ENTRIES)
	assert set(ENTRIES) <= set(_ffi.SIGNATURES)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	assert set(ENTRIES) <= exported
	lib = _ffi.lib()
	for name in ENTRIES:
		assert getattr(lib, name) is not None


def test_library_refuses_bad_engine_arguments():
	import ctypes as C
	lib = _ffi.lib()
	h = C.c_void_p()
	assert lib.rk_bfs_create(C.byref(h), 1, 16) != 0 and h.value is None
	assert lib.rk_bfs_create(C.byref(h), 1000, 0) != 0 and h.value is None
	assert lib.rk_bfs_run(None, 1, None) != 0
	assert lib.rk_bfs_destroy(None) == 0
