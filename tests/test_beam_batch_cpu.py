"""
DeviceBeamSearchBatch without a GPU: the constructor and `search` refuse bad arguments before an engine is made; the class is a
direct `_NetStepped` subclass that adds no copy of the base's plumbing; the rk_beamb_* entries are declared, bound and exported
alike and refuse bad shapes and null handles before they touch a device; the Evaluator batches exactly `DeviceBeamSearch`; and,
on the model alone, the groups that tests/test_beam_batch_gpu.py compares bit for bit are not weak.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import _NetStepped, DeviceBeamSearch, DeviceBeamSearchBatch, DeviceSymBall
from librubiks_amd.solving.evaluation import Evaluator
from tests import beam_batch_groups as gg
from tests import beam_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rk_beamb_create", "rk_beamb_destroy", "rk_beamb_net_in", "rk_beamb_reset", "rk_beamb_rest", "rk_beamb_step", "rk_beamb_status",
           "rk_beamb_paths", "rk_beamb_export"]


class Net:
	def eval(self):
		return self


@pytest.mark.parametrize("kw", [dict(searches=0), dict(searches=1025), dict(searches=2.5), dict(searches=True), dict(width=0),
                                dict(width=1024, searches=65), dict(width=(1 << 16), searches=2), dict(max_depth=0), dict(max_depth=4097),
                                dict(poll=0), dict(ball=DeviceSymBall(3)), dict(ball=agents.DeviceGoalBall(2)), dict(ball=3)])
def test_constructor_refuses(kw):
	made = []
	with pytest.raises(ValueError):
		made.append(DeviceBeamSearchBatch(Net(), **{"width": 4, **kw}))
	assert not made


def test_constructor_and_search_refusals_make_no_engine():
	b = DeviceBeamSearchBatch(Net(), 22)
	assert (b.width, b.searches, b.max_depth, b.ball, b.prune_inverse, b.poll) == (22, 64, 64, None, True, 8)
	assert b._h is None and len(b) == 0 and b.captures == 0 and b.lockstep_depths == 0 and b.on_poll is None
	assert b.status.shape == (0, 12) and b.lengths.shape == (0,) and b.depths.shape == (0,) and b.meetings == []
	assert DeviceBeamSearchBatch(Net(), 64, searches=1024).searches == 1024 and DeviceBeamSearchBatch(Net(), 1 << 16, searches=1).width == 1 << 16
	states = np.zeros((3, 20), np.int8)
	for bad in (dict(max_states=[5, 5]), dict(max_states=[5, 5, 5, 5]), dict(max_states=np.zeros((3, 1), np.int64)), dict(max_states=-1),
	            dict(max_states=[5, -2, 5]), dict(max_states=2.5)):
		with pytest.raises(ValueError):
			b.search(states, **bad)
		assert b._h is None
	for shape in ((3, 19), (41,)):
		with pytest.raises(ValueError):
			b.search(np.zeros(shape, np.int8))
		assert b._h is None
	assert b.search(np.zeros((0, 20), np.int8)).shape == (0,) and b._h is None      # nothing to run: nothing is made
	with pytest.raises(ValueError):
		b.sizes_of(0)
	with pytest.raises(ValueError):
		b.back_of(0, 1)


def test_class_shape():
	b = DeviceBeamSearchBatch(Net(), 22, searches=3, max_depth=9)
	assert isinstance(b, _NetStepped) and DeviceBeamSearchBatch.__mro__[1] is _NetStepped
	for method in ("_net_in", "_free", "_net_batches", "_kept_steps", "_strict_ints"):
		assert method not in vars(DeviceBeamSearchBatch), method                    # one copy, the base's
	assert b._holders() == (b,)
	for _ in range(2):
		assert b._h is None and b.captures == 0 and b._batch is None and b._graph_cache is None
		b._free()


def test_abi_entries_in_header_binding_and_library():
	text = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
	exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
	lib = _ffi.lib()
	assert set(re.findall(r"\b(rk_beamb_[a-z0-9_]+)\s*\(", text)) == set(ENTRIES)
	assert {s for s in _ffi.SIGNATURES if s.startswith("rk_beamb_")} == set(ENTRIES)
	assert {s for s in exported if s.startswith("rk_beamb_")} == set(ENTRIES)
	for name in ENTRIES:
		assert getattr(lib, name) is not None


def test_create_refuses_bad_shapes_before_any_allocation():
	lib = _ffi.lib()
	h = C.c_void_p()
	for searches, width, depth in ((0, 4, 8), (1025, 4, 8), (-1, 4, 8), (4, 0, 8), (1, (1 << 16) + 1, 8), (65, 1024, 8), (2, 1 << 16, 8),
	                               (1024, 65, 8), (4, 4, 0), (4, 4, 4097)):
		assert lib.rk_beamb_create(C.byref(h), None, searches, width, depth, 1) == -1 and h.value is None, (searches, width, depth)
		assert lib.rk_last_error().startswith(b"rk_beamb_create: ")
	assert lib.rk_beamb_create(None, None, 4, 4, 8, 1) == -1 and lib.rk_last_error().startswith(b"rk_beamb_create: ")


def test_null_handles_are_refused():
	lib = _ffi.lib()
	buf = np.zeros(64, np.int64)
	ptr, rows = C.c_void_p(), C.c_size_t()
	calls = (("net_in", (None, 0, C.byref(ptr), C.byref(rows))), ("reset", (None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None)),
	         ("rest", (None, 1, buf.ctypes.data, None)), ("step", (None, buf.ctypes.data, 0, None)), ("status", (None, buf.ctypes.data, None)),
	         ("paths", (None, buf.ctypes.data, 8, None)), ("export", (None, 0, 1, buf.ctypes.data, buf.ctypes.data, 1, None)))
	assert {"rk_beamb_" + name for name, _ in calls} | {"rk_beamb_create", "rk_beamb_destroy"} == set(ENTRIES)
	for name, args in calls:
		assert getattr(lib, "rk_beamb_" + name)(*args) < 0, name
		assert lib.rk_last_error().startswith(b"rk_beamb_" + name.encode()), (name, lib.rk_last_error())
	assert lib.rk_beamb_destroy(None) == 0


def test_evaluator_batches_exactly_the_beam_search():
	class Sub(DeviceBeamSearch):
		pass
	net = Net()
	assert Evaluator.can_batch(DeviceBeamSearch(net, 22))
	assert not Evaluator.can_batch(Sub(net, 22))
	assert not Evaluator.can_batch(DeviceBeamSearchBatch(net, 22))
	assert not Evaluator.can_batch(agents.DeviceEGVM(net, 0.3, 4, 4))
	ev = Evaluator(4, [3], max_states=500)
	b = ev._batch_agent(DeviceBeamSearch(net, 22, 9, prune_inverse=False, poll=3), 4)
	assert type(b) is DeviceBeamSearchBatch and b.net is net
	assert (b.width, b.searches, b.max_depth, b.ball, b.prune_inverse, b.poll, b._fused_mode) == (22, 4, 9, None, False, 3, False)
	# more games than slots at this width: as many slots as the engine takes, the refill plays the rest
	assert ev._batch_agent(DeviceBeamSearch(net, 1 << 12), 64).searches == 16
	assert ev._batch_agent(DeviceBeamSearch(net, 1 << 16), 64).searches == 1
	assert ev._batch_agent(DeviceBeamSearch(net, 22, fused_first_layer="folded"), 2)._fused_mode == "folded"


def test_groups_are_not_weak():
	"""By the model alone: what the GPU groups hold between them."""
	results, kinds = [], dict.fromkeys(bm.KINDS, 0)
	for g in gg.GROUPS:
		assert g.states > g.slots, g
		assert g.width in bm.WIDTHS and g.slots * g.width <= DeviceBeamSearchBatch.MAX_BEAMS
		refs = gg.references(g)
		results += refs
		here = {k: sum(r.kinds[k] for r in refs) for k in bm.KINDS}
		if here["tie_cut"] and here["duplicates"]:
			kinds["tie_cut"] += 1
		assert len(gg.group_starts(g)) == g.states
	assert kinds["tie_cut"] >= 1                                             # a group with value ties across the cut AND duplicate children
	assert {g.prune for g in gg.GROUPS} == {True, False}
	assert len({r.depth for r in results if r.status == 1}) >= 3 and any(r.status == 3 for r in results)
	assert max(max(r.sizes) for r in gg.references(gg.GROUPS[-1])) == 1366     # the widest group fills its beam: 16 392 children in a depth
	assert max(max(r.sizes) for r in gg.references(gg.GROUPS[-2])) == 342
	# status 2 comes from the budgets: a state's own explored count still runs through, one below stops it
	budgets, refs = gg.budgets_and_references()
	free = gg.references(gg.BUDGET_GROUP)
	assert refs[gg.BUDGET_I][:3] == free[gg.BUDGET_I][:3] and budgets[gg.BUDGET_I] == free[gg.BUDGET_I].explored
	assert refs[gg.BUDGET_J].status == 2 and free[gg.BUDGET_J].status != 2 and budgets.count(None) == len(budgets) - 2
	# to the ball: starts inside it at the reset, wins at depths 1 and 3, the depth limit, and the solved start
	for net, width, slots, n in gg.BALL_GROUPS:
		refs = gg.ball_references(net, width, n)
		assert n + 1 > slots and len(gg.ball_starts(n)) == n + 1
		assert any(r.depth == 0 and r.meeting is not None and r.meeting[1] == -1 for r in refs)
		assert {1, 3} <= {r.depth for r in refs if r.status == 1} and any(r.status == 3 for r in refs)
		assert refs[-1].solved and refs[-1].meeting is None and refs[-1].queue == []
