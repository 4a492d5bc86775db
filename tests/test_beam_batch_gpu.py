"""
DeviceBeamSearchBatch (engine rk_beamb_*) on the GPU: every state of a batch gets what the plain-Python model of
tests/beam_model.py gives it ALONE, bit for bit -- solved, status, depth, states explored, sizes, every back row, the meeting and
the queue --, whatever slot it ran in, whenever it was started and whatever `searches` and `poll` are.  The groups and their
answers are tests/beam_batch_groups.py's; tests/test_beam_batch_cpu.py shows on the model alone that they are not weak.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube, gpu
from librubiks_amd.solving import _engine as eng
from librubiks_amd.solving.agents import DeviceBeamSearch, DeviceBeamSearchBatch, DeviceSymBall
from librubiks_amd.solving.evaluation import Evaluator
from oracle import cube_oracle as orc
from tests import beam_batch_groups as gg
from tests import beam_model as bm
from tests.repr686_nets import NoisyStubNet686

pytestmark = pytest.mark.gpu


def _device_net(name: str):
	net = bm.net_of(name)
	return net.to(gpu) if isinstance(net, torch.nn.Module) else net


def _batch(g, **kw) -> DeviceBeamSearchBatch:
	kw = {"searches": g.slots, "max_depth": g.max_depth, "prune_inverse": g.prune, "fused_first_layer": g.net == "linear_bf16", **kw}
	return DeviceBeamSearchBatch(_device_net(g.net), g.width, **kw)


def _rotate_all(state, queue):
	for a in queue:
		state = cube.rotate(state, *cube.action_space[a])
	return state


def _same(b: DeviceBeamSearchBatch, i: int, solved, ref: bm.Result, what):
	"""What tests/test_beam_gpu.py::_same compares of the single agent, of state i of the batch."""
	assert bool(solved[i]) == ref.solved, what
	assert (int(b.status[i, 0]), int(b.depths[i]), int(b.status[i, 2])) == (ref.status, ref.depth, ref.explored), what
	assert b.sizes_of(i).tolist() == ref.sizes, what
	for t in range(1, len(ref.sizes)):
		assert np.array_equal(b.back_of(i, t), ref.back[t]), (what, t)
	assert b.meetings[i] == ref.meeting, what
	assert list(b.action_queue_of(i)) == ref.queue, what
	assert int(b.lengths[i]) == (len(ref.queue) if ref.solved else -1), what


def _all_same(b, solved, refs, starts, what):
	assert len(solved) == len(refs)
	for i, ref in enumerate(refs):
		_same(b, i, solved, ref, (what, i))
		if ref.solved:
			assert cube.is_solved(_rotate_all(starts[i], b.action_queue_of(i))), (what, i)
	assert len(b) == sum(r.explored for r in refs)


@pytest.mark.parametrize("g", gg.GROUPS, ids=gg.group_id)
def test_groups_against_model(g):
	starts, refs = gg.group_starts(g), gg.references(g)
	b = _batch(g)
	_all_same(b, b.search(starts, keep_arrays=True), refs, starts, g)
	assert b.captures == 1 and b.lockstep_depths >= max(r.depth for r in refs)


@pytest.mark.parametrize("searches, poll", [(1, 1), (1, 8), (3, 1), (3, 8), (7, 1), (7, 8)])
def test_slot_and_order_independence(searches, poll):
	g = gg.GROUPS[3]
	starts, refs = gg.group_starts(g), gg.references(g)
	b = _batch(g, searches=searches, poll=poll)
	_all_same(b, b.search(starts, keep_arrays=True), refs, starts, (searches, poll))
	_all_same(b, b.search(starts[::-1], keep_arrays=True), refs[::-1], starts[::-1], (searches, poll, "reversed"))
	assert b.captures == 1


def test_budgets_per_state():
	g = gg.BUDGET_GROUP
	starts = gg.group_starts(g)
	budgets, refs = gg.budgets_and_references()
	assert refs[gg.BUDGET_J].status == 2 and refs[gg.BUDGET_I].status == 1
	b = _batch(g)
	_all_same(b, b.search(starts, max_states=budgets, keep_arrays=True), refs, starts, "budgets")
	free = gg.references(g)                                                   # one budget for all: the largest explored count stops nobody
	_all_same(b, b.search(starts, max_states=max(r.explored for r in free), keep_arrays=True), free, starts, "one budget")
	assert b.captures == 1


@pytest.fixture(scope="module")
def ball():
	return DeviceSymBall(bm.BALL_RADIUS).build()


@pytest.mark.parametrize("net, width, slots, n", gg.BALL_GROUPS)
def test_to_the_ball(ball, net, width, slots, n):
	starts, refs = gg.ball_starts(n), gg.ball_references(net, width, n)
	b = DeviceBeamSearchBatch(_device_net(net), width, searches=slots, max_depth=12, ball=ball)
	solved = b.search(starts, keep_arrays=True)
	_all_same(b, solved, refs, starts, (net, width))
	inside = [i for i, r in enumerate(refs) if r.meeting is not None and r.meeting[1] == -1]
	assert inside
	for i in inside:
		assert b.depths[i] == 0 and b.meetings[i][1] == -1
	for i in np.nonzero(solved)[0][:-1]:
		assert len(b.action_queue_of(i)) == b.depths[i] + b.meetings[i][2]
	assert solved[-1] and b.meetings[n] is None and b.lengths[n] == 0 and not b.status[n, 1:].any()      # the solved start: the host's answer


def _rows_of(batch: torch.Tensor, slot: int, width: int) -> np.ndarray:
	return batch.cpu().numpy()[slot * 12 * width:(slot + 1) * 12 * width]


def _record_of(lib, h, slot: int, depth: int, width: int):
	sizes = np.zeros(depth + 1, np.int64)
	_ffi.check(lib.rk_beamb_export(h, slot, 0, sizes.ctypes.data, None, 0, _ffi.stream_ptr()))
	back = np.zeros((depth + 1, width), np.int64)
	for t in range(1, depth + 1):
		_ffi.check(lib.rk_beamb_export(h, slot, t, None, back[t].ctypes.data, width, _ffi.stream_ptr()))
	return sizes, back


def _reset(lib, h, slots, starts, budgets=None):
	sl, rows = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(starts, np.int8)
	budgets = np.full(len(sl), 1 << 40, np.int64) if budgets is None else np.ascontiguousarray(budgets, np.int64)
	return lib.rk_beamb_reset(h, len(sl), sl.ctypes.data, rows.ctypes.data, budgets.ctypes.data, _ffi.stream_ptr())


def _status(lib, h, slots: int) -> np.ndarray:
	st = np.zeros((slots, 12), np.int64)
	_ffi.check(lib.rk_beamb_status(h, st.ctypes.data, _ffi.stream_ptr()))
	return st


def test_refill_leaves_the_other_slots_alone():
	"""On the 20-byte rows of the fused first layer: slot 2 is started again between two replays, slot 0 is mid-search."""
	g = gg.GROUPS[5]
	W, D = g.width, g.max_depth
	starts = gg.starts_of(9)
	a, c, other = starts[4], starts[8], starts[3]                             # (9-, 6- and 6-move scrambles)
	b = _batch(g)
	b.search(starts[:1])                                                      # makes the engine, the batch and the kept step; uses slot 0
	lib, h, batch, graph = _ffi.lib(), b._h, b._batch[1], b._graph_cache[1]
	assert batch.shape == (3 * 12 * W, 20) and batch.dtype == torch.int8
	assert _status(lib, h, 3)[:, 0].tolist() == [1, 5, 5]                     # slots 1 and 2 were never started: at rest
	_ffi.check(_reset(lib, h, [0, 2], [a, c]))
	for _ in range(2):
		graph.replay()
	st = _status(lib, h, 3)
	assert st[:, 0].tolist() == [0, 5, 0] and st[[0, 2], 9].tolist() == [2, 2]
	rows0, record0 = _rows_of(batch, 0, W), _record_of(lib, h, 0, D, W)
	assert (_rows_of(batch, 2, W)[12:] != orc.SOLVED).any()                    # slot 2 has moved on from what its reset wrote
	_ffi.check(_reset(lib, h, [2], [other]))
	st2 = _status(lib, h, 3)
	assert (st2[0] == st[0]).all() and st2[1, 0] == 5 and st2[2].tolist()[:4] == [0, 0, 0, 1]
	assert (_rows_of(batch, 0, W) == rows0).all()
	for x, y in zip(_record_of(lib, h, 0, D, W), record0):
		assert np.array_equal(x, y)
	rows2 = _rows_of(batch, 2, W)
	assert (rows2[:12] == orc.expand12(other[None])).all() and (rows2[12:] == orc.SOLVED).all()
	assert (_rows_of(batch, 1, W) == orc.SOLVED).all()
	sl = np.array([0, 2], np.int32)
	_ffi.check(lib.rk_beamb_rest(h, 2, sl.ctypes.data, _ffi.stream_ptr()))       # as the agent leaves it: nothing running
	assert _status(lib, h, 3)[:, 0].tolist() == [5, 5, 5]
	ref = gg.alone(g.net, W, D, g.prune, 4)
	solved = b.search(starts[4:5], keep_arrays=True)                          # and the agent goes on from there
	_same(b, 0, solved, ref, "after the raw calls")


def test_first_reset_in_a_form_writes_every_row_of_every_slot():
	lib = _ffi.lib()
	W = 22
	starts = gg.starts_of(9)
	h = C.c_void_p()
	_ffi.check(lib.rk_beamb_create(C.byref(h), None, 3, W, 12, 1))
	try:
		ptr, rows = C.c_void_p(), C.c_size_t()
		buf = np.zeros(64, np.int64)
		assert _reset(lib, h, [0], starts[:1]) == -4                          # RK_ESTATE: no form yet
		assert lib.rk_beamb_step(h, buf.ctypes.data, _ffi.OH_F32, _ffi.stream_ptr()) == -4
		_ffi.check(lib.rk_beamb_net_in(h, _ffi.OH_STATES, C.byref(ptr), C.byref(rows)))
		assert rows.value == 3 * 12 * W
		assert lib.rk_beamb_step(h, buf.ctypes.data, _ffi.OH_F32, _ffi.stream_ptr()) == -4      # no row is legal yet: no forward may read them
		batch = eng.engine_batch(ptr.value, rows.value, _ffi.OH_STATES)
		batch.fill_(77)                                                       # no cubie code
		torch.cuda.synchronize()
		bad = starts[:2].copy()
		bad[1, 7] = 24
		assert _reset(lib, h, [0, 2], bad) == -1 and b"start 1" in lib.rk_last_error()
		assert _reset(lib, h, [0, 0], starts[:2]) == -1 and _reset(lib, h, [0, 3], starts[:2]) == -1
		assert _reset(lib, h, [0], starts[:1], [-1]) == -1
		assert (batch.cpu().numpy() == 77).all()                              # the refusals came before anything was enqueued
		_ffi.check(_reset(lib, h, [0, 2], [starts[4], starts[8]]))
		got = batch.cpu().numpy()
		assert not (got == 77).any()
		for slot, start in ((0, starts[4]), (2, starts[8])):
			mine = got[slot * 12 * W:(slot + 1) * 12 * W]
			assert (mine[:12] == orc.expand12(start[None])).all() and (mine[12:] == orc.SOLVED).all()
		assert (got[12 * W:2 * 12 * W] == orc.SOLVED).all()
		assert _status(lib, h, 3)[:, 0].tolist() == [0, 5, 0]
		del batch, got
	finally:
		assert lib.rk_beamb_destroy(h) == 0


def test_kept_graph_and_clean_restart():
	g = gg.GROUPS[3]
	starts, refs = gg.group_starts(g), gg.references(g)
	b = _batch(g)
	b.search(starts[::-1])
	_all_same(b, b.search(starts, keep_arrays=True), refs, starts, "second call")
	assert b.captures == 1
	seen = []
	b.on_poll = lambda st: seen.append(st[:, 0].copy())
	solved = b.search(starts, time_limit=1e-9)
	b.on_poll = None
	assert not solved.any() and not b.status.any() and (b.lengths == -1).all() and len(seen) == 1
	assert (_status(_ffi.lib(), b._h, g.slots)[:, 0] != 0).all()              # no slot is running
	_all_same(b, b.search(starts, keep_arrays=True), refs, starts, "after the time limit")
	assert b.captures == 1
	b.search(starts[:2])
	with pytest.raises(ValueError):
		b.sizes_of(0)


@pytest.mark.parametrize("width", [6, 22])
def test_repr686_net(width):
	cube.set_is2024(False)
	net = NoisyStubNet686(seed=4).to(gpu)
	values = bm.values_of686(NoisyStubNet686(seed=4))
	s20s, s686s = [], []
	for k, scramble in enumerate((4, 9, 1, 6, 3)):
		np.random.seed(590 + k)
		faces, dirs = np.random.randint(0, 6, scramble), np.random.randint(0, 2, scramble)
		s20, s686 = orc.SOLVED.copy(), orc.SOLVED686.copy()
		for f, d in zip(faces, dirs):
			s20, s686 = orc.rotate(s20, f, d), orc.rotate686(s686, f, d)
		s20s.append(s20)
		s686s.append(s686)
	refs = [bm.search(values, a, width, 12, start686=z) for a, z in zip(s20s, s686s)]
	b = DeviceBeamSearchBatch(net, width, searches=3, max_depth=12)
	starts = np.array(s686s, np.int8)
	_all_same(b, b.search(starts, keep_arrays=True), refs, starts, width)
	bad = starts.copy()
	bad[1] = 0                                                                # no one-hot at all: not a cube
	fresh = DeviceBeamSearchBatch(net, width, searches=3, max_depth=12)
	with pytest.raises(ValueError):
		fresh.search(bad)
	assert fresh._h is None and fresh.captures == 0                            # nothing was launched


def _eval_both(agent_of, n_games=5, depths=(4, 6), **kw):
	ev = Evaluator(n_games, list(depths), max_states=50_000, batch_games=4, **kw)
	np.random.seed(640)
	res, states, _ = ev.eval(agent_of())
	assert ev.last_mode == "batched"
	np.random.seed(640)
	res1, states1, _ = ev.eval(agent_of(), batched=False)
	assert ev.last_mode == "sequential"
	assert np.array_equal(res, res1) and np.array_equal(states, states1)
	assert (res >= 0).any()
	return res


def test_evaluator(ball, monkeypatch):
	net = _device_net("noisy")
	_eval_both(lambda: DeviceBeamSearch(net, 22, 12))
	_eval_both(lambda: DeviceBeamSearch(net, 22, 12, ball=ball))
	made = []
	real = Evaluator._batch_agent
	monkeypatch.setattr(Evaluator, "_batch_agent", lambda self, agent, n: made.append(real(self, agent, n)) or made[-1])
	monkeypatch.setattr(DeviceBeamSearchBatch, "MAX_BEAMS", 44)               # two slots of width 22 for groups of four games
	_eval_both(lambda: DeviceBeamSearch(net, 22, 12))
	assert made and all(b.searches == 2 for b in made)
