"""
A frontier pool that grew is kept by its agent and reset for the next search: that second search must be a fresh agent's, bit for
bit.  The four growing engines through their agents, from a pool of 2 states and with few pops, so that a level spans many
iterations, the pool doubles many times and the budget of the first search cuts inside a batch.
"""
import ctypes as C

import numpy as np
import pytest

from librubiks_amd import _ffi, cube
from librubiks_amd.solving import _engine as eng
from librubiks_amd.solving.agents import DeviceBFS, DeviceBallSearch, DeviceBiBFS, DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch

pytestmark = pytest.mark.gpu

ENGINES = {
	"bfs": lambda **kw: DeviceBFS(**kw),
	"bibfs": lambda **kw: DeviceBiBFS(**kw),
	"bsearch": lambda **kw: DeviceBallSearch(_ball(DeviceGoalBall), **kw),
	"ssearch": lambda **kw: DeviceSymBallSearch(_ball(DeviceSymBall), **kw),
}
_BALLS = {}


def _ball(kind):
	"""One ball of radius 1 per kind for the whole module: the search from distance 4 then grows three levels of its own."""
	if kind not in _BALLS:
		_BALLS[kind] = kind(1, pops=64)
	return _BALLS[kind]


def _start() -> np.ndarray:
	"""Four quarter turns of four different faces, no two of them opposite in a row: distance 4."""
	s = cube.get_solved()
	for a in (0, 2, 4, 6):
		s = cube.rotate(s, *cube.action_space[a])
	return s


def _same(agent, fresh):
	assert len(agent) == len(fresh) and list(agent.action_queue) == list(fresh.action_queue)
	a, b = agent.arrays(), fresh.arrays()
	assert len(a) == len(b)
	for x, y in zip(a, b):
		assert x.shape == y.shape and (x == y).all()


@pytest.mark.parametrize("pops", [1, 5])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_reset_after_growth(engine, pops):
	cube.set_is2024(True)
	start = _start()
	fresh = ENGINES[engine](pops=pops, capacity=50_000)
	assert fresh.search(start, max_states=10 ** 9) and len(fresh.action_queue) == 4 and fresh.grown == 0
	budget = len(fresh) // 2 + 1                             # stops the first search half way, between two pops of a batch
	agent = ENGINES[engine](pops=pops, capacity=2)
	assert not agent.search(start, max_states=budget)
	assert budget <= len(agent) < budget + 12 and agent.grown > 0 and not agent.capacity_exhausted
	h, cap = agent._h, agent._h_cap
	if engine == "bfs":                                      # the resume path on the grown pool: the table is rebuilt, then it goes on
		lib, stream = _ffi.lib(), _ffi.stream_ptr()
		_ffi.check(lib.rk_bfs_set_budget(h, 10 ** 9, stream))
		st = (C.c_longlong * 8)()
		_ffi.check(lib.rk_bfs_status(h, st, stream))
		while not st[0]:
			if (agent._h_cap - int(st[2])) // (12 * pops) == 0:
				assert agent._grow(h)
			_ffi.check(lib.rk_bfs_run(h, 1, stream))
			_ffi.check(lib.rk_bfs_status(h, st, stream))
		assert st[1] == 1 and st[6] == 0
		agent._n, agent._cache = int(st[2]), None
		agent.action_queue = eng.read_path(lib.rk_bfs_path, h)
		_same(agent, fresh)
		cap = agent._h_cap
	assert agent.search(start, max_states=10 ** 9)         # the same agent again: the engine that grew, reset
	assert agent._h is h and agent._h_cap >= cap
	_same(agent, fresh)
	assert agent.iterations == fresh.iterations and agent.popped == fresh.popped
