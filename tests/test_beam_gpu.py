"""
DeviceBeamSearch (engine rk_beam_*) against the plain-Python model of tests/beam_model.py, bit for bit: solved, status, depth,
len(agent), sizes, every back_of(t), the meeting and the action queue.  Widths 1, 5, 6, 22, 342 and 1 366 put 12, 60, 72 (past a
wave), 264 (past a 256-thread tile), 4 104 (past 4 096) and 16 392 children (many tiles, more than one look-back round) into a
depth; tests/test_beam_cpu.py shows on the model alone that the cases hold value ties across the cut, duplicate children, NaN and
+-inf, short beams and every stop.
"""
import numpy as np
import pytest
import torch

from librubiks_amd import cube, gpu
from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import DeviceBeamSearch, DeviceSymBall
from librubiks_amd.solving.evaluation import Evaluator
from oracle import cube_oracle as orc
from tests import beam_model as bm
from tests.repr686_nets import NoisyStubNet686

pytestmark = pytest.mark.gpu


def _device_net(name: str):
	net = bm.net_of(name)
	return net.to(gpu) if isinstance(net, torch.nn.Module) else net


def _agent(case: bm.Case, **kw) -> DeviceBeamSearch:
	fused = True if case.net == "linear_bf16" else False
	return DeviceBeamSearch(_device_net(case.net), case.width, case.max_depth, prune_inverse=case.prune, fused_first_layer=fused, **kw)


def _same(agent: DeviceBeamSearch, solved: bool, ref: bm.Result, what):
	assert solved == ref.solved, what
	assert (agent.status, agent.depth, len(agent)) == (ref.status, ref.depth, ref.explored), what
	assert agent.sizes.tolist() == ref.sizes, what
	for t in range(1, len(ref.sizes)):
		assert np.array_equal(agent.back_of(t), ref.back[t]), (what, t)
	assert agent.meeting == ref.meeting, what
	assert list(agent.action_queue) == ref.queue, what


@pytest.mark.parametrize("case", bm.CASES + bm.SOLVING_CASES, ids=bm.case_id)
def test_against_model(case):
	start = bm.start_of(case.seed, case.scramble)
	ref = bm.reference(case)
	agent = _agent(case)
	_same(agent, agent.search(start, None, None), ref, case)
	if ref.solved:
		assert cube.is_solved(_rotate_all(start, agent.action_queue))
	if case.max_depth == 12:                                  # the budget at exactly the states explored, and one below
		_same(agent, agent.search(start, None, ref.explored), bm.reference(case, ref.explored), (case, "exact budget"))
		assert bm.reference(case, ref.explored)[:3] == ref[:3]
		below = bm.reference(case, ref.explored - 1)
		assert below.status == 2
		_same(agent, agent.search(start, None, ref.explored - 1), below, (case, "one below"))
		assert agent.captures == 1


def _rotate_all(state, queue):
	for a in queue:
		state = cube.rotate(state, *cube.action_space[a])
	return state


def test_repr686_net():
	"""A net of the 6x8x6 representation reads the engine's 20-byte rows through the adapter."""
	cube.set_is2024(False)
	net = NoisyStubNet686(seed=4).to(gpu)
	for width, seed, scramble in ((22, 590, 4), (6, 591, 9)):
		np.random.seed(seed)
		faces, dirs = np.random.randint(0, 6, scramble), np.random.randint(0, 2, scramble)
		s20, s686 = orc.SOLVED.copy(), orc.SOLVED686.copy()
		for f, d in zip(faces, dirs):
			s20, s686 = orc.rotate(s20, f, d), orc.rotate686(s686, f, d)
		ref = bm.search(bm.values_of686(NoisyStubNet686(seed=4)), s20, width, 12, start686=s686)
		agent = DeviceBeamSearch(net, width, 12)
		_same(agent, agent.search(s686, None, None), ref, (width, seed))
		if ref.solved:
			assert cube.is_solved(_rotate_all(s686, agent.action_queue))


@pytest.fixture(scope="module")
def ball():
	return DeviceSymBall(bm.BALL_RADIUS).build()


@pytest.mark.parametrize("case", bm.BALL_CASES, ids=bm.case_id)
def test_to_the_ball_against_model(ball, case):
	net, width, seed, scramble = case
	start = bm.start_of(seed, scramble)
	ref = bm.ball_reference(case)
	agent = DeviceBeamSearch(_device_net(net), width, 12, ball=ball)
	_same(agent, agent.search(start, None, None), ref, case)
	if ref.solved:
		assert cube.is_solved(_rotate_all(start, agent.action_queue))
		assert len(agent.action_queue) == agent.depth + agent.meeting[2]


@pytest.mark.parametrize("depth", [3, 4, 5])
def test_full_beam_to_the_ball_is_optimal(depth):
	"""The anchor of tests/test_beam_cpu.py on the device: a beam that keeps every state ends at the radius-2 ball after
	distance - 2 depths, and its queue is a shortest solution (the distance by a radius-5 ball's own depth)."""
	ball2, ball5 = DeviceSymBall(2).build(), DeviceSymBall(5).build()
	net = _device_net("noisy")
	for seed in range(610, 614):
		start = bm.start_of(seed, depth)
		dist = int(ball5.depth(start[None])[0])
		assert 1 <= dist <= depth
		agent = DeviceBeamSearch(net, 11 * 12 ** max(dist - 3, 0), depth, ball=ball2)
		assert agent.search(start, None, None) and len(agent.action_queue) == dist, (seed, depth)
		assert cube.is_solved(_rotate_all(start, agent.action_queue))
		if dist > 2:
			assert agent.depth == dist - 2 and agent.meeting[2] == 2


def test_kept_graph_and_clean_restart():
	case = bm.Case("lookup", 22, True, 2, 0, 0)
	first, second = bm.start_of(620, 9), bm.start_of(621, 4)
	agent = _agent(case)
	assert not agent.search(first, None, None) and agent.status == 3          # stopped by the depth limit ...
	solved = agent.search(second, None, None)                                 # ... and the next search starts clean
	assert agent.captures == 1
	fresh = _agent(case)
	assert fresh.search(second, None, None) == solved
	ref = bm.search(bm.values_of(bm.net_of("lookup")), second, 22, 2)
	for a in (agent, fresh):
		_same(a, solved, ref, "second search")


def test_reset_writes_every_row():
	"""The rows beyond the beam read back as the solved state after a reset: the net reads all 12 B rows at every depth."""
	from librubiks_amd import _ffi
	agent = _agent(bm.Case("linear_bf16", 22, True, 1, 0, 0))                 # the fused first layer: the batch holds the 20-byte rows
	start = bm.start_of(622, 9)
	agent.search(start, None, None)
	h, batch = agent._h, agent._batch[1]
	batch.fill_(77)                                                           # no cubie code
	_ffi.check(_ffi.lib().rk_beam_reset(h, np.ascontiguousarray(start, np.int8).ctypes.data, 100, _ffi.stream_ptr()))
	rows = batch.cpu().numpy()
	assert rows.shape == (12 * 22, 20)
	assert (rows[:12] == orc.expand12(start[None])).all() and (rows[12:] == orc.SOLVED).all()


def test_bad_arguments(ball):
	net = bm.net_of("noisy")
	for kw in ({"width": 0}, {"width": (1 << 16) + 1}, {"width": 2.5}, {"width": True}, {"max_depth": 0}, {"max_depth": 4097},
	           {"ball": DeviceSymBall(3)}, {"ball": agents.DeviceGoalBall(2)}, {"poll": 0}):
		with pytest.raises(ValueError):
			DeviceBeamSearch(net, **{"width": 4, **kw})
	agent = DeviceBeamSearch(net, 4)
	for bad in (np.zeros((2, 20), np.int8), np.zeros(19, np.int8), np.zeros((6, 8, 6), np.int8)):
		with pytest.raises(ValueError):
			agent.search(bad, None, 100)
	assert agent._h is None                                                   # no engine was made
	assert DeviceBeamSearch(net, 4).search(cube.get_solved(), None, 10) and len(agent.action_queue) == 0


def test_evaluator_runs_it():
	net = _device_net("noisy")
	np.random.seed(630)
	res, states, _ = Evaluator(3, [4], max_states=50_000).eval(DeviceBeamSearch(net, 22, 12))
	np.random.seed(630)
	agent = DeviceBeamSearch(net, 22, 12)
	for g in range(3):
		start = cube.scramble(4, True)[0]
		solved = agent.search(start, None, 50_000)
		assert res[0, g] == (len(agent.action_queue) if solved else -1) and states[0, g] == len(agent)
