"""
The two-phase search on the device (engine rk_twophase_*, `DeviceTwoPhaseSolver`) against the model of tests/twophase_model.py --
the four pruning tables byte for byte, lengths, phase lengths, every action byte, reason and node count bit for bit -- and
independently of the model: every queue solves under the oracle, no answer is longer than the chain's, the first p1 moves end in
the subgroup and the rest are its generators, first solutions are optimal against breadth-first searches.  Then that scheduling
cannot show (one call against one call per row, sizes around a wave, more rows than lanes, reversed order), rows that are no
legal state among good ones, and the Python surface.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceChainSolver, DeviceGoalBall, DeviceSymBall, DeviceTwoPhaseSolver, TowardsGoal
from librubiks_amd.solving.evaluation import Evaluator
from oracle import cube_oracle as orc
from tests import chain_model as CM
from tests import twophase_model as T
from tests.test_chain_gpu import _replay, _superflip

pytestmark = pytest.mark.gpu

SHALLOW, BUDGETED, DEEPER = (1, 4096), (1, 4096), (4, 1 << 16)          # (tries, max_nodes) of the three case sets
# seeds chosen on the CPU with the model so that reasons 0, 1 and 2 all occur over the two scrambled sets (reason 1 needs tries > 1:
# with one try the search ends by itself right after its first improvement)
SEED_BUDGETED, SEED_DEEPER = 29_001, 29_002
NEVER = 1 << 24                                                            # a budget no row of the "unlimited" test reaches (asserted)


@functools.lru_cache(maxsize=None)
def _chain():
	return DeviceChainSolver()


@functools.lru_cache(maxsize=None)
def _solver(tries, max_nodes, allow_illegal=False):
	return DeviceTwoPhaseSolver(chain=_chain(), tries=tries, max_nodes=max_nodes, allow_illegal=allow_illegal)


@functools.lru_cache(maxsize=None)
def _ball4() -> np.ndarray:
	ball = DeviceGoalBall(4).arrays()[0]
	assert len(ball) == 1 + 12 + 114 + 1068 + 10011
	return np.asarray(ball, np.int8)


@functools.lru_cache(maxsize=None)
def _shallow() -> np.ndarray:
	"""every state within 4 turns, solved, the 12 one-move states, the superflip, the subgroup's states of cost <= 6"""
	ones = np.stack([orc.rotate(orc.SOLVED, a // 2, 1 - a % 2) for a in range(12)])
	return np.concatenate([_ball4(), orc.SOLVED[None], ones, _superflip()[None], T.subgroup_states(6)[0]]).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _cases(name) -> np.ndarray:
	if name == "shallow":
		return _shallow()
	if name == "budgeted":
		return T.scrambles(SEED_BUDGETED, 1 + np.arange(32) * 3 % 100)
	return T.scrambles(SEED_DEEPER, 9 + np.arange(8))


PARAMS = {"shallow": SHALLOW, "budgeted": BUDGETED, "deeper": DEEPER}


@functools.lru_cache(maxsize=None)
def _answers(name):
	return _solver(*PARAMS[name]).solve(_cases(name), phase_lengths=True, details=True)


@functools.lru_cache(maxsize=None)
def _model_answers(name):
	return T.solve(_cases(name), *PARAMS[name])


def _same(got, want):
	return all(np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)) for g, w in zip(got, want))


def test_tables_and_status_against_the_model():
	solver = _solver(*SHALLOW)
	header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rubiks_hip.h")).read()
	grid = int(re.search(r"#define\s+RK_TWOPHASE_GRID\s+(\d+)", header).group(1))
	assert solver.table_counts == T.COUNTS and solver.table_sizes == T.SIZES and solver.table_depths == T.deepest()
	assert solver.grid_rows == grid * 256 == DeviceTwoPhaseSolver.GRID_ROWS and solver.max_length == CM.max_length() == 70
	for t in range(4):
		got, want = solver.export(t + 1), T.table(t)
		assert got.dtype == np.uint8 and got.shape == want.shape and (got == want).all(), t
		assert (got == 0).sum() == 1 and (got != 255).sum() == T.COUNTS[t]


@pytest.mark.parametrize("name", ["shallow", "budgeted", "deeper"])
def test_engine_against_the_model_bit_for_bit(name):
	got, want = _answers(name), _model_answers(name)
	lengths, actions, phases, reason, nodes = got
	assert lengths.dtype == np.int32 and actions.dtype == np.int8 and phases.dtype == np.int32 and reason.dtype == np.int32 and nodes.dtype == np.int64
	assert actions.shape == (len(_cases(name)), 70) and phases.shape == (len(_cases(name)), 2)
	for i, what in enumerate(("lengths", "actions", "phase lengths", "reason", "nodes")):
		assert np.array_equal(np.asarray(got[i], np.int64), np.asarray(want[i], np.int64)), what


def test_all_three_reasons_occur():
	reasons = np.concatenate([_answers("budgeted")[3], _answers("deeper")[3]])
	assert set(reasons.tolist()) == {0, 1, 2}
	assert set(_answers("budgeted")[3].tolist()) == {0, 2}                # one try: an improvement ends the search


@pytest.mark.parametrize("name", ["shallow", "budgeted", "deeper"])
def test_answers_without_the_model(name):
	states = _cases(name)
	lengths, actions, phases, reason, nodes = _answers(name)
	tries, max_nodes = PARAMS[name]
	# every queue solves its state
	assert (lengths >= 0).all() and orc.multi_is_solved(_replay(states, lengths, actions)).all()
	assert (np.where(np.arange(70)[None, :] >= lengths[:, None], actions, -1) == -1).all()
	assert (phases.sum(axis=1) == lengths).all() and (phases >= 0).all() and (nodes >= 0).all() and (nodes <= max_nodes).all()
	# never longer than the chain's, the chain's own row exactly where it is as long
	c_len, c_act, c_stages = _chain().solve(states, stage_lengths=True)
	assert (lengths <= c_len).all() and ((reason == 2) == (lengths == c_len)).all()
	kept = reason == 2
	assert (actions[kept] == c_act[kept]).all() and (phases[kept, 0] == c_stages[kept, :2].sum(axis=1)).all()
	assert ((reason != 1) | (nodes == max_nodes)).all()
	# the first p1 moves end in the subgroup, the rest are its generators
	mid = _replay(states, phases[:, 0], actions)
	assert (_chain().solve(mid, stage_lengths=True)[2][:, :2] == 0).all()
	for i in np.nonzero(~kept)[0]:
		rest = actions[i, phases[i, 0]:lengths[i]].tolist()
		while rest:
			a = rest.pop(0)
			assert a in (0, 1, 2, 3) or (a in (4, 6, 8, 10) and rest and rest.pop(0) == a), (i, a)
	if tries == 1:
		first = reason == 0
		assert (phases[first, 0] <= c_stages[first, :2].sum(axis=1)).all()


def test_first_solutions_are_optimal_against_breadth_first_searches():
	states = _shallow()
	lengths, actions, phases, reason, nodes = _answers("shallow")
	n4 = len(_ball4())
	dist = T.coset_distances(4)
	want = np.array([dist[k] for k in T.coset_key(states[:n4])])
	first = reason[:n4] == 0
	assert first.sum() > 100 and (phases[:n4, 0][first] == want[first]).all()
	sub, cost = T.subgroup_states(6)
	assert (states[-len(sub):] == sub).all()
	assert (phases[-len(sub):, 0] == 0).all() and (lengths[-len(sub):] == cost).all()


def test_more_tries_never_lengthen_at_an_unlimited_budget():
	states = np.concatenate([_ball4()[::40], T.subgroup_states(6)[0][::7].astype(np.int8)])
	one = _solver(1, NEVER).solve(states, details=True)
	four = _solver(4, NEVER).solve(states, details=True)
	assert (one[3] < NEVER).all() and (four[3] < NEVER).all()
	assert (four[0] <= one[0]).all() and (one[2] != 1).all() and (four[2] != 1).all()
	assert orc.multi_is_solved(_replay(states, four[0], four[1])).all()


def test_one_call_equals_one_call_per_row():
	states = np.concatenate([_cases("deeper"), _ball4()[[0, 5, 200, 2000, 11000, 11205]], _superflip()[None], orc.SOLVED[None]]).astype(np.int8)
	assert len(states) == 16
	solver = _solver(*DEEPER)
	together = solver.solve(states, phase_lengths=True, details=True)
	for i in range(16):
		assert _same(solver.solve(states[i:i + 1], phase_lengths=True, details=True), [x[i:i + 1] for x in together]), i


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sizes_around_a_wave(n):
	rows = _shallow()[5000:5000 + n]
	got = _solver(*SHALLOW).solve(rows, phase_lengths=True, details=True)
	assert [x.shape for x in got] == [(n,), (n, 70), (n, 2), (n,), (n,)]
	assert _same(got, [x[5000:5000 + n] for x in _answers("shallow")])


def test_more_rows_than_lanes_and_reversed_order():
	base, answers = _shallow(), [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in _answers("shallow")]
	solver = _solver(*SHALLOW)
	n = solver.grid_rows + 1
	at = torch.arange(n, device="cuda") % len(base)
	rows = torch.from_numpy(base).cuda()[at].contiguous()
	got = solver.solve(rows, phase_lengths=True, details=True)
	for g, w in zip(got, answers):
		assert torch.equal(g, w[at])
	back = solver.solve(torch.from_numpy(base[::-1].copy()).cuda(), phase_lengths=True, details=True)
	for g, w in zip(back, answers):
		assert torch.equal(g, w.flip(0))


def test_no_rows_touch_nothing():
	from tests import side_stream as S
	solver = _solver(*SHALLOW)
	outs = [S.sentinel((4,), torch.int32), S.sentinel((4, 70), torch.int8), S.sentinel((4, 2), torch.int32), S.sentinel((4,), torch.int32),
	        S.sentinel((4,), torch.int64), S.sentinel((1,), torch.int32)]
	q = torch.from_numpy(_shallow()[:4]).cuda()
	_ffi.check(_ffi.lib().rk_twophase_solve(solver._h, _chain()._h, q.data_ptr(), 0, 1, 10, *[t.data_ptr() for t in outs], _ffi.stream_ptr()))
	torch.cuda.synchronize()
	for t in outs:
		assert (S.bits(t) == S.SENTINEL).all()


@pytest.mark.parametrize("name", ["code out of range", "a flipped edge", "two swapped edges"])
def test_ill_formed_rows_among_good_ones(name):
	good_row = _cases("budgeted")[20].copy()
	bad = good_row.copy()
	if name == "code out of range":
		bad[3] = 24
	elif name == "a flipped edge":
		bad[8] ^= 1
	else:
		bad[[8, 9]] = bad[[9, 8]]
	assert not cube.is_legal(bad[None])[0]
	n, at = 600, (311, 570)
	rows = _shallow()[:n].copy()
	rows[list(at)] = bad
	with pytest.raises(ValueError, match=f"row {at[0]} "):
		_solver(*SHALLOW).solve(rows)
	got = _solver(*SHALLOW, allow_illegal=True).solve(rows, phase_lengths=True, details=True)
	good = np.ones(n, bool)
	good[list(at)] = False
	assert (got[0][~good] == -1).all() and (got[1][~good] == -1).all() and (got[2][~good] == -1).all()
	assert (got[3][~good] == 2).all() and (got[4][~good] == 0).all()
	assert _same([x[good] for x in got], [x[:n][good] for x in _answers("shallow")])


def test_python_surface():
	solver, rows = _solver(*SHALLOW), _shallow()[4000:4300]
	want = [x[4000:4300] for x in _answers("shallow")]
	got = solver.solve(torch.from_numpy(rows).cuda(), phase_lengths=True, details=True)
	assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got) and _same([t.cpu().numpy() for t in got], want)
	assert len(solver.solve(rows)) == 2 and len(solver.solve(rows, phase_lengths=True)) == 3 and len(solver.solve(rows, details=True)) == 4
	was = cube.get_is2024()
	try:
		cube.set_is2024(False)
		l686, a686 = solver.solve(cube.as686(rows))
		assert solver.search(cube.as686(rows[5:6])[0]) and list(solver.action_queue) == want[1][5, :want[0][5]].tolist()
	finally:
		cube.set_is2024(was)
	assert (l686 == want[0]).all() and (a686 == want[1]).all()
	for i in (0, 99, 250):
		assert solver.search(rows[i]) is True and len(solver) == 1
		assert list(solver.action_queue) == want[1][i, :want[0][i]].tolist()
	bad = rows[0].copy()
	bad[8] ^= 1
	with pytest.raises(ValueError):
		solver.search(bad)
	assert "Two-phase solver" in str(solver) and "tries=1" in str(solver)
	own = DeviceTwoPhaseSolver(tries=1, max_nodes=64)
	assert isinstance(own.chain, DeviceChainSolver) and own.chain is not _chain() and (own.tries, own.max_nodes) == (1, 64)
	for kwargs in ({"tries": 0}, {"tries": 1.5}, {"max_nodes": 0}, {"max_nodes": True}, {"chain": 3}, {"shorten": 3}):
		with pytest.raises(ValueError):
			DeviceTwoPhaseSolver(**kwargs)
	with pytest.raises(ValueError):
		solver.export(5)


def test_shorten_keeps_solving_and_never_lengthens():
	rows = _cases("budgeted")
	b_len = _answers("budgeted")[0]
	lengths, actions = DeviceTwoPhaseSolver(chain=_chain(), tries=1, max_nodes=4096, shorten=DeviceSymBall(6)).solve(rows)
	assert (lengths <= b_len).all() and (lengths < b_len).any() and (lengths >= 0).all()
	assert orc.multi_is_solved(_replay(rows, lengths, actions)).all()
	assert (np.where(np.arange(actions.shape[1])[None, :] >= lengths[:, None], actions, -1) == -1).all()


def test_evaluator_and_towards_goal():
	np.random.seed(29)
	solver = _solver(*SHALLOW)
	res, _, _ = Evaluator(n_games=20, scrambling_depths=[30], max_states=10).eval(solver)
	res = np.asarray(res)
	assert res.shape[-1] == 20 and (res >= 0).all()
	starts, goal = _cases("budgeted")[:6], _cases("budgeted")[9]
	agent = TowardsGoal(solver, goal)
	for i in range(6):
		assert agent.search(starts[i])
		s = starts[i].copy()
		for a in agent.action_queue:
			s = orc.rotate(s, a // 2, 1 - a % 2)
		assert (s == goal).all()
