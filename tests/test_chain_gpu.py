"""
The subgroup chain on the device (engine rk_chain_*, `DeviceChainSolver`) against the model of tests/chain_model.py -- the four
tables byte for byte, lengths, stage lengths and every action bit for bit -- and against the oracle alone: every returned queue,
replayed by the oracle, solves its state.  Then the grid-stride loop, n = 0, rows that are no legal state among good ones, and the
Python surface (tensors and arrays, 6x8x6 input, the agent protocol, shorten=, Evaluator).
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceChainSolver, DeviceGoalBall, DeviceSymBall
from librubiks_amd.solving.evaluation import Evaluator
from oracle import cube_oracle as orc
from tests import chain_model as M
from tests import side_stream as S

pytestmark = pytest.mark.gpu

COUNTS = (2048, 1082565, 29400, 663552)
SUPERFLIP = "U R2 F B R B2 R U2 L B2 R U' D' R2 F R' L B2 U2 F2"


@functools.lru_cache(maxsize=None)
def _solver():
	return DeviceChainSolver()


@functools.lru_cache(maxsize=None)
def _lenient():
	return DeviceChainSolver(allow_illegal=True)


def _superflip() -> np.ndarray:
	s = orc.SOLVED.copy()
	for m in SUPERFLIP.split():
		face, direction = "FBUDLR".index(m[0]), 1 if m.endswith("'") else 0
		for _ in range(2 if m.endswith("2") else 1):
			s = orc.rotate(s, face, direction)
	assert (s[:8] == orc.SOLVED[:8]).all() and (s[8:] == orc.SOLVED[8:] + 1).all()
	return s


@functools.lru_cache(maxsize=None)
def _cases() -> np.ndarray:
	"""4 096 seeded scrambles 1..100 moves deep in turn, solved, the 12 one-move states, the superflip, every state within 4 turns"""
	rs = np.random.RandomState(27_001)
	n = 4096
	s, want = orc.repeat_state(orc.SOLVED, n), 1 + np.arange(n) % 100
	for d in range(100):
		moved = orc.multi_rotate(s, rs.randint(0, 6, n), rs.randint(0, 2, n))
		s = np.where((want > d)[:, None], moved, s)
	ones = np.stack([orc.rotate(orc.SOLVED, a // 2, 1 - a % 2) for a in range(12)])
	ball = DeviceGoalBall(4).arrays()[0]
	assert len(ball) == 1 + 12 + 114 + 1068 + 10011
	return np.concatenate([s, orc.SOLVED[None], ones, _superflip()[None], ball]).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _answers():
	lengths, actions, stages = _solver().solve(_cases(), stage_lengths=True)
	return lengths, actions, stages


@functools.lru_cache(maxsize=None)
def _model_answers():
	return M.solve(_cases())


def _replay(states, lengths, actions) -> np.ndarray:
	s = np.array(states, np.int8)
	for t in range(actions.shape[1]):
		live = np.nonzero(lengths > t)[0]
		if len(live):
			a = actions[live, t].astype(np.int64)
			assert ((a >= 0) & (a < 12)).all()
			s[live] = orc.multi_rotate(s[live], a // 2, 1 - a % 2)
	return s


def test_tables_and_status_against_the_model():
	solver = _solver()
	assert solver.coset_counts == COUNTS and solver.table_sizes == M.SIZES
	assert solver.stage_depths == M.max_depths() and solver.max_length == M.max_length() == sum(solver.stage_depths)
	for stage in range(4):
		got, want = solver.export(stage + 1), M.table(stage)
		assert got.dtype == np.uint8 and got.shape == want.shape and (got == want).all(), stage
		assert (got == 0).sum() == 1 and (got != 255).sum() == COUNTS[stage]


def test_engine_against_the_model_bit_for_bit():
	(lengths, actions, stages), (m_len, m_act, m_stages) = _answers(), _model_answers()
	assert lengths.dtype == np.int32 and actions.dtype == np.int8 and stages.dtype == np.int32
	assert actions.shape == (len(_cases()), _solver().max_length) and stages.shape == (len(_cases()), 4)
	assert (lengths == m_len).all() and (stages == m_stages).all() and (actions == m_act).all()
	# a state one turn X from solved: the opposite turn, or -- where X is a lower generator of a stage whose goal XX meets -- X, then XX
	assert lengths[4096] == 0 and np.isin(lengths[4097:4109], (1, 3)).all()


def test_every_queue_solves_its_state_by_the_oracle():
	lengths, actions, stages = _answers()
	assert (lengths >= 0).all() and (lengths <= _solver().max_length).all() and (stages.sum(axis=1) == lengths).all()
	assert orc.multi_is_solved(_replay(_cases(), lengths, actions)).all()
	assert (np.where(np.arange(actions.shape[1])[None, :] >= lengths[:, None], actions, -1) == -1).all()
	assert lengths[:4096].max() > 30                                      # (random states are not near: the chain did work)


def test_grid_stride_and_one_row():
	header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rubiks_hip.h")).read()
	grid_rows = int(re.search(r"#define\s+RK_CHAIN_GRID\s+(\d+)", header).group(1)) * 256
	assert grid_rows == DeviceChainSolver.GRID_ROWS
	base, (b_len, b_act, b_stages) = _cases()[:4096], [x[:4096] for x in _answers()]
	n = grid_rows + 1
	rows = torch.from_numpy(base).cuda().repeat((n + 4095) // 4096, 1)[:n].contiguous()
	lengths, actions, stages = _solver().solve(rows, stage_lengths=True)
	at = torch.arange(n, device="cuda") % 4096
	assert torch.equal(lengths, torch.from_numpy(b_len).cuda()[at])
	assert torch.equal(stages, torch.from_numpy(b_stages).cuda()[at])
	assert torch.equal(actions, torch.from_numpy(b_act).cuda()[at])
	one = _solver().solve(base[77:78], stage_lengths=True)
	assert (one[0] == b_len[77:78]).all() and (one[1] == b_act[77:78]).all() and (one[2] == b_stages[77:78]).all()


def test_no_rows_touch_nothing():
	solver = _solver()
	lengths, actions, stages, err = S.sentinel((4,), torch.int32), S.sentinel((4, solver.max_length), torch.int8), S.sentinel((4, 4), torch.int32), \
		S.sentinel((1,), torch.int32)
	q = torch.from_numpy(_cases()[:4]).cuda()
	_ffi.check(_ffi.lib().rk_chain_solve(solver._h, q.data_ptr(), 0, lengths.data_ptr(), actions.data_ptr(), stages.data_ptr(), err.data_ptr(),
	                                     _ffi.stream_ptr()))
	_ffi.check(_ffi.lib().rk_chain_solve(solver._h, None, 0, None, None, None, None, _ffi.stream_ptr()))
	torch.cuda.synchronize()
	for t in (lengths, actions, stages, err):
		assert (S.bits(t) == S.SENTINEL).all()
	empty = solver.solve(np.zeros((0, 20), np.int8), stage_lengths=True)
	assert [x.shape for x in empty] == [(0,), (0, solver.max_length), (0, 4)]


def _ill_formed():
	"""name -> a row that is no legal state, made from a scramble"""
	good = _cases()[40].copy()
	out = {}
	r = good.copy(); r[3] = 24; out["code out of range"] = r
	r = good.copy(); r[1] = r[0]; out["two corners on one position"] = r
	r = good.copy(); r[8] ^= 1; out["a flipped edge"] = r
	r = good.copy(); r[0] = r[0] // 3 * 3 + (r[0] % 3 + 1) % 3; out["a twisted corner"] = r
	r = good.copy(); r[[8, 9]] = r[[9, 8]]; out["two swapped edges"] = r
	return out


@pytest.mark.parametrize("name", ["code out of range", "two corners on one position", "a flipped edge", "a twisted corner", "two swapped edges"])
def test_ill_formed_rows_among_good_ones(name):
	solver, bad = _solver(), _ill_formed()[name]
	assert not cube.is_legal(bad[None])[0]
	n, at = 600, (311, 570)                                              # in two workgroups
	rows = _cases()[:n].copy()
	rows[list(at)] = bad
	q = torch.from_numpy(rows).cuda()
	lengths, stages, err = S.sentinel((n,), torch.int32), S.sentinel((n, 4), torch.int32), S.sentinel((1,), torch.int32)
	actions = S.sentinel((n, solver.max_length), torch.int8)
	_ffi.check(_ffi.lib().rk_chain_solve(solver._h, q.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(), stages.data_ptr(), err.data_ptr(),
	                                     _ffi.stream_ptr()))
	lengths, stages, actions = lengths.cpu().numpy(), stages.cpu().numpy(), actions.cpu().numpy()
	assert int(err.item()) == at[0]
	good = np.ones(n, bool)
	good[list(at)] = False
	assert (lengths[~good] == -1).all() and (stages[~good] == -1).all() and (actions[~good].view(np.uint8) == S.SENTINEL).all()
	b_len, b_act, b_stages = [x[:n] for x in _answers()]
	assert (lengths[good] == b_len[good]).all() and (stages[good] == b_stages[good]).all()
	written = np.arange(solver.max_length)[None, :] < b_len[:, None]
	assert (actions[good][written[good]] == b_act[good][written[good]]).all()
	assert (actions[good].view(np.uint8)[~written[good]] == S.SENTINEL).all()       # the bytes beyond a queue are not written
	# no error word, no stage lengths: the same lengths
	again = S.sentinel((n,), torch.int32)
	_ffi.check(_ffi.lib().rk_chain_solve(solver._h, q.data_ptr(), n, again.data_ptr(), S.sentinel((n, solver.max_length), torch.int8).data_ptr(),
	                                     None, None, _ffi.stream_ptr()))
	assert (again.cpu().numpy() == lengths).all()
	# the Python surface
	with pytest.raises(ValueError, match=f"row {at[0]} "):
		solver.solve(rows)
	l2, a2, s2 = _lenient().solve(rows, stage_lengths=True)
	assert (l2 == lengths).all() and (s2 == stages).all() and (a2[~good] == -1).all() and (a2[good] == b_act[good]).all()


def test_python_surface_tensors_arrays_and_686():
	solver, rows = _solver(), _cases()[:500]
	b_len, b_act, b_stages = [x[:500] for x in _answers()]
	got = solver.solve(torch.from_numpy(rows).cuda(), stage_lengths=True)
	assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
	assert (got[0].cpu().numpy() == b_len).all() and (got[1].cpu().numpy() == b_act).all() and (got[2].cpu().numpy() == b_stages).all()
	assert len(solver.solve(rows)) == 2
	was = cube.get_is2024()
	try:
		cube.set_is2024(False)
		l686, a686 = solver.solve(cube.as686(rows))
		assert solver.search(cube.as686(rows[5:6])[0]) and list(solver.action_queue) == b_act[5, :b_len[5]].tolist()
	finally:
		cube.set_is2024(was)
	assert (l686 == b_len).all() and (a686 == b_act).all()


def test_search_fills_the_action_queue():
	solver = _solver()
	lengths, actions, _ = _answers()
	for i in (0, 99, 4096, 4100, 4109):
		assert solver.search(_cases()[i]) is True and len(solver) == 1
		assert list(solver.action_queue) == actions[i, :lengths[i]].tolist()
	with pytest.raises(ValueError):
		solver.search(_ill_formed()["a flipped edge"])


def test_shorten_keeps_solving_and_never_lengthens():
	ball = DeviceSymBall(6)
	rows = _cases()[:300]
	b_len = _answers()[0][:300]
	lengths, actions = DeviceChainSolver(shorten=ball).solve(rows)
	assert (lengths <= b_len).all() and (lengths < b_len).any() and (lengths >= 0).all()
	assert orc.multi_is_solved(_replay(rows, lengths, actions)).all()
	assert (np.where(np.arange(actions.shape[1])[None, :] >= lengths[:, None], actions, -1) == -1).all()


def test_evaluator_solves_every_game():
	np.random.seed(27)
	ev = Evaluator(n_games=20, scrambling_depths=[30], max_states=10)
	res, _, _ = ev.eval(_solver())
	res = np.asarray(res)
	assert res.shape[-1] == 20 and (res >= 0).all()                      # -1 marks a game that was not solved
