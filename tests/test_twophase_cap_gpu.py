"""
The cap on the two-phase search's phase-2 bound on the device (rk_twophase_solve_capped, `DeviceTwoPhaseSolver(phase2_cap=C)`)
against the model of tests/twophase_cap_model.py -- lengths, every action byte, phase lengths, reason, nodes and the two counts bit
for bit, on shallow inputs whose seeds were chosen on the CPU so that both changed conditions decide something --, at the boundary
C = c and C = c - 1 on states of the subgroup of exact cost c, without a cap and with one that cannot bind against the uncapped
engine, and independently of the model.  Then what scheduling cannot show (sizes around a wave, more rows than lanes, reversed
order, one call against one call per row), rows that are no legal state, the refusal of the C entry and the Python surface.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceTwoPhaseSolver
from librubiks_amd.solving.evaluation import Evaluator
from oracle import cube_oracle as orc
from tests import twophase_cap_model as M
from tests import twophase_model as T
from tests.test_chain_gpu import _replay
from tests.test_twophase_gpu import PARAMS, _answers, _cases, _chain, _same

pytestmark = pytest.mark.gpu

MOST_TRIES = (1 << 31) - 1
# (states, max_nodes, caps); the seeds were chosen on the CPU with the model so that the four conditions of
# test_the_seeds_make_both_conditions_decide hold over the two sets together
SEED_SHALLOW, SEED_DEEPER = 32_001, 32_002
SETS = {"shallow": (4096, (1, 4, 8)), "deeper": (1 << 14, (10,))}
KEYS = [(name, cap) for name, (_, caps) in SETS.items() for cap in caps]


@functools.lru_cache(maxsize=None)
def _rows(name) -> np.ndarray:
	if name == "shallow":
		return T.scrambles(SEED_SHALLOW, 1 + np.arange(32) % 16)           # 32 scrambles of 1..16 moves
	return T.scrambles(SEED_DEEPER, 9 + np.arange(8))                      # 8 scrambles of 9..16 moves


@functools.lru_cache(maxsize=None)
def _solver(max_nodes, cap, tries=None, allow_illegal=False):
	return DeviceTwoPhaseSolver(chain=_chain(), tries=tries, max_nodes=max_nodes, phase2_cap=cap, allow_illegal=allow_illegal)


def _all(solver, states):
	return solver.solve(states, phase_lengths=True, details=True, counts=True)


@functools.lru_cache(maxsize=None)
def _got(name, cap):
	return _all(_solver(SETS[name][0], cap), _rows(name))


@functools.lru_cache(maxsize=None)
def _model(name, cap):
	"""-> (the model's six outputs, its trace); cap None: the search without a cap at the same tries and max_nodes"""
	trace = {}
	return M.solve(_rows(name), MOST_TRIES, SETS[name][0], cap, trace=trace), trace


def test_the_seeds_make_both_conditions_decide():
	"""on the model's output: reasons 0, 1 and 2 all occur; a row is rejected by h2 > C at its first phase-1 solution; a row leaves
	phase 2 by D2 > C and later improves from another phase-1 word; a row is strictly shorter with the cap than without it"""
	reasons, rejected, came_back, shorter = set(), 0, 0, 0
	for name, cap in KEYS:
		out, trace = _model(name, cap)
		reasons |= set(out[3].tolist())
		rejected += int(trace["first_rejected"].sum())
		came_back += int(((trace["gave_up"] > 0) & trace["improved_after"]).sum())
		shorter += int((out[0] < _model(name, None)[0][0]).sum())
	assert reasons == {0, 1, 2}
	assert rejected > 0
	assert came_back > 0
	assert shorter > 0


@pytest.mark.parametrize("name,cap", KEYS)
def test_engine_against_the_model_bit_for_bit(name, cap):
	got, want = _got(name, cap), _model(name, cap)[0]
	n = len(_rows(name))
	assert [x.dtype for x in got] == [np.int32, np.int8, np.int32, np.int32, np.int64, np.int32]
	assert [x.shape for x in got] == [(n,), (n, 70), (n, 2), (n,), (n,), (n, 2)]
	for i, what in enumerate(("lengths", "actions", "phase lengths", "reason", "nodes", "counts")):
		assert np.array_equal(np.asarray(got[i], np.int64), np.asarray(want[i], np.int64)), what


@pytest.mark.parametrize("name,cap", KEYS)
def test_answers_without_the_model(name, cap):
	states, max_nodes = _rows(name), SETS[name][0]
	lengths, actions, phases, reason, nodes, counts = _got(name, cap)
	assert (lengths >= 0).all() and orc.multi_is_solved(_replay(states, lengths, actions)).all()
	assert (np.where(np.arange(70)[None, :] >= lengths[:, None], actions, -1) == -1).all()
	c_len, c_act = _chain().solve(states)
	assert (lengths <= c_len).all() and ((reason == 2) == (lengths == c_len)).all() and (actions[reason == 2] == c_act[reason == 2]).all()
	assert (phases.sum(axis=1) == lengths).all() and (phases >= 0).all()
	assert (phases[reason != 2, 1] <= cap).all()
	assert (nodes >= 0).all() and (nodes <= max_nodes).all() and ((reason != 1) | (nodes == max_nodes)).all()
	assert (counts[:, 1] <= counts[:, 0]).all() and (counts >= 0).all()


@functools.lru_cache(maxsize=None)
def _subgroup(c):
	states, cost = T.subgroup_states(6)
	return states[cost == c].astype(np.int8)


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 6])
def test_a_cap_at_the_exact_cost(c):
	"""states of the subgroup (the empty phase-1 word) of exact phase-2 cost c, C = c: the answer has length c"""
	states = _subgroup(c)
	got = _all(_solver(4096, c), states)
	assert len(states) and (got[0] == c).all() and (got[2][:, 0] == 0).all()
	assert orc.multi_is_solved(_replay(states, got[0], got[1])).all()
	assert _same(got, M.solve(states, MOST_TRIES, 4096, c))


@pytest.mark.parametrize("c", [2, 3, 4, 5, 6])
def test_a_cap_one_below_the_exact_cost(c):
	states = _subgroup(c)
	got = _all(_solver(4096, c - 1), states)
	assert ((got[2][:, 1] <= c - 1) | (got[3] == 2)).all()
	assert orc.multi_is_solved(_replay(states, got[0], got[1])).all()
	assert _same(got, M.solve(states, MOST_TRIES, 4096, c - 1))


@pytest.mark.parametrize("name", ["shallow", "budgeted", "deeper"])
def test_no_cap_and_a_cap_that_cannot_bind(name):
	"""the three case sets of tests/test_twophase_gpu.py: the uncapped solve's five outputs bit for bit"""
	tries, max_nodes = PARAMS[name]
	want = _answers(name)
	for cap in (None, _chain().max_length):
		solver = _solver(max_nodes, cap, tries)
		assert _same(solver.solve(_cases(name), phase_lengths=True, details=True), want), cap
		with_counts = _all(solver, _cases(name))
		assert _same(with_counts[:5], want), cap
		assert (with_counts[5][:, 1] <= with_counts[5][:, 0]).all() and (with_counts[5][:, 0] <= tries).all() and (with_counts[5] >= 0).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sizes_around_a_wave(n):
	at = np.arange(n) % 32
	got = _all(_solver(4096, 8), _rows("shallow")[at])
	assert [x.shape for x in got] == [(n,), (n, 70), (n, 2), (n,), (n,), (n, 2)]
	assert _same(got, [x[at] for x in _got("shallow", 8)])


def test_more_rows_than_lanes_and_reversed_order():
	base, answers = _rows("shallow"), [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in _got("shallow", 8)]
	solver = _solver(4096, 8)
	n = solver.grid_rows + 1
	at = torch.arange(n, device="cuda") % len(base)
	for order in (at, at.flip(0)):
		got = _all(solver, torch.from_numpy(base).cuda()[order].contiguous())
		for g, w in zip(got, answers):
			assert torch.equal(g, w[order])


def test_one_call_equals_one_call_per_row():
	states, together = _rows("deeper"), _got("deeper", 10)
	for i in range(len(states)):
		assert _same(_all(_solver(1 << 14, 10), states[i:i + 1]), [x[i:i + 1] for x in together]), i


@pytest.mark.parametrize("name", ["code out of range", "a flipped edge", "two swapped edges"])
def test_ill_formed_rows_among_good_ones(name):
	bad = _rows("shallow")[20].copy()
	if name == "code out of range":
		bad[3] = 24
	elif name == "a flipped edge":
		bad[8] ^= 1
	else:
		bad[[8, 9]] = bad[[9, 8]]
	assert not cube.is_legal(bad[None])[0]
	n, at = 200, (3, 131)
	pick = np.arange(n) % 32
	rows = _rows("shallow")[pick].copy()
	rows[list(at)] = bad
	with pytest.raises(ValueError, match=f"row {at[0]} "):
		_solver(4096, 8).solve(rows)
	got = _all(_solver(4096, 8, None, True), rows)
	good = np.ones(n, bool)
	good[list(at)] = False
	assert (got[0][~good] == -1).all() and (got[1][~good] == -1).all() and (got[2][~good] == -1).all()
	assert (got[3][~good] == 2).all() and (got[4][~good] == 0).all() and (got[5][~good] == 0).all()
	assert _same([x[good] for x in got], [x[pick][good] for x in _got("shallow", 8)])


def test_the_entry_refuses_a_cap_above_the_longest_row():
	solver, lib = _solver(4096, 8), _ffi.lib()
	status = (C.c_longlong * 16)()
	_ffi.check(lib.rk_twophase_status(solver._h, status))
	q = torch.from_numpy(_rows("shallow")[:4]).cuda()
	outs = [torch.zeros(4, dtype=torch.int32, device="cuda"), torch.full((4, 70), -1, dtype=torch.int8, device="cuda"),
	        torch.zeros((4, 2), dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"),
	        torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros((4, 2), dtype=torch.int32, device="cuda")]
	ptrs = [t.data_ptr() for t in outs]

	def call(cap, counts=ptrs[5]):
		return lib.rk_twophase_solve_capped(solver._h, _chain()._h, q.data_ptr(), 4, 1, 64, cap, *ptrs[:5], counts, None, _ffi.stream_ptr())
	assert call(int(status[14]) + 1) == -1 and b"phase2_cap" in lib.rk_last_error()
	torch.cuda.synchronize()
	assert all(int(t.abs().sum()) == (4 * 70 if t.dtype == torch.int8 else 0) for t in outs)       # refused before any launch
	assert call(8, ptrs[5] + 2) == -1 and b"aligned" in lib.rk_last_error()
	assert call(int(status[14])) == 0 and call(0) == 0 and call(-3) == 0 and call(8, None) == 0
	torch.cuda.synchronize()


def test_python_surface():
	for bad in (0, -1, 71, True, 1.5):
		with pytest.raises(ValueError):
			DeviceTwoPhaseSolver(chain=_chain(), phase2_cap=bad)
	capped, plain = _solver(4096, 8), DeviceTwoPhaseSolver(chain=_chain(), tries=3, max_nodes=4096)
	assert capped.tries == MOST_TRIES and capped.phase2_cap == 8 and plain.phase2_cap is None
	assert "phase2_cap=8" in str(capped) and "cap" not in str(plain) and "tries=3" in str(plain)
	rows, want = _rows("shallow"), _got("shallow", 8)
	assert len(capped.solve(rows)) == 2 and len(capped.solve(rows, counts=True)) == 3 and len(capped.solve(rows, details=True)) == 4
	assert len(capped.solve(rows, phase_lengths=True, counts=True)) == 4
	dev = _all(capped, torch.from_numpy(rows).cuda())
	assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev) and _same([t.cpu().numpy() for t in dev], want)
	assert capped.search(rows[17]) and list(capped.action_queue) == want[1][17, :want[0][17]].tolist()


def test_the_capped_solver_plays_in_the_evaluator():
	np.random.seed(32)
	res, _, _ = Evaluator(n_games=20, scrambling_depths=[30], max_states=10).eval(_solver(4096, 8))
	res = np.asarray(res)
	assert res.shape[-1] == 20 and (res >= 0).all()
