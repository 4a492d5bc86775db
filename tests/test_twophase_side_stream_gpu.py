"""
rk_twophase_create and rk_twophase_solve on a torch side stream behind a gate (tests/side_stream.py, pattern A): the tables are
uploaded on the side stream, the inputs arrive BEHIND the gate over other legal states, the outputs start as sentinel bytes, and
everything is compared bit for bit with a solver made and run on the default stream (which tests/test_twophase_gpu.py pins against
the model).
"""
import functools

import torch

import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceTwoPhaseSolver
from tests import side_stream as S

pytestmark = pytest.mark.gpu

N = 300
TRIES, MAX_NODES = 2, 2048


@functools.lru_cache(maxsize=None)
def _reference():
	solver = DeviceTwoPhaseSolver(tries=TRIES, max_nodes=MAX_NODES)
	torch.cuda.synchronize()
	return solver


@functools.lru_cache(maxsize=None)
def _side():
	"""-> a solver (and its chain) made on a side stream behind a gate (create synchronises, so the gate is checked before it), and
	that stream"""
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		ev = S.gate(s)
		S.held(ev)
		solver = DeviceTwoPhaseSolver(tries=TRIES, max_nodes=MAX_NODES)
		s.synchronize()
	return solver, s


@functools.lru_cache(maxsize=None)
def _states(seed=0) -> torch.Tensor:
	return torch.from_numpy(S.mixed_depths(N, 60, 2_900 + seed)).cuda()


def _out(solver):
	return [S.sentinel((N,), torch.int32), S.sentinel((N, solver.max_length), torch.int8), S.sentinel((N, 2), torch.int32),
	        S.sentinel((N,), torch.int32), S.sentinel((N,), torch.int64), S.sentinel((1,), torch.int32)]


def _solve(solver, q, out):
	_ffi.check(_ffi.lib().rk_twophase_solve(solver._h, solver.chain._h, q.data_ptr(), N, TRIES, MAX_NODES, *[t.data_ptr() for t in out],
	                                        _ffi.stream_ptr()))


def test_create_on_a_side_stream():
	ref, (solver, _) = _reference(), _side()
	assert solver.table_counts == ref.table_counts and solver.table_depths == ref.table_depths
	for table in range(1, 5):
		assert (solver.export(table) == ref.export(table)).all()


def test_solve_on_a_side_stream():
	ref, (solver, s) = _reference(), _side()
	true, buf = _states(), _states(1).clone()
	want, got = _out(ref), _out(solver)
	_solve(ref, true, want)
	torch.cuda.synchronize()
	s.wait_stream(torch.cuda.default_stream())
	with torch.cuda.stream(s):
		ev = S.gate(s)
		buf.copy_(true, non_blocking=True)
		_solve(solver, buf, got)
		S.held(ev)
		s.synchronize()
	for i, (a, b) in enumerate(zip(got, want)):
		assert S.same_bits(a, b), (i, int((S.bits(a) != S.bits(b)).sum()))
	lengths, reason = want[0].cpu().numpy(), want[3].cpu().numpy()
	assert (lengths == 0).any() and lengths.max() >= 30 and int(want[5]) == -1 and {0, 2} <= set(reason.tolist())
	decoy = _out(ref)
	_solve(ref, _states(1), decoy)
	assert not S.same_bits(decoy[0], want[0])                            # a launch that read the decoy would have shown
