"""
rk_chain_create and rk_chain_solve on a torch side stream behind a gate (tests/side_stream.py, pattern A): the tables are uploaded on
the side stream, the inputs arrive BEHIND the gate over other legal states, the outputs start as sentinel bytes, and everything is
compared bit for bit with a solver made and run on the default stream (which tests/test_chain_gpu.py pins against the model).
"""
import functools

import torch

import pytest

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceChainSolver
from tests import side_stream as S

pytestmark = pytest.mark.gpu

N = 300


@functools.lru_cache(maxsize=None)
def _reference():
	solver = DeviceChainSolver()
	torch.cuda.synchronize()
	return solver


@functools.lru_cache(maxsize=None)
def _side():
	"""-> a solver made on a side stream behind a gate (create synchronises, so the gate is checked before it), and that stream"""
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		ev = S.gate(s)
		S.held(ev)
		solver = DeviceChainSolver()
		s.synchronize()
	return solver, s


@functools.lru_cache(maxsize=None)
def _states(seed=0) -> torch.Tensor:
	return torch.from_numpy(S.mixed_depths(N, 60, 2_700 + seed)).cuda()


def _out(solver):
	return [S.sentinel((N,), torch.int32), S.sentinel((N, solver.max_length), torch.int8), S.sentinel((N, 4), torch.int32),
	        S.sentinel((1,), torch.int32)]


def _solve(solver, q, out):
	lengths, actions, stages, err = out
	_ffi.check(_ffi.lib().rk_chain_solve(solver._h, q.data_ptr(), N, lengths.data_ptr(), actions.data_ptr(), stages.data_ptr(), err.data_ptr(),
	                                     _ffi.stream_ptr()))


def test_create_on_a_side_stream():
	ref, (solver, _) = _reference(), _side()
	assert solver.coset_counts == ref.coset_counts and solver.stage_depths == ref.stage_depths
	for stage in range(1, 5):
		assert (solver.export(stage) == ref.export(stage)).all()


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
	lengths = want[0].cpu().numpy()
	assert (lengths == 0).any() and lengths.max() >= 30 and int(want[3]) == -1
	decoy = _out(ref)
	_solve(ref, _states(1), decoy)
	assert not S.same_bits(decoy[0], want[0])                            # a launch that read the decoy would have shown
