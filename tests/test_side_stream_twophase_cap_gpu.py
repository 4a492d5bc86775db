"""
rk_twophase_solve_capped on a torch side stream behind a gate (tests/side_stream.py, pattern A), in the style of
tests/test_side_stream_tables_gpu.py: the solver is made on the side stream, the inputs arrive BEHIND the gate over other legal
states, the outputs -- the two counts among them -- start as sentinel bytes, and everything is compared bit for bit with a solver
made and run on the default stream, which tests/test_twophase_cap_gpu.py pins against the model.
"""
import functools

import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceTwoPhaseSolver
from tests import side_stream as S

pytestmark = pytest.mark.gpu

N = 300
MAX_NODES, CAP = 2048, 8
DEPTH, SEED = 60, 3_200


def _entry(solver, q, out):
	_ffi.check(_ffi.lib().rk_twophase_solve_capped(solver._h, solver.chain._h, q.data_ptr(), N, solver.tries, MAX_NODES, CAP,
	                                               *[t.data_ptr() for t in out], _ffi.stream_ptr()))


def _out(solver):
	return [S.sentinel((N,), torch.int32), S.sentinel((N, solver.max_length), torch.int8), S.sentinel((N, 2), torch.int32),
	        S.sentinel((N,), torch.int32), S.sentinel((N,), torch.int64), S.sentinel((N, 2), torch.int32), S.sentinel((1,), torch.int32)]


def _make():
	return DeviceTwoPhaseSolver(tries=None, max_nodes=MAX_NODES, phase2_cap=CAP)


@functools.lru_cache(maxsize=None)
def _states(seed=0) -> torch.Tensor:
	return torch.from_numpy(S.mixed_depths(N, DEPTH, SEED + seed)).cuda()


def test_the_capped_entry_on_a_side_stream():
	ref = _make()
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		ev = S.gate(s)
		S.held(ev)
		made = _make()
		s.synchronize()
	true, buf = _states(), _states(1).clone()
	want, got = _out(ref), _out(made)
	_entry(ref, true, want)
	torch.cuda.synchronize()
	s.wait_stream(torch.cuda.default_stream())
	with torch.cuda.stream(s):
		ev = S.gate(s)
		buf.copy_(true, non_blocking=True)
		_entry(made, buf, got)
		S.held(ev)
		s.synchronize()
	for i, (a, b) in enumerate(zip(got, want)):
		assert S.same_bits(a, b), (i, int((S.bits(a) != S.bits(b)).sum()))
	lengths, reason, counts = want[0].cpu().numpy(), want[3].cpu().numpy(), want[5].cpu().numpy()
	assert (lengths == 0).any() and lengths.max() >= 30 and int(want[6]) == -1 and {0, 2} <= set(reason.tolist())
	assert (counts[:, 1] <= counts[:, 0]).all() and (counts >= 0).all() and counts[:, 1].max() >= 1
	decoy = _out(ref)
	_entry(ref, _states(1), decoy)
	assert not S.same_bits(decoy[0], want[0])                            # a launch that read the decoy would have shown
