"""
rk_pdb_depth and rk_pdb_solve on a torch side stream behind a gate (tests/side_stream.py, pattern A), for the cross: the inputs arrive
BEHIND the gate over other legal states, the outputs start as sentinel bytes, and everything is compared bit for bit with the same
entries on the default stream (which tests/test_pdb_gpu.py pins against the model).  The build on a side stream too: its table and
level sizes against a table built on the default stream.
"""
import functools

import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DevicePatternDB
from tests import side_stream as S

pytestmark = pytest.mark.gpu

N = 300


@functools.lru_cache(maxsize=None)
def _reference():
	db = DevicePatternDB.cross("D").build()
	torch.cuda.synchronize()
	return db


@functools.lru_cache(maxsize=None)
def _side():
	"""-> the table built on a side stream behind a gate (the build synchronises, so the gate is checked before it), and that stream"""
	torch.cuda.synchronize()
	s = S.side_stream()
	db = DevicePatternDB.cross("D")
	with torch.cuda.stream(s):
		ev = S.gate(s)
		S.held(ev)
		db.build()
		s.synchronize()
	return db, s


@functools.lru_cache(maxsize=None)
def _states(seed=0) -> torch.Tensor:
	return torch.from_numpy(S.mixed_depths(N, 12, 2_500 + seed)).cuda()


def _out(db):
	return [S.sentinel((N,), torch.int32), S.sentinel((N,), torch.int32), S.sentinel((N, db.max_depth), torch.int8),
	        torch.zeros(1, dtype=torch.int32, device="cuda")]


def _depth_solve(db, q, out):
	lib, st = _ffi.lib(), _ffi.stream_ptr()
	depth, lengths, actions, err = out
	_ffi.check(lib.rk_pdb_depth(db._h, q.data_ptr(), N, depth.data_ptr(), st))
	_ffi.check(lib.rk_pdb_solve(db._h, q.data_ptr(), N, lengths.data_ptr(), actions.data_ptr(), err.data_ptr(), st))


def test_build_on_a_side_stream():
	ref, (db, _) = _reference(), _side()
	assert db.level_sizes.tolist() == ref.level_sizes.tolist() and (db.table() == ref.table()).all()


def test_depth_and_solve_on_a_side_stream():
	ref, (db, s) = _reference(), _side()
	true, buf = _states(), _states(1).clone()
	want, got = _out(ref), _out(db)
	_depth_solve(ref, true, want)
	torch.cuda.synchronize()
	s.wait_stream(torch.cuda.default_stream())
	with torch.cuda.stream(s):
		ev = S.gate(s)
		buf.copy_(true, non_blocking=True)
		_depth_solve(db, buf, got)
		S.held(ev)
		s.synchronize()
	for i, (a, b) in enumerate(zip(got, want)):
		assert S.same_bits(a, b), (i, int((S.bits(a) != S.bits(b)).sum()))
	depth = want[0].cpu().numpy()
	assert (depth == 0).any() and depth.max() >= 5 and int(want[3]) == 0 and (want[1].cpu().numpy() == depth).all()
	decoy = _out(ref)
	_depth_solve(ref, _states(1), decoy)
	assert not S.same_bits(decoy[0], want[0])                            # a launch that read the decoy would have shown
