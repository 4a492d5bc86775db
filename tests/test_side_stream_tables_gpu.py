"""
The table-backed engines on a torch side stream behind a gate (tests/side_stream.py, pattern A), one record per kind: rk_chain_create
and rk_chain_solve, rk_twophase_create and rk_twophase_solve, rk_pdb_build (the cross) with rk_pdb_depth and rk_pdb_solve.  The
tables are made on the side stream, the inputs arrive BEHIND the gate over other legal states, the outputs start as sentinel bytes
(the pattern database's error word as zero), and everything is compared bit for bit with an object made and run on the default
stream, which tests/test_chain_gpu.py, tests/test_twophase_gpu.py and tests/test_pdb_gpu.py pin against the models.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceChainSolver, DevicePatternDB, DeviceTwoPhaseSolver
from tests import side_stream as S

pytestmark = pytest.mark.gpu

N = 300
TRIES, MAX_NODES = 2, 2048


def _chain_solve(solver, q, out):
	lengths, actions, stages, err = out
	_ffi.check(_ffi.lib().rk_chain_solve(solver._h, q.data_ptr(), N, lengths.data_ptr(), actions.data_ptr(), stages.data_ptr(), err.data_ptr(),
	                                     _ffi.stream_ptr()))


def _chain_same(solver, ref):
	assert solver.coset_counts == ref.coset_counts and solver.stage_depths == ref.stage_depths
	for stage in range(1, 5):
		assert (solver.export(stage) == ref.export(stage)).all()


def _chain_sane(want):
	lengths = want[0].cpu().numpy()
	assert (lengths == 0).any() and lengths.max() >= 30 and int(want[3]) == -1


def _twophase_solve(solver, q, out):
	_ffi.check(_ffi.lib().rk_twophase_solve(solver._h, solver.chain._h, q.data_ptr(), N, TRIES, MAX_NODES, *[t.data_ptr() for t in out],
	                                        _ffi.stream_ptr()))


def _twophase_same(solver, ref):
	assert solver.table_counts == ref.table_counts and solver.table_depths == ref.table_depths
	for table in range(1, 5):
		assert (solver.export(table) == ref.export(table)).all()


def _twophase_sane(want):
	lengths, reason = want[0].cpu().numpy(), want[3].cpu().numpy()
	assert (lengths == 0).any() and lengths.max() >= 30 and int(want[5]) == -1 and {0, 2} <= set(reason.tolist())


def _pdb_depth_solve(db, q, out):
	lib, st = _ffi.lib(), _ffi.stream_ptr()
	depth, lengths, actions, err = out
	_ffi.check(lib.rk_pdb_depth(db._h, q.data_ptr(), N, depth.data_ptr(), st))
	_ffi.check(lib.rk_pdb_solve(db._h, q.data_ptr(), N, lengths.data_ptr(), actions.data_ptr(), err.data_ptr(), st))


def _pdb_same(db, ref):
	assert db.level_sizes.tolist() == ref.level_sizes.tolist() and (db.table() == ref.table()).all()


def _pdb_sane(want):
	depth = want[0].cpu().numpy()
	assert (depth == 0).any() and depth.max() >= 5 and int(want[3]) == 0 and (want[1].cpu().numpy() == depth).all()


# make: the object, its tables made on the current stream (create and build synchronise); out: the entry's outputs as they start;
# entry: the call through _ffi.lib(); same: made on the side stream == made on the default stream; sane: the answers are not trivial
KINDS = {
	"chain": SimpleNamespace(
		make=DeviceChainSolver, depth=60, seed=2_700, entry=_chain_solve, same=_chain_same, sane=_chain_sane,
		out=lambda o: [S.sentinel((N,), torch.int32), S.sentinel((N, o.max_length), torch.int8), S.sentinel((N, 4), torch.int32),
		               S.sentinel((1,), torch.int32)]),
	"twophase": SimpleNamespace(
		make=lambda: DeviceTwoPhaseSolver(tries=TRIES, max_nodes=MAX_NODES), depth=60, seed=2_900, entry=_twophase_solve, same=_twophase_same,
		sane=_twophase_sane,
		out=lambda o: [S.sentinel((N,), torch.int32), S.sentinel((N, o.max_length), torch.int8), S.sentinel((N, 2), torch.int32),
		               S.sentinel((N,), torch.int32), S.sentinel((N,), torch.int64), S.sentinel((1,), torch.int32)]),
	"pdb": SimpleNamespace(
		make=lambda: DevicePatternDB.cross("D").build(), depth=12, seed=2_500, entry=_pdb_depth_solve, same=_pdb_same, sane=_pdb_sane,
		out=lambda o: [S.sentinel((N,), torch.int32), S.sentinel((N,), torch.int32), S.sentinel((N, o.max_depth), torch.int8),
		               torch.zeros(1, dtype=torch.int32, device="cuda")]),
}


@functools.lru_cache(maxsize=None)
def _reference(kind):
	made = KINDS[kind].make()
	torch.cuda.synchronize()
	return made


@functools.lru_cache(maxsize=None)
def _side(kind):
	"""-> the object made on a side stream behind a gate (making it synchronises, so the gate is checked before it), and that stream"""
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		ev = S.gate(s)
		S.held(ev)
		made = KINDS[kind].make()
		s.synchronize()
	return made, s


@functools.lru_cache(maxsize=None)
def _states(kind, seed=0) -> torch.Tensor:
	return torch.from_numpy(S.mixed_depths(N, KINDS[kind].depth, KINDS[kind].seed + seed)).cuda()


@pytest.mark.parametrize("kind", list(KINDS))
def test_made_on_a_side_stream(kind):
	KINDS[kind].same(_side(kind)[0], _reference(kind))


@pytest.mark.parametrize("kind", list(KINDS))
def test_entries_on_a_side_stream(kind):
	k, ref, (made, s) = KINDS[kind], _reference(kind), _side(kind)
	true, buf = _states(kind), _states(kind, 1).clone()
	want, got = k.out(ref), k.out(made)
	k.entry(ref, true, want)
	torch.cuda.synchronize()
	s.wait_stream(torch.cuda.default_stream())
	with torch.cuda.stream(s):
		ev = S.gate(s)
		buf.copy_(true, non_blocking=True)
		k.entry(made, buf, got)
		S.held(ev)
		s.synchronize()
	for i, (a, b) in enumerate(zip(got, want)):
		assert S.same_bits(a, b), (i, int((S.bits(a) != S.bits(b)).sum()))
	k.sane(want)
	decoy = k.out(ref)
	k.entry(ref, _states(kind, 1), decoy)
	assert not S.same_bits(decoy[0], want[0])                            # a launch that read the decoy would have shown
