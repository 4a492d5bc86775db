"""
Both kept balls on a torch side stream behind a gate (tests/side_stream.py, pattern A), at radius 4: the build (rk_ball_build,
rk_symball_build) and every reader -- depth, solve, child_values, state_at with the first build of the orbit index, child_depths and
the shortening pass of both balls.  The readers' inputs arrive BEHIND the gate over other legal inputs, outputs start as sentinel
bytes, and everything is compared bit for bit with a second ball built and read on the default stream (which
tests/test_ball_readers_batch_gpu.py, test_goal_ball_gpu.py, test_sym_gpu.py and test_ball_shorten_gpu.py pin against the models).
About 300 states scrambled 0 to 6 moves deep: rows inside the ball, on its rim and outside it.
"""
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall
from tests import side_stream as S

pytestmark = pytest.mark.gpu

RADIUS = 4
N = 300                        # 12 * 25: also the children of 25 rollout states for child_values
KINDS = {"goal": DeviceGoalBall, "sym": DeviceSymBall}


@functools.lru_cache(maxsize=None)
def _reference(kind):
	"""the ball built on the default stream"""
	ball = KINDS[kind](RADIUS).build()
	torch.cuda.synchronize()
	return ball


@functools.lru_cache(maxsize=None)
def _side(kind):
	"""-> the ball built on a side stream behind a gate (the build polls, so the gate is checked before it), and that stream"""
	torch.cuda.synchronize()
	s = S.side_stream()
	ball = KINDS[kind](RADIUS)
	with torch.cuda.stream(s):
		ev = S.gate(s)
		S.held(ev)
		ball.build()
		s.synchronize()
	return ball, s


@functools.lru_cache(maxsize=None)
def _states(seed=0) -> torch.Tensor:
	return torch.from_numpy(S.mixed_depths(N, 6, 400 + seed)).cuda()


def _gated(s, pairs, enqueue, held_first=False):
	"""pattern A on stream `s`: the gate, the true inputs over their decoys (`pairs` of (buffer, true)), `enqueue`, the gate still
	closed (`held_first`: checked before an entry that may block), then wait"""
	torch.cuda.synchronize()
	s.wait_stream(torch.cuda.default_stream())
	with torch.cuda.stream(s):
		ev = S.gate(s)
		for buf, true in pairs:
			buf.copy_(true, non_blocking=True)
		if held_first:
			S.held(ev)
		enqueue()
		if not held_first:
			S.held(ev)
		s.synchronize()


def _same(got, want):
	for i, (a, b) in enumerate(zip(got, want)):
		assert S.same_bits(a, b), (i, int((S.bits(a) != S.bits(b)).sum()))


@pytest.mark.parametrize("kind", ["goal", "sym"])
def test_build_on_a_side_stream(kind):
	ref, (ball, _) = _reference(kind), _side(kind)
	assert len(ball) == len(ref) and (ball.level_start == ref.level_start).all() and ball.iterations == ref.iterations
	for a, b in zip(ball.arrays(), ref.arrays()):
		assert a.dtype == b.dtype and (a == b).all()
	if kind == "sym":
		assert (ball.states_covered == ref.states_covered).all() and ball.states_covered.tolist() == list(DeviceGoalBall.LEVELS[:RADIUS + 1])


def _depth_solve(ball, q, out):
	lib, n, st = _ffi.lib(), len(q), _ffi.stream_ptr()
	depth, lengths, actions, err = out
	_ffi.check(ball._entry("depth")(ball._h, q.data_ptr(), n, depth.data_ptr(), st))
	if isinstance(ball, DeviceSymBall):
		_ffi.check(lib.rk_symball_solve(ball._h, q.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(), err.data_ptr(), st))
	else:
		_ffi.check(lib.rk_ball_solve(ball._h, q.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(), st))


def _depth_solve_out():
	return [S.sentinel((N,), torch.int32), S.sentinel((N,), torch.int32), S.sentinel((N, RADIUS), torch.int8), torch.zeros(1, dtype=torch.int32, device="cuda")]


@pytest.mark.parametrize("kind", ["goal", "sym"])
def test_depth_and_solve(kind):
	ref, (ball, s) = _reference(kind), _side(kind)
	true, buf = _states(), _states(1).clone()
	want, got = _depth_solve_out(), _depth_solve_out()
	_depth_solve(ref, true, want)
	_gated(s, [(buf, true)], lambda: _depth_solve(ball, buf, got))
	_same(got, want)
	depth = want[0].cpu().numpy()
	assert (depth == -1).any() and (depth == RADIUS).any() and (depth == 0).any() and int(want[3]) == 0
	decoy = _depth_solve_out()
	_depth_solve(ref, _states(1), decoy)
	assert not S.same_bits(decoy[0], want[0])


def _child_values(ball, sub, out):
	depths, values, rows, outside, count, scratch = out
	_ffi.check(_ffi.lib().rk_symball_child_values(ball._h, sub.data_ptr(), N, 1.0, depths.data_ptr(), values.data_ptr(), rows.data_ptr(),
	                                              outside.data_ptr(), count.data_ptr(), scratch.data_ptr(), scratch.numel(), _ffi.stream_ptr()))


def _child_values_out():
	need = int(_ffi.lib().rk_symball_child_values_scratch_bytes(N))
	assert need >= 0
	return [S.sentinel((N,), torch.int8), S.sentinel((N,), torch.float32), S.sentinel((N,), torch.int32), S.sentinel((N, 20), torch.int8),
	        S.sentinel((1,), torch.int32), torch.zeros(max(need, 4), dtype=torch.uint8, device="cuda")]


def test_child_values():
	ref, (ball, s) = _reference("sym"), _side("sym")
	true, buf = _states(), _states(1).clone()
	want, got = _child_values_out(), _child_values_out()
	_child_values(ref, true, want)
	_gated(s, [(buf, true)], lambda: _child_values(ball, buf, got))
	k = int(want[4])
	assert 0 < k < N and int(got[4]) == k
	_same([got[0], got[1], got[2][:k], got[3][:k]], [want[0], want[1], want[2][:k], want[3][:k]])      # (values keep the prefill outside the ball)


def _ranks():
	covered = DeviceGoalBall.LEVELS
	depths = np.concatenate([np.full(covered[d], d) for d in range(3)] + [np.full(64, 4)]).astype(np.int32)
	ranks = np.concatenate([np.arange(covered[d]) for d in range(3)] + [np.arange(64) * (covered[4] // 64) + 7]).astype(np.int64)
	return torch.from_numpy(depths).cuda(), torch.from_numpy(ranks).cuda()


def _state_at(ball, depths, ranks, out, err):
	_ffi.check(_ffi.lib().rk_symball_state_at(ball._h, depths.data_ptr(), ranks.data_ptr(), len(ranks), out.data_ptr(), err.data_ptr(), _ffi.stream_ptr()))


def test_state_at_with_the_first_index_build_on_the_side_stream():
	ref, (ball, s) = _reference("sym"), _side("sym")
	depths, ranks = _ranks()
	n = len(ranks)
	want, want_err = S.sentinel((n, 20), torch.int8), S.sentinel((1,), torch.int32)
	_state_at(ref, depths, ranks, want, want_err)
	assert int(want_err) == 0
	# every state once, at its depth
	host = want.cpu().numpy()
	assert len({r.tobytes() for r in host}) == n and (ref.depth(host) == depths.cpu().numpy()).all()
	first = ball.index_builds == 0
	for held_first in (True, False):                  # the first call makes the orbit index (it may allocate and wait), the second only reads it
		dbuf, rbuf = torch.full_like(depths, 1), torch.arange(n, dtype=torch.int64, device="cuda") % 12      # decoy: level 1, legal ranks
		got, err = S.sentinel((n, 20), torch.int8), S.sentinel((1,), torch.int32)
		_gated(s, [(dbuf, depths), (rbuf, ranks)], lambda: _state_at(ball, dbuf, rbuf, got, err), held_first=held_first)
		assert int(err) == 0 and S.same_bits(got, want)
	assert ball.index_builds == 1 and first


def _child_depths(ball, q, out):
	depth, children, err = out
	_ffi.check(_ffi.lib().rk_symball_child_depths(ball._h, q.data_ptr(), len(q), depth.data_ptr(), children.data_ptr(), err.data_ptr(), _ffi.stream_ptr()))


def test_child_depths():
	ref, (ball, s) = _reference("sym"), _side("sym")
	true, buf = _states(), _states(1).clone()
	make = lambda: [S.sentinel((N,), torch.int8), S.sentinel((N, 12), torch.int8), S.sentinel((1,), torch.int32)]
	want, got = make(), make()
	_child_depths(ref, true, want)
	_gated(s, [(buf, true)], lambda: _child_depths(ball, buf, got))
	_same(got, want)
	d = want[0].cpu().numpy()
	assert int(want[2]) == 0 and (d == -1).any() and (d == RADIUS + 1).any() and (d == 0).any()


@pytest.mark.parametrize("kind", ["goal", "sym"])
def test_shorten_pass(kind):
	"""one pass of rk_bshorten / rk_sshorten over 24 queues of 40 moves at window 8 (the last queue shorter: a padded row)"""
	ref, (ball, s) = _reference(kind), _side(kind)
	n, L, w = 24, 40, 8
	rs = np.random.RandomState(9)

	def queues():
		a = rs.randint(0, 12, (n, L)).astype(np.int8)
		a[:, 10:14] = a[:, 6:10][:, ::-1] ^ 1          # four moves undone at once: something to shorten in every queue
		lens = np.full(n, L, np.int32)
		lens[-1], a[-1, 29:] = 29, -1
		return torch.from_numpy(a).cuda(), torch.from_numpy(lens).cuda()
	(acts, lens), (abuf, lbuf) = queues(), queues()
	need = int(_ffi.lib().rk_bshorten_scratch_bytes(n, L, w))
	assert need > 0

	def out():
		return [S.sentinel((n, L), torch.int8), S.sentinel((n,), torch.int32), S.sentinel((1,), torch.int32), torch.zeros(need, dtype=torch.uint8, device="cuda")]

	def shorten(b, a, l, o):
		b._shorten(a.data_ptr(), l.data_ptr(), n, L, w, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), need, _ffi.stream_ptr())
	want, got = out(), out()
	shorten(ref, acts, lens, want)
	lbuf[-1] = L - 3
	abuf[-1] = abuf[0]
	assert not torch.equal(abuf, acts) and not torch.equal(lbuf, lens)
	_gated(s, [(abuf, acts), (lbuf, lens)], lambda: shorten(ball, abuf, lbuf, got))
	out_len = want[1].cpu().numpy()
	assert int(want[2]) == 0 and (out_len <= lens.cpu().numpy() - 4).all()
	assert S.same_bits(got[1], want[1]) and S.same_bits(got[2], want[2])
	for r in range(n):                                # (beyond a queue's new length its row keeps what it held)
		assert torch.equal(got[0][r, :out_len[r]], want[0][r, :out_len[r]]), r
