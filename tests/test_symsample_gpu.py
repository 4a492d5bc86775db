"""
`DeviceSymBall.state_at`, `sample`, `child_depths`, `cube.device.ball_state_at` / `ball_child_depths` (engines rk_symball_state_at,
rk_symball_child_depths) and `adi.ball_traindata` on the GPU, row for row against tests/symsample_model.py (pinned on the host by
tests/test_symsample_cpu.py), against the plain balls and against the existing entries (`depth`, `ball_child_values`).
  * radius 4 (251 orbits, one tile, 29 orbits smaller than 48) and radius 6 (20 624 orbits = 81 tiles, levels 5 and 6 start
    mid-tile at nodes 252 and 2 230, the last tile is short): EVERY rank of every level, so the map is checked to be a bijection;
  * mixed depths, any order, n = 1 and n = 0, a call cut in two; the documented draws of `sample`; misuse; 6x8x6 mode;
  * child_depths against true distances inside radius + 1 and -1 beyond; ball_traindata's targets; the index's accounting.
No ball above radius 6 is built.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.adi import ball_traindata
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall
from oracle import c_oracle
from oracle import cube_oracle as orc
from tests import ball_model, sym_model, symsample_model as model

pytestmark = pytest.mark.gpu
RK_EINVAL, RK_ESTATE = -1, -4
_BALLS = {}


def _ball(radius: int) -> DeviceSymBall:
	if radius not in _BALLS:
		_BALLS[radius] = DeviceSymBall(radius)
	return _BALLS[radius]


def _all_ranks(covered):
	depths = np.repeat(np.arange(len(covered)), covered)
	ranks = np.concatenate([np.arange(c) for c in covered])
	return depths, ranks


@functools.lru_cache(maxsize=None)
def _every_state(radius: int):
	"""(depths, ranks, states) of every rank of every level in ONE call; read-only"""
	ball = _ball(radius)
	depths, ranks = _all_ranks(ball.states_covered)
	states = ball.state_at(depths, ranks)
	for a in (depths, ranks, states):
		a.flags.writeable = False
	return depths, ranks, states


@functools.lru_cache(maxsize=None)
def _plain(radius: int):
	return ball_model.build(radius)


def _level(plain, d: int) -> np.ndarray:
	return plain.states[plain.level_start[d] - 1:plain.level_start[d + 1] - 1]


def _rows(a) -> set:
	return {r.tobytes() for r in np.ascontiguousarray(a, np.int8).reshape(-1, 20)}


def test_radius_4_every_rank_of_every_level():
	ball = _ball(4)
	depths, ranks, got = _every_state(4)
	assert got.shape == (11_206, 20) and got.dtype == np.int8 and len(ball) == 251
	want_ball = sym_model.build(4)
	assert (ball.arrays() == want_ball.states).all() and (ball.level_start == want_ball.level_start).all()
	assert (got == model.state_at(want_ball.states, want_ball.level_start, depths, ranks)).all()
	for d in range(5):
		assert _rows(got[depths == d]) == _rows(_level(_plain(4), d)), d
	_, first = model.orbits(want_ball.states)
	assert (first.sum(axis=0) < 48).sum() == 29


def test_radius_6_every_rank_of_every_level_is_a_bijection():
	ball = _ball(6)
	depths, ranks, got = _every_state(6)
	assert tuple(ball.states_covered) == DeviceGoalBall.LEVELS[:7] and len(got) == 983_926 == sum(DeviceGoalBall.LEVELS[:7])
	assert len(ball) == 20_624 and ball.level_start[5] == 252 and ball.level_start[6] == 2_230 and len(ball) % 256
	assert ball.index_bytes == 81 * 256 + 82 * 8
	assert (got == model.state_at(ball.arrays(), ball.level_start, depths, ranks)).all()
	assert (ball.depth(np.array(got)) == depths).all()
	assert len(np.unique(np.ascontiguousarray(got).view("V20"))) == 983_926


def test_any_order_mixed_depths_one_none_and_a_call_cut_in_two():
	ball = _ball(6)
	depths, ranks, states = _every_state(6)
	covered = ball.states_covered
	start = np.concatenate([[0], np.cumsum(covered)])
	ends = np.concatenate([start[:-1], start[1:] - 1])                  # the first and the last rank of every level
	pick = np.concatenate([ends, np.random.default_rng(5).permutation(len(ranks))[:5000]])
	got = ball.state_at(depths[pick], ranks[pick])
	assert (got == states[pick]).all()
	assert (ball.state_at(depths[pick[:77]], ranks[pick[:77]]) == got[:77]).all() and (ball.state_at(depths[pick[77:]], ranks[pick[77:]]) == got[77:]).all()
	one = ball.state_at(6, [covered[6] - 1])
	assert one.shape == (1, 20) and (one == states[-1]).all()
	assert (ball.state_at(0, [0]) == orc.SOLVED).all()
	assert (ball.state_at(3, np.arange(40, 50)) == states[start[3] + 40:start[3] + 50]).all()
	none = ball.state_at(np.zeros(0, np.int64), np.zeros(0, np.int64))
	assert none.shape == (0, 20) and none.dtype == np.int8 and ball.state_at(2, []).shape == (0, 20)
	# tensors in, tensors out, into a given tensor
	d_t = torch.from_numpy(depths[pick].astype(np.int32)).cuda()
	r_t = torch.from_numpy(ranks[pick]).cuda()
	out = torch.zeros((len(pick), 20), dtype=torch.int8, device="cuda")
	assert cube.device.ball_state_at(ball, d_t, r_t, out) is out and (out.cpu().numpy() == got).all()
	assert (cube.device.ball_state_at(ball, d_t, r_t).cpu().numpy() == got).all()


@pytest.mark.parametrize("radius", [4, 6])
def test_sample_makes_the_documented_draws(radius):
	ball = _ball(radius)
	covered = ball.states_covered
	n = 3000
	# an int
	a, b = np.random.default_rng(11), np.random.default_rng(11)
	states, depths = ball.sample(n, radius, a)
	ranks = b.integers(0, covered[np.full(n, radius)], dtype=np.int64)
	assert (depths == radius).all() and depths.dtype == np.int64 and (states == ball.state_at(radius, ranks)).all()
	assert a.bit_generator.state == b.bit_generator.state
	# an array
	want_d = np.random.default_rng(3).integers(0, radius + 1, n)
	states, depths = ball.sample(n, want_d, a)
	ranks = b.integers(0, covered[want_d], dtype=np.int64)
	assert (depths == want_d).all() and (states == ball.state_at(want_d, ranks)).all() and (ball.depth(states) == want_d).all()
	assert a.bit_generator.state == b.bit_generator.state
	# None: uniform over the whole ball
	states, depths = ball.sample(n, rng=a)
	g = b.integers(0, int(covered.sum()), n, dtype=np.int64)
	c = np.cumsum(covered)
	want_d = np.searchsorted(c, g, side="right")
	assert (depths == want_d).all() and (states == ball.state_at(want_d, g - (c - covered)[want_d])).all()
	assert a.bit_generator.state == b.bit_generator.state
	assert (ball.depth(states) == depths).all()
	# no generator: one of its own
	states, depths = ball.sample(7, 2)
	assert states.shape == (7, 20) and (ball.depth(states) == 2).all()
	assert ball.sample(0, 1, a)[0].shape == (0, 20)


def test_misuse_raises_before_any_launch():
	ball = _ball(4)
	ball.state_at(0, [0])
	builds = ball.index_builds
	for depths, ranks in ((-1, [0]), (5, [0]), (2, [-1]), (2, [114]), (4, [10_011]), ([1, 2], [0]), ([1], [0, 1]), (1.5, [0]), (1, [0.5])):
		with pytest.raises(ValueError):
			ball.state_at(depths, ranks)
	for n, depth in ((3, -1), (3, 5), (3, [1, 2]), (-1, 1), (3, 1.0)):
		with pytest.raises(ValueError):
			ball.sample(n, depth)
	with pytest.raises(TypeError):
		ball.sample(3, 1, np.random.RandomState(1))
	d_t, r_t = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
	with pytest.raises(TypeError):
		cube.device.ball_state_at(DeviceGoalBall(2), d_t, r_t)
	with pytest.raises(ValueError):
		cube.device.ball_state_at(ball, d_t.long(), r_t)
	with pytest.raises(ValueError):
		cube.device.ball_state_at(ball, d_t[:1], r_t)
	with pytest.raises(ValueError):
		cube.device.ball_child_depths(ball, torch.zeros((2, 21), dtype=torch.int8, device="cuda"))
	assert ball.index_builds == builds


def test_the_entry_flags_a_bad_rank_writes_zeros_and_goes_on():
	lib, stream = _ffi.lib(), _ffi.stream_ptr()
	ball = _ball(4).build()
	depths = torch.tensor([2, 2, 5, -1, 4, 4, 3], dtype=torch.int32, device="cuda")
	ranks = torch.tensor([5, 114, 0, 0, -1, 10_010, 7], dtype=torch.int64, device="cuda")
	bad = np.array([False, True, True, True, True, False, False])
	out = torch.full((7, 20), 77, dtype=torch.int8, device="cuda")
	err = torch.full((1,), 9, dtype=torch.int32, device="cuda")
	assert lib.rk_symball_state_at(ball._h, depths.data_ptr(), ranks.data_ptr(), 7, out.data_ptr(), err.data_ptr(), stream) == 0
	assert int(err.item()) == RK_EINVAL
	got = out.cpu().numpy()
	assert (got[bad] == 0).all()
	assert (got[~bad] == ball.state_at(depths.cpu().numpy()[~bad], ranks.cpu().numpy()[~bad])).all()
	with pytest.raises(ValueError):
		cube.device.ball_state_at(ball, depths, ranks)
	# the call after it works and clears the word
	assert lib.rk_symball_state_at(ball._h, depths[:1].data_ptr(), ranks[:1].data_ptr(), 1, out.data_ptr(), err.data_ptr(), stream) == 0
	assert int(err.item()) == 0 and (out[0].cpu().numpy() == got[0]).all()
	# argument errors come back as codes, before any launch
	args = [depths.data_ptr(), ranks.data_ptr(), 7, out.data_ptr(), err.data_ptr()]
	assert lib.rk_symball_state_at(None, *args, stream) == RK_EINVAL
	for i in (0, 1, 3, 4):
		a = list(args)
		a[i] = None
		assert lib.rk_symball_state_at(ball._h, *a, stream) == RK_EINVAL and b"null pointer" in lib.rk_last_error(), i
		a[i] = args[i] + 2
		assert lib.rk_symball_state_at(ball._h, *a, stream) == RK_EINVAL and b"aligned" in lib.rk_last_error(), i
	assert lib.rk_symball_child_depths(None, out.data_ptr(), 7, out.data_ptr(), out.data_ptr(), err.data_ptr(), stream) == RK_EINVAL
	assert lib.rk_symball_child_depths(ball._h, out.data_ptr(), 7, out.data_ptr(), None, err.data_ptr(), stream) == RK_EINVAL
	assert lib.rk_symball_child_depths(ball._h, out.data_ptr(), 7, out.data_ptr(), out.data_ptr(), None, stream) == RK_EINVAL
	fresh = C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(fresh), 2, 16, 0))
	try:                                                                 # not built: refused as rk_symball_depth refuses it
		assert lib.rk_symball_state_at(fresh, *args, stream) == RK_ESTATE and b"build the ball first" in lib.rk_last_error()
		assert lib.rk_symball_child_depths(fresh, out.data_ptr(), 7, out.data_ptr(), out.data_ptr(), err.data_ptr(), stream) == RK_ESTATE
		status = (C.c_longlong * 16)()
		assert lib.rk_symball_index_status(fresh, status) == 0 and not any(status)
		assert lib.rk_symball_index_status(None, status) == RK_EINVAL
	finally:
		assert lib.rk_symball_destroy(fresh) == 0
	torch.cuda.synchronize()
	assert int(err.item()) == 0


@functools.lru_cache(maxsize=None)
def _lookup(radius: int) -> dict:
	"""{20 state bytes: true distance} of every state within `radius` of solved; read-only"""
	plain = _plain(radius)
	return {k: ball_model.depth_of(plain, v) for k, v in plain.index.items()}


def test_child_depths_radius_4_against_true_distances():
	ball, plain6 = _ball(4), _plain(6)
	scrambles = np.stack([ball_model.scramble(700 + i, 20) for i in range(200)])
	inside = np.concatenate([_plain(4).states, _level(plain6, 5)])       # within radius + 1: every answer is exact
	beyond = _level(plain6, 6)
	got_d, got_c = ball.child_depths(np.concatenate([inside, beyond, scrambles]))
	assert got_d.dtype == got_c.dtype == np.int64 and got_c.shape == (len(got_d), 12)
	want_d, want_c = model.child_depths(_lookup(6), inside)
	assert (want_d >= 0).all() and (want_c >= 0).all() and want_d.max() == 5 and want_c.max() == 6
	assert (got_d[:len(inside)] == want_d).all() and (got_c[:len(inside)] == want_c).all()
	at = len(inside) + len(beyond)
	assert (got_d[len(inside):at] == -1).all() and (got_c[len(inside):at] == -1).all()
	# a scramble more than 5 moves from solved (the plain ball of radius 6 tells those within 6; the others are further still)
	lookup = _lookup(6)
	true_d = np.array([lookup.get(s.tobytes(), 99) for s in scrambles])
	far = true_d > 5
	assert far.sum() >= 190
	assert (got_d[at:][far] == -1).all() and (got_c[at:][far] == -1).all()
	near_d, near_c = model.child_depths(lookup, scrambles[~far])
	assert (got_d[at:][~far] == near_d).all() and (got_c[at:][~far] == near_c).all()


def test_child_depths_radius_6_against_the_plain_device_ball():
	ball = _ball(6)
	depths, _, states = _every_state(6)
	got_d, got_c = ball.child_depths(np.array(states))
	assert (got_d == depths).all()
	sub, _ = c_oracle.expand12(np.ascontiguousarray(states))
	want = DeviceGoalBall(6).depth(np.ascontiguousarray(sub, np.int8)).reshape(-1, 12)
	assert (want[depths < 6] >= 0).all() and (want[depths == 6] < 0).any()
	assert (got_c == np.where(want >= 0, want, 7)).all()


def test_repr686_gives_the_same_answers():
	ball = _ball(4)
	depths, ranks, states = _every_state(4)
	pick = np.random.default_rng(9).permutation(len(ranks))[:600]
	want_d, want_c = ball.child_depths(states[pick])
	try:
		cube.set_is2024(False)
		got = ball.state_at(depths[pick], ranks[pick])
		assert got.shape == (600, 6, 8, 6) and got.dtype == np.int8
		assert (got == cube.as686(states[pick])).all() and (cube.as2024(got) == states[pick]).all()
		s, d = ball.sample(50, 3, np.random.default_rng(2))
		assert s.shape == (50, 6, 8, 6) and (ball.depth(s) == 3).all()
		got_d, got_c = ball.child_depths(got)
		assert (got_d == want_d).all() and (got_c == want_c).all()
		assert ball.state_at(1, []).shape == (0, 6, 8, 6)
	finally:
		cube.set_is2024(True)
	assert (s == cube.as686(ball.sample(50, 3, np.random.default_rng(2))[0])).all()


@pytest.mark.parametrize("method", ["lapanfix", "reward0"])
def test_ball_traindata(method):
	ball, n, R = _ball(4), 4096, 4
	g = 0.0 if method == "reward0" else 1.0
	for depths in (np.arange(n) % 5, None):                              # every depth 1 / 5 of the rows (depth 0 included); the whole ball
		oh, policy, value, weights = ball_traindata(ball, n, depths, np.random.default_rng(21), method)
		states, d = ball.sample(n, depths, np.random.default_rng(21))
		assert oh.is_cuda and oh.dtype == torch.float32 and oh.shape == (n, 480)
		assert not policy.is_cuda and policy.dtype == torch.int64 and policy.shape == (n,)
		assert not value.is_cuda and value.dtype == torch.float32 and value.shape == (n,)
		assert not weights.is_cuda and weights.dtype == torch.float32 and (weights.numpy() == 1).all() and weights.shape == (n,)
		dev = torch.from_numpy(states).cuda()
		assert torch.equal(oh, cube.device.as_oh(dev)) and (oh.cpu().numpy() == orc.as_oh(states)).all()
		own, kids = model.child_depths(_lookup(5), states)
		assert (own == d).all() and (depths is None or (d == 0).sum() > 800)
		want_p, want_v = model.targets(own, kids, g)
		assert (policy.numpy() == want_p).all() and (value.numpy().view(np.uint32) == want_v.view(np.uint32)).all()
		assert (policy.numpy()[d == 0] == 0).all() and (value.numpy()[d == 0] == 0).all()
		# adi_traindata's own arithmetic on exact child values: values + rewards, argmax, the value at the argmax
		sub = cube.device.expand12(dev)[0].reshape(-1, 20)
		values, child_d, rows, _ = cube.device.ball_child_values(ball, sub, g)
		rewards = torch.where(child_d == 0, torch.tensor(g, device="cuda"), torch.tensor(-1.0, device="cuda"))
		both = (values + rewards).reshape(-1, 12)
		adi_p = torch.argmax(both, dim=1)
		adi_v = both[torch.arange(n, device="cuda"), adi_p]
		rows_in = (d >= 1) & (d <= R - 1)                                # all twelve children inside the ball
		assert rows_in.sum() > 50 and not np.isin(rows.cpu().numpy() // 12, np.nonzero(rows_in)[0]).any()
		assert (adi_p.cpu().numpy()[rows_in] == policy.numpy()[rows_in]).all()
		assert (adi_v.cpu().numpy()[rows_in] == value.numpy()[rows_in]).all()
	try:
		cube.set_is2024(False)
		oh686 = ball_traindata(ball, 64, 3, np.random.default_rng(4), method)
		s20 = torch.from_numpy(cube.as2024(ball.sample(64, 3, np.random.default_rng(4))[0])).cuda()
		assert oh686[0].shape == (64, 288) and torch.equal(oh686[0], cube.device.to686(s20, torch.float32))
	finally:
		cube.set_is2024(True)
	got = ball_traindata(ball, 64, 3, np.random.default_rng(4), method)
	assert torch.equal(got[1], oh686[1]) and torch.equal(got[2], oh686[2])
	with pytest.raises(TypeError):
		ball_traindata(DeviceGoalBall(2), 4)


def test_index_accounting_and_destroy_after_sampling():
	ball = DeviceSymBall(5)
	assert str(ball) == "Symmetry-reduced goal ball (device, radius=5)"
	ball.build()
	assert ball.index_builds == 0 and ball.index_bytes == 0 and ball.index_levels is None
	assert str(ball) == "Symmetry-reduced goal ball (device, radius=5)"
	first = ball.state_at(5, np.arange(100))
	assert ball.index_builds == 1 and (ball.index_levels == ball.states_covered).all()
	tiles = -(-len(ball) // 256)
	assert ball.index_bytes == 256 * tiles + 8 * (tiles + 1) and "orbit index" in str(ball)
	assert (ball.state_at(5, np.arange(100)) == first).all() and ball.sample(10)[0].shape == (10, 20)
	assert ball.index_builds == 1
	ball._free()                                                         # rk_symball_destroy with an index
	lib = _ffi.lib()
	h = C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(h), 3, 64, 0))
	_ffi.check(lib.rk_symball_build(h, 8, _ffi.stream_ptr()))
	d = torch.full((5,), 3, dtype=torch.int32, device="cuda")
	r = torch.arange(5, dtype=torch.int64, device="cuda")
	out = torch.empty((5, 20), dtype=torch.int8, device="cuda")
	err = torch.empty(1, dtype=torch.int32, device="cuda")
	assert lib.rk_symball_state_at(h, d.data_ptr(), r.data_ptr(), 5, out.data_ptr(), err.data_ptr(), _ffi.stream_ptr()) == 0
	torch.cuda.synchronize()
	assert lib.rk_symball_destroy(h) == 0
	other = DeviceSymBall(3, pops=7)                                     # another radius, other pops: the map does not depend on them
	want = sym_model.build(3)
	depths, ranks = _all_ranks(other.states_covered)
	got = other.state_at(depths, ranks)
	assert (got == model.state_at(want.states, want.level_start, depths, ranks)).all()
	assert (out.cpu().numpy() == got[depths == 3][:5]).all() and int(err.item()) == 0
