"""
The cube group on the device (engine rk_group_*, cube.apply_state / inverse / relative / is_legal, the balls' distance and path,
TowardsGoal) against the NumPy model of tests/group_model.py, bit for bit: one state, around a wave and a workgroup, and three rows
past a full pass of the capped grid; pairwise and one-for-all second operands; the output on top of an operand; the group identities
on the device; legality on a mix of legal rows, the 12 variants, out-of-range codes and repeated positions; the algebra on those
ill-formed rows (no fault, the legal rows beside them unaffected); both representations; both balls between pairs of states; two
agents towards a goal; and every entry on a side stream behind a gate.
"""
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch, DeviceSymBallSearchBatch, TowardsGoal
from tests import group_model as model
from tests import side_stream as S

pytestmark = pytest.mark.gpu

orc = model.orc
BASE = 4096
PAST_A_PASS = cube.device.GROUP_PASS_ROWS + 3
NS = (1, 2, 63, 64, 65, 255, 256, 257, PAST_A_PASS)


@functools.lru_cache(maxsize=None)
def _base():
	"""(a, b): BASE seeded scrambles each, 0..40 moves deep in turn (b the other way round), and what the model makes of them."""
	la, aa = model.word_actions(31_001, BASE)
	lb, ab = model.word_actions(31_002, BASE)
	a, b = model.states_of(model.full_actions(la, aa)), model.states_of(model.full_actions(lb[::-1].copy(), ab))
	for x in (a, b):                                                       # every (cubie, code) pair occurs: every table entry is read
		seen = np.zeros((20, 24), bool)
		seen[np.arange(20)[None, :], x] = True
		assert seen.all(), np.argwhere(~seen)
	want = {"apply": model.apply(a, b), "apply1": model.apply(a, b[5]), "inverse": model.inverse(a), "relative": model.relative(a, b),
	        "relative1": model.relative(a, b[5])}
	return a, b, want


def _rows(x: np.ndarray, n: int) -> np.ndarray:
	return x[np.arange(n) % BASE]


def _dev(x: np.ndarray) -> torch.Tensor:
	return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(op: str, a: torch.Tensor, b: torch.Tensor, out=None, check=False) -> torch.Tensor:
	if op == "inverse":
		return cube.device.inverse(a, out=out, check=check)
	f = cube.device.apply_state if op.startswith("apply") else cube.device.relative
	return f(a, b[5:6] if op.endswith("1") else b, out=out, check=check)


OPS = ("apply", "apply1", "inverse", "relative", "relative1")


@pytest.mark.parametrize("n", NS)
def test_algebra_equals_the_model(n):
	a, b, want = _base()
	da, db = _dev(_rows(a, n)), _dev(_rows(b, max(n, 6)))
	for op in OPS:
		second = db if op.endswith("1") else db[:n]
		got = S.sentinel((n, 20), torch.int8)
		assert _run(op, da, second, out=got) is got
		assert np.array_equal(got.cpu().numpy(), _rows(want[op], n)), op
	assert torch.equal(da, _dev(_rows(a, n))) and torch.equal(db, _dev(_rows(b, max(n, 6))))          # the operands are only read


@pytest.mark.parametrize("n", (1, 257, PAST_A_PASS))
def test_output_on_top_of_an_operand(n):
	a, b, want = _base()
	for op in OPS:
		da, db = _dev(_rows(a, n)), _dev(_rows(b, max(n, 6)))
		second = db if op.endswith("1") else db[:n]
		assert _run(op, da, second, out=da) is da and np.array_equal(da.cpu().numpy(), _rows(want[op], n)), op
	for op in ("apply", "relative"):                                       # ... and on top of the second operand, one for each state
		da, db = _dev(_rows(a, n)), _dev(_rows(b, n))
		_run(op, da, db, out=db)
		assert np.array_equal(db.cpu().numpy(), _rows(want[op], n)), op
	lib, (da, db) = _ffi.lib(), (_dev(a[:8]), _dev(b[:8]))
	assert lib.rk_group_apply(da.data_ptr(), 4, db.data_ptr(), 4, da.data_ptr() + 20, None) == -1 and b"overlaps" in lib.rk_last_error()
	assert lib.rk_group_relative(da.data_ptr(), 4, db.data_ptr(), 1, db.data_ptr(), None) == -1 and b"overlaps" in lib.rk_last_error()


def test_group_identities_on_the_device():
	a, b, _ = _base()
	da, db = _dev(a), _dev(b)
	dc = _dev(a[::-1].copy())
	solved = _dev(orc.repeat_state(orc.SOLVED, BASE))
	ap, inv, rel = cube.device.apply_state, cube.device.inverse, cube.device.relative
	assert torch.equal(ap(da, inv(da)), solved) and torch.equal(ap(inv(da), da), solved) and torch.equal(inv(inv(da)), da)
	assert torch.equal(ap(ap(da, db), dc), ap(da, ap(db, dc)))               # associative
	assert torch.equal(rel(da, da), solved) and torch.equal(rel(da, solved[:1]), da)
	assert torch.equal(rel(da, db), ap(inv(db), da))
	for m in range(12):
		acts = torch.full((BASE,), m, dtype=torch.uint8, device="cuda")
		one = _dev(orc.rotate(orc.SOLVED, m // 2, 1 - m % 2)[None])
		moved = cube.device.multi_rotate(da, acts)
		assert torch.equal(ap(da, one), moved), m
		assert torch.equal(rel(moved, db), cube.device.multi_rotate(rel(da, db), acts)), m


def _mixed(n: int) -> np.ndarray:
	"""n rows: legal scrambles, the 12 variants of some, out-of-range codes (24, 127, -1, -128, 31) and repeated positions, interleaved."""
	a = _base()[0]
	x = a[100:100 + n].copy()
	rs = np.random.RandomState(4242 + n)
	for i in range(n):
		kind = i % 6
		if kind == 1:
			x[i] = model.variants(x[i])[1 + (i // 6) % 11]
		elif kind == 3:
			x[i, rs.randint(20)] = (24, 127, -1, -128, 31)[(i // 6) % 5]
		elif kind == 5:
			at = rs.randint(19)
			at -= at == 7                                                    # bytes at and at + 1 of one kind
			x[i, at + 1] = x[i, at] ^ ((i // 6) % 2 if at >= 8 else 0)
	return x


def _legal(x: np.ndarray):
	d = _dev(x)
	stats = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")
	flags = cube.device.is_legal(d, stats=stats)
	return flags.cpu().numpy(), stats.tolist()


@pytest.mark.parametrize("n", (1, 65, 257))
def test_legal_equals_the_model(n):
	for x in (_mixed(n), _mixed(n + 1)[1:]):
		want = model.is_legal(x)
		flags, stats = _legal(x)
		assert flags.dtype == np.uint8 and np.array_equal(flags.astype(bool), want)
		bad = np.nonzero(~want)[0]
		assert stats == [len(bad), bad[0] if len(bad) else _ffi.INT64_MAX]
		assert np.array_equal(cube.is_legal(x), want)
	assert n == 1 or 0 < (~model.is_legal(_mixed(n))).sum() < n


def test_legal_none_and_last():
	a = _base()[0][:257].copy()
	flags, stats = _legal(a)
	assert flags.all() and stats == [0, _ffi.INT64_MAX]
	for x in model.variants(a[256])[1:]:
		a[256] = x
		flags, stats = _legal(a)
		assert flags[:256].all() and not flags[256] and stats == [1, 256]
	# past a pass of the grid: a thread's second row, and the count of many
	big = _rows(_base()[1], PAST_A_PASS).copy()
	big[::1000, 3] = 24
	big[-1, 8] ^= 1
	flags, stats = _legal(big)
	want = np.ones(PAST_A_PASS, bool)
	want[::1000] = want[-1] = False
	assert np.array_equal(flags.astype(bool), want) and stats == [int((~want).sum()), 0]
	stats_only = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")
	rest = _dev(big[1:])
	_ffi.check(_ffi.lib().rk_group_legal(rest.data_ptr(), PAST_A_PASS - 1, None, stats_only.data_ptr(), _ffi.stream_ptr()))
	assert stats_only.tolist() == [int((~want).sum()) - 1, 999]


def test_ill_formed_rows_leave_the_others_alone():
	x, y = _mixed(257), _mixed(259)[2:]
	ok = model.is_legal(x) & model.is_legal(y)
	assert 20 < ok.sum() < 200
	junk = np.random.RandomState(9).randint(-128, 128, (257, 20)).astype(np.int8)
	keep = np.arange(257) % 3 == 0
	z = np.where(keep[:, None], _base()[0][:257], junk)
	for p, q, legal in ((x, y, ok), (z, np.roll(z, 3, axis=0), keep & np.roll(keep, 3))):
		dp, dq = _dev(p), _dev(q)
		for op, f in (("apply", model.apply), ("relative", model.relative), ("inverse", None)):
			got = _run(op, dp, dq).cpu().numpy()
			want = model.inverse(p[legal]) if f is None else f(p[legal], q[legal])
			assert np.array_equal(got[legal], want), op
		for op, f in (("apply1", model.apply), ("relative1", model.relative)):
			one = _base()[1]
			assert np.array_equal(_run(op, dp, _dev(one)).cpu().numpy()[legal], f(p[legal], one[5])), op
	torch.cuda.synchronize()


def test_both_representations_and_check(monkeypatch):
	a, b, want = _base()
	a, b = a[:65], b[:65]
	for is2024 in (True, False):
		cube.set_is2024(is2024)
		give = (lambda x: x) if is2024 else cube.as686
		shape = (65, 20) if is2024 else (65, 6, 8, 6)
		for got, key in ((cube.apply_state(give(a), give(b)), "apply"), (cube.apply_state(give(a), give(b[5])), "apply1"),
		                 (cube.inverse(give(a)), "inverse"), (cube.relative(give(a), give(b)), "relative"),
		                 (cube.relative(give(a), give(b[5:6])), "relative1")):
			assert got.shape == shape and got.dtype == np.int8 and np.array_equal(got, give(want[key][:65])), (is2024, key)
		assert cube.is_legal(give(a)).all() and cube.is_legal(give(a)).shape == (65,)
		assert cube.apply_state(give(a)[:0], give(b[5])).shape == (0,) + shape[1:]
	cube.set_is2024(False)
	twisted = cube.as686(model.variants(a[3])[4:5])                        # a well-formed 6x8x6 cube with a twisted corner
	assert cube.is_legal(twisted).tolist() == [False]
	broken = cube.as686(a[:3]).copy()
	broken[1, 0, 0] = 0
	assert cube.is_legal(broken).tolist() == [True, False, True]
	cube.set_is2024(True)
	bad = a.copy()
	bad[[7, 30]] = model.variants(a[7])[[2, 9]]
	for use in (lambda c: cube.apply_state(bad, b, check=c), lambda c: cube.apply_state(a, bad, check=c), lambda c: cube.inverse(bad, check=c),
	            lambda c: cube.relative(bad, b[:1], check=c), lambda c: cube.relative(a, bad, check=c)):
		with pytest.raises(ValueError, match=r"2 of 65 rows .* \(the first is row 7\)"):
			use(True)
	with pytest.raises(ValueError, match=r"1 of 1 rows of goal .* \(the first is row 0\)"):
		cube.relative(a, bad[7], check=True)
	calls = []
	lib, legal = _ffi.lib(), _ffi.lib().rk_group_legal
	monkeypatch.setattr(lib, "rk_group_legal", lambda *args: calls.append(args) or legal(*args))
	cube.apply_state(a, b)
	assert len(calls) == 2
	cube.apply_state(bad, b, check=False), cube.inverse(bad, check=False), cube.relative(a, bad, check=False)
	assert len(calls) == 2                                                 # check=False launches no check


@pytest.fixture(scope="module", params=[DeviceSymBall, DeviceGoalBall])
def ball(request):
	return request.param(5).build()


@functools.lru_cache(maxsize=None)
def _pairs():
	"""a: 96 scrambles of 30 moves; b: a moved along a word of 0..7 moves; the words' own states."""
	a = S.scrambles(96, 30, 601)
	lengths, actions = model.word_actions(602, 96, 7)
	b, w = a.copy(), orc.repeat_state(orc.SOLVED, 96)
	for t in range(7):
		live = (lengths > t)[:, None]
		f, d = actions[:, t] // 2, 1 - actions[:, t] % 2
		b, w = np.where(live, orc.multi_rotate(b, f, d), b), np.where(live, orc.multi_rotate(w, f, d), w)
	return a, b, w


def _walk(states: np.ndarray, lengths: np.ndarray, actions: np.ndarray) -> np.ndarray:
	s = states.copy()
	for t in range(actions.shape[1]):
		live = (lengths > t)[:, None]
		act = np.where(lengths > t, actions[:, t], 0)
		s = np.where(live, orc.multi_rotate(s, act // 2, 1 - act % 2), s)
	return s


def test_balls_between_pairs(ball):
	a, b, w = _pairs()
	depth = ball.depth(w)
	assert (depth >= 0).sum() > 40 and (depth < 0).sum() > 5 and depth.max() == 5
	d = ball.distance(a, b)
	assert d.dtype == np.int64 and np.array_equal(d, depth) and np.array_equal(ball.distance(b, a), depth)
	assert np.array_equal(ball.depth(cube.inverse(w)), depth)
	assert np.array_equal(ball.distance(a, a), np.zeros(96, np.int64)) and ball.distance(a, a[0]).tolist()[0] == 0
	assert np.array_equal(ball.distance(a, b[0]), ball.depth(cube.relative(a, b[0])))
	lengths, actions = ball.path(a, b)
	assert actions.shape == (96, 5) and np.array_equal(lengths, depth)
	inside = depth >= 0
	assert np.array_equal(_walk(a[inside], lengths[inside], actions[inside]), b[inside])
	assert ball.distance(a[:0], b[:0]).shape == (0,) and ball.path(a[:0], b[0])[1].shape == (0, 5)
	with pytest.raises(ValueError, match="the first is row 2"):
		ball.distance(model.variants(a[0])[:5][[0, 0, 3, 0, 4]], b[:5])
	if isinstance(ball, DeviceSymBall):
		rel = cube.relative(a, b)
		want_len, want_act = ball.solve_beyond(rel, 2)
		far = ball.distance(a, b, extra=2)
		assert np.array_equal(far, want_len) and (far >= 0).all() and far.max() >= 6 and np.array_equal(far[inside], depth[inside])
		lengths, actions = ball.path(a, b, extra=2)
		assert actions.shape == (96, 7) and np.array_equal(lengths, want_len) and np.array_equal(actions, want_act)
		assert np.array_equal(_walk(a, lengths, actions), b)


def test_towards_goal():
	ball = DeviceSymBall(5).build()
	goal = S.scrambles(1, 30, 701)[0]
	lengths, actions = model.word_actions(702, 16, 9)
	lengths = 6 + np.arange(16) % 4
	starts = _walk(orc.repeat_state(goal, 16), lengths, actions)
	rel = cube.relative(starts, goal)
	one, own = TowardsGoal(DeviceSymBallSearch(ball), goal), DeviceSymBallSearch(ball)
	for i in range(16):
		assert one.search(starts[i]) and own.search(rel[i])
		queue = np.array(one.action_queue, np.int64)
		assert len(queue) == len(own.action_queue) <= lengths[i] and len(one) == len(own)
		assert np.array_equal(_walk(starts[i:i + 1], np.array([len(queue)]), queue[None]), goal[None])
	many, alone = TowardsGoal(DeviceSymBallSearchBatch(ball, searches=8), goal), DeviceSymBallSearchBatch(ball, searches=8)
	assert many.search(starts).all() and alone.search(rel).all()
	assert np.array_equal(many.lengths, alone.lengths) and len(many) == len(alone)
	for i in range(16):
		queue = np.array(many.action_queue_of(i), np.int64)
		assert len(queue) == many.lengths[i] and np.array_equal(_walk(starts[i:i + 1], np.array([len(queue)]), queue[None]), goal[None])
	cube.set_is2024(False)
	assert one.search(cube.as686(starts[3])) and np.array_equal(one.goal, cube.as686(goal))
	cube.set_is2024(True)
	with pytest.raises(ValueError, match="goal"):
		TowardsGoal(own, model.variants(goal)[6])
	with pytest.raises(ValueError, match="the first is row 0"):
		one.search(model.variants(starts[0])[1])


@pytest.mark.parametrize("n", (257, 1000))
def test_entries_on_a_side_stream(n):
	a, b, _ = _base()
	true_a, true_b = _dev(a[:n]), _dev(b[:n])
	decoy_a, decoy_b = _dev(a[n:2 * n]), _dev(b[n:2 * n])
	mixed = _dev(_mixed(n))
	lib = _ffi.lib()

	def launch(op, x, y, out):
		if op == "legal":
			flags, stats = out
			_ffi.check(lib.rk_group_legal(x.data_ptr(), n, flags.data_ptr(), stats.data_ptr(), _ffi.stream_ptr()))
		elif op == "inverse":
			_ffi.check(lib.rk_group_inverse(x.data_ptr(), n, out.data_ptr(), _ffi.stream_ptr()))
		else:
			f = lib.rk_group_apply if op.startswith("apply") else lib.rk_group_relative
			_ffi.check(f(x.data_ptr(), n, y.data_ptr(), 1 if op.endswith("1") else n, out.data_ptr(), _ffi.stream_ptr()))
	for op in OPS + ("legal",):
		tx = mixed if op == "legal" else true_a
		if op == "legal":
			want = (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda"))
			got = (S.sentinel((n,), torch.uint8), torch.tensor([5, 3], dtype=torch.int64, device="cuda"))
			init = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")
		else:
			want, got = torch.empty((n, 20), dtype=torch.int8, device="cuda"), S.sentinel((n, 20), torch.int8)
		launch(op, tx, true_b, want)
		bx, by = decoy_a.clone(), decoy_b.clone()
		torch.cuda.synchronize()
		s = S.side_stream()
		with torch.cuda.stream(s):
			ev = S.gate(s)
			bx.copy_(tx, non_blocking=True)
			by.copy_(true_b, non_blocking=True)
			if op == "legal":
				got[1].copy_(init, non_blocking=True)
			launch(op, bx, by, got)
			S.held(ev)
			s.synchronize()
		if op == "legal":
			assert S.same_bits(got[0], want[0]) and got[1].tolist() == want[1].tolist() and want[1].tolist()[0] > 0, op
		else:
			assert S.same_bits(got, want), op
