"""
The CPU half of the tests of `adi_traindata(..., ball=DeviceSymBall(R))` (tests/test_adi_ball_gpu.py holds the GPU half): the model
(tests/adi_ball_model.py) alone, no GPU anywhere.
  * Exactness: every state whose own depth d satisfies 1 <= d <= R - 1 has the value target V*(d) exactly and the lowest action whose
    child lies one level nearer as its policy target, whatever the net -- for every case, with lapanfix, paper and reward0.
  * Consistency: a net whose answers on the ball's states are V* itself makes plain adi_model give the ball model's targets.
  * The cases are not weak: in every main case the ball answers between 10 % and 90 % of the children and a state has both kinds among
    its twelve children; a case has no outside child at all; a case's last net call is a single row.  The figures are printed.
  * Each planted defect changes at least one target bit in at least one case.
  * The engine's argument checks that need no device.
"""
import ctypes as C

import numpy as np
import pytest

from librubiks_amd import _ffi
from oracle import cube_oracle as orc
from tests.adi_ball_model import DEFECTS, adi_ball_model, ball_slices, child_depths, goal_reward, vstar
from tests.adi_nets import adi_model, net_of
from tests.test_adi_real_valued_cpu import bits

# (net, seed, games, depth, method, ff_batches, radius).  12 n children; the net sees only those outside the ball.
#   37 x 9, ff 7     3 996 children: steps that cut through a state's twelve children
#   64 x 5           3 840 children: whole tiles of 256 rows
#   100 x 25, ff 7   30 000 children: more rows than the fixed grid has waves (8 192), 118 scan tiles
#   5 x 5, ff 24     300 children; seeds 441 and 443: the last of the slices of 4 (6) rows is a single row
#   3 x 2, ff 50     72 children, more slices asked for than there are outside rows
LOOKUP_MAIN = [
	("lookup", 401, 37, 9, "lapanfix", 7, 3), ("lookup", 402, 37, 9, "paper", 7, 5), ("lookup", 403, 37, 9, "schultzfix", 7, 3),
	("lookup", 404, 37, 9, "reward0", 7, 5), ("lookup_bf16", 405, 64, 5, "lapanfix", 5, 1), ("lookup_bf16", 406, 64, 5, "reward0", 7, 3),
	("lookup_special", 407, 100, 25, "paper", 7, 5), ("lookup", 441, 5, 5, "lapanfix", 24, 3), ("lookup", 409, 3, 2, "lapanfix", 50, 1),
]
#: the edges: no outside child at all (one solved state: twelve children at depth 1), radius 0 (the ball is the solved state), radius 1
LOOKUP_EDGE = [
	("lookup", 410, 1, 1, "lapanfix", 1, 1), ("lookup", 411, 1, 1, "paper", 1, 0), ("lookup", 412, 37, 9, "paper", 7, 0),
	("lookup_special", 413, 37, 9, "lapanfix", 7, 1), ("lookup", 414, 1, 1, "lapanfix", 1, 5),
]
LINEAR_MAIN = [
	("linear", 421, 37, 9, "lapanfix", 7, 3), ("linear", 422, 64, 5, "paper", 5, 3), ("linear", 443, 5, 5, "schultzfix", 24, 3),
	("linear", 425, 3, 2, "lapanfix", 50, 1), ("linear_bf16", 431, 37, 9, "lapanfix", 7, 5), ("linear_bf16", 432, 64, 5, "reward0", 5, 3),
	("linear_bf16", 433, 100, 25, "lapanfix", 7, 5), ("linear_bf16", 435, 5, 5, "lapanfix", 24, 1),
]
LINEAR_EDGE = [("linear", 424, 1, 1, "lapanfix", 1, 5), ("linear_bf16", 434, 1, 1, "paper", 1, 0)]
LOOKUP_CASES, LINEAR_CASES = LOOKUP_MAIN + LOOKUP_EDGE, LINEAR_MAIN + LINEAR_EDGE
MAIN, CASES = LOOKUP_MAIN + LINEAR_MAIN, LOOKUP_CASES + LINEAR_CASES
_MODEL = {}


def case_id(case) -> str:
	return "-".join(str(x) for x in case)


def model_of(case):
	"""the model's targets of an input tuple, made once and left unchanged -> (policy, value, info)"""
	if case not in _MODEL:
		name, seed, games, depth, method, ff, radius = case
		info = {}
		np.random.seed(seed)
		policy, value = adi_ball_model(net_of(name), games, depth, method, ff, radius, info=info)
		for a in (policy, value):
			a.flags.writeable = False
		_MODEL[case] = (policy, value, info)
	return _MODEL[case]


def test_cases_cover_what_they_say():
	assert {c[6] for c in CASES} == {0, 1, 3, 5} and {c[0] for c in LOOKUP_CASES} == {"lookup", "lookup_bf16", "lookup_special"}
	assert {c[0] for c in LINEAR_CASES} == {"linear", "linear_bf16"}
	assert {(c[2], c[3]) for c in CASES} == {(1, 1), (3, 2), (5, 5), (37, 9), (64, 5), (100, 25)}
	assert len({c[1] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exact_targets_inside_the_ball(case):
	"""1 <= d <= R - 1: all twelve children lie in the ball, so no answer of the net reaches the target."""
	name, seed, games, depth, _, ff, radius = case
	checked = 0
	for method in ("lapanfix", "paper", "reward0"):
		info = {}
		np.random.seed(seed)
		policy, value = adi_ball_model(net_of(name), games, depth, method, ff, radius, info=info)
		d, c = info["state_depth"], info["child_depth"].reshape(-1, 12)
		rows = np.nonzero((d >= 1) & (d <= radius - 1))[0]
		if not len(rows):
			continue
		assert (c[rows] >= 0).all()
		nearer = c[rows] == (d[rows] - 1)[:, None]
		assert nearer.any(axis=1).all()
		assert (policy[rows] == nearer.argmax(axis=1)).all(), (case, method)
		assert (bits(value[rows]) == bits(vstar(d[rows], goal_reward(method)))).all(), (case, method)
		checked += len(rows)
	assert checked > 0 or radius < 2 or games * depth == 1, case
	if case in MAIN and radius >= 3:
		assert checked >= 3


class _ExactOnBall:
	"""`net`, except that a row whose state the ball holds gets V* itself"""
	def __init__(self, net, radius: int, g: float):
		self.net, self.radius, self.g = net, radius, g

	def __call__(self, x, policy=False, value=True):
		assert value and not policy
		v = np.asarray(self.net(x, policy=False, value=True), np.float32).reshape(-1).copy()
		c = child_depths(np.asarray(x).reshape(len(x), 20, 24).argmax(axis=2).astype(np.int8), self.radius)
		v[c >= 0] = vstar(c, self.g)[c >= 0]
		return v.reshape(-1, 1)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_consistent_with_the_plain_model(case):
	name, seed, games, depth, method, ff, radius = case
	policy, value, _ = model_of(case)
	np.random.seed(seed)
	p2, v2 = adi_model(_ExactOnBall(net_of(name), radius, goal_reward(method)), games, depth, method, ff)
	assert (policy == p2).all() and (bits(value) == bits(v2)).all()


def test_cases_are_not_weak():
	count0 = single = 0
	for case in CASES:
		_, _, games, depth, _, ff, _ = case
		_, _, info = model_of(case)
		m12, count = 12 * games * depth, info["count"]
		share = 1 - count / m12
		inside = (info["child_depth"] >= 0).reshape(-1, 12).sum(axis=1)
		mixed = int(((inside > 0) & (inside < 12)).sum())
		cuts = ball_slices(count, ff)
		assert info["calls"] == [hi - lo for lo, hi in cuts]
		print(f"{case_id(case)}: the ball answers {m12 - count} of {m12} children ({share:.1%}), {mixed} states with both kinds, {len(cuts)} net calls"
		      + (f", the last of {cuts[-1][1] - cuts[-1][0]}" if cuts else ""))
		if case in MAIN:
			assert 0.1 <= share <= 0.9, case
			assert mixed >= 1, case
		count0 += count == 0
		single += len(cuts) > 1 and cuts[0][1] - cuts[0][0] > 1 and cuts[-1][1] - cuts[-1][0] == 1
	assert count0 >= 1 and single >= 2
	assert model_of(("lookup", 410, 1, 1, "lapanfix", 1, 1))[2]["count"] == 0
	_, _, info = model_of(("lookup", 409, 3, 2, "lapanfix", 50, 1))
	assert 0 < info["count"] < 50                                        # more slices asked for than there are outside rows


class _SeesItsBatch:
	"""a net that is NOT independent of its batch: every answer has the number of rows of the call added (slices_of_all shows only so)"""
	def __init__(self, net):
		self.net = net

	def __call__(self, x, policy=False, value=True):
		return np.asarray(self.net(x, policy=False, value=True), np.float32) + np.float32(len(x))


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_planted_defect_changes_a_target(defect):
	caught = []
	for case in MAIN:
		name, seed, games, depth, method, ff, radius = case
		if games * depth > 400 and len(caught) >= 2:
			continue
		net = net_of(name)
		if defect == "slices_of_all":
			net = _SeesItsBatch(net)
			np.random.seed(seed)
			policy, value = adi_ball_model(net, games, depth, method, ff, radius)
		else:
			policy, value, _ = model_of(case)
		info = {}
		np.random.seed(seed)
		p2, v2 = adi_ball_model(net, games, depth, method, ff, radius, defect=defect, info=info)
		if (policy != p2).any() or (bits(value) != bits(v2)).any():
			caught.append(case_id(case))
		if defect == "slices_of_all" and info["count"] and ff > 1:
			assert info["calls"] != model_of(case)[2]["calls"]              # what the GPU tests compare the recorded calls with
	print(f"{defect}: caught by {caught}")
	assert caught, defect


def test_engine_argument_checks_need_no_device():
	lib = _ffi.lib()
	assert [lib.rk_symball_child_values_scratch_bytes(m) for m in (0, 12, 256, 264, 30000)] == [0, 4, 4, 8, 4 * 118]
	assert lib.rk_symball_child_values_scratch_bytes(1 << 31) == -1
	buf = np.zeros(64, np.int64)
	p = buf.ctypes.data
	assert lib.rk_symball_child_values(None, p, 12, 1.0, p, p, p, p, p, p, 8, None) == -1 and b"null ball" in lib.rk_last_error()
	h = C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(h), 2, 16, 0))
	try:
		assert lib.rk_symball_child_values(h, p, 12, 1.0, p, p, p, p, p, p, 8, None) == -4 and b"build the ball first" in lib.rk_last_error()
	finally:
		assert lib.rk_symball_destroy(h) == 0


def test_python_surface_refuses_other_balls_before_anything_else():
	from librubiks_amd.adi import adi_traindata
	from librubiks_amd import cube
	from librubiks_amd.solving.agents import DeviceGoalBall
	for ball in (DeviceGoalBall(2), 3):
		with pytest.raises(TypeError, match="DeviceSymBall"):
			adi_traindata(None, 1, 1, 0.5, "lapanfix", ball=ball)
		with pytest.raises(TypeError, match="DeviceSymBall"):
			cube.device.ball_child_values(ball, None, 1.0)
