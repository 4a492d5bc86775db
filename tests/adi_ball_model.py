"""
`adi_traindata(..., ball=DeviceSymBall(radius))` restated in NumPy -- TEST INFRASTRUCTURE, not imported by the product.

adi_ball_model is tests/adi_nets.adi_model with these differences:
  * the ball depth c of every child comes from the plain-Python symmetry ball (tests/sym_model.build(radius), sym_model.depth);
  * a child with c >= 0 gets, BEFORE the reward is added, V*(0) = 0.0, V*(c) = g - (c - 1) for 1 <= c <= radius in float32, with g
    the goal reward of the method (0.0 for reward0, 1.0 otherwise);
  * the net is called on the rows with c < 0 only, in ascending row order, in slices of ceil(count / ff) rows; with count = 0 it is
    not called at all.
Everything behind the children's values is adi_model's: + reward, first maximum, the lapanfix / schultzfix overrides.

One planted defect at a time (DEFECTS):
  vstar_off_by_one     V*(c) = g - c for c >= 1
  solved_as_deeper     c = 0 is treated as c >= 1: the solved child gets g + 1
  descending_outside   the outside STATES are compacted in descending row order while the row indices stay ascending (a compaction
                       that compacts states and indices in the same wrong order only permutes the net's batch; with nets whose answers
                       do not depend on the batch no target could tell)
  slices_of_all        the slices are cut from 12 n instead of count: fewer, longer net calls.  A net whose answer for a row does not
                       depend on its batch gives the same targets; the recorded calls differ, and so do the targets of a net that does
                       look at its batch (tests/test_adi_ball_cpu.py uses one for this defect)
  scatter_by_position  the net's answer for outside row number p goes to values[p] instead of values[rows[p]]; what no one wrote is 0

The child depths of a walk are computed once per (children, radius) and kept: sym_model.depth canonicalises in NumPy, about a second
for the 30 000 children of the largest case.
"""
import hashlib

import numpy as np
import torch

from oracle import cube_oracle as orc
from tests import sym_model

DEFECTS = ("vstar_off_by_one", "solved_as_deeper", "descending_outside", "slices_of_all", "scatter_by_position")
_BALLS, _DEPTHS = {}, {}


def ball_of(radius: int) -> sym_model.SymBall:
	if radius not in _BALLS:
		_BALLS[radius] = sym_model.build(radius)
	return _BALLS[radius]


def child_depths(sub: np.ndarray, radius: int) -> np.ndarray:
	"""int64 (len(sub),): the ball depth of every 20-byte row, -1 outside; distinct rows are canonicalised once"""
	sub = np.ascontiguousarray(sub, np.int8)
	key = (hashlib.sha1(sub.tobytes()).hexdigest(), radius)
	if key not in _DEPTHS:
		uniq, inverse = np.unique(sub, axis=0, return_inverse=True)
		d = np.concatenate([sym_model.depth(ball_of(radius), uniq[lo:lo + 4096]) for lo in range(0, len(uniq), 4096)])
		out = d[inverse.reshape(-1)].astype(np.int64)
		out.flags.writeable = False
		_DEPTHS[key] = out
	return _DEPTHS[key]


def goal_reward(method: str) -> float:
	return 0.0 if method == "reward0" else 1.0


def vstar(c: np.ndarray, g: float) -> np.ndarray:
	"""float32: 0 at c = 0, g - (c - 1) at c >= 1 (entries with c < 0 are meaningless)"""
	c = np.asarray(c, np.int64)
	return np.where(c == 0, np.float32(0), np.float32(g) - (c - 1).astype(np.float32)).astype(np.float32)


def ball_slices(count: int, ff: int):
	"""(lo, hi) of the net calls on `count` outside rows: step = ceil(count / ff)"""
	step = max(1, -(-count // max(1, ff)))
	return [(lo, min(lo + step, count)) for lo in range(0, count, step)]


def _walk686(games: int, depth: int, with_solved: bool, faces, dirs):
	cur = orc.repeat_state(orc.SOLVED686, games)
	seq = [cur] if with_solved else []
	for d in range(depth - int(with_solved)):
		cur = orc.multi_rotate686(cur, faces[d], dirs[d])
		seq.append(cur)
	return np.stack(seq, axis=1).reshape(games * depth, 6, 8, 6)


def adi_ball_model(net, games: int, depth: int, method: str, ff: int, radius: int, defect: str = None, repr686: bool = False, info: dict = None):
	"""
	-> (policy int64, value float32).  The caller seeds NumPy as for adi_traindata.  `net` takes a NumPy one-hot batch (the nets of
	tests/adi_nets.py); with `repr686` it is a torch module of the 6x8x6 representation, the walks are made in both representations
	with the same draws (as adi_nets.adi686_oracle makes them) and the net reads the 288-wide rows of the outside children.
	`info`, if given, receives: "calls" the rows of every net call in order, "count", "child_depth" (12 n,), "state_depth" (n,),
	"states" (n, 20), "rows" the outside rows, with `repr686` "states686" (n, 6, 8, 6).
	"""
	assert defect is None or defect in DEFECTS
	with_solved = method == "lapanfix"
	if repr686:
		faces = np.random.randint(0, 6, (depth, games))
		dirs = np.random.randint(0, 2, (depth, games))
		states = orc.sequence_states(faces, dirs, with_solved)
		f, d = orc.iter_actions(len(states))
		states686 = _walk686(games, depth, with_solved, faces, dirs)
		sub686 = orc.multi_rotate686(np.repeat(states686, 12, axis=0), f, d)
	else:
		states, _ = orc.sequence_scrambler(games, depth, with_solved)
	n = len(states)
	solved_scrambled = orc.multi_is_solved(states)
	sub = orc.expand12(states)
	solved_sub = orc.multi_is_solved(sub)
	g = goal_reward(method)
	rewards = np.where(solved_sub, g, -1.0).astype(np.float32)
	c = child_depths(sub, radius)
	inside = c >= 0
	exact = vstar(c, g)
	if defect == "vstar_off_by_one":
		exact = np.where(c == 0, np.float32(0), np.float32(g) - c.astype(np.float32)).astype(np.float32)
	elif defect == "solved_as_deeper":
		exact = (np.float32(g) - (c - 1).astype(np.float32)).astype(np.float32)
	values = np.zeros(12 * n, np.float32)
	values[inside] = exact[inside]
	rows = np.nonzero(~inside)[0]
	count = len(rows)
	batch = rows[::-1] if defect == "descending_outside" else rows
	cuts = ball_slices(12 * n, ff) if defect == "slices_of_all" else ball_slices(count, ff)
	calls = []
	for lo, hi in cuts:
		lo, hi = min(lo, count), min(hi, count)
		if hi == lo:
			continue
		if repr686:
			with torch.no_grad():
				v = net(torch.from_numpy(orc.as_oh686(sub686[batch[lo:hi]])), policy=False, value=True).reshape(-1).float().numpy()
		else:
			v = np.asarray(net(orc.as_oh(sub[batch[lo:hi]]), policy=False, value=True), np.float32).reshape(-1)
		calls.append(hi - lo)
		values[np.arange(lo, hi) if defect == "scatter_by_position" else rows[lo:hi]] = v
	with_reward = (values + rewards).reshape(-1, 12)
	policy = with_reward.argmax(axis=1)
	value = with_reward[np.arange(n), policy].copy()
	if method == "lapanfix":
		value[solved_scrambled] = 0
	elif method == "schultzfix":
		value[np.arange(0, n, depth)] = 0
	if info is not None:
		if repr686:
			info["states686"] = states686
		info.update(calls=calls, count=count, child_depth=c, state_depth=child_depths(states, radius), states=states, rows=rows)
	return policy.astype(np.int64), value.astype(np.float32)
