"""
The yardstick of tests/test_symsample_gpu.py pinned on the host: the unranking model (tests/symsample_model.state_at) over the model
symmetry ball of radius 4 gives, for all ranks of level d, exactly the level-d states of the plain model ball -- 1 / 12 / 114 /
1 068 / 10 011 of them, none twice -- and the model's child depths and targets are what their definitions say on states whose
answers are known by hand.
"""
import numpy as np

from oracle import cube_oracle as orc
from tests import ball_model, sym_model, symsample_model as model

LEVELS = (1, 12, 114, 1_068, 10_011)


def _rows(a: np.ndarray) -> set:
	return {r.tobytes() for r in np.ascontiguousarray(a, np.int8).reshape(-1, 20)}


def test_every_rank_of_every_level_is_the_plain_balls_level():
	sym, plain = sym_model.build(4), ball_model.build(4)
	assert tuple(model.level_sizes(sym.states, sym.level_start)) == LEVELS == tuple(sym.covered)
	_, first = model.orbits(sym.states)
	assert sym.len == 251 and (first.sum(axis=0) < 48).sum() == 29 and first[0].all()      # 29 orbits with a stabiliser
	for d, size in enumerate(LEVELS):
		got = model.state_at(sym.states, sym.level_start, d, np.arange(size))
		want = plain.states[plain.level_start[d] - 1:plain.level_start[d + 1] - 1]
		assert got.shape == (size, 20) and got.dtype == np.int8
		assert len(_rows(got)) == size and _rows(got) == _rows(want), d
	# rank 0 of a level is its first node's representative itself (symmetry 0 is always a first one); depths may be mixed
	d = np.array([4, 0, 2, 4, 1])
	r = np.array([0, 0, 113, 10_010, 5])
	got = model.state_at(sym.states, sym.level_start, d, r)
	assert (got[0] == sym.states[sym.level_start[4] - 1]).all() and (got[1] == orc.SOLVED).all()
	for i in range(5):
		assert (got[i] == model.state_at(sym.states, sym.level_start, int(d[i]), r[i:i + 1])[0]).all()
		assert ball_model.depth(plain, got[i]) == d[i]


def test_child_depths_and_targets_of_the_model():
	plain = ball_model.build(3)
	lookup = {k: ball_model.depth_of(plain, v) for k, v in plain.index.items()}
	one = orc.rotate(orc.SOLVED, 2, 1)
	two = orc.rotate(one, 4, 0)
	far = ball_model.scramble(5, 20)
	own, kids = model.child_depths(lookup, np.stack([orc.SOLVED, one, two, far]))
	assert own.tolist()[:3] == [0, 1, 2] and (kids[0] == 1).all()
	assert sorted(kids[1].tolist()) == [0] + [2] * 11 and sorted(kids[2].tolist()) == [1] + [3] * 11
	assert own[3] == -1 and (kids[3] == -1).all()
	policy, value = model.targets(own[:3], kids[:3], 1.0)
	assert policy[0] == 0 and kids[1, policy[1]] == 0 and kids[2, policy[2]] == 1
	assert value.dtype == np.float32 and value.tolist() == [0.0, 1.0, 0.0]
	assert model.targets(own[:3], kids[:3], 0.0)[1].tolist() == [0.0, 0.0, -1.0]
