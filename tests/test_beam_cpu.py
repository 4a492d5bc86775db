"""
The beam-search model (tests/beam_model.py) on the oracle's cube arithmetic alone: its queues solve, a beam wide enough to keep
every state is optimal -- the anchor that does not depend on the model's own ranking --, the case list that the GPU test compares
bit for bit is not weak, and each of five planted defects changes at least one case.
"""
import numpy as np
import pytest

from oracle import cube_oracle as orc
from oracle.search_oracle import BFSOracle
from tests import beam_model as bm


def _bfs_distance(start) -> int:
	ref = BFSOracle()
	assert ref.search(start, 1_000_000)
	return len(ref.action_queue)


def _all_2024():
	return [bm.reference(c) for c in bm.CASES + bm.SOLVING_CASES]


def test_queues_solve():
	solved = 0
	for case in bm.CASES + bm.SOLVING_CASES:
		r = bm.reference(case)
		assert r.solved == (r.status == 1) and len(r.sizes) == len(r.back)
		if r.solved:
			solved += 1
			assert orc.is_solved(bm.apply(bm.start_of(case.seed, case.scramble), r.queue)), case
			assert len(r.queue) == r.depth
	for case in bm.BALL_CASES:
		r = bm.ball_reference(case)
		if r.solved:
			solved += 1
			assert orc.is_solved(bm.apply(bm.start_of(case[2], case[3]), r.queue)), case
			assert len(r.queue) == r.depth + r.meeting[2]
	assert solved >= 12


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_full_beam_is_optimal(depth):
	"""B >= 11 * 12^(d-1) keeps every state of every depth up to d, so the first win is a shortest solution, whatever the ranking."""
	values = bm.values_of(bm.net_of("lookup"))
	for seed in range(600, 606):
		start = bm.start_of(seed, depth)
		r = bm.search(values, start, 11 * 12 ** (depth - 1), max_depth=depth + 1)
		assert r.solved and len(r.queue) == _bfs_distance(start), (seed, depth)


@pytest.mark.parametrize("depth", [3, 4, 5])
def test_full_beam_to_the_ball_is_optimal(depth):
	"""The same to a radius-2 ball: length = distance to the ball + ball depth = the breadth-first distance."""
	ball = bm.ball_model(2)
	values = bm.values_of(bm.net_of("noisy"))
	for seed in range(610, 614):
		start = bm.start_of(seed, depth)
		dist = _bfs_distance(start)
		r = bm.search(values, start, 11 * 12 ** max(dist - 3, 0), max_depth=depth, ball=ball)
		assert r.solved and len(r.queue) == dist, (seed, depth)
		assert orc.is_solved(bm.apply(start, r.queue))
		if dist > 2:
			assert r.depth == dist - 2 and r.meeting[2] == 2


def test_case_list_is_not_weak():
	results = _all_2024()
	kinds = {k: sum(r.kinds[k] for r in results) for k in bm.KINDS}
	print(kinds, [r.status for r in results])
	for k in ("tie_cut", "duplicates", "nan_inf", "short_beam"):
		assert kinds[k] > 0, k
	assert {1, 2, 3} <= {r.status for r in results} | {bm.reference(c, max(bm.reference(c).explored - 1, 0)).status for c in bm.CASES[2::3]}
	assert sum(r.status == 1 and r.depth > 1 for r in results) >= 3              # beams that solve past the start's own children
	balls = [bm.ball_reference(c) for c in bm.BALL_CASES]
	assert balls[0].depth == 0 and balls[0].meeting[1] == -1                       # inside the ball at the reset
	assert sum(r.solved and r.depth >= 1 for r in balls) >= 3
	thin = [bm.thin_reference(c) for c in bm.THIN_CASES]
	assert sum(r.kinds["multi_hit"] for r in thin) > 0
	for c, r in zip(bm.THIN_CASES, thin):                                           # (the thinned ball's descents still find their way)
		assert r.solved and orc.is_solved(bm.apply(bm.thin_start(c[2]), r.queue))


def _differs(a: bm.Result, b: bm.Result) -> bool:
	if a.queue != b.queue or len(a.back) != len(b.back):
		return True
	return any(not np.array_equal(x, y) for x, y in zip(a.back[1:], b.back[1:]))


@pytest.mark.parametrize("defect", bm.DEFECTS)
def test_planted_defects_show(defect):
	if defect == "win_lowest_c":
		pairs = [(bm.thin_reference(c), bm.thin_reference(c, defect)) for c in bm.THIN_CASES]
	else:
		cases = [c for c in bm.CASES + bm.SOLVING_CASES if c.width <= 342]
		pairs = [(bm.reference(c), bm.reference(c, None, defect)) for c in cases]
	assert any(_differs(a, b) for a, b in pairs), defect
