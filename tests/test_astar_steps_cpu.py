"""
The inputs of tests/test_astar_steps_gpu.py, checked on the model alone: the schedule that tests/astar_steps_model.py drives -- the pop
count and the values of every iteration -- is not a weak one.  The engine has to equal the model bit for bit, so what the schedule
reaches here is what the GPU run reaches.
"""
import functools

import numpy as np
import pytest

from tests import astar_steps_model as sm

CASES = [(gi, bf16) for gi in range(len(sm.GEOMETRIES)) for bf16 in (False, True)]
IDS = [f"N{sm.GEOMETRIES[gi].N}-{'bf16' if bf16 else 'f32'}" for gi, bf16 in CASES]


@functools.lru_cache(maxsize=None)
def schedule(gi, bf16):
	return sm.run(sm.GEOMETRIES[gi], bf16)


def test_geometry_table_sits_on_the_switches():
	"""what the table of geometries claims about the engine's forms, from the restated constants"""
	form = {g.N: sm.sort_geometry(g.N) for g in sm.GEOMETRIES}
	assert form[21][:3] == (252, 256, 256) and form[22][:3] == (264, 256, 512)
	assert form[170] == (2040, 256, 2048, "runs of 256") and form[171] == (2052, 2048, 4096, "chunks as they are")
	assert form[1365] == (16380, 2048, 16384, "chunks as they are") and form[1366] == (16392, 2048, 18432, "merge passes")
	levels = {g.N: len(sm.queue_plan(g.N, g.capacity)) for g in sm.GEOMETRIES}
	assert levels[2048] == levels[2049] == 3 and levels[2048] * 2048 == sm.POP_LDS and levels[2049] * 2049 == sm.POP_LDS + 3
	assert sm.queue_plan(1, 6000) == [4096, 6001] and sm.queue_plan(3, 9000) == [4096, 9001]
	assert sm.queue_plan(170, 200_000) == [8160, 32640, 130560, 200001]
	assert sm.targets(1365)[0] == [0, 1, 127, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 16380, 16383]
	assert sm.targets(170)[1] == [0, 1, 127, 128, 129, 255, 256, 257, 512, 513] and sm.targets(1)[1] == [0, 1, 12]


@pytest.mark.parametrize("gi,bf16", CASES, ids=IDS)
def test_schedule_is_not_weak(gi, bf16):
	g = sm.GEOMETRIES[gi]
	m, log = schedule(gi, bf16)
	c = sm.coverage(g, log)
	print(f"N = {g.N} {'bf16' if bf16 else 'f32'}: {c['iterations']} iterations, {len(m)} states, n_new hit {c['hit']}, missed {c['missed']}, "
	      f"n_expand: {c['distinct']} values, {c['changes']} changes, {c['repeats']} repeats; {m.G.lowered} relaxations")
	assert not m.won and all(r.step.popped for r in log), "the schedule neither wins nor ends on the loop guard"
	assert len(c["missed"]) <= 2, f"N = {g.N}: n_new targets missed: {c['missed']} (hit: {c['hit']})"
	# (an engine with N < 5 has no five pop counts to offer; one with N = 1 none to change between)
	n_exp = [r.n_expand for r in log]
	assert c["distinct"] >= min(5, g.N) and c["repeats"] >= 3 and (g.N == 1 or c["changes"] >= 10), c
	assert g.N in n_exp[1:] and (g.N == 1 or 1 in n_exp)
	back = [i for i in range(1, len(n_exp)) if n_exp[i] == g.N and n_exp[i - 1] != g.N]
	away = [i for i in range(1, len(n_exp)) if n_exp[i] != g.N and n_exp[i - 1] == g.N]
	assert g.N == 1 or (len(back) >= 3 and len(away) >= 3), "n_expand returns to N and leaves it again, several times"
	assert c["patterns"] == sorted(sm.PATTERNS)
	assert m.G.lowered > 0, "no relaxation"
	cost, idx = m.open_sorted()
	assert (cost < 0).any() and (cost >= 0).any() and len(np.unique(cost)) < len(cost)
	assert len(m) + 12 * g.N <= g.capacity, "the pool and the budget leave room: the loop guard is not what ends the run"
	if g.N <= 3:
		assert max(r.step.level for r in log) == len(m.caps) - 1 >= 1, "the pushes did not reach the top queue level"
	if g.N >= 1365:
		assert len(m) < 1_000_000 and sum(1 for s in m.levels if s) >= 2, "two queue levels hold records at the end"


def test_values_are_what_they_say():
	rng = np.random.RandomState(5)
	G = np.arange(3000, dtype=np.float64) % 23
	for bf16 in (False, True):
		for p in sm.PATTERNS:
			v = sm.make_values(p, G, 0.5, rng, bf16)
			assert v.dtype == np.float32 and len(v) == len(G) and not np.isnan(v).any()
			assert not bf16 or not (v.view(np.uint32) & 0xFFFF).any(), "bfloat16 holds every value of its leg exactly"
			assert len(sm.make_values(p, G[:0], 0.5, rng, bf16)) == 0 and len(sm.make_values(p, G[:1], 0.5, rng, bf16)) == 1
		asc, desc = (sm.make_values(p, G, 0.5, rng, bf16) for p in ("ascending", "descending"))
		assert (np.diff(asc) > 0).all() and (np.diff(desc) < 0).all() and asc[0] < 0 < asc[-1]
		eq = sm.make_values("equal", G, 0.5, rng, bf16)
		assert len(np.unique(eq)) == 1 and len(np.unique(sm.make_values("alternate", G, 0.5, rng, bf16))) == 2
		blocks = sm.make_values("blocks", G, 0.5, rng, bf16)
		edges = np.flatnonzero(np.diff(blocks) != 0) + 1
		assert set(edges) <= {64, 128, 256, 2048, 2112, 2176, 2304} and len(edges) >= 3
		pairs = sm.make_values("ulp_pairs", G, 0.5, rng, bf16).view(np.uint32).astype(np.int64)
		assert (pairs[1::2] - pairs[0::2] == (1 << 16 if bf16 else 1)).all()
		cost = 0.5 * G - sm.make_values("zero_cross", G, 0.5, rng, bf16).astype(np.float64)
		assert (cost < 0).any() and (cost > 0).any() and (cost == 0).any()
		sp = sm.make_values("specials", G, 0.5, rng, bf16)
		assert np.isposinf(sp).any() and np.isneginf(sp).any() and (np.abs(sp[sp != 0]) < 1e-37).any() and (np.abs(sp[np.isfinite(sp)]) > 9e29).any()
		rb = sm.make_values("random_bits", G, 0.5, rng, bf16)
		assert np.isfinite(rb).all() and len(np.unique(rb.view(np.uint32) >> 23)) > 300


def test_loop_guard_case_stops_and_goes_on():
	"""the short case that ends on the guard on purpose: nothing popped, the model unchanged, and a larger budget lets it go on"""
	g = sm.GUARD_CASE
	m, log = sm.run(g, False, budget=sm.GUARD_BUDGET)
	last = log[-1]
	assert not last.step.popped and last.n_new == 0 and len(log) > 5 and len(m) + 12 * last.n_expand > sm.GUARD_BUDGET
	assert m.runs(1) or len(m) + 12 > sm.GUARD_BUDGET
	n = len(m)
	m.budget = g.capacity
	assert m.runs(g.N) and m.step(g.N, np.zeros(m.dry(g.N)[0][-1], np.float32)).n_states > n
