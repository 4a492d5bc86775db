"""
The A* engine through the three-call form of an iteration (rk_astar_expand, rk_astar_new_states_oh, rk_astar_commit), with the pop
count and the values of every iteration chosen by the test: tests/astar_steps_model.py drives the CPU model and the engine in
lock-step and the engine has to equal the model EXACTLY after every iteration -- no tolerance anywhere.

What this reaches that a whole search with a fixed `expansions` and a net does not:
  * n_expand different from the previous call: k_pop_select_only, in a wide engine k_pop_wide with C_NEXP < N, and pop lists of
    fewer than N nodes -- selected unstaged (k_pop_select_only), staged in LDS (k_end) and by the grid (N = 2049);
  * the number of new records steered onto the sizes where k_records_sort<256>, k_records_sort<2048>, k_merge_pass and
    k_queue_insert change their form (astar_steps_model.targets), in engines that sit next to each geometry switch;
  * values chosen by position (astar_steps_model.PATTERNS): the worst cases of a stable merge by rank and of the multi-way insert.
tests/test_astar_steps_cpu.py asserts on the model alone that the schedule really gets there.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from oracle import cube_oracle as orc
from tests import astar_steps_model as sm

pytestmark = pytest.mark.gpu

ESTATE = -4


class Engine:
	"""One rk_astar handle following the model; `iteration` is what astar_steps_model.run calls."""

	def __init__(self, g, bf16, budget):
		self.lib, self.g, self.bf16, self.it = _ffi.lib(), g, bf16, 0
		self.h = C.c_void_p()
		_ffi.check(self.lib.rk_astar_create(C.byref(self.h), g.capacity, g.N))
		_ffi.check(self.lib.rk_astar_set_values_dtype(self.h, _ffi.OH_BF16 if bf16 else _ffi.OH_F32))
		start = np.ascontiguousarray(sm.start_state(g))
		_ffi.check(self.lib.rk_astar_reset(self.h, start.ctypes.data, g.lambda_, None))
		_ffi.check(self.lib.rk_astar_set_budget(self.h, budget, None))
		self.info = (C.c_longlong * 5)()
		self.pops = np.zeros(g.N + 8, np.int64)
		self.n_exp = g.N                                                       # what the engine's pending pop list was selected for
		self.open_checks = 0

	def close(self):
		if self.h:
			self.lib.rk_astar_destroy(self.h)
			self.h = None

	def where(self, n_expand, n_new, pattern):
		return f"N = {self.g.N} {'bf16' if self.bf16 else 'f32'}, iteration {self.it}: n_expand {n_expand}, n_new {n_new}, pattern {pattern}"

	def next_pops(self):
		n = self.lib.rk_astar_next_pops(self.h, self.pops.ctypes.data, len(self.pops), None)
		assert n >= 0, n
		return self.pops[:n].tolist()

	def status(self):
		st = np.zeros(8, np.int64)
		_ffi.check(self.lib.rk_astar_status(self.h, st.ctypes.data, None))
		return st.tolist()

	def check_open(self, m, at):
		want_cost, want_idx = m.open_sorted()
		n = int(self.lib.rk_astar_open_size(self.h))
		assert n == len(want_idx), (at, n, len(want_idx))
		cost, idx = np.zeros(n + 1), np.zeros(n + 1, np.int64)
		assert self.lib.rk_astar_export_open(self.h, cost.ctypes.data, idx.ctypes.data, n + 1, None) == n, at
		assert (idx[:n] == want_idx).all(), (at, "open queue: indices", int(np.flatnonzero(idx[:n] != want_idx)[0]))
		assert (cost[:n].view(np.uint64) == want_cost.view(np.uint64)).all(), (at, "open queue: cost bits")
		self.open_checks += 1

	def check_new_states(self, m, step, at):
		"""rk_astar_new_states_oh of the pending expansion, in every kind the search agents ask for"""
		n, first = step.n_new, step.n_states - step.n_new + 1
		states = np.array(m.states[first:first + n], np.int8).reshape(n, 20)
		oh = orc.as_oh(states)
		out = torch.zeros((n + 1, 480), dtype=torch.float32, device="cuda")
		_ffi.check(self.lib.rk_astar_new_states_oh(self.h, out.data_ptr(), _ffi.OH_F32, None))
		assert (out[:n].cpu().numpy() == oh).all() and not out[n].any(), (at, "one-hot float32")
		out = torch.zeros((n + 1, 480), dtype=torch.bfloat16, device="cuda")
		_ffi.check(self.lib.rk_astar_new_states_oh(self.h, out.data_ptr(), _ffi.OH_BF16, None))
		assert (out[:n].float().cpu().numpy() == oh).all() and not out[n].any(), (at, "one-hot bfloat16")
		out = torch.full((n + 1, 20), -1, dtype=torch.int8, device="cuda")
		_ffi.check(self.lib.rk_astar_new_states_oh(self.h, out.data_ptr(), _ffi.OH_STATES, None))
		assert (out[:n].cpu().numpy() == states).all() and (out[n] == -1).all(), (at, "raw states")

	def upload(self, values):
		"""the values as the engine takes them: float32, or the upper halves as bfloat16"""
		if self.bf16:
			return torch.from_numpy((values.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)).cuda()
		return torch.from_numpy(values).cuda()

	def iteration(self, m, n_expand, values, pattern, target):
		lib, h, g = self.lib, self.h, self.g
		at = self.where(n_expand, len(values), pattern)
		_ffi.check(lib.rk_astar_expand(h, n_expand, self.info, None))
		step = m.step(n_expand, values)
		info = list(self.info)
		assert info == [len(step.popped), step.n_new, step.won, step.solved, step.n_states], (at, info, step._replace(popped=len(step.popped)))
		# the list the expansion worked on: with n_expand != the previous call's it was selected again (k_pop_select_only, k_pop_wide)
		assert self.next_pops() == step.popped, (at, "pop list of this call", "selected again" if n_expand != self.n_exp else "as k_end left it")
		self.n_exp = n_expand
		if not step.popped:
			assert lib.rk_astar_commit(h, None, None) == ESTATE, (at, "nothing popped must leave nothing pending")
			return step
		special = target is not None or self.it == 0
		if special and step.n_new:
			self.check_new_states(m, step, at)
		dev = self.upload(values)
		_ffi.check(lib.rk_astar_commit(h, dev.data_ptr() if len(values) else None, None))
		assert self.next_pops() == m.next_pops(n_expand), (at, "pop list after the commit")
		st = self.status()
		assert st[:6] == [int(not m.runs(n_expand)), int(m.won), len(m), m.iterations, len(m.open), m.solved] and st[6] == 0, (at, st)
		assert st[7] == len(m.next_pops(n_expand)) and lib.rk_astar_size(h) == len(m), (at, st)
		if g.N <= 200 or special or self.it % 5 == 0:
			self.check_open(m, at)
		self.it += 1
		return step

	def check_end(self, m, seed):
		lib, h, n = self.lib, self.h, len(m)
		at = self.where("-", "-", "end")
		self.check_open(m, at)
		states, G = np.zeros((n, 20), np.int8), np.zeros(n)
		parents, pact = np.zeros(n, np.int64), np.zeros(n, np.int64)
		_ffi.check(lib.rk_astar_export(h, 1, n, states.ctypes.data, G.ctypes.data, parents.ctypes.data, pact.ctypes.data, None))
		assert (states == np.array(m.states[1:n + 1], np.int8)).all(), (at, "states")
		assert (G == np.array(m.G[1:n + 1])).all(), (at, "G after all relaxations")
		assert (parents == np.array(m.parents[1:n + 1])).all() and (pact[1:] == np.array(m.parent_actions[2:n + 1])).all(), (at, "parents / actions")
		rng = np.random.RandomState(seed)
		acts = np.zeros(4096, np.int64)
		for i in rng.randint(1, n + 1, 50).tolist():
			got = lib.rk_astar_path(h, i, acts.ctypes.data, len(acts), None)
			assert got >= 0 and acts[:got].tolist() == m.path(i), (at, "path", i)
		for i in rng.randint(1, n + 1, 50).tolist():
			assert lib.rk_astar_lookup(h, np.ascontiguousarray(m.states[i]).ctypes.data, None) == i, (at, "lookup", i)
		absent = orc.rotate(orc.rotate(orc.SOLVED, 0, 0), 3, 1)
		assert absent.tobytes() not in m.index and lib.rk_astar_lookup(h, np.ascontiguousarray(absent).ctypes.data, None) == 0


CASES = [(gi, bf16) for gi in range(len(sm.GEOMETRIES)) for bf16 in (False, True)]
IDS = [f"N{sm.GEOMETRIES[gi].N}-{'bf16' if bf16 else 'f32'}" for gi, bf16 in CASES]


@pytest.mark.parametrize("gi,bf16", CASES, ids=IDS)
def test_engine_follows_the_model_step_by_step(gi, bf16):
	g = sm.GEOMETRIES[gi]
	t0 = time.perf_counter()
	e = Engine(g, bf16, g.capacity)
	try:
		if g.N >= 2048:
			assert len(sm.queue_plan(g.N, g.capacity)) == 3                   # 3 * 2048 = POP_LDS: one workgroup selects; 3 * 2049: the grid
		m, log = sm.run(g, bf16, engine=e)
		e.check_end(m, g.seed)
	finally:
		e.close()
	c = sm.coverage(g, log)
	assert len(c["missed"]) <= 2 and not m.won, c
	print(f"N = {g.N} {'bf16' if bf16 else 'f32'}: {c['iterations']} iterations, {len(m)} states, {e.open_checks} open-queue comparisons, n_new hit {c['hit']}, "
	      f"missed {c['missed']}, {c['changes']} n_expand changes, {time.perf_counter() - t0:.2f} s")


def test_loop_guard_leaves_nothing_pending_and_a_budget_lets_it_go_on():
	"""The one run whose budget ends it: the expansion that the guard refuses pops nothing, reports the pool as it is and leaves
	nothing to commit; after rk_astar_set_budget the engine goes on, equal to the model."""
	g = sm.GUARD_CASE
	e = Engine(g, False, sm.GUARD_BUDGET)
	try:
		m, log = sm.run(g, False, engine=e, budget=sm.GUARD_BUDGET)
		assert not log[-1].step.popped and len(log) > 5
		st = e.status()
		assert st[0] == 1 and st[1] == 0 and st[2] == len(m) and st[3] == m.iterations and st[7] == 0, st
		e.check_open(m, "stopped on the guard")
		_ffi.check(e.lib.rk_astar_set_budget(e.h, g.capacity, None))
		m.budget = g.capacity
		assert e.status()[0] == 0 and e.next_pops() == m.next_pops(e.n_exp)
		_, more = sm.run(g, False, engine=e, model=m, iterations=25)
		assert len(more) == 25 and all(r.step.popped for r in more)
		e.check_end(m, 3)
	finally:
		e.close()
