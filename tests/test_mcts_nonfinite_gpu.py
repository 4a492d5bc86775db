"""
What the MCTS engine (rk_mcts_*) does with a NaN or an infinity from the net ("No NaN enters a tree").

The descent's arg-max is only right while no score is NaN, and a wrong arg-max there is an action of -1: writes far outside a node's
record.  So the engine refuses what would become a NaN where it ENTERS a tree: a NaN value, or a NaN among the priors after the
softmax (a NaN or a +inf logit), of a NEW child or of a root stops that tree with error 4 before anything of the simulation is
written.  These tests pin down both sides of that rule:
  * what is refused: the tree stops at once, its statistics are the oracle's after the simulation before, nothing of the path is
    out of range, the other trees do not notice (a, b, f, g);
  * what is NOT refused, because the reference never reads it or handles it: the rows of children that are already in the tree (c),
    the rows of a tree that is done (d), infinite values (e) -- there the engine equals the oracle bit for bit.

The poison is planted ON THE DEVICE (`PoisonNet`: a device counter of forwards and a torch.where), so the same net works eagerly and
inside a replayed hipGraph.  Which (tree, simulation, child) to poison is read from the oracle's own run, and every test asserts that
the chosen child is new, or known, as its case requires: a seed that no longer gives that fails, it does not skip.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import MCTSBatch
from oracle import cube_oracle as orc
from oracle.search_oracle import LookupNet, MCTSOracle, StubNet
from tests.test_mcts_gpu import _same_tree
from tests.test_real_valued_search_gpu import engine_priors

pytestmark = pytest.mark.gpu

T, CAP, C_PUCT = 4, 2000, 5.0
NAN, INF = float("nan"), float("inf")
ERR_NONFINITE = 4


class PoisonNet:
	"""`net` with chosen numbers of ONE forward overwritten: at forward number `at` (0 = the first call, which in a search is the
	roots' forward, so simulation s of `MCTSBatch.search` is forward s) the rows `rows` get `value` in the value head and / or
	`logit` in column `col` of the policy head.  On torch inputs the forward count is an int64 on the device, compared and then
	incremented in place, and the overwrite is a torch.where: no host decision, so a captured forward poisons the replay whose turn
	it is.  On NumPy inputs (the oracle's side) the count is a host integer.  `merged`: both heads leave as views of one
	(rows, 13) tensor, policy in columns 0..11 and value in column 12, as a net with merged heads hands them over."""

	def __init__(self, net, at: int, rows, value: float = None, logit: float = None, col: int = 0, merged: bool = False):
		self.net, self.at, self.rows, self.value, self.logit, self.col, self.merged = net, int(at), list(rows), value, logit, col, merged
		self.counter = torch.zeros((), dtype=torch.int64, device="cuda")
		self.at_dev = torch.tensor(self.at, dtype=torch.int64, device="cuda")
		self.host_calls = 0
		self._row_masks = {}

	def eval(self):
		return self

	def _rows_of(self, n: int) -> torch.Tensor:
		if n not in self._row_masks:                                      # (made before any capture: the first forwards are eager)
			m = torch.zeros((n, 1), dtype=torch.bool)
			for r in self.rows:
				if r < n:
					m[r] = True
			self._row_masks[n] = m.cuda()
		return self._row_masks[n]

	def __call__(self, x, policy=True, value=True):
		out = self.net(x, policy=policy, value=value)
		heads = list(out) if isinstance(out, (list, tuple)) else [out]
		p = heads[0] if policy else None
		v = heads[-1] if value else None
		if isinstance(x, torch.Tensor):
			hit = (self.counter == self.at_dev) & self._rows_of(len(x))   # (n, 1) bool, all False except in forward `at`
			self.counter.add_(1)
			if v is not None and self.value is not None:
				v = torch.where(hit.reshape(v.shape[0], *([1] * (v.dim() - 1))), torch.full_like(v, self.value), v)
			if p is not None and self.logit is not None:
				cols = torch.arange(12, device=p.device) == self.col
				p = torch.where(hit & cols, torch.full_like(p, self.logit), p)
			if self.merged and p is not None and v is not None:
				both = torch.empty((len(p), 13), dtype=p.dtype, device=p.device)
				both[:, :12] = p
				both[:, 12] = v.reshape(-1).to(p.dtype)
				p, v = both[:, :12], both[:, 12:]
		else:
			if self.host_calls == self.at:
				for r in self.rows:
					if v is not None and self.value is not None:
						v = np.array(v, copy=True)
						v[r] = self.value
					if p is not None and self.logit is not None:
						p = np.array(p, copy=True)
						p[r, self.col] = self.logit
			self.host_calls += 1
		res = ([p] if policy else []) + ([v] if value else [])
		return res if len(res) > 1 else res[0]


def _starts(seed: int, n: int = T) -> np.ndarray:
	out = []
	for i in range(n):
		np.random.seed(seed + i)
		out.append(orc.scramble(3 + i % 3, True)[0])                      # 3 .. 5 moves
	return np.array(out)


def _oracle(net, start, budget: int, max_sims: int = None, hook: bool = False) -> MCTSOracle:
	ref = MCTSOracle(net, C_PUCT, False, priors=engine_priors(net, "kernel") if hook else None)
	ref.solved = ref.search(start, budget, max_sims)
	return ref


def _before(net, start, budget: int, s: int, hook: bool = False):
	"""The oracle's tree BEFORE simulation `s`, which must then take place and solve nothing: -> (tree, leaf that simulation s
	expands, which of the leaf's 12 children are new to the tree)."""
	ref = _oracle(net, start, budget, s - 1, hook)
	assert not ref.solved and ref.sims == s - 1 and len(ref) + 12 <= budget, "pick another seed: simulation s does not take place"
	leaf = 1
	for a in ref.action_queue:
		leaf = int(ref.neighbors[leaf, a])
	assert leaf > 0 and ref.leaves[leaf]
	children = orc.expand12(ref.states[leaf][None])
	assert not orc.multi_is_solved(children).any(), "pick another seed: simulation s solves the tree"
	new = np.array([c.tobytes() not in ref.index for c in children])
	return ref, leaf, new


def _status(h) -> np.ndarray:
	st = np.zeros((T, 6), np.int64)                                       # done, solved, n_states, simulations, path_len, error
	_ffi.check(_ffi.lib().rk_mcts_status(h, st.ctypes.data, _ffi.stream_ptr()))
	return st


def _export(h, tree: int, n: int) -> dict:
	"""rows 0..n of one tree in the reference's dtypes, straight from the C ABI (MCTSBatch.tree_arrays raises on an engine error)"""
	out = dict(states=np.zeros((n + 1, 20), np.int8), neighbors=np.zeros((n + 1, 12), np.int64), leaves=np.ones(n + 1, np.uint8),
	           P=np.zeros((n + 1, 12)), V=np.zeros(n + 1), N=np.zeros((n + 1, 12), np.int64), W=np.zeros((n + 1, 12)), L=np.zeros((n + 1, 12)))
	_ffi.check(_ffi.lib().rk_mcts_export(h, tree, 1, n, out["states"][1:].ctypes.data, out["neighbors"][1:].ctypes.data, out["leaves"][1:].ctypes.data,
	                                     out["P"][1:].ctypes.data, out["V"][1:].ctypes.data, out["N"][1:].ctypes.data, out["W"][1:].ctypes.data,
	                                     out["L"][1:].ctypes.data, _ffi.stream_ptr()))
	out["leaves"] = out["leaves"].astype(bool)
	out["n"] = n
	return out


def _refused_tree_is_the_oracle_before(h, tree: int, st: np.ndarray, before: MCTSOracle, new: np.ndarray, s: int, ahead: bool = True):
	"""The tree that met the NaN in simulation `s`: stopped with error 4, simulation s not counted, and its statistics those of the
	oracle stopped after simulation s - 1.

	L is compared as well.  `MCTSOracle.search(max_sims=s - 1)` ends with find_leaf of the path that simulation s would have
	expanded, so the virtual loss of that path is outstanding in the oracle exactly as in the engine, whose backup of simulation
	s - 1 ended with the same descent and whose refused backup of simulation s cleared nothing.  What differs, and is not compared,
	is the expansion itself: the engine expands ahead (states, neighbour links and the leaf's flag of simulation s are in the tree
	when its net outputs are refused; `ahead`), the oracle has not expanded yet."""
	n = len(before)
	print(f"refused tree {tree} at simulation {s}: status {st[tree].tolist()}, oracle before: {n} states, {int(new.sum())} new children; all trees' simulations {st[:, 3].tolist()}")
	assert list(st[tree, [0, 1, 5]]) == [1, 0, ERR_NONFINITE] and st[tree, 3] == s - 1, st
	assert st[tree, 2] == n + (int(new.sum()) if ahead else 0)
	got = _export(h, tree, int(st[tree, 2]))
	for k in ("P", "V", "W", "L"):
		assert not np.isnan(got[k]).any(), k                              # the whole pool in use, the refused children's rows included
		assert (got[k][1:n + 1] == getattr(before, k)[1:n + 1]).all(), k
	assert (got["N"][1:n + 1] == before.N[1:n + 1]).all()
	assert not got["P"][n + 1:].any() and not got["V"][n + 1:].any() and not got["W"][n + 1:].any() and not got["N"][n + 1:].any()
	plen = int(st[tree, 4])
	acts, nodes = (C.c_longlong * plen)(*([-1] * plen)), (C.c_longlong * plen)()
	n_act = _ffi.lib().rk_mcts_path(h, tree, acts, nodes, plen, _ffi.stream_ptr())
	assert n_act == plen - 1 and all(0 <= a < 12 for a in acts[:n_act]) and all(1 <= x <= st[tree, 2] for x in nodes[:plen])
	assert list(acts[:n_act]) == list(before.action_queue)


@contextlib.contextmanager
def _count_calls(name: str):
	"""-> a one-element list: how often the library entry `name` was called inside"""
	lib, entry, calls = _ffi.lib(), getattr(_ffi.lib(), name), [0]

	def counted(*args):
		calls[0] += 1
		return entry(*args)
	setattr(lib, name, counted)
	try:
		yield calls
	finally:
		setattr(lib, name, entry)


# ---- (a), (b): a NaN that would enter the tree stops it ----------------------------------------------------------------------------
def _search_is_refused(net_of, hook: bool, seed: int, tree: int, s: int, use_graph: bool, **poison):
	starts, budget = _starts(seed), 400
	before, _, new = _before(net_of(), starts[tree], budget, s, hook)
	k = int(np.flatnonzero(new)[-1])                                      # the LAST new child: not simply lane 0
	assert new[k] and new.sum() >= 2
	net = PoisonNet(net_of(), s, [12 * tree + k], **poison)
	agent = MCTSBatch(net, C_PUCT, T, capacity=CAP)
	with _count_calls("rk_mcts_backup_select_logits") as calls:
		with pytest.raises(_ffi.RubiksHipError, match="NaN"):
			agent.search(starts, max_states=budget, use_graph=use_graph, poll=8)
	assert calls[0] >= (3 if use_graph else s)                            # the entry under test is the one the search went through
	assert int(net.counter) > s
	st = _status(agent._h)
	_refused_tree_is_the_oracle_before(agent._h, tree, st, before, new, s)
	assert not st[[t for t in range(T) if t != tree], 5].any(), st
	assert agent.captures == int(use_graph)


@pytest.mark.parametrize("use_graph", [False, True])
def test_nan_value_of_a_new_child_stops_the_tree(use_graph):
	"""(a) StubNet, simulation 6 of tree 2 (behind the two eager simulations of a captured search: a replay meets the NaN)."""
	_search_is_refused(StubNet, False, 4104, 2, 6, use_graph, value=NAN)


@pytest.mark.parametrize("logit,dtype,merged,use_graph", [(NAN, "float32", False, False), (INF, "float32", True, True),
                                                          (NAN, "bfloat16", True, False), (INF, "bfloat16", False, True)])
def test_nan_or_plus_inf_logit_of_a_new_child_stops_the_tree(logit, dtype, merged, use_graph):
	"""(b) real-valued logits through rk_mcts_backup_select_logits, float32 and bfloat16, heads apart (stride 12) and merged (stride
	13).  A +inf logit is the row's maximum, exp(inf - inf) is a NaN, and so is the whole row after the division."""
	_search_is_refused(lambda: LookupNet(seed=7, dtype=dtype), True, 4104, 1, 5, use_graph, logit=logit, col=7, merged=merged)


# ---- (c), (d): what the reference never reads changes nothing -------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_nan_in_the_row_of_a_known_child_changes_nothing(use_graph):
	"""(c) Simulation 6 of tree 2 expands a leaf whose child k is in the tree already (agents.py:556-557 assign the new children
	only): NaN in that row's value and logit, and the whole batch is the unpoisoned oracle's to the end of the search."""
	starts, budget, tree, s = _starts(4104), 400, 2, 6
	_, _, new = _before(StubNet(), starts[tree], budget, s)
	assert new.any() and not new.all()
	k = int(np.flatnonzero(~new)[0])
	assert not new[k]
	net = PoisonNet(StubNet(), s, [12 * tree + k], value=NAN, logit=NAN, col=3)
	agent = MCTSBatch(net, C_PUCT, T, capacity=CAP)
	solved = agent.search(starts, max_states=budget, use_graph=use_graph, poll=8)
	assert int(net.counter) > s
	print(f"known child {k} of tree {tree} poisoned at simulation {s}: {int(net.counter)} forwards, {agent.captures} captures, status {agent.status.tolist()}")
	for t in range(T):
		ref = _oracle(StubNet(), starts[t], budget)
		assert bool(solved[t]) == ref.solved and int(agent.status[t, 3]) == ref.sims and ref.sims >= (s if t == tree else 1), t
		_same_tree(agent.tree_arrays(t), ref)
		assert list(agent.action_queue_of(t)) == list(ref.action_queue), t


def test_nan_in_the_rows_of_done_trees_changes_nothing():
	"""(d) Tree 1 starts solved, tree 3 runs out of its budget of 30 states in its second simulation; at simulation 5 all 24 rows of
	the two carry NaN in value and logit.  Neither tree changes or reports an error, the others are the oracle's."""
	starts, s = _starts(4301), 5
	starts[1] = orc.SOLVED
	budgets = np.array([400, 400, 400, 30])
	rows = list(range(12, 24)) + list(range(36, 48))
	net = PoisonNet(StubNet(), s, rows, value=NAN, logit=NAN, col=0)
	agent = MCTSBatch(net, C_PUCT, T, capacity=CAP)
	solved = agent.search(starts, max_states=budgets, poll=8)
	assert int(net.counter) > s and not agent.status[:, 5].any()
	assert list(agent.status[1, :4]) == [1, 2, 1, 0] and solved[1]        # done, solved at the root, one state, no simulation
	for t in (0, 2, 3):
		ref = _oracle(StubNet(), starts[t], int(budgets[t]))
		assert bool(solved[t]) == ref.solved and int(agent.status[t, 3]) == ref.sims, t
		_same_tree(agent.tree_arrays(t), ref)
		assert list(agent.action_queue_of(t)) == list(ref.action_queue), t
	assert agent.status[3, 3] < s <= min(agent.status[0, 3], agent.status[2, 3])     # tree 3 was done, trees 0 and 2 were running


# ---- (e): infinities are not refused ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value,more_sims", [(INF, 6), (-INF, None)])
def test_infinite_values_are_not_refused(value, more_sims):
	"""(e) +inf / -inf as the value of a new child of simulation 6 of tree 2, in the engine's net and -- the same child -- in the
	oracle's: W = +-inf gives the same infinity in all twelve scores or in one, no NaN, and the kernel's first-lane rule is
	np.argmax.  Engine and oracle agree on every array and on the action queue.
	-inf: to the end of the budget.  +inf: for 6 more simulations -- from then on every descent runs through that child (its edge's W
	is +inf for good, virtual losses do not lower it), and once the child's own children are expanded the descent has nowhere
	else to go: the reference then loops for ever (the engine would stop at max_path), which is not what this test is about."""
	starts, budget, tree, s = _starts(4104), 400, 2, 6
	_, _, new = _before(StubNet(), starts[tree], budget, s)
	k = int(np.flatnonzero(new)[-1])
	assert new[k] and new.sum() >= 2
	max_sims = s + more_sims if more_sims else None
	net = PoisonNet(StubNet(), s, [12 * tree + k], value=value)
	agent = MCTSBatch(net, C_PUCT, T, capacity=CAP)
	solved = agent.search(starts, max_states=budget, max_sims=max_sims, poll=8)
	print(f"value {value} for child {k} of tree {tree} at simulation {s}: status {agent.status.tolist()}")
	assert not agent.status[:, 5].any()
	for t in range(T):
		row_in_oracle = int(new[:k].sum())                                # the oracle's net sees the new children only
		ref = _oracle(PoisonNet(StubNet(), s, [row_in_oracle], value=value) if t == tree else StubNet(), starts[t], budget, max_sims)
		assert bool(solved[t]) == ref.solved and int(agent.status[t, 3]) == ref.sims, t
		got = agent.tree_arrays(t)
		_same_tree(got, ref)
		assert list(agent.action_queue_of(t)) == list(ref.action_queue), t
		if t == tree:
			assert ref.sims > s and (got["V"] == value).sum() == 1 and (got["W"] == value).any() and not np.isnan(got["W"]).any()


# ---- (f): the root, and the probabilities entry, through the C ABI -----------------------------------------------------------------
def _engine(starts, c: float = C_PUCT):
	lib, h = _ffi.lib(), C.c_void_p()
	_ffi.check(lib.rk_mcts_create(C.byref(h), len(starts), CAP, 256))
	_ffi.check(lib.rk_mcts_reset(h, starts.ctypes.data, None, c, 100.0, _ffi.stream_ptr()))
	return h


def _root_pv(h, net, n_trees: int = T):
	"""the roots' priors and values as a search hands them to rk_mcts_set_root_pv (agents.py:470-473)"""
	root_oh = torch.empty((n_trees, 480), device="cuda")
	_ffi.check(_ffi.lib().rk_mcts_roots_oh(h, root_oh.data_ptr(), _ffi.OH_F32, _ffi.stream_ptr()))
	p, v = net(root_oh)
	return p.float().softmax(dim=1).contiguous(), v.float().reshape(-1).contiguous()


def _net_outputs(h, net, n_trees: int = T):
	lib = _ffi.lib()
	_ffi.check(lib.rk_mcts_expand(h, _ffi.stream_ptr()))
	oh = torch.empty((12 * n_trees, 480), device="cuda")
	_ffi.check(lib.rk_mcts_children_oh(h, oh.data_ptr(), _ffi.OH_F32, _ffi.stream_ptr()))
	logits, values = net(oh)
	return logits.float().contiguous(), values.float().reshape(-1).contiguous()


@pytest.mark.parametrize("where", ["prior", "value", "infinite prior"])
def test_nan_at_a_root_stops_that_tree_only(where):
	"""(f) rk_mcts_reset, rk_mcts_set_root_pv with a NaN among tree 1's priors / in its value (or an infinite "probability", which
	times sqrt(0) visits would be a NaN score), one step: tree 1 reports error 4, no simulation and a root that holds nothing; its
	neighbours step normally.  A solved start's root is never read: a NaN there is no error."""
	lib, starts = _ffi.lib(), _starts(4400)
	starts[3] = orc.SOLVED
	h = _engine(starts)
	p, v = _root_pv(h, StubNet())
	if where == "value":
		v[1] = v[3] = NAN
	else:
		p[1, 11] = p[3, 2] = NAN if where == "prior" else INF
	_ffi.check(lib.rk_mcts_set_root_pv(h, p.data_ptr(), v.data_ptr(), _ffi.stream_ptr()))
	st = _status(h)
	assert list(st[1]) == [1, 0, 1, 0, 1, ERR_NONFINITE] and list(st[3]) == [1, 2, 1, 0, 1, 0] and not st[[0, 2]][:, [0, 5]].any(), st
	logits, values = _net_outputs(h, StubNet())
	_ffi.check(lib.rk_mcts_backup_select_logits(h, logits.data_ptr(), 12, values.data_ptr(), 1, _ffi.OH_F32, _ffi.stream_ptr()))
	st = _status(h)
	assert list(st[1]) == [1, 0, 1, 0, 1, ERR_NONFINITE] and list(st[3]) == [1, 2, 1, 0, 1, 0], st
	root = _export(h, 1, 1)
	assert not root["P"].any() and not root["V"].any() and not root["W"].any() and root["leaves"][1]
	for t in (0, 2):
		ref = _oracle(StubNet(), starts[t], CAP, 1)
		assert list(st[t]) == [0, 0, len(ref), 1, 2, 0], st
		_same_tree(_export(h, t, len(ref)), ref)
	_ffi.check(lib.rk_mcts_destroy(h))


@pytest.mark.parametrize("poison", [NAN, INF])
def test_probabilities_entry_refuses_a_nan_prior_of_a_new_child(poison):
	"""(f) rk_mcts_backup_select, the entry that takes probabilities: simulation 1, in which all 12 children of a root are new, with a
	NaN (an infinity) in one prior of child 9 of tree 2."""
	lib, starts = _ffi.lib(), _starts(4400)
	h = _engine(starts)
	p, v = _root_pv(h, StubNet())
	_ffi.check(lib.rk_mcts_set_root_pv(h, p.data_ptr(), v.data_ptr(), _ffi.stream_ptr()))
	logits, values = _net_outputs(h, StubNet())
	st = _status(h)
	assert (st[:, 2] == 13).all() and not st[:, 5].any()                  # every root's 12 children are new
	probs = logits.softmax(dim=1).contiguous()
	probs[12 * 2 + 9, 4] = poison
	_ffi.check(lib.rk_mcts_backup_select(h, probs.data_ptr(), values.data_ptr(), _ffi.stream_ptr()))
	st = _status(h)
	assert list(st[2]) == [1, 0, 13, 0, 1, ERR_NONFINITE], st
	got = _export(h, 2, 13)
	assert not got["P"][2:].any() and not got["V"][2:].any() and not got["W"].any() and not got["N"].any()
	for t in (0, 1, 3):
		ref = _oracle(StubNet(), starts[t], CAP, 1)
		assert list(st[t]) == [0, 0, 13, 1, 2, 0], st
		_same_tree(_export(h, t, 13), ref)
	_ffi.check(lib.rk_mcts_destroy(h))


def test_reset_refuses_an_exploration_constant_that_is_not_finite():
	lib, starts, h = _ffi.lib(), _starts(4400), C.c_void_p()
	_ffi.check(lib.rk_mcts_create(C.byref(h), T, CAP, 256))
	for c, nu in ((INF, 100.0), (NAN, 100.0), (1.0, INF), (1.0, NAN)):
		assert lib.rk_mcts_reset(h, starts.ctypes.data, None, c, nu, _ffi.stream_ptr()) == -1 and b"finite" in lib.rk_last_error()
	_ffi.check(lib.rk_mcts_destroy(h))


# ---- (g): the batch in two ranges on two streams ---------------------------------------------------------------------------------------
def test_ranges_on_two_streams_stop_the_right_tree():
	"""(g) Every simulation advances trees 0-1 and trees 2-3 by rk_mcts_backup_select_logits_range on two streams, each range with
	the net's outputs of ITS children only (row 0 = child 0 of the range's first tree), expand-ahead on as in the step that
	MCTSBatch captures for its halves.  The NaN sits in the second range's own numbering: row 12 + k is child k of tree 3.
	Tree 3 stops; trees 0, 1 and 2 are the oracle's after all the simulations."""
	lib, starts, budget, tree, s, sims = _ffi.lib(), _starts(4104), 400, 3, 5, 9
	before, _, new = _before(LookupNet(seed=7), starts[tree], budget, s, hook=True)
	k = int(np.flatnonzero(new)[-1])
	assert new[k] and new.sum() >= 2
	plain = LookupNet(seed=7)
	second = PoisonNet(LookupNet(seed=7), s - 1, [12 * (tree - 2) + k], logit=NAN, col=2)     # its forward 0 is simulation 1
	h = C.c_void_p()
	_ffi.check(lib.rk_mcts_create(C.byref(h), T, CAP, 256))
	ms = np.full(T, budget, np.int64)
	_ffi.check(lib.rk_mcts_reset(h, starts.ctypes.data, ms.ctypes.data, C_PUCT, 100.0, _ffi.stream_ptr()))
	p, v = _root_pv(h, plain)
	_ffi.check(lib.rk_mcts_set_root_pv(h, p.data_ptr(), v.data_ptr(), _ffi.stream_ptr()))
	_ffi.check(lib.rk_mcts_set_expand_ahead(h, sims))
	oh = torch.empty((12 * T, 480), device="cuda")
	cur, sides, keep = torch.cuda.current_stream(), (torch.cuda.Stream(), torch.cuda.Stream()), []
	for _ in range(sims):
		_ffi.check(lib.rk_mcts_expand(h, _ffi.stream_ptr()))
		_ffi.check(lib.rk_mcts_children_oh(h, oh.data_ptr(), _ffi.OH_F32, _ffi.stream_ptr()))
		for half, (net, side) in enumerate(zip((plain, second), sides)):
			logits, values = net(oh[24 * half:24 * half + 24])
			logits, values = logits.contiguous(), values.reshape(-1).contiguous()
			keep.append((logits, values))
			side.wait_stream(cur)
			with torch.cuda.stream(side):
				_ffi.check(lib.rk_mcts_backup_select_logits_range(h, 2 * half, 2, logits.data_ptr(), 12, values.data_ptr(), 1, _ffi.OH_F32, _ffi.stream_ptr()))
		for side in sides:
			cur.wait_stream(side)
	st = _status(h)
	_refused_tree_is_the_oracle_before(h, tree, st, before, new, s)
	for t in range(3):
		ref = _oracle(LookupNet(seed=7), starts[t], budget, sims, hook=True)
		assert list(st[t, [1, 2, 3, 5]]) == [int(ref.solved), len(ref), ref.sims, 0], (t, st)
		_same_tree(_export(h, t, len(ref)), ref)
	_ffi.check(lib.rk_mcts_destroy(h))
