"""
The two kept balls -- the plain goal ball (`DeviceGoalBall`) and the symmetry-reduced one (`DeviceSymBall`) -- as the GPU suites of
their readers see them: one record per kind that names everything in which the plain and the symmetry tests of a shared contract
differ, so that tests/test_ball_shorten_gpu.py and tests/test_ball_readers_batch_gpu.py state each contract once.
A helper for those suites and for tests/test_symball_shorten_gpu.py, tests/test_ball_batch_gpu.py and
tests/test_symsearch_batch_gpu.py, not a test module.

The constants of a kind are the ones its own suite had; they are not harmonised.  Where the reason for a difference is known it
stands beside the value.
"""
import dataclasses
import functools
import types

import numpy as np
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import (DeviceBallSearch, DeviceBallSearchBatch, DeviceGoalBall, DeviceSymBall, DeviceSymBallSearch,
                                          DeviceSymBallSearchBatch)
from tests import ball_model
from tests import shorten_model
from tests import sym_model
from tests import symsearch_model
from tests import symshorten_model
from tests import test_goal_ball_gpu as plain_suite
from tests import test_symsearch_cpu as sym_starts
from tests import test_symsearch_gpu as sym_suite

LENGTHS = symshorten_model.LENGTHS                 # the mixed batch of both kinds begins with queues of these lengths
CAPACITY = 300_000               # per slot: the largest pool of the symmetry starts (33 055 states) and the widest iteration behind it fit


@dataclasses.dataclass(frozen=True, eq=False)
class Kind:
	name: str
	ball: type                       # the device ball, its single search and its batch
	search: type
	batch: type
	build_model: object              # radius -> the model's ball
	shorten_model: types.ModuleType  # one_pass, shorten, detour_word, inverse, rev, ball_word
	shorten_entry: str               # the C entry of one pass
	batch_entries: str               # the prefix of the batch engine's C entries
	ball_create: tuple               # (entry prefix, arguments after the handle) of an unbuilt ball of radius 1
	extra_words: int                 # queues of the mixed batch behind the eight of LENGTHS
	#: (cap, window) of the scratch-chunk test: every cap cuts the first pass into several calls.  Why the second cap is 400 000
	#: for the plain ball and 10 000 for the symmetry ball is not recorded.
	scratch_caps: tuple
	scratch_slack: int               # bytes a call may exceed the cap by: the symmetry ball's d(i, j) bytes are rounded up to 16
	# --- the batch ---
	search_ball: object              # radius -> the device ball of the kind's single-search suite, which the batch tests share
	radius: int                      # of the ball most batch tests end at
	pops: int                        # the small pop count of those tests
	budget_pops: tuple
	batch_kw: dict                   # the plain tests take the default capacity per slot, the symmetry tests CAPACITY
	keys: tuple                      # the starts of the model comparison: plain (depth, seed), sym an index of test_symsearch_cpu.starts()
	state: object                    # key -> the 20-byte start
	model: object                    # (radius, key, budget=None) -> (the model's result, its pops or None where the model counts none)
	duplicate: object                # the start that five slots hold at once
	refill_long: object              # isolation on refill: the long search ...
	refill_short: tuple              # ... and the short ones that come and go beside it
	budget_full: object              # the start whose unbudgeted pool sizes two of the budgets ...
	budget_cases: object             # ... that pool's size -> ((key, budget or None), ...)
	pool_full: tuple                 # seven starts of which the second overflows a pool of 3 000
	edge: object                     # the edges test, at radius 2: the start that is searched alone ...
	edge_between: object             # ... and the one between two solved states
	time_limit: tuple                # two long starts and two short ones
	time_limit_again: slice          # which of them the engine runs afterwards

	def __repr__(self):
		return self.name

	def states(self, keys) -> np.ndarray:
		return np.stack([self.state(k) for k in keys])


# ---- plain ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _plain_words() -> tuple:
	"""Seeded scrambles with detours, cut to the lengths of the mixed batch."""
	return tuple(tuple(shorten_model.detour_word(40 + k, min(n, 20), n)[:n]) for k, n in enumerate(LENGTHS))


def _plain_model(radius: int, key, budget: int = None):
	return plain_suite._model(radius, *key, budget), None


PLAIN = Kind(
	name="plain", ball=DeviceGoalBall, search=DeviceBallSearch, batch=DeviceBallSearchBatch,
	build_model=ball_model.build, shorten_model=shorten_model, shorten_entry="rk_bshorten", batch_entries="rk_bsearchb",
	ball_create=("rk_ball", (1, 8)), extra_words=0,
	scratch_caps=((1, None), (400_000, None), (1, 8), (10_000, 8)), scratch_slack=0,
	search_ball=plain_suite._ball, radius=2, pops=7, budget_pops=(7, 4096), batch_kw={},
	keys=tuple(plain_suite.STARTS), state=lambda key: plain_suite._start(*key), model=_plain_model,
	duplicate=(7, 1),
	refill_long=(8, 0), refill_short=tuple((d, s) for d in (1, 2, 3) for s in (0, 1)) * 20,
	budget_full=(7, 0),
	budget_cases=lambda full: (((7, 0), 150), ((7, 1), None), ((7, 0), 5_000), ((5, 0), None), ((7, 0), 1), ((7, 0), full - 12),
	                           ((7, 0), full), ((6, 1), 2), ((3, 0), 1), ((8, 1), None)),
	pool_full=((5, 0), (8, 0), (3, 1), (5, 1), (2, 0), (3, 0), (1, 1)),
	edge=(6, 0), edge_between=(5, 0),
	time_limit=((8, 0), (8, 1), (7, 0), (2, 0)), time_limit_again=slice(0, None))


# ---- sym ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sym_starts() -> tuple:
	return tuple(sym_starts.starts())


def _sym_model(radius: int, key: int, budget: int = None):
	seed, moves, start = _sym_starts()[key]
	if radius == sym_starts.RADIUS and budget is None:
		return sym_starts.modelled(seed, moves)
	return symsearch_model.search(start, sym_starts.sym_ball(radius), max_states=budget)


SYM = Kind(
	name="sym", ball=DeviceSymBall, search=DeviceSymBallSearch, batch=DeviceSymBallSearchBatch,
	build_model=sym_model.build, shorten_model=symshorten_model, shorten_entry="rk_sshorten", batch_entries="rk_ssearchb",
	ball_create=("rk_symball", (1, 8, 0)), extra_words=4,
	scratch_caps=((1, None), (10_000, None), (1, 8), (10_000, 8)), scratch_slack=15,
	search_ball=sym_suite._sball, radius=sym_starts.RADIUS, pops=5, budget_pops=(5, 16_384), batch_kw={"capacity": CAPACITY},
	keys=tuple(range(24)), state=lambda key: _sym_starts()[key][2], model=_sym_model,
	duplicate=6,                     # own depth 3
	refill_long=7,                   # own depth 4
	refill_short=tuple(k for k in range(24) if _sym_starts()[k][1] <= 4) * 5,
	budget_full=6,                   # own depth 3
	budget_cases=lambda full: ((6, 150), (5, None), (6, 5_000), (3, None), (6, 1), (6, full - 12), (6, full), (12, 2), (2, 1), (14, None)),
	pool_full=(4, 6, 2, 12, 1, 9, 16),
	edge=5, edge_between=5,
	time_limit=(7, 15, 6, 1), time_limit_again=slice(2, None))

KINDS = (PLAIN, SYM)
IDS = [k.name for k in KINDS]


# ---- the shorten suites' balls and words: one device ball and one model ball per (kind, radius) for the session ------------------

_device_balls = {}


def device_ball(kind: Kind, radius: int):
	"""The shorten suite's device ball (it is read-only once built).  The batch tests take `kind.search_ball`'s instead: the balls
	that the single-search suites have built already."""
	if (kind, radius) not in _device_balls:
		_device_balls[kind, radius] = kind.ball(radius).build()
	return _device_balls[kind, radius]


@functools.lru_cache(maxsize=None)
def model_ball(kind: Kind, radius: int):
	return kind.build_model(radius)


@functools.lru_cache(maxsize=None)
def words(kind: Kind) -> tuple:
	"""The mixed batch: the eight queues of LENGTHS and, for the symmetry ball, four whose replaced segment has several shortest words."""
	return _plain_words() if kind is PLAIN else symshorten_model.mixed_batch()


@functools.lru_cache(maxsize=None)
def want_words(kind: Kind, radius: int, window, passes) -> tuple:
	"""What the kind's model makes of the mixed batch."""
	return tuple(tuple(kind.shorten_model.shorten(model_ball(kind, radius), w, window, passes)) for w in words(kind))


def lists(arrays) -> list:
	assert all(isinstance(a, np.ndarray) and a.dtype == np.int64 and a.ndim == 1 for a in arrays)
	return [a.tolist() for a in arrays]


def one_pass_direct(kind: Kind, ball, words, window, max_len=None):
	"""The kind's entry called directly: (rows (n, max_len) int8, lengths (n,) int32, error word)."""
	lib = _ffi.lib()
	n = len(words)
	max_len = max_len or max(len(w) for w in words)
	window = max_len if window is None else min(window, max_len)
	acts = np.full((n, max_len), -1, np.int8)
	for r, w in enumerate(words):
		acts[r, :len(w)] = w
	lens = torch.tensor([len(w) for w in words], dtype=torch.int32, device="cuda")
	d_acts = torch.from_numpy(acts).cuda()
	out = torch.full((n, max_len), 77, dtype=torch.int8, device="cuda")
	out_len = torch.full((n,), -5, dtype=torch.int32, device="cuda")
	err = torch.full((1,), 9, dtype=torch.int32, device="cuda")
	need = lib.rk_bshorten_scratch_bytes(n, max_len, window)                # one size and layout for both balls
	assert need > 0
	scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
	entry = getattr(lib, kind.shorten_entry)
	_ffi.check(entry(ball._h, d_acts.data_ptr(), lens.data_ptr(), n, max_len, window, out.data_ptr(), out_len.data_ptr(),
	                 err.data_ptr(), scratch.data_ptr(), need, _ffi.stream_ptr()))
	assert (d_acts.cpu().numpy() == acts).all()                          # the input is only read
	return out.cpu().numpy(), out_len.cpu().numpy(), int(err.item())


# The two contracts with forty cases per kind.  They are plain functions of the kind, called by a test of the same name in
# tests/test_ball_shorten_gpu.py (plain) and in tests/test_symball_shorten_gpu.py (sym), so that the eighty cases keep their ids.

def one_pass_of_the_entry_equals_one_pass_of_the_model(kind: Kind, radius: int, window):
	batch = words(kind)
	assert [len(w) for w in batch[:8]] == list(LENGTHS) and len(batch) == 8 + kind.extra_words
	want = want_words(kind, radius, window, 1)
	rows, lengths, err = one_pass_direct(kind, device_ball(kind, radius), batch, window)
	assert err == 0 and lengths.tolist() == [len(w) for w in want]
	for r, w in enumerate(want):
		assert rows[r, :len(w)].tolist() == list(w) and (rows[r, len(w):] == -1).all()
	if window == 1:
		assert [list(w) for w in want] == [list(w) for w in batch]
	# the method's single pass is the same pass
	assert lists(device_ball(kind, radius).shorten(batch, window=window, passes=1)) == [list(w) for w in want]


def fixed_point_equals_the_model(kind: Kind, radius: int, window):
	batch = words(kind)
	want = want_words(kind, radius, window, None)
	got = lists(device_ball(kind, radius).shorten(batch, window=window))
	assert got == [list(w) for w in want]
	assert all(len(g) <= len(w) for g, w in zip(got, batch))
	if window != 1:
		assert sum(map(len, got)) < sum(map(len, batch))
	# idempotent (a further call returns it unchanged), and the same state from a scrambled start
	assert lists(device_ball(kind, radius).shorten(got, window=window)) == got
	start = ball_model.scramble(321, 25)
	for g, w in zip(got, batch):
		assert (ball_model.apply(start, g) == ball_model.apply(start, w)).all()


# ---- the batch suites -----------------------------------------------------------------------------------------------------------

def assert_state_equals_model(b, i: int, ok: bool, want, popped=None, arrays: bool = True):
	"""State i of the batch's last call against the model's result (and the model's pop count where it gives one)."""
	in_repr = plain_suite._in_repr
	assert bool(ok) == want.result
	assert list(b.action_queue_of(i)) == want.queue
	assert b.lengths[i] == (len(want.queue) if want.result else -1)
	assert b.sizes[i] == want.len and b.status[i, 2] == want.len and b.depths[i] == want.depth
	assert b.meeting_depths[i] == (-1 if want.meeting is None else want.meeting_depth)
	assert (b.status[i, 9] == 0) == (want.meeting is None)          # the meeting node (`meeting_nodes` of the symmetry batch)
	assert b.status[i, 0] == 1 and b.status[i, 1] == int(want.result) and b.status[i, 6] == 0
	if popped is not None:
		assert b.popped[i] == popped
	if arrays:
		states, parents, actions = b.arrays(i)
		assert states.dtype == np.int8 and states.shape[0] == want.len and parents.dtype == np.int64 and actions.dtype == np.int64
		assert (states == in_repr(want.states)).all()
		assert (parents == want.parents).all() and (actions == want.actions).all()
