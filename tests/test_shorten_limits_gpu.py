"""
DeviceGoalBall.shorten (rk_bshorten) and DeviceSymBall.shorten (rk_sshorten) at the limit they promise: queues of 4 096 moves and
windows of the whole queue, against the fast exact reference of tests/shorten_long_ref.py (pinned to the plain-Python models by
tests/test_shorten_limits_cpu.py, which also proves that its words get there).  Everything is integer work: every comparison is
exact.  What each test reaches --
  * one pass of the entry, max_len = 4 096, radius 4, `collapse`, `nested`, a 4 095-move prefix, one move and no move in ONE call,
    windows 4 096 and 8: the DP's key with k - 1 = 4 095 and cost[] and pred[] up to entry 4 096 of 4 097; sixteen trips of a DP
    thread's loop with tied minima more than 256 apart (trips) and 64..256 apart (waves); the windows kernels over 64 chunks with
    the byte index up to 16.7 M per queue and past 2^26 in the call; the emit's re-composition of edges of 2, 5..6, 16 and 64
    chunks, and pos / nxt[] at both ends of an edge (0, 4 096); rows, -1 padding, lengths and the error word.  Radius 0: the whole
    queue is one identity window and the result the empty word;
  * `incompressible`, window 1, radius 3: cost[4 096] = 4 096 in the uint16 cost, the queue back byte for byte;
  * the fixed point of the method on [collapse, nested], window None and 300, equals the reference iterated as the models iterate;
    a further call returns it; the symmetry ball's lengths are the plain ball's; every output has its input's effect
    (cube.multi_rotate);
  * 17 queues of 4 096 moves with every window and the real 256 MB cap: the first pass is cut into calls of 15 and 2;
  * rk_bshorten_scratch_bytes at the limit, and (max_len, window) = (4 096, 4 097) refused.

Measured on an MI355X: the twelve cases take 8 s together.  4.4 s of them go to the first case, which computes the reference's
three depth tables (`collapse` and `nested` at radius 4, `collapse(0)` at radius 0; the 4 095-move prefix and the narrower windows
read the same tables) -- every later case finds them kept: one pass at the limit for the other kind 0.17 s, a fixed point 0.14 s
to 0.22 s, the seventeen queues under the real cap 0.06 s (plain) and 0.11 s (sym), the rest under 0.05 s.
"""
import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from tests import ball_model
from tests import shorten_long_ref as ref
from tests.ball_kinds import IDS, KINDS, PLAIN, device_ball, lists, one_pass_direct
from tests.test_symball_shorten_gpu import _apply_all

pytestmark = pytest.mark.gpu

LIMIT = 4096
CAP = 256 << 20


def _assert_rows_equal_one_pass(kind, radius: int, batch, window: int):
	rows, lengths, err = one_pass_direct(kind, device_ball(kind, radius), batch, window, max_len=LIMIT)
	want = [ref.one_pass(kind.name, w, radius, window).word for w in batch]
	assert err == 0 and rows.shape == (len(batch), LIMIT) and lengths.tolist() == [len(w) for w in want]
	for r, w in enumerate(want):
		assert rows[r, :len(w)].tolist() == list(w) and (rows[r, len(w):] == -1).all()
	return want


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_one_pass_of_the_entry_at_4096_moves_and_windows_of_4096(kind):
	collapse, nested = ref.collapse(4), ref.nested()
	batch = [collapse, nested, nested[:LIMIT - 1], nested[:1], ()]
	assert [len(w) for w in batch] == [LIMIT, LIMIT, LIMIT - 1, 1, 0]
	want = _assert_rows_equal_one_pass(kind, 4, batch, LIMIT)
	assert len(want[0]) == 4 and 4 < len(want[1]) < LIMIT and want[3] == nested[:1] and want[4] == ()
	want = _assert_rows_equal_one_pass(kind, 4, batch, 8)
	assert 1000 < len(want[0]) < LIMIT and len(want[1]) < LIMIT
	# radius 0: only identity windows are held, and the whole queue is one
	nothing = ref.collapse(0)
	assert _assert_rows_equal_one_pass(kind, 0, [nothing], LIMIT) == [()]
	assert 0 < len(_assert_rows_equal_one_pass(kind, 0, [nothing], 8)[0]) < LIMIT


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_incompressible_comes_back_byte_for_byte_at_the_limit(kind):
	word = ref.incompressible()
	assert ref.one_pass(kind.name, word, 3, 1).cost == LIMIT
	rows, lengths, err = one_pass_direct(kind, device_ball(kind, 3), [word], 1, max_len=LIMIT)
	assert err == 0 and lengths.tolist() == [LIMIT] and rows[0].tolist() == list(word)
	assert lists(device_ball(kind, 3).shorten([word], window=1)) == [list(word)]


@pytest.mark.parametrize("window", (None, 300))
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_fixed_point_of_the_method_equals_the_reference(kind, window):
	batch = [ref.collapse(4), ref.nested()]
	want = [list(ref.shorten(kind.name, w, 4, window)) for w in batch]
	ball = device_ball(kind, 4)
	got = lists(ball.shorten(batch, window=window))
	assert got == want
	assert len(got[0]) == 4 and len(got[1]) < LIMIT
	assert lists(ball.shorten(got, window=window)) == got                  # a further call returns it unchanged
	plain = got if kind is PLAIN else lists(device_ball(PLAIN, 4).shorten(batch, window=window))
	assert [len(g) for g in got] == [len(p) for p in plain]                # the symmetry ball's lengths are the plain ball's
	assert (_apply_all(got) == _apply_all([list(w) for w in batch])).all()


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_the_real_scratch_cap_cuts_seventeen_queues(monkeypatch, kind):
	"""A queue of 4 096 moves with every window needs 4 096 * 4 096 + 2 * 4 097 = 16 785 410 bytes of scratch: fifteen fit under
	the method's own 256 MB, seventeen do not."""
	lib = _ffi.lib()
	assert lib.rk_bshorten_scratch_bytes(17, LIMIT, LIMIT) > CAP >= lib.rk_bshorten_scratch_bytes(15, LIMIT, LIMIT)
	ball = device_ball(kind, 4)
	assert kind.ball.shorten_scratch_bytes == CAP and "shorten_scratch_bytes" not in vars(ball)
	words = (ref.collapse(4), ref.nested())
	order = np.random.RandomState(17).permutation([0] * 8 + [1] * 9).tolist()
	single = [lists(ball.shorten([w]))[0] for w in words]
	assert single == [list(ref.shorten(kind.name, w, 4, None)) for w in words]
	real, calls = getattr(lib, kind.shorten_entry), []
	monkeypatch.setattr(lib, kind.shorten_entry, lambda *a: calls.append((a[3], a[4], a[10])) or real(*a))
	got = lists(ball.shorten([words[k] for k in order]))
	assert got == [single[k] for k in order]
	first = [c for c in calls if c[1] == LIMIT]                              # the first pass: later ones have shorter queues
	assert [n for n, _, _ in first] == [15, 2] and len(calls) > 2
	assert all(scratch <= CAP + kind.scratch_slack for _, _, scratch in calls)


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_limits_from_the_inside(kind):
	lib = _ffi.lib()
	for n, max_len, window in ((1, LIMIT, LIMIT), (17, LIMIT, LIMIT), (1, LIMIT - 1, LIMIT - 1), (3, LIMIT, 1), (5, 4093, 4091)):
		depth_bytes = (n * max_len * window + 15) & ~15                      # the d(i, j) bytes, rounded so that the pred rows are aligned
		assert lib.rk_bshorten_scratch_bytes(n, max_len, window) == depth_bytes + n * (max_len + 1) * 2 > 0
	assert lib.rk_bshorten_scratch_bytes(1, LIMIT, LIMIT) == 16_777_216 + 8_194
	assert lib.rk_bshorten_scratch_bytes(1, LIMIT, LIMIT + 1) < 0 and lib.rk_bshorten_scratch_bytes(1, LIMIT + 1, LIMIT + 1) < 0
	ball = device_ball(kind, 3)
	known = np.stack([ball_model.scramble(5, 2), ball_model.scramble(20_000, 20)])
	acts = torch.zeros((1, LIMIT), dtype=torch.int8, device="cuda")
	lens = torch.tensor([LIMIT], dtype=torch.int32, device="cuda")
	out, n_out, err = torch.full((1, LIMIT), 77, dtype=torch.int8, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
	need = lib.rk_bshorten_scratch_bytes(1, LIMIT, LIMIT)
	scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
	entry = getattr(lib, kind.shorten_entry)
	args = lambda window: (ball._h, acts.data_ptr(), lens.data_ptr(), 1, LIMIT, window, out.data_ptr(), n_out.data_ptr(), err.data_ptr(),
	                       scratch.data_ptr(), need, _ffi.stream_ptr())
	assert entry(*args(LIMIT + 1)) == -1
	torch.cuda.synchronize()
	assert (n_out.item(), err.item()) == (1, 1) and (out == 77).all().item()      # nothing was launched
	assert ball.depth(known).tolist() == [2, -1]
	_ffi.check(entry(*args(LIMIT)))                                         # 4 096 turns of one face: 1 024 identity loops
	torch.cuda.synchronize()
	assert (n_out.item(), err.item()) == (0, 0) and (out == -1).all().item()
	assert ball.depth(known).tolist() == [2, -1]
