"""
The 6x8x6 per-row kernels and the two converters against the oracle, at the sizes where each kernel changes form: the tail of a
tile, the second workgroup step, the second grid pass, the clamp of the input pipeline.

  k_rotate686<false>   groups of 64 rows, grid capped at 2 048 workgroups, next group prefetched with clamped loads
  k_is_solved686       groups of 128 rows, 18 chunk-mismatch bytes per row folded through LDS
  k_as_oh686           2 048 x 256 dwords = 7 281.8 rows per grid pass
  k_as_correct686      2 048 x 256 slots = 10 922.7 rows per grid pass
  k_oh686_from2024     tiles of 64 rows, grid capped at 8 192 workgroups
  k_686_to2024         tiles of 64 rows, grid capped at 8 192 workgroups

No expected value comes from a kernel: inputs are the paired oracle walks of tests/repr686_pairs.py (the same draws applied by
`orc.multi_rotate` and `orc.multi_rotate686`), expected outputs are the oracle's.  `to686`, `from686` and `device.multi_rotate`
appear only as the thing under test; the one exception is the round trip of the flipped edge / twisted corner.  Everything is
compared bit for bit; large results are compared on the device and a mismatch names the first differing row.
"""
import os
import re

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from oracle import c_oracle, cube_oracle as orc
from tests import repr686_pairs as pairs

pytestmark = pytest.mark.gpu

ROTATE_GROUP, ROTATE_GRID = 64, 2048                    # k_rotate686<false>: GROUP, launch_rotate686's grid cap
SOLVED_GROUP = 128                                      # k_is_solved686: GROUP
PASS_THREADS = 2048 * 256                               # k_as_oh686 (dwords) and k_as_correct686 (slots): grid cap x block
TILE, TILE_GRID = 64, 8192                              # R686_TILE, the two converters' grid cap
N_ROTATE = ROTATE_GRID * ROTATE_GROUP + ROTATE_GROUP + 5          # 131 141: two groups on the second pass, the last one of 5 rows
N_CONVERT = TILE_GRID * TILE + TILE + 3                           # 524 355: two tiles on the second pass, the last one of 3 rows
SENTINEL = 0x5A


@pytest.fixture(scope="module", autouse=True)
def _native_library_loaded():
	lib = _ffi.lib()
	assert lib.rk_init(0) == 0, lib.rk_last_error()
	assert "librubiks_hip.so" in open("/proc/self/maps").read()


def dev(a) -> torch.Tensor:
	return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def bits(t: torch.Tensor) -> torch.Tensor:
	return t.view(_BITS[t.dtype]) if t.dtype in _BITS else t


def assert_rows_equal(got: torch.Tensor, want: torch.Tensor, what=""):
	"""Bit equality on the device; a mismatch names the first differing row."""
	assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
	g, w = bits(got), bits(want)
	if torch.equal(g, w):
		return
	n = g.shape[0]
	bad = (g.reshape(n, -1) != w.reshape(n, -1)).any(dim=1).nonzero().reshape(-1)
	pytest.fail(f"{what}: {len(bad)} of {n} rows differ, the first is row {int(bad[0])}")


def new_stats() -> torch.Tensor:
	return torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device="cuda")


def guarded(n: int, row_shape, dtype=torch.int8) -> torch.Tensor:
	"""n + 1 rows filled with the sentinel byte: the kernel gets the first n, row n must keep the sentinel."""
	t = torch.empty((n + 1, *row_shape), dtype=dtype, device="cuda")
	t.view(torch.int8).fill_(SENTINEL)
	return t


def guard_intact(t: torch.Tensor) -> bool:
	return bool((t[-1].contiguous().view(torch.int8) == SENTINEL).all())


def edge_rows(n: int, *groups) -> list:
	"""Row 0, row n - 1, and for every group size the last row of the last full group and the first row of the partial last group."""
	rows = {0, n - 1}
	for g in groups:
		full = n // g * g
		if full:
			rows.add(full - 1)
		if full < n:
			rows.add(full)
	return sorted(rows)


def face_dir(a):
	return np.asarray(a) // 2, 1 - np.asarray(a) % 2


@pytest.fixture(scope="module")
def big():
	"""N_CONVERT paired rows on the device, shared and never written: tests clone what they edit."""
	idx, s20, s686 = pairs.gather(N_CONVERT, 524)
	return {"idx": idx, "s20": dev(s20), "s686": dev(s686)}


def paired(n: int, big):
	"""(pool indices, 20-byte rows, 6x8x6 rows) on the device: a small gather of its own, or the shared large one."""
	if n == N_CONVERT:
		return big["idx"], big["s20"], big["s686"]
	idx, s20, s686 = pairs.gather(n, 40 + n)
	return idx, dev(s20), dev(s686)


# ------------------------------------------------------------------------------------------------------ k_rotate686<false>
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, N_ROTATE])
def test_multi_rotate_equals_the_oracle(n):
	_, _, s686 = pairs.gather(n, 1000 + n)
	acts = np.random.RandomState(n).randint(0, 12, n)
	if n >= 12:
		acts[n - 12:] = np.arange(12)                                        # every action, in the last group
	want = orc.multi_rotate686(s686, *face_dir(acts))
	cube.set_is2024(False)
	src = dev(s686)
	keep = src.clone()
	full = guarded(n, (6, 8, 6))
	cube.device.bad_actions_seen()
	out = cube.device.multi_rotate(src, dev(acts.astype(np.uint8)), out=full[:n])
	assert_rows_equal(out, dev(want), "multi_rotate")
	assert torch.equal(src, keep) and guard_intact(full)
	assert not cube.device.bad_actions_seen()                                # codes 0..11 leave no mark


def test_bad_action_code_is_action_0_and_leaves_the_mark():
	n = 129
	_, _, s686 = pairs.gather(n, 12)
	acts = np.random.RandomState(12).randint(1, 12, n)
	bad = acts.copy()
	bad[[0, 64, 128]] = [12, 255, 13]
	acts[[0, 64, 128]] = 0
	want = orc.multi_rotate686(s686, *face_dir(acts))
	cube.set_is2024(False)
	cube.device.bad_actions_seen()
	out = cube.device.multi_rotate(dev(s686), dev(bad.astype(np.uint8)))
	assert_rows_equal(out, dev(want), "multi_rotate with codes >= 12")
	assert cube.device.bad_actions_seen() and not cube.device.bad_actions_seen()


# ---------------------------------------------------------------------------------------------------------- k_is_solved686
def _near_solved():
	"""Solved but for one slot of chunk 0 (bytes 0..15) / of chunk 17 (bytes 272..287): must read unsolved."""
	a, b = orc.SOLVED686.copy().reshape(48, 6), orc.SOLVED686.copy().reshape(48, 6)
	a[0] = np.eye(6, dtype=np.int8)[1]
	b[47] = np.eye(6, dtype=np.int8)[4]
	for s, chunk in ((a, 0), (b, 17)):
		assert set(np.nonzero(s.ravel() != orc.SOLVED686.ravel())[0] // 16) == {chunk}
	return a.reshape(6, 8, 6), b.reshape(6, 8, 6)


@pytest.mark.parametrize("n", [1, 127, 128, 129, N_ROTATE])
def test_multi_is_solved_at_group_edges_and_single_chunk_differences(n):
	_, _, s686 = pairs.gather(n, 2000 + n)
	plants = edge_rows(n, SOLVED_GROUP)
	s686[plants] = orc.SOLVED686
	near0, near17 = _near_solved()
	used = set(plants)
	for p in plants:                                                         # the near misses sit next to the solved rows
		for r, row in ((p + 1, near0), (p - 1, near17), (p + 2, near17), (p - 2, near0)):
			if 0 <= r < n and r not in used:
				s686[r] = row
				used.add(r)
	want = orc.multi_is_solved686(s686)
	assert np.nonzero(want)[0].tolist() == plants and (n < 3 or len(used) > len(plants))
	cube.set_is2024(False)
	x = dev(s686)
	want_dev = dev(want.astype(np.uint8))
	stats = new_stats()
	flags = cube.device.multi_is_solved(x, stats=stats)
	assert_rows_equal(flags, want_dev, "flags")
	assert stats.tolist() == [len(plants), plants[0]]
	assert_rows_equal(cube.device.multi_is_solved(x), want_dev, "flags only")
	only = new_stats()
	_ffi.check(_ffi.lib().rk_multi_is_solved(_ffi.REPR_686, x.data_ptr(), None, only.data_ptr(), n, _ffi.stream_ptr()))
	assert only.tolist() == [len(plants), plants[0]]
	if len(plants) > 1:                                                      # from row 1 on, the first solved row is not row 0
		late = new_stats()
		assert_rows_equal(cube.device.multi_is_solved(x[1:], stats=late), want_dev[1:], "flags from row 1 on")
		assert late.tolist() == [len(plants) - 1, plants[1] - 1]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, N_ROTATE])
def test_multi_rotate_solved_equals_the_oracle(n):
	_, _, s686 = pairs.gather(n, 3000 + n)
	acts = np.random.RandomState(3000 + n).randint(0, 12, n)
	plants = edge_rows(n, ROTATE_GROUP, SOLVED_GROUP)
	used = set(plants)
	for k, p in enumerate(plants):                                           # one move from solved, and the action that undoes it
		a = (5 * k + 2) % 12
		s686[p] = orc.rotate686(orc.SOLVED686, *face_dir(a ^ 1))
		acts[p] = a
		if p + 1 < n and p + 1 not in used:                                  # the same state with the move repeated: not solved
			s686[p + 1] = s686[p]
			acts[p + 1] = a ^ 1
			used.add(p + 1)
	want = orc.multi_rotate686(s686, *face_dir(acts))
	want_fl = orc.multi_is_solved686(want)
	assert np.nonzero(want_fl)[0].tolist() == plants
	cube.set_is2024(False)
	src, a_dev, want_dev, want_fl_dev = dev(s686), dev(acts.astype(np.uint8)), dev(want), dev(want_fl.astype(np.uint8))
	keep = src.clone()
	full = guarded(n, (6, 8, 6))
	stats = new_stats()
	out, flags = cube.device.multi_rotate_solved(src, a_dev, out=full[:n], stats=stats)
	assert_rows_equal(out, want_dev, "moved states")
	assert_rows_equal(flags, want_fl_dev, "flags")
	assert stats.tolist() == [len(plants), 0] and torch.equal(src, keep) and guard_intact(full)
	out2, flags2 = cube.device.multi_rotate_solved(src, a_dev)
	assert_rows_equal(out2, want_dev, "moved states, flags only")
	assert_rows_equal(flags2, want_fl_dev, "flags only")
	only = new_stats()
	out3 = torch.empty_like(src)
	_ffi.check(_ffi.lib().rk_multi_rotate_solved(_ffi.REPR_686, src.data_ptr(), a_dev.data_ptr(), out3.data_ptr(), None, only.data_ptr(), n,
	                                             _ffi.stream_ptr()))
	assert_rows_equal(out3, want_dev, "moved states, stats only")
	assert only.tolist() == [len(plants), 0]


# -------------------------------------------------------------------------------------------- k_as_oh686, k_as_correct686
@pytest.mark.parametrize("n", [1, 5, PASS_THREADS // 72, PASS_THREADS // 72 + 2, 20_001])
def test_as_oh_equals_the_oracle_in_every_dtype(n):
	"""7 281 rows end inside the first grid pass, 7 283 rows start the second (row 7 281 straddles the two)."""
	_, _, s686 = pairs.gather(n, 4000 + n)
	want = torch.from_numpy(orc.as_oh686(s686))
	cube.set_is2024(False)
	x = dev(s686)
	for dtype in (torch.float32, torch.float16, torch.bfloat16):
		got = cube.device.as_oh(x, dtype=dtype)
		assert got.shape == (n, 288)
		assert_rows_equal(got, want.to(dtype).cuda(), f"as_oh {dtype}")


@pytest.mark.parametrize("n", [1, 5, PASS_THREADS // 48, PASS_THREADS // 48 + 1, 30_011])
def test_as_correct_equals_the_oracle(n):
	"""10 922 rows end inside the first grid pass, 10 923 rows start the second (row 10 922 straddles the two)."""
	_, _, s686 = pairs.gather(n, 5000 + n)
	if n > 2:
		s686[n // 2] = orc.SOLVED686
		s686[n - 1] = orc.rotate686(orc.SOLVED686, 3, 1)
	want = orc.as_correct686(s686)
	assert (want == 1).any() and (want == -1).any()                          # both signs occur
	cube.set_is2024(False)
	got = cube.as_correct(dev(s686))
	assert got.shape == (n, 6, 8) and got.dtype == torch.float32
	assert_rows_equal(got, dev(want), "as_correct")


# -------------------------------------------------------------------------------------------------------- k_oh686_from2024
_KINDS = (torch.int8, torch.float32, torch.float16, torch.bfloat16)


def _want686(s686: torch.Tensor, dtype) -> torch.Tensor:
	"""The paired 6x8x6 rows, cast (a plain torch cast of the oracle's rows)."""
	return s686 if dtype == torch.int8 else s686.reshape(len(s686), 288).to(dtype)


@pytest.mark.parametrize("n", [1, 63, 64, 65, N_CONVERT])
def test_to686_equals_the_paired_rows_in_every_output_kind(n, big):
	_, s20, s686 = paired(n, big)
	keep = s20.clone()
	for dtype in _KINDS:                                                     # one after the other: the f32 form of 524 355 rows is 604 MB
		full = guarded(n, (6, 8, 6) if dtype == torch.int8 else (288,), dtype)
		out = cube.device.to686(s20, dtype, out=full)
		assert out is full
		want = _want686(s686, dtype)
		assert_rows_equal(full[:n], want, f"to686 {dtype}")
		assert guard_intact(full)
		fresh = cube.device.to686(s20, dtype)
		assert_rows_equal(fresh, want, f"to686 {dtype}, own output")
		del full, out, want, fresh
	assert torch.equal(s20, keep)


def test_to686_meaningless_rows_leave_their_neighbours_exact(big):
	"""Rows of -1 bytes (what `from686` writes for an illegal row) and rows of codes 24..127 among legal rows, in the first tile, in
	the partial last tile and past the grid cap: the kernel keeps such a code inside its table, the row's content is meaningless and
	nothing is asserted about it; every other row is exact and the guard row untouched."""
	n = N_CONVERT
	s20 = big["s20"].clone()
	rng = np.random.RandomState(24)
	minus = [5, 63, TILE_GRID * TILE + 12, n - 2]
	codes = [0, 40, TILE_GRID * TILE + 13, TILE_GRID * TILE + TILE - 1, n - 1]
	s20[minus] = -1
	s20[codes] = dev(rng.randint(24, 128, (len(codes), 20)).astype(np.int8))
	s20[TILE_GRID * TILE + 30, 7] = 24                                       # one code just past the table in an otherwise legal row
	junk = torch.tensor(sorted(minus + codes + [TILE_GRID * TILE + 30]), device="cuda")
	assert int(junk[-1]) // TILE == n // TILE and n % TILE and int(junk[0]) < TILE
	for dtype in _KINDS:
		full = guarded(n, (6, 8, 6) if dtype == torch.int8 else (288,), dtype)
		cube.device.to686(s20, dtype, out=full)
		want = _want686(big["s686"], dtype)
		full[junk] = want[junk]
		assert_rows_equal(full[:n], want, f"to686 {dtype} around meaningless rows")
		assert guard_intact(full)
		del full, want


# ------------------------------------------------------------------------------------------------------------ k_686_to2024
@pytest.mark.parametrize("n", [1, 63, 64, 65, N_CONVERT])
def test_from686_equals_the_paired_rows(n, big):
	_, s20, s686 = paired(n, big)
	keep = s686.clone()
	full = guarded(n, (20,))
	stats = new_stats()
	out = cube.device.from686(s686, out=full, stats=stats)
	assert out is full
	assert_rows_equal(full[:n], s20, "from686")
	assert stats.tolist() == [0, _ffi.INT64_MAX] and guard_intact(full) and torch.equal(s686, keep)
	assert_rows_equal(cube.device.from686(s686), s20, "from686, checked")
	assert_rows_equal(cube.device.from686(s686.reshape(n, 288), check=False), s20, "from686 of (n, 288), unchecked")


def _expect_illegal(big, rows):
	"""The large input with one illegal kind per row of `rows`; -1 bytes in exactly those rows, counted and located."""
	n = N_CONVERT
	pool686 = pairs.pool()[1]
	s686 = big["s686"].clone()
	for r, kind in rows.items():
		s686[r] = dev(pairs.make_illegal(pool686[big["idx"][r]], kind))
	want = big["s20"].clone()
	want[sorted(rows)] = -1
	assert not bool((big["s20"] == -1).any())
	stats = new_stats()
	full = guarded(n, (20,))
	cube.device.from686(s686, out=full, stats=stats)
	assert stats.tolist() == [len(rows), min(rows)]
	assert_rows_equal(full[:n], want, "from686 with illegal rows")
	assert guard_intact(full)
	assert_rows_equal(cube.device.from686(s686, stats=None, check=False), want, "from686 with illegal rows, unchecked")
	with pytest.raises(ValueError, match=rf"^{len(rows)} of {n} rows .*first is row {min(rows)}\)$"):
		cube.device.from686(s686)


def test_from686_illegal_rows_in_every_tile_position(big):
	"""One row of every kind: at row 0 and row 63 (the ends of the first tile), in the second tile, in the middle, in the last tile
	of the first grid pass, in a tile >= 8 192 (second pass), and as the first and last rows of the partial last tile."""
	n = N_CONVERT
	last = n // TILE * TILE
	at = [0, TILE - 1, TILE, 300_000, TILE_GRID * TILE - 1, TILE_GRID * TILE + 17, last, n - 1]
	assert last // TILE > TILE_GRID and last < n - 1 and len(at) == len(pairs.ILLEGAL_KINDS)
	_expect_illegal(big, dict(zip(at, pairs.ILLEGAL_KINDS)))


def test_from686_first_illegal_row_in_a_tile_visited_late(big):
	"""All illegal rows in tiles >= 8 192, which a workgroup reaches only on its second pass: the smallest index is then reported by a
	late step, after the counts of the partial last tile's neighbours in the grid."""
	n = N_CONVERT
	rows = {TILE_GRID * TILE + 17: "edge_twice", TILE_GRID * TILE + TILE - 1: "one_is_minus1", n // TILE * TILE: "opposite_faces_edge",
	        n - 1: "corner_mirrored"}
	_expect_illegal(big, rows)


def test_illegal_kinds_one_by_one():
	"""Each kind alone in 65 rows (a full tile and one row), so that no kind hides behind another's count."""
	n = TILE + 1
	_, s20, s686 = pairs.gather(n, 77)
	for k, kind in enumerate(pairs.ILLEGAL_KINDS):
		r = (9 * k + 7) % n if k < len(pairs.ILLEGAL_KINDS) - 1 else n - 1
		bad = s686.copy()
		bad[r] = pairs.make_illegal(s686[r], kind)
		want = s20.copy()
		want[r] = -1
		stats = new_stats()
		out = cube.device.from686(dev(bad), stats=stats)
		assert stats.tolist() == [1, r], kind
		assert_rows_equal(out, dev(want), kind)


def test_flipped_edge_and_twisted_corner_are_well_formed():
	"""An edge flipped in place, a corner twisted in place: each cubie still shows once, so the row converts without being counted,
	differs from the untouched row's 20 bytes in exactly that cubie's byte (`flipped20` / `twisted20`, whose pictures the CPU test
	compares with the edited 6x8x6 rows'), and `to686` maps it back to the same 288 bytes."""
	n = TILE + 6
	_, s20, s686 = pairs.gather(n, 99)
	edited, want = s686.copy(), s20.copy()
	rows = [(3 * pos + 1, pos, pairs.flip_edge, pairs.flipped20) for pos in range(12)]
	rows += [(40 + 3 * pos, pos, pairs.twist_corner, pairs.twisted20) for pos in range(7)] + [(n - 1, 7, pairs.twist_corner, pairs.twisted20)]
	assert len({r[0] for r in rows}) == 20
	for r, pos, edit686, edit20 in rows:
		edited[r] = edit686(s686[r], pos)
		want[r] = edit20(s20[r], pos)
		assert (want[r] != s20[r]).sum() == 1
	stats = new_stats()
	e_dev = dev(edited)
	out = cube.device.from686(e_dev, stats=stats)
	assert stats.tolist() == [0, _ffi.INT64_MAX]
	assert_rows_equal(out, dev(want), "from686 of flipped edges and twisted corners")
	assert_rows_equal(cube.device.to686(out), e_dev, "to686 of the converted rows")


# ------------------------------------------------------------------------------------------------------------ host entries
def _zero_copy_max() -> int:
	src = open(os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), "csrc", "rk_api.hip")).read()
	m = re.search(r"constexpr\s+size_t\s+ZERO_COPY_MAX\s*=\s*(\d+)u?\s*<<\s*(\d+)\s*;", src)
	assert m, "ZERO_COPY_MAX not found in rk_api.hip"
	return int(m.group(1)) << int(m.group(2))


def test_host_entries_on_both_sides_of_the_zero_copy_limit():
	"""`cube.as686` stages its 20-byte rows through the page-locked buffer while they fit it (rounded up to 256 bytes); one row more
	goes through a device copy.  `cube.as2024` at the same two sizes, in either current representation."""
	fit = _zero_copy_max() // 256 * 256 // 20
	assert (fit * 20 + 255) // 256 * 256 <= _zero_copy_max() < ((fit + 1) * 20 + 255) // 256 * 256
	for n in (fit, fit + 1):
		_, s20, s686 = pairs.gather(n, n)
		cube.set_is2024(n == fit)
		got686 = cube.as686(s20)
		assert got686.shape == (n, 6, 8, 6) and got686.dtype == np.int8 and np.array_equal(got686, s686), n
		got20 = cube.as2024(s686)
		assert got20.shape == (n, 20) and got20.dtype == np.int8 and np.array_equal(got20, s20), n
	bad = s686[:TILE + 1].copy()
	bad[TILE] = pairs.make_illegal(bad[TILE], "edge_twice")
	with pytest.raises(ValueError, match=rf"first is row {TILE}\)"):
		cube.as2024(bad)


# Every rk_*_host entry at the exact edge of ITS layout.  A host call lays its arrays out at 256-byte steps in declaration order;
# while the total fits ZERO_COPY_MAX it goes through the page-locked buffer, one row more goes through device scratch.  The
# totals below are the layouts of rk_api.hip (its static_asserts pin the arithmetic); the tests assert results only.
def _up256(b: int) -> int:
	return (b + 255) // 256 * 256


def _largest_fit(total) -> int:
	"""The largest n whose layout `total(n)` (nondecreasing) fits ZERO_COPY_MAX."""
	limit = _zero_copy_max()
	lo, hi = 1, limit
	assert total(lo) <= limit < total(hi)
	while hi - lo > 1:
		mid = (lo + hi) // 2
		lo, hi = (mid, hi) if total(mid) <= limit else (lo, mid)
	assert total(lo) <= limit < total(lo + 1), (lo, total(lo), total(lo + 1))
	return lo


def _ptr(a):
	return None if a is None else a.ctypes.data


def _put(row: int, state):
	"""An edit of gather()'s 20-byte rows: `state` at `row`."""
	def edit(s20):
		s20[row] = state
	return edit


def _run_multi_rotate(repr_, n):
	_, s20, s686 = pairs.gather(n, n)
	s = s686 if repr_ else s20
	acts = np.random.RandomState(n).randint(0, 12, n).astype(np.uint8)
	out = np.full_like(s, SENTINEL)
	_ffi.check(_ffi.lib().rk_multi_rotate_host(repr_, _ptr(s), _ptr(acts), _ptr(out), n, None))
	assert np.array_equal(out, c_oracle.multi_rotate686(s, acts) if repr_ else c_oracle.multi_rotate(s, acts)), n


def _run_expand12(n, flags=True, counters=False, edit=None):
	_, s20, _ = pairs.gather(n, n)
	if edit:
		edit(s20)
	want_ch, want_fl = c_oracle.expand12(s20)
	ch, fl, st = np.full((12 * n, 20), SENTINEL, np.int8), np.full(12 * n, SENTINEL, np.uint8), np.full(2, 7, np.int64)
	_ffi.check(_ffi.lib().rk_expand12_host(0, _ptr(s20), _ptr(ch), _ptr(fl if flags else None), _ptr(st if counters else None), n, None))
	assert np.array_equal(ch, want_ch), n
	assert np.array_equal(fl, want_fl) if flags else (fl == SENTINEL).all(), n          # the guard: not passed, not written
	assert st.tolist() == ([int(want_fl.sum()), int(np.argmax(want_fl)) if want_fl.any() else -1] if counters else [7, 7]), n
	return st.tolist()


def _run_is_solved(n, flags=True, counters=False, edit=None):
	_, s20, _ = pairs.gather(n, n)
	if edit:
		edit(s20)
	want = orc.multi_is_solved(s20)
	fl, st = np.full(n, SENTINEL, np.uint8), np.full(2, 7, np.int64)
	_ffi.check(_ffi.lib().rk_multi_is_solved_host(0, _ptr(s20), _ptr(fl if flags else None), _ptr(st if counters else None), n, None))
	assert np.array_equal(fl.astype(bool), want) and fl.max() <= 1 if flags else (fl == SENTINEL).all(), n
	assert st.tolist() == ([int(want.sum()), int(np.argmax(want)) if want.any() else -1] if counters else [7, 7]), n
	return st.tolist()


SEQ_DEPTH = 6


def _run_apply_sequences(games):
	seq = np.random.RandomState(games).randint(0, 12, (SEQ_DEPTH, games)).astype(np.uint8)
	got = np.full((games * SEQ_DEPTH, 20), SENTINEL, np.int8)
	_ffi.check(_ffi.lib().rk_apply_sequences_host(0, _ptr(seq), SEQ_DEPTH, games, 0, 0, _ptr(got), None))
	assert np.array_equal(got, orc.sequence_states(seq // 2, 1 - seq % 2, False)), games


def _run_as_oh(repr_, n):
	_, s20, s686 = pairs.gather(n, n)
	oh = torch.full((n, 288 if repr_ else 480), float(SENTINEL), dtype=torch.float32, device="cuda")
	_ffi.check(_ffi.lib().rk_as_oh_host(repr_, _ptr(s686 if repr_ else s20), oh.data_ptr(), _ffi.OH_F32, n, None))
	assert np.array_equal(oh.cpu().numpy(), orc.as_oh686(s686) if repr_ else c_oracle.as_oh(s20)), n


def _run_oh686_from2024(n):
	_, s20, s686 = pairs.gather(n, n)
	oh = torch.full((n, 288), float(SENTINEL), dtype=torch.float32, device="cuda")
	_ffi.check(_ffi.lib().rk_oh686_from2024_host(_ptr(s20), oh.data_ptr(), _ffi.OH_F32, n, None))
	assert np.array_equal(oh.cpu().numpy(), orc.as_oh686(s686)), n


def _run_686_to2024(n):
	_, s20, s686 = pairs.gather(n, n)
	out, st = np.full((n, 20), SENTINEL, np.int8), np.full(2, 7, np.int64)
	_ffi.check(_ffi.lib().rk_686_to2024_host(_ptr(s686), _ptr(out), _ptr(st), n, None))
	assert np.array_equal(out, s20) and st.tolist() == [0, _ffi.INT64_MAX], n             # the raw counters: no illegal row


#: entry -> (its layout's total bytes at n rows, the call checked against the oracle at n rows)
HOST_ENTRIES = {
	"multi_rotate-2024": (lambda n: 2 * _up256(20 * n) + _up256(n), lambda n: _run_multi_rotate(0, n)),
	"multi_rotate-686": (lambda n: 2 * _up256(288 * n) + _up256(n), lambda n: _run_multi_rotate(1, n)),
	"expand12": (lambda n: _up256(20 * n) + _up256(240 * n) + _up256(12 * n), _run_expand12),
	"multi_is_solved": (lambda n: _up256(20 * n) + _up256(n), _run_is_solved),
	"apply_sequences": (lambda g: _up256(SEQ_DEPTH * g) + _up256(g * SEQ_DEPTH * 20), _run_apply_sequences),
	"as_oh-2024": (lambda n: _up256(20 * n), lambda n: _run_as_oh(0, n)),
	"as_oh-686": (lambda n: _up256(288 * n), lambda n: _run_as_oh(1, n)),
	"oh686_from2024": (lambda n: _up256(20 * n), _run_oh686_from2024),
	"686_to2024": (lambda n: _up256(288 * n) + _up256(20 * n), _run_686_to2024),        # always staged (it counts): same results at both
}


@pytest.mark.parametrize("entry", list(HOST_ENTRIES))
def test_every_host_entry_at_its_own_zero_copy_limit(entry):
	"""The largest call that fits the page-locked buffer and the one a row (a game) larger, byte for byte against the oracle."""
	total, run = HOST_ENTRIES[entry]
	fit = _largest_fit(total)
	for n in (fit, fit + 1):
		run(n)


@pytest.mark.parametrize("entry", ["expand12", "multi_is_solved"])
def test_host_counters_and_null_flags_at_the_zero_copy_limit(entry):
	"""With the counters (always through device memory) and without the flag output, at the same two sizes: `[1, index]` with one
	solved row (one solved child) at a known index, `[0, -1]` with none; flags that are not asked for are not written."""
	total, run = HOST_ENTRIES[entry]
	fit = _largest_fit(total)
	for n in (fit, fit + 1):
		row = n - 3
		if entry == "expand12":                         # one quarter turn from solved: of its 12 children, the one by the opposite turn
			edit, index = _put(row, orc.rotate(orc.SOLVED, 4, 0)), 12 * row + 8
		else:
			edit, index = _put(row, orc.SOLVED), row
		assert run(n, counters=True) == [0, -1]
		assert run(n, counters=True, edit=edit) == [1, index]
		assert run(n, flags=False, counters=True, edit=edit) == [1, index]
		run(n, flags=False)


def test_host_entries_in_any_order_share_the_buffer_and_the_slots():
	"""The pinned buffer and the cached scratch slots are per thread and shared by all entries: a large staged call, a small
	zero-copy one, a large call of another entry (other slot sizes), and back -- each against the oracle."""
	above = {e: _largest_fit(HOST_ENTRIES[e][0]) + 1 for e in ("multi_rotate-2024", "expand12", "multi_is_solved", "as_oh-686")}
	_run_multi_rotate(0, above["multi_rotate-2024"])
	_run_is_solved(12)
	_run_expand12(above["expand12"])
	_run_multi_rotate(0, 1)
	_run_is_solved(above["multi_is_solved"], counters=True, edit=_put(5, orc.SOLVED))
	_run_expand12(1, flags=False)
	_run_as_oh(1, above["as_oh-686"])
	_run_apply_sequences(3)
	_run_686_to2024(above["expand12"])
	_run_multi_rotate(1, 7)


def test_host_entries_with_nothing_to_do_and_with_null_pointers():
	"""n = 0 returns 0 before any pointer is looked at; a null array with n > 0 is refused with -1."""
	lib = _ffi.lib()
	_, s20, s686 = pairs.gather(3, 3)
	acts, out20, out686 = np.zeros(SEQ_DEPTH * 3, np.uint8), np.empty((SEQ_DEPTH * 3, 20), np.int8), np.empty_like(s686)
	ch, st = np.empty((36, 20), np.int8), np.zeros(2, np.int64)
	oh = torch.empty((3, 480), dtype=torch.float32, device="cuda")
	for n, a, b, want in ((0, None, None, 0), (3, None, _ptr(out20), -1), (3, _ptr(s20), None, -1)):
		assert lib.rk_multi_rotate_host(0, a, _ptr(acts), b, n, None) == want
		assert lib.rk_multi_rotate_host(1, a and _ptr(s686), _ptr(acts), b and _ptr(out686), n, None) == want
		assert lib.rk_expand12_host(0, a, b and _ptr(ch), None, None, n, None) == want
		assert lib.rk_apply_sequences_host(0, a and _ptr(acts), SEQ_DEPTH, n, 0, 0, b, None) == want
		assert lib.rk_as_oh_host(0, a, b and oh.data_ptr(), _ffi.OH_F32, n, None) == want
		assert lib.rk_oh686_from2024_host(a, b and oh.data_ptr(), _ffi.OH_F32, n, None) == want
		assert lib.rk_686_to2024_host(a and _ptr(s686), b, None, n, None) == want
	assert lib.rk_multi_rotate_host(0, _ptr(s20), None, _ptr(out20), 3, None) == -1
	assert lib.rk_multi_is_solved_host(0, None, None, None, 0, None) == 0 and lib.rk_multi_is_solved_host(0, None, None, None, 3, None) == -1
	st[:] = 7
	assert lib.rk_multi_is_solved_host(0, None, None, _ptr(st), 0, None) == 0 and st.tolist() == [0, -1]     # the counters of an empty call
	st[:] = 7
	assert lib.rk_expand12_host(0, None, None, None, _ptr(st), 0, None) == 0 and st.tolist() == [0, -1]
