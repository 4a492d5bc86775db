"""
Pattern databases on the device (engine rk_pdb_*, `DevicePatternDB`) against the NumPy model of tests/pdb_model.py: whole tables bit
for bit for five small patterns, `depth` and `solve` row for row with every word replayed, the all-corners table (too big for the
model) by its own invariants, against the goal ball and against a dictionary search, `lower_bound`, rows that are no partial
pattern (answered -1 before any table access, their neighbours untouched), the shapes and the refusals.
"""
import functools

import numpy as np
import pytest
import torch

from librubiks_amd import cube
from librubiks_amd.cube import maps
from librubiks_amd.solving.agents import DeviceGoalBall, DevicePatternDB
from tests import pdb_model as M
from tests import side_stream as S

pytestmark = pytest.mark.gpu

orc = M.orc
CROSS_D = tuple(sorted(int(e) for e in orc._FACES[3][1]))
PATTERNS = {"corner": ((5,), ()), "edge": ((), (7,)), "corners3": ((0, 3, 6), ()), "cross": ((), CROSS_D), "mixed": ((1, 6), (2, 9))}
BASE = 4096


@functools.lru_cache(maxsize=None)
def _model(name):
	p = M.Pattern(*PATTERNS[name])
	table, sizes = p.table()
	return p, table, sizes


@functools.lru_cache(maxsize=None)
def _db(name):
	return DevicePatternDB(*PATTERNS[name]).build()


@functools.lru_cache(maxsize=None)
def _corners():
	return DevicePatternDB.corners().build()


@functools.lru_cache(maxsize=None)
def _scrambles():
	"""BASE legal states, 0..40 seeded moves deep in turn"""
	return S.mixed_depths(BASE, 40, 25_001)


@functools.lru_cache(maxsize=None)
def _ball5():
	"""(states, depths) of every state within 5 quarter turns of solved"""
	ball = DeviceGoalBall(5)
	states = ball.arrays()[0]
	return states, ball.depth(states)


def _replay(states, lengths, actions) -> np.ndarray:
	"""the states after each row's word"""
	s = np.array(states, np.int8)
	for t in range(actions.shape[1]):
		live = np.nonzero(lengths > t)[0]
		if len(live):
			a = actions[live, t].astype(np.int64)
			assert ((a >= 0) & (a < 12)).all()
			s[live] = cube.multi_rotate(s[live], a // 2, 1 - a % 2)
	assert (np.where(np.arange(actions.shape[1])[None, :] >= np.maximum(lengths, 0)[:, None], actions, -1) == -1).all()     # padded with -1
	return s


@pytest.mark.parametrize("name", list(PATTERNS))
def test_whole_table_against_the_model(name):
	(p, table, sizes), db = _model(name), _db(name)
	assert db.size == p.size == len(db) and db.built
	assert db.level_sizes.tolist() == sizes.tolist() and db.levels == len(sizes) and db.max_depth == len(sizes) - 1
	got = db.table()
	assert got.dtype == np.uint8 and got.shape == (p.size,) and (got == table).all()
	assert db.build() is db and (db.table() == table).all()             # idempotent


def test_sizes_and_the_cross_from_the_face_definitions():
	assert _db("mixed").size == 266_112 and _db("cross").size == 190_080
	cross = DevicePatternDB.cross("D")
	assert cross.edge_cubies == CROSS_D == tuple(sorted(int(e) for e in maps._FACES[3, 4:8])) and cross.corner_cubies == ()
	assert DevicePatternDB.cross(3).edge_cubies == CROSS_D and DevicePatternDB.cross("F").edge_cubies == tuple(sorted(orc._FACES[0][1]))


@pytest.mark.parametrize("name", ["cross", "mixed"])
def test_depth_and_solve_against_the_model(name):
	(p, table, sizes), db, s = _model(name), _db(name), _scrambles()
	want_depth = p.depth(table, s)
	want_len, want_act = p.solve(table, s, db.max_depth)
	depth = db.depth(s)
	lengths, actions = db.solve(s)
	assert depth.dtype == np.int32 and lengths.dtype == np.int32 and actions.dtype == np.int8 and actions.shape == (BASE, db.max_depth)
	assert (depth == want_depth).all() and (lengths == want_len).all() and (actions == want_act).all()
	assert (lengths == depth).all() and depth.min() == 0 and depth.max() >= 2
	end = _replay(s, lengths, actions)
	assert (p.select(end) == p.goal[None]).all()                        # every word brings the selected cubies home


def test_all_corners_builds_and_is_consistent():
	db = _corners()
	assert db.size == 88_179_840 == int(db.level_sizes.sum()) and db.level_sizes[0] == 1 and db.level_sizes[1] == 12
	table = db.table()
	assert not (table == 255).any() and int(table.max()) == db.max_depth
	assert (np.bincount(table, minlength=db.levels) == db.level_sizes).all()
	# 2^20 seeded scrambles, made on the device
	n, rs = 1 << 20, np.random.RandomState(25_002)
	s = torch.from_numpy(orc.repeat_state(orc.SOLVED, n)).cuda()
	for _ in range(40):
		a = rs.randint(0, 12, n)
		s = cube.multi_rotate(s, torch.from_numpy(a // 2).cuda(), torch.from_numpy(1 - a % 2).cuda())
	depth = db.depth(s)
	assert isinstance(depth, torch.Tensor) and depth.dtype == torch.int32 and int(depth.min()) >= 0
	child = db.depth(cube.expand(s)).reshape(n, 12)
	assert int((child - depth[:, None]).abs().max()) <= 1
	assert bool(((child == depth[:, None] - 1).any(dim=1) | (depth == 0)).all())


def test_all_corners_against_the_ball_and_a_dictionary_search():
	db, (states, ball_depth) = _corners(), _ball5()
	depth = db.depth(states)
	assert (ball_depth >= 0).all() and (depth >= 0).all() and (depth <= ball_depth).all()
	p = M.Pattern(range(8), ())
	dist = M.dictionary_bfs(p, limit=6)
	assert max(dist.values()) == 6
	rows = np.concatenate([states, _scrambles()])
	got = db.depth(rows)
	want = np.array([dist.get(t, -1) for t in map(tuple, p.select(rows).tolist())])
	assert ((got == want) | ((want < 0) & (got > 6))).all()
	assert (want[:len(states)] >= 0).all() and (want[len(states):] < 0).any()       # both branches are taken
	# the index itself, last twist left out, is the model's: the exported table read at the model's rank is what depth answers, and
	# holds the dictionary's distance at the model's rank of every placement within 6 moves
	table = db.table()
	assert (table[p.rank(p.select(rows))] == got).all()
	keys = np.array(list(dist), np.int64)
	assert (table[p.rank(keys)] == np.array(list(dist.values()))).all()


def test_lower_bound():
	(states, ball_depth), dbs = _ball5(), [_corners(), _db("cross")]
	low = DevicePatternDB.lower_bound(states, dbs)
	assert low.dtype == np.int32 and (low == np.maximum(dbs[0].depth(states), dbs[1].depth(states))).all()
	assert (low >= 0).all() and (low <= ball_depth).all()
	assert (np.nonzero(low == 0)[0] == np.nonzero(ball_depth == 0)[0]).all() and (ball_depth == 0).sum() == 1
	on_device = DevicePatternDB.lower_bound(torch.from_numpy(states).cuda(), dbs)
	assert isinstance(on_device, torch.Tensor) and (on_device.cpu().numpy() == low).all()
	with pytest.raises(ValueError):
		DevicePatternDB.lower_bound(states, [])


def test_invalid_rows_get_minus_one_and_their_neighbours_are_untouched():
	"""The kernel validates before it indexes: a row whose SELECTED codes are no partial pattern is answered -1 and reads no table
	entry; a row that is garbage only in unselected bytes gets the legal answer."""
	(p, table, sizes), db = _model("mixed"), _db("mixed")
	s = np.array(_scrambles()[:256])
	legal = s.copy()
	c0, c1, e0, e1 = p.columns                                          # cubies 1 and 6, bytes 8 + 2 and 8 + 9
	bad = {}
	for k, v in enumerate((24, 127, -1, -128)):
		s[10 + 2 * k, c1] = v
		s[11 + 2 * k, e0] = v
		bad[10 + 2 * k] = bad[11 + 2 * k] = True
	s[40, e1] = s[40, e0] ^ 1                                           # two selected edges on one position
	s[41, e1] = s[41, e0]
	s[42, c1] = s[42, c0] // 3 * 3 + (s[42, c0] + 1) % 3                # two selected corners on one position
	bad.update({40: True, 41: True, 42: True})
	others = np.setdiff1d(np.arange(20), p.columns)
	for k, v in enumerate((99, -7, 24, -128)):
		s[60 + k][others] = v                                           # garbage in unselected bytes only
	s[64, others] = s[64, others[0]]
	depth = db.depth(s)
	lengths, actions = db.solve(s)
	want = p.depth(table, legal)
	want_len, want_act = p.solve(table, legal, db.max_depth)
	rows = np.array(sorted(bad))
	assert (depth[rows] == -1).all() and (lengths[rows] == -1).all() and (actions[rows] == -1).all()
	good = np.setdiff1d(np.arange(len(s)), rows)
	assert (depth[good] == want[good]).all() and (lengths[good] == want_len[good]).all() and (actions[good] == want_act[good]).all()
	assert (p.depth(table, s) == depth).all()                           # the model reads the rows the same way


def test_shapes_and_representations():
	(p, table, sizes), db, base = _model("cross"), _db("cross"), _scrambles()
	want = p.depth(table, base)
	want_len, want_act = p.solve(table, base, db.max_depth)
	# n = 0 and n = 1
	assert db.depth(np.zeros((0, 20), np.int8)).shape == (0,)
	l0, a0 = db.solve(np.zeros((0, 20), np.int8))
	assert l0.shape == (0,) and a0.shape == (0, db.max_depth)
	assert db.depth(base[7:8]).tolist() == [want[7]] and db.solve(base[7:8])[1].tolist() == [want_act[7].tolist()]
	# three rows past a full pass of the capped grid: one thread takes two rows
	n = DevicePatternDB.GRID_ROWS + 3
	pick = np.arange(n) % BASE
	big = torch.from_numpy(base[pick]).cuda()
	depth = db.depth(big)
	lengths, actions = db.solve(big)
	assert isinstance(depth, torch.Tensor) and isinstance(lengths, torch.Tensor) and actions.dtype == torch.int8
	assert (depth.cpu().numpy() == want[pick]).all() and (lengths.cpu().numpy() == want_len[pick]).all()
	assert (actions.cpu().numpy() == want_act[pick]).all()
	# a slice of a larger tensor that starts 4 bytes in
	flat = torch.zeros(20 * BASE + 8, dtype=torch.int8, device="cuda")
	flat[4:4 + 20 * BASE] = torch.from_numpy(base).cuda().reshape(-1)
	view = flat[4:4 + 20 * BASE].view(BASE, 20)
	assert view.data_ptr() % 16 == 4
	assert (db.depth(view).cpu().numpy() == want).all() and (db.solve(view)[1].cpu().numpy() == want_act).all()
	# numpy in -> numpy out
	assert isinstance(db.depth(base), np.ndarray) and (db.depth(base) == want).all()
	# 6x8x6 mode gives the same answers
	s686 = cube.as686(base[:512])
	cube.set_is2024(False)
	try:
		assert (db.depth(s686) == want[:512]).all()
		l6, a6 = db.solve(torch.from_numpy(s686).cuda())
		assert (l6.cpu().numpy() == want_len[:512]).all() and (a6.cpu().numpy() == want_act[:512]).all()
	finally:
		cube.set_is2024(True)


def test_refusals():
	for kwargs in ({}, {"corners": (1, 1)}, {"edges": (3, 4, 3)}, {"edges": range(11)}, {"corners": range(8), "edges": (0, 1)}, {"corners": (8,)},
	               {"edges": (-1,)}, {"corners": (True,)}):
		with pytest.raises(ValueError):
			DevicePatternDB(**kwargs)
	with pytest.raises(ValueError):
		DevicePatternDB.cross("X")
	db = DevicePatternDB(corners=(2,))
	for query in (db.depth, db.solve, lambda s: db.table(), lambda s: db.level_sizes):
		with pytest.raises(ValueError):
			query(_scrambles()[:4])
	assert len(db) == 24 and not db.built
	assert db.build().depth(orc.SOLVED[None]).tolist() == [0]
	db._free()                                                          # the table is gone: queries ask for a build again
	assert not db.built
	with pytest.raises(ValueError):
		db.depth(orc.SOLVED[None])
	assert db.build().depth(orc.SOLVED[None]).tolist() == [0]


def test_the_engine_refuses_on_its_own():
	"""The entries' own checks, past the Python class: RK_EINVAL (-1) from rk_pdb_create with nothing made, RK_ESTATE (-4) from a
	query, export or solve on a handle that is not built, RK_EINVAL from a solve without an action buffer with nothing enqueued."""
	import ctypes as C
	from librubiks_amd import _ffi
	lib = _ffi.lib()

	def create(corners, edges, out=True):
		h = C.c_void_p()
		c, e = np.array(corners, np.uint8), np.array(edges, np.uint8)
		rc = lib.rk_pdb_create(C.byref(h) if out else None, c.ctypes.data if len(c) else None, len(c), e.ctypes.data if len(e) else None, len(e))
		return rc, h

	for corners, edges, word in (((), (), b"empty"), ((3, 1), (), b"ascend"), ((2, 2), (), b"ascend"), ((), (0, 12), b"outside"), ((8,), (), b"outside"),
	                             ((), tuple(range(11)), b"parity"), ((), tuple(range(12)), b"parity"), (tuple(range(8)), (0, 1), b"more than"),
	                             ((), tuple(range(8)), b"more than"), ((), tuple(range(10)), b"more than")):
		rc, h = create(corners, edges)
		assert rc == -1 and h.value is None and word in lib.rk_last_error(), (corners, edges, lib.rk_last_error())
	assert create((1,), (), out=False)[0] == -1
	assert lib.rk_pdb_create(C.byref(C.c_void_p()), None, 9, None, 0) == -1 and lib.rk_pdb_create(C.byref(C.c_void_p()), None, 2, None, 0) == -1
	rc, h = create((1,), (4,))
	assert rc == 0 and h.value
	try:
		q = torch.from_numpy(_scrambles()[:8]).cuda()
		out = torch.full((8,), 77, dtype=torch.int32, device="cuda")
		actions = torch.full((8, 16), 77, dtype=torch.int8, device="cuda")
		err = torch.full((1,), 77, dtype=torch.int32, device="cuda")
		status = (C.c_longlong * 64)()
		assert lib.rk_pdb_status(h, status) == 0 and list(status[:5]) == [0, 24 * 24, 1, 1, 0]
		assert lib.rk_pdb_depth(h, q.data_ptr(), 8, out.data_ptr(), None) == -4 and b"build" in lib.rk_last_error()
		assert lib.rk_pdb_solve(h, q.data_ptr(), 8, out.data_ptr(), actions.data_ptr(), err.data_ptr(), None) == -4
		assert lib.rk_pdb_export(h, 0, 1, np.zeros(1, np.uint8).ctypes.data, None) == -4
		assert lib.rk_pdb_build(None, None) == -1 and lib.rk_pdb_status(None, status) == -1
		assert lib.rk_pdb_build(h, _ffi.stream_ptr()) == 0 and lib.rk_pdb_build(h, _ffi.stream_ptr()) == 0
		assert lib.rk_pdb_status(h, status) == 0 and status[0] == 1 and sum(status[5:5 + status[4]]) == 24 * 24 and status[5] == 1
		# refused calls enqueue nothing: the error word keeps its 77
		assert lib.rk_pdb_solve(h, q.data_ptr(), 8, out.data_ptr(), None, err.data_ptr(), _ffi.stream_ptr()) == -1
		assert lib.rk_pdb_solve(h, q.data_ptr(), 8, out.data_ptr(), actions.data_ptr(), None, _ffi.stream_ptr()) == -1
		assert lib.rk_pdb_depth(h, q.data_ptr() + 1, 8, out.data_ptr(), _ffi.stream_ptr()) == -1 and b"aligned" in lib.rk_last_error()
		assert lib.rk_pdb_depth(h, None, 8, out.data_ptr(), _ffi.stream_ptr()) == -1
		assert lib.rk_pdb_depth(h, q.data_ptr(), (1 << 31), out.data_ptr(), _ffi.stream_ptr()) == -1
		assert lib.rk_pdb_export(h, 24 * 24, 1, np.zeros(1, np.uint8).ctypes.data, _ffi.stream_ptr()) == -1
		torch.cuda.synchronize()
		assert err.tolist() == [77] and (out == 77).all() and (actions == 77).all()
		assert lib.rk_pdb_depth(h, None, 0, None, _ffi.stream_ptr()) == 0     # n = 0 does nothing
	finally:
		assert lib.rk_pdb_destroy(h) == 0
