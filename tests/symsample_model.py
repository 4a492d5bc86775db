"""
Unranking the symmetry ball (`DeviceSymBall.state_at`, engine rk_symball_state_at) and the exact depths around a state
(`DeviceSymBall.child_depths`, engine rk_symball_child_depths) restated in plain NumPy on top of tests/sym_model.py.  A helper for
tests/test_symsample_*.py, not a test module.

The state of (d, r): the nodes of level d in index order, each counting for the size of its orbit; j is the node whose cumulative
range holds r, k = r minus the sizes in front of j, and the state is the k-th DISTINCT conjugate of j's representative in
ascending symmetry order -- conj_s for s = 0 .. 47, a conjugate that a lower symmetry gave already left out.

child_depths knows nothing of balls, radii or parity: it looks the state and its twelve children (action order) up in a table of
true distances, -1 for what the table does not hold.
"""
import numpy as np

from oracle import cube_oracle as orc
from tests import sym_model

N_SYM = sym_model.N_SYM


def orbits(reps: np.ndarray):
	"""(conj int8 (48, n, 20), first bool (48, n)): all conjugates of every representative, and which of them no lower symmetry gives"""
	conj = sym_model.all_conjugates(np.ascontiguousarray(reps, np.int8).reshape(-1, 20))
	first = np.ones(conj.shape[:2], bool)
	for s in range(1, N_SYM):
		for t in range(s):
			first[s] &= (conj[t] != conj[s]).any(axis=1)
	return conj, first


def state_at(reps: np.ndarray, level_start: np.ndarray, depth, rank) -> np.ndarray:
	"""int8 (n, 20).  reps (len, 20): row i = node i + 1; level_start (radius + 2,); depth an int or (n,), rank (n,), all in range."""
	rank = np.asarray(rank, np.int64).reshape(-1)
	depth = np.broadcast_to(np.asarray(depth, np.int64), rank.shape)
	level_start = np.asarray(level_start, np.int64)
	conj, first = orbits(reps)
	size = first.sum(axis=0).astype(np.int64)
	cum = np.concatenate([[0], np.cumsum(size)])                    # cum[p]: the orbit sizes of the nodes 1 .. p
	base = cum[level_start - 1]                                      # ... of the nodes below each level
	assert ((0 <= depth) & (depth <= len(level_start) - 2)).all()
	assert ((0 <= rank) & (rank < (base[1:] - base[:-1])[depth])).all()
	g = base[depth] + rank
	p = np.searchsorted(cum, g, side="right") - 1                   # node - 1
	k = g - cum[p]
	order = np.argsort(~first, axis=0, kind="stable")               # column p: its first symmetries in ascending order, then the others
	return conj[order[k, p], p]


def level_sizes(reps: np.ndarray, level_start: np.ndarray) -> np.ndarray:
	"""The orbit sizes of every level added up"""
	_, first = orbits(reps)
	cum = np.concatenate([[0], np.cumsum(first.sum(axis=0).astype(np.int64))])
	return np.diff(cum[np.asarray(level_start, np.int64) - 1])


def child_depths(plain_depth_lookup: dict, states: np.ndarray):
	"""(depth int64 (n,), children int64 (n, 12)) from a table {20 state bytes: true distance to solved}; -1 for a state it lacks"""
	x = np.ascontiguousarray(states, np.int8).reshape(-1, 20)
	sub = np.ascontiguousarray(orc.expand12(x), np.int8)
	own = np.array([plain_depth_lookup.get(r.tobytes(), -1) for r in x], np.int64)
	kids = np.array([plain_depth_lookup.get(r.tobytes(), -1) for r in sub], np.int64).reshape(len(x), 12)
	return own, kids


def targets(depth: np.ndarray, children: np.ndarray, g: float):
	"""(policy int64, value float32) of `ball_traindata` from exact depths: the lowest action whose child lies one level nearer (0 at
	depth 0); V*(0) = 0, V*(d) = g - (d - 1)"""
	depth = np.asarray(depth, np.int64)
	nearer = np.asarray(children, np.int64) == (depth - 1)[:, None]
	assert nearer.any(axis=1)[depth > 0].all()
	policy = nearer.argmax(axis=1).astype(np.int64)
	value = np.where(depth == 0, np.float32(0), np.float32(g) - (depth - 1).astype(np.float32)).astype(np.float32)
	return policy, value
