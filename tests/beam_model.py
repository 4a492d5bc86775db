"""
DeviceBeamSearch (engine rk_beam_*) restated in plain Python / NumPy over the oracle's cube arithmetic: what the engine has to
reproduce bit for bit.  A helper for tests/test_beam_*.py, not a test module.

Depth t holds a beam F_t of m_t <= B states in a fixed order, F_0 the start; child c = 12 i + a is member i under action a.
  1. live      with prune_inverse, child (i, a) is dead when a == (the action that made member i) ^ 1
  2. budget    explored + n_live > max_states stops with status 2, else explored += n_live
  3. win       the live child that is solved -- with a ball: that the ball holds -- with the least (ball depth, c): status 1; the
               queue is the path to member i, then a, then the ball's descent (the lowest action that gets one level nearer)
  4. dedup     of live children with equal states the lowest c survives (nothing across depths)
  5. select    the best min(B, survivors): larger value first, any NaN above every number, -0.0 == +0.0, ties to the lower c;
               F_{t+1} is stored in ASCENDING c, back[t + 1][j] = i << 4 | a
  6. depth     t + 1 == max_depth stops with status 3
`depth` counts the depths whose children were counted, `sizes` the beams formed (m_0 ..).

The ball is a dict from canonical state to depth.  In a COMPLETE ball of radius R every hit of a search has ball depth R: a beam
member lies at distance > R (else it had been a hit itself) and a quarter turn changes the distance by one.  Hits at different
ball depths -- what the rule "least (ball depth, c)" is for -- therefore need a ball with holes, and since all members of a beam lie
at distances of one parity, a hole two levels inside the rim: BallModel(radius, thin=seed) drops one orbit of level radius - 1 and
every orbit further out that is left without a child one level nearer (so that every descent still finds its way).  A start one
move outside the hole is not recognised; at the next depth the hole's children hit at levels radius - 2 and radius together.
The device ball is always complete, so those cases are the model's alone.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import cube_oracle as orc
from tests import sym_model

DEFECTS = ("last_maximum", "dedup_highest", "rank_order", "nan_lowest", "win_lowest_c")
KINDS = ("tie_cut", "duplicates", "nan_inf", "short_beam", "multi_hit")

Result = namedtuple("Result", "solved status depth explored sizes back meeting queue kinds")


class BallModel:
	"""canonical state -> depth for the states within `radius` quarter turns of solved; `thin`: a seed, the ball gets a hole (see above)"""
	def __init__(self, radius: int, thin: int = None):
		ball = sym_model.build(radius)
		self.radius = radius
		self.level = {}
		for node in range(1, ball.len + 1):
			self.level[ball.states[node - 1].tobytes()] = int(np.searchsorted(ball.level_start, node, side="right") - 1)
		self.hole = None
		if thin is not None:
			inner = sorted(k for k, v in self.level.items() if v == radius - 1)
			hole = inner[np.random.RandomState(thin).randint(len(inner))]
			self.hole = np.frombuffer(hole, np.int8).copy()
			del self.level[hole]
			for k in sorted(k for k, v in self.level.items() if v == radius):            # (level radius only: the hole is one level below)
				if not (self.depth(orc.expand12(np.frombuffer(k, np.int8)[None])) == radius - 1).any():
					del self.level[k]

	def depth(self, states20: np.ndarray) -> np.ndarray:
		reps, _, _ = sym_model.canonical(np.asarray(states20, np.int8).reshape(-1, 20))
		return np.array([self.level.get(r.tobytes(), -1) for r in reps], np.int64)

	def descend(self, state20: np.ndarray) -> list:
		x, out = np.array(state20, np.int8), []
		d = int(self.depth(x)[0])
		while d > 0:
			nearer = np.nonzero(self.depth(orc.expand12(x[None])) == d - 1)[0]
			a = int(nearer[0])
			out.append(a)
			x = orc.expand12(x[None])[a]
			d -= 1
		return out


@functools.lru_cache(maxsize=None)
def ball_model(radius: int, thin: int = None) -> BallModel:
	return BallModel(radius, thin)


def values_of(net):
	"""children (n, 20) -> float32 (n,): the value head of a net that takes NumPy one-hot batches"""
	return lambda states20, twin=None: np.asarray(net(orc.as_oh(states20), policy=False, value=True), np.float32).reshape(-1)


def values_of686(net):
	"""the same for a torch net of the 6x8x6 representation, evaluated on the CPU on the twin states"""
	import torch

	def f(states20, twin):
		with torch.no_grad():
			return net(torch.from_numpy(orc.as_oh686(twin)), policy=False, value=True).reshape(-1).float().numpy()
	return f


def _rank_key(v: np.float32, c: int, defect):
	nan = bool(np.isnan(v))
	cls = (2 if defect == "nan_lowest" else 0) if nan else 1
	return (cls, 0.0 if nan else -(float(v) + 0.0), -c if defect == "last_maximum" else c)


def _path(back: list, t: int, i: int) -> list:
	acts = []
	for tt in range(t, 0, -1):
		w = int(back[tt][i])
		acts.append(w & 15)
		i = w >> 4
	assert i == 0
	return acts[::-1]


def search(values, start20, width: int, max_depth: int = 64, ball: BallModel = None, prune_inverse: bool = True, max_states: int = None,
           defect: str = None, start686=None) -> Result:
	assert defect is None or defect in DEFECTS
	start = np.asarray(start20, np.int8).reshape(20)
	kinds = dict.fromkeys(KINDS, 0)
	sizes, back = [1], [None]
	if orc.is_solved(start):
		return Result(True, 1, 0, 0, sizes, back, None, [], kinds)
	if ball is not None and ball.depth(start)[0] >= 0:
		return Result(True, 1, 0, 0, sizes, back, (0, -1, int(ball.depth(start)[0])), ball.descend(start), kinds)
	beam, last = start[None].copy(), np.array([-1])
	twin = None if start686 is None else np.asarray(start686, np.int8)[None].copy()
	explored, t = 0, 0
	while True:
		m = len(beam)
		kinds["short_beam"] += m < width
		children = orc.expand12(beam)
		c_all = np.arange(12 * m)
		i_of, a_of = c_all // 12, c_all % 12
		children_twin = None
		if twin is not None:
			children_twin = orc.multi_rotate686(np.repeat(twin, 12, axis=0), a_of // 2, 1 - a_of % 2)
		live = np.ones(12 * m, bool)
		if prune_inverse:
			live &= ~((last[i_of] >= 0) & (a_of == (last[i_of] ^ 1)))
		n_live = int(live.sum())
		if max_states is not None and explored + n_live > max_states:
			return Result(False, 2, t, explored, sizes, back, None, [], kinds)
		explored += n_live
		lc = c_all[live]
		if ball is not None:
			lv = ball.depth(children[lc])
			hits = [(int(l), int(c)) for l, c in zip(lv, lc) if l >= 0]
		else:
			hits = [(0, int(c)) for c in lc[orc.multi_is_solved(children[lc])]]
		if hits:
			kinds["multi_hit"] += len({l for l, _ in hits}) > 1
			l, c = min(hits, key=(lambda h: h[1]) if defect == "win_lowest_c" else None)
			i, a = c // 12, c % 12
			queue = _path(back, t, i) + [a] + (ball.descend(children[c]) if ball is not None else [])
			return Result(True, 1, t + 1, explored, sizes, back, (i, a, l), queue, kinds)
		first = {}
		for c in (lc[::-1] if defect == "dedup_highest" else lc):
			first.setdefault(children[c].tobytes(), int(c))
		surv = sorted(first.values())
		kinds["duplicates"] += len(surv) < n_live
		v = values(children, children_twin)
		lvals = v[lc]
		kinds["nan_inf"] += bool(np.isnan(lvals).any() and np.isposinf(lvals).any() and np.isneginf(lvals).any())
		ranked = sorted(surv, key=lambda c: _rank_key(v[c], c, defect))
		if len(ranked) > width:
			kinds["tie_cut"] += _rank_key(v[ranked[width - 1]], 0, None) == _rank_key(v[ranked[width]], 0, None)
		chosen = ranked[:width]
		order = np.array(chosen if defect == "rank_order" else sorted(chosen), np.int64)
		beam, last = children[order], a_of[order]
		if twin is not None:
			twin = children_twin[order]
		back.append((i_of[order] << 4) | a_of[order])
		sizes.append(len(order))
		t += 1
		if t == max_depth:
			return Result(False, 3, t, explored, sizes, back, None, [], kinds)


def apply(start20, queue) -> np.ndarray:
	x = np.array(start20, np.int8)
	for a in queue:
		x = orc.rotate(x, a // 2, 1 - a % 2)
	return x


# ---- the nets and the cases that the CPU and the GPU tests share ----------------------------------------------------------------
WIDTHS = (1, 5, 6, 22, 342, 1366)
NET_NAMES = ("lookup", "lookup_bf16", "lookup_special", "linear_bf16", "noisy")
_NETS = {}


def net_of(name: str):
	"""Made once per process; the special net gets rows of NaN on top of plant_adi_rows' +-inf before its first use."""
	if name not in _NETS:
		from oracle.search_oracle import LookupNet, NoisyStubNet
		from tests.adi_nets import LinearLookupNet, plant_adi_rows
		if name == "lookup":
			net = plant_adi_rows(LookupNet(seed=60), 1060)
		elif name == "lookup_bf16":
			net = plant_adi_rows(LookupNet(seed=61, dtype="bfloat16"), 1061)
		elif name == "lookup_special":
			net = plant_adi_rows(LookupNet(seed=62, special=True), 1062, infinite=48)
			taken = np.zeros(net.M, bool)
			for key, rows in net.planted.items():
				rows = rows[0] if key == "special" else rows
				taken[np.concatenate(rows) if isinstance(rows, tuple) else rows] = True
			free = np.nonzero(~taken)[0]
			nan_rows = np.random.RandomState(2062).permutation(free)[:48]
			vt = net.value_table.reshape(net.M, 21)
			vt[nan_rows[:24]] = np.float32(np.nan)
			vt[nan_rows[24:]] = np.array([0x7FC00001, 0xFFC00000, 0x7F800001], np.uint32).view(np.float32)[np.arange(21) % 3]   # other NaN bit patterns
			net.planted["nan"] = nan_rows
		elif name == "linear_bf16":
			net = LinearLookupNet(seed=63, dtype="bfloat16")
		elif name == "noisy":
			net = NoisyStubNet(seed=3)
		else:
			raise KeyError(name)
		_NETS[name] = net
	return _NETS[name]


def start_of(seed: int, depth: int) -> np.ndarray:
	np.random.seed(seed)
	return orc.scramble(depth, True)[0]


Case = namedtuple("Case", "net width prune max_depth seed scramble")


def _cases():
	out = []
	for k, (width, prune, max_depth) in enumerate((w, p, d) for w in WIDTHS for p in (True, False) for d in (1, 2, 12)):
		out.append(Case(NET_NAMES[k % len(NET_NAMES)], width, prune, max_depth, 500 + k, (1, 4, 9)[(k + k // 3) % 3]))
	return out


CASES = _cases()
#: more starts for the net that makes beams solve, so that status 1 past the first depth occurs at several widths
SOLVING_CASES = [Case("noisy", w, True, 12, 560 + n, 4) for n, w in enumerate((5, 22, 342))]
BALL_RADIUS = 3
#: (net, width, seed, scramble depth) with the radius-3 ball: inside the ball at the reset, then beams that have to reach it
BALL_CASES = [("noisy", 5, 570, 2), ("lookup", 22, 570, 4), ("lookup", 6, 572, 6), ("noisy", 22, 572, 6), ("lookup_special", 342, 570, 6),
              ("noisy", 342, 571, 9), ("lookup_bf16", 342, 571, 9), ("lookup_bf16", 5, 572, 9)]
#: the model's alone: a ball with a hole (see the head of this file); case k starts one move outside the hole
THIN_SEED = 7
THIN_CASES = [("noisy", 22, k) for k in range(4)] + [("lookup", 22, k) for k in range(4)]


def thin_start(k: int) -> np.ndarray:
	ball = ball_model(BALL_RADIUS, THIN_SEED)
	outside = [s for s in orc.expand12(ball.hole[None]) if ball.depth(s)[0] < 0 and ball_model(BALL_RADIUS).depth(s)[0] == BALL_RADIUS]
	return outside[k % len(outside)]


@functools.lru_cache(maxsize=None)
def thin_reference(case: tuple, defect: str = None) -> Result:
	net, width, k = case
	return search(values_of(net_of(net)), thin_start(k), width, 12, ball_model(BALL_RADIUS, THIN_SEED), True, None, defect)


def case_id(case) -> str:
	return "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=None)
def reference(case: Case, max_states: int = None, defect: str = None) -> Result:
	"""The model's result of a 2024 case; computed once per process and shared (treat it as read-only)."""
	return search(values_of(net_of(case.net)), start_of(case.seed, case.scramble), case.width, case.max_depth, None, case.prune, max_states, defect)


@functools.lru_cache(maxsize=None)
def ball_reference(case: tuple, defect: str = None, max_depth: int = 12) -> Result:
	net, width, seed, scramble = case
	return search(values_of(net_of(net)), start_of(seed, scramble), width, max_depth, ball_model(BALL_RADIUS), True, None, defect)
