"""
Nets, input tuples and NumPy restatements for the exact ADI tests -- TEST INFRASTRUCTURE, not imported by the product.

  LinearLookupNet   a net of the reference's structure (`shared_net` = Sequential starting with nn.Linear(480, H), `policy_net`,
                    `value_net`), so that `fuse_first_linear` accepts it, whose outputs are nevertheless LookupNet's table entries:
                    arbitrary float32 / bfloat16 bit patterns, the same bits from NumPy, torch on a one-hot and torch on states
                    through `fused_net(net, mode)`.
  plant_adi_rows    rows of a LookupNet's value table that make exact ties and one-ulp neighbours AFTER the reward is added frequent
                    among twelve siblings (LookupNet's own planted rows are 64 pairs of 4093: two siblings almost never meet them).
  Recorded          any net plus a record of the batches it was given (and, for a net that is no torch module, the parameter dtype
                    that makes adi_traindata hand it its rows in that dtype).
  LOOKUP_CASES, LINEAR_CASES, REPR686_CASES     the (net, seed, games, depth, method, ff_batches) tuples of the GPU tests;
                    tests/test_adi_real_valued_cpu.py checks on the oracle alone that they are not weak.
  adi_model         adi_traindata's arithmetic between the net and the targets restated in NumPy (slices included), with one planted
                    defect at a time: what the CPU tests use to prove that the exact comparisons have teeth.
  adi686_oracle     adi_traindata_oracle for a net of the 6x8x6 representation: the same walks in both forms, 288-wide rows.

Why every number of LinearLookupNet is exact.  The first layer's weights are integers 0..12 and its bias 0..3, so a pre-activation
is the sum of twenty weights and the bias: every partial sum is an integer below 256 -- exact in float32 in any order, exact in
bfloat16 (8 significant bits), exact through the MFMA route's bfloat16 output.  ELU and ReLU are the identity on non-negative
integers.  Both BatchNorm1d layers have eps = 2^-6 and running variance 1 - 2^-6 (six bits: exact in bfloat16 too), so var + eps is
exactly 1 in float32 and in float64 and the scale exactly 1; means and shifts are integers 0..3 with shift >= mean.  The second
Linear copies sixteen units (one weight 1 per row) and adds a bias 0..3.  All values stay integers in 0..252.  Folding the second
BatchNorm into that Linear ("folded") multiplies its weights by 1.0 and adds integers to its bias: exact in both dtypes, so "folded"
is covered in bfloat16 as well.  (The heads are gathers, not Linear stacks: the merged heads and TailLinear of "folded" do not apply.)
Unit 0 has the solved one-hot as weights and nothing added anywhere, so it carries 20 - k, k = StubNet's count.  The heads turn the
sixteen integers into h = (sum c_j u_j) mod M in int64 and gather value_table[21 h + k] / logit_table[h], LookupNet's tables.
"""
import numpy as np
import torch

from oracle import cube_oracle as orc
from oracle.search_oracle import LookupNet

BN_EPS = 2.0 ** -6


# ---- the value table ------------------------------------------------------------------------------------------------------------
def plant_adi_rows(net: LookupNet, seed: int, solved_h: int = None, quantised: int = 1600, ulp: int = 600, infinite: int = 24) -> LookupNet:
	"""
	Overwrites rows of net.value_table that LookupNet has not planted itself (call before the net's first torch use):
	  * `quantised` rows hold q - k / 2 with q a multiple of 1/2 near the row's own noise: among twelve siblings several such entries
	    meet, and value + reward (+-1, 0) then ties EXACTLY, at the maximum too;
	  * `ulp` rows (float32 tables only) hold v with float32(v - 1) one float32 ulp above a multiple of 1/2: next to a quantised
	    sibling the two are one ulp apart after the reward -1 is added.  Entries for which v - 1 would not round there stay quantised.
	    (In a bfloat16 table two different entries are at least a bfloat16 ulp apart and v - 1 is exact: there is nothing to plant.)
	  * the solved state's entry (row `solved_h`, by default the row LookupNet's own index gives it; k = 0) is -1: the solved state has
	    ONE value per net, and a random one either always wins with its reward or never does.  At -1 the reward +1 makes it +0.0, which
	    wins against some siblings' value - 1 and loses against others, and is the maximum of the net's values alone only rarely.
	  * with `special`, `infinite` more rows of +inf and as many of -inf (LookupNet plants four of each: too few for 4 000 children).
	Exact in bfloat16 as well: multiples of 1/2 below 32 have at most six significant bits.
	"""
	rng = np.random.RandomState(seed)
	M = net.M
	vt = net.value_table.reshape(M, 21)                              # a view: the net's own table changes
	taken = np.zeros(M, bool)
	for key, rows in net.planted.items():
		rows = rows[0] if key == "special" else rows                 # "special" is (rows, their values)
		taken[np.concatenate(rows) if isinstance(rows, tuple) else rows] = True
	free = rng.permutation(np.nonzero(~taken)[0])
	k = np.arange(21, dtype=np.float32)
	rows_q, rows_u = free[:quantised], free[quantised:quantised + ulp]
	for rows in (rows_q, rows_u):
		q = np.round(vt[rows, 0] * 2) / 2
		vt[rows] = (q[:, None] - k[None, :] / 2).astype(np.float32)
	if net.dtype == "float32":
		t = (vt[rows_u] - np.float32(1)).astype(np.float32)          # exact: multiples of 1/2
		up = np.nextafter(t, np.float32(np.inf))
		v = (up + np.float32(1)).astype(np.float32)
		ok = (v - np.float32(1)).astype(np.float32) == up
		vt[rows_u] = np.where(ok, v, vt[rows_u])
	planted = dict(net.planted, quantised=rows_q, ulp_after_reward=rows_u)
	if net.special:
		rows_i = free[quantised + ulp:quantised + ulp + 2 * infinite]
		vt[rows_i[:infinite]] = np.float32(np.inf)
		vt[rows_i[infinite:]] = np.float32(-np.inf)
		planted["infinite"] = rows_i
	if solved_h is None:
		solved_h = int(net.rows(orc.as_oh(orc.SOLVED))[0][0])
	vt[solved_h, 0] = np.float32(-1)
	planted["solved"] = np.array([solved_h])
	net.planted = planted
	assert not np.isnan(vt).any() and not net._tables_dev
	return net


# ---- the net --------------------------------------------------------------------------------------------------------------------
class _Index(torch.nn.Module):
	"""(n, U) integers held in floats -> (n, 2) int64: h = (sum_j c_j u_j) mod M over units 1.., k = 20 - u_0"""
	def __init__(self, coef: np.ndarray, M: int):
		super().__init__()
		self.M = M
		self.register_buffer("coef", torch.from_numpy(coef.astype(np.int64)))

	def forward(self, y):
		u = y.long()
		return torch.stack([(u[:, 1:] * self.coef).sum(dim=1) % self.M, 20 - u[:, 0]], dim=1)


class _Gather(torch.nn.Module):
	"""(n, 2) int64 (h, k) -> table[21 h + k] as (n, 1) for the value table (M * 21,), table[h] for the logit table (M, 12)"""
	def __init__(self, table: np.ndarray):
		super().__init__()
		self.register_buffer("table", torch.from_numpy(table.copy()))

	def forward(self, hk):
		if self.table.dim() == 1:
			return self.table[21 * hk[:, 0] + hk[:, 1]].reshape(-1, 1)
		return self.table[hk[:, 0]]


class LinearLookupNet(torch.nn.Module):
	"""
	LookupNet's tables behind a real nn.Linear(480, H) -> activation -> BatchNorm1d -> [BatchNorm1d -> Linear(H, U) -> index] with
	gathering heads; see the head of this file for why every number is exact.  H is a multiple of 64 (what rk_ohl_create accepts);
	192 leaves the direct MFMA form's second 128-column group half empty.  `lookup` is the LookupNet whose tables these are
	(`plant_adi_rows` applied); a NumPy batch goes through integer arithmetic of its own (a gather of the twenty weight rows in int64).
	"""
	U = 16

	def __init__(self, seed: int = 0, dtype: str = "float32", special: bool = False, H: int = 192, activation: str = "elu", **lookup_args):
		super().__init__()
		self.lookup = LookupNet(seed=seed, dtype=dtype, special=special, **lookup_args)
		self.dtype, self.M, self.H = dtype, self.lookup.M, H
		rng = np.random.RandomState(seed + 2000)
		W = rng.randint(0, 13, (H, 480))
		b1, m1, d1, m2, d2 = (rng.randint(0, 4, H) for _ in range(5))
		W[0] = orc.as_oh(orc.SOLVED)[0]
		for a in (b1, m1, d1, m2, d2):
			a[0] = 0
		sel = np.concatenate([[0], 1 + rng.choice(H - 1, self.U - 1, replace=False)])
		b2 = rng.randint(0, 4, self.U)
		b2[0] = 0
		coef = rng.randint(1, self.M, self.U - 1)
		# the whole trunk as integers, for the NumPy form: u2 = (sum of twenty rows of Wt + add1)[:, sel] + add2
		self._Wt, self._add1, self._sel, self._add2, self._coef = W.T.astype(np.int64).copy(), (b1 + d1 + d2).astype(np.int64), sel, b2.astype(np.int64), coef.astype(np.int64)
		plant_adi_rows(self.lookup, seed + 1000, solved_h=int(self.rows(orc.as_oh(orc.SOLVED))[0][0]))

		def bn(mean, shift):
			m = torch.nn.BatchNorm1d(H, eps=BN_EPS)
			with torch.no_grad():
				m.running_var.fill_(1.0 - BN_EPS)
				m.running_mean.copy_(torch.from_numpy(mean.astype(np.float32)))
				m.weight.fill_(1.0)
				m.bias.copy_(torch.from_numpy((mean + shift).astype(np.float32)))
			return m
		first, second = torch.nn.Linear(480, H), torch.nn.Linear(H, self.U)
		W2 = np.zeros((self.U, H), np.float32)
		W2[np.arange(self.U), sel] = 1
		with torch.no_grad():
			first.weight.copy_(torch.from_numpy(W.astype(np.float32)))
			first.bias.copy_(torch.from_numpy(b1.astype(np.float32)))
			second.weight.copy_(torch.from_numpy(W2))
			second.bias.copy_(torch.from_numpy(b2.astype(np.float32)))
		act = {"elu": torch.nn.ELU, "relu": torch.nn.ReLU}[activation]()
		self.shared_net = torch.nn.Sequential(first, act, bn(m1, d1), bn(m2, d2), second, _Index(coef, self.M))
		self.value_net = torch.nn.Sequential(_Gather(self.lookup.value_table))
		self.policy_net = torch.nn.Sequential(_Gather(self.lookup.logit_table))
		for p in self.parameters():
			p.requires_grad_(False)
		if dtype == "bfloat16":
			self.to(torch.bfloat16)                                      # the tables hold bfloat16 numbers already: an exact cast
		self.eval()

	def rows(self, x: np.ndarray):
		"""(h, k) of every row of a NumPy one-hot batch, by integer arithmetic"""
		x = np.asarray(x)
		cols = 24 * np.arange(20)[None, :] + x.reshape(len(x), 20, 24).argmax(axis=2)
		assert (x[np.arange(len(x))[:, None], cols] == 1).all() and (x.sum(axis=1) == 20).all(), "not a one-hot"
		u = np.concatenate([self._Wt[cols[lo:lo + 2048]].sum(axis=1) for lo in range(0, len(cols), 2048)]) if len(cols) else np.zeros((0, self.H), np.int64)
		u = (u + self._add1)[:, self._sel] + self._add2
		return (u[:, 1:] * self._coef).sum(axis=1) % self.M, 20 - u[:, 0]

	def forward(self, x, policy=True, value=True):
		if isinstance(x, torch.Tensor):
			hk = self.shared_net(x.to(self.shared_net[0].weight.dtype))
			out = ([self.policy_net(hk)] if policy else []) + ([self.value_net(hk)] if value else [])
		else:
			h, k = self.rows(x)
			out = ([self.lookup.logit_table[h]] if policy else []) + ([self.lookup.value_table[21 * h + k].reshape(-1, 1)] if value else [])
		return out if len(out) > 1 else out[0]


class Recorded:
	"""A net and the (rows, dtype) of every batch it was given.  `rows_dtype`: parameters() then yields one tensor of that dtype, which is
	how adi_traindata and the agents learn the dtype a net wants its one-hot rows in (a LookupNet is no torch module and has none)."""
	def __init__(self, net, rows_dtype: torch.dtype = None):
		self.net, self.calls = net, []
		self._marker = torch.zeros(1, dtype=rows_dtype) if rows_dtype is not None else None

	def parameters(self):
		if self._marker is not None:
			yield self._marker
		elif callable(getattr(self.net, "parameters", None)):
			yield from self.net.parameters()

	def eval(self):
		self.net.eval()
		return self

	def __call__(self, x, policy=True, value=True):
		self.calls.append((len(x), x.dtype))
		return self.net(x, policy=policy, value=value)


# ---- the input tuples -----------------------------------------------------------------------------------------------------------
#: name -> constructor of the nets below; made once per process (`net_of`): the tables are read-only after planting
NETS = {
	"lookup": lambda: plant_adi_rows(LookupNet(seed=40), 1040),
	"lookup_bf16": lambda: plant_adi_rows(LookupNet(seed=41, dtype="bfloat16"), 1041),
	"lookup_special": lambda: plant_adi_rows(LookupNet(seed=42, special=True), 1042),
	"linear": lambda: LinearLookupNet(seed=43),
	"linear_bf16": lambda: LinearLookupNet(seed=44, dtype="bfloat16"),
	"linear_special": lambda: LinearLookupNet(seed=45, special=True, activation="relu"),
}
_NETS = {}


def net_of(name: str):
	if name not in _NETS:
		_NETS[name] = NETS[name]()
	return _NETS[name]


def slices(n: int, ff: int):
	"""(lo, hi) of adi_traindata's net calls for n states: step = ceil(12 n / ff)"""
	step = -(-12 * n // max(1, ff))
	return [(lo, min(lo + step, 12 * n)) for lo in range(0, 12 * n, step)]


# (net, seed, games, depth, method, ff_batches).  12 n children in slices of step = ceil(12 n / ff):
#   37 x 9,  ff 7:  3 996 children, step 571 (= 7 mod 12, 59 mod 64, 11 mod 16), last slice 570
#   64 x 5,  ff 5:  3 840 children, step 768 -- a whole multiple of 12 and of 64, and the largest batch of the direct MFMA form
#   64 x 5,  ff 7:  step 549 (= 9 mod 12, 37 mod 64, 5 mod 16), last slice 546
#   1 x 1,   ff 1:  one state, twelve children, one of them solved
#   3 x 2,   ff 50: 72 children, step 2: more slices asked for than there are states, 36 net calls of 2 rows
#   37 x 9,  ff 40: step 100 (= 4 mod 12, 36 mod 64), last slice 96: more than 64 and fewer than 128 rows
#   5 x 5,   ff 24: 300 children, step 13, last slice exactly 1 row
#   41 x 9,  ff 5:  4 428 children, step 886 (= 10 mod 12, 54 mod 64, 6 mod 16) > 768: the LDS-tiled MFMA form, last slice 884
#   100 x 25, ff 7: 30 000 children, step 4 286 (= 2 mod 12, 62 mod 64, 14 mod 16), last slice 4 284: several row groups per launch
LOOKUP_CASES = [
	("lookup", 201, 37, 9, "lapanfix", 7), ("lookup", 202, 37, 9, "paper", 7), ("lookup", 203, 37, 9, "schultzfix", 7),
	("lookup", 204, 37, 9, "reward0", 7),
	("lookup_bf16", 205, 64, 5, "lapanfix", 5), ("lookup_bf16", 206, 64, 5, "reward0", 7),
	("lookup_special", 207, 37, 9, "paper", 7), ("lookup", 208, 64, 5, "schultzfix", 5),
	("lookup", 209, 1, 1, "lapanfix", 1), ("lookup", 210, 1, 1, "paper", 1), ("lookup", 211, 1, 1, "schultzfix", 1),
	("lookup", 212, 1, 1, "reward0", 1),
	("lookup", 213, 3, 2, "lapanfix", 50), ("lookup_special", 214, 100, 25, "schultzfix", 7),
]
LINEAR_CASES = [
	("linear", 221, 37, 9, "lapanfix", 7), ("linear", 222, 64, 5, "paper", 5), ("linear", 223, 64, 5, "schultzfix", 7),
	("linear", 224, 1, 1, "reward0", 1), ("linear", 225, 3, 2, "lapanfix", 50), ("linear", 226, 37, 9, "paper", 40),
	("linear", 227, 5, 5, "schultzfix", 24), ("linear_special", 228, 41, 9, "lapanfix", 5), ("linear_special", 229, 100, 25, "paper", 7),
	("linear_bf16", 231, 37, 9, "lapanfix", 7), ("linear_bf16", 332, 64, 5, "reward0", 5), ("linear_bf16", 233, 1, 1, "paper", 1),
	("linear_bf16", 234, 37, 9, "schultzfix", 40), ("linear_bf16", 235, 5, 5, "lapanfix", 24), ("linear_bf16", 236, 41, 9, "paper", 5),
	("linear_bf16", 237, 100, 25, "lapanfix", 7), ("linear_bf16", 238, 3, 2, "schultzfix", 50),
]
#: (seed of NoisyStubNet686, seed, games, depth, method, ff_batches): shapes tests/golden/repr686_search.npz does not hold
REPR686_CASES = [(4, 241, 37, 9, "lapanfix", 7), (5, 242, 64, 5, "schultzfix", 7), (4, 243, 5, 5, "paper", 24), (6, 244, 37, 9, "reward0", 40),
                 (4, 245, 1, 1, "lapanfix", 1)]
ALPHA = 0.3


def case_id(case) -> str:
	return "-".join(str(x) for x in case)


# ---- adi_traindata between the net and the targets, in NumPy --------------------------------------------------------------------
DEFECTS = ("last_maximum", "reward_after_argmax", "slice_off_by_one", "lapanfix_child_flag", "schultzfix_stride")


def adi_model(net, games: int, depth: int, method: str, ff: int, defect: str = None):
	"""
	librubiks_amd/adi.py from the walks to the targets with the oracle's cube arithmetic: the children's values slice by slice as
	adi_traindata cuts them, + reward, first maximum, the overrides.  -> (policy int64, value float32).  Without a defect this equals
	adi_traindata_oracle (tests/test_adi_real_valued_cpu.py asserts it); `defect` plants one of DEFECTS:
	  last_maximum          the last of equal maxima wins
	  reward_after_argmax   the argmax is taken on the net's values, the reward is added to the value taken
	  slice_off_by_one      the children of every slice are read from row lo + 1 (the last row of all is read twice)
	  lapanfix_child_flag   lapanfix zeroes the states whose CHOSEN CHILD is solved instead of the solved scrambled states
	  schultzfix_stride     schultzfix zeroes every (depth + 1)-th state instead of every depth-th
	"""
	assert defect is None or defect in DEFECTS
	states, _ = orc.sequence_scrambler(games, depth, method == "lapanfix")
	n = len(states)
	solved_scrambled = orc.multi_is_solved(states)
	sub = orc.expand12(states)
	solved_sub = orc.multi_is_solved(sub)
	rewards = np.where(solved_sub, 0.0 if method == "reward0" else 1.0, -1.0).astype(np.float32)
	values = np.empty(12 * n, np.float32)
	for lo, hi in slices(n, ff):
		rows = np.arange(lo, hi) + (defect == "slice_off_by_one")
		values[lo:hi] = np.asarray(net(orc.as_oh(sub[np.minimum(rows, 12 * n - 1)]), policy=False, value=True), np.float32).reshape(-1)
	with_reward = (values + rewards).reshape(-1, 12)
	ranked = values.reshape(-1, 12) if defect == "reward_after_argmax" else with_reward
	policy = 11 - ranked[:, ::-1].argmax(axis=1) if defect == "last_maximum" else ranked.argmax(axis=1)
	value = with_reward[np.arange(n), policy].copy()
	if method == "lapanfix":
		value[solved_sub.reshape(-1, 12)[np.arange(n), policy] if defect == "lapanfix_child_flag" else solved_scrambled] = 0
	elif method == "schultzfix":
		value[np.arange(0, n, depth + (defect == "schultzfix_stride"))] = 0
	return policy.astype(np.int64), value.astype(np.float32)


def adi686_oracle(net, games: int, depth: int, alpha: float, method: str):
	"""
	adi_traindata_oracle for a torch net of the 6x8x6 representation: the draws of `sequence_scrambler`, walked by the oracle in both
	representations (`multi_rotate` and `multi_rotate686` with the same faces and directions, as tests/repr686_pairs.py pairs its
	rows), the 288-wide one-hot of every child to the net on the CPU.  Same return values as adi_traindata_oracle, rows 288 wide.
	"""
	with_solved = method == "lapanfix"
	faces = np.random.randint(0, 6, (depth, games))
	dirs = np.random.randint(0, 2, (depth, games))
	states20 = orc.sequence_states(faces, dirs, with_solved)
	cur = orc.repeat_state(orc.SOLVED686, games)
	seq = [cur] if with_solved else []
	for d in range(depth - int(with_solved)):
		cur = orc.multi_rotate686(cur, faces[d], dirs[d])
		seq.append(cur)
	states = np.stack(seq, axis=1).reshape(games * depth, 6, 8, 6)
	n = len(states)
	f, d = orc.iter_actions(n)
	sub = orc.multi_rotate686(np.repeat(states, 12, axis=0), f, d)
	solved_scrambled, solved_sub = orc.multi_is_solved686(states), orc.multi_is_solved686(sub)
	assert (solved_scrambled == orc.multi_is_solved(states20)).all() and (solved_sub == orc.multi_is_solved(orc.expand12(states20))).all()
	rewards = np.where(solved_sub, 0.0 if method == "reward0" else 1.0, -1.0).astype(np.float32)
	with torch.no_grad():
		values = net(torch.from_numpy(orc.as_oh686(sub)), policy=False, value=True).reshape(-1).float().numpy() + rewards
	values = values.reshape(-1, 12)
	policy = values.argmax(axis=1)
	value = values[np.arange(n), policy].copy()
	if method == "lapanfix":
		value[solved_scrambled] = 0
	elif method == "schultzfix":
		value[np.arange(0, n, depth)] = 0
	w = np.tile(1 / np.arange(1, depth + 1), games)
	lw = ((1 - alpha) * w / w.sum() + alpha / len(w)) * (w.sum() + len(w))
	return orc.as_oh686(states), policy.astype(np.int64), value.astype(np.float32), lw.astype(np.float32)
