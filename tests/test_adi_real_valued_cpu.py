"""
The CPU half of the exact ADI tests (tests/test_adi_real_valued_gpu.py holds the GPU half): no GPU anywhere.
  * LinearLookupNet (tests/adi_nets.py) returns the same bits from its NumPy form and its torch form, for any batching;
  * adi_traindata_oracle equals the UNMODIFIED reference `Train.ADI_traindata` on real-valued nets (tests/golden/adi_real_trace.npz,
    written by oracle/gen_golden.py);
  * the input tuples of the GPU tests are not weak: on the oracle alone, each tuple of 300 states or more has later maxima, exact
    ties at the maximum, top entries one float32 ulp apart after the reward, solved children whose reward turns the argmax,
    infinities with `special`, zero targets -- the counts are printed (pytest -s) and asserted;
  * the comparisons have teeth: adi_traindata's arithmetic restated with one defect at a time (adi_nets.adi_model) differs from the
    oracle on those tuples.  The table of which tuple catches which defect is printed.
"""
import os

import numpy as np
import pytest
import torch

from oracle import cube_oracle as orc
from oracle.search_oracle import LookupNet, adi_traindata_oracle
from tests import adi_nets
from tests.adi_nets import ALPHA, DEFECTS, LINEAR_CASES, LOOKUP_CASES, adi_model, case_id, net_of
from tests.helpers import sha

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = LOOKUP_CASES + LINEAR_CASES
LARGE = 300                                    # states: tuples of at least this size must meet every condition on their own
_ORACLE = {}


def bits(a) -> np.ndarray:
	return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_of(case):
	"""adi_traindata_oracle of an input tuple, made once and left unchanged -> (one-hot, policy, value, loss weights)"""
	if case not in _ORACLE:
		name, seed, games, depth, method, _ = case
		np.random.seed(seed)
		out = adi_traindata_oracle(net_of(name), games, depth, ALPHA, method)
		for a in out:
			a.flags.writeable = False
		_ORACLE[case] = out
	return _ORACLE[case]


def oracle_children(case):
	"""the children of an input tuple's walks -> (20-byte states (12 n, 20), solved flags (12 n,))"""
	_, seed, games, depth, method, _ = case
	np.random.seed(seed)
	states, _ = orc.sequence_scrambler(games, depth, method == "lapanfix")
	sub = orc.expand12(states)
	return sub, orc.multi_is_solved(sub)


# ---- the same bits in every form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["linear", "linear_bf16", "linear_special"])
def test_linear_net_same_bits_from_numpy_and_torch(name):
	"""A few hundred oracle children (legal cubes reached by scrambling): NumPy against torch on the CPU, as one batch and in slices of
	1, 7 and 13 rows; values and logits by their bits.  The NumPy form is integer arithmetic, the torch form the real modules."""
	net = net_of(name)
	sub, _ = oracle_children((name, 77, 9, 5, "paper", 1))
	oh = orc.as_oh(sub)
	assert len(oh) == 540
	p_np, v_np = net(oh)
	assert p_np.dtype == np.float32 and v_np.dtype == np.float32 and v_np.shape == (540, 1) and p_np.shape == (540, 12)
	dt = torch.bfloat16 if net.dtype == "bfloat16" else torch.float32
	x = torch.from_numpy(oh)
	for size in (len(oh), 1, 7, 13):
		ps, vs = zip(*(net(x[lo:lo + size]) for lo in range(0, len(oh), size)))
		p, v = torch.cat(ps), torch.cat(vs)
		assert p.dtype == dt and v.dtype == dt
		assert (bits(p.float().numpy()) == bits(p_np)).all() and (bits(v.float().numpy()) == bits(v_np)).all(), size
	assert (net(x, policy=False).float().numpy() == v_np).all() and (net(oh, value=False) == p_np).all()
	h, k = net.rows(oh)
	stub_k = 20 - (oh * orc.as_oh(orc.SOLVED)[0]).sum(axis=1)
	distinct = len(np.unique(sub, axis=0))                               # walks revisit states: a state's parent is among its children
	assert (k == stub_k).all() and len(np.unique(h)) > 0.9 * distinct > 300 and h.min() >= 0 and h.max() < net.M
	assert net.shared_net[0].in_features == 480 and net.shared_net[0].out_features % 64 == 0
	assert isinstance(net.shared_net[1], (torch.nn.ELU, torch.nn.ReLU)) and isinstance(net.shared_net[2], torch.nn.BatchNorm1d) and not net.training


def test_linear_net_trunk_is_exact_in_both_dtypes():
	"""Every intermediate of the trunk is an integer in 0..255 (so bfloat16 holds it), and the BatchNorm affine maps that the fused paths
	compute in float64 (`batchnorm_affine`) have scale exactly 1 and integer shifts, in float32 and after the cast to bfloat16."""
	from librubiks_amd.oh_linear import batchnorm_affine
	sub, _ = oracle_children(("linear", 78, 9, 5, "paper", 1))
	x = torch.from_numpy(orc.as_oh(sub))
	for name in ("linear", "linear_bf16", "linear_special"):
		net = net_of(name)
		y = x.to(net.shared_net[0].weight.dtype)
		for m in list(net.shared_net)[:-1]:
			y = m(y)
			f = y.double()
			assert (f == f.round()).all() and f.min() >= 0 and f.max() <= 255, (name, m)
		for bn in (net.shared_net[2], net.shared_net[3]):
			scale, shift = batchnorm_affine(bn)
			assert (scale == 1).all() and (shift == shift.round()).all() and shift.min() >= 0 and shift.max() <= 3


def test_planted_rows_are_what_they_say():
	for name in ("lookup", "lookup_bf16", "lookup_special", "linear"):
		net = net_of(name)
		net = getattr(net, "lookup", net)
		vt = net.value_table.reshape(net.M, 21)
		q = vt[net.planted["quantised"]]
		assert (q * 2 == np.round(q * 2)).all()
		u = vt[net.planted["ulp_after_reward"]]
		t = (u - np.float32(1)).astype(np.float32)
		near = np.round(t * 2) / 2
		one_up = np.nextafter(near.astype(np.float32), np.float32(np.inf)) == t
		if net.dtype == "float32":
			assert one_up.mean() > 0.5 and (one_up | (t == near)).all()
		else:
			assert (t == near).all()
		assert vt[net.planted["solved"][0], 0] == -1
		if net.special:
			assert np.isinf(vt[net.planted["infinite"]]).all()


# ---- the oracle against the unmodified reference ------------------------------------------------------------------------------------
def _trace():
	with np.load(os.path.join(GOLDEN, "adi_real_trace.npz")) as z:
		return {k: z[k] for k in z.files}


def test_oracle_reproduces_reference_on_real_valued_nets():
	"""tests/golden/adi_real_trace.npz: the unmodified reference's Train.ADI_traindata on a float32 LookupNet and on LinearLookupNet
	(their torch forms on the CPU), every reward method on each: policy, value bits, one-hot hash, loss weights."""
	t = _trace()
	tags = sorted(k[:-len("_params")] for k in t if k.endswith("_params"))
	assert len(tags) == 8 and {str(t[f"{g}_net"]) for g in tags} == {"lookup", "linear"}
	assert {str(t[f"{g}_method"]) for g in tags} == {"lapanfix", "paper", "schultzfix", "reward0"}
	for tag in tags:
		seed, games, depth, ff = (int(x) for x in t[f"{tag}_params"])
		np.random.seed(seed)
		oh, policy, value, lw = adi_traindata_oracle(net_of(str(t[f"{tag}_net"])), games, depth, float(t[f"{tag}_alpha"]), str(t[f"{tag}_method"]))
		assert sha(oh) == str(t[f"{tag}_oh_sha256"]), tag
		assert (policy == t[f"{tag}_policy"]).all() and policy.dtype == np.int64, tag
		assert t[f"{tag}_value_bits"].dtype == np.uint32 and (bits(value) == t[f"{tag}_value_bits"]).all(), tag
		assert np.allclose(lw, t[f"{tag}_loss_weights"], rtol=1e-6, atol=0), tag
		ties = int((t[f"{tag}_policy"] != 0).sum())
		print(tag, "n", len(policy), "later maxima", ties, "zero targets", int((value == 0).sum()))
		assert ties >= len(policy) // 10


# ---- the inputs are not weak ----------------------------------------------------------------------------------------------------
def input_counts(case) -> dict:
	"""What the oracle's run of an input tuple holds of every edge the GPU comparison is meant to see."""
	name, seed, games, depth, method, ff = case
	net = net_of(name)
	sub, solved_sub = oracle_children(case)
	rewards = np.where(solved_sub, 0.0 if method == "reward0" else 1.0, -1.0).astype(np.float32)
	raw = np.asarray(net(orc.as_oh(sub), policy=False, value=True), np.float32).reshape(-1)
	w, raw = (raw + rewards).reshape(-1, 12), raw.reshape(-1, 12)
	n = len(w)
	_, policy, value, _ = oracle_of(case)
	top = w[np.arange(n), policy]
	assert (top == w.max(axis=1)).all()
	tie = (w == top[:, None]).sum(axis=1) > 1
	assert (policy[tie] == (w[tie] == top[tie, None]).argmax(axis=1)).all()           # the first index wins
	srt = np.sort(w, axis=1)
	with np.errstate(invalid="ignore"):
		ulp = (srt[:, -2] != srt[:, -1]) & (np.nextafter(srt[:, -2], np.float32(np.inf)) == srt[:, -1])
	solved_chosen = solved_sub.reshape(-1, 12)[np.arange(n), policy]
	zero = value == 0
	return dict(states=n, slices=len(adi_nets.slices(n, ff)), last_slice=int(np.diff(adi_nets.slices(n, ff)[-1])[0]),
	            later_maximum=int((policy != 0).sum()), ties=int(tie.sum()), ties_won_by_a_later_index=int((tie & (policy != 0)).sum()),
	            one_ulp_apart=int(ulp.sum()), reward_turns_argmax=int((solved_chosen & (raw.argmax(axis=1) != policy)).sum()),
	            plus_inf_targets=int((value == np.inf).sum()), minus_inf_among_twelve=int((w == -np.inf).any(axis=1).sum()),
	            zero_targets=int(zero.sum()), zero_targets_from_the_sum=int((top == 0).sum()), minus_zero_targets=int((zero & np.signbit(value)).sum()))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_inputs_are_not_weak(case):
	"""
	Conditions, not measurements: every tuple of LARGE states or more meets each of them on the oracle alone.  (One state or six cannot
	hold them all; their counts are printed.)  A target is never -0.0: x + y is -0.0 only for (-0.0) + (-0.0) and no reward is -0.0, so
	a zero target -- the solved child's -1 + 1, a sibling's 1 - 1, the -0.0 row + 0 under reward0, or an override -- must have a clear
	sign bit; the GPU comparison is by bits, so a -0.0 there would show.  One float32 ulp between the top two after the reward cannot
	happen on a bfloat16 table (entries differ by a bfloat16 ulp or more and entry - 1 is exact): asserted for float32 tables.
	"""
	name, seed, games, depth, method, ff = case
	c = input_counts(case)
	print(case_id(case), c)
	n = c["states"]
	assert c["minus_zero_targets"] == 0
	if (games, depth) == (1, 1):
		_, solved_sub = oracle_children(case)
		assert solved_sub.sum() == (0 if method == "lapanfix" else 1)     # lapanfix: the one state IS the solved state (value target 0)
	if n < LARGE:
		return
	assert c["later_maximum"] * 10 >= n
	assert c["ties"] >= 1 and c["ties_won_by_a_later_index"] >= 1
	if "bf16" not in name:
		assert c["one_ulp_apart"] >= 1
	if method != "reward0":
		assert c["reward_turns_argmax"] >= 1
	if "special" in name:
		assert c["plus_inf_targets"] >= 1 and c["minus_inf_among_twelve"] >= 1
	assert c["zero_targets"] >= 1 and c["zero_targets_from_the_sum"] >= 1


def test_cuts_are_the_ones_asked_for():
	"""The slice arithmetic of the tuples: ragged tails, steps that cut through a state's twelve children and through 16- and 64-row
	tiles, a last slice of 65..127 rows, one of exactly 1 row, more slices asked for than states, and both MFMA forms (<= 768 < rows)."""
	shapes = {(g, d, ff) for _, _, g, d, _, ff in CASES}
	assert {(37, 9, 7), (64, 5, 5), (1, 1, 1), (3, 2, 50)} <= shapes
	lasts, steps = set(), set()
	for g, d, ff in shapes:
		s = adi_nets.slices(g * d, ff)
		steps.add(s[0][1] - s[0][0])
		lasts.add(s[-1][1] - s[-1][0])
		if (g, d, ff) not in ((64, 5, 5), (1, 1, 1), (3, 2, 50)):
			step = s[0][1]
			assert step % 12 and step % 16 and step % 64 and (12 * g * d) % ff, (g, d, ff)
	assert 1 in lasts and any(64 < x < 128 for x in lasts) and any(x > 768 for x in steps) and any(x <= 768 for x in steps)
	assert len(adi_nets.slices(6, 50)) == 36
	for bf16 in (False, True):                 # the fused paths meet every cut in both dtypes
		mine = {(g, d, ff) for name, _, g, d, _, ff in LINEAR_CASES if ("bf16" in name) == bf16}
		assert {(37, 9, 7), (64, 5, 5), (1, 1, 1), (3, 2, 50), (37, 9, 40), (5, 5, 24), (41, 9, 5), (100, 25, 7)} <= mine


# ---- teeth ----------------------------------------------------------------------------------------------------------------------
def _model(case, defect=None):
	name, seed, games, depth, method, ff = case
	np.random.seed(seed)
	return adi_model(net_of(name), games, depth, method, ff, defect)


def test_model_without_a_defect_is_the_oracle():
	for case in CASES:
		policy, value = _model(case)
		assert (policy == oracle_of(case)[1]).all() and (bits(value) == bits(oracle_of(case)[2])).all(), case


def test_every_planted_defect_is_caught():
	"""Each defect differs from the oracle in policy or value bits on at least one tuple (the GPU tests compare exactly these with the
	device); the printed table names the tuples that catch each one."""
	caught = {d: [] for d in DEFECTS}
	for case in CASES:
		_, want_p, want_v, _ = oracle_of(case)
		for d in DEFECTS:
			policy, value = _model(case, d)
			if (policy != want_p).any() or (bits(value) != bits(want_v)).any():
				caught[d].append(case_id(case))
	for d in DEFECTS:
		print(d, "caught by", len(caught[d]), "tuples:", ", ".join(caught[d]))
		assert caught[d], d
	# where each one must show: ties and rewards at every large tuple, cuts at every tuple of more than one state (with one state the
	# shifted twelve may keep their first maximum in place), each override at every large tuple of its method
	large = [c for c in CASES if c[2] * c[3] >= LARGE]
	assert all(case_id(c) in caught["last_maximum"] for c in large)
	assert all(case_id(c) in caught["slice_off_by_one"] for c in CASES if c[2] * c[3] > 1)
	assert all(case_id(c) in caught["reward_after_argmax"] for c in large if c[4] != "reward0")
	assert all(case_id(c) in caught["lapanfix_child_flag"] for c in large if c[4] == "lapanfix")
	assert all(case_id(c) in caught["schultzfix_stride"] for c in large if c[4] == "schultzfix")
