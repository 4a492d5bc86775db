"""
ADI targets on REAL-VALUED nets, bit for bit against the oracle: where `adi_traindata` (librubiks_amd/adi.py) hands the net its rows
and what it makes of the answers.  The nets (tests/adi_nets.py) return arbitrary float32 / bfloat16 bit patterns that are the same
on the host and on the device for any batching, so policy, value bits and one-hot states are compared for EQUALITY; the loss weights
keep the relative 1e-6 of tests/test_adi_gpu.py.  tests/test_adi_real_valued_cpu.py pins the oracle to the unmodified reference on
these nets, checks that the input tuples are not weak and that each comparison would catch a wrong slice, maximum, reward or override.
  * LookupNet, unfused: every reward method, bfloat16 rows, `special` values, at `ff_batches` that cut through a state's twelve
    children and through the encoder's tiles, leave a ragged last slice, ask for more slices than there are states, down to one state;
  * LinearLookupNet -- a real nn.Linear(480, H) in front -- unfused and with `fused_first_layer` True, "epilogue" and "folded", float32
    (gather route) and bfloat16 (both MFMA forms): the fused kernels read `substates[lo:hi]` where it lies, 4-byte aligned;
  * a 6x8x6 net on the same cuts, against the oracle walking both representations (288-wide rows).
"""
import numpy as np
import pytest
import torch

from librubiks_amd import cube
from librubiks_amd.adi import adi_traindata
from tests.adi_nets import ALPHA, LINEAR_CASES, LOOKUP_CASES, REPR686_CASES, Recorded, adi686_oracle, case_id, net_of, slices
from tests.repr686_nets import NoisyStubNet686
from tests.test_adi_real_valued_cpu import bits, oracle_of

pytestmark = pytest.mark.gpu
_DEVICE_NETS = {}


def _same(got, want, what):
	oh, policy, value, lw = got
	assert oh.is_cuda and oh.dtype == torch.float32 and (oh.cpu().numpy() == want[0]).all(), what
	assert policy.dtype == torch.int64 and (policy.numpy() == want[1]).all(), what
	assert value.dtype == torch.float32 and (bits(value.numpy()) == bits(want[2])).all(), what
	assert np.allclose(lw.numpy(), want[3], rtol=1e-6, atol=0), what


@pytest.mark.parametrize("case", LOOKUP_CASES, ids=case_id)
def test_lookup_net_unfused(case):
	name, seed, games, depth, method, ff = case
	want = oracle_of(case)                                           # reseeds NumPy itself (made once, shared with the CPU tests)
	bf16 = "bf16" in name
	net = Recorded(net_of(name), torch.bfloat16 if bf16 else None)
	np.random.seed(seed)
	got = adi_traindata(net, games, depth, ALPHA, method, ff_batches=ff)
	_same(got, want, case)
	# the net saw exactly the slices, in order, in the dtype it asked for
	assert [rows for rows, _ in net.calls] == [hi - lo for lo, hi in slices(games * depth, ff)]
	assert {dt for _, dt in net.calls} == {torch.bfloat16 if bf16 else torch.float32}
	if bf16:
		assert net.net(torch.zeros(2, 480, device="cuda", dtype=torch.bfloat16), policy=False).dtype == torch.bfloat16


def _device_net(name):
	if name not in _DEVICE_NETS:
		import copy
		_DEVICE_NETS[name] = copy.deepcopy(net_of(name)).cuda().eval()   # the host net stays on the host: it is the oracle's
	return _DEVICE_NETS[name]


@pytest.mark.parametrize("case", LINEAR_CASES, ids=case_id)
def test_linear_net_unfused_and_fused(case):
	"""All four routes equal the oracle, and so each other.  A float32 net takes the gather route; a bfloat16 net the MFMA route, its
	direct form up to 768 rows a slice and the LDS-tiled one beyond."""
	name, seed, games, depth, method, ff = case
	want = oracle_of(case)
	net = _device_net(name)
	assert next(net.parameters()).dtype == (torch.bfloat16 if "bf16" in name else torch.float32)
	for mode in (False, True, "epilogue", "folded"):
		np.random.seed(seed)
		got = adi_traindata(net, games, depth, ALPHA, method, ff_batches=ff, fused_first_layer=mode)
		_same(got, want, (case, mode))


def test_fused_routes_take_the_kernels_they_are_meant_to():
	"""What the cases above rely on: the fused callable of each mode really holds the fused layer (with the epilogue's activation and
	BatchNorm inside for "epilogue" and "folded", the second BatchNorm folded away for "folded"), on the route of the net's dtype."""
	from librubiks_amd.oh_linear import OhLinear, fused_net
	for name, route in (("linear", "gather"), ("linear_bf16", "mfma")):
		net = _device_net(name)
		for mode, rest_len, bns in ((True, 5, 2), ("epilogue", 3, 1), ("folded", 2, 0)):
			f = fused_net(net, mode)
			assert isinstance(f.first, OhLinear) and f.first.route == route and f.first.out_features == net.H
			rest = f.modules[0]
			assert len(rest) == rest_len and sum(isinstance(m, torch.nn.BatchNorm1d) for m in rest) == bns, (name, mode)


@pytest.mark.parametrize("case", REPR686_CASES, ids=case_id)
def test_repr686_net_on_the_same_cuts(case):
	"""NoisyStubNet686 (exact integers) at shapes tests/golden/repr686_search.npz does not hold, float32 and bfloat16 rows: one-hot
	states 288 wide, targets and loss weights against the oracle's walk of both representations."""
	net_seed, seed, games, depth, method, ff = case
	np.random.seed(seed)
	want = adi686_oracle(NoisyStubNet686(net_seed), games, depth, ALPHA, method)
	try:
		cube.set_is2024(False)
		for dtype in (torch.float32, torch.bfloat16):
			net = Recorded(NoisyStubNet686(net_seed, dtype).cuda())
			np.random.seed(seed)
			got = adi_traindata(net, games, depth, ALPHA, method, ff_batches=ff)
			assert got[0].shape == (games * depth, 288)
			_same(got, want, (case, dtype))
			assert [rows for rows, _ in net.calls] == [hi - lo for lo, hi in slices(games * depth, ff)]
			assert {dt for _, dt in net.calls} == {dtype}
	finally:
		cube.set_is2024(True)
