"""
`adi_traindata(..., ball=DeviceSymBall(R))` and `cube.device.ball_child_values` (engine rk_symball_child_values) on the GPU, bit for bit
against the model (tests/adi_ball_model.py) with the exact nets of tests/adi_nets.py: their answers do not depend on the batch, which
is what makes the compacted batch of the children outside the ball comparable.  tests/test_adi_ball_cpu.py checks on the model alone
that the input tuples are not weak and that each planted defect would show.
  * LookupNet unfused (float32, bfloat16 rows, `special`) and LinearLookupNet unfused and with `fused_first_layer` True, "epilogue" and
    "folded" (float32, bfloat16), radii 0, 1, 3 and 5, from one state whose twelve children all lie in the ball (the net is not called)
    to 30 000 children (every wave of the fixed grid strides, the compaction crosses its 256-row tiles); the recorded net calls are the
    model's slices of the outside count, in the dtype the net asked for;
  * the device function on the 30 000 rows: depths against the existing rk_symball_depth, the ascending row list, the compacted
    states, V* and an intact sentinel;
  * one 6x8x6 case; `ball=None` is the call without the argument; other balls raise TypeError; the entry's argument errors.
Every test passes `ball=` or calls the new device function.  No ball above radius 5 is built.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from librubiks_amd.adi import adi_traindata
from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall
from oracle import cube_oracle as orc
from tests.adi_ball_model import adi_ball_model, child_depths, vstar
from tests.adi_nets import ALPHA, Recorded, net_of
from tests.repr686_nets import NoisyStubNet686
from tests.test_adi_ball_cpu import LINEAR_CASES, LOOKUP_CASES, case_id, model_of
from tests.test_adi_real_valued_cpu import bits

pytestmark = pytest.mark.gpu
_BALLS, _DEVICE_NETS = {}, {}


def _ball(radius: int) -> DeviceSymBall:
	if radius not in _BALLS:
		_BALLS[radius] = DeviceSymBall(radius)
	return _BALLS[radius]


def _loss_weights(games: int, depth: int) -> np.ndarray:
	w = np.tile(1 / np.arange(1, depth + 1), games)
	return ((1 - ALPHA) * w / w.sum() + ALPHA / len(w)) * (w.sum() + len(w))


def _same(got, policy, value, oh, games, depth, what):
	assert got[0].is_cuda and got[0].dtype == torch.float32 and (got[0].cpu().numpy() == oh).all(), what
	assert got[1].dtype == torch.int64 and (got[1].numpy() == policy).all(), what
	assert got[2].dtype == torch.float32 and (bits(got[2].numpy()) == bits(value)).all(), what
	assert np.allclose(got[3].numpy(), _loss_weights(games, depth), rtol=1e-6, atol=0), what


@pytest.mark.parametrize("case", LOOKUP_CASES, ids=case_id)
def test_lookup_net_unfused(case):
	name, seed, games, depth, method, ff, radius = case
	policy, value, info = model_of(case)
	bf16 = "bf16" in name
	net = Recorded(net_of(name), torch.bfloat16 if bf16 else None)
	np.random.seed(seed)
	got = adi_traindata(net, games, depth, ALPHA, method, ff_batches=ff, ball=_ball(radius))
	_same(got, policy, value, orc.as_oh(info["states"]), games, depth, case)
	# the net saw exactly the model's slices of the outside rows, in order, in the dtype it asked for; none at all with count = 0
	assert [rows for rows, _ in net.calls] == info["calls"]
	assert {dt for _, dt in net.calls} <= {torch.bfloat16 if bf16 else torch.float32}


def _device_net(name):
	if name not in _DEVICE_NETS:
		import copy
		_DEVICE_NETS[name] = copy.deepcopy(net_of(name)).cuda().eval()   # the host net stays on the host: it is the model's
	return _DEVICE_NETS[name]


@pytest.mark.parametrize("case", LINEAR_CASES, ids=case_id)
def test_linear_net_unfused_and_fused(case):
	name, seed, games, depth, method, ff, radius = case
	policy, value, info = model_of(case)
	net = Recorded(_device_net(name))
	for mode in (False, True, "epilogue", "folded"):
		net.calls.clear()
		np.random.seed(seed)
		got = adi_traindata(net if mode is False else net.net, games, depth, ALPHA, method, ff_batches=ff, fused_first_layer=mode, ball=_ball(radius))
		_same(got, policy, value, orc.as_oh(info["states"]), games, depth, (case, mode))
		if mode is False:
			assert [rows for rows, _ in net.calls] == info["calls"]
			assert {dt for _, dt in net.calls} <= {torch.bfloat16 if "bf16" in name else torch.float32}


def _children(seed: int, games: int, depth: int, with_solved: bool):
	np.random.seed(seed)
	faces = np.random.randint(0, 6, (depth, games))
	dirs = np.random.randint(0, 2, (depth, games))
	acts = torch.from_numpy((2 * faces + (1 - dirs)).astype(np.uint8)).cuda()
	return cube.device.rollout_fanout(acts, with_solved)[2]


@pytest.mark.parametrize("radius,g", [(5, 1.0), (3, 0.0), (0, 1.0)])
def test_device_function_on_30000_rows(radius, g):
	ball = _ball(radius)
	sub = _children(501, 100, 25, True)
	assert sub.shape == (30000, 20)
	sentinel = np.float32(-12345.5)
	values = torch.full((30000,), float(sentinel), dtype=torch.float32, device="cuda")
	got_values, depths, rows, outside = cube.device.ball_child_values(ball, sub, g, values)
	assert got_values is values and depths.dtype == torch.int8 and rows.dtype == torch.int32 and outside.dtype == torch.int8
	assert all(t.is_cuda for t in (depths, rows, outside)) and outside.shape == (len(rows), 20)
	host = sub.cpu().numpy()
	want = ball.depth(host)                                              # the existing entry on the same rows
	assert (want == child_depths(host, radius)).all()
	assert (depths.cpu().numpy().astype(np.int64) == want).all()
	want_rows = np.nonzero(want < 0)[0]
	assert 0 < len(want_rows) < 30000
	assert (rows.cpu().numpy() == want_rows).all()
	assert (outside.cpu().numpy() == host[want_rows]).all()
	v = values.cpu().numpy()
	assert (bits(v[want >= 0]) == bits(vstar(want[want >= 0], g))).all()
	assert (bits(v[want_rows]) == bits(sentinel)).all()
	# without `values` a new tensor holds the same exact values
	v2, d2, r2, o2 = cube.device.ball_child_values(ball, sub, g)
	assert (bits(v2.cpu().numpy()[want >= 0]) == bits(v[want >= 0])).all() and torch.equal(d2, depths) and torch.equal(r2, rows) and torch.equal(o2, outside)


def test_device_function_with_no_child_outside_and_with_none_at_all():
	ball = _ball(1)
	solved = torch.from_numpy(orc.SOLVED.astype(np.int8)[None]).cuda()
	sub = cube.device.expand12(solved)[0]
	values, depths, rows, outside = cube.device.ball_child_values(ball, sub, 1.0)
	assert (depths.cpu().numpy() == 1).all() and (values.cpu().numpy() == 1.0).all() and rows.shape == (0,) and outside.shape == (0, 20)
	values, depths, rows, outside = cube.device.ball_child_values(ball, sub[:0], 1.0)
	assert values.shape == depths.shape == rows.shape == (0,) and outside.shape == (0, 20)
	with pytest.raises(ValueError):
		cube.device.ball_child_values(ball, sub[:11], 1.0)


def test_repr686_net():
	"""NoisyStubNet686 (exact integers) at 37 x 9, float32 and bfloat16 rows, against the model walking both representations."""
	net_seed, seed, games, depth, method, ff, radius = 4, 451, 37, 9, "lapanfix", 7, 3
	info = {}
	np.random.seed(seed)
	policy, value = adi_ball_model(NoisyStubNet686(net_seed), games, depth, method, ff, radius, repr686=True, info=info)
	assert 0.1 < 1 - info["count"] / (12 * games * depth) < 0.9
	oh = orc.as_oh686(info["states686"])
	try:
		cube.set_is2024(False)
		for dtype in (torch.float32, torch.bfloat16):
			net = Recorded(NoisyStubNet686(net_seed, dtype).cuda())
			np.random.seed(seed)
			got = adi_traindata(net, games, depth, ALPHA, method, ff_batches=ff, ball=_ball(radius))
			assert got[0].shape == (games * depth, 288)
			assert (got[0].cpu().numpy() == oh).all()
			assert (got[1].numpy() == policy).all() and (bits(got[2].numpy()) == bits(value)).all(), dtype
			assert [rows for rows, _ in net.calls] == info["calls"] and {dt for _, dt in net.calls} == {dtype}
	finally:
		cube.set_is2024(True)


def test_ball_none_is_the_call_without_the_argument():
	net = Recorded(net_of("lookup"))
	np.random.seed(461)
	a = adi_traindata(net, 37, 9, ALPHA, "lapanfix", ff_batches=7)
	calls = list(net.calls)
	net.calls.clear()
	np.random.seed(461)
	b = adi_traindata(net, 37, 9, ALPHA, "lapanfix", ff_batches=7, ball=None)
	assert net.calls == calls
	for x, y in zip(a, b):
		assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu())
	# and a ball changes them: the targets near solved no longer come from the net
	np.random.seed(461)
	c = adi_traindata(net, 37, 9, ALPHA, "lapanfix", ff_batches=7, ball=_ball(3))
	assert not torch.equal(a[2], c[2])


def test_other_balls_raise_type_error():
	net = Recorded(net_of("lookup"))
	for ball in (DeviceGoalBall(2), 3):
		with pytest.raises(TypeError):
			adi_traindata(net, 3, 2, ALPHA, "lapanfix", ball=ball)
		with pytest.raises(TypeError):
			cube.device.ball_child_values(ball, torch.zeros((12, 20), dtype=torch.int8, device="cuda"), 1.0)
	assert not net.calls


def test_entry_argument_errors_come_back_as_codes():
	lib = _ffi.lib()
	ball = _ball(1).build()
	h, stream = ball._h, _ffi.stream_ptr()
	sub = _children(502, 3, 2, True)
	m12 = len(sub)
	depth = torch.full((m12,), 77, dtype=torch.int8, device="cuda")
	values = torch.zeros(m12, dtype=torch.float32, device="cuda")
	rows = torch.zeros(m12, dtype=torch.int32, device="cuda")
	outside = torch.zeros((m12, 20), dtype=torch.int8, device="cuda")
	count = torch.full((1,), -5, dtype=torch.int32, device="cuda")
	scratch = torch.zeros(16, dtype=torch.uint8, device="cuda")
	good = [sub.data_ptr(), m12, 1.0, depth.data_ptr(), values.data_ptr(), rows.data_ptr(), outside.data_ptr(), count.data_ptr(), scratch.data_ptr(), 16]

	def call(handle=h, **change):
		args = list(good)
		for k, v in change.items():
			args[int(k[1:])] = v
		return lib.rk_symball_child_values(handle, *args, stream)
	assert call(handle=None) == -1
	for i in (0, 3, 4, 5, 6, 7, 8):                                      # every pointer
		assert call(**{f"a{i}": None}) == -1 and b"null pointer" in lib.rk_last_error(), i
	for i in (0, 4, 5, 6, 7, 8):                                         # every pointer read or written as dwords
		assert call(**{f"a{i}": good[i] + 1}) == -1 and b"aligned" in lib.rk_last_error(), i
	assert call(a1=m12 - 1) == -1 and b"twelve" in lib.rk_last_error()
	assert call(a1=(1 << 31) + 4) == -1                                  # a multiple of 12 above INT32_MAX
	assert call(a9=3) == -1 and b"scratch" in lib.rk_last_error()
	fresh = C.c_void_p()
	_ffi.check(lib.rk_symball_create(C.byref(fresh), 1, 16, 0))
	try:
		assert call(handle=fresh) == -4                                  # RK_ESTATE: not built
	finally:
		assert lib.rk_symball_destroy(fresh) == 0
	# nothing was launched: the outputs hold what they held
	torch.cuda.synchronize()
	assert (depth.cpu().numpy() == 77).all() and int(count.item()) == -5
	assert call() == 0
	k = int(count.item())
	want = child_depths(sub.cpu().numpy(), 1)
	assert (depth.cpu().numpy() == want).all() and k == int((want < 0).sum()) and (rows[:k].cpu().numpy() == np.nonzero(want < 0)[0]).all()
