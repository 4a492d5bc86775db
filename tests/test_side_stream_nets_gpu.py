"""
The first-layer and tail entries on a torch side stream behind a gate (tests/side_stream.py, pattern A): rk_ohl_forward on every
route, rk_ohl_set_epilogue, rk_ohl_set_weights, rk_ohl_backward, rk_tail_linear, StateLinear's autograd backward and one optimizer
step of train_on_states.  The inputs arrive on the side stream BEHIND the gate, over decoys of the same kind; outputs start as
sentinel bytes; everything is compared bit for bit with the same calls on the default stream by a second handle (whose behaviour
tests/test_oh_linear_exact_gpu.py and tests/test_ohl_backward_gpu.py pin against float64).  A launch or copy sent to stream 0
instead of the caller's stream runs during the gate, on the decoys, and the bits differ.
"""
import functools

import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.oh_linear import BACKWARD_MIN_ROWS, OhLinear, StateLinear, TailLinear, train_on_states
from tests import oh_linear_ref as R
from tests import ohl_backward_ref as B
from tests import side_stream as S
from tests.train_nets import SmallNet

pytestmark = pytest.mark.gpu

SEED = 41
H = 192
THREE_RANGES = 2 * BACKWARD_MIN_ROWS + 1


@functools.lru_cache(maxsize=None)
def _states(n, seed=SEED) -> torch.Tensor:
	return torch.from_numpy(R.random_states(n, seed + n)).cuda()


def _decoy_states(n) -> torch.Tensor:
	"""other codes in 0 .. 23 at every position (a fresh tensor: the true states are copied over it behind the gate)"""
	d = _states(n, SEED + 1000).clone()
	assert not torch.equal(d, _states(n))
	return d


def _layer(dtype, seed, bias=True, out_features=H):
	g = torch.Generator().manual_seed(seed)
	lin = torch.nn.Linear(480, out_features, bias=bias)
	with torch.no_grad():
		lin.weight.copy_(torch.randn((out_features, 480), generator=g) * 0.1)
		if bias:
			lin.bias.copy_(torch.randn(out_features, generator=g) * 0.3)
	return lin.cuda().to(dtype).requires_grad_(False)


def _affine(seed):
	g = torch.Generator().manual_seed(seed)
	return (torch.rand(H, generator=g) + 0.5).cuda(), torch.randn(H, generator=g).cuda()


def _set_epilogue(handle, scale, shift):
	_ffi.check(_ffi.lib().rk_ohl_set_epilogue(handle._h, _ffi.OHL_ACT_ELU, 1.0, scale.data_ptr(), shift.data_ptr(), _ffi.stream_ptr()))


def _out_dtype(route, dtype):
	return torch.bfloat16 if route.startswith("mfma") else dtype


def test_gate_is_calibrated_and_holds():
	"""the figures DESIGN.md quotes, and the gate doing what the other tests need of it: closed right after it is enqueued, open
	within its length (twice over, for a busy device)"""
	rate = S.sleep_rate()
	print(f"gate form: {S.gate_form()}; _sleep cycles per ms: {rate:.0f}")
	torch.cuda.synchronize()
	s = S.side_stream()
	ev = S.gate(s)
	S.held(ev)
	t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	torch.cuda.synchronize()
	with torch.cuda.stream(s):
		t[0].record()
		S.delay(S.GATE_MS)
		t[1].record()
	t[1].synchronize()
	ms = t[0].elapsed_time(t[1])
	print(f"a {S.GATE_MS:.0f} ms gate took {ms:.2f} ms")
	assert S.GATE_MS / 2 <= ms <= 2 * S.GATE_MS


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("route", ["gather", "mfma_direct", "mfma_tiled"])
def test_forward_behind_a_gate(route, dtype, n, epilogue):
	layer = _layer(dtype, SEED)
	mine, other = OhLinear(layer), OhLinear(layer)
	true = _states(n)
	scale, shift = _affine(SEED)
	if epilogue:
		_set_epilogue(other, scale, shift)
	want = other(true, route=route)
	buf = _decoy_states(n)
	out = S.sentinel((n, H), _out_dtype(route, dtype))
	sc, sh = _affine(SEED + 1)                        # decoy scale and shift
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		if epilogue:                                  # the epilogue's copies behind a gate of their own: the entry synchronises
			ev = S.gate(s)
			sc.copy_(scale, non_blocking=True)
			sh.copy_(shift, non_blocking=True)
			S.held(ev)
			_set_epilogue(mine, sc, sh)
		ev = S.gate(s)
		buf.copy_(true, non_blocking=True)
		mine(buf, out=out, route=route)
		S.held(ev)
		s.synchronize()
	assert S.same_bits(out, want), int((S.bits(out) != S.bits(want)).sum())
	assert not S.same_bits(want, other(_decoy_states(n), route=route))       # the decoy would have shown


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_set_weights_then_forward_behind_one_gate(dtype):
	"""rk_ohl_set_weights does not synchronise: the new weights reach their tensor behind the gate, the refresh and a forward follow at
	once, and the gate is still closed when both have been enqueued"""
	n = 1000
	old, new, decoy = _layer(dtype, SEED), _layer(dtype, SEED + 1), _layer(dtype, SEED + 2)
	code = _ffi.OH_F32 if dtype == torch.float32 else _ffi.OH_BF16
	for route in ("gather", "mfma_direct", "mfma_tiled"):
		mine, fresh = OhLinear(old), OhLinear(new)
		want = fresh(_states(n), route=route)
		w, b = decoy.weight.detach().clone(), decoy.bias.detach().clone()
		buf = _decoy_states(n)
		out = S.sentinel((n, H), _out_dtype(route, dtype))
		torch.cuda.synchronize()
		s = S.side_stream()
		with torch.cuda.stream(s):
			ev = S.gate(s)
			w.copy_(new.weight, non_blocking=True)
			b.copy_(new.bias, non_blocking=True)
			buf.copy_(_states(n), non_blocking=True)
			_ffi.check(_ffi.lib().rk_ohl_set_weights(mine._h, w.data_ptr(), code, b.data_ptr(), _ffi.stream_ptr()))
			mine(buf, out=out, route=route)
			S.held(ev)
			s.synchronize()
		assert S.same_bits(out, want), route
		assert not S.same_bits(want, OhLinear(old)(_states(n), route=route))


def _int_dy(n, seed) -> torch.Tensor:
	g = torch.Generator().manual_seed(seed)
	return torch.randint(-8, 9, (n, H), generator=g).float().cuda()


def _backward(eng, states, dy, dw, db):
	_ffi.check(_ffi.lib().rk_ohl_backward(eng._h, states.data_ptr(), dy.data_ptr(), len(dy), dw.data_ptr(), db.data_ptr() if db is not None else None,
	                                      _ffi.stream_ptr()))


def test_backward_three_row_ranges_behind_a_gate():
	"""rk_ohl_backward at 2 * BACKWARD_MIN_ROWS + 1 rows: three row ranges and the second launch that sums their partial slices.  Integer
	dY, so the float64 reference is exact.  The handle's partial buffer holds a decoy call's slices when the gated call starts."""
	n = THREE_RANGES
	layer = _layer(torch.float32, SEED)
	mine, other = OhLinear(layer, "gather"), OhLinear(layer, "gather")
	states, dy = _states(n), _int_dy(n, SEED)
	sbuf, ybuf = _decoy_states(n), _int_dy(n, SEED + 1)
	dw, db = S.sentinel((H, 480), torch.float32), S.sentinel((H,), torch.float32)
	_backward(mine, sbuf, ybuf, dw, db)               # the decoy call on the default stream: allocates the partial slices and fills them
	decoy_dw = dw.clone()
	S.bits(dw).fill_(S.SENTINEL)
	S.bits(db).fill_(S.SENTINEL)
	want_w, want_b = torch.empty_like(dw), torch.empty_like(db)
	_backward(other, states, dy, want_w, want_b)
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		ev = S.gate(s)
		sbuf.copy_(states, non_blocking=True)
		ybuf.copy_(dy, non_blocking=True)
		_backward(mine, sbuf, ybuf, dw, db)
		S.held(ev)
		s.synchronize()
	assert S.same_bits(dw, want_w), int((S.bits(dw) != S.bits(want_w)).sum())
	assert S.same_bits(db, want_b)
	dW, dB, _, _, _ = B.first_layer_grad64(states, dy)
	assert float(dW.abs().max()) < 2 ** 24
	assert S.same_bits(dw, dW.float()) and S.same_bits(db, dB.float())
	assert not S.same_bits(decoy_dw, want_w)


@pytest.mark.parametrize("n,K,M,act", [(37, 512, 1, None), (37, 512, 1, "elu"), (16 * 9 + 5, 512, 13, "elu")])
def test_tail_linear_behind_a_gate(n, K, M, act):
	"""rk_tail_linear through TailLinear: one workgroup takes 16 rows, neither n is a multiple"""
	torch.manual_seed(K + M)
	lin = torch.nn.Linear(K, M).cuda().to(torch.bfloat16).requires_grad_(False)
	tail = TailLinear(R.module_of(act), lin)
	g = torch.Generator(device="cuda").manual_seed(n)
	x = (torch.randn(n, K, device="cuda", generator=g) * 1.5).to(torch.bfloat16)
	buf = (torch.randn(n, K, device="cuda", generator=g) * 1.5).to(torch.bfloat16)
	want = tail(x)
	assert not S.same_bits(want, tail(buf))
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		ev = S.gate(s)
		buf.copy_(x, non_blocking=True)
		got = tail(buf)
		S.held(ev)
		s.synchronize()
	assert S.same_bits(got, want)


@pytest.mark.parametrize("bias", [True, False])
def test_state_linear_autograd_on_the_forwards_stream(bias):
	"""StateLinear forward and loss.backward() inside torch.cuda.stream(s): autograd runs the backward on the forward's stream and
	_ffi.stream_ptr() must see that stream there.  .grad bit for bit equal to the default-stream run."""
	n = THREE_RANGES
	lin = _layer(torch.float32, SEED, bias=bias)
	lin.requires_grad_(True)
	layer = StateLinear(lin)
	states = _states(n)
	coef = _int_dy(n, SEED + 5)

	def grads(rows):
		for p in layer.parameters():
			p.grad = None
		(layer(rows) * coef).sum().backward()
		return [p.grad for p in layer.parameters()]

	want = [g.clone() for g in grads(states)]
	decoy = [g.clone() for g in grads(_decoy_states(n))]          # and the handle's partial slices now hold the decoy's
	assert not S.same_bits(decoy[0], want[0])
	buf = _decoy_states(n)
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		ev = S.gate(s)
		buf.copy_(states, non_blocking=True)
		got = grads(buf)
		S.held(ev)
		s.synchronize()
	assert len(got) == (2 if bias else 1)
	for a, b in zip(got, want):
		assert S.same_bits(a, b)


def test_one_training_step_on_states_behind_a_gate():
	"""One SGD step of train_on_states on the smallest training net at 65 rows, training-mode BatchNorm included: every parameter and
	buffer after the step bit for bit equal to the default-stream step.  (A first step of a third net warms the side stream up -- BLAS
	handle, workspaces, the allocator's blocks -- so that the gated step only enqueues.)"""
	n = 65
	states = _states(n)
	g = torch.Generator().manual_seed(SEED)
	target_p = torch.randint(0, 12, (n,), generator=g).cuda()
	target_v = torch.randn(n, 1, generator=g).cuda()

	def step(net, forward, opt, rows):
		opt.zero_grad(set_to_none=True)
		p, v = forward(rows)
		loss = torch.nn.functional.cross_entropy(p, target_p) + torch.nn.functional.mse_loss(v, target_v)
		loss.backward()
		opt.step()

	def make():
		net = SmallNet(seed=SEED).cuda().train()
		return net, train_on_states(net), torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9)

	ref, mine, warm = make(), make(), make()
	step(*ref, states)
	buf = _decoy_states(n)
	torch.cuda.synchronize()
	s = S.side_stream()
	with torch.cuda.stream(s):
		step(*warm, buf)
		s.synchronize()
		ev = S.gate(s)
		buf.copy_(states, non_blocking=True)
		step(*mine, buf)
		S.held(ev)
		s.synchronize()
	a, b = ref[0].state_dict(), mine[0].state_dict()
	assert a.keys() == b.keys()
	for k in a:
		assert S.same_bits(a[k], b[k]), k
	fresh = SmallNet(seed=SEED).cuda().state_dict()
	assert not S.same_bits(a["shared_net.0.weight"], fresh["shared_net.0.weight"])      # the step moved the first layer
