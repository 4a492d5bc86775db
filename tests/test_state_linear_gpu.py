"""
`StateLinear` and `train_on_states` (librubiks_amd/oh_linear.py): the first layer on 20-byte states as an autograd module that SHARES the
net's Parameters and follows their live values.

Exactness: the weights are dyadic (multiples of 2^-6, |w| <= 2), the upstream gradient G is integer-valued and loss = (y * G).sum(), so the
output (a bias and twenty weights), dW (sums of integers) and db are exact in float32 in any order, and must equal what nn.Linear in float64
gives on as_oh(states): equal as numbers, every element.  The same holds after an SGD step with lr = 0.5 on those numbers, which is what shows
that the forward follows the live weights; a module that snapshots them at construction fails `test_forward_follows_live_weights`.
"""
import copy

import numpy as np
import pytest
import torch

from librubiks_amd import cube
from librubiks_amd.oh_linear import OhLinear, StateLinear, train_on_states
from tests import oh_linear_ref as R
from tests.helpers import random_walk
from tests.train_nets import SmallNet

pytestmark = pytest.mark.gpu

N, H, SEED = 300, 128, 31


def _dyadic_layer(bias=True, seed=SEED):
	g = torch.Generator().manual_seed(seed)
	lin = torch.nn.Linear(480, H, bias=bias)
	with torch.no_grad():
		lin.weight.copy_(torch.randint(-128, 129, (H, 480), generator=g).float() / 64)
		if bias:
			lin.bias.copy_(torch.randint(-128, 129, (H,), generator=g).float() / 64)
	return lin.cuda()


def _states():
	return torch.from_numpy(np.concatenate([R.cover_states(SEED)[:200], random_walk(N - 200, 12, seed=SEED)])).cuda()


def _G():
	return torch.randint(-8, 9, (N, H), generator=torch.Generator().manual_seed(SEED + 1)).float().cuda()


def _model64(lin, states, G):
	"""nn.Linear in float64 on the one-hot rows, loss = (y * G).sum() -> (y, weight.grad, bias.grad)"""
	ref = torch.nn.Linear(480, H, bias=lin.bias is not None).cuda().double()
	with torch.no_grad():
		ref.weight.copy_(lin.weight.detach().double())
		if lin.bias is not None:
			ref.bias.copy_(lin.bias.detach().double())
	y = ref(cube.device.as_oh(states).double())
	(y * G.double()).sum().backward()
	return y.detach(), ref.weight.grad, ref.bias.grad if lin.bias is not None else None


@pytest.mark.parametrize("bias", [True, False])
def test_exact_output_and_gradients(bias):
	lin, states, G = _dyadic_layer(bias), _states(), _G()
	first = StateLinear(lin)
	y = first(states)
	assert y.dtype == torch.float32 and y.shape == (N, H) and y.requires_grad
	(y * G).sum().backward()
	y64, dW64, db64 = _model64(lin, states, G)
	assert torch.equal(y.detach().double(), y64)
	assert lin.weight.grad.shape == (H, 480) and torch.equal(lin.weight.grad.double(), dW64)
	if bias:
		assert torch.equal(lin.bias.grad.double(), db64)
	else:
		assert lin.bias is None and first.bias is None
	assert states.grad is None and not states.requires_grad
	# bit-identical to the inference module made at this moment
	assert torch.equal(y.detach().view(torch.int32), OhLinear(lin, "gather")(states).view(torch.int32))
	# a second backward accumulates into .grad like any torch layer (the kernel overwrites its own output, autograd adds)
	(first(states) * G).sum().backward()
	assert torch.equal(lin.weight.grad.double(), 2 * dW64)


def test_parameters_are_the_nets_own():
	net = SmallNet(seed=1).cuda()
	keys, ids = list(net.state_dict().keys()), [id(p) for p in net.parameters()]
	f = train_on_states(net)
	assert f.first.weight is net.shared_net[0].weight and f.first.bias is net.shared_net[0].bias
	assert id(f.first.weight) == ids[0] and id(f.first.bias) == ids[1]
	assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == ids
	assert [id(p) for p in f.first.parameters()] == ids[:2]


def test_forward_follows_live_weights():
	lin, states, G = _dyadic_layer(), _states(), _G()
	first = StateLinear(lin)
	opt = torch.optim.SGD(lin.parameters(), lr=0.5)
	(first(states) * G).sum().backward()
	before = lin.weight.detach().clone()
	opt.step()                                                              # w - 0.5 * (integer): still dyadic, still exact
	assert not torch.equal(before, lin.weight.detach())
	opt.zero_grad()
	y = first(states)
	(y * G).sum().backward()
	y64, dW64, db64 = _model64(lin, states, G)
	assert torch.equal(y.detach().double(), y64) and torch.equal(lin.weight.grad.double(), dW64) and torch.equal(lin.bias.grad.double(), db64)
	# param.data.copy_(...) does not move the version counter autograd sees on the Parameter (train.py:347 writes this way)
	other = _dyadic_layer(seed=SEED + 5)
	lin.weight.data.copy_(other.weight.data)
	lin.bias.data.copy_(other.bias.data)
	assert torch.equal(first(states).detach().double(), _model64(other, states, G)[0])
	# load_state_dict, and a forward under no_grad
	third = _dyadic_layer(seed=SEED + 6)
	lin.load_state_dict(third.state_dict())
	with torch.no_grad():
		y = first(states)
	assert not y.requires_grad and torch.equal(y.double(), _model64(third, states, G)[0])


def test_constructor_refusals():
	with pytest.raises(ValueError):
		StateLinear(torch.nn.Linear(288, 64).cuda())
	with pytest.raises(ValueError):
		StateLinear(torch.nn.Linear(480, 64))                               # not on the GPU
	with pytest.raises(ValueError):
		StateLinear(torch.nn.Linear(480, 64).cuda().to(torch.bfloat16))
	with pytest.raises(ValueError):
		StateLinear(torch.nn.Linear(480, 96).cuda())
	first = StateLinear(torch.nn.Linear(480, 64).cuda())
	with pytest.raises(ValueError):
		first(torch.zeros((4, 20), dtype=torch.int64, device="cuda"))
	with pytest.raises(TypeError):
		train_on_states(torch.nn.Linear(480, 64).cuda())


def test_train_on_states_is_the_live_net():
	net = SmallNet(seed=2).cuda()
	states = _states()
	with torch.no_grad():                                                   # running statistics worth applying
		for m in net.modules():
			if isinstance(m, torch.nn.BatchNorm1d):
				m.running_mean.uniform_(-0.3, 0.3)
				m.running_var.uniform_(0.5, 1.5)
	twin = copy.deepcopy(net)
	f = train_on_states(net)

	def by_hand(n):
		x = OhLinear(n.shared_net[0], "gather")(states)
		x = n.shared_net[1:](x)
		return n.policy_net(x), n.value_net(x)
	net.eval(), twin.eval()
	with torch.no_grad():
		p, v = f(states)
		hp, hv = by_hand(twin)
		assert torch.equal(p.view(torch.int32), hp.view(torch.int32)) and torch.equal(v.view(torch.int32), hv.view(torch.int32))
		assert torch.equal(f(states, policy=False), v) and torch.equal(f(states, value=False), p)
	assert p.shape == (N, 12) and v.shape == (N, 1)
	stats = lambda n: [b.clone() for m in n.modules() if isinstance(m, torch.nn.BatchNorm1d) for b in (m.running_mean, m.running_var, m.num_batches_tracked)]
	frozen = stats(net)
	assert all(torch.equal(a, b) for a, b in zip(frozen, stats(twin)))
	net.train(), twin.train()
	p, v = f(states)
	assert p.requires_grad and v.requires_grad
	by_hand(twin)
	moved, want = stats(net), stats(twin)
	assert len(moved) == 12 and all(torch.equal(a, b) for a, b in zip(moved, want))
	assert not any(torch.equal(a, b) for a, b in zip(moved, frozen))
	# and every parameter of the net gets a gradient through it
	(p.sum() + v.sum()).backward()
	assert all(q.grad is not None for q in net.parameters())
