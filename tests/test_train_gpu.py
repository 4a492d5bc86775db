"""
`librubiks_amd.train.Train` against the reference loop restated here in plain torch (`_restated`, every step citing librubiks/train.py), and
the `return_states` option of the two data sources.

Shapes: the small net of tests/train_nets.py, 3 rollouts of 4 games x depth 5 (20 states: batches of 8, 8 and 4), update_interval = 1,
alpha_update = 0.5, gamma = 0.5, tau = 0.5, seeded np.random and torch.  Both sides issue the same torch operations on the same tensors in
the same order, so the losses per rollout and the final parameters are compared bit for bit -- unless the restated loop itself, run twice,
is not bit-reproducible on this torch build: then within 4 x ITS run-to-run spread (never Train's).  Measured on the MI355X: spread 0, both
paths, so the comparison made is equality.
"""
import copy

import numpy as np
import pytest
import torch

from librubiks_amd import cube
from librubiks_amd.adi import adi_traindata, ball_traindata
from librubiks_amd.oh_linear import train_on_states
from librubiks_amd.solving.agents import DeviceSymBall, ValueSearch
from librubiks_amd.solving.evaluation import Evaluator
from librubiks_amd.train import Train
from tests import oh_linear_ref as R
from tests.train_nets import SmallNet

pytestmark = pytest.mark.gpu

ROLLOUTS, GAMES, DEPTH, BATCH, LR, GAMMA, TAU, ALPHA_UPDATE, SEED = 3, 4, 5, 8, 1e-3, 0.5, 0.5, 0.5, 77


def _seed():
	np.random.seed(SEED)
	torch.manual_seed(SEED)


def _restated(net, first_layer):
	"""train.py:138-201 in plain torch with the first-layer path under test -> what a run leaves behind"""
	gen = copy.deepcopy(net)                                                                             # :138
	alpha = 1 if ALPHA_UPDATE == 1 else 0                                                                # :140
	opt = torch.optim.RMSprop(net.parameters(), lr=LR)                                                   # :141
	sched = torch.optim.lr_scheduler.StepLR(opt, 1, GAMMA)                                               # :142
	pc, vc = torch.nn.CrossEntropyLoss(reduction="none"), torch.nn.MSELoss(reduction="none")            # :84-85
	pl, vl, alphas, lrs, steps = np.zeros(ROLLOUTS), np.zeros(ROLLOUTS), [], [], 0
	fwd = train_on_states(net) if first_layer == "states" else net
	for rollout in range(ROLLOUTS):                                                                      # :148
		gp, npar = gen.state_dict(), net.state_dict()                                                    # :151, :341-352 (tau != 1)
		new = dict(gp)
		for k, p in npar.items():
			new[k].data.copy_(TAU * p.data + (1 - TAU) * new[k].data)
		gen.load_state_dict(new)
		alphas.append(alpha)
		lrs.append(opt.param_groups[0]["lr"])
		data, pt, vt, lw = adi_traindata(gen, GAMES, DEPTH, alpha, "lapanfix", return_states=first_layer == "states")      # :154
		data, pt, vt, lw = data.cuda(), pt.cuda(), vt.cuda(), lw.cuda()                                  # :156-159
		net.train()                                                                                      # :166
		size = GAMES * DEPTH                                                                             # :167, :401-410
		nb = int(np.ceil(size / BATCH))
		idcs = np.arange(size)
		np.random.shuffle(idcs)
		batches = [slice(b * BATCH, (b + 1) * BATCH) for b in range(nb)]
		batches[-1] = slice(batches[-1].start, size)
		for batch in batches:                                                                            # :168-179
			opt.zero_grad()
			pp, vp = fwd(data[batch], policy=True, value=True)
			ploss = pc(pp, pt[batch]) * lw[batch]
			vloss = vc(vp.squeeze(), vt[batch]) * lw[batch]
			torch.mean(ploss + vloss).backward()
			opt.step()
			steps += 1
			pl[rollout] += ploss.detach().cpu().numpy().mean() / len(batches)
			vl[rollout] += vloss.detach().cpu().numpy().mean() / len(batches)
		if rollout and rollout % 1 == 0:                                                                 # :191-201 (update_interval = 1)
			sched.step()
			if alpha + ALPHA_UPDATE <= 1 or np.isclose(alpha + ALPHA_UPDATE, 1):
				alpha += ALPHA_UPDATE
			elif alpha < 1:
				alpha = 1
	alphas.append(alpha)
	lrs.append(opt.param_groups[0]["lr"])
	return dict(pl=pl, vl=vl, alphas=alphas, lrs=lrs, steps=steps, rng=np.random.get_state(),
	            params=[p.detach().clone() for p in net.state_dict().values()])


def _run_restated(first_layer):
	_seed()
	return _restated(SmallNet(seed=SEED).cuda(), first_layer)


def _run_train(first_layer, **kw):
	_seed()
	net = SmallNet(seed=SEED).cuda()
	t = Train(ROLLOUTS, BATCH, GAMES, DEPTH, torch.optim.RMSprop, ALPHA_UPDATE, LR, GAMMA, 1, tau=TAU, reward_method="lapanfix",
	          first_layer=first_layer, **kw)
	out, best = t.train(net)
	assert out is net and best is not net
	return t, net, best


def _same_rng(a, b):
	return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("first_layer", ["states", "onehot"])
def test_train_is_the_restated_reference_loop(first_layer):
	a, b = _run_restated(first_layer), _run_restated(first_layer)
	spread_l = max(np.abs(a["pl"] - b["pl"]).max(), np.abs(a["vl"] - b["vl"]).max())
	spread_p = max(float((x.double() - y.double()).abs().max()) for x, y in zip(a["params"], b["params"]))
	print(f"restated loop ({first_layer}) run twice: loss spread {spread_l:.3g}, parameter spread {spread_p:.3g}")
	t, net, _ = _run_train(first_layer)
	got = [p.detach() for p in net.state_dict().values()]
	if spread_l == 0 and spread_p == 0:
		assert np.array_equal(t.policy_losses, a["pl"]) and np.array_equal(t.value_losses, a["vl"])
		assert all(torch.equal(x, y) for x, y in zip(got, a["params"]))
	else:                                                                   # torch itself is not reproducible here: 4 x ITS spread
		assert np.abs(t.policy_losses - a["pl"]).max() <= 4 * spread_l and np.abs(t.value_losses - a["vl"]).max() <= 4 * spread_l
		assert all(float((x.double() - y.double()).abs().max()) <= 4 * spread_p for x, y in zip(got, a["params"]))
	assert np.array_equal(t.train_losses, t.policy_losses + t.value_losses) and np.isfinite(t.train_losses).all()
	assert t.alphas == a["alphas"] == [0, 0, 0.5, 1.0]                       # as applied per rollout, then what is left: 0, .5, 1 in turn
	assert t.lrs == a["lrs"] and np.allclose(t.lrs, [LR, LR, LR / 2, LR / 4], rtol=1e-12)
	assert t.optimizer_steps == a["steps"] == ROLLOUTS * 3
	assert _same_rng(np.random.get_state(), a["rng"])
	assert t.sol_percents == [] and len(t.evaluation_rollouts) == 0


def test_states_and_onehot_first_batch_losses_agree_within_the_forward_bound():
	"""Rollout 0, first batch, identical initial nets and identical ADI data (asserted).  The two paths differ in the first layer alone: each
	is within 21 u mag of the exact pre-activation x (oh_linear_ref.assert_f32_preactivation: twenty float32 adds; a GEMM over a one-hot row
	adds the same twenty non-zero terms and exact zeros), so they differ by at most d = 42 u mag.  Pushed through the loss in float64 -- the
	rest of the net, training-mode BatchNorm included, evaluated in float64 on each path's own float32 first-layer output -- the losses
	differ by at most sum |dL/dx| d to first order; the bound allows twice that for the higher orders (d / |x| is below 1e-5)."""
	_seed()
	net = SmallNet(seed=SEED).cuda()
	states, pt, vt, lw = adi_traindata(net, GAMES, DEPTH, 0, "lapanfix", return_states=True)
	_seed()
	oh, pt2, vt2, lw2 = adi_traindata(net, GAMES, DEPTH, 0, "lapanfix")
	assert torch.equal(cube.device.as_oh(states), oh) and torch.equal(pt, pt2) and torch.equal(vt, vt2) and torch.equal(lw, lw2)
	b = slice(0, BATCH)
	pt, vt, lw = pt.cuda()[b], vt.cuda()[b].double(), lw.cuda()[b].double()
	lin = net.shared_net[0]
	with torch.no_grad():
		x_s = train_on_states(net).first(states[b])
		x_o = torch.nn.functional.linear(oh[b], lin.weight, lin.bias)
	x64, mag = R.first_layer64(states[b], lin.weight, lin.bias)
	R.assert_f32_preactivation(x_s, x64, mag, "states path")
	R.assert_f32_preactivation(x_o, x64, mag, "one-hot path")
	net64 = copy.deepcopy(net).double().train()

	def loss64(x):
		x = x.double().clone().requires_grad_(True)
		h = net64.shared_net[1:](x)
		pp, vp = net64.policy_net(h), net64.value_net(h)
		pl = torch.nn.functional.cross_entropy(pp, pt, reduction="none") * lw
		vl = torch.nn.functional.mse_loss(vp.squeeze(), vt, reduction="none") * lw
		loss = torch.mean(pl + vl)
		loss.backward()
		return float(loss.detach()), x.grad
	l_s, _ = loss64(x_s)
	l_o, _ = loss64(x_o)
	_, g = loss64(x64)
	bound = 2 * float((g.abs() * 42 * R.U * mag).sum())
	print(f"first-batch loss: states {l_s!r}, one-hot {l_o!r}, |difference| {abs(l_s - l_o):.3g}, bound {bound:.3g}")
	assert bound < 1e-3 * abs(l_s) and abs(l_s - l_o) <= bound                # (a bound that binds: far below the loss itself)


def test_return_states_of_both_data_sources():
	net = SmallNet(seed=3).cuda()
	_seed()
	oh, pt, vt, lw = adi_traindata(net, GAMES, DEPTH, 0.5, "lapanfix")
	rng_default = np.random.get_state()
	_seed()
	oh2, pt2, vt2, lw2 = adi_traindata(net, GAMES, DEPTH, 0.5, "lapanfix")                               # the default call: unchanged and repeatable
	assert _same_rng(np.random.get_state(), rng_default)
	assert oh.shape == (GAMES * DEPTH, 480) and oh.dtype == torch.float32 and oh.is_cuda and not pt.is_cuda and pt.dtype == torch.int64
	assert torch.equal(oh, oh2) and torch.equal(pt, pt2) and torch.equal(vt, vt2) and torch.equal(lw, lw2)
	_seed()
	st, pt3, vt3, lw3 = adi_traindata(net, GAMES, DEPTH, 0.5, "lapanfix", return_states=True)
	assert _same_rng(np.random.get_state(), rng_default)
	assert st.shape == (GAMES * DEPTH, 20) and st.dtype == torch.int8 and st.is_cuda
	assert torch.equal(cube.device.as_oh(st), oh) and torch.equal(pt, pt3) and torch.equal(vt, vt3) and torch.equal(lw, lw3)
	ball = DeviceSymBall(4)
	a = ball_traindata(ball, 50, None, np.random.default_rng(5))
	c = ball_traindata(ball, 50, None, np.random.default_rng(5), return_states=True)
	assert c[0].shape == (50, 20) and c[0].dtype == torch.int8 and c[0].is_cuda and a[0].shape == (50, 480)
	assert torch.equal(cube.device.as_oh(c[0]), a[0]) and all(torch.equal(x, y) for x, y in zip(a[1:], c[1:]))
	cube.set_is2024(False)
	with pytest.raises(ValueError):
		adi_traindata(net, GAMES, DEPTH, 0.5, "lapanfix", return_states=True)
	with pytest.raises(ValueError):
		ball_traindata(ball, 5, None, np.random.default_rng(5), return_states=True)


class _RecordingEvaluator(Evaluator):
	"""keeps the agent's net as it was at every evaluation"""
	def eval(self, agent, batched=None):
		self.seen = getattr(self, "seen", []) + [copy.deepcopy(agent.net.state_dict())]
		return super().eval(agent, batched)


def test_ball_targets_evaluations_and_best_net():
	_seed()
	net = SmallNet(seed=SEED).cuda()
	ev = _RecordingEvaluator(n_games=6, scrambling_depths=[2], max_states=30)
	t = Train(ROLLOUTS, BATCH, GAMES, DEPTH, torch.optim.RMSprop, ALPHA_UPDATE, LR, GAMMA, 1, agent=ValueSearch(net), evaluator=ev,
	          evaluation_interval=1, tau=TAU, reward_method="lapanfix", ball=DeviceSymBall(4))
	assert t.evaluation_rollouts.tolist() == [0, 1, 2]
	out, best = t.train(net)
	assert out is net and best is not net and ev.last_mode == "batched"
	assert len(t.sol_percents) == 3 == len(ev.seen) and all(0 <= s <= 1 for s in t.sol_percents)
	assert np.isfinite(t.train_losses).all()
	assert t.agent.net is net and not net.training
	if max(t.sol_percents) > 0:
		at = ev.seen[int(np.argmax(t.sol_percents))]                        # the first evaluation that reached the best share
		assert all(torch.equal(v, at[k]) for k, v in best.state_dict().items())
	assert all(p is not q for p, q in zip(best.parameters(), net.parameters()))
