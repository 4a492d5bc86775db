"""
The reference's training loop on the device data sources (reference: `Train`, librubiks/train.py:28-247, :341-352, :401-410).

    train = Train(rollouts, batch_size, rollout_games, rollout_depth, optim_fn, alpha_update, lr, gamma, update_interval,
                  tau=..., reward_method=..., agent=ValueSearch(net), evaluator=Evaluator(...), evaluation_interval=...)
    net, best_net = train.train(net)

`train()` is the loop of train.py:138-225 line for line -- the generator net mixed with `tau`, alpha and the learning rate on the reference's
schedule, its batches (with the shuffle of an index array it then does not use: the draw is part of the RNG stream), its per-batch loss
bookkeeping, its evaluation and best-net rule -- with two differences, both about where the data lives:

  * the rollout's data comes from `adi.adi_traindata` (one launch for the walks and the fan-out, `ball=` for exact targets inside the
    symmetry ball); the targets and weights go to the GPU once per rollout;
  * `first_layer="states"` (the default) trains on the 20-byte states themselves: `adi_traindata(..., return_states=True)` and
    `oh_linear.train_on_states(net)`, whose first layer reads states and has its own backward kernel -- the (games * depth, 480) float32
    one-hot (432 MB at 7 500 x 30) never exists and the layer's weight gradient is not a dense GEMM against it.  `first_layer="onehot"`
    is the reference's own path, `net(oh[batch])`.

No plotting, no analysis, no logger: `policy_losses`, `value_losses`, `train_losses`, `sol_percents` and `evaluation_rollouts` are the
results.  float32 nets of the 20-byte representation for "states"; "onehot" takes whatever `adi_traindata` serves.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from librubiks_amd import gpu
from librubiks_amd.adi import adi_traindata


class Train:
	def __init__(self, rollouts: int, batch_size: int, rollout_games: int, rollout_depth: int, optim_fn, alpha_update: float, lr: float,
	             gamma: float, update_interval: int, agent=None, evaluator=None, evaluation_interval: int = 0, tau: float = 1.0,
	             reward_method: str = "lapanfix", policy_criterion=torch.nn.CrossEntropyLoss, value_criterion=torch.nn.MSELoss,
	             first_layer: str = "states", ball=None, adi_ff_batches: int = 1, fused_first_layer=False):
		if first_layer not in ("states", "onehot"):
			raise ValueError('first_layer is "states" or "onehot"')
		if evaluation_interval and (agent is None or evaluator is None):
			raise ValueError("evaluations need an agent and an evaluator (evaluation_interval=0: none)")
		self.rollouts = rollouts
		self.train_rollouts = np.arange(self.rollouts)
		self.rollout_games, self.rollout_depth = rollout_games, rollout_depth
		self.states_per_rollout = rollout_depth * rollout_games
		self.batch_size = self.states_per_rollout if not batch_size else batch_size                      # train.py:58
		self.adi_ff_batches = adi_ff_batches
		self.reward_method = reward_method
		if evaluation_interval:                                                                          # train.py:65-74
			self.evaluation_rollouts = np.arange(0, self.rollouts, evaluation_interval) - 1
			if evaluation_interval == 1:
				self.evaluation_rollouts = self.evaluation_rollouts[1:]
			else:
				self.evaluation_rollouts[0] = 0
			if self.rollouts - 1 != self.evaluation_rollouts[-1]:
				self.evaluation_rollouts = np.append(self.evaluation_rollouts, self.rollouts - 1)
		else:
			self.evaluation_rollouts = np.array([])
		self.agent, self.evaluator = agent, evaluator
		self.tau, self.alpha_update, self.lr, self.gamma, self.update_interval = tau, alpha_update, lr, gamma, update_interval
		self.optim = optim_fn
		self.policy_criterion = policy_criterion(reduction="none")
		self.value_criterion = value_criterion(reduction="none")
		self.first_layer, self.ball, self.fused_first_layer = first_layer, ball, fused_first_layer
		self.policy_losses = self.value_losses = self.train_losses = None
		self.sol_percents = []
		self.alphas, self.lrs, self.optimizer_steps = [], [], 0          # alpha and learning rate every rollout ran with, then the values left behind

	@staticmethod
	def _clone(net):
		return net.clone() if hasattr(net, "clone") else copy.deepcopy(net)

	def train(self, net):
		"""train.py:111-247 -> (the net after the last rollout, the net with the best evaluation)"""
		best_solve = 0
		best_net = self._clone(net)                                                                      # train.py:133
		if self.agent is not None:
			self.agent.net = net
		generator_net = self._clone(net)                                                                 # train.py:138
		alpha = 1 if self.alpha_update == 1 else 0
		optimizer = self.optim(net.parameters(), lr=self.lr)
		lr_scheduler = torch.optim.lr_scheduler.StepLR(optimizer, 1, self.gamma)
		self.policy_losses = np.zeros(self.rollouts)
		self.value_losses = np.zeros(self.rollouts)
		self.train_losses = np.empty(self.rollouts)
		self.sol_percents = []
		self.alphas, self.lrs, self.optimizer_steps = [], [], 0
		states_first = self.first_layer == "states"
		forward = None
		if states_first:
			from librubiks_amd.oh_linear import train_on_states
			forward = train_on_states(net)

		for rollout in range(self.rollouts):
			generator_net = self._update_gen_net(generator_net, net) if self.tau != 1 else net          # train.py:151
			self.alphas.append(alpha)
			self.lrs.append(optimizer.param_groups[0]["lr"])
			training_data, policy_targets, value_targets, loss_weights = adi_traindata(                  # train.py:154
				generator_net, self.rollout_games, self.rollout_depth, alpha, self.reward_method, ff_batches=self.adi_ff_batches,
				fused_first_layer=self.fused_first_layer, ball=self.ball, return_states=states_first)
			training_data = training_data.to(gpu)                                                        # train.py:156-159, once per rollout
			policy_targets, value_targets, loss_weights = policy_targets.to(gpu), value_targets.to(gpu), loss_weights.to(gpu)

			net.train()                                                                                  # train.py:166
			batches = self._get_batches(self.states_per_rollout, self.batch_size)
			for batch in batches:
				optimizer.zero_grad()
				if states_first:
					policy_pred, value_pred = forward(training_data[batch], policy=True, value=True)
				else:
					policy_pred, value_pred = net(training_data[batch], policy=True, value=True)
				policy_loss = self.policy_criterion(policy_pred, policy_targets[batch]) * loss_weights[batch]      # train.py:173-175
				value_loss = self.value_criterion(value_pred.squeeze(), value_targets[batch]) * loss_weights[batch]
				loss = torch.mean(policy_loss + value_loss)
				loss.backward()
				optimizer.step()
				self.optimizer_steps += 1
				self.policy_losses[rollout] += policy_loss.detach().cpu().numpy().mean() / len(batches)   # train.py:178-179
				self.value_losses[rollout] += value_loss.detach().cpu().numpy().mean() / len(batches)
			self.train_losses[rollout] = self.policy_losses[rollout] + self.value_losses[rollout]

			if rollout and self.update_interval and rollout % self.update_interval == 0:                 # train.py:191-201
				if self.gamma != 1:
					lr_scheduler.step()
				if (alpha + self.alpha_update <= 1 or np.isclose(alpha + self.alpha_update, 1)) and self.alpha_update:
					alpha += self.alpha_update
				elif alpha < 1 and alpha + self.alpha_update > 1 and self.alpha_update:
					alpha = 1

			if rollout in self.evaluation_rollouts:                                                      # train.py:211-225
				net.eval()
				self.agent.net = net
				eval_results, _, _ = self.evaluator.eval(self.agent)
				eval_reward = (eval_results != -1).mean()
				self.sol_percents.append(eval_reward)
				if eval_reward > best_solve:
					best_solve = eval_reward
					best_net = self._clone(net)
		self.alphas.append(alpha)                                        # ... and what the next rollout would have run with
		self.lrs.append(optimizer.param_groups[0]["lr"])
		return net, best_net

	def _update_gen_net(self, generator_net, net):
		"""train.py:341-352: the generator's parameters and buffers become tau * net's + (1 - tau) * its own"""
		genparams, netparams = generator_net.state_dict(), net.state_dict()
		new_genparams = dict(genparams)
		for pname, param in netparams.items():
			new_genparams[pname].data.copy_(self.tau * param.data.to(gpu) + (1 - self.tau) * new_genparams[pname].data.to(gpu))
		generator_net.load_state_dict(new_genparams)
		return generator_net.to(gpu)

	@staticmethod
	def _get_batches(size: int, bsize: int):
		"""train.py:401-410, the unused shuffle included: its draw is part of the NumPy stream"""
		nbatches = int(np.ceil(size / bsize))
		idcs = np.arange(size)
		np.random.shuffle(idcs)
		batches = [slice(batch * bsize, (batch + 1) * bsize) for batch in range(nbatches)]
		batches[-1] = slice(batches[-1].start, size)
		return batches
