"""
Autodidactic-Iteration data generation on the device (reference: `Train.ADI_traindata`, librubiks/train.py:256-339).

The reference scrambles on the host, builds 12 x (games*depth) action tuples, fans out with NumPy and one-hot encodes
2.7 M children on the host before the net sees them.  Here the random walks, the 12-child fan-out with its fused goal
test and the one-hot encoding are HIP kernels on device-resident buffers; only the RNG draws (NumPy legacy generator,
the reference's order, so seeds reproduce the same scrambles) and the final small target tensors touch the host.

    oh_states, policy_targets, value_targets, loss_weights = adi_traindata(net, games, depth, alpha, reward_method)

Same return values as the reference (one-hot states on `gpu`, the three target tensors on the CPU).
"""
from __future__ import annotations

import numpy as np
import torch

from librubiks_amd import gpu, no_grad, _ffi, cube


@no_grad
def adi_traindata(net, rollout_games: int, rollout_depth: int, alpha: float, reward_method: str = "lapanfix",
                  ff_batches: int = 1, fused_first_layer=False, ball=None, return_states: bool = False):
	"""
	`return_states`: the first value is the (games * depth, 20) int8 device tensor of the scrambled states themselves instead of their
	one-hot rows (for `oh_linear.train_on_states`; 20-byte representation only).  Same draws, same other three values.
	`ball`: a `DeviceSymBall(R)` (built at first use), or None for the reference's targets.  With a ball, a child whose orbit the ball
	holds at depth c gets, as its value BEFORE the reward is added, the exact V*(0) = 0, V*(c) = g - (c - 1) for 1 <= c <= R, where g
	is the method's goal reward (0 for reward0, else 1): the fixed point of V(s) = max_a [r(s.a) + V(s.a)] with V(solved) = 0.
	lapanfix pins that value itself; for paper, schultzfix and reward0 it is the convention this option adopts.  The net runs only on
	the children outside the ball, compacted on the device in ascending row order and cut into ceil(count / ff_batches) rows a call;
	with no child outside it is not called at all.  Everything behind the children's values -- the rewards, the first maximum over
	twelve siblings, the lapanfix / schultzfix overrides, the loss weights -- is unchanged, so every state within R - 1 moves of
	solved gets its exact value target and the lowest optimal move as its policy target.  Works in both representations.
	"""
	assert reward_method in ("paper", "lapanfix", "schultzfix", "reward0")
	if ball is not None:
		from librubiks_amd.solving.agents import DeviceSymBall
		if not isinstance(ball, DeviceSymBall):
			raise TypeError(f"ball must be a DeviceSymBall or None, not {type(ball).__name__}")
	_ffi.require_gpu()
	is2024 = cube.get_is2024()             # 6x8x6: the same walks in 20-byte form, the net's rows from the fused converter + encoder
	if fused_first_layer and not is2024:
		raise ValueError("fused_first_layer reads 20-byte states into a Linear(480, H); a 6x8x6 net has 288 inputs")
	if return_states and not is2024:
		raise ValueError("return_states hands out 20-byte states for a Linear(480, H); a 6x8x6 net has 288 inputs")
	net.eval()
	with_solved = reward_method == "lapanfix"
	# scrambling: draws as cube.sequence_scrambler (cube.py:226-227), walks on the device           train.py:277
	faces = np.random.randint(0, 6, (rollout_depth, rollout_games))
	dirs = np.random.randint(0, 2, (rollout_depth, rollout_games))
	acts = torch.from_numpy((2 * faces + (1 - dirs)).astype(np.uint8)).to(gpu)
	# walks, goal test of the scrambled states, fan-out and its goal test: ONE launch              train.py:277, :281, :285, :292
	states, solved_scrambled, substates, solved_sub = cube.device.rollout_fanout(acts, with_solved)  # (games*depth, 20), ..., (12*games*depth, 20), ...
	n = len(states)
	oh_states = states if return_states else cube.device.as_oh(states) if is2024 else cube.device.to686(states, torch.float32)
	solved_scrambled, solved_sub = solved_scrambled.bool(), solved_sub.bool()
	rewards = torch.where(solved_sub, torch.tensor(0.0 if reward_method == "reward0" else 1.0, device=gpu),
	                      torch.tensor(-1.0, device=gpu))                                         # train.py:294-296
	# value of every child, in slices so that the one-hot batch stays bounded                      train.py:301-303
	values = torch.empty(12 * n, dtype=torch.float32, device=gpu)
	if ball is None:
		net_states, rows = substates, None
	else:
		# exact values where the ball holds the child's orbit; the net's batch is the rest, compacted in row order
		_, _, rows, net_states = cube.device.ball_child_values(ball, substates, 0.0 if reward_method == "reward0" else 1.0, values)
		rows = rows.long()
	m = len(net_states)

	def put(lo, hi, v):
		if rows is None:
			values[lo:hi] = v
		else:
			values[rows[lo:hi]] = v
	step = max(1, -(-m // max(1, ff_batches)))
	if fused_first_layer:
		# the net's first Linear reads the 2.7 M children's 20-byte states directly: the (12 n, 480) one-hot never exists
		from librubiks_amd.oh_linear import fused_net
		from_states = fused_net(net, fused_first_layer)
		for lo in range(0, m, step):
			hi = min(lo + step, m)
			put(lo, hi, from_states(net_states[lo:hi], policy=False, value=True).reshape(-1).float())
	else:
		from librubiks_amd.solving.agents import _oh_dtype
		oh_dtype = _oh_dtype(net)                  # a bf16 net gets bf16 rows straight from the kernel (0 / 1 are exact)
		buf = torch.empty((min(step, m), 480 if is2024 else 288), dtype=oh_dtype, device=gpu)
		for lo in range(0, m, step):
			hi = min(lo + step, m)
			if is2024:
				cube.device.as_oh(net_states[lo:hi], buf[:hi - lo], oh_dtype)
			else:
				cube.device.to686(net_states[lo:hi], oh_dtype, buf[:hi - lo])
			put(lo, hi, net(buf[:hi - lo], policy=False, value=True).reshape(-1).float())
	values = (values + rewards).reshape(-1, 12)                                                   # train.py:313-314
	policy_targets = torch.argmax(values, dim=1)
	value_targets = values[torch.arange(n, device=gpu), policy_targets]
	if reward_method == "lapanfix":
		value_targets[solved_scrambled] = 0                                                       # train.py:319
	elif reward_method == "schultzfix":
		value_targets[torch.arange(0, n, rollout_depth, device=gpu)] = 0                          # train.py:322-324
	weighted = np.tile(1 / np.arange(1, rollout_depth + 1), rollout_games)                        # train.py:329-332
	unweighted = np.ones_like(weighted)
	ws, us = weighted.sum(), len(unweighted)
	loss_weights = ((1 - alpha) * weighted / ws + alpha * unweighted / us) * (ws + us)
	return oh_states, policy_targets.cpu(), value_targets.cpu(), torch.from_numpy(loss_weights).float()


def ball_traindata(ball, n: int, depths=None, rng=None, reward_method: str = "lapanfix", return_states: bool = False):
	"""
	Supervised ADI data from a `DeviceSymBall(R)` alone, no net involved: n states drawn by `ball.sample(n, depths, rng)` -- uniform
	at the given depth(s), or uniform over the whole ball for None; the draws are `sample`'s, so a seeded numpy.random.Generator
	reproduces the rows -- each with its exact targets from `cube.device.ball_child_depths`.  The same four values as `adi_traindata`:
	the one-hot states on `gpu` (float32, 480 or 288 wide by the representation), then on the CPU
	  value_targets   float32: V*(0) = 0, V*(d) = g - (d - 1) for d >= 1, g = 0 for reward0 and else 1 (`adi_traindata(ball=)`'s convention)
	  policy_targets  int64: the lowest action whose child lies one level nearer (`solve`'s rule, and `argmax`'s on ties); 0 at d = 0
	  loss_weights    float32: all 1
	A row costs one `state_at` sample and thirteen ball probes.  `return_states`: the (n, 20) int8 device tensor of the states instead of
	their one-hot rows, as in `adi_traindata` (20-byte representation only).
	"""
	assert reward_method in ("paper", "lapanfix", "schultzfix", "reward0")
	from librubiks_amd.solving.agents import DeviceSymBall
	if not isinstance(ball, DeviceSymBall):
		raise TypeError(f"ball must be a DeviceSymBall, not {type(ball).__name__}")
	_ffi.require_gpu()
	is2024 = cube.get_is2024()
	if return_states and not is2024:
		raise ValueError("return_states hands out 20-byte states for a Linear(480, H); a 6x8x6 net has 288 inputs")
	cube.set_is2024(True)                  # the sample as 20-byte rows, whatever the caller's representation
	try:
		states, _ = ball.sample(n, depths, rng)
	finally:
		cube.set_is2024(is2024)
	states = torch.from_numpy(states).to(gpu)
	oh_states = states if return_states else cube.device.as_oh(states) if is2024 else cube.device.to686(states, torch.float32)
	own, children = cube.device.ball_child_depths(ball, states)
	own, children = own.long(), children.long()
	nearer = children == (own - 1).unsqueeze(1)
	if bool(((own > 0) & ~nearer.any(dim=1)).any()) or bool((own < 0).any()):
		raise _ffi.RubiksHipError("rk_symball_child_depths: a sampled state has no child one level nearer")
	policy_targets = torch.argmax(nearer.float(), dim=1)                     # the first of the maxima: the lowest such action
	g = 0.0 if reward_method == "reward0" else 1.0
	value_targets = torch.where(own == 0, torch.zeros((), device=gpu), g - (own - 1).float())
	return oh_states, policy_targets.cpu(), value_targets.cpu(), torch.ones(len(states), dtype=torch.float32)
