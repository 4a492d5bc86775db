"""A small float32 net of the reference's structure (model.py:117-161) for the training tests: shared 480 -> 64 -> 64, heads 64 -> 64 -> 12 / 1,
ELU + BatchNorm1d behind every Linear but a head's last, Xavier-uniform weights."""
import torch
import torch.nn as nn


def _stack(sizes, final):
	layers = []
	for i in range(len(sizes) - 1):
		lin = nn.Linear(sizes[i], sizes[i + 1])
		nn.init.xavier_uniform_(lin.weight)
		layers.append(lin)
		if not (final and i == len(sizes) - 2):
			layers += [nn.ELU(), nn.BatchNorm1d(sizes[i + 1])]
	return nn.Sequential(*layers)


class SmallNet(nn.Module):
	def __init__(self, seed: int = 0):
		super().__init__()
		torch.manual_seed(seed)
		self.shared_net = _stack([480, 64, 64], False)
		self.policy_net = _stack([64, 64, 12], True)
		self.value_net = _stack([64, 64, 1], True)

	def forward(self, x, policy=True, value=True):
		assert policy or value
		x = self.shared_net(x)
		out = ([self.policy_net(x)] if policy else []) + ([self.value_net(x)] if value else [])
		return out if len(out) > 1 else out[0]
