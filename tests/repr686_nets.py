"""
Stub nets for the 6x8x6 representation (288 one-hot inputs, element 48 f + 6 p + c = colour c at ring position p of face f), exact
on any hardware: every output is a small integer (or 0 / -inf) computed in float32 from 0 / 1 inputs, whatever dtype the one-hot
arrives in.  Shared by the fixture generator (tools/gen_golden_repr686.py, which drives the unmodified reference with them) and the
tests, so both sides evaluate the same functions.

  StubNet686        value = -(48 - stickers on their solved colour), zero policy logits
  NoisyStubNet686   + ((x . w) mod 7) - 3 with w = RandomState(seed).randint(0, 50, 288)
  PolicyStubNet686  the plain value and logits of 0 / -inf: 8 finite ones when the key (colours of slots 0 and 1) is even, 4 when
                    odd, so a softmax is exactly 0, 1/8 or 1/4

`dtype` gives the module one parameter of that dtype: the agents then hand it its one-hot in that dtype.
"""
import numpy as np
import torch

SOLVED_OH686 = (np.arange(288) % 6 == np.arange(288) // 48).astype(np.float32)


def policy_table686() -> np.ndarray:
	t = np.zeros((36, 12), np.float32)
	for k in range(36):
		banned = [(k + 3 * j) % 12 for j in range(4)] if k % 2 == 0 else [(k + j) % 12 for j in range(8)]
		t[k, banned] = -np.inf
	return t


class StubNet686(torch.nn.Module):
	def __init__(self, dtype: torch.dtype = torch.float32):
		super().__init__()
		self.marker = torch.nn.Parameter(torch.zeros(1, dtype=dtype), requires_grad=False)
		self._const = {}

	def _c(self, name: str, arr: np.ndarray, device):
		key = (name, str(device))
		if key not in self._const:
			self._const[key] = torch.from_numpy(arr).to(device)
		return self._const[key]

	def _value(self, x: torch.Tensor) -> torch.Tensor:
		x = x.float()
		return -(48 - (x * self._c("solved", SOLVED_OH686, x.device)).sum(dim=1, keepdim=True))

	def _logits(self, x: torch.Tensor) -> torch.Tensor:
		return torch.zeros(len(x), 12, device=x.device)

	def forward(self, x, policy=True, value=True):
		out = ([self._logits(x)] if policy else []) + ([self._value(x)] if value else [])
		return out if len(out) > 1 else out[0]


class NoisyStubNet686(StubNet686):
	def __init__(self, seed: int = 0, dtype: torch.dtype = torch.float32):
		super().__init__(dtype)
		self.w = np.random.RandomState(seed).randint(0, 50, 288).astype(np.float32)

	def _value(self, x):
		noise = torch.remainder((x.float() * self._c("w", self.w, x.device)).sum(dim=1, keepdim=True), 7.0) - 3.0
		return super()._value(x) + noise


class PolicyStubNet686(StubNet686):
	def _logits(self, x):
		x = x.float()
		key = x[:, 0:6].argmax(dim=1) + 6 * x[:, 6:12].argmax(dim=1)
		return self._c("table", policy_table686(), x.device)[key]
