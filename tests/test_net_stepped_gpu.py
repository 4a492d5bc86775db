"""
The form switch of the net-stepped agents (DeviceEGVM, GreedyBatch, DeviceBeamSearch; `_NetStepped` in solving/agents.py, `NetBatches`
in csrc/rk_search_host.h): ONE agent searches with a float32 net, then with a bfloat16 net -- the RK_OH_* code of the batch
changes, so the agent has to fetch the engine's other batch and capture its steps again on it --, then with the float32 net again.
Every search gives what a fresh agent built with that net gives, and `captures` rises by one per kept graph at each switch.
All nets are exact (small integers, or table look-ups), so nothing depends on float rounding.
"""
import numpy as np
import pytest
import torch

from librubiks_amd import _ffi
from librubiks_amd.solving.agents import DeviceBeamSearch, DeviceEGVM, GreedyBatch
from oracle import cube_oracle as orc
from oracle.search_oracle import NoisyStubNet
from tests import beam_model as bm
from tests.adi_nets import Recorded
from tests.test_greedy_batch_gpu import Bf16Out

pytestmark = pytest.mark.gpu


def _bf16(net):
	"""`net` as a bfloat16 net: it asks for bfloat16 one-hot rows (RK_OH_BF16) and answers in bfloat16."""
	return Recorded(net if getattr(net, "dtype", None) == "bfloat16" else Bf16Out(net), rows_dtype=torch.bfloat16)


def _scramble(seed: int, depth: int) -> np.ndarray:
	rng = np.random.RandomState(seed)
	s = orc.SOLVED.copy()
	while orc.is_solved(s):
		s = orc.SOLVED.copy()
		for a in rng.randint(0, 12, depth):
			s = orc.rotate(s, int(a) // 2, 1 - int(a) % 2)
	return np.ascontiguousarray(s, np.int8)


# ---- per agent: (make(net), run(agent) -> everything a search leaves behind, the nets (float32, bfloat16), kept graphs) ----
def _run_egvm(agent):
	np.random.seed(31)
	# (NoisyStubNet(1) solves this start in its fourth round -- the draws are rewound --, NoisyStubNet(2) spends the six rounds)
	solved = agent.search(_scramble(14, 2), time_limit=None, max_states=3 * 4 * 6)
	return (bool(solved), len(agent), agent.rounds, [int(a) for a in agent.action_queue], int(np.random.randint(0, 2 ** 31 - 1)))


def _run_greedy(agent):
	starts = np.array([_scramble(40 + d, d) for d in (1, 3, 6, 25)])
	solved = agent.search(starts, time_limit=None, max_states=12)
	return (solved.tolist(), agent.status.tolist(), agent.steps.tolist(), agent.handed_back.tolist(), len(agent), agent.launched,
	        [[int(a) for a in agent.action_queue_of(g)] for g in range(4)])


def _run_beam(agent):
	out = []
	for seed, depth in ((620, 9), (562, 4)):                       # the depth limit stops the first, the second is solved at depth 4
		solved = agent.search(bm.start_of(seed, depth), None, None)
		out.append((bool(solved), agent.status, agent.depth, len(agent), agent.sizes.tolist(), agent.meeting, [int(a) for a in agent.action_queue],
		            [agent.back_of(t).tolist() for t in range(1, len(agent.sizes))]))
	return out


AGENTS = {
	"egvm": (lambda net: DeviceEGVM(net, 0.3, 3, 4, poll=2), _run_egvm, lambda: (NoisyStubNet(1), _bf16(NoisyStubNet(2))), 2),
	"greedy": (lambda net: GreedyBatch(net, "value", 4), _run_greedy, lambda: (NoisyStubNet(4), _bf16(NoisyStubNet(5))), 1),
	"beam": (lambda net: DeviceBeamSearch(net, 22, 9), _run_beam, lambda: (bm.net_of("lookup"), _bf16(bm.net_of("lookup_bf16"))), 1),
}


@pytest.mark.parametrize("name", sorted(AGENTS))
def test_form_switch_on_one_agent(name):
	make, run, nets, graphs = AGENTS[name]
	f32, bf16 = nets()
	want = {id(f32): run(make(f32)), id(bf16): run(make(bf16))}
	print(name, "float32", want[id(f32)], "bfloat16", want[id(bf16)])
	assert want[id(f32)] != want[id(bf16)]                             # the two nets lead the searches differently
	agent = make(f32)
	batches = []
	for n, (net, code) in enumerate(((f32, _ffi.OH_F32), (bf16, _ffi.OH_BF16), (f32, _ffi.OH_F32)), 1):
		agent.net = net
		got = run(agent)
		print(name, "search", n, got)
		assert got == want[id(net)], (name, n)
		assert agent.captures == graphs * n, (name, n)
		assert agent._batch[0] == code and len(agent._batch) == 1 + graphs
		assert all(t.dtype == (torch.float32 if code == _ffi.OH_F32 else torch.bfloat16) and t.shape[1] == 480 for t in agent._batch[1:])
		batches.append([t.data_ptr() for t in agent._batch[1:]])
		assert run(agent) == want[id(net)] and agent.captures == graphs * n        # the same form again: nothing is captured
	assert batches[0] == batches[2] and not set(batches[0]) & set(batches[1])      # the engine kept the batch of either form
