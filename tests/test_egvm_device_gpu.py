"""
DeviceEGVM (engine rk_egvm_*) against the reference's EGVM (ref:librubiks/solving/agents.py:649-726): for every case of
tests/golden/egvm_trace.npz (tools/gen_golden_egvm.py, 20-byte representation) and the `egvm` / `egvm_policy` cases of
tests/golden/repr686_search.npz (tools/gen_golden_repr686.py, 6x8x6) the return value, len(agent), the action queue and the next
draw of the global NumPy generator equal the unmodified reference's, whatever the number of rounds between two polls.  The stub nets
give small integers, 0 and -inf, so nothing depends on float rounding.
"""
import os

import numpy as np
import pytest
import torch

from librubiks_amd import cube
from librubiks_amd.solving.agents import DeviceEGVM, EGVM
from oracle import cube_oracle as orc
from oracle.search_oracle import StubNet, NoisyStubNet, PolicyStubNet
from tests.repr686_nets import NoisyStubNet686, PolicyStubNet686

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["walk_solve", "first_move_solve", "second_round_solve", "late_solve", "noisy_budget", "policy_budget", "eps0", "eps1",
         "one_worker", "wire"]
CASES686 = {"egvm": (lambda: NoisyStubNet686(2), 0.3, 20, 8), "egvm_policy": (lambda: PolicyStubNet686(), 0.5, 16, 6)}


def _load(name):
	with np.load(os.path.join(GOLDEN, name)) as z:
		return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def trace():
	return _load("egvm_trace.npz")


@pytest.fixture(scope="module")
def trace686():
	return _load("repr686_search.npz")


def _case(t, tag):
	seed, _, max_states, workers, depth, kind, nseed = (int(x) for x in t[f"{tag}_params"])
	net = PolicyStubNet() if kind == 2 else NoisyStubNet(nseed) if kind == 1 else StubNet()
	return seed, max_states, net, float(t[f"{tag}_epsilon"]), workers, depth


def _check(t, tag, agent, solved):
	"""Prints every figure, then compares it with the reference's."""
	got = (bool(solved), len(agent), [int(a) for a in agent.action_queue], int(np.random.randint(0, 2 ** 31 - 1)))
	want = (bool(t[f"{tag}_solved"]), int(t[f"{tag}_len"]), t[f"{tag}_action_queue"].tolist(), int(t[f"{tag}_rng_after"]))
	print(tag, type(agent).__name__, "got", got, "want", want)
	assert got[0] == want[0] and got[1] == want[1], tag
	assert got[2] == want[2], tag
	assert got[3] == want[3], tag


def test_fixture_covers_every_way_a_search_ends(trace):
	t = trace
	at = {tag: tuple(int(x) for x in t[f"{tag}_solved_at"]) for tag in CASES}
	assert any(bool(t[f"{g}_solved"]) and at[g][1] >= 2 and at[g][0] != 0 for g in CASES)
	assert any(bool(t[f"{g}_solved"]) and int(t[f"{g}_rounds"]) >= 3 for g in CASES)
	assert any(not bool(t[f"{g}_solved"]) and int(t[f"{g}_rounds"]) >= 3 for g in CASES)
	assert {0.0, 1.0} <= {float(t[f"{g}_epsilon"]) for g in CASES} and any(int(t[f"{g}_params"][3]) == 1 for g in CASES)
	assert {k[:-len("_params")] for k in t if k.endswith("_params")} == set(CASES)


@pytest.mark.parametrize("poll", [1, 4, 1000])
@pytest.mark.parametrize("tag", CASES)
def test_equals_reference(trace, tag, poll):
	t = trace
	seed, max_states, net, eps, workers, depth = _case(t, tag)
	assert poll != 1000 or poll > int(t[f"{tag}_rounds"])
	agent = DeviceEGVM(net, eps, workers, depth, poll=poll)
	np.random.seed(seed)
	solved = agent.search(t[f"{tag}_start"], time_limit=None, max_states=max_states)
	_check(t, tag, agent, solved)
	assert agent.rounds == int(t[f"{tag}_rounds"])


@pytest.mark.parametrize("tag", CASES)
def test_host_agent_gives_the_same(trace, tag):
	"""The same seeds through the host class (existing code, itself pinned to the reference)."""
	t = trace
	seed, max_states, net, eps, workers, depth = _case(t, tag)
	agent = EGVM(net, eps, workers, depth)
	np.random.seed(seed)
	solved = agent.search(t[f"{tag}_start"], time_limit=None, max_states=max_states)
	_check(t, tag, agent, solved)


@pytest.mark.parametrize("poll", [1, 1000])
@pytest.mark.parametrize("tag", sorted(CASES686))
def test_equals_reference_686(trace686, tag, poll):
	t = trace686
	make, eps, workers, depth = CASES686[tag]
	seed, sdepth, max_states = (int(x) for x in t[f"{tag}_params"])
	cube.set_is2024(False)
	np.random.seed(seed)
	state, _, _ = cube.scramble(sdepth, True)
	assert (state == t[f"{tag}_start"]).all()
	agent = DeviceEGVM(make(), eps, workers, depth, poll=poll)
	solved = agent.search(state, time_limit=None, max_states=max_states)
	_check(t, tag, agent, solved)


def test_low_precision_stub_686(trace686):
	"""A bfloat16 6x8x6 net gets its one-hot in bfloat16 from the 20-byte rows (0 / 1 are exact): the same search."""
	t, tag = trace686, "egvm"
	seed, sdepth, max_states = (int(x) for x in t[f"{tag}_params"])
	cube.set_is2024(False)
	np.random.seed(seed)
	state, _, _ = cube.scramble(sdepth, True)
	agent = DeviceEGVM(NoisyStubNet686(2, torch.bfloat16), 0.3, 20, 8)
	solved = agent.search(state, time_limit=None, max_states=max_states)
	_check(t, tag, agent, solved)


class TinyNet(torch.nn.Module):
	"""Random-init float net with the reference's call signature (model.py:131-141)."""
	def __init__(self):
		super().__init__()
		torch.manual_seed(0)
		self.body = torch.nn.Sequential(torch.nn.Linear(480, 256), torch.nn.ELU(), torch.nn.Linear(256, 64), torch.nn.ELU())
		self.p, self.v = torch.nn.Linear(64, 12), torch.nn.Linear(64, 1)

	def forward(self, x, policy=True, value=True):
		h = self.body(x)
		out = ([self.p(h)] if policy else []) + ([self.v(h)] if value else [])
		return out if len(out) > 1 else out[0]


def _replay(start, queue):
	s = start
	for a in queue:
		s = orc.rotate(s, int(a) // 2, 1 - int(a) % 2)
	return bool(orc.is_solved(s))


def _starts():
	out = []
	for seed, depth in ((2, 1), (3, 2), (5, 4), (6, 12)):
		rng = np.random.RandomState(seed)
		s = orc.SOLVED.copy()
		for a in rng.randint(0, 12, depth):
			s = orc.rotate(s, int(a) // 2, 1 - int(a) % 2)
		if not orc.is_solved(s):
			out.append(np.ascontiguousarray(s, dtype=np.int8))
	return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fused", [False, True, "epilogue", "folded"])
def test_real_net_queue_solves_exactly_when_search_says_so(dtype, fused):
	"""A float net (TinyNet; fc_small where the first layer is fused, which needs the reference's structure): the action queue
	applied to the start is solved exactly when search returned True, and len(agent) counts whole walks."""
	if fused:
		from benchmarks.nets import FcSmall
		net = FcSmall(seed=2).cuda().eval().to(dtype)
	else:
		net = TinyNet().cuda().eval().to(dtype)
	agent = DeviceEGVM(net, 0.5, 24, 6, poll=3, fused_first_layer=fused)
	some_solved = False
	for i, start in enumerate(_starts()):
		np.random.seed(100 + i)
		solved = agent.search(start, time_limit=None, max_states=24 * 6 * 12)
		print(dtype, fused, i, solved, len(agent), list(agent.action_queue))
		assert _replay(start, agent.action_queue) == solved
		some_solved |= solved
		if solved:
			assert 0 < len(agent) <= 24 * 6 * 12 and len(agent) % 24 == 0
		else:
			assert len(agent) == 24 * 6 * 12 and agent.rounds == 12
	# one move from the goal, 24 walkers at epsilon 0.5: a round's first move solves with probability 1 - (23/24)^24 = 0.64
	assert some_solved
	assert agent.captures == 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_engine_argmax_is_first_maximum_with_nan_as_maximum(dtype):
	"""The engine alone on hand-made net outputs: ties, -inf, +-0 and NaN in the logits (ndarray.argmax, ref:agents.py:701) and in
	the values (torch.argmax on the CPU, ref:agents.py:674), float32 and bfloat16."""
	import ctypes as C
	from librubiks_amd import _ffi
	from librubiks_amd.solving import _engine as eng
	lib, W, D = _ffi.lib(), 70, 3
	nan, inf = float("nan"), float("inf")
	rng = np.random.RandomState(5)
	logits = rng.randint(-3, 4, (W, 12)).astype(np.float32)              # small integers: many ties, exact in bfloat16
	logits[3, 4] = logits[3, 9] = nan
	logits[4] = -inf
	logits[5, 11] = inf
	logits[6] = nan
	logits[7] = 0.0
	logits[7, 5] = -0.0
	logits[8, :] = -inf
	logits[8, 7] = -5.0
	want_a = logits.argmax(axis=1)
	assert want_a[3] == 4 and want_a[4] == 0 and want_a[5] == 11 and want_a[6] == 0 and want_a[7] == 0 and want_a[8] == 7
	root = _starts()[-1]
	h = C.c_void_p()
	_ffi.check(lib.rk_egvm_create(C.byref(h), W, D, 2))
	try:
		ptr, rows = C.c_void_p(), C.c_size_t()
		_ffi.check(lib.rk_egvm_net_in(h, 1, _ffi.OH_STATES, C.byref(ptr), C.byref(rows)))
		assert rows.value == W * D
		visited = eng.engine_batch(ptr.value, rows.value, _ffi.OH_STATES)
		d_logits = torch.from_numpy(logits).cuda().to(dtype)
		code = _ffi.OH_BF16 if dtype == torch.bfloat16 else _ffi.OH_F32
		draws = np.full((2, D, W), -1, np.int8)
		draws[:, :, 0] = 6                                                   # walker 0 acts "at random": action 6 whatever its logits
		want_a[0] = 6
		for values in (rng.randint(-9, 3, W * D).astype(np.float32), None, None):
			if values is None:
				values = rng.randint(-9, 3, W * D).astype(np.float32)
				values[[37, 101]] = nan if rng.randint(2) else values.max() + 1      # two NaNs, or a tie at the top
			best = int(torch.from_numpy(values).to(dtype).float().argmax())
			assert values[best] != values[best] or (values[best] == values.max() and best == int(np.flatnonzero(values == values.max())[0]))
			_ffi.check(lib.rk_egvm_reset(h, root.ctypes.data, 2 * W * D, _ffi.stream_ptr()))
			_ffi.check(lib.rk_egvm_set_draws(h, draws.ctypes.data, 2, _ffi.stream_ptr()))
			for _ in range(D + 2):                                               # steps beyond the walk change nothing
				_ffi.check(lib.rk_egvm_step(h, d_logits.data_ptr(), code, _ffi.stream_ptr()))
			d_values = torch.from_numpy(values).cuda().to(dtype)
			_ffi.check(lib.rk_egvm_round_end(h, d_values.data_ptr(), code, _ffi.stream_ptr()))
			status = (C.c_longlong * 8)()
			_ffi.check(lib.rk_egvm_status(h, status, _ffi.stream_ptr()))
			assert list(status)[:7] == [0, 0, 1, W * D, -1, -1, 0]
			got = visited.cpu().numpy().reshape(W, D, 20)
			for w in range(W):
				s = root
				for d in range(D):
					s = orc.rotate(s, int(want_a[w]) // 2, 1 - int(want_a[w]) % 2)
					assert (got[w, d] == s).all(), (w, d)
			rec = np.zeros((1, D + 2), np.int64)
			_ffi.check(lib.rk_egvm_records(h, 0, 1, rec.ctypes.data, _ffi.stream_ptr()))
			assert rec[0, 0] == best % D + 1 and rec[0, 1] == 0 and (rec[0, 2:2 + best % D + 1] == want_a[best // D]).all()
			assert lib.rk_egvm_records(h, 0, 2, rec.ctypes.data, _ffi.stream_ptr()) == -1        # round 1 is not closed
	finally:
		lib.rk_egvm_destroy(h)


def test_solved_root_and_budget_below_one_round():
	agent = DeviceEGVM(StubNet(), 0.3, 10, 5)
	np.random.seed(1)
	before = np.random.get_state()[1].copy()
	assert agent.search(orc.SOLVED.copy(), time_limit=None, max_states=1000) is True
	assert len(agent.action_queue) == 0 and len(agent) == 0
	start = _starts()[-1]
	assert agent.search(start, time_limit=None, max_states=49) is False           # not one round fits: the reference draws nothing
	assert len(agent.action_queue) == 0 and len(agent) == 0
	assert (np.random.get_state()[1] == before).all()
	cube.set_is2024(False)
	assert agent.search(cube.get_solved(), time_limit=None, max_states=1000) is True and len(agent.action_queue) == 0


def test_second_search_reuses_the_graphs(trace):
	t, tag = trace, "late_solve"
	seed, max_states, net, eps, workers, depth = _case(t, tag)
	agent = DeviceEGVM(net, eps, workers, depth, poll=2)
	for _ in range(3):
		np.random.seed(seed)
		solved = agent.search(t[f"{tag}_start"], time_limit=None, max_states=max_states)
		_check(t, tag, agent, solved)
		assert agent.captures == 2
	other = "noisy_budget"                                                          # another search on the same engine and net
	np.random.seed(int(t[f"{other}_params"][0]))
	agent.search(t[f"{other}_start"], time_limit=None, max_states=500)
	assert agent.captures == 2 and len(agent) == 256 and agent.rounds == 1
	agent.net = NoisyStubNet(5)                                                     # another net: captured again
	np.random.seed(seed)
	agent.search(t[f"{tag}_start"], time_limit=None, max_states=max_states)
	assert agent.captures == 4


def test_tiny_time_limit_returns_false_cleanly(trace):
	t, tag = trace, "wire"
	seed, max_states, net, eps, workers, depth = _case(t, tag)
	agent = DeviceEGVM(net, eps, workers, depth)
	np.random.seed(seed)
	assert agent.search(t[f"{tag}_start"], time_limit=1e-9, max_states=None) is False
	assert len(agent) % (workers * depth) == 0 and len(agent.action_queue) <= len(agent)
	np.random.seed(seed)                                                            # and the agent is as good as new afterwards
	solved = agent.search(t[f"{tag}_start"], time_limit=None, max_states=max_states)
	_check(t, tag, agent, solved)


def test_plays_in_the_sequential_evaluator():
	from librubiks_amd.solving.evaluation import Evaluator
	ev = Evaluator(3, [3], max_states=2_000)
	np.random.seed(21)
	res_d, _, _ = ev.eval(DeviceEGVM(StubNet(), 0.4, 16, 6), batched=False)
	np.random.seed(21)
	res_h, _, _ = ev.eval(EGVM(StubNet(), 0.4, 16, 6), batched=False)
	assert (np.asarray(res_d) == np.asarray(res_h)).all()
