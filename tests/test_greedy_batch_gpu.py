"""
GreedyBatch (engine rk_greedy_*) against the one-step agents it plays in lock-step: `PolicySearch` (greedy,
ref:librubiks/solving/agents.py:138-142) and `ValueSearch` (ref:agents.py:156-166) inside THIS repository's `Agent.search` loop,
which counts a game's moves against max_states at every step (librubiks_amd/solving/agents.py, Agent.search; in the reference
len(self) stays 0 until search returns, ref:agents.py:30-38).  `restated_search` below writes both `_step` rules and that loop out in
NumPy over oracle.cube_oracle moves; the engine must equal it, and the host agents played game by game in the same process, in
`status`, `steps` and every action queue.  All nets give small integers, 0 or -inf, so nothing depends on float rounding, and no
game may be handed back -- except where a test plants a near-tie or a NaN on purpose.
"""
import os

import numpy as np
import pytest
import torch

from librubiks_amd import cube
from librubiks_amd.solving import agents
from librubiks_amd.solving.agents import GreedyBatch, PolicySearch, ValueSearch
from librubiks_amd.solving.evaluation import Evaluator
from oracle import cube_oracle as orc
from oracle.search_oracle import NoisyStubNet, PolicyStubNet, StubNet
from tests.repr686_nets import StubNet686
from tests.test_astar_gpu import TinyNet

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEPTHS = (1, 2, 3, 4, 5, 6, 25)
BUDGETS = (200, 7, 1)                    # the largest first: one engine, and so one capture, serves all three


# ---- nets -------------------------------------------------------------------------------------------------------------------
class TableNet:
	"""Policy logits that are small integers looked up from one-hot columns: T0[code of cubie 0] + T1[code of cubie 1], each entry
	in 0..4, so two logits are equal or at least 1 apart.  The value head is StubNet's.  `plant(state, row)`: for exactly that
	state the logits are `row` instead (the near-tie and NaN cases)."""
	def __init__(self, seed: int = 3):
		rng = np.random.RandomState(seed)
		self.t0 = rng.randint(0, 5, (24, 12)).astype(np.float32)
		self.t1 = rng.randint(0, 5, (24, 12)).astype(np.float32)
		self.stub = StubNet()
		self.planted = None
		self._dev = {}

	def plant(self, state: np.ndarray, row: np.ndarray):
		self.planted = (orc.as_oh(state)[0], np.asarray(row, np.float32))
		self._dev = {}
		return self

	def eval(self):
		return self

	def _consts(self, device):
		if device not in self._dev:
			arrs = [self.t0, self.t1] + (list(self.planted) if self.planted else [])
			self._dev[device] = [torch.from_numpy(a).to(device) for a in arrs]
		return self._dev[device]

	def __call__(self, x, policy=True, value=True):
		if not isinstance(x, torch.Tensor):
			x = torch.from_numpy(np.asarray(x, np.float32))
		out = []
		if policy:
			c = self._consts(x.device)
			xf = x.float()
			logits = c[0][xf[:, :24].argmax(dim=1)] + c[1][xf[:, 24:48].argmax(dim=1)]
			if self.planted:
				hit = (xf * c[2]).sum(dim=1, keepdim=True) == 20
				logits = torch.where(hit, c[3].expand_as(logits), logits)
			out.append(logits)
		if value:
			out.append(self.stub(x, policy=False, value=True))
		return out if len(out) > 1 else out[0]


class TeacherNet:
	"""Policy logit a = StubNet's value of child a.  A move is a fixed permutation of the 480 one-hot columns, so the 12
	permutations are built once, from cube.expand on the host; the logit is then a sum of at most twenty ones minus 20."""
	def __init__(self):
		self.stub = StubNet()
		codes = np.repeat(np.arange(24, dtype=np.int8)[:, None], 20, axis=1)          # row c: every cubie on code c
		kids = cube.expand(codes).reshape(24, 12, 20).astype(np.intp)                             # kids[c, a, i]: where move a takes code c of cubie i
		m = np.zeros((480, 12), np.float32)
		for a in range(12):
			for i in range(20):
				m[24 * i + np.arange(24), a] = self.stub.solved_oh[24 * i + kids[:, a, i]]
		self.m = m
		self._dev = {}

	def eval(self):
		return self

	def __call__(self, x, policy=True, value=True):
		if not isinstance(x, torch.Tensor):
			x = torch.from_numpy(np.asarray(x, np.float32))
		out = []
		if policy:
			if x.device not in self._dev:
				self._dev[x.device] = torch.from_numpy(self.m).to(x.device)
			out.append((x.float()[:, :, None] * self._dev[x.device][None]).sum(dim=1) - 20.0)
		if value:
			out.append(self.stub(x, policy=False, value=True))
		return out if len(out) > 1 else out[0]


class Bf16Out:
	"""The wrapped net's outputs as bfloat16 (small integers, 0 and -inf are exact there)."""
	def __init__(self, net):
		self.net = net

	def eval(self):
		return self

	def __call__(self, x, policy=True, value=True):
		out = self.net(x, policy=policy, value=value)
		if isinstance(out, (list, tuple)):
			return [o.to(torch.bfloat16) for o in out]
		return out.to(torch.bfloat16)


_NETS = {}


def net_of(name: str):
	if name not in _NETS:
		_NETS[name] = {"stub": StubNet, "noisy": lambda: NoisyStubNet(4), "policy_stub": PolicyStubNet, "table": TableNet,
		               "teacher": TeacherNet}[name]()
	return _NETS[name]


CASES = [("policy", "stub"), ("policy", "policy_stub"), ("policy", "table"), ("policy", "teacher"),
         ("value", "stub"), ("value", "noisy"), ("value", "policy_stub"), ("value", "teacher")]


# ---- the NumPy restatement --------------------------------------------------------------------------------------------------
def move(state, a: int):
	return orc.rotate(state, a // 2, 1 - a % 2)


def _numbers(out) -> np.ndarray:
	return (out.float().cpu().numpy() if isinstance(out, torch.Tensor) else np.asarray(out, np.float32))


def policy_step(net, state):
	"""ref:agents.py:138-142 with sample_policy false: argmax of the float32 softmax of the logits."""
	logits = _numbers(net(orc.as_oh(state), value=False)).reshape(12)
	with np.errstate(invalid="ignore"):
		e = np.exp(logits - logits.max())
		policy = e / e.sum()
	a = int(policy.argmax())
	state = move(state, a)
	return a, state, orc.is_solved(state)


def value_step(net, state):
	"""ref:agents.py:156-166."""
	children = orc.expand12(state[None])
	solutions = orc.multi_is_solved(children)
	if solutions.any():
		a = int(np.where(solutions)[0][0])
		return a, children[a], True
	v = _numbers(net(orc.as_oh(children), policy=False)).reshape(12)
	a = int(np.argmax(v))
	return a, children[a], False


def restated_search(net, mode: str, state, max_states: int, stop_at=None):
	"""This repository's Agent.search loop without the clock -> (status, action queue).  `stop_at`: a state at which a running game
	is handed back (status 3) instead of moved."""
	queue = []
	if orc.is_solved(state):
		return 1, queue
	step = policy_step if mode == "policy" else value_step
	solved = False
	while not solved and len(queue) < max_states:
		if stop_at is not None and (state == stop_at).all():
			return 3, queue
		a, state, solved = step(net, state)
		queue.append(a)
	return (1 if solved else 2), queue


def host_search(net, mode: str, state, max_states: int):
	agent = PolicySearch(net) if mode == "policy" else ValueSearch(net)
	solved = agent.search(state, time_limit=None, max_states=max_states)
	assert len(agent) == len(agent.action_queue)
	return (1 if solved else 2), [int(a) for a in agent.action_queue]


def make_starts() -> np.ndarray:
	"""Three scrambles of every depth in DEPTHS and a solved root."""
	rng = np.random.RandomState(11)
	out = []
	for depth in DEPTHS:
		for _ in range(3):
			s = orc.SOLVED.copy()
			while orc.is_solved(s):
				s = orc.SOLVED.copy()
				for a in rng.randint(0, 12, depth):
					s = move(s, int(a))
			out.append(s)
	out.insert(4, orc.SOLVED.copy())
	return np.array(out, dtype=np.int8)


STARTS = make_starts()
_WANT = {}


def wanted(mode: str, name: str, budget: int):
	"""(restated, host) results of every start, each a list of (status, queue); made once per case."""
	key = (mode, name, budget)
	if key not in _WANT:
		net = net_of(name)
		_WANT[key] = ([restated_search(net, mode, s, budget) for s in STARTS], [host_search(net, mode, s, budget) for s in STARTS])
	return _WANT[key]


def play(agent, starts, budget: int):
	"""The starts in groups of agent.games (the last group may be smaller) -> [(status, queue)], and checks the bookkeeping."""
	got = []
	for lo in range(0, len(starts), agent.games):
		group = starts[lo:lo + agent.games]
		solved = agent.search(group, time_limit=None, max_states=budget)
		assert solved.dtype == bool and solved.shape == (len(group),) and (solved == (agent.status == 1)).all()
		assert agent.status.shape == agent.steps.shape == (len(group),)
		assert len(agent) == int(agent.steps.sum()) and agent.launched <= budget
		for i in range(len(group)):
			q = agent.action_queue_of(i)
			assert len(q) == agent.steps[i]
			got.append((int(agent.status[i]), [int(a) for a in q]))
		assert len(agent.handed_back) == 0, agent.handed_back           # integer logits: gaps are 0 or >= 1
	return got


# ---- the engine against the restatement and the host agents ----------------------------------------------------------------
@pytest.mark.parametrize("games", [1, 5, 64])
@pytest.mark.parametrize("mode, name", CASES)
def test_equals_restatement_and_host_agent(mode, name, games):
	agent = GreedyBatch(net_of(name), mode, games, poll=3)
	for budget in BUDGETS:
		restated, host = wanted(mode, name, budget)
		got = play(agent, STARTS, budget)
		for i, (g, r, h) in enumerate(zip(got, restated, host)):
			print(mode, name, games, budget, i, "engine", g, "restated", r, "host", h)
		assert got == restated
		assert got == host
	assert agent.captures == 1                                      # every later search replayed the first one's graph


def test_inputs_cover_every_way_a_game_ends():
	"""Over the cases above: games solved after more than one move, games that spend the budget, a root that is already solved."""
	for mode, name in (("policy", "teacher"), ("value", "stub"), ("value", "noisy")):
		restated, _ = wanted(mode, name, 200)
		assert any(st == 1 and len(q) > 1 for st, q in restated), (mode, name)
		assert any(st == 1 and len(q) == 0 for st, q in restated)
	for mode, name in CASES:
		assert any(st == 2 and len(q) == 7 for st, q in wanted(mode, name, 7)[0]), (mode, name)
	assert any(st == 2 and len(q) == 200 for st, q in wanted("policy", "stub", 200)[0])
	assert sum(orc.is_solved(s) for s in STARTS) == 1 and len(STARTS) == 3 * len(DEPTHS) + 1


@pytest.mark.parametrize("mode, name", [("policy", "table"), ("policy", "policy_stub"), ("policy", "teacher"), ("value", "noisy"), ("value", "teacher")])
def test_bfloat16_outputs_give_the_same_games(mode, name):
	agent = GreedyBatch(Bf16Out(net_of(name)), mode, 32)
	for budget in (200, 7):
		assert play(agent, STARTS, budget) == wanted(mode, name, budget)[0]
	assert agent.captures == 1


def test_solved_roots_polls_and_time_limit():
	agent = GreedyBatch(net_of("stub"), "value", 4, poll=1000)
	solved = agent.search(np.stack([orc.SOLVED] * 3), max_states=10)
	assert solved.all() and (agent.steps == 0).all() and len(agent) == 0 and agent.launched == 0
	assert play(agent, STARTS[:4], 200) == wanted("value", "stub", 200)[0][:4]           # poll beyond the budget
	seen = []
	agent.on_poll = lambda st: seen.append(st.copy())
	agent.search(STARTS[:4], max_states=200)
	agent.on_poll = None
	assert seen and (seen[-1] == agent.status).all()
	solved = agent.search(STARTS[:4], time_limit=1e-9, max_states=200)                    # no poll fits: nothing is launched
	assert agent.launched == 0 and not solved[0] and list(agent.status) == [0, 0, 0, 0] and len(agent) == 0
	with pytest.raises(ValueError):
		agent.search(STARTS[:5], max_states=10)                                            # more games than the engine has
	assert play(agent, STARTS[:4], 7) == wanted("value", "stub", 7)[0][:4]                # and the agent is as good as new


# ---- the Evaluator ---------------------------------------------------------------------------------------------------------
def _eval_both(make_agent, batch_games: int, max_states: int = 30, games: int = 5, depths=(1, 2, 4, 6, 25), seed: int = 77):
	ev = Evaluator(games, list(depths), max_states=max_states, batch_games=batch_games)
	np.random.seed(seed)
	res_b, states_b, times_b = ev.eval(make_agent())
	assert ev.last_mode == "batched" and (times_b > 0).all()
	after_b = np.random.get_state()
	replayed = ev.replayed
	np.random.seed(seed)
	res_s, states_s, _ = ev.eval(make_agent(), batched=False)
	assert ev.last_mode == "sequential"
	after_s = np.random.get_state()
	print("batched", res_b.tolist(), states_b.tolist(), "sequential", res_s.tolist(), states_s.tolist(), "replayed", replayed)
	assert (res_b == res_s).all() and (states_b == states_s).all()
	assert after_b[0] == after_s[0] and (after_b[1] == after_s[1]).all() and after_b[2:] == after_s[2:]
	return res_b, replayed


@pytest.mark.parametrize("batch_games", [64, 7])
@pytest.mark.parametrize("mode, name", [("policy", "teacher"), ("policy", "table"), ("value", "noisy"), ("value", "stub")])
def test_evaluator_plays_in_lock_step(mode, name, batch_games):
	make = (lambda: PolicySearch(net_of(name))) if mode == "policy" else (lambda: ValueSearch(net_of(name)))
	res, replayed = _eval_both(make, batch_games)
	assert replayed == 0
	if name != "table":
		assert (res[0] == 1).all() and (res > 1).any() and (res == -1).any()


def _drawn_starts(games, depths, seed):
	np.random.seed(seed)
	return [orc.scramble(int(d), True)[0] for d in depths for _ in range(games)]


@pytest.mark.parametrize("what", ["near_tie", "nan"])
@pytest.mark.parametrize("batch_games", [64, 4])
def test_games_that_reach_a_planted_state_are_handed_back_and_replayed(what, batch_games):
	"""One logit 2^-22 below the maximum at a lower index (or a NaN) for one chosen state: the engine hands back exactly the games
	that reach it, the Evaluator plays those with the host agent, and the matrices still equal the sequential run's."""
	games, depths, seed, budget = 6, (1, 2, 3), 5, 12
	starts = _drawn_starts(games, depths, seed)
	plain = TableNet()
	# the chosen state: where the last game of depth 2 stands after one move; a game of depth 1 passes through it after two moves
	a, chosen, solved = policy_step(plain, starts[2 * games - 1])
	assert not solved
	row = np.array([0, 1, 3, 0, 2, 1, 0, 3, 1, 0, 2, 0], np.float32)
	if what == "near_tie":
		row[7] = 3.0                                                        # the maximum,
		row[2] = np.float32(3.0) - np.float32(2.0 ** -22)                   # and 2^-22 below it at a lower index
		assert 0 < row[7] - row[2] < 2.0 ** -20
	else:
		row[5] = np.nan
	net = TableNet().plant(chosen, row)
	want = [restated_search(plain, "policy", s, budget, stop_at=chosen) for s in starts]
	reached = [i for i, (st, _) in enumerate(want) if st == 3]
	assert 2 * games - 1 in reached and 2 <= len(reached) < len(starts) and len({len(want[i][1]) for i in reached}) > 1
	# the engine alone
	agent = GreedyBatch(net, "policy", len(starts))
	agent.search(np.array(starts), max_states=budget)
	print(what, "status", agent.status.tolist(), "steps", agent.steps.tolist(), "want", want)
	assert agent.handed_back.tolist() == reached
	assert [(int(st), [int(x) for x in agent.action_queue_of(i)]) for i, st in enumerate(agent.status)] == want
	# and under the Evaluator
	_, replayed = _eval_both(lambda: PolicySearch(net), batch_games, max_states=budget, games=games, depths=depths, seed=seed)
	assert replayed == len(reached)


# ---- the 6x8x6 representation ----------------------------------------------------------------------------------------------
def test_686_value_cases_equal_the_reference():
	"""`value` and `value_3` of tests/golden/repr686_search.npz: start, max_states, solved flag, len and action queue of the
	unmodified reference's ValueSearch on the 6x8x6 representation (both games are solved, so no budget rule is involved)."""
	with np.load(os.path.join(GOLDEN, "repr686_search.npz")) as z:
		t = {k: z[k] for k in z.files}
	tags = ["value", "value_3"]
	budget = int(t["value_params"][2])
	assert all(int(t[f"{g}_params"][2]) == budget for g in tags)
	cube.set_is2024(False)
	agent = GreedyBatch(StubNet686(), "value", 3)
	for played_by in (agent, GreedyBatch(StubNet686(torch.bfloat16), "value", 2)):          # (a bfloat16 net gets a bfloat16 one-hot)
		solved = played_by.search(np.stack([t[f"{g}_start"] for g in tags]), max_states=budget)
		for i, g in enumerate(tags):
			got = (bool(solved[i]), int(played_by.steps[i]), [int(a) for a in played_by.action_queue_of(i)])
			want = (bool(t[f"{g}_solved"]), int(t[f"{g}_len"]), t[f"{g}_action_queue"].tolist())
			print(g, "got", got, "want", want)
			assert got == want
		assert len(played_by.handed_back) == 0
	one = agent.search(t["value_3_start"], max_states=40)                                  # one (6, 8, 6) state is one game
	assert one.tolist() == [True] and agent.captures == 1
	bad = np.zeros_like(t["value_start"])                                                 # no cube has 48 stickers of one colour
	with pytest.raises(ValueError):
		agent.search(np.stack([t["value_start"], bad]), max_states=40)
	with pytest.raises(ValueError, match="fused_first_layer"):
		GreedyBatch(StubNet686(), "value", 2, fused_first_layer=True).search(t["value_start"], max_states=40)


# ---- real-valued nets ------------------------------------------------------------------------------------------------------
def _replay(start, queue) -> bool:
	s = start
	for a in queue:
		s = move(s, int(a))
	return orc.is_solved(s)


def _consistent(agent, starts, budget):
	solved = agent.search(starts, max_states=budget)
	for i, start in enumerate(starts):
		q = agent.action_queue_of(i)
		st = int(agent.status[i])
		print(agent, i, st, list(q))
		assert all(0 <= a < 12 for a in q) and len(q) == agent.steps[i] <= budget
		assert st in (1, 2, 3) and bool(solved[i]) == (st == 1)
		assert _replay(start, q) == (st == 1)
		if st == 1 and len(q):
			assert not _replay(start, list(q)[:-1])                       # the game stopped at the first solved state
		if st == 2:
			assert len(q) == budget
	return solved


@pytest.mark.parametrize("mode", ["policy", "value"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_real_net_queues_are_consistent(mode, dtype):
	"""No bit parity is claimed for real-valued nets (a forward on G rows need not equal one on 1 row bit for bit): the queue
	replayed from the start reaches a solved state exactly when the status says solved."""
	agent = GreedyBatch(TinyNet().cuda().eval().to(dtype), mode, len(STARTS))
	solved = _consistent(agent, STARTS, 20)
	if mode == "value":
		assert solved[:3].all() and solved[4] and agent.steps[4] == 0      # one move from the goal: the solved child is taken
	_consistent(agent, STARTS, 9)
	assert agent.captures == 1


@pytest.mark.parametrize("mode", ["policy", "value"])
@pytest.mark.parametrize("fused", [True, "epilogue", "folded"])
def test_fused_first_layer_runs_and_is_consistent(mode, fused):
	"""The fused forms read the engine's 20-byte rows.  They need the reference's net structure (shared_net / policy_net /
	value_net), which TinyNet does not have -- there the option is refused -- so fc_small stands in, as in the other engines' tests."""
	from benchmarks.nets import FcSmall
	with pytest.raises(TypeError):
		GreedyBatch(TinyNet().cuda().eval(), mode, 4, fused_first_layer=True).search(STARTS[:4], max_states=5)
	agent = GreedyBatch(FcSmall(seed=2).cuda().eval().to(torch.bfloat16), mode, len(STARTS), fused_first_layer=fused)
	_consistent(agent, STARTS, 12)
	_consistent(agent, STARTS[:6], 12)
	assert agent.captures == 1
