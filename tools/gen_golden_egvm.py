"""
Fixtures of the epsilon-greedy value search -- TEST INFRASTRUCTURE, run on a CPU machine that has the unmodified reference checked out
(REFERENCE=path; default: a `reference` directory beside the repository).  No test imports this file; the tests read only what it writes.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_egvm.py

It drives the reference's `EGVM.search` (agents.py:649-726) in the 20-byte representation with the exact stub nets of
oracle/search_oracle.py (StubNet, NoisyStubNet, PolicyStubNet: small integers, 0 and -inf, the same on any hardware) under a state
budget alone, and writes data only to tests/golden/egvm_trace.npz.  Per case:

  {tag}_params         [seed, scramble depth, max_states, workers, depth, net (0 plain, 1 noisy, 2 policy), seed of the noisy net]
  {tag}_epsilon        epsilon
  {tag}_start          the start state (scrambled with RandomState(seed), apart from the global generator)
  {tag}_solved         what search returned
  {tag}_len            len(agent)
  {tag}_action_queue   the action queue
  {tag}_rng_after      np.random.randint(0, 2**31 - 1) drawn right after the search: pins every draw the search made
  {tag}_rounds         how often the reference called expand
  {tag}_solved_at      (walker, moves) of the solve, (-1, -1) without one

The global generator is seeded with `seed` right before the search.  main() asserts that the cases cover: a solve inside a walk after
at least two moves by a walker other than 0; a solve after at least two full rounds; a search that the budget stops unsolved after at
least three rounds; epsilon 0 and 1; a single worker.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden", "egvm_trace.npz")

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore", category=DeprecationWarning)

from librubiks import cube  # noqa: E402
from librubiks.solving import agents  # noqa: E402
from oracle.search_oracle import StubNet, NoisyStubNet, PolicyStubNet  # noqa: E402

PLAIN, NOISY, POLICY = 0, 1, 2

#: tag -> (seed, scramble depth, max_states, epsilon, workers, depth, net, seed of the noisy net)
CASES = {
	"walk_solve": (21, 4, 6_000, 0.5, 24, 6, PLAIN, 0),
	"first_move_solve": (14, 4, 6_000, 0.5, 24, 6, PLAIN, 0),
	"second_round_solve": (22, 5, 20_000, 0.4, 32, 8, PLAIN, 0),
	"late_solve": (24, 6, 20_000, 0.4, 32, 8, PLAIN, 0),
	"noisy_budget": (5, 12, 2_000, 0.3, 20, 8, NOISY, 2),
	"policy_budget": (6, 10, 1_500, 0.375, 10, 25, POLICY, 0),
	"eps0": (7, 8, 700, 0.0, 8, 10, POLICY, 0),
	"eps1": (9, 4, 3_000, 1.0, 16, 6, PLAIN, 0),
	"one_worker": (10, 5, 260, 0.6, 1, 50, NOISY, 1),
	"wire": (12, 7, 5_000, 0.375, 10, 50, NOISY, 3),
}


def make_net(kind: int, seed: int):
	return PolicyStubNet() if kind == POLICY else NoisyStubNet(seed) if kind == NOISY else StubNet()


def scramble(seed: int, depth: int) -> np.ndarray:
	rng = np.random.RandomState(seed)
	state = cube.get_solved()
	for a in rng.randint(0, 12, depth):
		state = cube.rotate(state, *cube.action_space[a])
	return state


def run(seed, sdepth, max_states, epsilon, workers, depth, kind, nseed):
	cube.set_is2024(True)
	start = scramble(seed, sdepth)
	agent = agents.EGVM(make_net(kind, nseed), epsilon=epsilon, workers=workers, depth=depth)
	calls = []
	inner = agent.expand
	agent.expand = lambda s: (lambda r: (calls.append(tuple(int(x) for x in r[3])), r)[1])(inner(s))
	np.random.seed(seed)
	solved = bool(agent.search(start, time_limit=None, max_states=max_states))
	after = int(np.random.randint(0, 2 ** 31 - 1))
	return start, agent, solved, after, calls


def main():
	torch.set_num_threads(4)
	out, seen = {}, set()
	for tag, c in CASES.items():
		seed, sdepth, max_states, epsilon, workers, depth, kind, nseed = c
		start, agent, solved, after, calls = run(*c)
		at = calls[-1] if solved else (-1, -1)
		out[f"{tag}_params"] = np.array([seed, sdepth, max_states, workers, depth, kind, nseed], np.int64)
		out[f"{tag}_epsilon"] = np.array(float(epsilon))
		out[f"{tag}_start"] = np.asarray(start, np.int8)
		out[f"{tag}_solved"] = np.array(solved)
		out[f"{tag}_len"] = np.array(len(agent), np.int64)
		out[f"{tag}_action_queue"] = np.array([int(a) for a in agent.action_queue], np.int64)
		out[f"{tag}_rng_after"] = np.array(after, np.int64)
		out[f"{tag}_rounds"] = np.array(len(calls), np.int64)
		out[f"{tag}_solved_at"] = np.array(at, np.int64)
		if solved and at[1] >= 2 and at[0] != 0:
			seen.add("a solve inside a walk after two moves or more by a walker other than 0")
		if solved and len(calls) >= 3:
			seen.add("a solve after two full rounds or more")
		if not solved and len(calls) >= 3 and len(agent) + workers * depth > max_states:
			seen.add("unsolved after three rounds or more, stopped by the budget")
		seen.update({0.0: {"epsilon 0"}, 1.0: {"epsilon 1"}}.get(float(epsilon), set()))
		if workers == 1:
			seen.add("one worker")
		print(tag, "solved" if solved else "unsolved", "len", len(agent), "rounds", len(calls), "at", at, "queue", len(agent.action_queue), flush=True)
	want = {"a solve inside a walk after two moves or more by a walker other than 0", "a solve after two full rounds or more",
	        "unsolved after three rounds or more, stopped by the budget", "epsilon 0", "epsilon 1", "one worker"}
	assert seen == want, want - seen
	np.savez_compressed(OUT, **out)
	print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
	main()
