"""
Fixtures of the breadth-first search -- TEST INFRASTRUCTURE, run on a CPU machine that has the unmodified reference checked out
(REFERENCE=path; default: a `reference` directory beside the repository).  No test imports this file; the tests read only what it writes.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_bfs.py

It runs the reference's `BFS.search` (agents.py:92-129) with a state budget alone on seeded scrambles of depth 3-6, in the 20-byte
and in the 6x8x6 representation, and writes data only to tests/golden/bfs_trace.npz.  Per case and representation:

  {tag}_{repr}_start     the start state
  {tag}_{repr}_result    [return value, len(agent), length of the action queue]
  {tag}_{repr}_queue     the action queue
  {tag}_{repr}_sha       SHA-256 of the states dict in insertion order (digest() below)
  {tag}_{repr}_keys      the first 256 keys in insertion order, as (k, state bytes) uint8
  {tag}_params           [seed, scramble depth, max_states]

The budgets are chosen so that searches end solved, mid-level and mid-pop (a budget that is not a multiple of anything).
"""
import hashlib
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden", "bfs_trace.npz")

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
warnings.filterwarnings("ignore", category=DeprecationWarning)

from librubiks import cube  # noqa: E402
from librubiks.solving import agents  # noqa: E402

#: tag -> (seed, scramble depth, max_states)
CASES = {
	"d3_solved": (31, 3, 1_000),
	"d3_budget": (32, 3, 97),
	"d4_budget": (44, 4, 1_237),
	"d4_solved": (42, 4, 12_000),
	"d5_budget": (51, 5, 7_777),
	"d5_solved": (55, 5, 100_000),
	"d6_solved": (64, 6, 30_011),
	"d6_large": (62, 6, 200_003),
}


def digest(states: dict) -> str:
	"""SHA-256 over the dict in insertion order: key, predecessor key (nothing for the start), action (255 for the start)."""
	h = hashlib.sha256()
	for k, (p, a) in states.items():
		h.update(k)
		h.update(p if p is not None else b"")
		h.update(bytes([255 if a is None else int(a)]))
	return h.hexdigest()


def scramble(is2024: bool, seed: int, depth: int) -> np.ndarray:
	cube.set_is2024(is2024)
	rng = np.random.RandomState(seed)
	state = cube.get_solved()
	for a in rng.randint(0, 12, depth):
		state = cube.rotate(state, *cube.action_space[a])
	return state


def main():
	out = {}
	for tag, (seed, depth, budget) in CASES.items():
		out[f"{tag}_params"] = np.array([seed, depth, budget], np.int64)
		for rep, is2024 in (("2024", True), ("686", False)):
			start = scramble(is2024, seed, depth)
			agent = agents.BFS()
			ok = bool(agent.search(start, max_states=budget))
			keys = list(agent.states)[:256]
			out[f"{tag}_{rep}_start"] = np.asarray(start, np.int8)
			out[f"{tag}_{rep}_result"] = np.array([int(ok), len(agent), len(agent.action_queue)], np.int64)
			out[f"{tag}_{rep}_queue"] = np.array(list(agent.action_queue), np.int64)
			out[f"{tag}_{rep}_sha"] = np.array(digest(agent.states))
			out[f"{tag}_{rep}_keys"] = np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), -1)
			print(tag, rep, ok, len(agent), list(agent.action_queue), flush=True)
	cube.set_is2024(True)
	np.savez_compressed(OUT, **out)
	print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
	main()
