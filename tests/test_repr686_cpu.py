"""
CPU checks of the 6x8x6 path: the committed fixtures (tools/gen_golden_repr686.py) are self-consistent -- every colour row is a
legal 6x8x6 one-hot, the recorded hashes belong to the rows, the stub nets give integer values -- and the new C-ABI entries refuse
to run without a device instead of falling back.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube
from tests.repr686_nets import SOLVED_OH686, StubNet686, NoisyStubNet686, PolicyStubNet686

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
	with np.load(os.path.join(GOLDEN, name)) as z:
		return {k: z[k] for k in z.files}


def as_states(colours: np.ndarray) -> np.ndarray:
	"""(n, 48) colours -> (n, 6, 8, 6) int8 one-hot states."""
	return (np.asarray(colours)[:, :, None] == np.arange(6)).astype(np.int8).reshape(-1, 6, 8, 6)


def _legal_colours(c: np.ndarray) -> bool:
	# every colour shows on 8 slots, and the 48 slots hold 0..5 only
	return c.min() >= 0 and c.max() <= 5 and all((np.bincount(row, minlength=6) == 8).all() for row in c.astype(np.int64))


def test_cube_fixture_is_consistent():
	f = _load("repr686_cube.npz")
	c = f["colours686"]
	assert c.shape == (len(f["actions"]), 48) and _legal_colours(c)
	assert hashlib.sha256(as_states(c).tobytes()).hexdigest() == str(f["sha686"])
	# depth 0 is solved in both forms; the 12 single moves differ from solved and from each other
	assert (c[0] == np.arange(48) // 8).all() and (f["states20"][0] == np.r_[3 * np.arange(8), 2 * np.arange(12)]).all()
	assert len({r.tobytes() for r in c[1:13]}) == 12 and not (c[1:13] == c[0]).all(axis=1).any()


def test_search_fixture_is_consistent():
	f = _load("repr686_search.npz")
	for kind in ("astar_a", "astar_b", "astar_c", "mcts_a", "mcts_b"):
		c = f[f"{kind}_states"]
		assert len(c) == int(f[f"{kind}_n"]) and _legal_colours(c)
		assert hashlib.sha256(as_states(c).tobytes()).hexdigest() == str(f[f"{kind}_states_sha"])
		assert len({r.tobytes() for r in c}) == len(c)                     # node identity: every state once
	for method in ("lapanfix", "paper", "schultzfix", "reward0"):
		c = f[f"adi_{method}_colours"]
		assert _legal_colours(c)
		assert hashlib.sha256(as_states(c).astype(np.float32).reshape(len(c), 288).tobytes()).hexdigest() == str(f[f"adi_{method}_oh_sha256"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stub_nets_give_integers(dtype):
	f = _load("repr686_search.npz")
	x = torch.from_numpy(as_states(f["astar_b_states"]).reshape(-1, 288)).to(dtype)
	for net in (StubNet686(dtype), NoisyStubNet686(1, dtype), PolicyStubNet686(dtype)):
		p, v = net(x)
		assert v.dtype == torch.float32 and (v == v.round()).all() and (v <= 3).all() and (v >= -51).all()
		assert ((p == 0) | (p == -np.inf)).all()
	solved = torch.from_numpy(SOLVED_OH686)[None]
	assert float(StubNet686()(solved, policy=False)) == 0.0
	finite = (PolicyStubNet686()(x, value=False) == 0).sum(dim=1)
	assert set(finite.tolist()) <= {4, 8}


def test_new_entries_refuse_without_device():
	lib = _ffi.lib()
	if torch.cuda.is_available():
		pytest.skip("a device is visible: the no-device refusal is not observable here")
	with pytest.raises(_ffi.RubiksHipError):
		cube.as686(cube.get_solved()[None])
	cube.set_is2024(False)
	with pytest.raises(_ffi.RubiksHipError):
		cube.as2024(cube.get_solved()[None])
	# argument checks come before any launch: a bad dtype, a misaligned pointer
	assert lib.rk_oh686_from2024(16, 16, 9, 1, None) == -1
	assert lib.rk_oh686_from2024(16, 24, _ffi.OH_F32, 1, None) == -1
	assert lib.rk_686_to2024(24, 16, None, 1, None) == -1
	assert lib.rk_686_to2024(None, None, None, 0, None) == 0
