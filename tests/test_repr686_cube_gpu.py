"""
The 20-byte <-> 6x8x6 kernels (rk_oh686_from2024, rk_686_to2024) against the unmodified reference's paired walks
(tests/golden/repr686_cube.npz, tools/gen_golden_repr686.py) and against the existing 6x8x6 one-hot (as_oh in 6x8x6 mode).
"""
import os

import numpy as np
import pytest
import torch

from librubiks_amd import _ffi, cube, gpu
from tests.test_repr686_cpu import as_states

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def walks():
	with np.load(os.path.join(GOLDEN, "repr686_cube.npz")) as z:
		return {k: z[k] for k in z.files}


def _random20(n: int, seed: int) -> torch.Tensor:
	rng = np.random.RandomState(seed)
	s = torch.from_numpy(np.tile(np.r_[3 * np.arange(8), 2 * np.arange(12)].astype(np.int8), (n, 1))).to(gpu)
	for _ in range(25):
		s = cube.device.multi_rotate(s, torch.from_numpy(rng.randint(0, 12, n).astype(np.uint8)).to(gpu))
	return s


def test_to686_and_back_equal_the_reference_walks(walks):
	s20 = torch.from_numpy(walks["states20"]).to(gpu)
	want = as_states(walks["colours686"])
	got = cube.device.to686(s20)
	assert got.shape == (len(want), 6, 8, 6) and (got.cpu().numpy() == want).all()
	assert (cube.device.from686(got).cpu().numpy() == walks["states20"]).all()
	# host-level pair, in either current repr
	assert (cube.as686(walks["states20"]) == want).all()
	cube.set_is2024(False)
	assert (cube.as2024(want) == walks["states20"]).all()
	assert (cube.as686(walks["states20"][5]) == want[5]).all() and (cube.as2024(want[7]) == walks["states20"][7]).all()


def test_as633_of_both_forms_agrees():
	s20 = _random20(50, 3)
	s686 = cube.device.to686(s20).cpu().numpy()
	pics = [cube.as633(s) for s in s20.cpu().numpy()]
	cube.set_is2024(False)
	assert all((cube.as633(s686[i]) == pics[i]).all() for i in range(50))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, (1 << 20) + 3])
def test_encodings_equal_as_oh_of_the_686_state(n):
	s20 = _random20(n, n)
	s686 = cube.device.to686(s20)
	cube.set_is2024(False)
	for dtype in (torch.float32, torch.float16, torch.bfloat16):
		want = cube.device.as_oh(s686, dtype=dtype)
		got = cube.device.to686(s20, dtype)
		assert got.shape == (n, 288) and torch.equal(got, want), dtype
		del want, got
	if n:
		assert int(s686.reshape(n, -1).sum(dim=1, dtype=torch.int64).min()) == 48 == int(s686.reshape(n, -1).sum(dim=1, dtype=torch.int64).max())


def test_illegal_rows_are_counted_and_located():
	s686 = cube.device.to686(_random20(200, 9)).reshape(200, 48, 6).clone()
	s686[17, 5] = s686[17, 5].roll(1)                       # one slot shows another colour (a colour then appears 9 times)
	s686[40, 3, :] = 0                                      # an empty slot
	s686[90, 7, (s686[90, 7].argmax() + 1) % 6] = 1         # two ones in a slot
	s686[150, 0], s686[150, 16] = s686[150, 16].clone(), s686[150, 0].clone()  # two stickers of one corner swapped: its mirror image
	stats = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device=gpu)
	out = cube.device.from686(s686.reshape(200, 6, 8, 6), stats=stats)
	bad = {17, 40, 90, 150}
	assert stats.tolist() == [4, 17]
	o = out.cpu().numpy()
	assert (o[sorted(bad)] == -1).all() and (o[[i for i in range(200) if i not in bad]] >= 0).all()
	with pytest.raises(ValueError, match="first is row 17"):
		cube.device.from686(s686.reshape(200, 6, 8, 6))
	cube.set_is2024(False)
	with pytest.raises(ValueError):
		cube.as2024(s686[40:41].reshape(1, 6, 8, 6).cpu().numpy())
	from librubiks_amd.solving.agents import AStar
	from tests.repr686_nets import StubNet686
	with pytest.raises(ValueError):
		AStar(StubNet686(), 0.5, 10).search(s686[90].reshape(6, 8, 6).cpu().numpy(), max_states=1000)


def test_bad_arguments_fail_before_any_launch():
	lib = _ffi.lib()
	s20 = _random20(4, 1)
	out = torch.empty((8, 288), dtype=torch.float32, device=gpu)
	assert lib.rk_oh686_from2024(s20.data_ptr(), out.data_ptr(), 3, 4, None) == -1            # RK_OH_STATES is not an output kind here
	assert lib.rk_oh686_from2024(s20.data_ptr(), out.data_ptr(), 7, 4, None) == -1
	assert lib.rk_oh686_from2024(s20.data_ptr(), out.data_ptr() + 4, _ffi.OH_F32, 4, None) == -1
	assert lib.rk_oh686_from2024(s20.data_ptr() + 2, out.data_ptr(), _ffi.OH_F32, 4, None) == -1
	assert lib.rk_oh686_from2024(None, out.data_ptr(), _ffi.OH_F32, 4, None) == -1
	s686 = cube.device.to686(s20)
	o20 = torch.empty((4, 20), dtype=torch.int8, device=gpu)
	assert lib.rk_686_to2024(s686.data_ptr() + 4, o20.data_ptr(), None, 4, None) == -1
	assert lib.rk_686_to2024(s686.data_ptr(), o20.data_ptr() + 1, None, 4, None) == -1
	st = torch.zeros(3, dtype=torch.int64, device=gpu)
	assert lib.rk_686_to2024(s686.data_ptr(), o20.data_ptr(), st.data_ptr() + 4, 4, None) == -1
	assert lib.rk_686_to2024(None, None, None, 0, None) == 0
	with pytest.raises(ValueError):
		cube.device.to686(s20, torch.int32)
	torch.cuda.synchronize()
	assert torch.equal(cube.device.from686(s686), s20)                                        # nothing was written by the refused calls
