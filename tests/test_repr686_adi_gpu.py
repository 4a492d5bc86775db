"""ADI training data for a net of the 6x8x6 representation against the unmodified reference's Train.ADI_traindata in 6x8x6 mode
(tests/golden/repr686_search.npz): the same walks, 288-wide one-hot states, the targets and the loss weights, all four reward methods."""
import hashlib
import os

import numpy as np
import pytest

from librubiks_amd import cube
from librubiks_amd.adi import adi_traindata
from tests.repr686_nets import NoisyStubNet686

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("method", ["lapanfix", "paper", "schultzfix", "reward0"])
def test_adi_equals_reference(method):
	with np.load(os.path.join(GOLDEN, "repr686_search.npz")) as z:
		t = {k: z[k] for k in z.files if k.startswith(f"adi_{method}_")}
	p = f"adi_{method}_"
	seed, games, depth, ff = (int(x) for x in t[p + "params"])
	cube.set_is2024(False)
	np.random.seed(seed)
	oh, policy, value, lw = adi_traindata(NoisyStubNet686(4), games, depth, float(t[p + "alpha"]), method, ff_batches=ff)
	oh = oh.cpu().numpy()
	assert oh.shape == (games * depth, 288)
	assert hashlib.sha256(oh.tobytes()).hexdigest() == str(t[p + "oh_sha256"])
	assert (policy.numpy() == t[p + "policy"]).all()
	assert (value.numpy() == t[p + "value"]).all()
	assert (lw.numpy() == t[p + "loss_weights"]).all()
	with pytest.raises(ValueError):
		adi_traindata(NoisyStubNet686(4), 2, 2, 0.5, method, fused_first_layer=True)
