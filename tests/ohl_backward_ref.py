"""
The float64 statement of the first layer's backward (rk_ohl_backward, librubiks_amd/csrc/rk_oh_linear.hip) and its error bound.  Plain torch:
runs on the CPU (tests/test_ohl_backward_ref_cpu.py proves on emulations that the bound accepts a faithful kernel in two summation orders and
rejects five subtly wrong ones) and on the device (tests/test_ohl_backward_gpu.py holds the kernel to it).

    dW[h, 24 i + v] = sum over the rows r with code(r, i) = v of dY[r, h]          db[h] = sum_r dY[r, h]

code(r, i) is the forward's: the byte read as unsigned, anything >= 24 counts as 23.

The bound is derived, not tuned.  A float32 sum of c terms x_1 .. x_c, in ANY order (sequential, pairwise, in splits), errs by at most
gamma_{c-1} sum |x_j| with gamma_k = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); for
c < 2^20 that is below c u sum |x_j|.  So an element of dW whose bin holds `count` rows is within count * u * magW of the float64 sum, magW
the same sum over |dY|, and db[h] within n * u * magB.  An empty bin has bound 0: it must be exactly zero.  The check itself is
oh_linear_ref._check: every element, NaN exactly where the reference has one, an infinity only as the same infinity.
"""
import torch

from tests import oh_linear_ref as R

U = R.U


def codes_of(states) -> torch.Tensor:
	"""(n, 20) int64 codes as the kernels read them: the byte as unsigned, anything >= 24 counts as 23"""
	c = torch.as_tensor(states).long() & 0xFF
	return torch.where(c < 24, c, torch.full_like(c, 23))


def first_layer_grad64(states, dy):
	"""-> (dW, db, magW, magB, count): dW (H, 480) and db (H,) in float64 by index_add on dY's float32 values widened; magW / magB the same
	sums of |dY|; count (480,) int64 the number of rows in every bin."""
	dy = dy.detach().double()
	n, H = dy.shape
	dev = dy.device
	idx = codes_of(states).to(dev) + 24 * torch.arange(20, device=dev)      # (n, 20) one-hot columns
	dWt = torch.zeros((480, H), dtype=torch.float64, device=dev)
	magWt = torch.zeros_like(dWt)
	count = torch.zeros(480, dtype=torch.int64, device=dev)
	for i in range(20):
		dWt.index_add_(0, idx[:, i], dy)
		magWt.index_add_(0, idx[:, i], dy.abs())
		count.index_add_(0, idx[:, i], torch.ones(n, dtype=torch.int64, device=dev))
	return dWt.t().contiguous(), dy.sum(0), magWt.t().contiguous(), dy.abs().sum(0), count


def assert_grad(dw, db, ref, what="first layer backward"):
	"""dW within count u magW and db within n u magB of `ref` = first_layer_grad64(...).  -> the largest error / bound ratio seen."""
	dW, dB, magW, magB, count = ref
	n = int(count[:24].sum())
	assert n < 2 ** 20, "the bound c u mag needs c < 2^20"
	ratio = R._check(dw, dW, count.double()[None, :] * U * magW, what + ": dW")
	if db is not None:
		ratio = max(ratio, R._check(db, dB, n * U * magB, what + ": db"))
	return ratio
