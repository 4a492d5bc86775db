"""
The float64 statement of the fused net ends (librubiks_amd/oh_linear.py, csrc/rk_oh_linear.hip) and the error bounds of their routes.
Plain torch: runs on the CPU (tests/test_oh_linear_ref_cpu.py proves on emulations that the bounds accept a faithful kernel and reject a
subtly wrong one) and on the device (tests/test_oh_linear_exact_gpu.py holds the kernels to them).

    x   = b + sum_i W[:, 24 i + s_i]                      first_layer64: by indexing, in float64, on the values the kernel reads
    ref = scale * act(x) + shift                          epilogue64: ELU as alpha expm1(x), a NaN stays a NaN

u = 2^-24 is the unit roundoff of float32.  Every helper checks EVERY element and names the worst one; none leaves any out.  A NaN in the
reference must be a NaN in the output and the other way round; an infinity must be the same infinity.
"""
import numpy as np
import torch

U = 2.0 ** -24
ACTS = {None: (None, 1.0), "elu": ("elu", 1.0), "elu0.7": ("elu", 0.7), "relu": ("relu", 1.0)}     # name -> (kind, alpha)


def module_of(name):
	return {None: None, "elu": torch.nn.ELU(), "elu0.7": torch.nn.ELU(alpha=0.7), "relu": torch.nn.ReLU()}[name]


def route_weight(weight: torch.Tensor, route: str) -> torch.Tensor:
	"""The values a route sums: the layer's own for the gather route, rounded to bfloat16 (nearest even) for the matrix cores."""
	w = weight.detach()
	return w.float() if route == "gather" else w.to(torch.bfloat16).float()


def first_layer64(states, weight, bias):
	"""-> (x, mag): x[n, h] = b[h] + sum_i W[h, 24 i + s[n, i]] in float64, by indexing the 20 selected columns (no one-hot, no GEMM), and
	mag = |b| + sum_i |w_i|, the scale of the sum's rounding error.  `weight` (H, 480) holds the values the kernel uses (route_weight),
	`bias` (H,) or None."""
	states = torch.as_tensor(states)
	wt = weight.detach().double().t().contiguous()                          # (480, H)
	idx = states.to(wt.device).long() + 24 * torch.arange(20, device=wt.device)
	n, H = len(idx), wt.shape[1]
	b = bias.detach().double() if bias is not None else torch.zeros(H, dtype=torch.float64, device=wt.device)
	x, mag = b.expand(n, H).clone(), b.abs().expand(n, H).clone()
	for i in range(20):
		w = wt[idx[:, i]]
		x += w
		mag += w.abs()
	return x, mag


def act64(x, act, alpha=1.0):
	"""The activation in float64: ELU = x for x > 0, alpha expm1(x) for x <= 0; ReLU; a NaN comes out as a NaN."""
	x = x.double()
	if act == "elu":
		return torch.where(x > 0, x, alpha * torch.expm1(torch.where(x > 0, torch.zeros_like(x), x)))     # NaN > 0 is false: expm1(NaN) = NaN
	if act == "relu":
		return torch.where(x < 0, torch.zeros_like(x), x)                   # NaN < 0 is false: the NaN stays
	assert act is None, act
	return x


def epilogue64(x, act, alpha=1.0, scale=None, shift=None):
	"""scale * act(x) + shift in float64; `scale` and `shift` are the float32 tensors of `batchnorm_affine`, widened (or both None)."""
	a = act64(x, act, alpha)
	if scale is not None:
		a = a * scale.double() + shift.double()
	return a


def cover_states(seed: int) -> np.ndarray:
	"""480 rows (int8): in row j cubie j // 24 holds code j % 24, the other 19 cubies hold seeded codes in 0 .. 23 -- every (cubie, code)
	pair is selected by some row, the codes 0, 7, 8, 15, 16 and 23 on the edges of the MFMA fragment's 8-column windows among them.
	The rows are NOT legal cubes and need not be: the layer is a table lookup per cubie, and all three kernels accept any code below 24."""
	rows = np.random.RandomState(seed).randint(0, 24, size=(480, 20))
	j = np.arange(480)
	rows[j, j // 24] = j % 24
	return rows.astype(np.int8)


def random_states(n: int, seed: int) -> np.ndarray:
	"""n rows of seeded codes in 0 .. 23 (not legal cubes, see cover_states): for shapes where only the launch geometry matters"""
	return np.random.RandomState(seed).randint(0, 24, size=(n, 20)).astype(np.int8)


def _check(y, ref, bound, what):
	"""Every element of y within `bound` of ref; NaN exactly where ref is NaN, an infinity exactly where ref is that infinity.
	Where ref is infinite the bound (built from |ref| and mag) is infinite too and says nothing: such an element passes only as the same
	infinity, and any other element whose bound is not finite is out of bound, so no element can pass on inf <= inf.
	-> the largest |y - ref| / bound seen (for the record; never a NaN).  Fails naming the worst element."""
	y, ref, bound = y.detach().double(), ref.detach().double(), bound.detach().double()
	assert y.shape == ref.shape == bound.shape, (y.shape, ref.shape, bound.shape)
	settled = (torch.isnan(y) & torch.isnan(ref)) | (torch.isinf(ref) & (y == ref))
	zero = torch.zeros_like(ref)
	err, bound = torch.where(settled, zero, (y - ref).abs()), torch.where(settled, zero, bound)
	# a NaN on one side only or a NaN bound fails the compare; another value where ref is an infinity; a bound that cannot bind
	bad = ~(err <= bound) | (torch.isinf(ref) & ~settled) | ~torch.isfinite(bound)
	ratio = torch.where(bad & ~(torch.isfinite(err) & torch.isfinite(bound)), torch.full_like(err, float("inf")), err / bound.clamp_min(1e-300))
	ratio = torch.where(settled, zero, ratio)
	assert not torch.isnan(ratio).any()
	worst = int(ratio.argmax())
	if bad.any():
		at = np.unravel_index(worst, tuple(y.shape))
		raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst at {tuple(int(a) for a in at)}: "
		                     f"got {float(y.reshape(-1)[worst])!r}, reference {float(ref.reshape(-1)[worst])!r}, "
		                     f"|diff| {float(err.reshape(-1)[worst]):.6g} > bound {float(bound.reshape(-1)[worst]):.6g}")
	return float(ratio.reshape(-1)[worst])


def assert_f32_preactivation(y, x, mag, what="f32 pre-activation"):
	"""The gather route without an epilogue: twenty sequential float32 adds, |y - x| <= 21 u mag (gamma_20 = 20 u / (1 - 20 u) < 21 u)."""
	return _check(y, x, 21 * U * mag, what)


def assert_bf16_output(y, x, mag, act=None, alpha=1.0, scale=None, shift=None, what="bf16 output"):
	"""A bfloat16 result of the layer (either MFMA form; the gather route with a bfloat16 output) against epilogue64(x):

	    |y - ref| <= 2^-8 |ref| + |scale| max(1, alpha) 64 u mag + T_exp

	2^-8 |ref|: the half ulp of bfloat16 (8 significant bits, nearest even).  64 u mag: the sum of at most 21 non-zero terms in float32
	(21 u mag if every add rounded to nearest), times three because the matrix core's internal add rounding is not documented as nearest
	even; |scale| max(1, alpha) is the Lipschitz constant of the epilogue behind it.  T_exp = |scale| alpha 2^-21 for ELU, else 0: the
	absolute error of the fast exp(x) - 1, a value near 1 rounded to float32 (2^-24) and the hardware exp's own few ulp of it."""
	ref = epilogue64(x, act, alpha, scale, shift)
	s = scale.double().abs() if scale is not None else torch.ones((), dtype=torch.float64, device=ref.device)
	t_exp = s * alpha * 2.0 ** -21 if act == "elu" else 0.0
	bound = 2.0 ** -8 * ref.abs() + s * max(1.0, alpha if act == "elu" else 1.0) * 64 * U * mag + t_exp
	return _check(y, ref, bound.expand_as(ref), what)


def assert_f32_epilogue(y, x32, act=None, alpha=1.0, scale=None, shift=None, what="f32 epilogue"):
	"""The float32 epilogue on its own: x32 is the gather route's float32 output WITHOUT an epilogue (proven bit-exact elsewhere), y the same
	launch with the epilogue, ref = epilogue64(x32):

	    |y - ref| <= 2^-20 |scale act64(x32)| + 2^-23 |ref| + 1e-37

	2^-20 = 16 u relative to the product: 4 ulp (8 u) for expm1f, one rounding each for alpha * e and scale * a; 2^-23 |ref| = 2 u for the
	add of the shift; 1e-37 for results in the denormal range.  This is the bound that tells expm1(x) from exp(x) - 1, whose absolute error
	of 2^-25 .. 2^-24 is 1e-4 relative at x = -1e-3: a bound on the whole layer cannot, the sum's own 21 u mag is larger."""
	assert x32.dtype == torch.float32 and y.dtype == torch.float32
	a = act64(x32, act, alpha)
	ref = epilogue64(x32, act, alpha, scale, shift)
	prod = (a * scale.double()).abs() if scale is not None else a.abs()
	return _check(y, ref, 2.0 ** -20 * prod + 2.0 ** -23 * ref.abs() + 1e-37, what)


def assert_tail(y, ref, mag, what="tail"):
	"""rk_tail_linear against float64 on the same bfloat16 numbers: the final rounding to bfloat16 (2^-8 relative) and the float32
	accumulation (1e-5 of the sum of magnitudes), the bound of test_tail_linear_is_activation_plus_linear."""
	return _check(y, ref, 2.0 ** -8 * ref.abs() + 1e-5 * mag + 1e-30, what)


def elu_teeth(x32) -> int:
	"""How many pre-activations lie in (-0.1, -1e-3), where exp(x) - 1 in float32 is off by 1e-4 relative and expm1 is not."""
	return int(((x32 > -0.1) & (x32 < -1e-3)).sum())
