"""
What the agents that drive a device engine share on the host, each concern defined once: how the net is fed and read, how a
step becomes a kept hipGraph, and how a finished search is read back (the lifetime of a library object is `_ffi.Owner`).  The
engines: `rk_astar_*` (single and sharded), `rk_astarb_*`, `rk_mcts_*`; the breadth-first and ball searches `rk_bfs_*`,
`rk_bibfs_*`, `rk_bsearch_*`, `rk_ssearch_*` and the batched `rk_bsearchb_*`, `rk_ssearchb_*`, which run no net; and the net-stepped engines
`rk_egvm_*`, `rk_greedy_*`, `rk_beam_*`, `rk_beamb_*`, which own their net batch (`engine_batch`).  agents.py and sharded.py hold what differs
between the engines; what the agents of a family share beyond this module is a private base there (`_PoolSearch`, `_BallSearch`,
`_BallSearchBatch`, and `_NetStepped`: the engine-owned batches as tensors, the kept steps and their lifetime).
"""
from __future__ import annotations

import ctypes as C
import warnings
from collections import deque

import numpy as np
import torch

from librubiks_amd import gpu, _ffi
from librubiks_amd import cube
from librubiks_amd.cube.cube import _solved2024 as SOLVED20  # the 20-byte solved state, whatever the repr


# -- the net's input and output -----------------------------------------------------------------------------------------
OH_CODES = {torch.float32: _ffi.OH_F32, torch.float16: _ffi.OH_F16, torch.bfloat16: _ffi.OH_BF16}
OH_DTYPES = {_ffi.OH_F32: torch.float32, _ffi.OH_F16: torch.float16, _ffi.OH_BF16: torch.bfloat16, _ffi.OH_STATES: torch.int8}


# -- the A* engines' error codes (rk_astar_status slot 6, rk_astarb_status column 6, slot 7 of a sharded decision) ----------
ASTAR_ERRORS = {1: "pool capacity exceeded", 2: "look-back chain broken", 3: "more new states than net rows were evaluated",
                4: "NaN among the net's values of the new states"}


def astar_errors(codes) -> str:
	"""The texts of the non-zero A* error codes in `codes` (ints), for the message of a RubiksHipError."""
	return "; ".join(f"{k}: {ASTAR_ERRORS.get(k, '?')}" for k in sorted({int(c) for c in codes if int(c)}))


def param_dtype(net):
	"""The dtype of the net's first floating-point parameter; None for anything that is not a torch module with one."""
	params = getattr(net, "parameters", None)
	if callable(params):
		for prm in params():
			if prm.dtype in OH_CODES:
				return prm.dtype
	return None


def oh_dtype(net) -> torch.dtype:
	"""
	The dtype the net wants its one-hot input in: that of its first floating-point parameter (a bf16/fp16 net gets a
	bf16/fp16 one-hot straight from the kernel -- 0/1 are exact, and no cast kernel or float32 copy is needed);
	float32 for anything that is not a torch module.
	"""
	return param_dtype(net) or torch.float32


def has_f32_weights(net) -> bool:
	"""True for a torch module whose first floating-point parameter is float32 (a forward pass on thousands of rows then
	costs milliseconds); False for low-precision nets and for parameter-free heuristics."""
	return param_dtype(net) == torch.float32


def net_batch(rows: int, code: int, kept: torch.Tensor = None, zeros: bool = True) -> torch.Tensor:
	"""
	The buffer an engine writes the net's batch into: (rows, 20) int8 for RK_OH_STATES -- solved states, so that every row holds
	valid codes before the engine has written it -- else a (rows, 480) one-hot in the dtype of `code`, zeroed unless told otherwise.
	`kept`, the buffer a kept hipGraph was captured on, is used again when it fits (the step rewrites rows before they are read).
	"""
	dtype = OH_DTYPES[code]
	if kept is not None and len(kept) == rows and kept.dtype == dtype:
		return kept
	if code == _ffi.OH_STATES:
		return torch.from_numpy(cube.repeat_state(SOLVED20, rows)).to(gpu)
	return (torch.zeros if zeros else torch.empty)((rows, 480), dtype=dtype, device=gpu)


#: Rows per net forward.  A forward on B rows streams B x 4096 activations per layer through every elementwise kernel
#: of the torch module (Linear, ELU, BatchNorm ...); while a slice's activations fit the 256 MiB Infinity Cache those
#: kernels run out of it, beyond that every one of them goes to HBM: 64 searches x 12 000 rows in ONE forward ran four
#: times slower PER ROW than 12 000-row forwards (profiles/r02_astar_batch.json: batch 0.22x of sequential at N = 1000).
#: 16 384 rows x 4 096 x 2 B = 134 MB (bf16).  The reference slices its own large forwards the same way (train.py:301-311).
NET_SLICE_ROWS = 16_384


def value_of(out):
	return out[-1] if isinstance(out, (list, tuple)) else out


def sliced_value_forward(forward, rows: torch.Tensor, max_rows: int = None):
	"""The value head of `forward` on `rows`, evaluated in slices of at most `max_rows` rows (see NET_SLICE_ROWS)."""
	max_rows = max_rows or NET_SLICE_ROWS
	n = len(rows)
	if n <= max_rows:
		return value_of(forward(rows, policy=False, value=True))
	return torch.cat([value_of(forward(rows[i:i + max_rows], policy=False, value=True)).reshape(-1) for i in range(0, n, max_rows)])


def engine_values(out):
	"""
	-> (values, RK_OH_* code): the net's value head as the A* engines take it.  A bfloat16 net's values go in as they are (the
	engine widens them, exactly), anything else as a contiguous float32 vector on the GPU.  The caller tells its engine the code:
	the single engine with every batch (rk_astar_set_values_dtype), the batched one when it changes (rk_astarb_set_values_dtype).
	One call deep on purpose: it runs once per eager iteration, which is host-bound at small N.
	"""
	v = out[-1] if isinstance(out, (list, tuple)) else out
	if isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.bfloat16 and v.is_contiguous():
		return v.detach().reshape(-1), _ffi.OH_BF16
	return v.detach().to(device=gpu, dtype=torch.float32).reshape(-1).contiguous(), _ffi.OH_F32


def engine_logits(out):
	"""-> (logits (rows, 12) contiguous, RK_OH_* code): the net's policy head as an engine takes it, bfloat16 as it is, anything
	else as float32 (widening is exact)."""
	p = (out[0] if isinstance(out, (list, tuple)) else out).detach()
	if p.is_cuda and p.dtype == torch.bfloat16:
		return p.reshape(-1, 12).contiguous(), _ffi.OH_BF16
	return p.to(device=gpu, dtype=torch.float32).reshape(-1, 12).contiguous(), _ffi.OH_F32


class _DeviceBytes:
	"""`nbytes` bytes of device memory that the library owns, for torch.as_tensor (the CUDA array interface)."""
	def __init__(self, ptr: int, nbytes: int):
		self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def engine_batch(ptr: int, rows: int, code: int) -> torch.Tensor:
	"""A net batch that an ENGINE owns (rk_egvm_net_in) as a tensor, no copy: (rows, 20) int8 for RK_OH_STATES, else (rows, 480)
	in the dtype of `code`.  The memory lives as long as the engine: whoever holds the tensor drops it before the engine goes."""
	dtype = OH_DTYPES[code]
	cols = 20 if code == _ffi.OH_STATES else 480
	raw = torch.as_tensor(_DeviceBytes(ptr, rows * cols * dtype.itemsize))
	if raw.data_ptr() != ptr or not raw.is_cuda:
		raise _ffi.RubiksHipError("torch copied the engine's batch instead of wrapping it")
	return raw.view(dtype).reshape(rows, cols)


# -- a step as a hipGraph ---------------------------------------------------------------------------------------------
#: How every search step is captured: errors of the capture are judged per THREAD.  In a process with a torch.distributed process group
#: the NCCL (RCCL) watchdog thread polls events while the main thread captures; under the default "global" mode such a call from another
#: thread invalidates the capture -- a sporadic failure of the first search of a rank (seen once in the round-5 test runs).
CAPTURE = {"capture_error_mode": "thread_local"}


def capture_key(net, forward) -> tuple:
	"""What a captured search step holds of the net: the module, its mode, and the storage of every parameter and buffer (their
	VALUES are read at replay time, so in-place training between searches keeps a captured step valid), and `forward`, what the
	step calls (DeepAgent._begin_net): the net itself, its 6x8x6 adapter, or the fused copy, which is rebuilt -- a new object --
	whenever the values change."""
	ptrs = []
	for get in ("parameters", "buffers"):
		it = getattr(net, get, None)
		if callable(it):
			ptrs += [(t.data_ptr(), t.dtype) for t in it()]
	return (id(net), bool(getattr(net, "training", False)), tuple(ptrs), id(forward))


def capture(warm, step) -> torch.cuda.CUDAGraph:
	"""`warm()` -- real work that also warms the allocator -- on a side stream, then what `step()` enqueues as a hipGraph."""
	side = torch.cuda.Stream()
	side.wait_stream(torch.cuda.current_stream())
	with torch.cuda.stream(side):
		warm()
	torch.cuda.current_stream().wait_stream(side)
	graph = torch.cuda.CUDAGraph()
	with torch.cuda.graph(graph, **CAPTURE):
		step()
	return graph


def kept_graph(agent, key: tuple, warm, step, oh: torch.Tensor, keep):
	"""
	-> (hipGraph of `step`, whether it is the one kept from an earlier search).  A captured step holds addresses and scalars
	passed by value, nothing of a search, so the agent keeps it in `_graph_cache` = (key, graph, batch buffer, *keep) and captures
	again (`capture`, counted in `agent.captures`) only when `key` -- everything the step holds -- differs.  `keep` is what must
	stay alive with the graph because the graph holds its addresses (the net and what the step calls of it): a tuple, or a
	callable that returns one once the graph is made, for items that the warm-up makes.
	"""
	kept = agent._graph_cache
	if kept is not None and kept[0] == key:
		return kept[1], True
	agent._graph_cache = kept = None               # the old graph goes before the new one is made (unless the caller still holds it)
	graph = capture(warm, step)
	agent._graph_cache = (key, graph, oh, *(keep() if callable(keep) else keep))
	agent.captures += 1
	return graph, False


# -- arguments ---------------------------------------------------------------------------------------------------------
def int_in(name: str, value, lo: int, hi: int = None, none_ok: bool = False, what: str = None):
	"""`value` as an int when it is an integer (no bool, no fraction) in lo..hi -- `hi` None: no upper limit --, None for a None
	that `none_ok` allows; else ValueError "<name> must be <what>, got <value>", `what` by default "an integer in lo..hi"."""
	if value is None and none_ok:
		return None
	if isinstance(value, bool) or int(value) != value or int(value) < lo or (hi is not None and int(value) > hi):
		raise ValueError(f"{name} must be {what or f'an integer in {lo}..{hi}'}, got {value!r}")
	return int(value)


# -- the search loop and its results ----------------------------------------------------------------------------------------
def burst(poll: int, room: int, K: int) -> int:
	"""Iterations to launch before the host looks again.  Never launch past the budget: a search grows by at most K states per
	iteration, so with `room` states left it cannot reach its budget in fewer than room // K iterations -- launch that many (at
	least one, at most `poll`)."""
	return max(1, min(poll, room // K))


def events(n: int) -> list:
	"""Measurement aid: `n` HIP timing events for the marks of one step, made before the step so that making them is not timed."""
	return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def mark(marks, i: int):
	"""Records mark `i` of a step on the current stream; nothing when `marks` is None."""
	if marks is not None:
		marks[i].record()


class CapacityExhausted(RuntimeWarning):
	"""A search that was limited only by time stopped because its node pool was full (the reference grows its arrays)."""


def pool_exhausted(agent, capacity: int, why: str = "is full with time left"):
	agent.capacity_exhausted = True
	warnings.warn(f"{agent}: node pool of {capacity} states {why}; raise max_capacity", CapacityExhausted, stacklevel=2)


def read_path(entry, *lead, length: int = 4096, strict: bool = True):
	"""The action queue that `entry(*lead, buffer, length, stream)` -- an engine's `*_path` -- writes.  A negative count is the
	library's error code: raised, or None when not `strict` (the caller has another way to the path)."""
	buf = (C.c_longlong * length)()
	n = entry(*lead, buf, length, _ffi.stream_ptr())
	if n < 0:
		if not strict:
			return None
		_ffi.check(int(n))
	return deque(int(a) for a in buf[:n])


def export_pool(entry, lead: tuple, n: int, rows: int = None):
	"""(states, G, parents, parent_actions) with `rows` (default n + 1) rows in the reference's dtypes; rows 1..n are filled by
	`entry(*lead, 1, n, ...)`, an engine's `*_export` (None: there is no engine yet), the others stay zero."""
	rows = rows or n + 1
	states, G = np.zeros((rows, 20), np.int8), np.zeros(rows, np.float64)
	parents, pact = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
	if n and entry is not None:
		_ffi.check(entry(*lead, 1, n, states[1:].ctypes.data, G[1:].ctypes.data, parents[1:].ctypes.data, pact[1:].ctypes.data, _ffi.stream_ptr()))
	return states, G, parents, pact


def export_frontier(entry, lead: tuple, n: int, firsts: int = 1, tags: bool = False) -> tuple:
	"""(states, parents, actions[, tags]) with n + 1 rows of a breadth-first pool (the frontier pool of DESIGN 3.5): rows 1..n are
	filled by `entry(*lead, 1, n, ...)`, an engine's `*_export` (None: there is no engine yet), row 0 stays zero.  The first `firsts`
	nodes have no parent: their action is -1.  `tags`: the export has a fourth column (DeviceBiBFS's sides)."""
	states = np.zeros((n + 1, 20), np.int8)
	cols = [np.zeros(n + 1, np.int64) for _ in range(3 if tags else 2)]
	if n and entry is not None:
		_ffi.check(entry(*lead, 1, n, states[1:].ctypes.data, *(c[1:].ctypes.data for c in cols), _ffi.stream_ptr()))
	cols[1][1:1 + min(firsts, n)] = -1
	return (states, *cols)
