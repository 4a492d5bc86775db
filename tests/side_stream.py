"""
Side-stream test infrastructure ("Streams"): the gate, its calibration and the bit comparisons that the
tests/test_side_stream_*_gpu.py files share.  A helper module: no test, no fixture.

torch's side streams are non-blocking: nothing orders the null stream against them.  `gate(stream, ms)` puts a device-side delay
on `stream`; the work under test is enqueued behind it while the gate is still pending (`held` asserts exactly that: a gate that has
opened makes the test void, and `held` fails saying so).  A launch, copy or wait that an entry point sends to stream 0 instead of
its argument then runs DURING the gate: it reads the decoy the buffers held before the true inputs arrive behind the gate, or is
overwritten, and the bits differ from the default-stream run.  Decoys are valid data of the same kind (other legal states, other
finite values), so a misdirected launch computes a wrong answer and never makes an out-of-range access.

The delay is `torch.cuda._sleep(cycles)`; cycles per millisecond are measured once per process between two events.  Were `_sleep`
not to delay (a gate of the target length must measure at least half of it), the delay would be a run of mid-size 12-child
fan-outs into scratch, calibrated the same way.  That second form has never run on hardware (`_sleep` delays on gfx950): its row
count is below the library's documented threshold for the paced forms, not measured, and if one fan-out is short the host may not
enqueue a whole gate in time -- the tests would then fail as VOID, never pass wrongly.  `gate_form()` says which form is in use;
both figures are printed.
"""
import contextlib
import ctypes as C
import functools
import math

import numpy as np
import torch

from librubiks_amd import _ffi
from oracle import cube_oracle as orc

GATE_MS = 30.0        # long enough that the host has enqueued the work under test while the gate is pending
NET_GATE_MS = 2.0     # GatedNet: re-armed at every iteration of an eager search
MAX_GATE_MS = 200.0
SENTINEL = 0x5A       # output prefill: 0x5A5A5A5A is a finite float32 (1.5e16), 0x5A5A a finite bfloat16, 90 as a byte
_FANOUT_ROWS = 150_000                   # below the paced forms, which order streams among themselves


def _timed(enqueue) -> float:
	"""milliseconds on the device of what `enqueue` puts on the current stream"""
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	torch.cuda.synchronize()
	a.record()
	enqueue()
	b.record()
	b.synchronize()
	return a.elapsed_time(b)


@functools.lru_cache(maxsize=None)
def _fanout_delay():
	"""(enqueue one fan-out, milliseconds of one) for the gate's second form"""
	parents = torch.from_numpy(orc.repeat_state(orc.SOLVED, _FANOUT_ROWS)).cuda()
	children = torch.empty((12 * _FANOUT_ROWS, 20), dtype=torch.int8, device="cuda")
	flags = torch.empty(12 * _FANOUT_ROWS, dtype=torch.uint8, device="cuda")

	def one():
		_ffi.check(_ffi.lib().rk_expand12(_ffi.REPR_2024, parents.data_ptr(), children.data_ptr(), flags.data_ptr(), None, _FANOUT_ROWS, _ffi.stream_ptr()))
	one()
	ms = _timed(lambda: [one() for _ in range(32)]) / 32
	print(f"side_stream: one unpaced fan-out of {_FANOUT_ROWS} parents takes {ms:.4f} ms")
	return one, ms


@functools.lru_cache(maxsize=None)
def sleep_rate() -> float:
	"""Cycles of torch.cuda._sleep per millisecond on this device, measured once; 0.0 if _sleep does not delay (then the gate is
	built from fan-outs).  Also the one place that checks what the whole argument rests on: torch's default stream IS stream 0."""
	assert torch.cuda.default_stream().cuda_stream == 0, "torch's default stream is not the null stream: the side-stream tests prove nothing"
	assert _ffi.lib().rk_init(0) == 0, _ffi.lib().rk_last_error()
	torch.cuda._sleep(1000)
	cycles, ms = 100_000, 0.0
	while cycles < 10 ** 9:                # (a tenfold step from below 2 ms stays below 20 ms)
		cycles *= 10
		ms = _timed(lambda: torch.cuda._sleep(cycles))
		if ms >= 2.0:
			break
	rate = cycles / max(ms, 1e-6)
	got = _timed(lambda: torch.cuda._sleep(int(rate * GATE_MS))) if ms >= 2.0 else 0.0
	delays = got >= GATE_MS / 2
	print(f"side_stream: torch.cuda._sleep({cycles}) took {ms:.3f} ms = {rate:.0f} cycles/ms; a {GATE_MS:.0f} ms gate measured {got:.2f} ms; "
	      f"gate form: {'_sleep' if delays else 'fan-outs'}")
	return rate if delays else 0.0


def gate_form() -> str:
	return "_sleep" if sleep_rate() else "fan-outs"


def delay(ms: float) -> None:
	"""`ms` milliseconds of device-side delay on the current stream"""
	assert 0 < ms <= MAX_GATE_MS
	rate = sleep_rate()
	if rate:
		torch.cuda._sleep(int(rate * ms))
		return
	one, each = _fanout_delay()
	for _ in range(int(math.ceil(ms / each))):
		one()


def gate(stream: torch.cuda.Stream, ms: float = GATE_MS) -> torch.cuda.Event:
	"""A delay of `ms` on `stream`; -> an event recorded behind it (complete once the gate has opened)."""
	sleep_rate()
	with torch.cuda.stream(stream):
		delay(ms)
		ev = torch.cuda.Event()
		ev.record(stream)
	return ev


def held(ev: torch.cuda.Event) -> None:
	"""After the last enqueue-only call, before the first blocking one: the gate is still closed, or the test is void."""
	assert not ev.query(), "VOID: the gate had opened before the work under test was enqueued -- nothing was shown (lengthen the gate or enqueue less)"


def side_stream() -> torch.cuda.Stream:
	"""A side stream that starts behind everything the default stream holds now (step 2 of pattern A)."""
	sleep_rate()
	s = torch.cuda.Stream()
	assert s.cuda_stream != 0
	s.wait_stream(torch.cuda.default_stream())
	return s


class GatedNet:
	"""A net (any callable of the agents' kind) whose every call first puts a short gate on the current stream: its outputs arrive
	late at every iteration of an eager search, so a commit or backup sent to the null stream reads the previous iteration's (valid,
	stale) outputs.  `last` is the event behind the newest gate; everything else is the wrapped net's."""

	def __init__(self, net, ms: float = NET_GATE_MS):
		self.net, self.ms, self.calls, self.last = net, ms, 0, None

	def eval(self):
		self.net.eval()
		return self

	def __call__(self, *args, **kwargs):
		delay(self.ms)
		self.last = torch.cuda.Event()
		self.last.record()
		self.calls += 1
		return self.net(*args, **kwargs)

	def __getattr__(self, name):
		return getattr(self.__dict__["net"], name)

	def fresh_gate(self):
		"""-> callable for `watch`: the newest gate's event the first time it is asked after a forward, None until the next forward"""
		seen = [self.calls]

		def event():
			if self.calls == seen[0]:
				return None
			seen[0] = self.calls
			return self.last
		return event


@contextlib.contextmanager
def watch(names, event_of, before: bool = False, once: bool = False):
	"""While inside, every call of the library entries `names` notes whether the gate of `event_of()` (None: nothing to note) was
	still closed -- after the call returns (an enqueue-only entry: the last enqueue behind that gate) or `before` it starts (an entry
	that synchronises), `once`: at the first such call only.  -> the list of notes; a test asserts that it is non-empty and all True."""
	lib, notes, saved = _ffi.lib(), [], {}

	def note():
		ev = event_of()
		if ev is not None and not (once and notes):
			notes.append(not ev.query())

	def wrap(entry):
		def call(*args):
			if before:
				note()
			out = entry(*args)
			if not before:
				note()
			return out
		return call
	for name in names:
		saved[name] = getattr(lib, name)
		setattr(lib, name, wrap(saved[name]))
	try:
		yield notes
	finally:
		for name, entry in saved.items():
			setattr(lib, name, entry)


def all_held(notes) -> None:
	assert notes and all(notes), f"VOID: {len(notes)} gated calls, {sum(1 for x in notes if not x)} of them after their gate had opened"


def bits(t: torch.Tensor) -> torch.Tensor:
	"""the tensor's bytes, for bitwise comparison (NaN == NaN, -0.0 != +0.0)"""
	return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
	return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def sentinel(shape, dtype) -> torch.Tensor:
	"""an output buffer on the device with every byte SENTINEL (made on the current stream)"""
	t = torch.empty(shape, dtype=dtype, device="cuda")
	bits(t).fill_(SENTINEL)
	return t


def scrambles(n: int, depth: int, seed: int) -> np.ndarray:
	"""n legal 20-byte states, each `depth` seeded random moves from solved"""
	rs = np.random.RandomState(seed)
	s = orc.repeat_state(orc.SOLVED, n)
	for _ in range(depth):
		s = orc.multi_rotate(s, rs.randint(0, 6, n), rs.randint(0, 2, n))
	return s


def mixed_depths(n: int, deepest: int, seed: int) -> np.ndarray:
	"""n legal states scrambled 0 .. `deepest` moves deep in turn (row i: i % (deepest + 1) moves)"""
	rs = np.random.RandomState(seed)
	s = orc.repeat_state(orc.SOLVED, n)
	want = np.arange(n) % (deepest + 1)
	for d in range(deepest):
		moved = orc.multi_rotate(s, rs.randint(0, 6, n), rs.randint(0, 2, n))
		s = np.where((want > d)[:, None], moved, s)
	return s


def status_words(entry, handle, words: int, *before) -> list:
	"""one blocking rk_*_status on the current stream -> its words"""
	st = (C.c_longlong * words)()
	_ffi.check(entry(handle, *before, st, _ffi.stream_ptr()))
	return list(st)
