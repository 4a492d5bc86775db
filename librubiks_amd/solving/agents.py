"""
Search agents whose expand-children loops run on the MI355X (reference: librubiks/solving/agents.py).

`AStar` and `MCTS` keep the reference's constructor arguments, `search(state, time_limit, max_states) -> bool`
protocol, `action_queue`, `len(agent)` and inspection arrays (`states`, `G`, `parents`, `neighbors`, ...), but the
node pool, the state -> index map, the open queue and all per-iteration work live in HBM inside librubiks_hip.so
(engines `rk_astar_*` / `rk_mcts_*` of include/rubiks_hip.h).  The value/policy network stays a PyTorch module:
the engine writes the one-hot batch straight into a torch tensor and reads the net's output from one.

`net` is anything with `.eval()` and `__call__(x, policy=True, value=True)` returning logits (B, 12) and/or a value
(B, 1) for a float32 (B, 480) one-hot batch on `librubiks_amd.gpu` (reference: model.py:131-141).
"""
from __future__ import annotations

import ctypes as C
import time
from collections import deque

import numpy as np
import torch

from librubiks_amd import gpu, no_grad, _ffi
from librubiks_amd import cube
from librubiks_amd.solving import _engine as eng
from librubiks_amd.solving._engine import (  # noqa: F401  (callers import these names from here)
	CAPTURE, NET_SLICE_ROWS, CapacityExhausted, OH_CODES as _OH_CODES, SOLVED20 as _SOLVED20, oh_dtype as _oh_dtype,
	sliced_value_forward as _sliced_value_forward)


class Agent:
	"""Protocol of the reference's agents (agents.py:14-64): one-step agents implement `_step`."""
	eps = np.finfo("float").eps
	_explored_states = 0

	def __init__(self):
		self.action_queue = deque()

	@no_grad
	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		time_limit, max_states = self.reset(time_limit, max_states)
		t0 = time.perf_counter()
		if cube.is_solved(state):
			return True
		solved = False
		while not solved and time.perf_counter() - t0 < time_limit and len(self) < max_states:
			action, state, solved = self._step(state)
			self.action_queue.append(action)
			self._explored_states = len(self.action_queue)
		return solved

	def _step(self, state: np.ndarray):
		"""-> (action index, new state, is solved)"""
		raise NotImplementedError

	def reset(self, time_limit: float, max_states: int):
		self._explored_states = 0
		self.action_queue = deque()
		if hasattr(self, "net"):
			self.net.eval()
		assert time_limit or max_states
		return time_limit or 1e10, max_states or int(1e10)

	def __len__(self):
		return self._explored_states


def _net_signature(net):
	"""Changes whenever the net is swapped or its parameters / buffers are modified in place (optimizer steps,
	load_state_dict, BatchNorm statistics): module identity + training flag + the tensors' storage and version counters.
	Writes through `.data` (`p.data.add_(...)`, the idiom of hand-written update loops) do not bump a tensor's version counter, so
	the signature also carries a checksum of the first floating-point parameter -- the layer the fused form copies -- read at the
	start of a search (one small reduction and one device-to-host wait per search); an update that leaves that one tensor's
	sum unchanged bit for bit and bypasses the version counters of all others is the remaining blind spot."""
	sig = [id(net), bool(getattr(net, "training", False))]
	first = None
	for get in ("parameters", "buffers"):
		it = getattr(net, get, None)
		if callable(it):
			for t in it():
				sig.append((t.data_ptr(), t._version))
				if first is None and t.is_floating_point():
					first = t
	if first is not None:
		sig.append(float(first.detach().double().sum()))
	return tuple(sig)


def _roots20(is2024: bool, states, n: int) -> np.ndarray:
	"""A search's start states as (n, 20) int8 rows; in 6x8x6 mode converted (ValueError for a state that is not a legal cube)."""
	if is2024:
		return np.ascontiguousarray(states, dtype=np.int8).reshape(n, 20)
	return np.ascontiguousarray(cube.as2024(np.asarray(states, dtype=np.int8).reshape(n, 6, 8, 6)))


def _device_rows20(states):
	"""A batch of states as ((n, 20) int8 rows on the device, whether the caller gave a device tensor), in the representation
	cube.get_is2024() names."""
	if cube.cube._is_dev(states):
		t = states if states.dtype == torch.int8 else states.to(torch.int8)
		if cube.get_is2024():
			if t.numel() % 20 or (t.dim() and t.shape[-1] != 20):
				raise ValueError(f"states must be (n, 20), got shape {tuple(t.shape)}")
			q = t.reshape(-1, 20)
			if not q.is_contiguous() or q.data_ptr() % 4:
				q = q.clone(memory_format=torch.contiguous_format)
		else:
			if t.numel() % 288 or (t.dim() and t.shape[-1] != 6):
				raise ValueError(f"states must be (n, 6, 8, 6) in 6x8x6 mode, got shape {tuple(t.shape)}")
			q = cube.as2024(t.reshape(-1, 6, 8, 6))
		return q, True
	rows = cube.cube._rows2024(states)
	return (torch.from_numpy(rows).to(gpu) if len(rows) else torch.empty((0, 20), dtype=torch.int8, device=gpu)), False


def _batch_out(was_device: bool, *tensors):
	"""A batch's answer as the caller gave the states: device tensors, or numpy arrays; one tensor alone, several as a tuple."""
	out = tensors if was_device else tuple(t.cpu().numpy() for t in tensors)
	return out[0] if len(out) == 1 else out


def _states_out(is2024: bool, states20: np.ndarray, n: int) -> np.ndarray:
	"""An exported (rows, 20) array whose rows 1..n hold nodes, in the search's representation (other rows stay zero)."""
	if is2024:
		return states20
	out = np.zeros((len(states20), 6, 8, 6), np.int8)
	if n:
		out[1:n + 1] = cube.as686(states20[1:n + 1])
	return out


class DeepAgent(Agent):
	"""
	An agent with a value/policy net.  `fused_first_layer` (False, True, "epilogue", "folded"; librubiks_amd.oh_linear)
	makes the net's first Linear(480, H) read the engine's 20-byte states; that form COPIES weights (and, folded, BatchNorm
	statistics and the merged heads), while the reference trains its net in place and reassigns `agent.net` during
	training (train.py:134, :214).  So the copy is never trusted blindly: `_from_states` -- read at the start of every
	search -- rebuilds it whenever the net's signature (module identity, training flag, every parameter's and buffer's
	storage and in-place version counter) differs from the one the copy was taken at.
	"""
	def __init__(self, net, fused_first_layer=False):
		super().__init__()
		if fused_first_layer not in (False, None, True, "epilogue", "folded"):
			raise ValueError('fused_first_layer is False, True, "epilogue" or "folded"')
		self._fused_mode = fused_first_layer or False
		self._fused, self._fused_sig = None, None
		self._fs = None                    # `_from_states` as checked at the start of the running search (hot loops use this)
		self._is2024 = True                # the representation of the last search (cube.get_is2024() when it began); its exports follow it
		self._r686 = None                  # the kept 6x8x6 adapter of this agent's net (_Net686), the same object from search to search
		self._n686 = None                  # ... while the running search is in 6x8x6 mode, else None
		self._forward = None               # what the running search evaluates: `_fs`, `_n686` or the net itself (_begin_net)
		self.net = net

	@property
	def net(self):
		return self._net

	@net.setter
	def net(self, net):
		self._net = net                    # the signature holds the module's identity: a swapped net is re-copied at the next search

	@property
	def _from_states(self):
		"""callable(states (n, 20) int8, policy, value) equal to net(as_oh(states), policy, value), or None when not fused."""
		if not self._fused_mode:
			return None
		self._net.eval()
		sig = _net_signature(self._net)
		if self._fused is None or sig != self._fused_sig:
			from librubiks_amd.oh_linear import fused_net
			self._fused, self._fused_sig = fused_net(self._net, self._fused_mode), sig
		return self._fused

	def _begin_repr(self):
		"""Fixes the representation of the search that starts (the reference's agents follow cube.get_is2024()).  In 6x8x6 mode the
		engines still run on 20-byte states and hand the net their rows as RK_OH_STATES; `_n686` turns them into the 6x8x6 one-hot
		the net was trained on (rk_oh686_from2024)."""
		self._is2024 = cube.get_is2024()
		if self._is2024:
			self._n686 = None
			return
		if self._fused_mode:
			raise ValueError("fused_first_layer reads 20-byte states into a Linear(480, H); a net of the 6x8x6 representation has 288 "
			                 "inputs and no fused form")
		if self._r686 is None or self._r686.net is not self._net:
			self._r686 = _Net686(self._net)
		self._n686 = self._r686

	def _begin_net(self):
		"""A search's view of the net, taken when it starts: fixes the representation, re-copies the fused form if the net changed
		since the last search, and returns (forward, reads_states, code): the callable the search evaluates (`self._forward`, which
		the hot loops use), whether it reads the engine's 20-byte rows (the fused copy, the 6x8x6 adapter) rather than a 480-wide
		one-hot, and the RK_OH_* code of the batch the engine is to write for it."""
		self._begin_repr()
		self._fs = self._from_states
		rows_net = self._fs or self._n686      # the net as a function of 20-byte rows, or None
		self._forward = rows_net or self._net
		if rows_net is not None:
			return self._forward, True, _ffi.OH_STATES
		return self._forward, False, _OH_CODES[_oh_dtype(self._net)]

	def _roots20(self, states, n: int) -> np.ndarray:
		return _roots20(self._is2024, states, n)

	def _states_out(self, states20: np.ndarray, n: int) -> np.ndarray:
		return _states_out(self._is2024, states20, n)

	@classmethod
	def from_saved(cls, loc: str, use_best: bool, loader=None):
		"""agents.py:72-76."""
		return cls(_load_net(loc, use_best, loader))


class _Net686:
	"""
	`net(as_oh(6x8x6 form of rows))` for (n, 20) int8 rows: what a net trained on the 6x8x6 representation sees of the engines'
	20-byte states.  One launch (rk_oh686_from2024) writes the one-hot in the net's dtype into a buffer this object keeps, then the
	net runs on it.  The object and its buffers outlive a search, so a captured step that holds their addresses stays valid and a
	second search replays it; a larger batch gets a new buffer and the old ones are kept (a kept graph may still read them).
	"""
	def __init__(self, net):
		self.net = net
		self._bufs = []

	def _buffer(self, n: int, dtype: torch.dtype) -> torch.Tensor:
		for b in reversed(self._bufs):
			if b.dtype == dtype and len(b) >= n:
				return b[:n]
		b = torch.empty((max(n, 64), 288), dtype=dtype, device=gpu)
		self._bufs.append(b)
		return b[:n]

	def __call__(self, rows: torch.Tensor, policy: bool = True, value: bool = True):
		dtype = _oh_dtype(self.net)
		x = self._buffer(len(rows), dtype)
		cube.device.to686(rows, dtype, x)
		return self.net(x, policy=policy, value=value)


def _host_softmax(logits_cpu: torch.Tensor) -> torch.Tensor:
	"""`logits.softmax(dim=1)` of a small CPU tensor on ONE intra-op thread (same kernel, same bits: rows are independent).  torch
	forks its whole thread pool even for twelve rows; on a host whose CPU share is a fraction of its thread count the pool's threads
	spin after every call and starve the thread that launches GPU work (measured: 3.3 ms per MCTS simulation instead of 0.29)."""
	threads = torch.get_num_threads()
	if threads != 1:
		torch.set_num_threads(1)
	try:
		return logits_cpu.softmax(dim=1)
	finally:
		if threads != 1:
			torch.set_num_threads(threads)


class RandomSearch(Agent):
	"""Random walk (agents.py:82-89)."""
	def _step(self, state):
		action = np.random.randint(cube.action_dim)
		state = cube.rotate(state, *cube.action_space[action])
		return action, state, cube.is_solved(state)

	def __str__(self):
		return "Random depth-first search"


class BFS(Agent):
	"""Breadth-first search over the 12-move graph (agents.py:92-129).  The reference pops one state at a time and moves it
	twelve times; here the children of up to `chunk` queued states come from ONE fan-out launch (with the goal test), and the
	reference's loop -- same order, same checks before every pop -- then runs over them, so `states`, the action queue and
	len(agent) are the reference's."""
	states = dict()
	chunk = 16_384                          # queued states expanded per launch (their 12 x chunk children are held on the host)

	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		time_limit, max_states = self.reset(time_limit, max_states)
		t0 = time.perf_counter()
		self.states = {}
		if cube.is_solved(state):
			return True
		self.states = {state.tobytes(): (None, None)}          # state -> (predecessor key, action)
		queue = deque([np.ascontiguousarray(state, dtype=np.int8)])
		while queue and time.perf_counter() - t0 < time_limit and len(self) < max_states:
			# the states that will be popped next, in order; a first-in-first-out queue only ever grows at the far end, so the
			# children of its head do not depend on what the loop below appends
			head = [queue[i] for i in range(min(len(queue), self.chunk, max(1, (max_states - len(self)) // 11 + 1)))]
			children, solved = cube.expand(np.array(head), return_solved=True)
			for j in range(len(head)):
				if not (time.perf_counter() - t0 < time_limit and len(self) < max_states):      # agents.py:105, before every pop
					return False
				pkey = queue.popleft().tobytes()
				for a in range(cube.action_dim):
					child = children[12 * j + a]
					ckey = child.tobytes()
					if ckey in self.states:
						continue
					if solved[12 * j + a]:
						self.action_queue.appendleft(a)
						while self.states[pkey][0] is not None:
							pkey, act = self.states[pkey]
							self.action_queue.appendleft(act)
						return True
					self.states[ckey] = (pkey, a)
					queue.append(child.copy())                      # (a view would keep the whole launch's children alive)
		return False

	def __str__(self):
		return "Breadth-first search"

	def __len__(self):
		return len(self.states)


class _PoolSearch(Agent, _ffi.Owner):
	"""What the agents that drive a frontier pool share -- `DeviceBFS`, `DeviceBiBFS` and the searches that end at a
	kept ball: the arguments and their checks, the engine that is kept between searches, the pool growth, the host loop of a
	search and the export of the pool.  A subclass names its engine and maps the status words that are its own."""
	default_capacity = 8_000_000
	max_capacity = 400_000_000
	MAX_POPS = 1 << 22                      # the limit of every rk_*_create
	MAX_CAPACITY = 0x3FFFFFF0
	_entries = None                         # the prefix of the engine's entry points
	_status_words = 8                       # what its *_status writes
	_first_nodes = 1                        # nodes a reset stores (they have no parent)
	_unlimited = False                      # a search may run without either limit (an exact search)
	_engine_name = None                     # in the text of an engine error

	def __init__(self, pops: int = 16_384, capacity: int = None, max_capacity: int = None, poll: int = 8):
		super().__init__()
		self.pops = eng.int_in("pops", pops, 1, self.MAX_POPS)
		self.capacity = eng.int_in("capacity", capacity, 2, self.MAX_CAPACITY, none_ok=True)
		if eng.int_in("max_capacity", max_capacity, 2, self.MAX_CAPACITY, none_ok=True) is not None:
			self.max_capacity = int(max_capacity)
		self.poll = eng.int_in("poll", poll, 1, what="a positive integer")
		self._h, self._h_cap = None, 0
		self._n = 0
		self._is2024 = True
		self._cache = None
		self.iterations = 0
		self.popped = 0                     # nodes the last search popped (each has 12 children)
		self.grown = 0
		self.capacity_exhausted = False

	def _entry(self, name: str):
		return getattr(_ffi.lib(), f"{self._entries}_{name}")

	def _create_args(self) -> tuple:
		"""What the engine's create takes before the capacity and the pops."""
		return ()

	def _engine(self, capacity: int):
		if self._h is not None and self._h_cap >= capacity:
			return self._h                  # (a pool that grew in an earlier search is kept: the reset clears its table)
		self._h_cap = capacity
		return self._create(f"{self._entries}_create", f"{self._entries}_destroy", *self._create_args(), capacity, self.pops)

	def _grow(self, h) -> bool:
		if self._h_cap >= self.max_capacity:
			eng.pool_exhausted(self, self._h_cap, "cannot take the next iteration")
			return False
		cap = min(2 * self._h_cap, self.max_capacity)
		_ffi.check(self._entry("grow")(h, cap, _ffi.stream_ptr()))
		self._h_cap = cap
		self.grown += 1
		return True

	def _fewer_pops(self, h, pops: int) -> int:
		"""A pool that cannot grow: a lower pop count (< `pops`) for the iterations to come, told to the engine, or 0 to give up."""
		return 0

	def _pool_full(self, h, t0: float, time_limit: float) -> bool:
		"""What `search` returns once the pool takes no more pops: an engine that can go on without a pool does so here."""
		return False

	def _begin(self, root: np.ndarray) -> bool:
		"""Before the engine is touched: clears the subclass's results; True when `root` needs no search."""
		raise NotImplementedError

	def _read(self, status):
		"""The status words beyond states and iterations, to their attributes."""
		raise NotImplementedError

	@no_grad
	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		_ffi.require_gpu()
		t0 = time.perf_counter()
		time_limit, max_states = self.reset(time_limit or 1e10 if self._unlimited else time_limit, max_states)
		self._n, self._cache, self.iterations, self.grown, self.capacity_exhausted = 0, None, 0, 0, False
		self.popped = 0
		self._is2024 = cube.get_is2024()
		root = _roots20(self._is2024, state, 1)[0]          # ValueError for an illegal 6x8x6 state
		if self._begin(root):
			return True
		stream = _ffi.stream_ptr()
		run, read_status = self._entry("run"), self._entry("status")
		K = 12 * self.pops
		budget = int(min(max_states, 2 ** 31 - 1))
		cap = self.capacity or min(budget + K, self.default_capacity)
		cap = max(2, min(cap, self.max_capacity, self.MAX_CAPACITY))
		h = self._engine(cap)
		_ffi.check(self._entry("reset")(h, root.ctypes.data, budget, stream))
		self._n = self._first_nodes
		status = (C.c_longlong * self._status_words)()
		_ffi.check(read_status(h, status, stream))
		self._read(status)                                   # (a start that is answered at once: done, with its meeting)
		while not status[0]:
			room = (self._h_cap - self._n) // K              # iterations the pool takes whatever they find
			if room == 0:
				if self._grow(h):
					continue
				fewer = self._fewer_pops(h, K // 12)
				if not fewer:
					return self._pool_full(h, t0, time_limit)
				K = 12 * fewer
				continue
			_ffi.check(run(h, eng.burst(min(self.poll, room), budget - self._n, K), stream))
			_ffi.check(read_status(h, status, stream))
			self._n, self.iterations = int(status[2]), int(status[3])
			self._read(status)
			if status[6]:
				raise _ffi.RubiksHipError(f"{self._engine_name} engine error code {int(status[6])}")
			if not status[0] and time.perf_counter() - t0 >= time_limit:
				return False
		if status[1]:
			self.action_queue = eng.read_path(self._entry("path"), h)
			return True
		return False

	def _pool(self, tags: bool = False) -> tuple:
		"""arrays() of the pool: rows 1 .. len(agent), the states in the search's representation."""
		if self._cache is None:
			n = self._n
			states, *cols = eng.export_frontier(self._entry("export") if self._h is not None else None, (self._h,), n, self._first_nodes, tags)
			self._cache = (_states_out(self._is2024, states, n)[1:], *(c[1:] for c in cols))
		return self._cache

	def arrays(self):
		"""(states, parents, actions) of the pool's nodes 1 .. len(agent) in index order, as `DeviceBFS.arrays()`."""
		return self._pool()

	def __len__(self):
		return self._n


class DeviceBFS(_PoolSearch):
	"""
	Breadth-first search (agents.py:92-129) with the whole search in HBM (engine rk_bfs_*, csrc/rk_bfs.hip): the node pool, the
	parent and action of every node, and a hash table of the states seen.  The FIFO queue is the pool in index order.  One
	iteration pops up to `pops` queued nodes, fans out their 12 children, tests them against the table, stores the first
	occurrences of new states in order and applies the reference's stopping rules exactly: the state budget before every pop
	(:105) and the return of the first solved child before it is stored (:111-118).  So the pool, len(agent) and the action
	queue are the reference's, without a host round trip per child.  The host polls every `poll` iterations; the time limit is
	checked there, not before every pop, so a time-limited search does not stop where the reference would.

	`capacity` is the pool size a search starts with (default: what the budget needs, at most `default_capacity`).  Before an
	iteration whose children might not fit, the pool doubles in place (rk_bfs_grow) up to `max_capacity`; at `max_capacity` the
	search warns with `CapacityExhausted`, sets `capacity_exhausted` and returns False.  `grown` counts the growths.

	The representation follows cube.get_is2024() when a search starts; the engine always runs on 20-byte states (the two forms
	map one to one under the same moves), so `states` and `arrays()` convert on the way out.
	"""
	_entries = "rk_bfs"
	_engine_name = "BFS"

	def __init__(self, pops: int = 16_384, capacity: int = None, max_capacity: int = None, poll: int = 8):
		super().__init__(pops, capacity, max_capacity, poll)

	def _begin(self, root) -> bool:
		return bool((root == _SOLVED20).all())

	def _read(self, status):
		self.popped = int(status[4]) - 1                    # word 4 is the head of the queue: the nodes before it were popped

	def arrays(self):
		"""(states, parents, actions) of nodes 1 .. len(agent) in index order = the reference's dict in insertion order: states
		(n, 20) int8, or (n, 6, 8, 6) in 6x8x6 mode; parents int64 node indices (0 for the start); actions int64 (-1 for the start)."""
		return self._pool()

	@property
	def states(self) -> dict:
		"""The reference's `self.states` (agents.py:103, :120): state bytes -> (predecessor bytes, action), (None, None) for the
		start, in insertion order.  Built on the host from arrays(): meant for small searches."""
		states, parents, actions = self.arrays()
		keys = [s.tobytes() for s in states]
		return {k: (None, None) if p == 0 else (keys[p - 1], int(a)) for k, p, a in zip(keys, parents.tolist(), actions.tolist())}

	def __str__(self):
		return f"Breadth-first search (device, pops={self.pops})"


class DeviceBiBFS(_PoolSearch):
	"""
	Two-sided breadth-first search with the whole search in HBM (engine rk_bibfs_*, csrc/rk_bibfs.hip): a SHORTEST solution in
	the quarter-turn metric.  One pool in index order holds two balls, side S around the start (node 1) and side G around the
	solved state (node 2); they grow one level at a time, S when both have as many complete levels, else G.  A level's parents
	are popped in index order, their children taken in action order: a child its own side holds is skipped, a child the other
	side holds is the meeting (the search ends, the child is not stored), any other is appended.  With `f` and `b` complete
	levels every solution has at least f + b + 1 moves and a meeting in the next level has exactly that many, so the first
	meeting is optimal.  The state budget is checked before every pop, as in `DeviceBFS`; the time limit when the host polls
	(every `poll` iterations).  `action_queue`, len(agent), the pool and `depths` do not depend on `pops`.

	`capacity`, `max_capacity`, `grown` and `capacity_exhausted` are `DeviceBFS`'s, for the pool of both sides together.  The
	representation follows cube.get_is2024() when a search starts; the engine always runs on 20-byte states.
	"""
	_entries = "rk_bibfs"
	_status_words = 12
	_first_nodes = 2
	_unlimited = True
	_engine_name = "two-sided BFS"

	def __init__(self, pops: int = 16_384, capacity: int = None, max_capacity: int = None, poll: int = 8):
		super().__init__(pops, capacity, max_capacity, poll)
		self._meet = 0                      # the stored node that the meeting child equals
		self.depths = (0, 0)                # complete levels (f, b) of sides S and G after the last search

	def _begin(self, root) -> bool:
		self._meet, self.depths = 0, (0, 0)
		return bool((root == _SOLVED20).all())

	def _read(self, status):
		self.popped = int(status[4])                         # both sides together
		self.depths, self._meet = (int(status[8]), int(status[9])), int(status[10])

	def arrays(self):
		"""(states, parents, actions, sides) of nodes 1 .. len(agent) in index order: states (n, 20) int8, or (n, 6, 8, 6) in 6x8x6
		mode; parents int64 node indices (0 for nodes 1 and 2); actions int64, the move from the parent -- on side G away from
		solved -- (-1 for nodes 1 and 2); sides int64, 0 = around the start, 1 = around the solved state."""
		return self._pool(tags=True)

	@property
	def meeting(self):
		"""The state where the sides met -- the child that was not stored, held by the other side -- in the representation of the
		search; None when the last search did not meet."""
		if not self._meet:
			return None
		return self.arrays()[0][self._meet - 1].copy()

	def __str__(self):
		return f"Two-sided breadth-first search (device, pops={self.pops})"


def _words_of(ranks: np.ndarray, extra: int, last: np.ndarray) -> np.ndarray:
	"""int64 (n, extra): word `ranks[i]` of `extra` moves behind the action `last[i]` (-1: none), rk_sdeepen's numbering: digit k of
	the rank counts the allowed actions below action k, the opposite turn of the action before it left out."""
	rem, prev = np.array(ranks, np.int64), np.array(last, np.int64)
	out = np.empty((len(rem), extra), np.int64)
	for k in range(extra):
		d, rem = np.divmod(rem, 11 ** (extra - 1 - k))
		out[:, k] = prev = np.where(prev < 0, d, d + (d >= (prev ^ 1)))
	return out


class _KeptBall(_ffi.Owner):
	"""What `DeviceGoalBall` and `DeviceSymBall` share: a ball around the solved state that is built once, at first use, and
	read-only from then on, its level boundaries, and the one-launch answers `depth` and `solve`.  `_entries` is the prefix of the
	engine's entry points, `_status_words` what its status writes."""
	MAX_POPS = 1 << 22                      # the limit of rk_ball_create and rk_symball_create
	poll = 8                                # iterations of the build between two looks of the host
	_entries = None
	_status_words = 16

	def __init__(self, radius: int, pops: int):
		self.radius = eng.int_in("radius", radius, 0, self.MAX_RADIUS)
		self.pops = eng.int_in("pops", pops, 1, self.MAX_POPS)
		self._h = None
		self._n = 0
		self._level_start = None
		self._cache = {}
		self.iterations = 0                 # of the build

	def _entry(self, name: str):
		return getattr(_ffi.lib(), f"{self._entries}_{name}")

	def _create_args(self) -> tuple:
		"""What the engine's create takes behind the radius and the pops."""
		return ()

	def _built(self, status):
		"""The status words of a built ball that are the subclass's own."""

	@property
	def built(self) -> bool:
		return self._level_start is not None

	def build(self):
		"""Builds the ball on the device (nothing if it is built)."""
		if self.built:
			return self
		_ffi.require_gpu()
		if self._h is None:
			self._create(f"{self._entries}_create", f"{self._entries}_destroy", self.radius, self.pops, *self._create_args())
		_ffi.check(self._entry("build")(self._h, self.poll, _ffi.stream_ptr()))
		status = (C.c_longlong * self._status_words)()
		_ffi.check(self._entry("status")(self._h, status))
		self._n, self.iterations = int(status[1]), int(status[2])
		self._built(status)
		self._level_start = np.array(status[6:6 + self.radius + 2], np.int64)
		return self

	@property
	def level_start(self) -> np.ndarray:
		"""int64 (radius + 2,): level l holds the nodes level_start[l] .. level_start[l + 1] - 1."""
		return self.build()._level_start

	def __len__(self):
		return self.build()._n

	def _rows(self, states) -> np.ndarray:
		"""Query states in the current representation as (n, 20) int8 rows (ValueError for an illegal 6x8x6 state)."""
		raise NotImplementedError

	def depth(self, states) -> np.ndarray:
		"""int64 (n,): the exact distance to solved of every state the ball holds (`DeviceSymBall`: whose orbit it holds), -1 for
		the others.  One launch."""
		self.build()
		rows = self._rows(states)
		if len(rows) == 0:
			return np.zeros(0, np.int64)
		return self._depth_of(torch.from_numpy(rows).to(gpu))

	def _depth_of(self, q: torch.Tensor) -> np.ndarray:
		"""`depth` of (n, 20) rows on the device, n > 0."""
		n = len(q)
		out = torch.empty(n, dtype=torch.int32, device=gpu)
		_ffi.check(self._entry("depth")(self._h, q.data_ptr(), n, out.data_ptr(), _ffi.stream_ptr()))
		return out.cpu().numpy().astype(np.int64)

	def _solve(self, q, n: int, lengths, actions):
		"""The engine's solve launch on device tensors."""
		_ffi.check(self._entry("solve")(self._h, q.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(), _ffi.stream_ptr()))

	def solve(self, states):
		"""(lengths int64 (n,), actions int64 (n, radius)): a shortest solution of every state the ball holds (`DeviceSymBall`: whose
		orbit it holds, at each step the lowest action that gets one level nearer), rows padded with -1; length -1 for a state
		outside the ball.  One launch."""
		self.build()
		rows = self._rows(states)
		if len(rows) == 0:
			return np.zeros(0, np.int64), np.zeros((0, self.radius), np.int64)
		return self._solve_of(torch.from_numpy(rows).to(gpu))

	def _solve_of(self, q: torch.Tensor):
		"""`solve` of (n, 20) rows on the device, n > 0."""
		n = len(q)
		lengths = torch.empty(n, dtype=torch.int32, device=gpu)
		actions = torch.empty((n, max(self.radius, 1)), dtype=torch.int8, device=gpu)
		self._solve(q, n, lengths, actions)
		return lengths.cpu().numpy().astype(np.int64), actions.cpu().numpy().astype(np.int64)[:, :self.radius]

	def _relative(self, a, b, check: bool):
		"""(n, 20) rows on the device: a[i] seen from b[i] (`b`: one state or n), in the representation cube.get_is2024() names;
		None for no rows.  The rows stay on the device: what reads them next is the ball's own launch."""
		self.build()
		rows, goals = self._rows(a), self._rows(b)
		if len(goals) not in (1, len(rows)):
			raise ValueError(f"b must be one state or one for each of the {len(rows)} states of a, got {len(goals)}")
		if len(rows) == 0:
			return None
		q = torch.from_numpy(rows).to(gpu)
		return cube.device.relative(q, torch.from_numpy(goals).to(gpu), out=q, check=check)

	def distance(self, a, b, check: bool = True) -> np.ndarray:
		"""int64 (n,): the exact number of quarter turns from a[i] to b[i] (`b`: one state or n) where the ball holds it, -1 elsewhere:
		`depth` of `cube.relative(a, b)`, the relative states made on the device and read there by the depth launch.  `check`:
		ValueError for a row that is no legal cube state (`cube.device.relative`)."""
		q = self._relative(a, b, check)
		return np.zeros(0, np.int64) if q is None else self._depth_of(q)

	def path(self, a, b, check: bool = True):
		"""(lengths int64 (n,), actions int64 (n, radius)) shaped like `solve`'s: a shortest sequence of moves that turns a[i] into
		b[i] (`b`: one state or n), length -1 where the two are further apart than the ball reaches: `solve` of
		`cube.relative(a, b)`, made and read on the device."""
		q = self._relative(a, b, check)
		return (np.zeros(0, np.int64), np.zeros((0, self.radius), np.int64)) if q is None else self._solve_of(q)

	MAX_QUEUE = 4096                        # the longest queue of rk_bshorten and rk_sshorten
	shorten_scratch_bytes = 256 << 20       # the most scratch one call of the engine is given; a batch is cut into calls to fit
	_shorten_entry = None                   # the engine's shortening entry

	def _shorten(self, *args):
		"""The engine's shortening pass on device pointers: what follows the handle in rk_bshorten's argument list."""
		_ffi.check(getattr(_ffi.lib(), self._shorten_entry)(self._h, *args))

	def shorten(self, action_queues, window: int = None, passes: int = None) -> list:
		"""
		Every action queue (a sequence of actions 0..11, at most 4096 of them; any agent's solution) made locally optimal against
		the ball, on the device (engine rk_bshorten_* for `DeviceGoalBall`, rk_sshorten for `DeviceSymBall`): a list of int64 arrays,
		each no longer than its queue and with the same effect on any state.  Neither start states nor a net are needed: the moves
		i .. j-1 of a queue, applied to the solved state, give a state whose ball depth is the distance between the queue's states i
		and j, so every window of at most `window` moves is looked up in the ball, and the best set of replacements by the ball's own
		words is a shortest path through a small DAG.  A pass runs on all queues, further passes on those that
		got shorter, until none does or `passes` passes are done.  Then every window of at most `window` moves whose net effect the
		ball holds has exactly that state's depth in moves.  `window=None`: every window of every queue.

		Which word a replaced window gets depends on the ball; its length does not.  `DeviceGoalBall`: the ball's stored word for the
		window's net effect X, the stored actions from node 1 down to X's node.  `DeviceSymBall`: the inverse of the descent -- `solve`'s
		word for X (at each step the lowest action whose child lies one level nearer) reversed, every action replaced by its
		opposite turn.  Both lead from solved to X, so a pass of either ball over the same queues gives equal lengths at equal radius,
		queue for queue, and the same states; the symmetry ball does it from 1/60 of the memory, and at radius 9 and 10 as well.
		(Later passes start from words that may differ where a window has several shortest words, so the two fixed points of a
		narrow window -- both locally optimal -- need not have equal lengths in every queue.)
		"""
		queues = [np.asarray(q, dtype=np.int64).reshape(-1) for q in action_queues]
		eng.int_in("window", window, 1, none_ok=True, what="an integer >= 1 or None")
		eng.int_in("passes", passes, 0, none_ok=True, what="an integer >= 0 or None")
		for q in queues:
			if len(q) > self.MAX_QUEUE:
				raise ValueError(f"an action queue of {len(q)} moves: at most {self.MAX_QUEUE}")
			if len(q) and not (0 <= q.min() and q.max() < 12):
				raise ValueError("actions must be in 0..11")
		self.build()
		lib, stream = _ffi.lib(), _ffi.stream_ptr()
		active = [i for i, q in enumerate(queues) if len(q)]
		done = 0
		while active and (passes is None or done < passes):
			longest = max(len(queues[i]) for i in active)
			w = longest if window is None else min(int(window), longest)
			per_queue = longest * w + 2 * (longest + 1)
			step = max(1, self.shorten_scratch_bytes // per_queue)
			shorter = []
			for at in range(0, len(active), step):
				part = active[at:at + step]
				n = len(part)
				max_len = max(len(queues[i]) for i in part)
				wc = max_len if window is None else min(int(window), max_len)
				acts = np.full((n, max_len), -1, np.int8)
				for r, i in enumerate(part):
					acts[r, :len(queues[i])] = queues[i]
				lens = np.array([len(queues[i]) for i in part], np.int32)
				need = lib.rk_bshorten_scratch_bytes(n, max_len, wc)
				if need < 0:
					_ffi.check(need)
				d_acts, d_lens = torch.from_numpy(acts).to(gpu), torch.from_numpy(lens).to(gpu)
				d_out = torch.empty((n, max_len), dtype=torch.int8, device=gpu)
				d_out_len = torch.empty(n, dtype=torch.int32, device=gpu)
				d_err = torch.empty(1, dtype=torch.int32, device=gpu)
				scratch = torch.empty(need, dtype=torch.uint8, device=gpu)
				self._shorten(d_acts.data_ptr(), d_lens.data_ptr(), n, max_len, wc, d_out.data_ptr(), d_out_len.data_ptr(), d_err.data_ptr(),
				              scratch.data_ptr(), need, stream)
				out, out_len, err = d_out.cpu().numpy(), d_out_len.cpu().numpy(), int(d_err.item())
				if err:
					raise _ffi.RubiksHipError(f"{self._shorten_entry} reported error {err} for queues that passed the host's checks")
				for r, i in enumerate(part):
					if out_len[r] < len(queues[i]):
						shorter.append(i)
					queues[i] = out[r, :out_len[r]].astype(np.int64)
			active = [i for i in shorter if len(queues[i])]
			done += 1
		return queues

	def depth_of_node(self, node: int) -> int:
		"""The depth of node `node` (1 .. len(ball)), from the level boundaries."""
		return int(np.searchsorted(self.level_start, node, side="right")) - 1


class DeviceGoalBall(_KeptBall):
	"""
	The ball around the solved state, built once and kept in HBM (engine rk_ball_*, csrc/rk_ball.hip): every state within `radius`
	quarter turns, in `DeviceBFS`'s order without goal test or budget.  Node 1 is the solved state; a level's parents are popped in
	index order, their children taken in action order, a child the pool holds is skipped, any other appended with its parent and
	its action (the move away from solved).  Level `radius` is stored and never expanded.  Level l is the index range
	`level_start[l] .. level_start[l + 1] - 1`, so depths come from indices.  The pool does not depend on `pops`.

	The ball is built at first use (or by `build()`) and read-only from then on: `depth` and `solve` answer a batch of states in
	one launch each, and any number of `DeviceBallSearch` agents may share it.  States are in the representation cube.get_is2024()
	names when a method is called.  Radius 8 holds 86.0 M states in about 3.2 GB.
	"""
	LEVELS = (1, 12, 114, 1_068, 10_011, 93_840, 878_880, 8_221_632, 76_843_595)    # states at distance 0 .. 8, quarter turns
	MAX_RADIUS = len(LEVELS) - 1
	_entries = "rk_ball"
	_shorten_entry = "rk_bshorten"          # a replaced window gets the stored actions from node 1 down to the window's node

	def __init__(self, radius: int, pops: int = 16_384):
		super().__init__(radius, pops)

	def _rows(self, states) -> np.ndarray:
		is2024 = cube.get_is2024()
		arr = np.asarray(states, dtype=np.int8)
		width = 20 if is2024 else 288
		if arr.size % width or (arr.ndim and arr.shape[-1] != (20 if is2024 else 6)):
			raise ValueError(f"states must be (n, 20), or (n, 6, 8, 6) in 6x8x6 mode, got shape {arr.shape}")
		return _roots20(is2024, arr, arr.size // width)

	def arrays(self):
		"""(states, parents, actions) of nodes 1 .. len(ball) in index order, like `DeviceBFS.arrays()`: parent 0 and action -1 for
		the solved state; an action is the move from the parent, away from solved."""
		is2024 = cube.get_is2024()
		if is2024 not in self._cache:
			n = len(self)
			states, parents, actions = eng.export_frontier(_ffi.lib().rk_ball_export, (self._h,), n)
			self._cache = {is2024: (_states_out(is2024, states, n)[1:], parents[1:], actions[1:])}
		return self._cache[is2024]

	def __str__(self):
		return f"Goal ball (device, radius={self.radius})"


class DeviceSymBall(_KeptBall):
	"""
	The goal ball reduced by the 48 whole-cube symmetries (engine rk_symball_*, csrc/rk_sym.hip): one canonical representative
	(`cube.canonical`) per orbit of the states within `radius` quarter turns of solved.  Conjugation keeps the distance to solved,
	so a representative's depth is the depth of the up to 48 states of its orbit; nearly every orbit has 48.  Node 1 is the solved
	state; a level's representatives are popped in index order, their children taken in action order and canonicalised, a
	representative the pool holds is skipped, any other appended.  Level l is the index range `level_start[l] ..
	level_start[l + 1] - 1`.  The pool holds states only -- no parents, no actions: `solve` descends, at each step the lowest
	action whose child lies one level nearer.  The pool does not depend on `pops`.

	`shorten` makes action queues locally optimal against this ball as `DeviceGoalBall.shorten` does against the plain one, a pass
	giving the same lengths at the same radius -- radius 8 from about 53 MB instead of 3.2 GB -- and windows whose net effect lies 9
	or 10 quarter turns from solved at radius 9 or 10.  With no stored word, a replaced window gets the inverse of the descent (`solve`'s
	word for the window's net effect, reversed, every turn the opposite one).

	`capacity` is the number of orbits the pool can hold (None: the sum over the levels of ceil(level size / 48 * 1.02) + 64);
	a build that does not fit stops cleanly with a RubiksHipError (RK_ECAPACITY).  `states_covered[l]` is the sum of the orbit
	sizes of level l: the number of states of the plain ball's level (checked by the engine for levels 0..8).  States are in the
	representation cube.get_is2024() names when a method is called.

	The ball also hands out states: `state_at(depths, ranks)` unranks it -- rank r of level d is one of the `states_covered[d]`
	states at distance exactly d, each exactly once --, `sample` draws uniform ranks, and `child_depths` gives the exact depth of a
	state and of its twelve children within radius + 1.  The first `state_at` adds an orbit index of one byte per orbit and eight
	bytes per 256 orbits to the ball's memory (`index_bytes`, shown by `str(ball)` once it exists).
	"""
	LEVELS = DeviceGoalBall.LEVELS                                  # states at distance 0 .. 8: what states_covered is checked against
	MAX_RADIUS = 10
	MAX_CAPACITY = 0x3FFFFFF0
	_entries = "rk_symball"
	_status_words = 32
	_shorten_entry = "rk_sshorten"          # a replaced window gets the inverse of the descent from the window's net effect

	def __init__(self, radius: int, pops: int = 16_384, capacity: int = None):
		super().__init__(radius, pops)
		self.capacity = eng.int_in("capacity", capacity, 1, self.MAX_CAPACITY, none_ok=True, what=f"an integer in 1..{self.MAX_CAPACITY} or None")
		self._covered = None

	def _create_args(self) -> tuple:
		return (self.capacity or 0,)

	def _built(self, status):
		self.capacity = int(status[4])
		self._covered = np.array(status[18:18 + self.radius + 1], np.int64)

	@property
	def states_covered(self) -> np.ndarray:
		"""int64 (radius + 1,): the orbit sizes of every level added up = the states at that distance from solved."""
		return self.build()._covered

	def _rows(self, states) -> np.ndarray:
		return cube.cube._rows2024(states)

	def _solve(self, q, n: int, lengths, actions):
		err = torch.empty(1, dtype=torch.int32, device=gpu)
		_ffi.check(_ffi.lib().rk_symball_solve(self._h, q.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(), err.data_ptr(),
		                                       _ffi.stream_ptr()))
		if int(err.item()):
			raise _ffi.RubiksHipError(f"rk_symball_solve reported error {int(err.item())}: a state of the ball has no child one level nearer")

	MAX_EXTRA = 8                           # the longest word of rk_sdeepen
	deepen_cap = None                       # probes per launch (None: rk_sdeepen_max_probes()); tests lower it to split a round

	def _launch_cap(self) -> int:
		most = int(_ffi.lib().rk_sdeepen_max_probes())
		return most if self.deepen_cap is None else eng.int_in("deepen_cap", self.deepen_cap, 1, most)

	probes = 0                              # after solve_beyond / distance / path with extra: the words issued ...
	lookups = 0                             # ... and the ball look-ups made (fewer with `prune`)

	def solve_beyond(self, states, extra: int, last_actions=None, time_limit: float = None, prune=None):
		"""
		(lengths int64 (n,), actions int64 (n, extra + radius)), rows padded with -1: shortest solutions past the radius by depth-first
		probes (engine rk_sdeepen).  A state whose orbit the ball holds gets what `solve` gives.  The others run rounds
		e = 1 .. `extra`, each on the still unanswered states only: every word of e moves is applied to the state and the result
		looked up in the ball.  In the first round with a hit the answer is the state's lowest word in lexicographic order of its
		actions, then `solve`'s descent from the moved state; its length e + radius is the distance to solved.  Length -1: no hit
		within `extra` moves (or within `time_limit` seconds, checked between launches).  `extra` = 0 is `solve`.

		`last_actions` (n,) names the move that led to each state, -1 for none: words that begin with its opposite turn are not
		tried.  That is right when the state before that move is known to be no nearer to the ball -- a search's parent --; a
		caller that cannot say so passes None.  States are in the representation cube.get_is2024() names.

		`prune` (a `DevicePatternBound`, or a list of 1..4 `DevicePatternDB` that is wrapped into one) leaves out look-ups that
		cannot hit (engine rk_sdeepen_pruned).  With R the radius, a word of e moves that hits leads into the ball, so the state
		after k of its moves is at most (e - k) + R from solved and its admissible bound is no greater: a state whose bound is
		greater than R + (e - k) has no hit behind it, and every word through it is dropped.  No prefix of a hit word is ever
		dropped, so the answers -- lengths and actions -- are those of the unpruned call, bit for bit.  Afterwards `probes` is the
		words issued and `lookups` the ball look-ups made (equal without `prune`).
		"""
		extra = eng.int_in("extra", extra, 0, self.MAX_EXTRA)
		prune = DevicePatternBound.of(prune)
		self.build()
		rows = self._rows(states)
		return self._solve_beyond_of(torch.from_numpy(rows).to(gpu) if len(rows) else None, len(rows), extra, last_actions, time_limit, prune)

	def _solve_beyond_of(self, q, n: int, extra: int, last_actions=None, time_limit: float = None, prune=None):
		"""`solve_beyond` of (n, 20) rows on the device (None for n = 0), `extra` checked, `prune` a usable DevicePatternBound or None."""
		self.probes = self.lookups = 0
		width = extra + self.radius
		last = None
		if last_actions is not None:
			last = np.asarray(last_actions, dtype=np.int64).reshape(-1)
			if len(last) != n or (n and not (-1 <= last.min() and last.max() < 12)):
				raise ValueError("last_actions must be n actions in 0..11, or -1 for none")
		lengths, actions = np.full(n, -1, np.int64), np.full((n, width), -1, np.int64)
		if n == 0:
			return lengths, actions
		t0 = time.perf_counter()
		got = torch.empty(n, dtype=torch.int32, device=gpu)
		word = torch.empty((n, max(self.radius, 1)), dtype=torch.int8, device=gpu)
		self._solve(q, n, got, word)
		lengths[:] = got.cpu().numpy()
		actions[:, :self.radius] = word.cpu().numpy()[:, :self.radius]
		todo = np.nonzero(lengths < 0)[0]
		looked = None if prune is None else torch.zeros(1, dtype=torch.int64, device=gpu)
		try:
			self._deepen_rounds(q, extra, last, time_limit, prune, looked, t0, todo, lengths, actions, word)
		finally:
			self.lookups = self.probes if looked is None else int(looked.item())
		return lengths, actions

	def _deepen_rounds(self, q, extra, last, time_limit, prune, looked, t0, todo, lengths, actions, word):
		"""The rounds of `_solve_beyond_of` on the unanswered rows `todo`; fills `lengths` and `actions`, counts `probes`."""
		lib, stream, cap = _ffi.lib(), _ffi.stream_ptr(), self._launch_cap()
		for e in range(1, extra + 1):
			m = len(todo)
			if m == 0:
				break
			sub = q[torch.from_numpy(todo).to(gpu)].contiguous()
			sub_last = None if last is None else last[todo]
			d_last = None if last is None else torch.from_numpy(sub_last.astype(np.int8)).to(gpu)
			words = (12 if last is None or (sub_last < 0).any() else 11) * 11 ** (e - 1)
			best = torch.full((m,), -1, dtype=torch.int32, device=gpu)      # 0xFFFFFFFF: no hit
			per = max(1, min(m, cap // words))                              # states per launch; a state's words in ranges of <= cap
			for at in range(0, m, per):
				cnt = min(per, m - at)
				step = min(words, cap // cnt)
				for first in range(0, words, step):
					args = (sub[at:].data_ptr(), None if d_last is None else d_last[at:].data_ptr(), cnt, e, first, min(step, words - first),
					        best[at:].data_ptr())
					if prune is None:
						_ffi.check(lib.rk_sdeepen(self._h, *args, stream))
					else:
						_ffi.check(lib.rk_sdeepen_pruned(self._h, prune._h, *args, looked.data_ptr(), stream))
					self.probes += cnt * min(step, words - first)
					if time_limit is not None:
						torch.cuda.current_stream().synchronize()
						if time.perf_counter() - t0 >= time_limit:
							return
			rank = best.cpu().numpy().view(np.uint32).astype(np.int64)
			hit = np.nonzero(rank != 0xFFFFFFFF)[0]
			if len(hit):
				moves = _words_of(rank[hit], e, -np.ones(len(hit), np.int64) if last is None else sub_last[hit])
				moved = sub[torch.from_numpy(hit).to(gpu)].contiguous()
				for k in range(e):                                          # the hit states moved along their words, on the device
					a = torch.from_numpy(moves[:, k].astype(np.uint8)).to(gpu)
					_ffi.check(lib.rk_multi_rotate(_ffi.REPR_2024, moved.data_ptr(), a.data_ptr(), moved.data_ptr(), len(hit), stream))
				got = torch.empty(len(hit), dtype=torch.int32, device=gpu)
				self._solve(moved, len(hit), got, word)
				down = got.cpu().numpy().astype(np.int64)
				if (down != self.radius).any():
					raise _ffi.RubiksHipError("rk_sdeepen reported a hit that does not lie at the ball's radius")
				lengths[todo[hit]] = e + down
				actions[todo[hit], :e] = moves
				actions[todo[hit], e:e + self.radius] = word.cpu().numpy()[:len(hit), :self.radius]
			todo = todo[rank == 0xFFFFFFFF]

	def distance(self, a, b, extra: int = 0, check: bool = True, prune=None) -> np.ndarray:
		"""`_KeptBall.distance`; with `extra` > 0 pairs up to radius + extra quarter turns apart are answered, by `solve_beyond`'s
		probes on the relative states (its lengths); `prune` as there: fewer look-ups, the same answers."""
		return self.path(a, b, extra, check, prune)[0] if extra else super().distance(a, b, check)

	def path(self, a, b, extra: int = 0, check: bool = True, prune=None):
		"""`_KeptBall.path`; with `extra` > 0 through `solve_beyond`: (lengths, actions (n, extra + radius)), pairs up to radius +
		extra quarter turns apart answered; `prune` as there: fewer look-ups, the same answers."""
		extra = eng.int_in("extra", extra, 0, self.MAX_EXTRA)
		if not extra:
			return super().path(a, b, check)
		prune = DevicePatternBound.of(prune)
		q = self._relative(a, b, check)
		return self._solve_beyond_of(q, 0 if q is None else len(q), extra, prune=prune)

	def _depths_ranks(self, depths, ranks):
		"""(depths int64 (n,), ranks int64 (n,)) of a `state_at` call, checked on the host: ValueError for anything but integers,
		for lengths that differ, a depth outside 0..radius or a rank outside [0, states_covered[depth])."""
		r = np.asarray(ranks)
		d = np.asarray(depths)
		for what, a in (("depths", d), ("ranks", r)):
			if a.dtype == bool or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
				raise ValueError(f"{what} must be integers, got dtype {a.dtype}")
		if r.dtype == np.uint64 and r.size and int(r.max()) > _ffi.INT64_MAX:
			raise ValueError("a rank above 2^63 - 1")
		r = r.astype(np.int64).reshape(-1)
		if d.ndim == 0:
			d = np.full(len(r), int(d), np.int64)
		d = d.astype(np.int64).reshape(-1)
		if len(d) != len(r):
			raise ValueError(f"{len(d)} depths for {len(r)} ranks")
		if len(r):
			if d.min() < 0 or d.max() > self.radius:
				raise ValueError(f"a depth outside 0..{self.radius}")
			if r.min() < 0 or (r >= self.states_covered[d]).any():
				raise ValueError("a rank outside [0, states_covered[depth])")
		return d, r

	def state_at(self, depths, ranks) -> np.ndarray:
		"""
		The states of (depths[i], ranks[i]), int8 (n, 20) or (n, 6, 8, 6) in the representation cube.get_is2024() names (engine
		rk_symball_state_at, one launch, a wave per sample).  THE STATE OF (d, r) is the k-th distinct conjugate, in ascending symmetry
		order, of the node j of level d whose cumulative orbit range holds r: the nodes of level d in index order, each counting
		for the size of its orbit, j the one whose range holds r and k = r minus the sizes in front of j.  For every d this maps
		[0, states_covered[d]) one to one onto the states at distance exactly d from solved, so a uniform rank is a uniform state
		at that distance; the map does not depend on `pops`.

		`depths` is an int (all ranks at that depth) or an array as long as `ranks`.  ValueError, before anything is launched, for a
		depth outside 0..radius, a rank outside [0, states_covered[depth]) or lengths that differ.  The first call makes the ball's
		orbit index on the device -- a byte per orbit and a 64-bit prefix per 256 orbits (`index_bytes`; 161 MB at radius 10 beside
		the ball's 5.3 GB) -- which is kept until the ball goes; a ball that never samples holds none.
		"""
		self.build()
		d, r = self._depths_ranks(depths, ranks)
		n = len(r)
		is2024 = cube.get_is2024()
		rows = np.zeros((n + 1, 20), np.int8)
		if n:
			out = cube.device.ball_state_at(self, torch.from_numpy(d.astype(np.int32)).to(gpu), torch.from_numpy(r).to(gpu))
			rows[1:] = out.cpu().numpy()
		return _states_out(is2024, rows, n)[1:]

	def sample(self, n: int, depth=None, rng=None):
		"""
		(states, depths int64 (n,)): n states drawn uniformly, by `state_at` of uniform ranks.  `rng` is a numpy.random.Generator
		(None: np.random.default_rng()), and it is asked exactly ONCE, so a generator seeded alike reproduces the states:
		  depth an int or an (n,) array   ranks = rng.integers(0, self.states_covered[depths], dtype=np.int64) with depths the (n,)
		                                  array (an int repeated n times): state i is uniform among the states at distance depths[i];
		  depth None                      g = rng.integers(0, self.states_covered.sum(), n, dtype=np.int64): uniform over the whole
		                                  ball; with c = np.cumsum(self.states_covered), depths = np.searchsorted(c, g, side="right")
		                                  and ranks = g - (c - self.states_covered)[depths].
		"""
		n = eng.int_in("n", n, 0)
		if rng is None:
			rng = np.random.default_rng()
		elif not isinstance(rng, np.random.Generator):
			raise TypeError(f"rng must be a numpy.random.Generator or None, not {type(rng).__name__}")
		covered = self.states_covered
		if depth is None:
			g = rng.integers(0, int(covered.sum()), n, dtype=np.int64)
			c = np.cumsum(covered)
			depths = np.searchsorted(c, g, side="right").astype(np.int64)
			ranks = g - (c - covered)[depths]
		else:
			depths = np.asarray(depth)
			if depths.dtype == bool or not np.issubdtype(depths.dtype, np.integer):
				raise ValueError(f"depth must be an integer, an integer array or None, got dtype {depths.dtype}")
			depths = np.full(n, int(depths), np.int64) if depths.ndim == 0 else depths.astype(np.int64).reshape(-1)
			if len(depths) != n:
				raise ValueError(f"{len(depths)} depths for n = {n}")
			if n and (depths.min() < 0 or depths.max() > self.radius):
				raise ValueError(f"a depth outside 0..{self.radius}")
			ranks = rng.integers(0, covered[depths], dtype=np.int64)
		return self.state_at(depths, ranks), depths

	def child_depths(self, states):
		"""(depth int64 (n,), children int64 (n, 12)): the exact distance to solved of every state and of its twelve children in action
		order (engine rk_symball_child_depths, one launch).  A quarter turn changes the distance by exactly one, so the answers are
		exact for every state within radius + 1 of solved -- radius + 1 for a state outside the ball with a child inside, radius + 2
		for such a state's other children --; a state further out gets -1 thirteen times."""
		self.build()
		rows = self._rows(states)
		n = len(rows)
		if n == 0:
			return np.zeros(0, np.int64), np.zeros((0, 12), np.int64)
		depth, children = cube.device.ball_child_depths(self, torch.from_numpy(rows).to(gpu))
		return depth.cpu().numpy().astype(np.int64), children.cpu().numpy().astype(np.int64)

	def _index_status(self):
		status = (C.c_longlong * 16)()
		_ffi.check(_ffi.lib().rk_symball_index_status(self.build()._h, status))
		return status

	@property
	def index_builds(self) -> int:
		"""How often this ball's orbit index was made: 0 before the first `state_at`, 1 from then on."""
		return int(self._index_status()[0])

	@property
	def index_bytes(self) -> int:
		"""The device memory of the orbit index: 0 before the first `state_at`."""
		return int(self._index_status()[1])

	@property
	def index_levels(self) -> np.ndarray:
		"""int64 (radius + 1,): the orbit sizes of every level as the orbit index adds them up (= `states_covered`), None before the
		first `state_at`."""
		status = self._index_status()
		return np.diff(np.array(status[4:4 + self.radius + 2], np.int64)) if status[0] else None

	def arrays(self):
		"""The representatives of nodes 1 .. len(ball) in index order."""
		is2024 = cube.get_is2024()
		if is2024 not in self._cache:
			n = len(self)
			states = np.zeros((n + 1, 20), np.int8)
			_ffi.check(_ffi.lib().rk_symball_export(self._h, 1, n, states[1:].ctypes.data, _ffi.stream_ptr()))
			self._cache = {is2024: _states_out(is2024, states, n)[1:]}
		return self._cache[is2024]

	def __str__(self):
		index = f", orbit index {self.index_bytes / 1e6:.1f} MB" if self.built and self.index_builds else ""
		return f"Symmetry-reduced goal ball (device, radius={self.radius}{index})"


class DevicePatternDB(_ffi.Owner):
	"""
	A pattern database (engine rk_pdb_*, csrc/rk_pdb.hip): the exact number of quarter turns that bring a SUBSET of the cubies
	home, the others anywhere, for every placement of that subset, as a dense table of one byte per placement in HBM.  A move
	maps every cubie's code on its own, so the selected codes are closed under the 12 moves; the table index is the
	partial-permutation rank and orientation word of the selected corners, then of the selected edges.

	`corners` are cubies 0..7 and `edges` cubies 0..11 -- byte 8 + e of a 20-byte row --, in any order without repeats; at most
	2^31 entries, which admits seven edges at most (eleven or twelve edges are refused for the permutation parity; ValueError).  `cross(face)` selects the four edges of a face, `corners()` all eight
	corners (88 179 840 entries).  `build()` makes the table -- one sweep launch per level, every entry reached (the engine
	checks it) --, read-only from then on; a query before it is a ValueError.  `depth` and `solve` answer a batch in one launch
	each: numpy in -> numpy out, device tensor in -> device tensor out.  States are in the representation cube.get_is2024() names when a method is
	called.  A 20-byte row whose selected codes are no partial pattern (a code outside 0..23, two selected cubies of a kind on one
	position) gets -1; its other bytes are not looked at.

	A pattern's depth never exceeds the distance to solved, so `lower_bound(states, dbs)`, the elementwise maximum over several
	databases, is an admissible lower bound for every state.

	Out of scope: goals other than the home positions; orientation-only or position-only patterns (not closed under the moves in
	a cubie-indexed state); any use inside A*, MCTS or the beam (the deepening probes of the symmetry ball read them:
	`DevicePatternBound`).
	"""
	MAX_EDGES = 10
	MAX_SIZE = 1 << 31
	GRID_ROWS = 2048 * 256                  # RK_PDB_GRID workgroups of 256 states: beyond this many rows a thread takes several

	def __init__(self, corners=(), edges=()):
		self.corner_cubies = self._cubies("corners", corners, 8)
		self.edge_cubies = self._cubies("edges", edges, 12)
		kc, ke = len(self.corner_cubies), len(self.edge_cubies)
		if kc + ke == 0:
			raise ValueError("a pattern needs at least one cubie")
		if ke > self.MAX_EDGES:
			raise ValueError(f"edges must be at most {self.MAX_EDGES} cubies (with more the permutation parity leaves entries unreachable), got {ke}")
		size = 3 ** (7 if kc == 8 else kc) << ke
		for i in range(kc):
			size *= 8 - i
		for i in range(ke):
			size *= 12 - i
		if size > self.MAX_SIZE:
			raise ValueError(f"the pattern has {size} entries, more than {self.MAX_SIZE}")
		self.size = size
		self._h = None
		self._level_sizes = None

	@staticmethod
	def _cubies(name: str, cubies, limit: int) -> tuple:
		out = tuple(sorted(eng.int_in(name, c, 0, limit - 1, what=f"cubies in 0..{limit - 1}") for c in cubies))
		if len(set(out)) != len(out):
			raise ValueError(f"{name} must not repeat a cubie, got {tuple(cubies)!r}")
		return out

	@classmethod
	def cross(cls, face="D"):
		"""The four edges of a face ("F", "B", "T", "D", "L", "R" or 0..5), read from the library's face definitions."""
		faces = "FBTDLR"
		f = faces.index(face) if isinstance(face, str) and len(face) == 1 and face in faces else eng.int_in("face", face, 0, 5, what="one of F B T D L R or 0..5")
		from librubiks_amd.cube import maps
		return cls(edges=tuple(int(e) for e in maps._FACES[f, 4:8]))

	@classmethod
	def corners(cls):
		"""All eight corners: positions and twists, the last twist implied by the others."""
		return cls(corners=range(8))

	@property
	def built(self) -> bool:
		return self._level_sizes is not None

	def build(self):
		"""Builds the table on the device (nothing if it is built)."""
		if self.built:
			return self
		_ffi.require_gpu()
		if self._h is None:
			c, e = np.array(self.corner_cubies, np.uint8), np.array(self.edge_cubies, np.uint8)
			self._create("rk_pdb_create", "rk_pdb_destroy", c.ctypes.data, len(c), e.ctypes.data, len(e))
		_ffi.check(_ffi.lib().rk_pdb_build(self._h, _ffi.stream_ptr()))
		status = (C.c_longlong * 64)()
		_ffi.check(_ffi.lib().rk_pdb_status(self._h, status))
		assert int(status[1]) == self.size
		self._level_sizes = np.array(status[5:5 + int(status[4])], np.int64)
		return self

	def _free(self):
		super()._free()
		self._level_sizes = None                                             # no handle, no table: a query says "build first"

	def _need_built(self):
		if not self.built:
			raise ValueError("build the pattern database first (build())")

	@property
	def level_sizes(self) -> np.ndarray:
		"""int64 (levels,): the entries at distance 0, 1, ... from the goal; they add up to `size`."""
		self._need_built()
		return self._level_sizes

	@property
	def levels(self) -> int:
		return len(self.level_sizes)

	@property
	def max_depth(self) -> int:
		"""The deepest entry: the length of `solve`'s action rows."""
		return self.levels - 1

	def __len__(self):
		return self.size

	def depth(self, states):
		"""int32 (n,): the exact number of quarter turns that bring the selected cubies home, -1 for a row whose selected codes are
		no partial pattern.  One launch, no synchronisation for device tensors."""
		self._need_built()
		q, dev = _device_rows20(states)
		n = len(q)
		out = torch.empty(n, dtype=torch.int32, device=gpu)
		_ffi.check(_ffi.lib().rk_pdb_depth(self._h, q.data_ptr(), n, out.data_ptr(), _ffi.stream_ptr()))
		return _batch_out(dev, out)

	def solve(self, states):
		"""(lengths int32 (n,), actions int8 (n, max_depth)): a shortest word that brings the selected cubies home -- at each step
		the lowest action whose child's entry is one less --, rows padded with -1; length -1 for a row whose selected codes are no
		partial pattern.  One launch; reading the error word is the call's one host read."""
		self._need_built()
		q, dev = _device_rows20(states)
		n = len(q)
		lengths = torch.empty(n, dtype=torch.int32, device=gpu)
		actions = torch.empty((n, self.max_depth), dtype=torch.int8, device=gpu)
		err = torch.empty(1, dtype=torch.int32, device=gpu)
		_ffi.check(_ffi.lib().rk_pdb_solve(self._h, q.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(), err.data_ptr(), _ffi.stream_ptr()))
		if int(err.item()):
			raise _ffi.RubiksHipError(f"rk_pdb_solve reported error {int(err.item())}: an entry of the table has no child one level nearer")
		return _batch_out(dev, lengths, actions)

	@staticmethod
	def lower_bound(states, dbs):
		"""int32 (n,): the elementwise maximum of the `dbs`' depths, an admissible lower bound on the distance to solved of every
		state (-1 only where every database answers -1)."""
		dbs = list(dbs)
		if not dbs or not all(isinstance(db, DevicePatternDB) for db in dbs):
			raise ValueError("dbs must be one or more DevicePatternDB")
		best = dbs[0].depth(states)
		for db in dbs[1:]:
			d = db.depth(states)
			best = torch.maximum(best, d) if isinstance(best, torch.Tensor) else np.maximum(best, d)
		return best

	def table(self) -> np.ndarray:
		"""uint8 (size,): the table, entry by index."""
		self._need_built()
		out = np.empty(self.size, np.uint8)
		_ffi.check(_ffi.lib().rk_pdb_export(self._h, 0, self.size, out.ctypes.data, _ffi.stream_ptr()))
		return out

	def __str__(self):
		return f"Pattern database (device, corners={self.corner_cubies}, edges={self.edge_cubies}, {self.size} entries)"


class DevicePatternBound(_ffi.Owner):
	"""
	An admissible lower bound from 1..4 pattern databases in one handle (engine rk_bound_*, csrc/rk_pdb.hip): the greatest of the
	databases' depths of a state.  `depth(states)` is `DevicePatternDB.lower_bound(states, dbs)` in ONE launch, with the same
	input rules (numpy in -> numpy out, device tensor in -> device tensor out, -1 only where every database answers -1).  The
	databases are built if need be and kept alive by this object; ValueError for an empty list, more than four databases, a repeat
	or anything that is no `DevicePatternDB`.

	Its use is `prune=` of `DeviceSymBall.solve_beyond` / `distance` / `path` and of `DeviceSymBallSearch(deepen=E)`: the probes past
	the ball skip every word behind a state whose bound shows that no state of the ball lies within the moves still to make.  The
	bound is admissible, so no word that hits is skipped and the answers are the unpruned engine's, bit for bit.
	"""
	MAX_DBS = 4

	def __init__(self, dbs):
		try:
			dbs = tuple(dbs)
		except TypeError:
			raise ValueError("dbs must be a sequence of DevicePatternDB") from None
		if not 1 <= len(dbs) <= self.MAX_DBS or not all(isinstance(db, DevicePatternDB) for db in dbs):
			raise ValueError(f"dbs must be 1..{self.MAX_DBS} DevicePatternDB, got {dbs!r}")
		if len({id(db) for db in dbs}) != len(dbs):
			raise ValueError("dbs must not repeat a database")
		self.dbs = dbs
		for db in dbs:
			db.build()
		handles = (C.c_void_p * len(dbs))(*(db._h.value for db in dbs))
		self._create("rk_bound_create", "rk_bound_destroy", handles, len(dbs))

	@classmethod
	def of(cls, prune):
		"""A `prune=` argument as the engines take it: None stays None, a `DevicePatternBound` must still be usable, a list of
		databases is wrapped into one."""
		if prune is None:
			return None
		bound = prune if isinstance(prune, cls) else cls(prune)
		bound._need_handle()
		return bound

	def _need_handle(self):
		"""ValueError for a bound that was freed, or whose databases were: the handle holds their tables' addresses."""
		if self._h is None or not all(db.built for db in self.dbs):
			raise ValueError("the pattern bound or one of its databases was freed")

	def depth(self, states):
		"""int32 (n,): the greatest of the databases' depths, an admissible lower bound on the distance to solved of every state.
		One launch, no synchronisation for device tensors."""
		self._need_handle()
		q, dev = _device_rows20(states)
		n = len(q)
		out = torch.empty(n, dtype=torch.int32, device=gpu)
		_ffi.check(_ffi.lib().rk_bound_depth(self._h, q.data_ptr(), n, out.data_ptr(), _ffi.stream_ptr()))
		return _batch_out(dev, out)

	def __str__(self):
		return "Pattern bound (device, " + "; ".join(f"corners={db.corner_cubies} edges={db.edge_cubies}" for db in self.dbs) + ")"


class _TableSolver(Agent, _ffi.Owner):
	"""What the table solvers share: `shorten` and `allow_illegal`, the error word that names the lowest row that is no legal state,
	the export of a table, and `search`.  A subclass makes its handle and writes `solve`, which returns lengths and actions first."""

	def __init__(self, shorten, allow_illegal):
		Agent.__init__(self)
		if shorten is not None and not isinstance(shorten, _KeptBall):
			raise ValueError("shorten must be a DeviceGoalBall, a DeviceSymBall or None")
		self.shorten, self.allow_illegal = shorten, bool(allow_illegal)

	def _error_word(self):                                               # where a solve entry names the lowest illegal row
		return None if self.allow_illegal else torch.full((1,), -1, dtype=torch.int32, device=gpu)

	def _raise_illegal(self, err):                                       # the call's one host read
		if err is not None and int(err.item()) >= 0:
			raise ValueError(f"row {int(err.item())} of states is not a legal cube state (the lowest such row)")

	def _shortened(self, lengths, actions):
		"""The queues after `self.shorten.shorten`, back in `solve`'s shape on the device."""
		h_len, h_act = lengths.cpu().numpy(), actions.cpu().numpy()
		queues = self.shorten.shorten([h_act[i, :max(int(h_len[i]), 0)] for i in range(len(h_len))])
		out = np.full(h_act.shape, -1, np.int8)
		for i, queue in enumerate(queues):
			out[i, :len(queue)] = queue
			if h_len[i] >= 0:
				h_len[i] = len(queue)
		return torch.from_numpy(h_len).to(gpu), torch.from_numpy(out).to(gpu)

	def _export(self, entry: str, which, what: str) -> np.ndarray:
		which = eng.int_in(what, which, 1, 4, what=f"a {what} 1..4")
		out = np.empty(self.table_sizes[which - 1], np.uint8)
		_ffi.check(getattr(_ffi.lib(), entry)(self._h, which, 0, len(out), out.ctypes.data, _ffi.stream_ptr()))
		return out

	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		"""The state's solution into `action_queue`; len(agent) is 1, the one state looked at.  Neither limit is needed or used."""
		self._explored_states = 0
		self.action_queue = deque()
		is2024 = cube.get_is2024()
		rows = _roots20(is2024, state, 1)
		was_illegal, self.allow_illegal = self.allow_illegal, False       # an agent cannot answer "no state"
		try:
			lengths, actions = self.solve(rows if is2024 else cube.as686(rows))
		finally:
			self.allow_illegal = was_illegal
		self._explored_states = 1
		self.action_queue = deque(int(a) for a in actions[0, :int(lengths[0])])
		return True


class DeviceChainSolver(_TableSolver):
	"""
	A solution for EVERY legal state, batched on the device (engine rk_chain_*, csrc/rk_chain.hip): the subgroup chain -- four
	stages, each a table of exact costs over the cosets of the next subgroup, built on the host when the solver is made and kept
	in HBM (2.5 MB) -- answered by four table descents in one launch, a thread per state: no search, no pool, no net.  Stage 1
	uses the 12 quarter turns, the later ones fewer and fewer of them and the half turns XX (the action 2 f twice) of the other
	faces.  Solutions are NOT optimal -- at most `max_length` moves, some tens on average --; `shorten=ball` (a
	`DeviceGoalBall` or `DeviceSymBall`) pipes every queue through `ball.shorten`, which makes it locally optimal.

	`solve(states)` takes a batch: numpy in -> numpy out, device tensor in -> device tensor out; states are in the representation
	cube.get_is2024() names when a method is called.  As an agent (`search(state)` fills `action_queue`; never fails on a legal
	state) it plays in `Evaluator` and under `TowardsGoal`.  A row that is no legal state (`cube.is_legal`) is a ValueError naming
	the lowest such row, or, with `allow_illegal`, gets length -1 (its stage lengths -1, its actions all -1).
	"""
	GRID_ROWS = 2048 * 256                  # RK_CHAIN_GRID workgroups of 256 states: beyond this many rows a thread takes several

	def __init__(self, shorten=None, allow_illegal: bool = False):
		super().__init__(shorten, allow_illegal)
		_ffi.require_gpu()
		self._create("rk_chain_create", "rk_chain_destroy", _ffi.stream_ptr())
		status = (C.c_longlong * 16)()
		_ffi.check(_ffi.lib().rk_chain_status(self._h, status))
		self.coset_counts = tuple(int(v) for v in status[0:4])
		self.stage_depths = tuple(int(v) for v in status[4:8])           # the deepest entry of each table
		self.max_length = int(status[8])                                 # the row length of `solve`'s actions
		self.table_sizes = tuple(int(v) for v in status[9:13])

	def solve(self, states, stage_lengths: bool = False):
		"""(lengths int32 (n,), actions int8 (n, max_length) padded with -1[, stage lengths int32 (n, 4)]): per stage, at each step
		the lowest generator whose entry equals the current entry minus its cost.  One launch; reading the error word (not with
		`allow_illegal`) is the call's one host read.  With `shorten` the queues come back through `ball.shorten` (lengths and
		actions then describe the shortened queues; the stage lengths stay the chain's own)."""
		q, dev = _device_rows20(states)
		n = len(q)
		lengths = torch.empty(n, dtype=torch.int32, device=gpu)
		actions = torch.full((n, self.max_length), -1, dtype=torch.int8, device=gpu)
		stages = torch.empty((n, 4), dtype=torch.int32, device=gpu) if stage_lengths else None
		err = self._error_word()
		_ffi.check(_ffi.lib().rk_chain_solve(self._h, q.data_ptr(), n, lengths.data_ptr(), actions.data_ptr(),
		                                     stages.data_ptr() if stage_lengths else None, None if err is None else err.data_ptr(), _ffi.stream_ptr()))
		self._raise_illegal(err)
		if self.shorten is not None and n:
			lengths, actions = self._shortened(lengths, actions)
		return _batch_out(dev, lengths, actions, *((stages,) if stage_lengths else ()))

	def export(self, stage: int) -> np.ndarray:
		"""uint8 (table_sizes[stage - 1],): the table of stage 1..4, entry by index; 255 = no coset has this index."""
		return self._export("rk_chain_export", stage, "stage")

	def __str__(self):
		return "Subgroup chain solver (device)" + (f", shortened by {self.shorten}" if self.shorten is not None else "")


class DeviceTwoPhaseSolver(_TableSolver):
	"""
	SHORT solutions for every legal state, batched on the device, by search and without a net (engine rk_twophase_*,
	csrc/rk_twophase.hip): IDA* over the 12 quarter turns into the subgroup <F, B, TT, DD, LL, RR> -- the one the chain's stage 3
	starts in --, then IDA* inside it, over four pruning tables of exact costs and six move tables built on the host when the solver
	is made (5.6 MB in HBM).  The chain's answer (`chain`, a `DeviceChainSolver`; one is made and kept when none is passed) is every
	row's first best, so an answer is never longer than the chain's and the search never fails.  `tries` = the phase-1 solutions
	whose phase 2 is searched, `max_nodes` = the child evaluations a state may cost; the answer is a function of (state, tries,
	max_nodes) alone (include/rubiks_hip.h states the move-pruning and the budget rule, DESIGN 3.59.9 the kernel).  The defaults of
	`tries` and `max_nodes` were provisional until benchmarks/two_phase.py had run; they are now chosen from that run
	(profiles/r29_two_phase.json): on 40-move scrambles 35.8 moves on average against the chain's 48.4 at 85 000
	states/s, where max_nodes = 2^16 leaves 84 % of the rows with the chain's answer.

	`phase2_cap=C` (1..the chain's `max_length`; None: no cap, the search above answer for answer) cuts every phase 2 short: a
	phase-1 solution whose phase-2 entry is above C is left behind, and a phase 2 whose bound passes C is given up, so the budget
	goes to many phase-1 solutions instead of one deep phase 2 and an improved row has at most C moves inside the subgroup.  With a
	cap `tries` is no longer what ends a search: pass `tries=None`, 2^31 - 1.  The answer is then a function of (state, tries,
	max_nodes, C) alone.  Measured (profiles/r32_two_phase_cap.json): on 40-move scrambles `tries=None, max_nodes=1 << 20,
	phase2_cap=18` gives 30.1 moves where the defaults give 35.8, with 8 % of the rows still the chain's instead of 26 %, at 1.8x the
	defaults' time; at max_nodes = 2^16 no cap beats the search without one.

	`solve(states)` has `DeviceChainSolver.solve`'s rules: numpy in -> numpy out, device tensor in -> device tensor out, states in the
	representation cube.get_is2024() names, a row that is no legal state a ValueError naming the lowest such row or, with
	`allow_illegal`, length -1 (phase lengths -1, actions all -1, reason 2, no node).  As an agent it plays in `Evaluator` and under
	`TowardsGoal`; `shorten=ball` pipes every queue through `ball.shorten`.
	"""
	GRID_ROWS = 1024 * 256                  # RK_TWOPHASE_GRID workgroups of 256 lanes: beyond this many rows a lane takes several

	def __init__(self, chain=None, tries: int = 8, max_nodes: int = 1 << 20, phase2_cap: int = None, shorten=None, allow_illegal: bool = False):
		if chain is not None and not isinstance(chain, DeviceChainSolver):
			raise ValueError("chain must be a DeviceChainSolver or None")
		super().__init__(shorten, allow_illegal)
		self.tries = (1 << 31) - 1 if tries is None else eng.int_in("tries", tries, 1, (1 << 31) - 1)
		self.max_nodes = eng.int_in("max_nodes", max_nodes, 1, _ffi.INT64_MAX)
		_ffi.require_gpu()
		self.chain = chain if chain is not None else DeviceChainSolver()
		self._create("rk_twophase_create", "rk_twophase_destroy", _ffi.stream_ptr())
		status = (C.c_longlong * 16)()
		_ffi.check(_ffi.lib().rk_twophase_status(self._h, status))
		self.table_counts = tuple(int(v) for v in status[0:4])
		self.table_depths = tuple(int(v) for v in status[4:8])           # the deepest entry of each pruning table
		self.table_sizes = tuple(int(v) for v in status[8:12])
		self.grid_rows = int(status[12]) * int(status[13])
		self.max_length = self.chain.max_length                          # the row length of `solve`'s actions
		self.phase2_cap = eng.int_in("phase2_cap", phase2_cap, 1, self.max_length, none_ok=True)

	def solve(self, states, phase_lengths: bool = False, details: bool = False, counts: bool = False):
		"""(lengths int32 (n,), actions int8 (n, max_length) padded with -1[, phase lengths int32 (n, 2)][, reason int32 (n,), nodes
		int64 (n,)][, counts int32 (n, 2)]): reason 0 = the search ended by itself and improved the chain's answer, 1 = the budget ended it and the answer is
		from the search, 2 = the row holds the chain's answer; counts = the phase-1 solutions the search found and the phase-2 searches
		it entered (0 0 for a row that is no legal state).  Two launches; reading the error word (not with `allow_illegal`) is the
		call's one host read.  With `shorten` the queues come back through `ball.shorten` (lengths and actions then describe the
		shortened queues; phase lengths, reason, nodes and counts stay the search's own)."""
		if self.chain._h is None:
			raise ValueError("the chain solver was freed")
		q, dev = _device_rows20(states)
		n = len(q)
		lengths = torch.empty(n, dtype=torch.int32, device=gpu)
		actions = torch.full((n, self.max_length), -1, dtype=torch.int8, device=gpu)
		phases = torch.empty((n, 2), dtype=torch.int32, device=gpu)
		reason = torch.empty(n, dtype=torch.int32, device=gpu)
		nodes = torch.empty(n, dtype=torch.int64, device=gpu)
		both = torch.empty((n, 2), dtype=torch.int32, device=gpu) if counts else None
		err = self._error_word()
		_ffi.check(_ffi.lib().rk_twophase_solve_capped(self._h, self.chain._h, q.data_ptr(), n, self.tries, self.max_nodes, self.phase2_cap or 0,
		                                               lengths.data_ptr(), actions.data_ptr(), phases.data_ptr(), reason.data_ptr(), nodes.data_ptr(),
		                                               both.data_ptr() if counts else None, None if err is None else err.data_ptr(),
		                                               _ffi.stream_ptr()))
		self._raise_illegal(err)
		if self.shorten is not None and n:
			lengths, actions = self._shortened(lengths, actions)
		return _batch_out(dev, lengths, actions, *((phases,) if phase_lengths else ()), *((reason, nodes) if details else ()),
		                  *((both,) if counts else ()))

	def export(self, table: int) -> np.ndarray:
		"""uint8 (table_sizes[table - 1],): pruning table 1..4, entry by index (every entry is reached)."""
		return self._export("rk_twophase_export", table, "table")

	def __str__(self):
		return f"Two-phase solver (device, tries={self.tries}, max_nodes={self.max_nodes}" + \
			(f", phase2_cap={self.phase2_cap})" if self.phase2_cap is not None else ")") + \
			(f", shortened by {self.shorten}" if self.shorten is not None else "")


class _BallSearch(_PoolSearch):
	"""What `DeviceBallSearch` and `DeviceSymBallSearch` share on top of `_PoolSearch`: the ball they end at (`_ball_type` is its
	kind), the meeting and the levels around the start.  Their engines have one argument list and one status layout."""
	_status_words = 10
	_unlimited = True
	_engine_name = "ball search"
	_ball_type = None

	def __init__(self, ball, pops: int = 16_384, capacity: int = None, max_capacity: int = None, poll: int = 8):
		if not isinstance(ball, self._ball_type):
			raise TypeError(f"ball must be a {self._ball_type.__name__}, got {type(ball).__name__}")
		super().__init__(pops, capacity, max_capacity, poll)
		self.ball = ball
		self._root = None                   # the start of the last search, 20 bytes
		self._meet = 0                      # the ball's node that the meeting child (or the start itself) equals
		self.depth = 0                      # complete levels around the start after the last search

	def _create_args(self) -> tuple:
		return (self.ball._h,)

	def _begin(self, root) -> bool:
		self._meet, self.depth = 0, 0
		self._root = root
		self.ball.build()
		return False                        # (a solved start is the ball's node 1: the engine answers it without a pop)

	def _read(self, status):
		self.popped = int(status[4])
		self.depth, self._meet = int(status[8]), int(status[9])

	@property
	def meeting_depth(self):
		"""The depth in the ball of the node the search met; None when the last search did not meet."""
		return self.ball.depth_of_node(self._meet) if self._meet else None


class DeviceBallSearch(_BallSearch):
	"""
	A SHORTEST solution (quarter-turn metric) by a one-sided breadth-first search from the start that ends at the first child a
	kept `DeviceGoalBall` holds (engine rk_bsearch_*, csrc/rk_ball.hip).  Node 1 of the own pool is the start; levels grow as in
	`DeviceBiBFS`: a child the own pool holds is skipped, a child the ball holds is the meeting (the search ends, the child is
	not stored, the lowest batch position wins), any other is appended.  A start at distance D > radius meets while level
	D - radius grows, in a node of ball depth `radius`, so the first meeting is optimal.  A start the ball holds is answered by
	the ball's path: then len(agent) == 1 and nothing is popped.  The state budget is checked before every pop, the time limit
	when the host polls.  `action_queue`, len(agent), the pool, `depth` and the meeting do not depend on `pops`.

	`capacity`, `max_capacity`, `grown` and `capacity_exhausted` are `DeviceBFS`'s, for the own pool; its table is sized to it and
	a new search clears that table, never the ball's.  Several agents may share one ball; each holds a reference to it.
	"""
	_entries = "rk_bsearch"
	_ball_type = DeviceGoalBall

	def __init__(self, ball: DeviceGoalBall, pops: int = 16_384, capacity: int = None, max_capacity: int = None, poll: int = 8):
		super().__init__(ball, pops, capacity, max_capacity, poll)

	@property
	def meeting(self):
		"""The state where the search met the ball -- the child that was not stored, or the start itself when the ball holds it --
		in the representation of the search; None when the last search did not meet."""
		if not self._meet:
			return None
		state = np.zeros((2, 20), np.int8)
		_ffi.check(_ffi.lib().rk_ball_export(self.ball._h, self._meet, 1, state[1:].ctypes.data, None, None, _ffi.stream_ptr()))
		return _states_out(self._is2024, state, 1)[1]

	def __str__(self):
		return f"Breadth-first search to a goal ball (device, radius={self.ball.radius}, pops={self.pops})"


class DeviceSymBallSearch(_BallSearch):
	"""
	`DeviceBallSearch` that ends at a kept `DeviceSymBall` (engine rk_ssearch_*, csrc/rk_sym.hip): the own pool holds raw states
	with parent and action, and a child is the meeting when the symmetry ball holds its canonical representative.  A state lies
	in the plain ball of radius R exactly when its representative lies in the symmetry ball of radius R, so `arrays()`, len(agent),
	`depth`, `popped`, `iterations` and `meeting` equal `DeviceBallSearch`'s on a `DeviceGoalBall(R)`; the ball's half of
	`action_queue` is the descent of `DeviceSymBall.solve` from the meeting state and has the same length.  The symmetry ball
	reaches radius 10 where the plain one ends at 8, and every level of radius saves the search a level of its own (x 9.3 states).
	An iteration costs one launch more than `DeviceBallSearch`'s: the canonical forms of the batch, a wave per child.

	`meeting` is the RAW state that met (the child that was not stored, or the start), `meeting_node` the node of its
	representative in the ball, `meeting_depth` that node's depth.  Several agents may share one ball.

	`deepen=E` > 0: a search that ends unsolved because the pool is exhausted -- and for no other reason -- goes on
	without a pool.  First the pop count is lowered until not even one pop fits, so the complete levels are those of `pops=1`.
	Then rounds e = 1..E apply every word of e moves to the nodes of the newest complete level L, in index order and in chunks of
	`deepen_chunk` nodes, and look the results up in the ball (engine rk_sdeepen_nodes).  The first chunk with a hit ends the
	search: the lowest node of it that has a hit, that node's lowest word, then the descent; `action_queue` is that path, of the
	optimal length L + e + radius, and does not depend on `pops`, the chunk or the launch cap.  Afterwards `deepened` is e (0: the
	pool sufficed), `probes` the probes issued, `capacity_exhausted` stays True, len(agent) and `arrays()` are still the pool
	(its partial next level included), and there is no meeting.  The time limit covers both phases.

	`prune` (with `deepen` > 0 only; a `DevicePatternBound` or a list of 1..4 `DevicePatternDB`) leaves out the look-ups that an
	admissible bound rules out (engine rk_sdeepen_nodes_pruned): a state whose bound exceeds the radius plus the moves still to
	make has no state of the ball behind it, and no prefix of a word that hits is such a state.  The hits are therefore the same:
	`action_queue`, `deepened` and `probes` are those of the search without `prune`, and `lookups` -- the ball look-ups made,
	equal to `probes` without `prune` -- is what drops.
	"""
	_entries = "rk_ssearch"
	_ball_type = DeviceSymBall
	deepen_chunk = None                     # frontier nodes per chunk (None: as many as one launch takes with all their words)

	def __init__(self, ball: DeviceSymBall, pops: int = 16_384, capacity: int = None, max_capacity: int = None, poll: int = 8, deepen: int = 0,
	             prune=None):
		super().__init__(ball, pops, capacity, max_capacity, poll)
		self.deepen = eng.int_in("deepen", deepen, 0, DeviceSymBall.MAX_EXTRA)
		if prune is not None and not self.deepen:
			raise ValueError("prune needs deepen > 0: only the probes past the pool are pruned")
		self.prune = prune if prune is None or isinstance(prune, DevicePatternBound) else DevicePatternBound(prune)
		self.deepened = 0
		self.probes = 0
		self.lookups = 0

	def _grow(self, h) -> bool:
		if not self.deepen or self._h_cap < self.max_capacity:
			return super()._grow(h)                              # (a growth the device refuses raises, with or without `deepen`)
		self.capacity_exhausted = True                           # no warning yet: the search goes on
		return False

	def _fewer_pops(self, h, pops: int) -> int:
		fit = (self._h_cap - self._n) // 12                      # pops the pool still takes whatever they find
		if not self.deepen or fit < 1:
			return 0
		fewer = min(fit, max(1, pops // 2))
		_ffi.check(_ffi.lib().rk_sdeepen_set_pops(h, fewer, _ffi.stream_ptr()))
		return fewer

	def _pool_full(self, h, t0: float, time_limit: float) -> bool:
		if not self.deepen:
			return False
		end = self._deepen_search(h, t0, time_limit)
		if end == "none":
			eng.pool_exhausted(self, self._h_cap, f"is full and {self.deepen} more moves from its newest complete level reach no state of the ball")
		return end == "hit"                                      # ("time": the limit ran out, as it may in the pool phase)

	@no_grad
	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		self.deepened, self.probes, self.lookups = 0, 0, 0
		if self.prune is not None:
			self.prune._need_handle()
		return super().search(state, time_limit, max_states)

	def _deepen_search(self, h, t0: float, time_limit: float) -> str:
		"""Rounds 1 .. `deepen` from the newest complete level of the pool: "hit" with `action_queue` and `deepened` set at the first
		hit, "none" when no round has one, "time" when `time_limit` seconds since `t0` are over (looked at after every launch)."""
		looked = None if self.prune is None else torch.zeros(1, dtype=torch.int64, device=gpu)
		try:
			return self._deepen_rounds(h, t0, time_limit, looked)
		finally:
			self.lookups = self.probes if looked is None else int(looked.item())

	def _deepen_rounds(self, h, t0: float, time_limit: float, looked) -> str:
		"""`_deepen_search`'s rounds; `looked`: the device word that counts the look-ups of a pruned search, None without `prune`."""
		lib, stream = _ffi.lib(), _ffi.stream_ptr()
		level = (C.c_longlong * 2)()
		_ffi.check(lib.rk_sdeepen_frontier(h, level, stream))
		lo, hi = int(level[0]), int(level[1])
		cap = self.ball._launch_cap()
		chunk = eng.int_in("deepen_chunk", self.deepen_chunk, 1, none_ok=True, what="a positive integer or None")
		for e in range(1, self.deepen + 1):
			words = (12 if lo == 1 else 11) * 11 ** (e - 1)                 # (node 1 has no last move; it is a level of its own)
			per = min(chunk or max(1, cap // words), cap)
			for at in range(lo, hi + 1, per):
				cnt = min(per, hi + 1 - at)
				best = torch.full((cnt,), -1, dtype=torch.int32, device=gpu)    # 0xFFFFFFFF: no hit
				step = max(1, min(words, cap // cnt))
				for first in range(0, words, step):
					count = min(step, words - first)
					if looked is None:
						_ffi.check(lib.rk_sdeepen_nodes(h, e, at, cnt, first, count, best.data_ptr(), stream))
					else:
						_ffi.check(lib.rk_sdeepen_nodes_pruned(h, self.prune._h, e, at, cnt, first, count, best.data_ptr(), looked.data_ptr(), stream))
					self.probes += cnt * count
					torch.cuda.current_stream().synchronize()
					if time.perf_counter() - t0 >= time_limit:
						return "time"
				rank = best.cpu().numpy().view(np.uint32)
				hit = np.nonzero(rank != 0xFFFFFFFF)[0]
				if len(hit):                                                 # the lowest node of the chunk with a hit, its lowest word
					k = int(hit[0])
					self.action_queue = eng.read_path(lib.rk_sdeepen_path, h, at + k, e, int(rank[k]))
					self.deepened = e
					return "hit"
		return "none"

	@property
	def meeting_node(self):
		"""The node in the ball of the representative of the state that met; None when the last search did not meet."""
		return self._meet or None

	@property
	def meeting(self):
		"""The state where the search met the ball -- the child that was not stored, or the start itself when the ball holds its
		orbit -- in the representation of the search; None when the last search did not meet.  The ball keeps representatives
		only, so this is the start moved along the own half of `action_queue`."""
		if not self._meet:
			return None
		state = np.zeros((2, 20), np.int8)
		state[1] = self._root
		own = np.asarray(list(self.action_queue)[:len(self.action_queue) - self.meeting_depth], np.uint8)      # (a deque)
		moved = np.empty(20, np.int8)
		for a in own:                                        # (a handful of moves, on 20-byte states whatever the representation)
			_ffi.check(_ffi.lib().rk_multi_rotate_host(_ffi.REPR_2024, state[1:].ctypes.data, a.reshape(1).ctypes.data, moved.ctypes.data, 1,
			                                           _ffi.stream_ptr()))
			state[1] = moved
		return _states_out(self._is2024, state, 1)[1]

	def __str__(self):
		return f"Breadth-first search to a symmetry-reduced goal ball (device, radius={self.ball.radius}, pops={self.pops})"


class _BallSearchBatch(_ffi.Owner):
	"""What `DeviceBallSearchBatch` and `DeviceSymBallSearchBatch` share, as `_BallSearch` serves the two single agents: the arguments
	and their checks, the engine that is kept between calls, and the host loop of a call -- slots, refill at every poll, budgets,
	the time limit, `keep_arrays`, `on_poll`, and putting live slots to rest.  `_entries` is the prefix of the engine's entry points
	(one argument list and one status layout for both), `_ball_type` the kind of ball it ends at."""
	default_capacity = 8_000_000
	MAX_SEARCHES = 1024                     # the limits of rk_bsearchb_create and rk_ssearchb_create
	MAX_POPS = 1 << 22
	MAX_CAPACITY = 0x3FFFFFF0
	PATH_WORDS = 64                         # actions read per slot at a poll (a longer queue is read again, whole)
	_entries = None
	_ball_type = None

	def __init__(self, ball, searches: int = 64, pops: int = 2_048, capacity: int = None, poll: int = 8):
		if not isinstance(ball, self._ball_type):
			raise TypeError(f"ball must be a {self._ball_type.__name__}, got {type(ball).__name__}")
		self.searches = eng.int_in("searches", searches, 1, self.MAX_SEARCHES)
		self.pops = eng.int_in("pops", pops, 1, self.MAX_POPS)
		self.capacity = eng.int_in("capacity", capacity, 2, self.MAX_CAPACITY, none_ok=True)
		self.poll = eng.int_in("poll", poll, 1, what="a positive integer")
		self.ball = ball
		self._h, self._h_cap = None, 0
		self._is2024 = True
		self.on_poll = None                 # callable(status (n, 10)): called at every poll
		self.lockstep_iterations = 0        # iterations of all slots the last call launched
		self._results(0, False)

	def _results(self, n: int, keep_arrays: bool):
		self.status = np.zeros((n, 10), np.int64)
		self.lengths = np.full(n, -1, np.int64)
		self._queues = [deque() for _ in range(n)]
		self._arrays = [None] * n if keep_arrays else None
		self._deep = {}                     # slot -> what a search that goes on past its full pool keeps on the host (`_pool_full`)

	# What an engine that goes on past a full pool hooks into the loop of `search` (as `_PoolSearch` has `_fewer_pops` / `_pool_full`);
	# here nothing does, and `_deep` stays empty.
	def _prepare(self, h):
		"""Before the first slot of a call is started."""

	def _pool_full(self, s: int, i: int) -> bool:
		"""Slot `s` stopped state `i` with reason 5, its status, queue and pool are recorded.  True: the slot stays held (in `_deep`)."""
		return False

	def _deepen_poll(self, h, holds: np.ndarray) -> list:
		"""At a poll, after the status was read: the slots of `_deep` that are finished, their results recorded."""
		return []

	def _deepen_launch(self, h):
		"""One launch for the slots of `_deep`, behind the burst of the others."""

	sizes = property(lambda self: self.status[:, 2])
	iterations = property(lambda self: self.status[:, 3])
	popped = property(lambda self: self.status[:, 4])
	stops = property(lambda self: self.status[:, 5])
	depths = property(lambda self: self.status[:, 8])
	capacity_exhausted = property(lambda self: self.status[:, 5] == 5)

	def _entry(self, name: str):
		return getattr(_ffi.lib(), f"{self._entries}_{name}")

	@property
	def meeting_depths(self) -> np.ndarray:
		"""int64 (n,): the depth in the ball of the node every search met, from the ball's level boundaries; -1 for a search that did
		not meet."""
		meet = self.status[:, 9]
		if not meet.any():
			return np.full(len(meet), -1, np.int64)
		return np.where(meet > 0, np.searchsorted(self.ball.level_start, meet, side="right") - 1, -1).astype(np.int64)

	def _engine(self, capacity: int):
		if self._h is not None and self._h_cap >= capacity:
			return self._h
		self._free()                        # the old pools go before the new ones are made
		self._h_cap = capacity
		return self._create(f"{self._entries}_create", f"{self._entries}_destroy", self.ball._h, self.searches, capacity, self.pops)

	def _start(self, h, slots: list, rows: np.ndarray, budgets: np.ndarray):
		sl = np.ascontiguousarray(slots, dtype=np.int32)
		rows, budgets = np.ascontiguousarray(rows, dtype=np.int8), np.ascontiguousarray(budgets, dtype=np.int64)
		_ffi.check(self._entry("reset")(h, len(sl), sl.ctypes.data, rows.ctypes.data, budgets.ctypes.data, _ffi.stream_ptr()))

	def _paths(self, h, max_len: int) -> np.ndarray:
		out = np.zeros((self.searches, 1 + max_len), np.int32)
		_ffi.check(self._entry("paths")(h, out.ctypes.data, max_len, _ffi.stream_ptr()))
		return out

	def _export(self, h, slot: int, n: int):
		states, parents, actions = eng.export_frontier(self._entry("export"), (h, slot), n)
		return _states_out(self._is2024, states, n)[1:], parents[1:], actions[1:]

	@no_grad
	def search(self, states, time_limit: float = None, max_states=None, keep_arrays: bool = False) -> np.ndarray:
		"""bool (n,): whether each state has a queue (`lengths` >= 0): its search met the ball, or went on past its full pool and
		found one.  `max_states`: one budget for all, or one per state (n,); `time_limit` bounds the whole call: searches still
		running or waiting when it passes come back False with stop reason 0 (5 for one that was past its full pool)."""
		t0 = time.perf_counter()
		time_limit = time_limit or 1e10         # (an exact search may run without either limit)
		self._is2024 = cube.get_is2024()
		arr = np.asarray(states, dtype=np.int8)
		width = 20 if self._is2024 else 288
		if arr.size % width:
			raise ValueError(f"states must be (n, 20), or (n, 6, 8, 6) in 6x8x6 mode, got shape {arr.shape}")
		n = arr.size // width
		budgets = np.asarray(int(1e10) if max_states is None else max_states)
		if budgets.ndim > 1 or (budgets.ndim == 1 and len(budgets) != n):
			raise ValueError(f"max_states must be a number or one per state, got shape {budgets.shape}")
		budgets = np.minimum(np.broadcast_to(budgets, (n,)).astype(np.int64), 2 ** 31 - 1)
		rows = _roots20(self._is2024, arr, n)   # ValueError for an illegal 6x8x6 state, before anything runs
		self._results(n, keep_arrays)
		self.lockstep_iterations = 0
		if n == 0:
			return np.zeros(0, bool)
		_ffi.require_gpu()
		self.ball.build()
		stream = _ffi.stream_ptr()
		run, read_status = self._entry("run"), self._entry("status")
		S, K = self.searches, 12 * self.pops
		cap = self.capacity or min(int(budgets.max()) + K, self.default_capacity)
		h = self._engine(max(2, min(cap, self.MAX_CAPACITY)))
		self._prepare(h)
		holds = np.full(S, -1, np.int64)        # the input position every slot runs, -1: free
		waiting = 0                             # the next input position to start
		st = np.zeros((S, 10), np.int64)
		try:
			while True:
				_ffi.check(read_status(h, st.ctypes.data, stream))
				if st[holds >= 0, 6].any():
					raise _ffi.RubiksHipError(f"ball search engine error codes {st[holds >= 0, 6].tolist()}")
				pool = holds >= 0                   # the held slots that are in their pool phase
				pool[list(self._deep)] = False
				done = np.nonzero(pool & (st[:, 0] != 0))[0]
				if len(done):
					paths = self._paths(h, self.PATH_WORDS) if st[done, 1].any() else None
					if paths is not None and paths[done, 0].max() > self.PATH_WORDS:
						paths = self._paths(h, 4096)
					for s in done.tolist():
						i = int(holds[s])
						self.status[i] = st[s]
						if st[s, 1]:
							if paths[s, 0] < 0:
								raise _ffi.RubiksHipError(f"{self._entries}_paths: the search of state {i} met the ball, but its queue cannot be walked ({int(paths[s, 0])})")
							self.lengths[i] = paths[s, 0]
							self._queues[i] = deque(paths[s, 1:1 + paths[s, 0]].tolist())
						if keep_arrays:
							self._arrays[i] = self._export(h, s, int(st[s, 2]))
						if st[s, 5] != 5 or not self._pool_full(s, i):
							holds[s] = -1
				holds[self._deepen_poll(h, holds)] = -1
				if self.on_poll is not None:
					self.on_poll(self.status)
				late = time.perf_counter() - t0 >= time_limit
				free = np.nonzero(holds < 0)[0]
				if waiting < n and len(free) and not late:
					free = free[:n - waiting]
					took = np.arange(waiting, waiting + len(free))
					self._start(h, free, rows[took], budgets[took])
					holds[free] = took
					waiting += len(free)
					continue                    # a start the ball holds is done already: look before running
				live = holds >= 0
				if late or not live.any():
					break
				live[list(self._deep)] = False      # every pass: the burst of the slots that still pop, then one launch for the others
				if live.any():
					room = int((budgets[holds[live]] - st[live, 2]).min())
					burst = eng.burst(self.poll, room, K)
					_ffi.check(run(h, burst, stream))
					self.lockstep_iterations += burst
				if self._deep:
					self._deepen_launch(h)
			live = np.nonzero(holds >= 0)[0]
			if len(live):                       # out of time: what the searches had reached, stop reason 0; then the slots are put to rest
				for s in live.tolist():
					i = int(holds[s])
					self.status[i] = st[s]
					if keep_arrays:
						self._arrays[i] = self._export(h, s, int(st[s, 2]))
				if keep_arrays:
					for i in range(waiting, n):
						self._arrays[i] = self._export(h, 0, 0)
				self._start(h, live, np.repeat(_SOLVED20[None], len(live), axis=0), np.ones(len(live), np.int64))
			self._deep = {}
		except Exception:
			self._free()                        # slots in an unknown state: the next call starts from a new engine
			raise
		return self.lengths >= 0

	def action_queue_of(self, i: int) -> deque:
		return deque(self._queues[i])

	def arrays(self, i: int):
		"""(states, parents, actions) of the pool of state i's search, as `DeviceBallSearch.arrays()`; needs `keep_arrays`."""
		if self._arrays is None:
			raise ValueError("the pools were not kept: search(..., keep_arrays=True)")
		return self._arrays[i]

	def __len__(self):
		return int(self.status[:, 2].sum())


class DeviceBallSearchBatch(_BallSearchBatch):
	"""
	Shortest solutions of many states at once: `searches` slots, each a whole `DeviceBallSearch` of its own (pool, table,
	counters), advanced in lock-step by the same four launches with the slot in the grid's second dimension (engine
	rk_bsearchb_*, csrc/rk_ball.hip).  A single search is latency-bound -- four launches per iteration on a few per cent of the
	card --; the batch pays those launches once for all slots.  Every state gets exactly what `DeviceBallSearch` gives it alone:
	result, queue, states stored, depth, nodes popped, meeting and pool, whatever slot it ran in and whenever it was started.

	`search(states)` takes any number of states.  Slots take them in input order; every `poll` iterations the host reads all
	slots' status, records the searches that finished (their queues; their pools with `keep_arrays`) and starts the next waiting
	states in the slots that became free, so short searches do not leave the card idle beside long ones.

	The pool of a slot does not grow: `capacity` states per slot (default: `DeviceBallSearch`'s rule from the largest budget of
	the call, at most `default_capacity`).  A search whose next iteration might not fit -- states + 12 x (nodes it would pop) >
	capacity -- stops before that iteration: False, stop reason 5, `capacity_exhausted[i]` set, the other searches undisturbed.

	After a call, indexed by input position: `lengths` (-1: not met), `status` (n, 10) -- rk_bsearch_status's words: done, won,
	states, iterations, popped, stop reason, error, next pops, complete levels, meeting node --, `sizes`, `depths`, `popped`,
	`iterations`, `meeting_depths` (-1: none), `stops`, `capacity_exhausted`, `action_queue_of(i)` and `arrays(i)`.
	`on_poll(status)`, if set, is called at every poll with the status of the states seen finished so far (zeros for the others).

	`pops` = 2 048 by default is provisional, not measured yet: 64 slots x 12 x 2 048 children fill an iteration with 1.6 M threads,
	eight times a single search's 16 384 pops, while a level of a few thousand nodes still takes few iterations.
	benchmarks/ball_batch.py sweeps 512 / 2 048 / 16 384 at 16 / 64 / 256 searches and names the value it favours at 64.
	"""
	_entries = "rk_bsearchb"
	_ball_type = DeviceGoalBall

	def __init__(self, ball: DeviceGoalBall, searches: int = 64, pops: int = 2_048, capacity: int = None, poll: int = 8):
		super().__init__(ball, searches, pops, capacity, poll)

	def __str__(self):
		return f"Breadth-first searches to a goal ball x{self.searches} (device, radius={self.ball.radius}, pops={self.pops})"


class DeviceSymBallSearchBatch(_BallSearchBatch):
	"""
	`DeviceBallSearchBatch` on a kept `DeviceSymBall`: `searches` slots, each a whole `DeviceSymBallSearch` of its own (pool, table,
	counters, the words of the probe launch), advanced in lock-step by the same five launches with the slot in the grid's second
	dimension (engine rk_ssearchb_*, csrc/rk_sym.hip).  A single symmetry search is 2-4 iterations of five latency-bound launches
	at optimal lengths 12 and 14; the batch pays those launches once for all slots, and a slot stores so few states beside a
	radius-10 ball (thousands where the plain search stores hundreds of thousands) that the same HBM holds far more of them.
	Every state gets exactly what `DeviceSymBallSearch` gives it alone -- result, queue, states stored, depth, nodes popped, meeting
	and pool, whatever slot it ran in and whenever it was started --, hence what `DeviceBallSearchBatch` gives it on a
	`DeviceGoalBall` of the same radius but for the ball's half of the queue, which has the same length.

	The constructor, `search`, the attributes, `action_queue_of`, `arrays`, `on_poll` and the pool-full rule (stop reason 5,
	`capacity_exhausted[i]`) are `DeviceBallSearchBatch`'s.  `meeting_depths` comes from the symmetry ball's level boundaries;
	`meeting_nodes` (status word 9) is the node in the ball of the REPRESENTATIVE of the state every search met, 0 for none.

	`deepen=E` > 0: a slot whose pool is full goes on as `DeviceSymBallSearch(deepen=E)` does, beside the slots that
	still pop, and every state gets bit for bit what that agent gives it alone in a pool of the slot's size.  A slot then pops only
	as many nodes as surely fit and ends its pool phase when not even one does, so its pool and levels are those of `pops=1`.
	Rounds e = 1..E probe every word of e moves behind the nodes of its newest complete level L; the first round with a hit
	answers with the lowest node that has a hit and that node's lowest word, a queue of the optimal length L + e + radius.  All
	deepening slots share one probe launch per poll, of at most `ball._launch_cap()` probes; slots may be in different rounds in
	it, and how the cap is shared shows in no result.  `search` returns `lengths >= 0`; `deepened` (n,) is the round that answered
	(0: the pool sufficed, or nothing answered), `probes` the probes the call issued.  `status[i]` of a deepened state is what
	the pool phase left -- not won, stop reason 5, no meeting --, `arrays(i)` its pool with the partial next level, and
	`iterations[i]` depends on `pops`.  A search that a meeting, its budget or an exhausted graph ends is never deepened.

	`pops` = 2 048 by default is provisional, taken over from `DeviceBallSearchBatch`.  benchmarks/symball_search_batch.py sweeps
	512 / 2 048 / 16 384 at 16 / 64 / 256 searches and names the value it favours at 64 on its mixed set; its one run so far
	(profiles/r16_symball_search_batch.json) is no reason to move: the mixed set, whose time is that of its 16-move starts, favours
	16 384 by 3 %, while 12- and 14-move starts run twice as fast at 512 or 2 048 as at 16 384.
	"""
	_entries = "rk_ssearchb"
	_ball_type = DeviceSymBall
	_NO_KEY = 0xFFFFFFFFFFFFFFFF            # rk_sdeepenb_keys: no hit

	def __init__(self, ball: DeviceSymBall, searches: int = 64, pops: int = 2_048, capacity: int = None, poll: int = 8, deepen: int = 0):
		self.deepen = eng.int_in("deepen", deepen, 0, DeviceSymBall.MAX_EXTRA)
		super().__init__(ball, searches, pops, capacity, poll)

	def _results(self, n: int, keep_arrays: bool):
		super()._results(n, keep_arrays)
		self.deepened = np.zeros(n, np.int64)
		self.probes = 0
		self._sent = []                     # (slot, round) of the jobs of the launch in flight

	meeting_nodes = property(lambda self: self.status[:, 9])

	def _prepare(self, h):
		_ffi.check(_ffi.lib().rk_sdeepenb_set(h, int(self.deepen > 0)))       # the pool-full rule of the slots this call starts; no launch

	def _pool_full(self, s: int, i: int) -> bool:
		if not self.deepen:
			return False
		self._deep[s] = None                # its cursor is made at this poll, once the frontiers are read
		return True

	def _deepen_poll(self, h, holds: np.ndarray) -> list:
		if not self._deep:
			return []
		stream = _ffi.stream_ptr()
		if any(c is None for c in self._deep.values()):
			level = np.zeros((self.searches, 2), np.int64)
			_ffi.check(_ffi.lib().rk_sdeepenb_frontiers(h, level.ctypes.data, stream))
			for s, c in self._deep.items():
				if c is None:                   # round, next node, next word, the frontier, "the next job starts a round"
					lo, hi = level[s].tolist()
					self._deep[s] = [1, lo, 0, lo, hi, 1]
		if not self._sent:
			return []
		keys = np.zeros(self.searches, np.uint64)
		_ffi.check(_ffi.lib().rk_sdeepenb_keys(h, keys.ctypes.data, stream))
		# After any launch a key is final: the nodes below the job's were probed with all their words and had no hit, and the job
		# was either whole nodes with all their words or one node's words in rising order.
		hits = [(s, e, int(keys[s]) >> 32, int(keys[s]) & 0xFFFFFFFF) for s, e in self._sent if int(keys[s]) != self._NO_KEY]
		over = [s for s, e in self._sent if int(keys[s]) == self._NO_KEY and self._deep[s][0] > self.deepen]      # no round up to `deepen` hit
		self._sent = []
		if hits:
			paths = self._deepen_paths(h, hits, self.PATH_WORDS)
			if paths[:, 0].max() > self.PATH_WORDS:
				paths = self._deepen_paths(h, hits, 4096)
			for (s, e, node, rank), row in zip(hits, paths):
				i = int(holds[s])
				if row[0] < 0:
					raise _ffi.RubiksHipError(f"rk_sdeepenb_paths: word {rank} of {e} moves from node {node} of state {i} cannot be walked ({int(row[0])})")
				self.lengths[i] = row[0]
				self._queues[i] = deque(row[1:1 + row[0]].tolist())
				self.deepened[i] = e
		finished = [s for s, *_ in hits] + over
		for s in finished:
			del self._deep[s]
		return finished

	def _deepen_paths(self, h, hits: list, max_len: int) -> np.ndarray:
		slots, extras, nodes, ranks = (np.array(col, dtype) for col, dtype in zip(zip(*hits), (np.int32, np.int32, np.int64, np.uint32)))
		out = np.zeros((len(hits), 1 + max_len), np.int32)
		_ffi.check(_ffi.lib().rk_sdeepenb_paths(h, len(hits), slots.ctypes.data, nodes.ctypes.data, extras.ctypes.data, ranks.ctypes.data, out.ctypes.data,
		                                       max_len, _ffi.stream_ptr()))
		return out

	def _deepen_launch(self, h):
		"""One launch for the deepening slots: the cap on the probes of a launch is shared out evenly; a slot's job is as many whole
		nodes with all their words as its share takes, or, where not even one node's words fit, the next words of one node."""
		cap = self.ball._launch_cap()
		slots = sorted(self._deep)[:cap]
		share = cap // len(slots)
		jobs = np.zeros((len(slots), 8), np.uint32)                          # rk_deepen_job_t
		for j, s in enumerate(slots):
			e, at, first, lo, hi, new = self._deep[s]
			words = (12 if lo == 1 else 11) * 11 ** (e - 1)                 # (node 1 has no last move; it is a level of its own)
			if first == 0 and share >= words:
				nodes, count = min(share // words, hi + 1 - at), words
			else:
				nodes, count = 1, min(share, words - first)
			jobs[j] = (s, e, at, nodes, first, count, new, 0)
			self.probes += nodes * count
			self._sent.append((s, e))
			at, first = (at + nodes, 0) if first + count == words else (at, first + count)
			self._deep[s] = [e + 1, lo, 0, lo, hi, 1] if at > hi else [e, at, first, lo, hi, 0]
		_ffi.check(_ffi.lib().rk_sdeepenb_probe(h, len(slots), jobs.ctypes.data, _ffi.stream_ptr()))

	def __str__(self):
		return (f"Breadth-first searches to a symmetry-reduced goal ball x{self.searches} (device, radius={self.ball.radius}, "
		        f"pops={self.pops})")


class PolicySearch(DeepAgent):
	"""Follow (or sample from) the policy head (agents.py:132-151)."""
	def __init__(self, net, sample_policy=False):
		super().__init__(net)
		self.sample_policy = sample_policy

	def _step(self, state):
		logits = self.net(cube.as_oh(state), value=False)
		policy = _host_softmax(logits.float().cpu()).numpy().squeeze()
		action = int(np.random.choice(cube.action_dim, p=policy)) if self.sample_policy else int(policy.argmax())
		state = cube.rotate(state, *cube.action_space[action])
		return action, state, cube.is_solved(state)

	@classmethod
	def from_saved(cls, loc: str, use_best: bool, sample_policy=False, loader=None):
		return cls(_load_net(loc, use_best, loader), sample_policy)

	def __str__(self):
		return f"{'Sampled' if self.sample_policy else 'Greedy'} policy"


class ValueSearch(DeepAgent):
	"""Greedy one-step look-ahead on the value head (agents.py:154-169); one fan-out launch per step."""
	def _step(self, state):
		children, solved = cube.expand(np.asarray(state)[None], return_solved=True)
		if solved.any():
			action = int(np.flatnonzero(solved)[0])
			return action, children[action], True
		v = self.net(cube.as_oh(children), policy=False).float().squeeze().cpu().numpy()
		action = int(np.argmax(v))
		return action, children[action], False

	def __str__(self):
		return "Greedy value"


class EGVM(DeepAgent):
	"""Epsilon-greedy value maximisation (agents.py:649-726): `workers` walkers of `depth` moves, restart from the best."""
	def __init__(self, net, epsilon: float, workers: int, depth: int):
		super().__init__(net)
		self.epsilon, self.workers, self.depth = epsilon, workers, depth

	@no_grad
	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		time_limit, max_states = self.reset(time_limit, max_states)
		t0 = time.perf_counter()
		if cube.is_solved(state):
			return True
		while time.perf_counter() - t0 < time_limit and len(self) + self.workers * self.depth <= max_states:
			paths, states, states_oh, solved = self.expand(state)
			if solved != (-1, -1):
				self.action_queue += deque(int(a) for a in paths[solved[0], :solved[1]])
				return True
			best = int(self.net(states_oh, policy=False).float().cpu().squeeze().argmax())
			state = states[best]
			worker, d = divmod(best, self.depth)
			self.action_queue += deque(int(a) for a in paths[worker, :d + 1])
		return False

	def _oh(self, rows: torch.Tensor) -> torch.Tensor:
		"""The float32 one-hot of 20-byte rows in the representation of the search (agents.py:697, :709: cube.as_oh)."""
		return cube.device.as_oh(rows) if self._is2024 else cube.device.to686(rows, torch.float32)

	def expand(self, state: np.ndarray):
		"""Walks all workers `depth` moves on the device; row w*depth + d = worker w after d+1 moves.  In 6x8x6 mode the walks run in
		20-byte form (the same draws), the net sees 288-wide rows and the states come back as (6, 8, 6)."""
		self._is2024 = cube.get_is2024()
		root = self._roots20(state, 1)[0]
		cur = torch.from_numpy(cube.repeat_state(root, self.workers)).to(gpu)
		paths = np.empty((self.workers, self.depth), dtype=int)
		visited = torch.empty((self.workers, self.depth, 20), dtype=torch.int8, device=gpu)
		flags = torch.empty(self.workers, dtype=torch.uint8, device=gpu)
		stats0 = torch.tensor([0, _ffi.INT64_MAX], dtype=torch.int64, device=gpu)
		stats = torch.empty_like(stats0)
		for d in range(self.depth):
			use_random = np.random.choice(2, self.workers, p=[1 - self.epsilon, self.epsilon]).astype(bool)
			actions = np.empty(self.workers, dtype=int)
			actions[use_random] = np.random.randint(0, cube.action_dim, use_random.sum())
			if (~use_random).any():
				p = self.net(self._oh(cur[torch.from_numpy(~use_random).to(gpu)].contiguous()), value=False).float().cpu().numpy()
				actions[~use_random] = p.argmax(axis=1)
			paths[:, d] = actions
			# move + goal test in one launch (agents.py:696-703); the host reads the two statistics words, not the flags
			stats.copy_(stats0)
			acts = torch.from_numpy(actions.astype(np.uint8)).to(gpu)
			nxt = torch.empty_like(cur)              # the walk is in 20-byte form whatever the repr: REPR_2024 explicitly
			_ffi.check(_ffi.lib().rk_multi_rotate_solved(_ffi.REPR_2024, cur.data_ptr(), acts.data_ptr(), nxt.data_ptr(), flags.data_ptr(),
			                                             stats.data_ptr(), self.workers, _ffi.stream_ptr()))
			cur = nxt
			hit = stats.cpu()
			if int(hit[0]):
				self._explored_states += (d + 1) * self.workers
				return paths, None, None, (int(hit[1]), d + 1)
			visited[:, d] = cur
		self._explored_states += self.workers * self.depth
		flat = visited.reshape(self.workers * self.depth, 20)
		return paths, (flat.cpu().numpy() if self._is2024 else cube.as686(flat).cpu().numpy()), self._oh(flat), (-1, -1)

	@classmethod
	def from_saved(cls, loc: str, use_best: bool, epsilon: float, workers: int, depth: int, loader=None):
		return cls(_load_net(loc, use_best, loader), epsilon=epsilon, workers=workers, depth=depth)

	def __str__(self):
		return f"EGVM (e={self.epsilon}, w={self.workers}, d={self.depth})"


def egvm_draw_round(epsilon: float, workers: int, depth: int) -> np.ndarray:
	"""The epsilon-greedy draws of `depth` moves of one EGVM walk, made with the reference's calls in the reference's order on the
	global NumPy generator (agents.py:694, :698) -- both calls at every depth, also when nobody acts at random.  -> int8
	(depth, workers): the action 0..11 where the reference acts at random, -1 where it follows the policy."""
	table = np.full((depth, workers), -1, np.int8)
	for d in range(depth):
		use_random = np.random.choice(2, workers, p=[1 - epsilon, epsilon]).astype(bool)
		table[d, use_random] = np.random.randint(0, cube.action_dim, use_random.sum())
	return table


def egvm_draw_rounds(epsilon: float, workers: int, depth: int, rounds: int):
	"""`rounds` full rounds of draws ahead of the device -> (int8 (rounds, depth, workers), the generator's state before each round)."""
	table, before = np.empty((rounds, depth, workers), np.int8), []
	for r in range(rounds):
		before.append(np.random.get_state())
		table[r] = egvm_draw_round(epsilon, workers, depth)
	return table, before


def egvm_rewind(before_round, epsilon: float, workers: int, moves: int) -> np.ndarray:
	"""A search that ended by a solve after `moves` moves of a round: the reference returned inside that walk (agents.py:710-713)
	and drew nothing further.  Back to the generator's state before the round, then the draws of those moves again: the global
	generator is left exactly where the reference leaves it."""
	np.random.set_state(before_round)
	return egvm_draw_round(epsilon, workers, moves)


class _KeptGraph:
	"""One kept hipGraph of an agent that keeps several (what _engine.kept_graph reads and writes of its agent)."""
	def __init__(self):
		self._graph_cache, self.captures = None, 0


class _NetStepped(DeepAgent, _ffi.Owner):
	"""
	What the agents of the net-stepped engines share (rk_egvm_*, rk_greedy_*, rk_beam_*, rk_beamb_*; the engines' side is at the end of
	csrc/rk_search_host.h).  The ENGINE owns the net's batch in HBM, one buffer per RK_OH_* form; `_batch` = (code, tensor, ...)
	wraps the form the net wants now.  A step -- a net forward on that batch plus the engine's launches -- is captured once as a
	hipGraph and kept from search to search in a holder that `_engine.kept_graph` writes to (`_holders`: the agent itself, or one
	`_KeptGraph` per step of an agent with several).  The host replays `poll` steps, then reads a counter block: each agent's own loop.
	"""
	_batch = None
	_graph_cache, captures = None, 0

	@staticmethod
	def _strict_ints(*args) -> list:
		"""(name, value, top), ...: the values as ints.  Only an int / np.integer in 1..top will do: no bool, no 2.0 (`_engine.int_in` takes it)."""
		for name, v, top in args:
			if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= top:
				raise ValueError(f"{name} must be an integer in 1..{top}, got {v!r}")
		return [int(v) for _, v, _ in args]

	def _holders(self) -> tuple:
		return (self,)

	def _free(self):
		for g in self._holders():
			g._graph_cache = None              # the graphs hold the engine's addresses,
		self._batch = None                     # and the batches are the engine's memory: both go before the engine does
		super()._free()

	def _net_batches(self, h, code: int, *calls) -> tuple:
		"""The engine's batches in form `code` as tensors, one per call (entry, *arguments between the handle and the code)."""
		if self._batch is None or self._batch[0] != code:
			got = []
			for entry, *lead in calls:
				ptr, rows = C.c_void_p(), C.c_size_t()
				_ffi.check(entry(h, *lead, code, C.byref(ptr), C.byref(rows)))
				got.append(eng.engine_batch(ptr.value, rows.value, code))
			self._batch = (code, *got)         # (the engine goes on writing the form it was asked for last)
		return self._batch[1:]

	def _kept_steps(self, key: tuple, forward, reset, *steps) -> list:
		"""The hipGraphs of `steps`, each (holder, step, batch), kept or captured now.  A captured step holds addresses (the engine's
		arrays and batches, the net's tensors) and dtype codes -- nothing of a search, which lives in device memory that `reset`, the
		engine's reset for the search that starts, rewrites: the graphs are kept while `key`, everything they hold, stays the same.
		A step is captured on an engine that has been reset, and what the warm-up's launches change there the last reset rewrites."""
		if any(g._graph_cache is None or g._graph_cache[0] != key for g, _, _ in steps):
			reset()
		graphs = [eng.kept_graph(g, key, step, step, batch, ((self.net, forward),))[0] for g, step, batch in steps]
		reset()
		return graphs


class DeviceEGVM(_NetStepped):
	"""
	Epsilon-greedy value maximisation (agents.py:649-726) with the whole round on the device (engine rk_egvm_*, csrc/rk_egvm.hip):
	the walkers, the states they visit, their actions and the two net batches live in HBM.  One move of all walkers is the policy
	forward and one launch (argmax or drawn action, move, goal test, the rows of both net batches); a round ends with the value
	forward and one launch (the solve, or the argmax over the workers x depth values, the new root and the loop guard).  Both are
	captured once as hipGraphs and kept from search to search; the host enqueues `poll` rounds, then reads the status and the
	rounds' action records.  The epsilon draws stay on the host: they depend on nothing the device computes, and made with the
	reference's calls in the reference's order (egvm_draw_rounds) they leave the action queue, len(agent) and the global NumPy
	generator exactly as the reference does -- a search that ends by a solve rewinds the generator to where the reference stopped
	drawing (egvm_rewind), and no more than max_states // (workers * depth) rounds are ever drawn.

	Two differences from the reference.  The time limit is checked where the host polls (before every `poll` rounds), not before
	every round, so a time-limited search does not stop where the reference would.  And the policy forward runs on ALL workers,
	not on the subset that follows the policy (agents.py:700): for a net whose GEMM results depend on the batch size in the last
	bit, a near-tie between two logits may resolve differently.

	The representation follows cube.get_is2024() when a search starts (6x8x6 nets read the engine's 20-byte rows through _Net686).
	"""
	MAX_WORKERS, MAX_DEPTH, MAX_POLL = 1 << 16, 1 << 12, 1 << 12          # rk_egvm_create's limits
	MAX_STATES = 1 << 22                                                    # ... on workers * depth

	def __init__(self, net, epsilon: float, workers: int, depth: int, poll: int = 4, fused_first_layer=False):
		super().__init__(net, fused_first_layer)
		workers, depth, poll = self._strict_ints(("workers", workers, self.MAX_WORKERS), ("depth", depth, self.MAX_DEPTH), ("poll", poll, self.MAX_POLL))
		if workers * depth > self.MAX_STATES:
			raise ValueError(f"workers * depth must not exceed {self.MAX_STATES}, got {workers * depth}")
		if workers * depth * poll > 1 << 28:
			raise ValueError(f"workers * depth * poll must not exceed {1 << 28}, got {workers * depth * poll}")
		if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float, np.floating, np.integer)) or not 0 <= float(epsilon) <= 1:
			raise ValueError(f"epsilon must be a number in 0..1, got {epsilon!r}")
		self.epsilon, self.workers, self.depth, self.poll = epsilon, workers, depth, poll
		self._shape = None
		self._walk, self._close = _KeptGraph(), _KeptGraph()       # policy forward + rk_egvm_step; value forward + rk_egvm_round_end
		self.rounds = 0                                            # rounds the last search closed

	@property
	def captures(self) -> int:
		"""hipGraph captures so far (a search on an unchanged engine and net replays the previous search's two graphs)."""
		return self._walk.captures + self._close.captures

	# -- engine lifetime ------------------------------------------------------------------------------------
	def _engine(self):
		shape = (self.workers, self.depth, self.poll)
		if self._h is None or self._shape != shape:
			self._create("rk_egvm_create", "rk_egvm_destroy", *shape)
			self._shape = shape
		return self._h

	def _holders(self) -> tuple:
		return self._walk, self._close

	# -- the two captured steps -------------------------------------------------------------------------------
	def _walk_step(self, h, pol_in):
		logits, code = eng.engine_logits(self._forward(pol_in, policy=True, value=False))
		self._keep_p = logits              # the kernel reads it after this call returns
		_ffi.check(_ffi.lib().rk_egvm_step(h, logits.data_ptr(), code, _ffi.stream_ptr()))

	def _close_step(self, h, val_in):
		values, code = eng.engine_values(_sliced_value_forward(self._forward, val_in))
		self._keep_v = values
		_ffi.check(_ffi.lib().rk_egvm_round_end(h, values.data_ptr(), code, _ffi.stream_ptr()))

	# -- search -------------------------------------------------------------------------------------------------
	@no_grad
	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		_ffi.require_gpu()
		t0 = time.perf_counter()
		time_limit, max_states = self.reset(time_limit, max_states)
		self.rounds = 0
		forward, _, code = self._begin_net()
		root = self._roots20(state, 1)[0]                      # ValueError for an illegal 6x8x6 state
		if (root == _SOLVED20).all():
			return True
		W, D = self.workers, self.depth
		max_rounds = int(max_states) // (W * D)                # the loop guard of agents.py:665 holds for exactly this many rounds
		if max_rounds == 0:
			return False
		lib, stream = _ffi.lib(), _ffi.stream_ptr()
		h = self._engine()
		pol_in, val_in = self._net_batches(h, code, (lib.rk_egvm_net_in, 0), (lib.rk_egvm_net_in, 1))
		key = (h.value, code, pol_in.data_ptr(), val_in.data_ptr(), eng.capture_key(self.net, forward))
		reset = lambda: _ffi.check(lib.rk_egvm_reset(h, root.ctypes.data, int(max_states), stream))       # noqa: E731
		walk, close = self._kept_steps(key, forward, reset, (self._walk, lambda: self._walk_step(h, pol_in), pol_in),
		                               (self._close, lambda: self._close_step(h, val_in), val_in))
		status = (C.c_longlong * 8)()
		drawn = 0
		while time.perf_counter() - t0 < time_limit:
			n = min(self.poll, max_rounds - drawn)             # >= 1: the engine is done when round max_rounds closes
			draws, before = egvm_draw_rounds(self.epsilon, W, D, n)
			_ffi.check(lib.rk_egvm_set_draws(h, draws.ctypes.data, n, stream))
			for _ in range(n):
				for _ in range(D):
					walk.replay()
				close.replay()
			_ffi.check(lib.rk_egvm_status(h, status, stream))
			done, solved, rounds, explored, _, moves, err = (int(status[i]) for i in range(7))
			if err:
				raise _ffi.RubiksHipError(f"EGVM engine error code {err}")
			closed = rounds - drawn                            # rounds of this burst that ran
			if closed > 0:
				rec = np.zeros((closed, D + 2), np.int64)
				_ffi.check(lib.rk_egvm_records(h, drawn, closed, rec.ctypes.data, stream))
				for row in rec:
					self.action_queue.extend(int(a) for a in row[2:2 + int(row[0])])         # agents.py:670, :677
			self.rounds, self._explored_states = rounds, explored
			if solved:
				egvm_rewind(before[closed - 1], self.epsilon, W, moves)
				return True
			drawn += n
			if done:
				return False
		return False

	@classmethod
	def from_saved(cls, loc: str, use_best: bool, epsilon: float, workers: int, depth: int, loader=None):
		return cls(_load_net(loc, use_best, loader), epsilon=epsilon, workers=workers, depth=depth)

	def __str__(self):
		return f"EGVM (device, e={self.epsilon}, w={self.workers}, d={self.depth})"


class GreedyBatch(_NetStepped):
	"""
	Up to `games` independent games of a one-step agent advanced in lock-step on the device (engine rk_greedy_*,
	csrc/rk_greedy.hip): `mode` "policy" plays every game as `PolicySearch(net)` does (greedy, agents.py:138-142), "value" as
	`ValueSearch(net)` does (agents.py:156-166).  The games' states, status, move counts, actions and the net batch live in HBM; a
	move of all games is one net forward on `games` (policy) or 12 x `games` (value) rows and one launch, captured once as a
	hipGraph and kept from search to search.  The host enqueues `poll` moves (never more than the budget has left), then reads the
	number of running games; games that have ended are skipped on the device and keep their rows, so the net's batch never
	changes shape.

	Every game follows THIS repository's host agents, which differ from the reference in one respect: their loop counts a game's
	moves against `max_states` at every step (Agent.search above), so a game that is not solved after `max_states` moves ends with
	status 2.  In the reference len(self) stays 0 until search returns (agents.py:30-38), so `max_states` never stops a one-step
	agent there -- only the time limit does.  `max_states` is required here: it sizes the action record.  The time limit is
	checked where the host polls, not before every move.

	Policy mode takes the first maximum of the logits where the host agent takes argmax(softmax(logits)) on the CPU.  Where the two
	might differ -- a logit less than 2^-20 below the maximum, a NaN logit, an infinite maximum; csrc/rk_greedy.hip has the proof
	that nothing else can -- the engine does not move the game: it gets status 3 and is listed in `handed_back`, for the caller
	to play on the host (`Evaluator` does).  With a real-valued net a forward on `games` rows need not equal a forward on one row bit
	for bit, so a near-tie between two logits or values may resolve differently than in a game played alone; with nets whose
	outputs are exact the games are the host agents' move for move.

	Not here: `PolicySearch(sample_policy=True)` and `RandomSearch` draw from the global NumPy generator once per move, and the
	number of draws a game makes decides where the next game's scramble is drawn from; such games cannot advance together and
	leave the reference's stream of draws intact, so they stay sequential.

	After a search: `status` (0 still running when the time ran out, 1 solved, 2 budget spent, 3 handed back), `steps`,
	`action_queue_of(i)`, `handed_back`; len(agent) is the sum of `steps`.  The representation follows cube.get_is2024() when a
	search starts (6x8x6 nets read the engine's 20-byte rows through _Net686).
	"""
	MODES = {"policy": 0, "value": 1}
	MAX_GAMES, MAX_POLL = 1 << 16, 1 << 12
	MAX_RECORD = 1 << 30                                                    # rk_greedy_create's limit on games * max_states

	def __init__(self, net, mode: str, games: int, poll: int = 8, fused_first_layer=False):
		super().__init__(net, fused_first_layer)
		if not isinstance(mode, str) or mode not in self.MODES:
			raise ValueError(f'mode is "policy" or "value", got {mode!r}')
		self.games, self.poll = self._strict_ints(("games", games, self.MAX_GAMES), ("poll", poll, self.MAX_POLL))
		self.mode = mode
		self._room = 0                                                      # the moves per game the engine has room for
		self.status = np.zeros(0, np.int64)
		self.steps = np.zeros(0, np.int64)
		self._actions = np.zeros((0, 0), np.uint8)
		self.launched = 0                                                   # moves the last search enqueued
		self.on_poll = None                                                 # callable(status): called with every per-game status the search reads

	# -- engine lifetime ------------------------------------------------------------------------------------
	def _budget(self, max_states) -> int:
		if max_states is None:
			raise ValueError("GreedyBatch needs max_states: it sizes every game's action record")
		if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or int(max_states) < 1:
			raise ValueError(f"max_states must be a positive integer, got {max_states!r}")
		if self.games * int(max_states) > self.MAX_RECORD:
			raise ValueError(f"games * max_states must not exceed {self.MAX_RECORD}, got {self.games * int(max_states)}")
		return int(max_states)

	def _engine(self, max_states: int):
		if self._h is None or self._room < max_states:
			self._create("rk_greedy_create", "rk_greedy_destroy", self.games, max_states, self.MODES[self.mode])
			self._room = max_states
		return self._h

	# -- the captured step: [net forward, rk_greedy_step] ---------------------------------------------------------
	def _move(self, h, batch):
		if self.mode == "policy":
			out, code = eng.engine_logits(self._forward(batch, policy=True, value=False))
		else:
			out, code = eng.engine_values(_sliced_value_forward(self._forward, batch))
		self._keep = out                       # the kernel reads it after this call returns
		_ffi.check(_ffi.lib().rk_greedy_step(h, out.data_ptr(), code, _ffi.stream_ptr()))

	def _read(self, h, n: int, actions: bool):
		self.status, self.steps = np.zeros(n, np.int64), np.zeros(n, np.int64)
		if actions:
			self._actions = np.zeros((n, self._max_states), np.uint8)
		_ffi.check(_ffi.lib().rk_greedy_export(h, self.status.ctypes.data, self.steps.ctypes.data, self._actions.ctypes.data if actions else None,
		                                       _ffi.stream_ptr()))
		self._explored_states = int(self.steps.sum())

	# -- search -------------------------------------------------------------------------------------------------
	@no_grad
	def search(self, states: np.ndarray, time_limit: float = None, max_states: int = None) -> np.ndarray:
		"""Plays the games (at most `games` start states) until each is solved, has made `max_states` moves or was handed back, or
		until a poll after `time_limit`; returns the bool vector `solved` over the games."""
		max_states = self._budget(max_states)                  # before anything asks for a device
		_ffi.require_gpu()
		t0 = time.perf_counter()
		time_limit, _ = self.reset(time_limit, max_states)
		forward, _, code = self._begin_net()
		states = np.asarray(states, dtype=np.int8)
		n = states.size // (20 if self._is2024 else 288)
		if not 1 <= n <= self.games or n * (20 if self._is2024 else 288) != states.size:
			raise ValueError(f"between 1 and {self.games} start states are played at once, got an array of shape {states.shape}")
		roots = self._roots20(states, n)                       # ValueError for an illegal 6x8x6 state
		self._max_states, self.launched = max_states, 0
		self.status, self.steps, self._actions = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, 0), np.uint8)
		lib, stream = _ffi.lib(), _ffi.stream_ptr()
		h = self._engine(max_states)
		batch, = self._net_batches(h, code, (lib.rk_greedy_net_in,))
		key = (h.value, code, batch.data_ptr(), self.mode, self.games, eng.capture_key(self.net, forward))
		reset = lambda: _ffi.check(lib.rk_greedy_reset(h, roots.ctypes.data, n, max_states, stream))      # noqa: E731
		graph, = self._kept_steps(key, forward, reset, (self, lambda: self._move(h, batch), batch))
		status = (C.c_longlong * 8)()
		running = int((roots != _SOLVED20).any(axis=1).sum())
		while running and self.launched < max_states and time.perf_counter() - t0 < time_limit:
			burst = min(self.poll, max_states - self.launched)  # a running game moves at every launch: none is left after max_states of them
			for _ in range(burst):
				graph.replay()
			self.launched += burst
			_ffi.check(lib.rk_greedy_status(h, status, stream))
			running, err = int(status[0]), int(status[2])
			if err:
				raise _ffi.RubiksHipError(f"greedy engine error code {err}")
			if self.on_poll is not None:
				self._read(h, n, False)
				self.on_poll(self.status)
		self._read(h, n, True)
		if self.on_poll is not None:
			self.on_poll(self.status)
		return self.status == 1

	@property
	def handed_back(self) -> np.ndarray:
		"""Indices of the games the engine would not decide (status 3): play them with the host agent."""
		return np.flatnonzero(self.status == 3)

	def action_queue_of(self, game: int) -> deque:
		return deque(int(a) for a in self._actions[game, :int(self.steps[game])])

	def __str__(self):
		return f"Greedy {self.mode} x{self.games} (device)"


class DeviceBeamSearch(_NetStepped):
	"""
	Beam search guided by the net's value head, higher is better as in `ValueSearch` (engine rk_beam_*, csrc/rk_beam.hip): every
	depth keeps the best `width` states.  The beam, the `back` record, the sizes, the dedup table and the net batch live in HBM; a
	depth is one net forward on the 12 x `width` rows of a batch that never changes shape and a fixed sequence of launches that
	read everything data-dependent from device counters, captured once as a hipGraph and kept from search to search.  The host
	enqueues `poll` depths, then reads the status; after a stop a replay writes nothing.  With `ball`, a built `DeviceSymBall`, the
	search ends at the first child whose orbit the ball holds and the ball's descent finishes the queue, so the beam has to get
	only within `ball.radius` quarter turns of solved; a start whose orbit the ball holds is answered at the reset.

	Depth t holds a beam F_t of m_t <= width states in a fixed order, F_0 the start; child c = 12 i + a is member i under action a.
	  1. With `prune_inverse`, child (i, a) is dead when a is the inverse (action ^ 1) of the action that made member i.
	  2. With n_live live children: explored + n_live > max_states stops the search (status 2), else explored += n_live.
	  3. The live child that is solved -- with a ball: whose orbit the ball holds -- with the least (ball depth, c) wins (status 1).
	  4. Of live children with equal states only the lowest c survives.  There is NO dedup across depths: a state may come back at
	     a later depth (the engine keeps no state but the current beam's), and `prune_inverse` removes only the two-move returns.
	  5. The best min(width, survivors) -- larger value first, any NaN above every number, -0.0 equal to +0.0, ties to the lower
	     c, bfloat16 values widened exactly -- form F_{t+1}, stored in ascending c; back[t + 1][j] = i << 4 | a.
	  6. t + 1 == max_depth stops the search (status 3).
	Status 0 is a search that was still running when `time_limit` passed; the time limit is checked only where the host polls.

	After a search: `status`, `depth` (the depths run), `sizes` (m_t of every beam formed), `back_of(t)`, `meeting` = (i, a, ball
	depth) of the winning child (a = -1: the start itself, inside the ball); len(agent) is the states explored.  With a real-valued
	net a forward on 12 x width rows need not equal a forward on other rows bit for bit, so which of two nearly equal values is
	kept may depend on the width.  The representation follows cube.get_is2024() when a search starts (6x8x6 nets read the engine's
	20-byte rows through _Net686).
	"""
	MAX_WIDTH, MAX_DEPTH, MAX_POLL = 1 << 16, 1 << 12, 1 << 12              # rk_beam_create's limits

	def __init__(self, net, width: int, max_depth: int = 64, ball: DeviceSymBall = None, prune_inverse: bool = True, poll: int = 8,
	             fused_first_layer=False):
		super().__init__(net, fused_first_layer)
		self.width, self.max_depth, self.poll = self._strict_ints(("width", width, self.MAX_WIDTH), ("max_depth", max_depth, self.MAX_DEPTH),
		                                                          ("poll", poll, self.MAX_POLL))
		if ball is not None and not (isinstance(ball, DeviceSymBall) and ball.built):
			raise ValueError(f"ball must be None or a built DeviceSymBall (call ball.build() first), got {ball!r}")
		self.ball, self.prune_inverse = ball, bool(prune_inverse)
		self._clear()

	def _clear(self):
		self.status, self.depth, self.meeting = 0, 0, None
		self.sizes = np.ones(1, np.int64)

	def reset(self, time_limit: float, max_states: int):
		"""As Agent.reset, but neither limit is required: a beam search ends by itself after max_depth depths."""
		self._explored_states = 0
		self.action_queue = deque()
		self.net.eval()
		return time_limit or 1e10, max_states

	# -- engine lifetime ------------------------------------------------------------------------------------
	def _engine(self):
		if self._h is None:
			self._create("rk_beam_create", "rk_beam_destroy", self.ball._h if self.ball is not None else None, self.width, self.max_depth,
			             int(self.prune_inverse))
		return self._h

	# -- the captured step: [net forward, rk_beam_step] -----------------------------------------------------------
	def _depth_step(self, h, batch):
		values, code = eng.engine_values(_sliced_value_forward(self._forward, batch))
		self._keep = values                    # the kernels read it after this call returns
		_ffi.check(_ffi.lib().rk_beam_step(h, values.data_ptr(), code, _ffi.stream_ptr()))

	def _poll(self, h):
		status = (C.c_longlong * 12)()
		_ffi.check(_ffi.lib().rk_beam_status(h, status, _ffi.stream_ptr()))
		return [int(x) for x in status]

	# -- search -------------------------------------------------------------------------------------------------
	@no_grad
	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		state = np.asarray(state)
		if state.shape != tuple(cube.shape()):                  # before anything asks for a device
			raise ValueError(f"the start is one state of shape {tuple(cube.shape())}, got an array of shape {state.shape}")
		if max_states is not None and (isinstance(max_states, bool) or int(max_states) != max_states or int(max_states) < 0):
			raise ValueError(f"max_states must be a non-negative integer or None, got {max_states!r}")
		_ffi.require_gpu()
		t0 = time.perf_counter()
		time_limit, _ = self.reset(time_limit, max_states)
		self._clear()
		forward, _, code = self._begin_net()
		root = self._roots20(state, 1)[0]                      # ValueError for an illegal 6x8x6 state
		if (root == _SOLVED20).all():
			self.status = 1                                    # (no launch: nothing met, no depth run)
			return True
		budget = _ffi.INT64_MAX if max_states is None else int(max_states)
		lib, stream = _ffi.lib(), _ffi.stream_ptr()
		h = self._engine()
		batch, = self._net_batches(h, code, (lib.rk_beam_net_in,))
		key = (h.value, code, batch.data_ptr(), eng.capture_key(self.net, forward))
		reset = lambda: _ffi.check(lib.rk_beam_reset(h, root.ctypes.data, budget, stream))                # noqa: E731
		graph, = self._kept_steps(key, forward, reset, (self, lambda: self._depth_step(h, batch), batch))
		st = self._poll(h)                                     # (a start inside the ball has won at the reset)
		launched = 0
		while st[0] == 0 and launched < self.max_depth and time.perf_counter() - t0 < time_limit:
			burst = min(self.poll, self.max_depth - launched)  # a running search advances at every replay: none is after max_depth of them
			for _ in range(burst):
				graph.replay()
			launched += burst
			st = self._poll(h)
		self.status, self.depth, self._explored_states = st[0], st[1], st[2]
		if st[0] == 4 or st[4]:
			raise _ffi.RubiksHipError(f"beam engine error code {st[4]}")
		sizes = np.zeros(self.max_depth + 1, np.int64)
		_ffi.check(lib.rk_beam_export(h, 0, sizes.ctypes.data, None, 0, stream))
		self.sizes = sizes[:st[9] + 1].copy()
		if st[0] != 1:
			return False
		self.meeting = (st[5], st[6], st[7])
		self.action_queue = eng.read_path(lib.rk_beam_path, h, length=self.max_depth + 1 + DeviceSymBall.MAX_RADIUS)
		return True

	def back_of(self, t: int) -> np.ndarray:
		"""int64 (m_t,): the `back` words i << 4 | a of the beam of depth t (1 .. len(sizes) - 1) of the last search."""
		t = eng.int_in("t", t, 1, len(self.sizes) - 1)
		out = np.zeros(int(self.sizes[t]), np.int64)
		_ffi.check(_ffi.lib().rk_beam_export(self._h, t, None, out.ctypes.data, len(out), _ffi.stream_ptr()))
		return out

	def __str__(self):
		return f"Beam search (device, width={self.width}" + (f", to a symmetry ball of radius {self.ball.radius})" if self.ball is not None else ")")


class DeviceBeamSearchBatch(_NetStepped):
	"""
	Beam searches of many states at once: `searches` slots, each a whole `DeviceBeamSearch` of its own (beam, `back` record, sizes,
	dedup table, histograms, look-back words, counters), advanced in lock-step (engine rk_beamb_*, csrc/rk_beam.hip).  A depth of
	ALL slots is one value forward on the searches x 12 x `width` rows of one batch -- slot s owns rows [12 width s, 12 width (s + 1))
	-- and the single engine's sequence of launches with the slot in the grid's second dimension, captured once as a hipGraph and
	kept from call to call.  A single beam search at the usual widths is bound by the latency of its launches, not by its work; the
	batch pays the launches and the forward once for all slots.

	`search(states)` takes any number of states.  Slots take them in input order; every `poll` replayed depths (never more than the
	running slots have left of `max_depth`) the host reads all slots' status, records the searches that finished -- their queues;
	with `keep_arrays` their `sizes` and every `back` row, before the slot is used again -- and starts the next waiting states in the
	slots that became free.  A solved start is answered on the host as `DeviceBeamSearch` does (status 1, depth 0, nothing explored,
	no meeting, an empty queue) and takes no slot; a start whose orbit the ball holds is done at its slot's reset.  `max_states`: one
	budget for all, or one per state (n,), None for no budget.  `time_limit` bounds the whole call and is checked at the polls:
	searches still running or waiting when it passes come back False with status 0.  After a call, whether it returned or raised,
	no slot is running; an exception frees the engine.

	On nets whose outputs do not depend on the shape of the batch, every state gets exactly what `DeviceBeamSearch(net, width,
	max_depth, ball, prune_inverse)` gives it alone -- solved, status, depth, states explored, sizes, every `back` word, the meeting
	and the queue --, bit for bit, whatever slot it ran in, whenever it was started and whatever `searches` and `poll` are.  With a
	real-valued net a forward on searches x 12 x width rows need not equal a forward on 12 x width rows bit for bit, so a near-tie
	between two values may resolve differently than in a search run alone.

	After a call, indexed by input position: `status` (n, 12) -- rk_beam_status's words: status (0 running when the time ran out, 1
	won, 2 budget, 3 depth limit), depths run, states explored, size of the last beam, error, the winning child's member, its action
	(-1: the start itself, inside the ball) and its ball depth, the budget, the depth of the last beam --, `lengths` (-1: no queue),
	`depths`, `meetings` ((i, a, ball depth) or None), `action_queue_of(i)`, and with `keep_arrays` `sizes_of(i)` and `back_of(i, t)`.
	`on_poll(status)`, if set, is called at every poll with the status of the states seen finished so far (zeros for the others).
	`lockstep_depths` counts the depths of all slots the last call launched, `captures` the hipGraph captures so far; len(b) is the
	sum of the states explored.  The representation follows cube.get_is2024() when a call starts (6x8x6 nets read the engine's
	20-byte rows through _Net686).
	"""
	MAX_SEARCHES, MAX_WIDTH, MAX_DEPTH, MAX_POLL = 1 << 10, 1 << 16, 1 << 12, 1 << 12      # rk_beamb_create's limits
	MAX_BEAMS = 1 << 16                                                                   # ... on searches * width

	def __init__(self, net, width: int, searches: int = 64, max_depth: int = 64, ball: DeviceSymBall = None, prune_inverse: bool = True,
	             poll: int = 8, fused_first_layer=False):
		super().__init__(net, fused_first_layer)
		self.width, self.searches, self.max_depth, self.poll = self._strict_ints(
			("width", width, self.MAX_WIDTH), ("searches", searches, self.MAX_SEARCHES), ("max_depth", max_depth, self.MAX_DEPTH),
			("poll", poll, self.MAX_POLL))
		if self.searches * self.width > self.MAX_BEAMS:
			raise ValueError(f"searches * width must not exceed {self.MAX_BEAMS}, got {self.searches * self.width}")
		if ball is not None and not (isinstance(ball, DeviceSymBall) and ball.built):
			raise ValueError(f"ball must be None or a built DeviceSymBall (call ball.build() first), got {ball!r}")
		self.ball, self.prune_inverse = ball, bool(prune_inverse)
		self.on_poll = None                    # callable(status (n, 12)): called at every poll
		self.lockstep_depths = 0               # depths of all slots the last call launched
		self._results(0, False)

	def _results(self, n: int, keep_arrays: bool):
		self.status = np.zeros((n, 12), np.int64)
		self.lengths = np.full(n, -1, np.int64)
		self.meetings = [None] * n
		self._queues = [deque() for _ in range(n)]
		self._arrays = [(np.ones(1, np.int64), [None]) for _ in range(n)] if keep_arrays else None      # (sizes, back rows) per state

	depths = property(lambda self: self.status[:, 1])

	# -- engine lifetime ------------------------------------------------------------------------------------
	def _engine(self):
		if self._h is None:
			self._create("rk_beamb_create", "rk_beamb_destroy", self.ball._h if self.ball is not None else None, self.searches, self.width,
			             self.max_depth, int(self.prune_inverse))
		return self._h

	# -- the captured step: [value forward on all searches x 12 width rows, rk_beamb_step] ---------------------------
	def _depth_step(self, h, batch):
		values, code = eng.engine_values(_sliced_value_forward(self._forward, batch))
		self._keep = values                    # the kernels read it after this call returns
		_ffi.check(_ffi.lib().rk_beamb_step(h, values.data_ptr(), code, _ffi.stream_ptr()))

	def _rest(self, h, slots):
		sl = np.ascontiguousarray(slots, dtype=np.int32)
		_ffi.check(_ffi.lib().rk_beamb_rest(h, len(sl), sl.ctypes.data if len(sl) else None, _ffi.stream_ptr()))

	def _start(self, h, slots, rows: np.ndarray, budgets: np.ndarray):
		sl = np.ascontiguousarray(slots, dtype=np.int32)
		rows, budgets = np.ascontiguousarray(rows, dtype=np.int8), np.ascontiguousarray(budgets, dtype=np.int64)
		_ffi.check(_ffi.lib().rk_beamb_reset(h, len(sl), sl.ctypes.data, rows.ctypes.data, budgets.ctypes.data, _ffi.stream_ptr()))

	def _paths(self, h) -> np.ndarray:
		max_len = self.max_depth + 1 + DeviceSymBall.MAX_RADIUS
		out = np.zeros((self.searches, 1 + max_len), np.int32)
		_ffi.check(_ffi.lib().rk_beamb_paths(h, out.ctypes.data, max_len, _ffi.stream_ptr()))
		return out

	def _record(self, h, s: int, t: int) -> tuple:
		"""(sizes, back rows) of the search in slot `s`, whose last beam is that of depth `t`, as `DeviceBeamSearch.sizes` and its `back_of(t)`."""
		lib, stream = _ffi.lib(), _ffi.stream_ptr()
		sizes = np.zeros(self.max_depth + 1, np.int64)
		_ffi.check(lib.rk_beamb_export(h, s, 0, sizes.ctypes.data, None, 0, stream))
		sizes = sizes[:t + 1].copy()
		back = [None]
		for t in range(1, len(sizes)):
			row = np.zeros(int(sizes[t]), np.int64)
			_ffi.check(lib.rk_beamb_export(h, s, t, None, row.ctypes.data, len(row), stream))
			back.append(row)
		return sizes, back

	@staticmethod
	def _budgets(max_states, n: int) -> np.ndarray:
		"""int64 (n,): one budget for all or one per state, None (also inside a list) for no budget."""
		if max_states is None or np.ndim(max_states) == 0:
			given = [max_states] * n
		else:
			given = list(max_states)
			if np.ndim(max_states) != 1 or len(given) != n:
				raise ValueError(f"max_states must be a number or one per state, got shape {np.shape(max_states)}")
		out = np.zeros(n, np.int64)
		for i, b in enumerate(given):
			if b is None:
				out[i] = _ffi.INT64_MAX
				continue
			if isinstance(b, (bool, np.bool_)) or int(b) != b or int(b) < 0:
				raise ValueError(f"max_states must be non-negative integers or None, got {b!r}")
			out[i] = min(int(b), _ffi.INT64_MAX)
		return out

	# -- search -------------------------------------------------------------------------------------------------
	@no_grad
	def search(self, states, time_limit: float = None, max_states=None, keep_arrays: bool = False) -> np.ndarray:
		"""bool (n,): whether each state's search won (`lengths` >= 0)."""
		t0 = time.perf_counter()
		time_limit = time_limit or 1e10
		arr = np.asarray(states, dtype=np.int8)
		row_size = 20 if cube.get_is2024() else 288
		if arr.size % row_size:                                # before anything asks for a device
			raise ValueError(f"states must be (n, 20), or (n, 6, 8, 6) in 6x8x6 mode, got shape {arr.shape}")
		n = arr.size // row_size
		budgets = self._budgets(max_states, n)
		self._results(n, keep_arrays)
		self.lockstep_depths = 0
		if n == 0:
			return np.zeros(0, bool)
		_ffi.require_gpu()
		self.net.eval()
		forward, _, code = self._begin_net()
		rows = self._roots20(arr, n)                           # ValueError for an illegal 6x8x6 state, before anything runs
		home = (rows == _SOLVED20).all(axis=1)                 # solved starts: no slot, no launch
		self.status[home, 0] = 1
		self.lengths[home] = 0
		pending = np.nonzero(~home)[0]
		if len(pending) == 0:
			return self.lengths >= 0
		lib, stream = _ffi.lib(), _ffi.stream_ptr()
		try:
			h = self._engine()
			batch, = self._net_batches(h, code, (lib.rk_beamb_net_in,))
			key = (h.value, code, batch.data_ptr(), self.searches, eng.capture_key(self.net, forward))
			# (every slot is at rest between calls, and resting makes every row legal in this form: the warm-up step moves nothing)
			graph, = self._kept_steps(key, forward, lambda: self._rest(h, []), (self, lambda: self._depth_step(h, batch), batch))
			S = self.searches
			holds = np.full(S, -1, np.int64)       # the input position every slot runs, -1: free
			waiting = 0                            # the next of `pending` to start
			st = np.zeros((S, 12), np.int64)
			while True:
				_ffi.check(lib.rk_beamb_status(h, st.ctypes.data, stream))
				held = holds >= 0
				if st[held, 4].any() or (st[held, 0] >= 4).any():
					raise _ffi.RubiksHipError(f"beam engine: status {st[held, 0].tolist()}, error codes {st[held, 4].tolist()}")
				done = np.nonzero(held & (st[:, 0] != 0))[0]
				if len(done):
					paths = self._paths(h) if (st[done, 0] == 1).any() else None
					for s in done.tolist():
						i = int(holds[s])
						self.status[i] = st[s]
						if st[s, 0] == 1:
							if paths[s, 0] < 0:
								raise _ffi.RubiksHipError(f"rk_beamb_paths: the search of state {i} won, but its queue cannot be walked ({int(paths[s, 0])})")
							self.lengths[i] = paths[s, 0]
							self._queues[i] = deque(paths[s, 1:1 + paths[s, 0]].tolist())
							self.meetings[i] = (int(st[s, 5]), int(st[s, 6]), int(st[s, 7]))
						if keep_arrays:
							self._arrays[i] = self._record(h, s, int(st[s, 9]))
						holds[s] = -1
				if self.on_poll is not None:
					self.on_poll(self.status)
				late = time.perf_counter() - t0 >= time_limit
				free = np.nonzero(holds < 0)[0]
				if waiting < len(pending) and len(free) and not late:
					free = free[:len(pending) - waiting]
					took = pending[waiting:waiting + len(free)]
					self._start(h, free, rows[took], budgets[took])
					holds[free] = took
					waiting += len(free)
					continue                       # a start the ball holds is done already: look before running
				live = holds >= 0
				if late or not live.any():
					break
				burst = max(1, min(self.poll, int((self.max_depth - st[live, 9]).max())))    # a running slot advances at every replay
				for _ in range(burst):
					graph.replay()
				self.lockstep_depths += burst
			live = np.nonzero(holds >= 0)[0]
			if len(live):                          # out of time: what the searches had reached, status 0; then the slots are put to rest
				for s in live.tolist():
					i = int(holds[s])
					self.status[i] = st[s]
					if keep_arrays:
						self._arrays[i] = self._record(h, s, int(st[s, 9]))
				self._rest(h, live)
		except Exception:
			self._free()                           # slots in an unknown state: the next call starts from a new engine
			raise
		return self.lengths >= 0

	def action_queue_of(self, i: int) -> deque:
		return deque(self._queues[i])

	def _kept(self, i: int) -> tuple:
		if self._arrays is None:
			raise ValueError("the records were not kept: search(..., keep_arrays=True)")
		return self._arrays[i]

	def sizes_of(self, i: int) -> np.ndarray:
		"""int64: m_t of every beam state i's search formed, as `DeviceBeamSearch.sizes`; needs `keep_arrays`."""
		return self._kept(i)[0]

	def back_of(self, i: int, t: int) -> np.ndarray:
		"""int64 (m_t,): the `back` words of the beam of depth t (1 .. len(sizes_of(i)) - 1) of state i's search; needs `keep_arrays`."""
		sizes, back = self._kept(i)
		return back[eng.int_in("t", t, 1, len(sizes) - 1)]

	def __len__(self):
		return int(self.status[:, 2].sum())

	def __str__(self):
		return (f"Beam searches x{self.searches} (device, width={self.width}"
		        + (f", to a symmetry ball of radius {self.ball.radius})" if self.ball is not None else ")"))


def _load_net(loc: str, use_best: bool, loader=None):
	"""The value/policy net of a saved model folder (reference: DeepAgent.from_saved, agents.py:72-75)."""
	if loader is not None:
		return loader(loc, use_best)
	try:
		from librubiks.model import Model          # the reference package, when installed beside this one
	except ImportError as e:
		raise ImportError("from_saved needs the reference's librubiks.model.Model (or pass loader=callable(loc, use_best) -> net); "
		                  "librubiks_amd replaces the cube and search engines, not the network") from e
	return Model.load(loc, load_best=use_best).to(gpu)


class AStar(DeepAgent, _ffi.Owner):
	"""
	Batch weighted A* (agents.py:171-413): expands the `expansions` cheapest open nodes per iteration,
	cost = lambda_ * G + (-value).  Same results as the reference (index numbering, G, parents, action_queue)
	whenever the net returns the same values.

	Two ways to drive an iteration, chosen by the batch size K = 12 * expansions:
	  * K < 2048 (latency regime, the reference's N = 27 ... 170): `rk_astar_step_expand` -> net forward on the fixed
	    (K, 480) one-hot batch -> `rk_astar_step_commit`: six small launches around the net, no host synchronisation; the
	    host polls the engine's status every few iterations (never past the state budget; steps after a win are no-ops
	    on the device).  `use_hipgraph=True` captures the iteration once (the net must be capturable) and replays it.
	  * `exact_batch` (default: K >= 2048 with a float32 net, i.e. when a forward pass costs milliseconds):
	    `rk_astar_expand` synchronises once per iteration so that the net runs on exactly the new states instead of the
	    padded batch (measured with fc_small at N = 700 ... 1000: 15 % faster in float32, but 20 % slower than running
	    ahead of the GPU with the three times faster bf16 net).

	`capacity` is the size the node pool starts with.  A search whose state budget is larger (or that is limited only by
	time) GROWS the pool in place when it fills up, as the reference's increase_stack_size does (agents.py:396-402):
	`rk_astar_grow` doubles it -- device-to-device copies and one rehash kernel, the open queue stays as it is -- and the
	search continues where it stood, so it ends with the arrays of a search that had started in the large pool.  At
	`max_capacity` a search that still fills the pool warns with `CapacityExhausted` and sets `self.capacity_exhausted`.
	`self.grown` counts the growths of the last search.
	"""
	default_capacity = 4_000_000
	max_capacity = 64_000_000

	def __init__(self, net, lambda_: float, expansions: int, capacity: int = None, poll: int = 4, use_hipgraph: bool = False,
	             fused_first_layer=False, exact_batch: bool = None):
		# fused_first_layer: the engine hands the net the new nodes' 20-byte states and the net's first Linear(480, H)
		# reads them directly (librubiks_amd.oh_linear) -- no one-hot batch exists at all (DeepAgent keeps the copy fresh)
		super().__init__(net, fused_first_layer)
		self.exact_batch = exact_batch
		self.lambda_ = lambda_
		self.expansions = int(expansions)
		self.capacity = capacity
		self.poll = max(1, int(poll))
		# use_hipgraph: True / False, or "auto" = replay the iteration as a hipGraph only where that wins.  Measured eager vs
		# graph, us per iteration (profiles/r03_astar_small.json): with a real net the graph wins while the HOST is the
		# bottleneck (fc_small bf16: N = 10 207 -> 124, N = 27 196 -> 140), ties at N = 100 and LOSES above (N = 700: 471 -> 589;
		# float32 1580 -> 1878), although the kernels and their order are the same and under rocprofv3 (which serialises both)
		# both modes take the same time kernel by kernel (profiles/r03_astar_graph_gaps.json).
		self.use_hipgraph = (self.expansions <= 50) if use_hipgraph == "auto" else bool(use_hipgraph)
		self._h = None
		self._h_cap = 0
		self._h_expansions = 0
		self._n = 0
		self._root = None
		self._cache = None
		self.iterations = 0
		self.capacity_exhausted = False
		self.grown = 0                # times the pool grew in place during the last search
		self.profile_events = None    # a list: every run-ahead iteration appends four HIP events (before expand, before the net, after it, after commit)
		self._graph_cache = None      # (key, hipGraph of one iteration, its batch buffer): kept from search to search, see search()
		self.captures = 0             # hipGraph captures so far (a search on an unchanged engine and net replays the previous search's graph)
		self.record_pops = False      # debugging aid: keep the popped indices of every iteration in self.pops
		self.pops = []

	# -- engine lifetime ------------------------------------------------------------------------------------
	def _engine(self, capacity: int):
		if self._h is not None and self._h_cap >= capacity and self._h_expansions == self.expansions:
			return self._h
		self._h_cap, self._h_expansions = capacity, self.expansions                  # (an engine is built for one batch size)
		return self._create("rk_astar_create", "rk_astar_destroy", capacity, self.expansions)

	def _free(self):
		self._graph_cache = None              # it holds the engine's addresses
		super()._free()

	# -- search ---------------------------------------------------------------------------------------------
	def reset(self, time_limit: float, max_states: int):
		time_limit, max_states = super().reset(time_limit, max_states)
		self._n = 0
		self._cache = None
		self._root = None
		self.iterations = 0
		self.pops = []
		self.capacity_exhausted = False
		return time_limit, max_states

	def _iteration(self, h, oh, code):
		lib = _ffi.lib()
		ev = self.profile_events           # measurement aid (bench.py): HIP events between the three parts of an iteration
		if ev is not None:                 # (tested inline: this runs once per eager iteration, which is host-bound at small N)
			marks = eng.events(4)
			marks[0].record()
		_ffi.check(lib.rk_astar_step_expand(h, oh.data_ptr(), code, _ffi.stream_ptr()))
		if ev is not None:
			marks[1].record()
		values, vcode = eng.engine_values(_sliced_value_forward(self._forward, oh))
		_ffi.check(lib.rk_astar_set_values_dtype(h, vcode))
		self._keep = values                # the commit kernels read it after this call returns
		if ev is not None:
			marks[2].record()
		_ffi.check(lib.rk_astar_step_commit(h, values.data_ptr(), _ffi.stream_ptr()))
		if ev is not None:
			marks[3].record()
			ev.append(marks)

	@no_grad
	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		_ffi.require_gpu()
		t0 = time.perf_counter()
		time_limit, max_states = self.reset(time_limit, max_states)
		state = np.ascontiguousarray(state, dtype=np.int8)
		if cube.is_solved(state):
			return True
		K = 12 * self.expansions
		cap = max(int(min(max_states, self.capacity or self.default_capacity)), K + 2)
		lib = _ffi.lib()
		forward, _, code = self._begin_net()   # 6x8x6: the engine runs on the root's 20-byte form, the net gets 6x8x6 rows
		root = self._roots20(state, 1)[0]
		# `cached` holds the kept graph until this search returns.  When the engine below is re-made for a larger pool, `_free` drops the
		# cache; a graph that died there would hand its private memory pool back before the new capture, whose empty_cache() then
		# returns it to the driver and whose allocations fetch it again (profiles/r07_engine_plumbing_ab.json).
		cached = self._graph_cache
		oh = eng.net_batch(K, code, cached[2] if cached is not None and self.use_hipgraph else None)
		status = (C.c_longlong * 8)()
		h = self._engine(cap)
		cap = self._h_cap
		_ffi.check(lib.rk_astar_reset(h, root.ctypes.data, float(self.lambda_), _ffi.stream_ptr()))
		_ffi.check(lib.rk_astar_set_budget(h, int(min(max_states, cap)), _ffi.stream_ptr()))
		self._root, self._n, self._cache = state.copy(), 1, None
		self.iterations, self.pops, self.grown = 0, [], 0
		exact = self.exact_batch if self.exact_batch is not None else (K >= 2048 and eng.has_f32_weights(self.net))
		exact = exact and not self.use_hipgraph and not self.record_pops
		info = (C.c_longlong * 5)()
		while True:                                                  # one round per pool size: the pool grows in place below
			graph = None
			if self.use_hipgraph and not self.record_pops:
				# The captured iteration holds addresses (engine pools, batch buffer, the net's tensors) and two scalars passed by
				# value (lambda, the values' dtype) -- nothing of the search itself, which lives in device memory that rk_astar_reset
				# rewrites.  So the graph is KEPT from search to search and captured again only when one of those changes (a grown
				# or new engine, another net or fused copy, another lambda): capturing cost every search about 7 ms
				# (profiles/NOTES.md section 7), as much as a hundred iterations.
				# The warm-up is a real iteration; after a growth the step is captured again (the key holds the pool's size).
				key = (h.value, cap, float(self.lambda_), code, oh.data_ptr(), eng.capture_key(self.net, forward))
				step = lambda: self._iteration(h, oh, code)            # noqa: E731
				graph, _ = eng.kept_graph(self, key, step, step, oh, ((self.net, forward),))
			budget = int(min(max_states, cap))
			done = won = err = solved_idx = 0
			while exact:
				# one synchronisation per iteration, the net sees exactly the new states (agents.py:315, :369-383)
				_ffi.check(lib.rk_astar_expand(h, self.expansions, info, _ffi.stream_ptr()))
				n_pop, n_new, won, solved_idx, self._n = (int(x) for x in info)
				if n_pop == 0:
					done = 1
					_ffi.check(lib.rk_astar_status(h, status, _ffi.stream_ptr()))      # why nothing was popped: the guard, or an error
					err = int(status[6])
					break
				self.iterations += 1
				if won:
					break
				values = None
				if n_new:
					_ffi.check(lib.rk_astar_new_states_oh(h, oh.data_ptr(), code, _ffi.stream_ptr()))
					values, vcode = eng.engine_values(_sliced_value_forward(forward, oh[:n_new]))
					_ffi.check(lib.rk_astar_set_values_dtype(h, vcode))
				_ffi.check(lib.rk_astar_commit(h, values.data_ptr() if values is not None else None, _ffi.stream_ptr()))
				if time.perf_counter() - t0 >= time_limit:
					break
			while not exact:
				poll = 1 if self.record_pops else eng.burst(self.poll, budget - self._n, K)
				for _ in range(poll):
					if self.record_pops:
						head = np.zeros(self.expansions, np.int64)
						got = lib.rk_astar_next_pops(h, head.ctypes.data, self.expansions, _ffi.stream_ptr())
						if got > 0:
							self.pops.append(head[:got].copy())
					if graph is not None:
						graph.replay()
					else:
						self._iteration(h, oh, code)
				_ffi.check(lib.rk_astar_status(h, status, _ffi.stream_ptr()))
				done, won, self._n, self.iterations, solved_idx, err = (int(status[i]) for i in (0, 1, 2, 3, 5, 6))
				if won or done or err or time.perf_counter() - t0 >= time_limit:
					break
			self._cache = None
			if err:
				raise _ffi.RubiksHipError(f"A* engine error {eng.astar_errors([err])}")
			if won:
				self.action_queue = eng.read_path(lib.rk_astar_path, h, solved_idx)
				return True
			# out of budget, out of time, or nothing left to expand
			pool_full = done and self._n + K > cap and lib.rk_astar_open_size(h) > 0
			if not (pool_full and max_states > cap and time.perf_counter() - t0 < time_limit):
				return False
			# the pool, not the caller's budget, ended the search: grow it like the reference's increase_stack_size
			# (agents.py:396-402) -- in place, the search goes on where it stood -- or say so
			if cap >= self.max_capacity:
				eng.pool_exhausted(self, cap)
				return False
			cap = min(2 * cap, self.max_capacity)
			_ffi.check(lib.rk_astar_grow(h, cap, _ffi.stream_ptr()))
			self._h_cap = cap
			_ffi.check(lib.rk_astar_set_budget(h, int(min(max_states, cap)), _ffi.stream_ptr()))
			self.grown += 1

	# -- inspection (what the reference's tests look at: tests/test_agents.py:96-145) --------------------------
	def _export(self):
		if self._cache is None:
			n = self._n
			rows = max(n + 1, 1000)            # the reference's arrays start with 1000 rows (agents.py:385-394); its tests write G of a reset agent
			states, G, parents, pact = eng.export_pool(_ffi.lib().rk_astar_export if self._h is not None else None, (self._h,), n, rows)
			self._cache = (self._states_out(states, n), G, parents, pact)
		return self._cache

	@property
	def states(self) -> np.ndarray:
		return self._export()[0]

	@property
	def G(self) -> np.ndarray:
		return self._export()[1]

	@property
	def parents(self) -> np.ndarray:
		return self._export()[2]

	@property
	def parent_actions(self) -> np.ndarray:
		return self._export()[3]

	@property
	def indices(self) -> dict:
		"""state bytes -> index, rebuilt on the host from the exported pool (the reference's dict, agents.py:201)."""
		states = self.states
		return {states[i].tobytes(): i for i in range(1, self._n + 1)}

	@property
	def open_queue(self) -> list:
		"""The open set as (cost, index) pairs in pop order."""
		if self._h is None or self._n == 0:
			return []
		n = int(_ffi.lib().rk_astar_open_size(self._h))
		costs, idx = np.zeros(n, np.float64), np.zeros(n, np.int64)
		got = _ffi.lib().rk_astar_export_open(self._h, costs.ctypes.data, idx.ctypes.data, n, _ffi.stream_ptr())
		return list(zip(costs[:got].tolist(), idx[:got].tolist()))

	def index_of(self, state: np.ndarray) -> int:
		state = self._roots20(state, 1)[0]
		return int(_ffi.lib().rk_astar_lookup(self._h, state.ctypes.data, _ffi.stream_ptr()))

	@no_grad
	def cost(self, states: np.ndarray, indeces: np.ndarray) -> np.ndarray:
		"""lambda * G + (-value) for given states (agents.py:369-383)."""
		H = -self.net(cube.as_oh(states), value=True, policy=False)
		H = H.cpu().squeeze().detach().numpy()
		return self.lambda_ * self.G[indeces] + H

	@classmethod
	def from_saved(cls, loc: str, use_best: bool, lambda_: float, expansions: int, loader=None):
		"""agents.py:405-407.  The net itself is the reference's `librubiks.model.Model` (out of this package's scope):
		it is loaded with `loader(loc, use_best)` if given, else with the reference's `Model.load` when that package is
		importable next to this one (the drop-in situation)."""
		return cls(_load_net(loc, use_best, loader), lambda_=lambda_, expansions=expansions)

	def __len__(self) -> int:
		return self._n

	def __str__(self) -> str:
		return f'AStar (lambda={self.lambda_}, N={self.expansions})'


def _policy_value_f32(out):
	"""(softmaxed policy (B,12), value (B,)) as contiguous float32 GPU tensors from the net's [logits, value]."""
	p, v = out
	p = p.detach().to(device=gpu, dtype=torch.float32).softmax(dim=1).contiguous()
	v = v.detach().to(device=gpu, dtype=torch.float32).reshape(-1).contiguous()
	return p, v


PRIORS = ("kernel", "torch", "reference")


class MCTSBatch(DeepAgent, _ffi.Owner):
	"""
	T independent Monte Carlo tree searches advanced in lock-step on the GPU (engine rk_mcts_*).  Each tree follows
	the reference's MCTS exactly (agents.py:415-645): same node numbering, neighbors, P, V, N, W, L and action queue
	as running the reference on that start state alone, whenever the net returns the same numbers.

	One simulation of all trees = expand kernel, one-hot kernel, net forward on the fixed (12 T, 480) batch,
	backup+select kernel.  Nothing in a step synchronises, so `use_graph=True` captures the step in a hipGraph
	(through torch.cuda.CUDAGraph) and replays it; the host only polls every `poll` simulations.

	priors -- where softmax(logits) (agents.py:472, :551-552) is computed:
	  "kernel"     inside the backup kernel from the net's raw float32 / bfloat16 logits: exp(x - max) / sum in float32, the sum
	               taken in the order torch.softmax's own kernel adds on this device (rk_mcts.hip, child_policy) -- no softmax,
	               conversion or copy kernels in the step; capturable.  The default of this class (the throughput form).
	  "torch"      torch.softmax on the device, float32; capturable.
	  "reference"  the reference's own two lines: the root's priors by `p.softmax(dim=1)` on the device (agents.py:472), every
	               other node's by `p.cpu().softmax(dim=1)` (agents.py:551-552: on the HOST), bit for bit whatever torch's CPU
	               kernel does.  One device-to-host wait per simulation, so not capturable.  The default of `MCTS`.
	`search_graph`: after the search, every solved tree gets the reference's graph completion and breadth-first shortening
	(agents.py:597-633) on the device (rk_mcts_search_graph); `action_queue_of` then returns the shortened queue.
	`max_capacity`: pools that fill up while a tree's own budget is larger grow in place (rk_mcts_grow; agents.py:450-460),
	doubling up to this many states per tree.
	"""

	def __init__(self, net, c: float, n_trees: int, capacity: int = 50_000, max_path: int = None, nu: float = 100.0,
	             fused_first_layer=False, torch_softmax: bool = False, priors: str = None, search_graph: bool = False,
	             max_capacity: int = None, overlap_halves: bool = False):
		# fused_first_layer: the net's first Linear(480, H) reads the children's 20-byte states (librubiks_amd.oh_linear)
		super().__init__(net, fused_first_layer)
		priors = priors or ("torch" if torch_softmax else "kernel")
		if priors not in PRIORS:
			raise ValueError(f"priors is one of {PRIORS}")
		self.priors = priors
		self.search_graph = bool(search_graph)
		# overlap_halves (hipGraph mode, fused first layer, priors in the kernel): the captured step advances the batch as two halves
		# on two streams, skewed by half a step, so that one half's latency-bound backup + descent runs under the other half's net
		# forward (see _capture_halves).  Trees are independent: every tree's arrays are what they would be without it.
		self.overlap_halves = bool(overlap_halves)
		self.c, self.nu, self.n_trees = float(c), float(nu), int(n_trees)
		self.capacity = int(capacity)
		self.max_capacity = int(max_capacity) if max_capacity else None
		self._auto_path = max_path is None
		self.max_path = int(max_path or max(4096, 2 * self.capacity))
		self._h = None
		self._shape = None
		self.status = None
		self.simulations = 0
		self.grown = 0
		self.profile_events = None        # a list: every eager simulation step appends a HIP event pair around its backup + select launch
		self.on_poll = None               # callable(status): called with every status the search reads (solving/evaluation.py times games with it)
		self._graph_cache = None          # (key, hipGraph of one step, its batch buffer): kept from search to search, see _capture
		self.captures = 0                 # hipGraph captures so far

	@property
	def torch_softmax(self) -> bool:
		return self.priors == "torch"

	def _engine(self):
		shape = (self.n_trees, self.capacity, self.max_path)
		if self._h is None or self._shape != shape:
			self._create("rk_mcts_create", "rk_mcts_destroy", *shape)
			self._shape = shape
		return self._h

	def _free(self):
		self._graph_cache = None              # it holds the engine's addresses
		super()._free()

	_ERRORS = {1: "path longer than max_path", 2: "broken neighbour link", 3: "backup without a pending expansion (rk_mcts_expand missing from the step)",
	           4: "NaN in the net's policy or value"}

	def _poll(self):
		st = np.zeros((self.n_trees, 6), np.int64)
		_ffi.check(_ffi.lib().rk_mcts_status(self._h, st.ctypes.data, _ffi.stream_ptr()))
		if (st[:, 5] != 0).any():
			codes = sorted(set(int(x) for x in st[:, 5] if x))
			raise _ffi.RubiksHipError(f"MCTS engine error codes {codes}: " + "; ".join(self._ERRORS.get(k, "?") for k in codes)
			                          + f" (max_path={self.max_path})")
		self.status = st
		if self.on_poll is not None:
			self.on_poll(st)
		return st

	def _step(self, oh, h, expand: bool = True):
		lib = _ffi.lib()
		if expand:
			_ffi.check(lib.rk_mcts_expand(h, _ffi.stream_ptr()))
		if self._fs is not None:
			# the first layer reads the children where the engine keeps them; no one-hot, no copy
			x = self._fs.first.from_pointer(lib.rk_mcts_children(h), 12 * self.n_trees)
			p, v = self._fs.tail(x)
		elif self._n686 is not None:
			# 6x8x6 net: the children's 20-byte rows, then their 6x8x6 one-hot in the net's dtype (one launch) and the net
			_ffi.check(lib.rk_mcts_children_oh(h, oh.data_ptr(), _ffi.OH_STATES, _ffi.stream_ptr()))
			p, v = self._n686(oh)
		else:
			_ffi.check(lib.rk_mcts_children_oh(h, oh.data_ptr(), _OH_CODES[oh.dtype], _ffi.stream_ptr()))
			p, v = self.net(oh)
		ev = self.profile_events           # measurement aid (bench.py): a HIP event pair around the backup + select launch
		if self.priors == "kernel" and isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == v.dtype and p.dtype in (torch.float32, torch.bfloat16) \
		   and p.dim() == 2 and p.stride(1) == 1 and p.stride(0) >= 12 and v.numel() == len(p) and v.reshape(len(p), -1).stride(0) >= 1:
			# raw logits and values in the net's dtype (rows may be views into one tensor of merged heads): the softmax
			# (agents.py:551) runs inside the backup kernel
			self._keep = (p, v)        # the kernels read these after this call returns
			if ev is not None:
				pair = eng.events(2)
				pair[0].record()
			_ffi.check(lib.rk_mcts_backup_select_logits(h, p.data_ptr(), p.stride(0), v.data_ptr(), v.reshape(len(p), -1).stride(0),
			                                            _OH_CODES[p.dtype], _ffi.stream_ptr()))
			if ev is not None:
				pair[1].record()
				ev.append(tuple(pair))
			return
		if self.priors == "reference":
			# agents.py:551-552 to the letter: `p.cpu().softmax(dim=1)` -- the HOST's softmax of the logits, the same CPU kernel on
			# the same numbers; only the plumbing differs: the logits travel through page-locked buffers, and the 144 numbers are
			# softmaxed by ONE thread.  torch forks its whole intra-op pool even for twelve rows, and a pool of 128 threads spinning
			# after every simulation on a host whose CPU share is a fraction of that starves the launching thread: 3.3 ms per
			# simulation instead of 0.25 (profiles/r04_mcts_priors_cost.json).  Rows are independent: the bits do not depend on it.
			v = v.detach().to(device=gpu, dtype=torch.float32).reshape(-1).contiguous()
			buf = getattr(self, "_ref_buf", None)
			if buf is None or buf[0].shape != p.shape or buf[0].dtype != p.dtype:
				buf = self._ref_buf = (torch.empty(p.shape, dtype=p.dtype).pin_memory(), torch.empty(p.shape, dtype=torch.float32).pin_memory(),
				                       torch.empty(p.shape, dtype=torch.float32, device=gpu))
			h_in, h_out, d_out = buf
			h_in.copy_(p.detach(), non_blocking=True)
			torch.cuda.current_stream().synchronize()                    # the one device-to-host wait of this mode
			h_out.copy_(_host_softmax(h_in))
			d_out.copy_(h_out, non_blocking=True)
			p = d_out
		else:
			p, v = _policy_value_f32((p, v))
		self._keep = (p, v)
		_ffi.check(lib.rk_mcts_backup_select(h, p.data_ptr(), v.data_ptr(), _ffi.stream_ptr()))

	@no_grad
	def search(self, states: np.ndarray, time_limit: float = None, max_states=None, max_sims: int = None,
	           use_graph: bool = False, poll: int = 16) -> np.ndarray:
		"""Runs all trees until each is solved or out of budget; returns the bool vector `solved` (T,)."""
		t0 = time.perf_counter()
		assert time_limit or max_states is not None or max_sims
		time_limit = time_limit or 1e10
		self._begin(states, max_states, max_sims, use_graph)
		while time.perf_counter() - t0 < time_limit and (max_sims is None or self.simulations < max_sims):
			self._advance(poll if max_sims is None else min(poll, max_sims - self.simulations))
			if self._poll()[:, 0].all() and not self._grow():
				break
		return self._finish()

	# The three stages of a search.  Everything is enqueued on the CURRENT stream, so several engines can be advanced in turn on
	# streams of their own (tried in round 3 with 2 and 4 engines sharing the 256 trees, so that one engine's descent would
	# overlap the others' net forwards: 0.166 and 0.242 ms per 256-tree step against 0.159 with one engine,
	# profiles/r03_mcts_variants.json -- the small GEMMs of the halves do not overlap each other; dropped).
	@no_grad
	def _begin(self, states: np.ndarray, max_states, max_sims, use_graph: bool):
		_ffi.require_gpu()
		self.net.eval()
		forward, reads_states, code = self._begin_net()      # 6x8x6: the trees grow in 20-byte form, the net gets 6x8x6 rows (_Net686)
		states = self._roots20(states, self.n_trees)
		if max_states is None:
			max_states = self.capacity
		self._budget = np.broadcast_to(np.asarray(max_states, dtype=np.int64), (self.n_trees,)).copy()      # what the caller asked for
		ms = np.minimum(self._budget, self.capacity)
		h, lib = self._engine(), _ffi.lib()
		_ffi.check(lib.rk_mcts_reset(h, states.ctypes.data, ms.ctypes.data, self.c, self.nu, _ffi.stream_ptr()))
		root_oh = torch.empty((self.n_trees, 20 if reads_states else 480), dtype=eng.OH_DTYPES[code], device=gpu)
		_ffi.check(lib.rk_mcts_roots_oh(h, root_oh.data_ptr(), code, _ffi.stream_ptr()))
		p, v = _policy_value_f32(forward(root_oh))                       # agents.py:470-473: the root's softmax runs on the device
		# the step's batch: the kept graph's buffer if it fits; a new one-hot stays uninitialised (the step writes every row it reads)
		oh = eng.net_batch(12 * self.n_trees, code, self._graph_cache[2] if self._graph_cache is not None else None, zeros=False)
		_ffi.check(lib.rk_mcts_set_root_pv(h, p.data_ptr(), v.data_ptr(), _ffi.stream_ptr()))
		# every backup + select launch also expands the leaf it found, while another simulation is to follow
		_ffi.check(lib.rk_mcts_set_expand_ahead(h, int(max_sims) if max_sims is not None else -1))
		self.simulations, self.grown = 0, 0
		self._max_sims, self._oh, self._graph = max_sims, oh, None
		self._use_graph = bool(use_graph) and self.priors != "reference"       # the host softmax waits for the device: nothing to capture
		if self._use_graph and (max_sims is None or max_sims > 2):
			self._capture(2)

	def _capture(self, warm: int):
		"""`warm` real simulations, then the step as a hipGraph.  After an eager step with expand-ahead on, every tree's next
		expansion is always done by the backup launch before it, so the captured step leaves rk_mcts_expand out (one launch less
		per replay); were that ever untrue, the backup kernel stops the tree with error 3 instead of using stale children."""
		h, oh = self._h, self._oh
		if self.overlap_halves and self._fs is not None and self.priors == "kernel" and self.n_trees >= 2:
			return self._capture_halves(warm)
		# The captured step holds addresses (pools, batch buffer, the net's tensors) and scalars passed by value (c, nu, sizes, the
		# simulation limit of the expand-ahead) --
		# nothing of the trees, which live in device memory that rk_mcts_reset rewrites.  So the graph is KEPT from search to
		# search and captured again only when one of those changes (grown or new engine, another net or fused copy).
		key = (h.value, self._shape, self.c, self.nu, self.priors, self._max_sims, oh.data_ptr(), oh.dtype, eng.capture_key(self.net, self._forward))
		self._graph, hit = eng.kept_graph(self, key, lambda: self._warm(warm), lambda: self._step(oh, h, expand=False), oh, ((self.net, self._forward),))
		if hit:
			self._warm(warm)                                           # on this stream: a kept graph still wants every tree expanded ahead

	def _warm(self, n: int):
		"""`n` real simulations before the captured step runs: after them every tree is expanded ahead (they also warm the allocator)."""
		for _ in range(n):
			self._step(self._oh, self._h)
			self.simulations += 1

	def _net_half(self, first: int, count: int):
		"""Raw logits and values of the trees first ... first + count - 1: the fused first layer reads their children where the engine keeps them."""
		lib = _ffi.lib()
		x = self._fs.first.from_pointer(lib.rk_mcts_children(self._h) + first * 12 * 20, 12 * count)
		return self._fs.tail(x)

	def _backup_half(self, first: int, count: int, p, v):
		_ffi.check(_ffi.lib().rk_mcts_backup_select_logits_range(self._h, first, count, p.data_ptr(), p.stride(0), v.data_ptr(), v.reshape(len(p), -1).stride(0),
		                                                          _OH_CODES[p.dtype], _ffi.stream_ptr()))

	def _capture_halves(self, warm: int):
		"""
		The step as a hipGraph that advances the batch in TWO HALVES, A = trees [0, T/2) and B = the rest, skewed by half a step
		(VERDICT r4 #3).  A step of one half is net forward -> backup + select (+ expand ahead); the second part is one wave per
		tree chasing pointers for ~45 us with < 2 % of the chip's wave slots occupied, the first is throughput-bound GEMMs.
		One replay =
		    phase 1:   backup+select A (simulation k)      ||   net B (simulation k)
		    phase 2:   net A (simulation k + 1)            ||   backup+select B (simulation k)
		on two streams forked and joined inside the capture, so each half's descent runs under the other half's GEMMs.  Before the
		first replay A's net outputs of simulation 1 are computed eagerly (`_prime_halves`); A's net of the simulation after the
		last one is computed in vain.  Every tree still sees select, expand, net, backup in the reference's order.
		"""
		h = self._h
		T = self.n_trees
		na = T // 2
		key = ("halves", h.value, self._shape, self.c, self.nu, self._max_sims, eng.capture_key(self.net, self._fs))
		caller, side = torch.cuda.current_stream(), torch.cuda.Stream()      # (`side`: the captured step's second stream)

		def warm_halves():
			self._warm(warm)
			pa, va = self._net_half(0, na)                             # shapes / dtypes of a half's outputs (and a warm-up of the half-size GEMMs)
			self._net_half(na, T - na)
			# A's outputs cross from one replay to the next (and from the eager priming into the first replay): they live in buffers
			# of their own, copied into at the end of phase 2 (two copies of a few KB); allocated as memory of the caller's stream
			with torch.cuda.stream(caller):
				self._half_bufs = (torch.empty_like(pa), torch.empty_like(va))

		def step_halves():
			XA, VA = self._half_bufs
			cur = torch.cuda.current_stream()
			side.wait_stream(cur)                                      # fork
			self._backup_half(0, na, XA, VA)                           # phase 1, this stream: backup + select A
			with torch.cuda.stream(side):
				pb, vb = self._net_half(na, T - na)                    # phase 1, side stream: net B
			cur.wait_stream(side)                                      # both streams meet between the phases
			side.wait_stream(cur)
			pa, va = self._net_half(0, na)                             # phase 2, this stream: net A of the NEXT simulation
			XA.copy_(pa)
			VA.copy_(va)
			with torch.cuda.stream(side):
				self._backup_half(na, T - na, pb, vb)                  # phase 2, side stream: backup + select B
			cur.wait_stream(side)                                      # join

		self._graph, hit = eng.kept_graph(self, key, warm_halves, step_halves, self._oh, lambda: ((self.net, self._fs), self._half_bufs))
		if hit:
			self._warm(warm)
			self._half_bufs = self._graph_cache[4]
		self._prime_halves()

	def _prime_halves(self):
		"""A's net outputs of the coming simulation into the buffers the graph's first phase reads (eager, once per run of replays)."""
		pa, va = self._net_half(0, self.n_trees // 2)
		self._half_bufs[0].copy_(pa)
		self._half_bufs[1].copy_(va)

	@no_grad
	def _advance(self, n: int):
		for _ in range(n):
			if self._graph is not None:
				self._graph.replay()
			else:
				self._step(self._oh, self._h)
		self.simulations += n

	def _grow(self) -> bool:
		"""All trees are done.  If some stopped only because the POOL was their budget (the caller's is larger), grow every
		pool in place (agents.py:450-460, :503-504) and let those trees go on.  True if the search continues."""
		st = self.status
		if not self.max_capacity or self.capacity >= self.max_capacity:
			return False
		want = (st[:, 1] == 0) & (st[:, 2] + 12 > np.minimum(self._budget, self.capacity)) & (self._budget > self.capacity)
		if not want.any():
			return False
		cap = min(2 * self.capacity, self.max_capacity)
		path = max(self.max_path, 2 * cap) if self._auto_path else self.max_path
		ms = np.minimum(self._budget, cap)
		_ffi.check(_ffi.lib().rk_mcts_grow(self._h, cap, path, ms.ctypes.data, _ffi.stream_ptr()))
		self.capacity, self.max_path = cap, path
		self._shape = (self.n_trees, cap, path)
		self.grown += 1
		if self._graph is not None:                                   # the captured step holds the old pools' addresses
			self._graph = None
			if self._max_sims is None or self._max_sims - self.simulations > 1:
				self._capture(1)
		return True

	@no_grad
	def _finish(self) -> np.ndarray:
		_ffi.check(_ffi.lib().rk_mcts_set_expand_ahead(self._h, 0))
		if (self._max_sims is None or self.simulations < self._max_sims) and not self._poll()[:, 0].all():
			# stopped early (time) with leaves expanded ahead: one more step (net + backup, no further expansion) completes
			# them, so that every tree is the reference's tree after a whole number of simulations
			self._step(self._oh, self._h)
			self.simulations += 1
		st = self._poll()
		self._graph_done = False
		if self.search_graph and (st[:, 1] == 1).any():                 # agents.py:483-486, on the device
			_ffi.check(_ffi.lib().rk_mcts_search_graph(self._h, _ffi.stream_ptr()))
			self._graph_done = True
		return st[:, 1] != 0

	# -- results ------------------------------------------------------------------------------------------------
	def action_queue_of(self, tree: int) -> deque:
		lib = _ffi.lib()
		if getattr(self, "_graph_done", False) and self.status[tree, 1] == 1:
			queue = eng.read_path(lib.rk_mcts_graph_path, self._h, tree, length=self.max_path, strict=False)
			if queue is not None:
				return queue
		return eng.read_path(lambda buf, n, stream: lib.rk_mcts_path(self._h, tree, buf, None, n, stream), length=self.max_path)

	def path_nodes_of(self, tree: int) -> list:
		acts = (C.c_longlong * self.max_path)()
		nodes = (C.c_longlong * self.max_path)()
		_ffi.lib().rk_mcts_path(self._h, tree, acts, nodes, self.max_path, _ffi.stream_ptr())
		return [int(x) for x in nodes[:int(self.status[tree, 4])]]

	def tree_arrays(self, tree: int) -> dict:
		"""The reference's arrays of one tree, rows 0..n (row 0 unused), in the reference's dtypes."""
		n = int(self._poll()[tree, 2])
		out = dict(
			states=np.zeros((n + 1, 20), np.int8), neighbors=np.zeros((n + 1, 12), np.int64), leaves=np.ones(n + 1, np.uint8),
			P=np.zeros((n + 1, 12)), V=np.zeros(n + 1), N=np.zeros((n + 1, 12), np.int64), W=np.zeros((n + 1, 12)), L=np.zeros((n + 1, 12)))
		_ffi.check(_ffi.lib().rk_mcts_export(
			self._h, tree, 1, n, out["states"][1:].ctypes.data, out["neighbors"][1:].ctypes.data, out["leaves"][1:].ctypes.data,
			out["P"][1:].ctypes.data, out["V"][1:].ctypes.data, out["N"][1:].ctypes.data, out["W"][1:].ctypes.data,
			out["L"][1:].ctypes.data, _ffi.stream_ptr()))
		out["leaves"] = out["leaves"].astype(bool)
		out["states"] = self._states_out(out["states"], n)
		out["n"] = n
		return out

	def __len__(self):
		return int(self.status[:, 2].sum()) if self.status is not None else 0

	def __str__(self):
		return f"Batched MCTS x{self.n_trees} (c={self.c})"


class MCTS(DeepAgent):
	"""
	The reference's single-tree agent (agents.py:415-645) on the device engine: `MCTS(net, c, search_graph)`,
	`search(state, time_limit, max_states)`, `action_queue`, `len(agent)`, and the arrays `states, neighbors, leaves,
	P, V, N, W, L, indices` for inspection (tests/test_agents.py:49-94).

	With default arguments the priors are computed exactly where and how the reference computes them (`priors="reference"`,
	see MCTSBatch: the root's softmax on the device, every other node's on the host, agents.py:472 and :551-552), so P equals
	the reference's bit for bit whenever the logits do; that costs one device-to-host wait per simulation.  `priors="kernel"`
	(softmax inside the backup kernel, no wait, hipGraph-capturable) is the fast form; `use_hipgraph=True` implies it unless
	`priors` is given.  The pool starts at `capacity` (default 200 000 nodes) and grows in place while the state budget allows
	(rk_mcts_grow, agents.py:450-460) up to `max_capacity`; graph completion and path shortening of a solved search
	(`search_graph`, agents.py:597-633) run on the device.
	"""
	default_capacity = 200_000
	max_capacity = 25_000_000           # 461 B per node: 11.5 GB

	def __init__(self, net, c: float, search_graph: bool, capacity: int = None, use_hipgraph: bool = False, torch_softmax: bool = False,
	             priors: str = None):
		super().__init__(net)
		self.priors = priors or ("torch" if torch_softmax else ("kernel" if use_hipgraph else "reference"))
		if self.priors not in PRIORS:
			raise ValueError(f"priors is one of {PRIORS}")
		self.c = c
		self.search_graph = search_graph
		self.nu = 100
		self.capacity = capacity
		self.use_hipgraph = use_hipgraph          # replay the simulation step as a captured hipGraph (the net must be capturable)
		self._batch = None
		self._arrays = None
		self._n = 0
		self.capacity_exhausted = False

	@property
	def grown(self) -> int:
		return self._batch.grown if self._batch is not None else 0

	def reset(self, time_limit: float, max_states: int):
		time_limit, max_states = super().reset(time_limit, max_states)
		self._arrays, self._n = None, 0
		return time_limit, max_states

	@no_grad
	def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
		time_limit, max_states = self.reset(time_limit, max_states)
		self.capacity_exhausted = False
		cap = max(int(min(max_states, self.capacity or self.default_capacity)), 13)      # a pool holds at least the root and its 12 children
		b = self._batch
		if b is None or b.capacity < cap or b.c != float(self.c) or b.priors != self.priors or b.search_graph != bool(self.search_graph) \
		   or b.max_capacity != self.max_capacity:
			b = self._batch = MCTSBatch(self.net, self.c, 1, capacity=cap, nu=self.nu, priors=self.priors, search_graph=self.search_graph,
			                            max_capacity=self.max_capacity)
		b.net = self.net
		self._is2024 = cube.get_is2024()
		# the pool grows in place inside the batch engine while the budget is larger (agents.py:496-503)
		solved = bool(b.search(np.asarray(state)[None], time_limit=time_limit, max_states=int(min(max_states, 2 ** 62)), poll=8,
		                       use_graph=self.use_hipgraph)[0])
		self._n = int(b.status[0, 2])
		if not solved and self._n + 12 > b.capacity and max_states > b.capacity and b.capacity >= self.max_capacity:
			eng.pool_exhausted(self, b.capacity)
		self.action_queue = b.action_queue_of(0)       # with search_graph: completed and shortened on the device (agents.py:483-486)
		return solved

	# -- inspection -------------------------------------------------------------------------------------------
	def _export(self) -> dict:
		if self._arrays is None:
			self._arrays = self._batch.tree_arrays(0) if self._batch is not None and self._n else dict(
				states=np.zeros((1, 20) if self._is2024 else (1, 6, 8, 6), np.int8), neighbors=np.zeros((1, 12), np.int64), leaves=np.ones(1, bool),
				P=np.zeros((1, 12)), V=np.zeros(1), N=np.zeros((1, 12), np.int64), W=np.zeros((1, 12)), L=np.zeros((1, 12)), n=0)
		return self._arrays

	states = property(lambda self: self._export()["states"])
	neighbors = property(lambda self: self._export()["neighbors"])
	leaves = property(lambda self: self._export()["leaves"])
	P = property(lambda self: self._export()["P"])
	V = property(lambda self: self._export()["V"])
	N = property(lambda self: self._export()["N"])
	W = property(lambda self: self._export()["W"])
	L = property(lambda self: self._export()["L"])

	@property
	def indices(self) -> dict:
		"""state bytes -> index (the reference's dict, agents.py:419), rebuilt on the host from the exported states: inspection only"""
		st = self.states
		return {st[i].tobytes(): i for i in range(1, self._n + 1)}

	@classmethod
	def from_saved(cls, loc: str, use_best: bool, c: float, search_graph: bool, loader=None):
		"""agents.py:635-639."""
		return cls(_load_net(loc, use_best, loader), c=c, search_graph=search_graph)

	def __str__(self):
		return ("BFS" if self.search_graph else "Naive") + f" MCTS (c={self.c})"

	def __len__(self):
		return self._n


class AStarBatch(DeepAgent, _ffi.Owner):
	"""
	S independent batch weighted A* searches advanced in lock-step on the GPU (engine rk_astarb_*).  Every search
	follows the reference's AStar exactly (agents.py:171-413): same node numbering, G, parents and action queue as
	running the reference on that start state alone, whenever the net returns the same numbers.

	One iteration of all searches = one fixed sequence of launches around one net forward on the padded
	(S * 12 N, 480) batch; nothing synchronises, so `use_graph=True` captures the iteration in a hipGraph and replays
	it.  The host polls the per-search status every `poll` iterations (searches that are solved or out of budget are
	skipped on the device in between).  This is the throughput form for evaluating many scrambles -- the reference's
	Evaluator runs its games one after the other.
	"""

	def __init__(self, net, lambda_: float, expansions: int, n_searches: int, capacity: int = 200_000, fused_first_layer=False):
		super().__init__(net, fused_first_layer)           # fused: the net's first Linear reads the new nodes' 20-byte states
		self.net_slice_rows = None                         # rows per net forward (None: NET_SLICE_ROWS)
		self.lambda_, self.expansions, self.n_searches = float(lambda_), int(expansions), int(n_searches)
		self.capacity = max(int(capacity), 12 * self.expansions + 2)
		self._h = None
		self.status = None
		self.iterations = 0
		self.on_poll = None                                # callable(status): called with every status the search reads

	def _engine(self):
		if self._h is None:
			self._create("rk_astarb_create", "rk_astarb_destroy", self.n_searches, self.capacity, self.expansions)
		return self._h

	def _poll(self) -> np.ndarray:
		st = np.zeros((self.n_searches, 7), np.int64)
		_ffi.check(_ffi.lib().rk_astarb_status(self._h, st.ctypes.data, _ffi.stream_ptr()))
		if st[:, 6].any():
			bad = {int(s): int(st[s, 6]) for s in np.flatnonzero(st[:, 6])}
			raise _ffi.RubiksHipError(f"batched A* engine error codes {st[:, 6].tolist()}: searches {sorted(bad)} ended with "
			                          + eng.astar_errors(bad.values()))
		self.status = st
		if self.on_poll is not None:
			self.on_poll(st)
		return st

	def _step_exact(self, oh, code):
		"""One iteration with the net's batch compacted to the searches' NEW rows (one host wait for their count)."""
		lib, h = _ffi.lib(), self._h
		_ffi.check(lib.rk_astarb_step_expand_compact(h, oh.data_ptr(), code, self._n_rows.data_ptr(), _ffi.stream_ptr()))
		self._counted.record()
		self._counted.synchronize()
		rows = int(self._n_rows[0])
		self.net_rows_total += rows
		if rows == 0:
			values = self._no_values
		else:
			values = self._values(_sliced_value_forward(self._forward, oh[:min(len(oh), -(-rows // 64) * 64)], self.net_slice_rows or 12_288))
		self._keep = values
		_ffi.check(lib.rk_astarb_step_commit(h, values.data_ptr(), _ffi.stream_ptr()))

	def _values(self, out) -> torch.Tensor:
		"""The value head as the engine takes it (a bf16 net's values go in as they are); the engine is told only when the dtype changes."""
		values, vcode = eng.engine_values(out)
		if vcode != self._vcode:
			_ffi.check(_ffi.lib().rk_astarb_set_values_dtype(self._h, vcode, _ffi.stream_ptr()))
			self._vcode = vcode
		return values

	def _step(self, oh, code):
		lib, h = _ffi.lib(), self._h
		_ffi.check(lib.rk_astarb_step_expand(h, oh.data_ptr(), code, _ffi.stream_ptr()))
		self.net_rows_total += len(oh)
		# rows per forward: whole searches, as many as fit NET_SLICE_ROWS -- and exactly ONE search per forward once a search's
		# own batch is that large: then every forward has the shape a sequential AStar would give the net, so the batch can
		# not lose to it through the library's kernel choice (measured at N = 1000, 64 searches, bf16 fc_small: hipBLASLt and
		# torch's BatchNorm pick kernels for 16 384-row forwards that cost three times as much per row as for 12 000 rows)
		K = 12 * self.expansions
		rows = self.net_slice_rows or (K if K >= NET_SLICE_ROWS // 4 else (NET_SLICE_ROWS // K) * K)
		values = self._values(_sliced_value_forward(self._forward, oh, rows))
		self._keep = values
		_ffi.check(lib.rk_astarb_step_commit(h, values.data_ptr(), _ffi.stream_ptr()))

	@no_grad
	def search(self, states: np.ndarray, time_limit: float = None, max_states=None, use_graph: bool = False, poll: int = 8,
	           exact_batch: bool = None) -> np.ndarray:
		"""Runs all searches until each is solved or out of budget / time; returns the bool vector `solved` (S,).
		exact_batch: evaluate the net on exactly the new states of all searches (compacted on the device, one host wait per
		iteration) instead of on the padded (S * 12 N)-row batch.  Default: whenever the net is a torch module with parameters
		(a forward then costs far more than the wait) and the iteration is not replayed as a hipGraph."""
		_ffi.require_gpu()
		t0 = time.perf_counter()
		assert time_limit or max_states is not None
		self.net.eval()
		time_limit = time_limit or 1e10
		S, K = self.n_searches, 12 * self.expansions
		_, _, code = self._begin_net()         # 6x8x6: the searches run in 20-byte form, the net gets 6x8x6 rows (_Net686)
		states = self._roots20(states, S)
		budget = np.minimum(np.broadcast_to(np.asarray(self.capacity if max_states is None else max_states, dtype=np.int64), (S,)),
		                    self.capacity).copy()
		h, lib = self._engine(), _ffi.lib()
		_ffi.check(lib.rk_astarb_reset(h, states.ctypes.data, budget.ctypes.data, self.lambda_, _ffi.stream_ptr()))
		self._vcode = _ffi.OH_F32
		_ffi.check(lib.rk_astarb_set_values_dtype(h, self._vcode, _ffi.stream_ptr()))
		oh = eng.net_batch(S * K, code)
		self.iterations = 0
		self.net_rows_total = 0
		if exact_batch is None:
			exact_batch = not use_graph and callable(getattr(self.net, "parameters", None)) and any(True for _ in self.net.parameters())
		exact_batch = bool(exact_batch) and not use_graph
		if exact_batch:
			self._n_rows = torch.zeros(1, dtype=torch.int32).pin_memory()
			self._counted = torch.cuda.Event()
			self._no_values = torch.zeros(4, dtype=torch.float32, device=gpu)
		step = self._step_exact if exact_batch else self._step
		graph = None
		if use_graph:
			# the warm-up is a real iteration, which also fixes the values' dtype; captured on every search, the graph is not kept
			graph = eng.capture(lambda: self._step(oh, code), lambda: self._step(oh, code))
			self.iterations += 1
		# Steps after a search is done are no-ops on the device but still run the net on the padded batch, so the host must not
		# poll too rarely: a search grows by at most K states per iteration, so no live search can run out of budget in fewer
		# than (budget - states) // K iterations -- poll after that many (at most `poll`).  Round 2's harness polled every 64
		# iterations of a search that needs 12: that, not a kernel, was the 0.22x of profiles/r02_astar_batch.json at N = 1000.
		n_states = np.ones(S, np.int64)
		live = np.ones(S, bool)
		while time.perf_counter() - t0 < time_limit:
			# the live search closest to its budget decides (min over searches of room // K = (min room) // K); none live: one iteration
			room = int((budget[live] - n_states[live]).min()) if live.any() else K
			burst = eng.burst(poll, room, K)
			for _ in range(burst):
				if graph is not None:
					graph.replay()
				else:
					step(oh, code)
			self.iterations += burst
			st = self._poll()
			live, n_states = st[:, 0] == 0, st[:, 2]
			if not live.any():
				break
		return self._poll()[:, 1] != 0

	def action_queue_of(self, search: int) -> deque:
		st = self.status[search]
		if st[1] != 1:                                                   # unsolved, or the start was already solved
			return deque()
		return eng.read_path(_ffi.lib().rk_astarb_path, self._h, search, int(st[5]))

	def arrays_of(self, search: int):
		"""(states, G, parents, parent_actions) of one search, rows 0..n (row 0 unused), in the reference's dtypes."""
		n = int(self._poll()[search, 2])
		states, G, parents, pact = eng.export_pool(_ffi.lib().rk_astarb_export, (self._h, search), n)
		return self._states_out(states, n), G, parents, pact

	def __len__(self):
		return int(self.status[:, 2].sum()) if self.status is not None else 0

	def __str__(self):
		return f"Batched AStar x{self.n_searches} (lambda={self.lambda_}, N={self.expansions})"


class TowardsGoal:
	"""
	Any agent as a solver towards `goal` instead of the solved state: `search` hands the wrapped agent `cube.relative(state, goal)`.
	Relabelling the cubies by a goal commutes with the 12 moves, so the relative state is as far from solved as the state is from
	the goal, the queue that solves it turns `state` into `goal`, and a net trained on the distance to solved is the heuristic for
	the distance to the goal.  Works for the one-state agents (`search(state, time_limit, max_states) -> bool`) and for the batch
	agents (`search(states, ...)` on all rows); `action_queue`, `len()`, `lengths`, `action_queue_of(i)` and every other attribute
	are the wrapped agent's.  States and goal are in the representation cube.get_is2024() names when a method is called.

	`goal` is checked once, here (ValueError unless `cube.is_legal`); with `check_states` every call checks its states the same
	way, at the price of a launch and a synchronisation.
	"""

	def __init__(self, agent, goal, check_states: bool = True):
		rows = cube.cube._rows2024(goal)
		if len(rows) != 1:
			raise ValueError(f"goal must be one state, got {len(rows)}")
		if not cube.is_legal(goal).all():
			raise ValueError("1 of 1 rows of goal are not legal cube states (the first is row 0)")
		self.agent, self.check_states = agent, bool(check_states)
		self._goal20 = rows.copy()

	@property
	def goal(self) -> np.ndarray:
		"""The goal in the current representation."""
		return cube.cube._rows_out(self._goal20)[0]

	def relative(self, states) -> np.ndarray:
		"""`states` (one, or n rows) seen from the goal, in the shape they came in."""
		if self.check_states:
			bad = np.nonzero(~cube.is_legal(states))[0]
			if len(bad):
				raise ValueError(f"{len(bad)} of {len(cube.cube._rows2024(states))} rows of states are not legal cube states (the first is row {bad[0]})")
		rows = cube.cube._rows2024(states)
		if len(rows) == 0:
			return np.asarray(states, dtype=np.int8)
		q = torch.from_numpy(rows).to(gpu)
		rel = cube.device.relative(q, torch.from_numpy(self._goal20).to(gpu), out=q, check=False)
		return cube.cube._rows_out(cube.cube._to_host(rel)).reshape(np.shape(states))

	def search(self, states, *args, **kwargs):
		return self.agent.search(self.relative(states), *args, **kwargs)

	def __getattr__(self, name):
		if name == "agent":                                              # (before __init__ has set it)
			raise AttributeError(name)
		return getattr(self.agent, name)

	def __len__(self):
		return len(self.agent)

	def __str__(self):
		return f"{self.agent} towards a goal"
