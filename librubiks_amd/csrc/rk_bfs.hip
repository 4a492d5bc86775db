// Device-resident breadth-first search (reference: librubiks/solving/agents.py:92-129), sync-free between polls.
//
// What lives in HBM (capacity C states, P = nodes popped per iteration, at most `pops`):
//   states  int8 (C+1, 20)   node pool as 5 x u32 per state, index 0 unused, root = 1   (the keys of `self.states`, :103)
//   parent  int32 (C+1), pact uint8 (C+1)                                                (its values: predecessor, action)
//   table   uint32 (T)       open-addressing hash table state -> index, T = pow2 >= 2C, tentative claims TENT | position
//   ctr     int32[16]        size, head, done, won, winning parent / action, stop reason, iterations, error, ...
// The pool, its counters and the scan, append, end and rehash launches are the frontier pool's (rk_frontier_dev.h, FrontierPool
// in rk_frontier_host.h); this file holds what is BFS's own: the stopping rule (bfs_next), the root, the goal test and membership
// rule (k_bfs_expand) and the walk.
// The FIFO queue is the pool itself in index order: the reference appends every new state to the queue as it stores it
// (:120-121) and pops from the front (:106), so the queue is always the index range head .. size.
//
// One iteration pops the P = min(pops, size - head + 1) nodes head .. head + P - 1 (P is read on the device; the grids
// are sized for `pops`) and is four launches, none of which synchronises with the host:
//   k_bfs_expand   one thread per child, parent-major / action-minor in pop order (:108-110): the move, the goal flag, the
//                  membership test against the table and the in-batch first-occurrence election (probe_elect)
//   k_fr_scan      first-occurrence flags and their exclusive prefix over the batch (tickets + look-back, one launch)
//   k_fr_append    the cut (below) and the order-preserving append: new states get indices size + 1 ... in batch order
//                  with their parent and action (:120-121), their tentative claims become those indices
//   k_bfs_end      one thread: where the cut fell, the new size and head, the done flags, the next P
// The reference checks `len(self) < max_states` before EVERY pop (:105) and returns a solved child BEFORE storing it
// (:111-118).  So pop j of the batch runs only if size_before + (new states of the pops before j) < max_states -- the
// first pop that fails ends the search -- and the winning child is the lowest batch position with a solved state among
// the pops that run.  The cut is min(12 x the first failing pop, the first solved position); no child at or after it is
// appended or counted.  Claims at or after the cut are left in the table only when the search has ended (rk_bfs_set_budget
// rebuilds the table before a search stopped by its budget goes on).
//
// The time limit is checked on the host clock whenever the host polls (every few iterations), where the reference checks
// before every pop: a time-limited run does not stop at the reference's state.  The pool is never what cuts an iteration:
// the host grows it (rk_bfs_grow) before an iteration whose children might not fit (size + 12 P > C); should one be launched
// anyway, it is skipped and reported as an error.  A search stopped by its budget goes on after rk_bfs_set_budget with a larger
// one: that entry first rebuilds the table from the pool (k_fr_rehash), which drops the claims the cut left behind.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_frontier_dev.h"
#include "rk_frontier_host.h"

namespace rk {

constexpr int B_COUNT = 16;                     // the common counter words, none of its own

// After a pop count change (reset, budget, end of an iteration): done flags and the next P.  One thread.
__device__ __forceinline__ void bfs_next(const FrontierDev &d)
{
	const int32_t size = d.ctr[F_SIZE], head = d.ctr[F_HEAD];
	int stop = F_STOP_NO;
	if (size >= d.ctr[F_BUDGET]) stop = F_STOP_BUDGET;                  // agents.py:105, checked before the next pop
	else if (head > size) stop = F_STOP_EMPTY;                           // the whole graph was seen
	const int P = stop ? 0 : min(d.pops, size - head + 1);
	d.ctr[F_STOP] = stop;
	d.ctr[F_DONE] = stop ? 1 : 0;
	d.ctr[F_NPOP] = stop ? 0 : P;
}

__global__ void k_bfs_root(FrontierDev d, const uint32_t *root, int budget)
{
	const int tid = threadIdx.x;
	if (tid < B_COUNT) d.ctr[tid] = 0;
	__syncthreads();
	if (tid != 0) return;
	uint32_t s[5];
	load5(root, s);
	#pragma unroll
	for (int j = 0; j < 5; j++) d.states[5 + j] = s[j];
	d.parent[1] = 0; d.pact[1] = 0;                                      // self.states = {state: (None, None)}   agents.py:103
	d.table[hash_state(s) & d.mask] = 1u;
	d.ctr[F_SIZE] = 1; d.ctr[F_HEAD] = 1;
	d.ctr[F_BUDGET] = budget;
	d.ctr[F_WINPOS] = (int32_t)F_NO_WIN;
	bfs_next(d);
}

__global__ void k_bfs_set_budget(FrontierDev d, int budget)
{
	if (threadIdx.x != 0) return;
	d.ctr[F_BUDGET] = budget;
	if (d.ctr[F_WON] || d.ctr[F_ERROR] || d.ctr[F_STOP] == F_STOP_EMPTY) return;
	bfs_next(d);
}

// fan-out + goal flag + membership / election: one thread per child                             agents.py:106-112
__global__ __launch_bounds__(256)
void k_bfs_expand(FrontierDev d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = fr_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P) return;
	const int32_t head = d.ctr[F_HEAD];
	const int i = c / 12, a = c - 12 * i;
	uint32_t s[5];
	child_state(d.states, head + i, s_act, (uint32_t)a, s);
	if (is_solved5(s)) atomicMin(reinterpret_cast<uint32_t *>(&d.ctr[F_WINPOS]), (uint32_t)c);
	uint32_t slot = 0;
	const uint32_t e = probe_elect(d.table, d.mask, d.states, s, c,
	                               [&](int c2, uint32_t o[5]) { child_state(d.states, head + c2 / 12, s_act, (uint32_t)(c2 % 12), o); }, &slot);
	d.slot[c] = e == 0u ? slot : NO_SLOT;
}

// neither a meeting node nor a popped count: status word 4 is the head
__global__ void k_bfs_end(FrontierDev d)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	fr_end<F_UNRECORDED, F_UNRECORDED>(d, [](const FrontierDev &x) { bfs_next(x); });
}

// the action queue of a won search: the path to the winner's parent, then the winner's action (agents.py:114-117).
// out[0] = length or -1 (no win, broken chain), then the actions root -> winner.
__global__ void k_bfs_walk(FrontierDev d, int32_t *out, int max_len)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (!d.ctr[F_WON]) { out[0] = -1; return; }
	const int index = d.ctr[F_WPARENT];
	int len = 0, i = index;
	while (i != 1) {
		i = d.parent[i];
		len++;
		if (i < 1 || (uint32_t)i >= d.cap1 || len > (int)d.cap1) { out[0] = -1; return; }
	}
	out[0] = len + 1;
	if (len < max_len) out[1 + len] = d.ctr[F_WACT];
	i = index;
	for (int k = len - 1; k >= 0; k--) {
		if (k < max_len) out[1 + k] = d.pact[i];
		i = d.parent[i];
	}
}

}  // namespace rk

using namespace rk;

struct rk_bfs : FrontierPool {};

extern "C" {

int rk_bfs_create(rk_bfs_t **out, size_t capacity, int pops)
{
	if (!out) return fail(RK_EINVAL, "rk_bfs_create: null out pointer");
	if (int e = FrontierPool::check_create("rk_bfs_create", capacity, pops)) return e;
	rk_bfs *h = new rk_bfs();
	if (int e = h->alloc(capacity, pops, B_COUNT)) { delete h; return e; }
	*out = h;
	return RK_OK;
}

int rk_bfs_destroy(rk_bfs_t *h)
{
	delete h;                                   // the pool and the landing buffer go with it
	return RK_OK;
}

int rk_bfs_reset(rk_bfs_t *h, const int8_t *h_start_state, long long max_states, void *stream)
{
	if (!h || !h_start_state) return fail(RK_EINVAL, "rk_bfs_reset: null argument");
	hipStream_t st = (hipStream_t)stream;
	return h->reset(h_start_state, st, [&] { hipLaunchKernelGGL(k_bfs_root, dim3(1), dim3(64), 0, st, h->d, h->root_dev, budget_of(max_states)); });
}

int rk_bfs_set_budget(rk_bfs_t *h, long long max_states, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bfs_set_budget")) return e;
	hipStream_t st = (hipStream_t)stream;
	int32_t c[B_COUNT];
	if (int e = h->read_ctr(c, st)) return e;
	// A budget stop inside a batch leaves the tentative claims (TENT | position) of the first occurrences at or after the cut in
	// the table.  A search that goes on would take them for claims of ITS batch positions: rebuild the table from the pool first.
	if (c[F_STOP] == F_STOP_BUDGET) RK_HIP(FrontierPool::rebuild_table(h->d, (size_t)c[F_SIZE] + 1, st));
	hipLaunchKernelGGL(k_bfs_set_budget, dim3(1), dim3(64), 0, st, h->d, budget_of(max_states));
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_bfs_run(rk_bfs_t *h, int iterations, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bfs_run")) return e;
	hipStream_t st = (hipStream_t)stream;
	// the append is the shared one: the winning child is the first solved one and is returned before it is stored (agents.py:105,
	// :111-121), which is fr_append's cut at F_WINPOS
	return h->run("rk_bfs_run", iterations, st, [&](unsigned grid) { hipLaunchKernelGGL(k_bfs_expand, dim3(grid), dim3(256), 0, st, h->d); },
	              k_fr_append, k_bfs_end);
}

int rk_bfs_status(rk_bfs_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_bfs_status: bad argument");
	int32_t c[B_COUNT];
	if (int e = h->read_ctr(c, (hipStream_t)stream)) return e;
	h_status[0] = c[F_DONE]; h_status[1] = c[F_WON]; h_status[2] = c[F_SIZE]; h_status[3] = c[F_ITERS];
	h_status[4] = c[F_HEAD]; h_status[5] = c[F_STOP]; h_status[6] = c[F_ERROR]; h_status[7] = c[F_NPOP];
	return RK_OK;
}

int rk_bfs_grow(rk_bfs_t *h, size_t new_capacity, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bfs_grow")) return e;
	return h->grow("rk_bfs_grow", new_capacity, (hipStream_t)stream);
}

long long rk_bfs_size(const rk_bfs_t *h) { return FrontierPool::size(h); }

int rk_bfs_export(rk_bfs_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bfs_export")) return e;
	return h->export_rows("rk_bfs_export", first, count, h_states, h_parents, h_actions, nullptr, (hipStream_t)stream);
}

long long rk_bfs_path(rk_bfs_t *h, long long *h_actions, size_t max_len, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bfs_path")) return e;
	if (!h_actions && max_len > 0) return fail(RK_EINVAL, "rk_bfs_path: null h_actions with max_len %zu", max_len);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_bfs_walk, dim3(1), dim3(64), 0, st, h->d, h->walk, FRONTIER_WALK_MAX);
	RK_HIP(hipGetLastError());
	int32_t len = 0;
	if (int e = read_walk(h->walk, FRONTIER_WALK_MAX, h_actions, max_len, st, &len)) return e;
	if (len < 0) return fail(RK_ESTATE, "rk_bfs_path: the search has not won (or its parent chain is broken)");
	return (long long)len;
}

}  // extern "C"
