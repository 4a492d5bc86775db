// Device-resident breadth-first search (reference: librubiks/solving/agents.py:92-129), sync-free between polls.
//
// What lives in HBM (capacity C states, P = nodes popped per iteration, at most `pops`):
//   states  int8 (C+1, 20)   node pool as 5 x u32 per state, index 0 unused, root = 1   (the keys of `self.states`, :103)
//   parent  int32 (C+1), pact uint8 (C+1)                                                (its values: predecessor, action)
//   table   uint32 (T)       open-addressing hash table state -> index, T = pow2 >= 2C, tentative claims TENT | position
//   ctr     int32[16]        size, head, done, won, winning parent / action, stop reason, iterations, error, ...
// The FIFO queue is the pool itself in index order: the reference appends every new state to the queue as it stores it
// (:120-121) and pops from the front (:106), so the queue is always the index range head .. size.
//
// One iteration pops the P = min(pops, size - head + 1) nodes head .. head + P - 1 (P is read on the device; the grids
// are sized for `pops`) and is four launches, none of which synchronises with the host:
//   k_bfs_expand   one thread per child, parent-major / action-minor in pop order (:108-110): the move, the goal flag, the
//                  membership test against the table and the in-batch first-occurrence election (probe_elect)
//   k_bfs_scan     first-occurrence flags and their exclusive prefix over the batch (tickets + look-back, one launch)
//   k_bfs_append   the cut (below) and the order-preserving append: new states get indices size + 1 ... in batch order
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
// one: that entry first rebuilds the table from the pool (k_bfs_rehash), which drops the claims the cut left behind.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"

namespace rk {

enum {
	B_SIZE = 0, B_HEAD, B_DONE, B_WON, B_WPARENT, B_WACT, B_STOP, B_ITERS, B_ERROR, B_NPOP, B_BUDGET, B_WINPOS, B_TOTAL, B_EPOCH,
	B_TICKET, B_COUNT = 16
};
enum { BFS_STOP_NO = 0, BFS_STOP_WON = 1, BFS_STOP_BUDGET = 2, BFS_STOP_EMPTY = 3, BFS_STOP_ERROR = 4 };
enum { BFS_ERR_NONE = 0, BFS_ERR_CAPACITY = 1 };

constexpr uint32_t NO_WIN = 0x7FFFFFFFu;

struct BfsDev {
	uint32_t mask, cap1;                        // table slots - 1, capacity + 1
	int pops;                                   // the most nodes an iteration pops (grid size)
	uint32_t *states; int32_t *parent; uint8_t *pact; uint32_t *table;
	int32_t *ctr;
	uint32_t *slot; int32_t *rank; uint8_t *first;                   // per child of the batch: claimed slot, exclusive prefix, first occurrence
	unsigned long long *chain;                                        // look-back words {epoch, total} of k_bfs_scan
};

// After a pop count change (reset, budget, end of an iteration): done flags and the next P.  One thread.
__device__ __forceinline__ void bfs_next(const BfsDev &d)
{
	const int32_t size = d.ctr[B_SIZE], head = d.ctr[B_HEAD];
	int stop = BFS_STOP_NO;
	if (size >= d.ctr[B_BUDGET]) stop = BFS_STOP_BUDGET;                // agents.py:105, checked before the next pop
	else if (head > size) stop = BFS_STOP_EMPTY;                         // the whole graph was seen
	const int P = stop ? 0 : min(d.pops, size - head + 1);
	d.ctr[B_STOP] = stop;
	d.ctr[B_DONE] = stop ? 1 : 0;
	d.ctr[B_NPOP] = stop ? 0 : P;
}

// The pops of this iteration, or 0 when it is done -- or when its children might not fit the pool: the host grows the pool
// before such an iteration (rk_bfs_grow), so that never cuts one; should it happen all four kernels skip the iteration and
// k_bfs_end reports an error.  Every kernel of the iteration reads the same counters, so they agree.
__device__ __forceinline__ int bfs_pops(const BfsDev &d)
{
	const int P = d.ctr[B_NPOP];
	return (uint64_t)d.ctr[B_SIZE] + 12ull * (uint64_t)P <= (uint64_t)d.cap1 - 1u ? P : 0;
}

__global__ void k_bfs_root(BfsDev d, const uint32_t *root, int budget)
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
	d.ctr[B_SIZE] = 1; d.ctr[B_HEAD] = 1;
	d.ctr[B_BUDGET] = budget;
	d.ctr[B_WINPOS] = (int32_t)NO_WIN;
	bfs_next(d);
}

__global__ void k_bfs_set_budget(BfsDev d, int budget)
{
	if (threadIdx.x != 0) return;
	d.ctr[B_BUDGET] = budget;
	if (d.ctr[B_WON] || d.ctr[B_ERROR] || d.ctr[B_STOP] == BFS_STOP_EMPTY) return;
	bfs_next(d);
}

// fan-out + goal flag + membership / election: one thread per child                             agents.py:106-112
__global__ __launch_bounds__(256)
void k_bfs_expand(BfsDev d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = bfs_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P) return;
	const int32_t head = d.ctr[B_HEAD];
	const int i = c / 12, a = c - 12 * i;
	uint32_t s[5];
	child_state(d.states, head + i, s_act, (uint32_t)a, s);
	if (is_solved5(s)) atomicMin(reinterpret_cast<uint32_t *>(&d.ctr[B_WINPOS]), (uint32_t)c);
	uint32_t slot = 0;
	const uint32_t e = probe_elect(d.table, d.mask, d.states, s, c,
	                               [&](int c2, uint32_t o[5]) { child_state(d.states, head + c2 / 12, s_act, (uint32_t)(c2 % 12), o); }, &slot);
	d.slot[c] = e == 0u ? slot : NO_SLOT;
}

// first-occurrence flags and their exclusive prefix in batch order (tickets + look-back: rk_search_dev.h)
__global__ __launch_bounds__(ASCAN)
void k_bfs_scan(BfsDev d)
{
	const int P = bfs_pops(d);
	if (P == 0) return;                                                  // done: no ticket drawn, nothing to reset
	frontier_scan(d.slot, d.table, d.rank, d.first, d.chain, &d.ctr[B_TICKET], (uint32_t)d.ctr[B_EPOCH] + 1u, &d.ctr[B_TOTAL], 12 * P);
}

// the cut and the append: child c is stored iff it is a first occurrence, lies before the winning position and its pop
// runs -- size_before + (new states of the earlier pops) < max_states.  That prefix only grows along the batch, so this is
// exactly "c is before the cut".                                                                  agents.py:105, :111-121
__global__ __launch_bounds__(256)
void k_bfs_append(BfsDev d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = bfs_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P || !d.first[c]) return;
	if ((uint32_t)c >= (uint32_t)d.ctr[B_WINPOS]) return;
	const int i = c / 12, a = c - 12 * i;
	const int32_t size0 = d.ctr[B_SIZE];
	if ((long long)size0 + d.rank[12 * i] >= (long long)d.ctr[B_BUDGET]) return;
	const uint32_t idx = (uint32_t)size0 + 1u + (uint32_t)d.rank[c];
	if (idx >= d.cap1) { d.ctr[B_ERROR] = BFS_ERR_CAPACITY; return; }
	const int32_t p = d.ctr[B_HEAD] + i;
	uint32_t s[5];
	child_state(d.states, p, s_act, (uint32_t)a, s);
	#pragma unroll
	for (int j = 0; j < 5; j++) d.states[(size_t)idx * 5 + j] = s[j];
	d.parent[idx] = p;
	d.pact[idx] = (uint8_t)a;
	d.table[d.slot[c]] = idx;
}

// where the cut fell, the new size / head, the done flags, the next P; resets the per-iteration counters.  One thread.
__global__ void k_bfs_end(BfsDev d)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (d.ctr[B_NPOP] == 0) return;
	const int P = bfs_pops(d);
	if (P == 0) {
		d.ctr[B_ERROR] = BFS_ERR_CAPACITY;
		d.ctr[B_STOP] = BFS_STOP_ERROR; d.ctr[B_DONE] = 1; d.ctr[B_NPOP] = 0;
		return;
	}
	const int32_t size0 = d.ctr[B_SIZE], head = d.ctr[B_HEAD];
	const long long budget = d.ctr[B_BUDGET];
	const int lo = first_refused_pop(d.rank, P, size0, budget);         // the first pop that fails the budget check (P: none)
	const int cut_b = 12 * lo;
	const int win = d.ctr[B_WINPOS];
	const int cut = min(cut_b, win);
	const int n_new = cut < 12 * P ? d.rank[cut] : d.ctr[B_TOTAL];
	d.ctr[B_SIZE] = size0 + n_new;
	d.ctr[B_ITERS] += 1;
	d.ctr[B_TICKET] = 0;
	d.ctr[B_EPOCH] += 1;
	d.ctr[B_WINPOS] = (int32_t)NO_WIN;
	if (d.ctr[B_ERROR]) {
		d.ctr[B_STOP] = BFS_STOP_ERROR; d.ctr[B_DONE] = 1; d.ctr[B_NPOP] = 0;
	} else if (win < cut_b) {                                            // agents.py:113-118
		d.ctr[B_WON] = 1;
		d.ctr[B_WPARENT] = head + win / 12;
		d.ctr[B_WACT] = win % 12;
		d.ctr[B_HEAD] = head + win / 12 + 1;
		d.ctr[B_STOP] = BFS_STOP_WON; d.ctr[B_DONE] = 1; d.ctr[B_NPOP] = 0;
	} else if (lo < P) {                                                 // agents.py:105 failed before pop `lo`
		d.ctr[B_HEAD] = head + lo;
		d.ctr[B_STOP] = BFS_STOP_BUDGET; d.ctr[B_DONE] = 1; d.ctr[B_NPOP] = 0;
	} else {
		d.ctr[B_HEAD] = head + P;
		bfs_next(d);
	}
}

// After a growth: every stored state back into the larger, cleared table.  Between iterations of a running search no slot
// is tentative, so this is a plain insert of indices 1..size.
__global__ __launch_bounds__(256)
void k_bfs_rehash(BfsDev d)
{
	rehash_pool(d.states, d.table, d.mask, d.ctr[B_SIZE], 1 + blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// the action queue of a won search: the path to the winner's parent, then the winner's action (agents.py:114-117).
// out[0] = length or -1 (no win, broken chain), then the actions root -> winner.
__global__ void k_bfs_walk(BfsDev d, int32_t *out, int max_len)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (!d.ctr[B_WON]) { out[0] = -1; return; }
	const int index = d.ctr[B_WPARENT];
	int len = 0, i = index;
	while (i != 1) {
		i = d.parent[i];
		len++;
		if (i < 1 || (uint32_t)i >= d.cap1 || len > (int)d.cap1) { out[0] = -1; return; }
	}
	out[0] = len + 1;
	if (len < max_len) out[1 + len] = d.ctr[B_WACT];
	i = index;
	for (int k = len - 1; k >= 0; k--) {
		if (k < max_len) out[1 + k] = d.pact[i];
		i = d.parent[i];
	}
}

}  // namespace rk

using namespace rk;

struct rk_bfs {
	BfsDev d{};
	size_t cap = 0;
	uint32_t *root_dev = nullptr;
	int32_t *walk = nullptr;
	Landing ctr_host;                           // page-locked landing place of the counter block
	bool ready = false;
	DevPool pool{64};
};

namespace {

constexpr int BFS_WALK_MAX = 1 << 12;

uint32_t bfs_table_mask(size_t capacity) { return (uint32_t)(table_slots(capacity, 1024) - 1); }

int bfs_read_ctr(rk_bfs *h, int32_t *out, hipStream_t st) { return h->ctr_host.read(h->d.ctr, B_COUNT, out, st); }

}  // namespace

extern "C" {

int rk_bfs_create(rk_bfs_t **out, size_t capacity, int pops)
{
	if (!out) return fail(RK_EINVAL, "rk_bfs_create: null out pointer");
	if (capacity < 2 || capacity > 0x3FFFFFF0ull) return fail(RK_EINVAL, "rk_bfs_create: capacity %zu out of range", capacity);
	if (pops < 1 || pops > (1 << 22)) return fail(RK_EINVAL, "rk_bfs_create: pops %d outside 1..%d", pops, 1 << 22);
	rk_bfs *h = new rk_bfs();
	h->cap = capacity;
	BfsDev &d = h->d;
	d.pops = pops;
	d.cap1 = (uint32_t)(capacity + 1);
	d.mask = bfs_table_mask(capacity);
	const size_t C1 = capacity + 1, K = (size_t)12 * pops;
	int e = RK_OK;
	#define A(ptr, cnt) if (!e) e = h->pool.alloc(&d.ptr, (cnt))
	A(states, C1 * 5); A(parent, C1); A(pact, C1); A(table, (size_t)d.mask + 1); A(ctr, B_COUNT);
	A(slot, K); A(rank, K); A(first, K); A(chain, frontier_scan_blocks(pops));
	#undef A
	if (!e) e = h->pool.alloc(&h->root_dev, 8);
	if (!e) e = h->pool.alloc(&h->walk, BFS_WALK_MAX + 8);
	if (!e) h->ctr_host.reserve(B_COUNT);
	if (e) { rk_bfs_destroy(h); return e; }
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
	BfsDev &d = h->d;
	RK_HIP(hipMemsetAsync(d.table, 0, ((size_t)d.mask + 1) * sizeof(uint32_t), st));
	RK_HIP(hipMemsetAsync(d.chain, 0, frontier_scan_blocks(d.pops) * sizeof(unsigned long long), st));      // look-back epochs restart
	RK_HIP(hipMemcpyAsync(h->root_dev, h_start_state, STATE_BYTES, hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(k_bfs_root, dim3(1), dim3(64), 0, st, d, h->root_dev, budget_of(max_states));
	RK_HIP(hipGetLastError());
	RK_HIP(hipStreamSynchronize(st));       // the host buffer may go away after return
	h->ready = true;
	return RK_OK;
}

int rk_bfs_set_budget(rk_bfs_t *h, long long max_states, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bfs_set_budget: reset the engine first");
	hipStream_t st = (hipStream_t)stream;
	int32_t c[B_COUNT];
	if (int e = bfs_read_ctr(h, c, st)) return e;
	if (c[B_STOP] == BFS_STOP_BUDGET) {
		// A budget stop inside a batch leaves the tentative claims (TENT | position) of the first occurrences at or after the cut in
		// the table.  A search that goes on would take them for claims of ITS batch positions: rebuild the table from the pool first.
		const BfsDev &d = h->d;
		RK_HIP(hipMemsetAsync(d.table, 0, ((size_t)d.mask + 1) * sizeof(uint32_t), st));
		hipLaunchKernelGGL(k_bfs_rehash, dim3(std::max<unsigned>(1u, std::min<unsigned>(blocks((size_t)c[B_SIZE] + 1), 4096u))), dim3(256), 0, st, d);
		RK_HIP(hipGetLastError());
	}
	hipLaunchKernelGGL(k_bfs_set_budget, dim3(1), dim3(64), 0, st, h->d, budget_of(max_states));
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_bfs_run(rk_bfs_t *h, int iterations, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bfs_run: reset the engine first");
	if (iterations < 0) return fail(RK_EINVAL, "rk_bfs_run: iterations %d < 0", iterations);
	hipStream_t st = (hipStream_t)stream;
	const BfsDev &d = h->d;
	const unsigned grid = blocks((size_t)12 * d.pops);
	for (int it = 0; it < iterations; it++) {
		hipLaunchKernelGGL(k_bfs_expand, dim3(grid), dim3(256), 0, st, d);
		hipLaunchKernelGGL(k_bfs_scan, dim3(blocks((size_t)12 * d.pops, ASCAN)), dim3(ASCAN), 0, st, d);
		hipLaunchKernelGGL(k_bfs_append, dim3(grid), dim3(256), 0, st, d);
		hipLaunchKernelGGL(k_bfs_end, dim3(1), dim3(64), 0, st, d);
	}
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_bfs_status(rk_bfs_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_bfs_status: bad argument");
	int32_t c[B_COUNT];
	if (int e = bfs_read_ctr(h, c, (hipStream_t)stream)) return e;
	h_status[0] = c[B_DONE]; h_status[1] = c[B_WON]; h_status[2] = c[B_SIZE]; h_status[3] = c[B_ITERS];
	h_status[4] = c[B_HEAD]; h_status[5] = c[B_STOP]; h_status[6] = c[B_ERROR]; h_status[7] = c[B_NPOP];
	return RK_OK;
}

int rk_bfs_grow(rk_bfs_t *h, size_t new_capacity, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bfs_grow: reset the engine first");
	if (new_capacity <= h->cap) return new_capacity == h->cap ? RK_OK : fail(RK_EINVAL, "rk_bfs_grow: %zu is below the current capacity %zu", new_capacity, h->cap);
	if (new_capacity > 0x3FFFFFF0ull) return fail(RK_EINVAL, "rk_bfs_grow: capacity %zu out of range", new_capacity);
	hipStream_t st = (hipStream_t)stream;
	const BfsDev old = h->d;
	BfsDev d = old;
	const size_t C1 = new_capacity + 1, C1_old = h->cap + 1;
	d.cap1 = (uint32_t)C1;
	d.mask = bfs_table_mask(new_capacity);
	Growth g(h->pool, "rk_bfs_grow");
	g.request(&d.states, C1 * 5); g.request(&d.parent, C1); g.request(&d.pact, C1); g.request(&d.table, (size_t)d.mask + 1);
	if (!g.granted()) return fail(RK_ECAPACITY, "rk_bfs_grow: no device memory for a pool of %zu states", new_capacity);
	const int e = g.fill(st, [&]() -> hipError_t {
		RK_FILL(hipMemcpyAsync(d.states, old.states, C1_old * STATE_BYTES, hipMemcpyDeviceToDevice, st));
		RK_FILL(hipMemcpyAsync(d.parent, old.parent, C1_old * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
		RK_FILL(hipMemcpyAsync(d.pact, old.pact, C1_old, hipMemcpyDeviceToDevice, st));
		RK_FILL(hipMemsetAsync(d.table, 0, ((size_t)d.mask + 1) * sizeof(uint32_t), st));
		hipLaunchKernelGGL(k_bfs_rehash, dim3(std::min<unsigned>(blocks(C1_old), 4096u)), dim3(256), 0, st, d);
		return hipGetLastError();
	});
	if (e) return e;
	g.commit();
	h->d = d;
	h->cap = new_capacity;
	return RK_OK;
}

long long rk_bfs_size(const rk_bfs_t *hc)
{
	rk_bfs_t *h = const_cast<rk_bfs_t *>(hc);
	if (!h || !h->ready) return 0;
	int32_t c[B_COUNT];
	if (bfs_read_ctr(h, c, nullptr)) return RK_EHIP;
	return c[B_SIZE];
}

int rk_bfs_export(rk_bfs_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bfs_export: reset the engine first");
	if (first + count > h->cap + 1) return fail(RK_EINVAL, "rk_bfs_export: rows %zu..%zu outside the pool", first, first + count);
	if (count == 0) return RK_OK;
	hipStream_t st = (hipStream_t)stream;
	const BfsDev &d = h->d;
	Widened<int32_t, long long> p;
	Widened<uint8_t, long long> a;
	if (h_states) RK_HIP(hipMemcpyAsync(h_states, d.states + first * 5, count * STATE_BYTES, hipMemcpyDeviceToHost, st));
	if (int e = p.start(d.parent + first, count, h_parents, st)) return e;
	if (int e = a.start(d.pact + first, count, h_actions, st)) return e;
	RK_HIP(hipStreamSynchronize(st));
	p.finish(); a.finish();
	return RK_OK;
}

long long rk_bfs_path(rk_bfs_t *h, long long *h_actions, size_t max_len, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bfs_path: reset the engine first");
	if (!h_actions && max_len > 0) return fail(RK_EINVAL, "rk_bfs_path: null h_actions with max_len %zu", max_len);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_bfs_walk, dim3(1), dim3(64), 0, st, h->d, h->walk, BFS_WALK_MAX);
	RK_HIP(hipGetLastError());
	int32_t len = 0;
	if (int e = read_walk(h->walk, BFS_WALK_MAX, h_actions, max_len, st, &len)) return e;
	if (len < 0) return fail(RK_ESTATE, "rk_bfs_path: the search has not won (or its parent chain is broken)");
	return (long long)len;
}

}  // extern "C"
