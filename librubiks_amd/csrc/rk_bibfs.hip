// Device-resident two-sided breadth-first search: shortest solutions in the quarter-turn metric, sync-free between polls.
//
// Two balls grow in ONE pool in index order, side S around the start (node 1) and side G around the solved state (node 2), one
// level at a time: S while both sides have as many complete levels (f == b), else G.  The parents of a level are popped in index
// order, their children taken in action order; a child that its own side already holds is skipped, a child that the OTHER side
// holds is the meeting -- the search ends there and the child is not stored --, every other child is appended with its parent,
// its action and its side.  With f and b complete levels and no meeting so far every solution has at least f + b + 1 moves, and
// a meeting while level f + 1 (or b + 1) grows has exactly that many: the first meeting is a shortest solution.
//
// What lives in HBM (capacity C states, P = nodes popped per iteration, at most `pops`):
//   states  int8 (C+1, 20)   node pool as 5 x u32 per state, index 0 unused
//   parent  int32 (C+1), pact uint8 (C+1)     predecessor; action | side << 4 (side 0 = S, 1 = G)
//   table   uint32 (T)       open-addressing hash table state -> index over BOTH sides, T = pow2 >= 2C, claims TENT | position
//   ctr     int32[32]        size, head, side, depths, the newest level of each side, done flags, the meeting, ...
// Each side's newest level is a contiguous index range; the level that grows is appended behind everything stored so far.
//
// One iteration pops the P = min(pops, what is left of the level) nodes head .. head + P - 1, never across a level boundary,
// in the four launches of rk_bfs.hip (the scan and the budget bisection are the same code, rk_search_dev.h):
//   k_bibfs_expand   one thread per child: the move, the look-up in the table; a stored state of the growing side is skipped, one
//                    of the other side enters its batch position for the meeting, a new state takes part in the election
//   k_bibfs_scan     first-occurrence flags and their exclusive prefix over the batch
//   k_bibfs_append   the order-preserving append before the cut, with the side bit
//   k_bibfs_end      one thread: the cut, the new size and head, the meeting, the end of a level (depth, ranges, next side)
// The budget is the per-pop rule of rk_bfs: pop j of the batch runs only if size_before + (new states of the pops before j) <
// max_states.  The cut is min(12 x the first refused pop, the lowest batch position of a meeting); nothing at or after it is
// stored or counted, so the pool, the depths and the action queue do not depend on `pops`.  Claims at or after the cut stay in
// the table only when the search has ended (rk_bibfs_reset clears it).  The host grows the pool before an iteration whose
// children might not fit (rk_bibfs_grow); one launched anyway is skipped and reported as an error.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"

namespace rk {

enum {
	W_SIZE = 0, W_HEAD, W_DONE, W_WON, W_WPARENT, W_WACT, W_STOP, W_ITERS, W_ERROR, W_NPOP, W_BUDGET, W_WINPOS, W_TOTAL, W_EPOCH,
	W_TICKET, W_SIDE, W_DEPTH /* [2] */, W_LO = W_DEPTH + 2 /* [2] */, W_HI = W_LO + 2 /* [2] */, W_NEWLO = W_HI + 2, W_MEET, W_POPPED,
	W_COUNT = 32
};
enum { BI_STOP_NO = 0, BI_STOP_WON = 1, BI_STOP_BUDGET = 2, BI_STOP_EMPTY = 3, BI_STOP_ERROR = 4 };
enum { BI_ERR_NONE = 0, BI_ERR_CAPACITY = 1 };

constexpr uint32_t BI_NO_WIN = 0x7FFFFFFFu;
constexpr uint32_t SIDE_SHIFT = 4;              // pact = action | side << 4

struct BiDev {
	uint32_t mask, cap1;                        // table slots - 1, capacity + 1
	int pops;                                   // the most nodes an iteration pops (grid size)
	uint32_t *states; int32_t *parent; uint8_t *pact; uint32_t *table;
	int32_t *ctr;
	uint32_t *slot; int32_t *rank; uint8_t *first;                   // per child of the batch: claimed slot (or TENT | meeting node), exclusive prefix, first occurrence
	unsigned long long *chain;                                        // look-back words of k_bibfs_scan
};

// After a pop count change (reset, end of an iteration): the end of a level, the done flags and the next P.  One thread.
__device__ __forceinline__ void bibfs_next(const BiDev &d)
{
	const int32_t size = d.ctr[W_SIZE];
	int side = d.ctr[W_SIDE];
	int32_t head = d.ctr[W_HEAD];
	if (head > d.ctr[W_HI + side]) {                                     // the level is exhausted and nothing met: it is complete
		d.ctr[W_DEPTH + side] += 1;
		d.ctr[W_LO + side] = d.ctr[W_NEWLO];
		d.ctr[W_HI + side] = size;
		side = d.ctr[W_DEPTH] == d.ctr[W_DEPTH + 1] ? 0 : 1;             // equal level sizes on both sides: alternate
		head = d.ctr[W_LO + side];
		d.ctr[W_SIDE] = side;
		d.ctr[W_HEAD] = head;
		d.ctr[W_NEWLO] = size + 1;
	}
	const int32_t hi = d.ctr[W_HI + side];
	int stop = BI_STOP_NO;
	if (head > hi) stop = BI_STOP_EMPTY;                                 // a level without a state: the whole graph was seen
	else if (size >= d.ctr[W_BUDGET]) stop = BI_STOP_BUDGET;            // checked before the next pop
	const int P = stop ? 0 : min(d.pops, hi - head + 1);
	d.ctr[W_STOP] = stop;
	d.ctr[W_DONE] = stop ? 1 : 0;
	d.ctr[W_NPOP] = stop ? 0 : P;
}

// The pops of this iteration, or 0 when it is done or its children might not fit the pool (rk_bfs.hip: bfs_pops).
__device__ __forceinline__ int bibfs_pops(const BiDev &d)
{
	const int P = d.ctr[W_NPOP];
	return (uint64_t)d.ctr[W_SIZE] + 12ull * (uint64_t)P <= (uint64_t)d.cap1 - 1u ? P : 0;
}

__global__ void k_bibfs_root(BiDev d, const uint32_t *root, int budget)
{
	const int tid = threadIdx.x;
	if (tid < W_COUNT) d.ctr[tid] = 0;
	__syncthreads();
	if (tid != 0) return;
	uint32_t s[5], g[5];
	load5(root, s);
	#pragma unroll
	for (int j = 0; j < 5; j++) { g[j] = SOLVED_DW[j]; d.states[5 + j] = s[j]; d.states[10 + j] = g[j]; }
	d.parent[1] = 0; d.pact[1] = 0;
	d.parent[2] = 0; d.pact[2] = (uint8_t)(1u << SIDE_SHIFT);
	const uint32_t s1 = hash_state(s) & d.mask;
	uint32_t s2 = hash_state(g) & d.mask;
	if (s2 == s1) s2 = (s2 + 1) & d.mask;
	d.table[s1] = 1u; d.table[s2] = 2u;
	d.ctr[W_SIZE] = 2; d.ctr[W_HEAD] = 1;
	d.ctr[W_LO] = 1; d.ctr[W_HI] = 1; d.ctr[W_LO + 1] = 2; d.ctr[W_HI + 1] = 2;
	d.ctr[W_NEWLO] = 3;
	d.ctr[W_BUDGET] = budget;
	d.ctr[W_WINPOS] = (int32_t)BI_NO_WIN;
	bibfs_next(d);
}

// fan-out + membership on either side + election among the new states: one thread per child
__global__ __launch_bounds__(256)
void k_bibfs_expand(BiDev d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = bibfs_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P) return;
	const int32_t head = d.ctr[W_HEAD];
	const uint32_t side = (uint32_t)d.ctr[W_SIDE];
	const int i = c / 12, a = c - 12 * i;
	uint32_t s[5];
	child_state(d.states, head + i, s_act, (uint32_t)a, s);
	uint32_t slot = 0;
	const uint32_t e = probe_elect(d.table, d.mask, d.states, s, c,
	                               [&](int c2, uint32_t o[5]) { child_state(d.states, head + c2 / 12, s_act, (uint32_t)(c2 % 12), o); }, &slot);
	if (e == 0u) { d.slot[c] = slot; return; }
	// a stored state: every node of the other side was stored before this level began, so e is final and so is its side bit
	if ((uint32_t)(d.pact[e] >> SIDE_SHIFT) == side) { d.slot[c] = NO_SLOT; return; }
	atomicMin(reinterpret_cast<uint32_t *>(&d.ctr[W_WINPOS]), (uint32_t)c);
	d.slot[c] = TENT | e;                                                // no claim (TENT bit); k_bibfs_end reads the meeting node here
}

__global__ __launch_bounds__(ASCAN)
void k_bibfs_scan(BiDev d)
{
	const int P = bibfs_pops(d);
	if (P == 0) return;                                                  // done: no ticket drawn, nothing to reset
	frontier_scan(d.slot, d.table, d.rank, d.first, d.chain, &d.ctr[W_TICKET], (uint32_t)d.ctr[W_EPOCH] + 1u, &d.ctr[W_TOTAL], 12 * P);
}

// child c is stored iff it is a first occurrence before the cut (rk_bfs.hip: k_bfs_append), with the side that grows
__global__ __launch_bounds__(256)
void k_bibfs_append(BiDev d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = bibfs_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P || !d.first[c]) return;
	if ((uint32_t)c >= (uint32_t)d.ctr[W_WINPOS]) return;
	const int i = c / 12, a = c - 12 * i;
	const int32_t size0 = d.ctr[W_SIZE];
	if ((long long)size0 + d.rank[12 * i] >= (long long)d.ctr[W_BUDGET]) return;
	const uint32_t idx = (uint32_t)size0 + 1u + (uint32_t)d.rank[c];
	if (idx >= d.cap1) { d.ctr[W_ERROR] = BI_ERR_CAPACITY; return; }
	const int32_t p = d.ctr[W_HEAD] + i;
	uint32_t s[5];
	child_state(d.states, p, s_act, (uint32_t)a, s);
	#pragma unroll
	for (int j = 0; j < 5; j++) d.states[(size_t)idx * 5 + j] = s[j];
	d.parent[idx] = p;
	d.pact[idx] = (uint8_t)((uint32_t)a | ((uint32_t)d.ctr[W_SIDE] << SIDE_SHIFT));
	d.table[d.slot[c]] = idx;
}

// where the cut fell, the new size / head, the meeting, the end of a level, the next P.  One thread, ordinary stores.
__global__ void k_bibfs_end(BiDev d)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (d.ctr[W_NPOP] == 0) return;
	const int P = bibfs_pops(d);
	if (P == 0) {
		d.ctr[W_ERROR] = BI_ERR_CAPACITY;
		d.ctr[W_STOP] = BI_STOP_ERROR; d.ctr[W_DONE] = 1; d.ctr[W_NPOP] = 0;
		return;
	}
	const int32_t size0 = d.ctr[W_SIZE], head = d.ctr[W_HEAD];
	const int lo = first_refused_pop(d.rank, P, size0, d.ctr[W_BUDGET]);
	const int cut_b = 12 * lo;
	const int win = d.ctr[W_WINPOS];
	const int cut = min(cut_b, win);
	const int n_new = cut < 12 * P ? d.rank[cut] : d.ctr[W_TOTAL];
	d.ctr[W_SIZE] = size0 + n_new;
	d.ctr[W_ITERS] += 1;
	d.ctr[W_TICKET] = 0;
	d.ctr[W_EPOCH] += 1;
	d.ctr[W_WINPOS] = (int32_t)BI_NO_WIN;
	if (d.ctr[W_ERROR]) {
		d.ctr[W_STOP] = BI_STOP_ERROR; d.ctr[W_DONE] = 1; d.ctr[W_NPOP] = 0;
	} else if (win < cut_b) {                                            // the first meeting among the pops that run
		d.ctr[W_WON] = 1;
		d.ctr[W_WPARENT] = head + win / 12;
		d.ctr[W_WACT] = win % 12;
		d.ctr[W_MEET] = (int32_t)(d.slot[win] & ~TENT);
		d.ctr[W_HEAD] = head + win / 12 + 1;
		d.ctr[W_POPPED] += win / 12 + 1;
		d.ctr[W_STOP] = BI_STOP_WON; d.ctr[W_DONE] = 1; d.ctr[W_NPOP] = 0;
	} else if (lo < P) {                                                 // the budget refused pop `lo`
		d.ctr[W_HEAD] = head + lo;
		d.ctr[W_POPPED] += lo;
		d.ctr[W_STOP] = BI_STOP_BUDGET; d.ctr[W_DONE] = 1; d.ctr[W_NPOP] = 0;
	} else {
		d.ctr[W_HEAD] = head + P;
		d.ctr[W_POPPED] += P;
		bibfs_next(d);
	}
}

// After a growth: every stored state of both sides back into the larger, cleared table (no slot is tentative between iterations).
__global__ __launch_bounds__(256)
void k_bibfs_rehash(BiDev d)
{
	rehash_pool(d.states, d.table, d.mask, d.ctr[W_SIZE], 1 + blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// steps from `node` to the root `root` of its side along the parents, or -1 for a broken chain
__device__ __forceinline__ int bibfs_chain(const BiDev &d, int node, int root)
{
	int len = 0;
	for (int i = node; i != root; len++) {
		if (i < 1 || (uint32_t)i >= d.cap1 || len > (int)d.cap1) return -1;
		i = d.parent[i];
	}
	return len;
}

// The action queue of a won search.  The meeting joins node s of side S and node g of side G by one move `mid` (S to G):
// growing S, s is the popped parent, mid its action and g the node found; growing G, g is the popped parent, whose action led
// AWAY from solved, so mid is its inverse, and s the node found.  The queue is path(start -> s), mid, then the inverse of every
// action on the way from g back to node 2 (side G's actions were applied moving away from solved).  out[0] = length or -1.
__global__ void k_bibfs_walk(BiDev d, int32_t *out, int max_len)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (!d.ctr[W_WON]) { out[0] = -1; return; }
	const bool grew_s = d.ctr[W_SIDE] == 0;
	const int s = grew_s ? d.ctr[W_WPARENT] : d.ctr[W_MEET];
	const int g = grew_s ? d.ctr[W_MEET] : d.ctr[W_WPARENT];
	const int mid = grew_s ? d.ctr[W_WACT] : d.ctr[W_WACT] ^ 1;          // cube.rev_action: the two turns of a face are a, a ^ 1
	const int ls = bibfs_chain(d, s, 1), lg = bibfs_chain(d, g, 2);
	if (ls < 0 || lg < 0) { out[0] = -1; return; }
	out[0] = ls + 1 + lg;
	int i = s;
	for (int k = ls - 1; k >= 0; k--) {
		if (k < max_len) out[1 + k] = d.pact[i] & 15;
		i = d.parent[i];
	}
	if (ls < max_len) out[1 + ls] = mid;
	i = g;
	for (int k = ls + 1; k <= ls + lg; k++) {
		if (k < max_len) out[1 + k] = (d.pact[i] & 15) ^ 1;
		i = d.parent[i];
	}
}

}  // namespace rk

using namespace rk;

struct rk_bibfs {
	BiDev d{};
	size_t cap = 0;
	uint32_t *root_dev = nullptr;
	int32_t *walk = nullptr;
	Landing ctr_host;                           // page-locked landing place of the counter block
	bool ready = false;
	DevPool pool{64};
};

namespace {

constexpr int BI_WALK_MAX = 1 << 12;
constexpr size_t BI_MAX_CAPACITY = 0x3FFFFFF0ull;

uint32_t bibfs_table_mask(size_t capacity) { return (uint32_t)(table_slots(capacity, 1024) - 1); }

int bibfs_read_ctr(rk_bibfs *h, int32_t *out, hipStream_t st) { return h->ctr_host.read(h->d.ctr, W_COUNT, out, st); }

}  // namespace

extern "C" {

int rk_bibfs_create(rk_bibfs_t **out, size_t capacity, int pops)
{
	if (!out) return fail(RK_EINVAL, "rk_bibfs_create: null out pointer");
	if (capacity < 2 || capacity > BI_MAX_CAPACITY) return fail(RK_EINVAL, "rk_bibfs_create: capacity %zu out of range", capacity);
	if (pops < 1 || pops > (1 << 22)) return fail(RK_EINVAL, "rk_bibfs_create: pops %d outside 1..%d", pops, 1 << 22);
	rk_bibfs *h = new rk_bibfs();
	h->cap = capacity;
	BiDev &d = h->d;
	d.pops = pops;
	d.cap1 = (uint32_t)(capacity + 1);
	d.mask = bibfs_table_mask(capacity);
	const size_t C1 = capacity + 1, K = (size_t)12 * pops;
	int e = RK_OK;
	#define A(ptr, cnt) if (!e) e = h->pool.alloc(&d.ptr, (cnt))
	A(states, C1 * 5); A(parent, C1); A(pact, C1); A(table, (size_t)d.mask + 1); A(ctr, W_COUNT);
	A(slot, K); A(rank, K); A(first, K); A(chain, frontier_scan_blocks(pops));
	#undef A
	if (!e) e = h->pool.alloc(&h->root_dev, 8);
	if (!e) e = h->pool.alloc(&h->walk, BI_WALK_MAX + 8);
	if (!e) h->ctr_host.reserve(W_COUNT);
	if (e) { rk_bibfs_destroy(h); return e; }
	*out = h;
	return RK_OK;
}

int rk_bibfs_destroy(rk_bibfs_t *h)
{
	delete h;                                   // the pool and the landing buffer go with it
	return RK_OK;
}

int rk_bibfs_reset(rk_bibfs_t *h, const int8_t *h_start_state, long long max_states, void *stream)
{
	if (!h || !h_start_state) return fail(RK_EINVAL, "rk_bibfs_reset: null argument");
	if (memcmp(h_start_state, SOLVED_DW, STATE_BYTES) == 0)
		return fail(RK_EINVAL, "rk_bibfs_reset: the start state is solved (nodes 1 and 2 would hold the same state)");
	hipStream_t st = (hipStream_t)stream;
	BiDev &d = h->d;
	RK_HIP(hipMemsetAsync(d.table, 0, ((size_t)d.mask + 1) * sizeof(uint32_t), st));
	RK_HIP(hipMemsetAsync(d.chain, 0, frontier_scan_blocks(d.pops) * sizeof(unsigned long long), st));      // look-back epochs restart
	RK_HIP(hipMemcpyAsync(h->root_dev, h_start_state, STATE_BYTES, hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(k_bibfs_root, dim3(1), dim3(64), 0, st, d, h->root_dev, budget_of(max_states));
	RK_HIP(hipGetLastError());
	RK_HIP(hipStreamSynchronize(st));       // the host buffer may go away after return
	h->ready = true;
	return RK_OK;
}

int rk_bibfs_run(rk_bibfs_t *h, int iterations, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bibfs_run: reset the engine first");
	if (iterations < 0) return fail(RK_EINVAL, "rk_bibfs_run: iterations %d < 0", iterations);
	hipStream_t st = (hipStream_t)stream;
	const BiDev &d = h->d;
	const unsigned grid = blocks((size_t)12 * d.pops);
	for (int it = 0; it < iterations; it++) {
		hipLaunchKernelGGL(k_bibfs_expand, dim3(grid), dim3(256), 0, st, d);
		hipLaunchKernelGGL(k_bibfs_scan, dim3(blocks((size_t)12 * d.pops, ASCAN)), dim3(ASCAN), 0, st, d);
		hipLaunchKernelGGL(k_bibfs_append, dim3(grid), dim3(256), 0, st, d);
		hipLaunchKernelGGL(k_bibfs_end, dim3(1), dim3(64), 0, st, d);
	}
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_bibfs_status(rk_bibfs_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_bibfs_status: bad argument");
	int32_t c[W_COUNT];
	if (int e = bibfs_read_ctr(h, c, (hipStream_t)stream)) return e;
	h_status[0] = c[W_DONE]; h_status[1] = c[W_WON]; h_status[2] = c[W_SIZE]; h_status[3] = c[W_ITERS];
	h_status[4] = c[W_POPPED]; h_status[5] = c[W_STOP]; h_status[6] = c[W_ERROR]; h_status[7] = c[W_NPOP];
	h_status[8] = c[W_DEPTH]; h_status[9] = c[W_DEPTH + 1]; h_status[10] = c[W_MEET]; h_status[11] = c[W_SIDE];
	return RK_OK;
}

int rk_bibfs_grow(rk_bibfs_t *h, size_t new_capacity, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bibfs_grow: reset the engine first");
	if (new_capacity <= h->cap) return new_capacity == h->cap ? RK_OK : fail(RK_EINVAL, "rk_bibfs_grow: %zu is below the current capacity %zu", new_capacity, h->cap);
	if (new_capacity > BI_MAX_CAPACITY) return fail(RK_EINVAL, "rk_bibfs_grow: capacity %zu out of range", new_capacity);
	hipStream_t st = (hipStream_t)stream;
	const BiDev old = h->d;
	BiDev d = old;
	const size_t C1 = new_capacity + 1, C1_old = h->cap + 1;
	d.cap1 = (uint32_t)C1;
	d.mask = bibfs_table_mask(new_capacity);
	Growth g(h->pool, "rk_bibfs_grow");
	g.request(&d.states, C1 * 5); g.request(&d.parent, C1); g.request(&d.pact, C1); g.request(&d.table, (size_t)d.mask + 1);
	if (!g.granted()) return fail(RK_ECAPACITY, "rk_bibfs_grow: no device memory for a pool of %zu states", new_capacity);
	const int e = g.fill(st, [&]() -> hipError_t {
		RK_FILL(hipMemcpyAsync(d.states, old.states, C1_old * STATE_BYTES, hipMemcpyDeviceToDevice, st));
		RK_FILL(hipMemcpyAsync(d.parent, old.parent, C1_old * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
		RK_FILL(hipMemcpyAsync(d.pact, old.pact, C1_old, hipMemcpyDeviceToDevice, st));
		RK_FILL(hipMemsetAsync(d.table, 0, ((size_t)d.mask + 1) * sizeof(uint32_t), st));
		hipLaunchKernelGGL(k_bibfs_rehash, dim3(std::min<unsigned>(blocks(C1_old), 4096u)), dim3(256), 0, st, d);
		return hipGetLastError();
	});
	if (e) return e;
	g.commit();
	h->d = d;
	h->cap = new_capacity;
	return RK_OK;
}

long long rk_bibfs_size(const rk_bibfs_t *hc)
{
	rk_bibfs_t *h = const_cast<rk_bibfs_t *>(hc);
	if (!h || !h->ready) return 0;
	int32_t c[W_COUNT];
	if (bibfs_read_ctr(h, c, nullptr)) return RK_EHIP;
	return c[W_SIZE];
}

int rk_bibfs_export(rk_bibfs_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions,
                    long long *h_sides, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bibfs_export: reset the engine first");
	if (first + count > h->cap + 1) return fail(RK_EINVAL, "rk_bibfs_export: rows %zu..%zu outside the pool", first, first + count);
	if (count == 0) return RK_OK;
	hipStream_t st = (hipStream_t)stream;
	const BiDev &d = h->d;
	Widened<int32_t, long long> p;
	std::vector<uint8_t> pa;
	if (h_states) RK_HIP(hipMemcpyAsync(h_states, d.states + first * 5, count * STATE_BYTES, hipMemcpyDeviceToHost, st));
	if (int e = p.start(d.parent + first, count, h_parents, st)) return e;
	if (h_actions || h_sides) {
		pa.resize(count);
		RK_HIP(hipMemcpyAsync(pa.data(), d.pact + first, count, hipMemcpyDeviceToHost, st));
	}
	RK_HIP(hipStreamSynchronize(st));
	p.finish();
	for (size_t i = 0; i < pa.size(); i++) {
		if (h_actions) h_actions[i] = pa[i] & 15;
		if (h_sides) h_sides[i] = pa[i] >> SIDE_SHIFT;
	}
	return RK_OK;
}

long long rk_bibfs_path(rk_bibfs_t *h, long long *h_actions, size_t max_len, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_bibfs_path: reset the engine first");
	if (!h_actions && max_len > 0) return fail(RK_EINVAL, "rk_bibfs_path: null h_actions with max_len %zu", max_len);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_bibfs_walk, dim3(1), dim3(64), 0, st, h->d, h->walk, BI_WALK_MAX);
	RK_HIP(hipGetLastError());
	int32_t len = 0;
	if (int e = read_walk(h->walk, BI_WALK_MAX, h_actions, max_len, st, &len)) return e;
	if (len < 0) return fail(RK_ESTATE, "rk_bibfs_path: the search has not met (or a parent chain is broken)");
	return (long long)len;
}

}  // extern "C"
