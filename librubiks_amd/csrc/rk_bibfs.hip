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
// in the four launches of the frontier pool (rk_frontier_dev.h; the scan, the append, the end with its cut and the rehash are its
// code, this file holds the level bookkeeping bibfs_next, the root, the membership rule k_bibfs_expand and the walk):
//   k_bibfs_expand   one thread per child: the move, the look-up in the table; a stored state of the growing side is skipped, one
//                    of the other side enters its batch position for the meeting, a new state takes part in the election
//   k_fr_scan        first-occurrence flags and their exclusive prefix over the batch
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
#include "rk_frontier_dev.h"
#include "rk_frontier_host.h"

namespace rk {

enum {
	W_SIDE = F_COMMON, W_DEPTH /* [2] */, W_LO = W_DEPTH + 2 /* [2] */, W_HI = W_LO + 2 /* [2] */, W_NEWLO = W_HI + 2, W_MEET, W_POPPED,
	W_COUNT = 32
};
constexpr uint32_t SIDE_SHIFT = PACT_TAG_SHIFT;  // pact = action | side << 4 (side 0 = S, 1 = G): the side is the pool's tag

// After a pop count change (reset, end of an iteration): the end of a level, the done flags and the next P.  One thread.
__device__ __forceinline__ void bibfs_next(const FrontierDev &d)
{
	const int32_t size = d.ctr[F_SIZE];
	int side = d.ctr[W_SIDE];
	int32_t head = d.ctr[F_HEAD];
	if (head > d.ctr[W_HI + side]) {                                     // the level is exhausted and nothing met: it is complete
		d.ctr[W_DEPTH + side] += 1;
		d.ctr[W_LO + side] = d.ctr[W_NEWLO];
		d.ctr[W_HI + side] = size;
		side = d.ctr[W_DEPTH] == d.ctr[W_DEPTH + 1] ? 0 : 1;             // equal level sizes on both sides: alternate
		head = d.ctr[W_LO + side];
		d.ctr[W_SIDE] = side;
		d.ctr[F_HEAD] = head;
		d.ctr[W_NEWLO] = size + 1;
	}
	const int32_t hi = d.ctr[W_HI + side];
	int stop = F_STOP_NO;
	if (head > hi) stop = F_STOP_EMPTY;                                 // a level without a state: the whole graph was seen
	else if (size >= d.ctr[F_BUDGET]) stop = F_STOP_BUDGET;            // checked before the next pop
	const int P = stop ? 0 : min(d.pops, hi - head + 1);
	d.ctr[F_STOP] = stop;
	d.ctr[F_DONE] = stop ? 1 : 0;
	d.ctr[F_NPOP] = stop ? 0 : P;
}

__global__ void k_bibfs_root(FrontierDev d, const uint32_t *root, int budget)
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
	d.ctr[F_SIZE] = 2; d.ctr[F_HEAD] = 1;
	d.ctr[W_LO] = 1; d.ctr[W_HI] = 1; d.ctr[W_LO + 1] = 2; d.ctr[W_HI + 1] = 2;
	d.ctr[W_NEWLO] = 3;
	d.ctr[F_BUDGET] = budget;
	d.ctr[F_WINPOS] = (int32_t)F_NO_WIN;
	bibfs_next(d);
}

// fan-out + membership on either side + election among the new states: one thread per child
__global__ __launch_bounds__(256)
void k_bibfs_expand(FrontierDev d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = fr_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P) return;
	const int32_t head = d.ctr[F_HEAD];
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
	atomicMin(reinterpret_cast<uint32_t *>(&d.ctr[F_WINPOS]), (uint32_t)c);
	d.slot[c] = TENT | e;                                                // no claim (TENT bit); k_bibfs_end reads the meeting node here
}

// with the side that grows above the action
__global__ __launch_bounds__(256)
void k_bibfs_append(FrontierDev d) { fr_append(d, [&] { return (uint32_t)d.ctr[W_SIDE]; }); }

// the win is the meeting: the node of the other side that the child equals, and the nodes popped, are recorded
__global__ void k_bibfs_end(FrontierDev d)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	fr_end<W_MEET, W_POPPED>(d, [](const FrontierDev &x) { bibfs_next(x); });
}

// steps from `node` to the root `root` of its side along the parents, or -1 for a broken chain
__device__ __forceinline__ int bibfs_chain(const FrontierDev &d, int node, int root)
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
__global__ void k_bibfs_walk(FrontierDev d, int32_t *out, int max_len)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (!d.ctr[F_WON]) { out[0] = -1; return; }
	const bool grew_s = d.ctr[W_SIDE] == 0;
	const int s = grew_s ? d.ctr[F_WPARENT] : d.ctr[W_MEET];
	const int g = grew_s ? d.ctr[W_MEET] : d.ctr[F_WPARENT];
	const int mid = grew_s ? d.ctr[F_WACT] : d.ctr[F_WACT] ^ 1;          // cube.rev_action: the two turns of a face are a, a ^ 1
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

struct rk_bibfs : FrontierPool {};

extern "C" {

int rk_bibfs_create(rk_bibfs_t **out, size_t capacity, int pops)
{
	if (!out) return fail(RK_EINVAL, "rk_bibfs_create: null out pointer");
	if (int e = FrontierPool::check_create("rk_bibfs_create", capacity, pops)) return e;
	rk_bibfs *h = new rk_bibfs();
	if (int e = h->alloc(capacity, pops, W_COUNT)) { delete h; return e; }
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
	return h->reset(h_start_state, st, [&] { hipLaunchKernelGGL(k_bibfs_root, dim3(1), dim3(64), 0, st, h->d, h->root_dev, budget_of(max_states)); });
}

int rk_bibfs_run(rk_bibfs_t *h, int iterations, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bibfs_run")) return e;
	hipStream_t st = (hipStream_t)stream;
	return h->run("rk_bibfs_run", iterations, st, [&](unsigned grid) { hipLaunchKernelGGL(k_bibfs_expand, dim3(grid), dim3(256), 0, st, h->d); },
	              k_bibfs_append, k_bibfs_end);
}

int rk_bibfs_status(rk_bibfs_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_bibfs_status: bad argument");
	int32_t c[W_COUNT];
	if (int e = h->read_ctr(c, (hipStream_t)stream)) return e;
	h_status[0] = c[F_DONE]; h_status[1] = c[F_WON]; h_status[2] = c[F_SIZE]; h_status[3] = c[F_ITERS];
	h_status[4] = c[W_POPPED]; h_status[5] = c[F_STOP]; h_status[6] = c[F_ERROR]; h_status[7] = c[F_NPOP];
	h_status[8] = c[W_DEPTH]; h_status[9] = c[W_DEPTH + 1]; h_status[10] = c[W_MEET]; h_status[11] = c[W_SIDE];
	return RK_OK;
}

int rk_bibfs_grow(rk_bibfs_t *h, size_t new_capacity, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bibfs_grow")) return e;
	return h->grow("rk_bibfs_grow", new_capacity, (hipStream_t)stream);
}

long long rk_bibfs_size(const rk_bibfs_t *h) { return FrontierPool::size(h); }

int rk_bibfs_export(rk_bibfs_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions,
                    long long *h_sides, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bibfs_export")) return e;
	return h->export_rows("rk_bibfs_export", first, count, h_states, h_parents, h_actions, h_sides, (hipStream_t)stream);
}

long long rk_bibfs_path(rk_bibfs_t *h, long long *h_actions, size_t max_len, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bibfs_path")) return e;
	if (!h_actions && max_len > 0) return fail(RK_EINVAL, "rk_bibfs_path: null h_actions with max_len %zu", max_len);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_bibfs_walk, dim3(1), dim3(64), 0, st, h->d, h->walk, FRONTIER_WALK_MAX);
	RK_HIP(hipGetLastError());
	int32_t len = 0;
	if (int e = read_walk(h->walk, FRONTIER_WALK_MAX, h_actions, max_len, st, &len)) return e;
	if (len < 0) return fail(RK_ESTATE, "rk_bibfs_path: the search has not met (or a parent chain is broken)");
	return (long long)len;
}

}  // extern "C"
