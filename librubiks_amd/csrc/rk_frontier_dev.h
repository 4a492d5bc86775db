// The frontier pool: what every breadth-first engine that keeps its whole search in HBM shares on the device -- rk_bfs.hip,
// rk_bibfs.hip, rk_ball.hip's search from a start (rk_bsearch_*) and its batch (rk_bsearchb_*), and rk_sym.hip's search that ends
// at the symmetry-reduced ball (rk_ssearch_*) and its batch (rk_ssearchb_*).  One descriptor, the common counter words, and the
// launches of an iteration that do not look at what the engine searches for: the scan, the append, the end of an iteration with
// the cut, and the rehash after a growth -- bodies (fr_*, srch_*) and, at the end of this file, the kernels around them (k_fr_scan,
// k_fr_append, k_fr_rehash, k_srch_end, kb_srch_*).  An engine keeps what makes it different: its counter words behind F_COMMON,
// its `next` (what follows a pop count change: the end of a level, the done flags, the next P), its root, its expand launch -- the
// membership rule -- and its walk.
// The host side is FrontierPool (rk_frontier_host.h), and FrontierSlots for the two batches.
//
// An iteration pops the P = F_NPOP nodes head .. head + P - 1 and is expand, scan, append, end; none synchronises with the host.
// Pop j of the batch runs only if size_before + (new states of the pops before j) < budget, and the winning child is the lowest
// batch position the expand launch entered in F_WINPOS among the pops that run.  The cut is min(12 x the first refused pop, the
// winning position); no child at or after it is appended or counted.  Claims at or after the cut stay in the table only when the
// search has ended.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rk_device.h"
#include "rk_search_dev.h"

namespace rk {

// the counter words every engine has; an engine's own words start at F_COMMON
enum {
	F_SIZE = 0, F_HEAD, F_DONE, F_WON, F_WPARENT, F_WACT, F_STOP, F_ITERS, F_ERROR, F_NPOP, F_BUDGET, F_WINPOS, F_TOTAL, F_EPOCH,
	F_TICKET, F_COMMON
};
enum { F_STOP_NO = 0, F_STOP_WON = 1, F_STOP_BUDGET = 2, F_STOP_EMPTY = 3, F_STOP_ERROR = 4 };
enum { F_ERR_NONE = 0, F_ERR_CAPACITY = 1 };
enum { F_UNRECORDED = -1 };                     // fr_end: the engine has no such counter word

constexpr uint32_t F_NO_WIN = 0x7FFFFFFFu;
constexpr uint32_t PACT_TAG_SHIFT = 4;          // pact = action | tag << 4 (the tag is rk_bibfs.hip's side; 0 everywhere else)
constexpr uint32_t PACT_ACTION = 15u;

struct FrontierDev {
	uint32_t mask, cap1;                        // table slots - 1, capacity + 1
	int pops;                                   // the most nodes an iteration pops (grid size)
	uint32_t *states; int32_t *parent; uint8_t *pact; uint32_t *table;
	int32_t *ctr;
	uint32_t *slot; int32_t *rank; uint8_t *first;                   // per child of the batch: claimed slot (or TENT | meeting node), exclusive prefix, first occurrence
	unsigned long long *chain;                                        // look-back words {epoch, total} of the scan
};

// The pops of this iteration, or 0 when it is done -- or when its children might not fit the pool: the host grows the pool
// before such an iteration, so that never cuts one; should it happen every kernel skips the iteration and fr_end reports
// an error.  Every kernel of the iteration reads the same counters, so they agree.
__device__ __forceinline__ int fr_pops(const FrontierDev &d)
{
	const int P = d.ctr[F_NPOP];
	return (uint64_t)d.ctr[F_SIZE] + 12ull * (uint64_t)P <= (uint64_t)d.cap1 - 1u ? P : 0;
}

// first-occurrence flags and their exclusive prefix in batch order (tickets + look-back: rk_search_dev.h)
__device__ __forceinline__ void fr_scan(const FrontierDev &d)
{
	const int P = fr_pops(d);
	if (P == 0) return;                                                  // done: no ticket drawn, nothing to reset
	frontier_scan(d.slot, d.table, d.rank, d.first, d.chain, &d.ctr[F_TICKET], (uint32_t)d.ctr[F_EPOCH] + 1u, &d.ctr[F_TOTAL], 12 * P);
}

// The cut and the append: child c is stored iff it is a first occurrence, lies before the winning position and its pop runs --
// size_before + (new states of the earlier pops) < budget.  That prefix only grows along the batch, so this is exactly "c is
// before the cut".  New states get the indices size + 1 ... in batch order with their parent and action; their tentative claims
// become those indices.  tag() is read for a child that is stored: what goes into pact above the action.
template <typename Tag>
__device__ __forceinline__ void fr_append(const FrontierDev &d, Tag &&tag)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = fr_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P || !d.first[c]) return;
	if ((uint32_t)c >= (uint32_t)d.ctr[F_WINPOS]) return;
	const int i = c / 12, a = c - 12 * i;
	const int32_t size0 = d.ctr[F_SIZE];
	if ((long long)size0 + d.rank[12 * i] >= (long long)d.ctr[F_BUDGET]) return;
	const uint32_t idx = (uint32_t)size0 + 1u + (uint32_t)d.rank[c];
	if (idx >= d.cap1) { d.ctr[F_ERROR] = F_ERR_CAPACITY; return; }
	const int32_t p = d.ctr[F_HEAD] + i;
	uint32_t s[5];
	child_state(d.states, p, s_act, (uint32_t)a, s);
	#pragma unroll
	for (int j = 0; j < 5; j++) d.states[(size_t)idx * 5 + j] = s[j];
	d.parent[idx] = p;
	d.pact[idx] = (uint8_t)((uint32_t)a | (tag() << PACT_TAG_SHIFT));
	d.table[d.slot[c]] = idx;
}
__device__ __forceinline__ void fr_append(const FrontierDev &d) { fr_append(d, [] { return 0u; }); }

// Where the cut fell, the new size / head, the win, then next(d): the done flags and the next P; resets the per-iteration
// counters.  One thread, ordinary stores.  MEET and POPPED are the engine's counter words for the node a winning child met
// (slot[win] without the TENT bit) and the nodes popped so far, or F_UNRECORDED for an engine without them.
template <int MEET, int POPPED, typename Next>
__device__ __forceinline__ void fr_end(const FrontierDev &d, Next &&next)
{
	if (d.ctr[F_NPOP] == 0) return;
	const int P = fr_pops(d);
	if (P == 0) {
		d.ctr[F_ERROR] = F_ERR_CAPACITY;
		d.ctr[F_STOP] = F_STOP_ERROR; d.ctr[F_DONE] = 1; d.ctr[F_NPOP] = 0;
		return;
	}
	const int32_t size0 = d.ctr[F_SIZE], head = d.ctr[F_HEAD];
	const int lo = first_refused_pop(d.rank, P, size0, d.ctr[F_BUDGET]); // the first pop that fails the budget check (P: none)
	const int cut_b = 12 * lo;
	const int win = d.ctr[F_WINPOS];
	const int cut = min(cut_b, win);
	const int n_new = cut < 12 * P ? d.rank[cut] : d.ctr[F_TOTAL];
	d.ctr[F_SIZE] = size0 + n_new;
	d.ctr[F_ITERS] += 1;
	d.ctr[F_TICKET] = 0;
	d.ctr[F_EPOCH] += 1;
	d.ctr[F_WINPOS] = (int32_t)F_NO_WIN;
	if (d.ctr[F_ERROR]) {
		d.ctr[F_STOP] = F_STOP_ERROR; d.ctr[F_DONE] = 1; d.ctr[F_NPOP] = 0;
	} else if (win < cut_b) {                                            // the first win among the pops that run
		d.ctr[F_WON] = 1;
		d.ctr[F_WPARENT] = head + win / 12;
		d.ctr[F_WACT] = win % 12;
		if constexpr (MEET != F_UNRECORDED) d.ctr[MEET] = (int32_t)(d.slot[win] & ~TENT);
		d.ctr[F_HEAD] = head + win / 12 + 1;
		if constexpr (POPPED != F_UNRECORDED) d.ctr[POPPED] += win / 12 + 1;
		d.ctr[F_STOP] = F_STOP_WON; d.ctr[F_DONE] = 1; d.ctr[F_NPOP] = 0;
	} else if (lo < P) {                                                 // the budget refused pop `lo`
		d.ctr[F_HEAD] = head + lo;
		if constexpr (POPPED != F_UNRECORDED) d.ctr[POPPED] += lo;
		d.ctr[F_STOP] = F_STOP_BUDGET; d.ctr[F_DONE] = 1; d.ctr[F_NPOP] = 0;
	} else {
		d.ctr[F_HEAD] = head + P;
		if constexpr (POPPED != F_UNRECORDED) d.ctr[POPPED] += P;
		next(d);
	}
}

// after a growth: every stored state back into the larger, cleared table (grid-stride).  Between iterations of a running search
// no slot is tentative, so this is a plain insert of indices 1..size.
__device__ __forceinline__ void fr_rehash(const FrontierDev &d)
{
	rehash_pool(d.states, d.table, d.mask, d.ctr[F_SIZE], 1 + blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// ---- the searches that end at a kept ball (rk_bsearch_*, rk_bsearchb_*, rk_ssearch_*): one side, level by level ----
enum { S_DEPTH = F_COMMON, S_HI, S_MEET, S_POPPED, S_LO, S_CLIP, S_COUNT = 32 };      // S_LO .. S_HI: the newest complete level

// After a pop count change: the end of a level, the done flags and the next P (rk_bibfs.hip: bibfs_next, one side).  One thread.
__device__ __forceinline__ void srch_next(const FrontierDev &d)
{
	const int32_t size = d.ctr[F_SIZE], head = d.ctr[F_HEAD];
	int32_t hi = d.ctr[S_HI];
	if (head > hi) {                                                     // the level is exhausted and nothing met: it is complete
		d.ctr[S_DEPTH] += 1;
		d.ctr[S_LO] = hi + 1;
		d.ctr[S_HI] = hi = size;
	}
	int stop = F_STOP_NO;
	if (head > hi) stop = F_STOP_EMPTY;                                  // a level without a state: the whole graph was seen
	else if (size >= d.ctr[F_BUDGET]) stop = F_STOP_BUDGET;             // checked before the next pop
	d.ctr[F_STOP] = stop;
	d.ctr[F_DONE] = stop ? 1 : 0;
	d.ctr[F_NPOP] = stop ? 0 : min(d.pops, hi - head + 1);
}

__device__ __forceinline__ void srch_end(const FrontierDev &d) { fr_end<S_MEET, S_POPPED>(d, [](const FrontierDev &x) { srch_next(x); }); }

// What a root launch stores once it knows e, the ball's node of the start (0: the ball does not hold it): node 1 = the start s,
// the counters, and either the win without a pop -- the ball's path from e is the answer -- or the first pop count.  One thread,
// after the counter block was zeroed.  S_LO is set for both balls: only rk_sdeepen_frontier and rk_sdeepenb_frontiers export it, no plain-ball entry does.
__device__ __forceinline__ void srch_root_store(const FrontierDev &d, const uint32_t s[5], int budget, uint32_t e)
{
	#pragma unroll
	for (int j = 0; j < 5; j++) d.states[5 + j] = s[j];
	d.parent[1] = 0; d.pact[1] = 0;
	d.table[hash_state(s) & d.mask] = 1u;
	d.ctr[F_SIZE] = 1; d.ctr[F_HEAD] = 1; d.ctr[S_HI] = 1; d.ctr[S_LO] = 1;
	d.ctr[F_BUDGET] = budget;
	d.ctr[F_WINPOS] = (int32_t)F_NO_WIN;
	if (e != 0u) {
		d.ctr[F_WON] = 1; d.ctr[S_MEET] = (int32_t)e;
		d.ctr[F_STOP] = F_STOP_WON; d.ctr[F_DONE] = 1;
		return;
	}
	srch_next(d);
}

// child c of the batch is node m of the ball: the meeting.  The lowest batch position wins; no claim in the own table.
__device__ __forceinline__ void srch_meet(const FrontierDev &d, int c, uint32_t m)
{
	atomicMin(reinterpret_cast<uint32_t *>(&d.ctr[F_WINPOS]), (uint32_t)c);
	d.slot[c] = TENT | m;                                                // no claim (TENT bit); fr_end reads the meeting node here
}

// child c, state s, is not in the ball: membership / election in the own table (the other children recomputed from their parents)
__device__ __forceinline__ void srch_claim(const FrontierDev &d, const u32x4 *s_act, int32_t head, int c, const uint32_t s[5])
{
	uint32_t slot = 0;
	const uint32_t e = probe_elect(d.table, d.mask, d.states, s, c,
	                               [&](int c2, uint32_t o[5]) { child_state(d.states, head + c2 / 12, s_act, (uint32_t)(c2 % 12), o); }, &slot);
	d.slot[c] = e == 0u ? slot : NO_SLOT;
}

// ---- such searches in lock-step (rk_bsearchb_*, rk_ssearchb_*): a slot's pool never grows ----
// A slot whose next iteration might not fit (size + 12 P > capacity) stops BEFORE that iteration with BS_STOP_FULL, so fr_pops()
// of a slot with P > 0 is P and the single engine's F_ERR_CAPACITY path is never taken.
// A slot whose root set S_CLIP (rk_sdeepenb_set; 0 in every other pool) is not stopped by a batch that might not fit: it
// pops as many nodes as surely fit, min(P, (capacity - size) / 12), and stops only when not even one does.  A pop that runs this
// way also runs at pops = 1, where it is asked for alone with at most as many states stored; the pool's order does not depend on
// the pops, a level is never crossed (srch_next), and the stop is pops = 1's: size + 12 > capacity.  So the pool, the nodes
// popped, the complete levels and the partial next level are those of pops = 1, whatever d.pops is.  Only F_NPOP is lowered:
// d.pops, the grids and the stride of a slot's scratch stay.
enum { BS_STOP_FULL = 5 };

// after the root or the end of an iteration of a slot: does the next iteration fit the pool whatever it finds?  One thread.
__device__ __forceinline__ void srch_fit(const FrontierDev &d)
{
	const int P = d.ctr[F_NPOP];
	if (P == 0 || (uint64_t)d.ctr[F_SIZE] + 12ull * (uint64_t)P <= (uint64_t)d.cap1 - 1u) return;
	if (d.ctr[S_CLIP]) {
		const uint32_t fit = (d.cap1 - 1u - (uint32_t)d.ctr[F_SIZE]) / 12u;  // (size <= capacity: the appends are bounded by it)
		if (fit >= 1u) { d.ctr[F_NPOP] = (int32_t)fit; return; }            // (fit < P: P did not fit)
	}
	d.ctr[F_STOP] = BS_STOP_FULL; d.ctr[F_DONE] = 1; d.ctr[F_NPOP] = 0;
}

// the table and the look-back words of one slot, zeroed by the workgroups (blockIdx.x, gridDim.x) of 256: 16 bytes per thread and
// step (a table is a power of two >= 1024 dwords, every slice 16-byte aligned)
__device__ __forceinline__ void srch_clear(const FrontierDev &d, int chain_words)
{
	u32x4 *t4 = reinterpret_cast<u32x4 *>(d.table);
	const size_t n4 = ((size_t)d.mask + 1) / 4;
	const u32x4 zero = {0u, 0u, 0u, 0u};
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) t4[i] = zero;
	if (blockIdx.x == 0)
		for (int i = threadIdx.x; i < chain_words; i += 256) d.chain[i] = 0ull;
}

constexpr int FRONTIER_WALK_MAX = 1 << 12;

// The climb from `node` to node 1 along the parents: the steps, or -1 for a broken chain (an index outside the pool, a cycle).
// The actions go root-first to out[0 .. min(steps, max_len) - 1] where `write` holds (one lane of a wave that walks together);
// the tag above the action is masked off (it is 0 in every pool but rk_bibfs.hip's).
__device__ __forceinline__ int fr_walk_up(const FrontierDev &d, int node, int32_t *out, int max_len, bool write)
{
	int steps = 0;
	for (int i = node; i != 1; steps++) {
		if (i < 1 || (uint32_t)i >= d.cap1 || steps > (int)d.cap1) return -1;
		i = d.parent[i];
	}
	for (int i = node, k = steps - 1; k >= 0; k--) {
		if (k < max_len && write) out[k] = d.pact[i] & PACT_ACTION;
		i = d.parent[i];
	}
	return steps;
}

// ---- the kernels that do not look at what an engine searches for ----
// Internal linkage: this header goes into several .hip files that are linked into one library without relocatable device code,
// so every file that launches one of these carries its own copy.
namespace {

__global__ __launch_bounds__(ASCAN)
void k_fr_scan(FrontierDev d) { fr_scan(d); }

__global__ __launch_bounds__(256)
void k_fr_append(FrontierDev d) { fr_append(d); }

__global__ __launch_bounds__(256)
void k_fr_rehash(FrontierDev d) { fr_rehash(d); }

__global__ void k_srch_end(FrontierDev d) { if (threadIdx.x == 0 && blockIdx.x == 0) srch_end(d); }

// The batch: slot blockIdx.y of `devs` per workgroup row.  A slot that is done, or was never started, has F_NPOP == 0: it leaves
// at that read, draws no ticket and leaves its epoch alone.

// the named slots' tables and look-back words, zeroed: slot slots[blockIdx.y]
__global__ __launch_bounds__(256)
void kb_srch_clear(const FrontierDev *devs, const int32_t *slots, int chain_words) { srch_clear(devs[slots[blockIdx.y]], chain_words); }

__global__ __launch_bounds__(ASCAN)
void kb_srch_scan(const FrontierDev *devs)
{
	const FrontierDev d = devs[blockIdx.y];
	if (d.ctr[F_NPOP] == 0) return;                                      // (every workgroup of a live slot draws a ticket)
	fr_scan(d);
}

__global__ __launch_bounds__(256)
void kb_srch_append(const FrontierDev *devs)
{
	const FrontierDev d = devs[blockIdx.y];
	if (blockIdx.x * 256 >= 12 * d.ctr[F_NPOP]) return;                  // done, never started, or a workgroup past the batch
	fr_append(d);
}

__global__ void kb_srch_end(const FrontierDev *devs)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const FrontierDev d = devs[blockIdx.y];
	if (d.ctr[F_NPOP] == 0) return;
	srch_end(d);
	srch_fit(d);
}

}  // namespace

}  // namespace rk
