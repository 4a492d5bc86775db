// What the searches that end at a kept goal ball share: rk_ball.hip's one-sided search from a start (rk_bsearch_*), its batch
// (rk_bsearchb_*) and rk_sym.hip's search that ends at the symmetry-reduced ball (rk_ssearch_*).  The counter block, the own pool's
// descriptor, the level bookkeeping, and the launches that do not look at the ball at all: the scan, the append, the end of an
// iteration and the rehash after a growth.  What differs between the engines is the membership test "the ball holds this child"
// (the root and the expand launch) and the ball's half of the path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rk_device.h"
#include "rk_search_dev.h"

namespace rk {

enum {
	S_SIZE = 0, S_HEAD, S_DONE, S_WON, S_WPARENT, S_WACT, S_STOP, S_ITERS, S_ERROR, S_NPOP, S_BUDGET, S_WINPOS, S_TOTAL, S_EPOCH,
	S_TICKET, S_DEPTH, S_HI, S_MEET, S_POPPED, S_COUNT = 32
};
enum { BS_STOP_NO = 0, BS_STOP_WON = 1, BS_STOP_BUDGET = 2, BS_STOP_EMPTY = 3, BS_STOP_ERROR = 4 };
enum { BS_ERR_NONE = 0, BS_ERR_CAPACITY = 1 };

constexpr uint32_t BS_NO_WIN = 0x7FFFFFFFu;

struct SrchDev {
	uint32_t mask, cap1;                        // table slots - 1, capacity + 1 of the OWN pool
	int pops;
	uint32_t *states; int32_t *parent; uint8_t *pact; uint32_t *table;
	int32_t *ctr;
	uint32_t *slot; int32_t *rank; uint8_t *first;                   // per child of the batch: claimed slot (or TENT | meeting node), exclusive prefix, first occurrence
	unsigned long long *chain;
};

// After a pop count change: the end of a level, the done flags and the next P (rk_bibfs.hip: bibfs_next, one side).  One thread.
__device__ __forceinline__ void srch_next(const SrchDev &d)
{
	const int32_t size = d.ctr[S_SIZE], head = d.ctr[S_HEAD];
	int32_t hi = d.ctr[S_HI];
	if (head > hi) {                                                     // the level is exhausted and nothing met: it is complete
		d.ctr[S_DEPTH] += 1;
		d.ctr[S_HI] = hi = size;
	}
	int stop = BS_STOP_NO;
	if (head > hi) stop = BS_STOP_EMPTY;                                 // a level without a state: the whole graph was seen
	else if (size >= d.ctr[S_BUDGET]) stop = BS_STOP_BUDGET;            // checked before the next pop
	d.ctr[S_STOP] = stop;
	d.ctr[S_DONE] = stop ? 1 : 0;
	d.ctr[S_NPOP] = stop ? 0 : min(d.pops, hi - head + 1);
}

// The pops of this iteration, or 0 when it is done or its children might not fit the pool (rk_bfs.hip: bfs_pops).
__device__ __forceinline__ int srch_pops(const SrchDev &d)
{
	const int P = d.ctr[S_NPOP];
	return (uint64_t)d.ctr[S_SIZE] + 12ull * (uint64_t)P <= (uint64_t)d.cap1 - 1u ? P : 0;
}

__device__ __forceinline__ void bsearch_scan(const SrchDev &d)
{
	const int P = srch_pops(d);
	if (P == 0) return;                                                  // done: no ticket drawn, nothing to reset
	frontier_scan(d.slot, d.table, d.rank, d.first, d.chain, &d.ctr[S_TICKET], (uint32_t)d.ctr[S_EPOCH] + 1u, &d.ctr[S_TOTAL], 12 * P);
}

// child c is stored iff it is a first occurrence before the cut (rk_bfs.hip: k_bfs_append)
__device__ __forceinline__ void bsearch_append(const SrchDev &d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = srch_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P || !d.first[c]) return;
	if ((uint32_t)c >= (uint32_t)d.ctr[S_WINPOS]) return;
	const int i = c / 12, a = c - 12 * i;
	const int32_t size0 = d.ctr[S_SIZE];
	if ((long long)size0 + d.rank[12 * i] >= (long long)d.ctr[S_BUDGET]) return;
	const uint32_t idx = (uint32_t)size0 + 1u + (uint32_t)d.rank[c];
	if (idx >= d.cap1) { d.ctr[S_ERROR] = BS_ERR_CAPACITY; return; }
	const int32_t p = d.ctr[S_HEAD] + i;
	uint32_t s[5];
	child_state(d.states, p, s_act, (uint32_t)a, s);
	#pragma unroll
	for (int j = 0; j < 5; j++) d.states[(size_t)idx * 5 + j] = s[j];
	d.parent[idx] = p;
	d.pact[idx] = (uint8_t)a;
	d.table[d.slot[c]] = idx;
}

// where the cut fell, the new size / head, the meeting, the end of a level, the next P.  One thread, ordinary stores.
__device__ __forceinline__ void bsearch_end(const SrchDev &d)
{
	if (d.ctr[S_NPOP] == 0) return;
	const int P = srch_pops(d);
	if (P == 0) {
		d.ctr[S_ERROR] = BS_ERR_CAPACITY;
		d.ctr[S_STOP] = BS_STOP_ERROR; d.ctr[S_DONE] = 1; d.ctr[S_NPOP] = 0;
		return;
	}
	const int32_t size0 = d.ctr[S_SIZE], head = d.ctr[S_HEAD];
	const int lo = first_refused_pop(d.rank, P, size0, d.ctr[S_BUDGET]);
	const int cut_b = 12 * lo;
	const int win = d.ctr[S_WINPOS];
	const int cut = min(cut_b, win);
	const int n_new = cut < 12 * P ? d.rank[cut] : d.ctr[S_TOTAL];
	d.ctr[S_SIZE] = size0 + n_new;
	d.ctr[S_ITERS] += 1;
	d.ctr[S_TICKET] = 0;
	d.ctr[S_EPOCH] += 1;
	d.ctr[S_WINPOS] = (int32_t)BS_NO_WIN;
	if (d.ctr[S_ERROR]) {
		d.ctr[S_STOP] = BS_STOP_ERROR; d.ctr[S_DONE] = 1; d.ctr[S_NPOP] = 0;
	} else if (win < cut_b) {                                            // the first meeting among the pops that run
		d.ctr[S_WON] = 1;
		d.ctr[S_WPARENT] = head + win / 12;
		d.ctr[S_WACT] = win % 12;
		d.ctr[S_MEET] = (int32_t)(d.slot[win] & ~TENT);
		d.ctr[S_HEAD] = head + win / 12 + 1;
		d.ctr[S_POPPED] += win / 12 + 1;
		d.ctr[S_STOP] = BS_STOP_WON; d.ctr[S_DONE] = 1; d.ctr[S_NPOP] = 0;
	} else if (lo < P) {                                                 // the budget refused pop `lo`
		d.ctr[S_HEAD] = head + lo;
		d.ctr[S_POPPED] += lo;
		d.ctr[S_STOP] = BS_STOP_BUDGET; d.ctr[S_DONE] = 1; d.ctr[S_NPOP] = 0;
	} else {
		d.ctr[S_HEAD] = head + P;
		d.ctr[S_POPPED] += P;
		srch_next(d);
	}
}

// after a growth: the stored states of the own pool back into its cleared table (grid-stride)
__device__ __forceinline__ void bsearch_rehash(const SrchDev &d)
{
	rehash_pool(d.states, d.table, d.mask, d.ctr[S_SIZE], 1 + blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

constexpr int BS_WALK_MAX = 1 << 12;
constexpr size_t BS_MAX_CAPACITY = 0x3FFFFFF0ull;

}  // namespace rk
