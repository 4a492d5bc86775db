// The level-by-level build: what the two kept balls -- rk_ball.hip's goal ball and rk_sym.hip's ball of orbit representatives --
// share on the device.  Node 1 is the solved state, the pool is in index order; a level's nodes are popped in index order, never
// across a level boundary, their children taken in action order 0..11; a child the pool holds (an earlier child of the batch
// included) is skipped, every other is appended.  Level `radius` is stored and never expanded; level l is the index range
// lstart[l] .. lstart[l + 1] - 1, so a node's depth follows from its index.  An iteration is expand (membership / election),
// scan, append, end, none of which synchronises with the host.  There is no goal test, budget or cut (none of the frontier
// pool's words for them, rk_frontier_dev.h): every claim of a batch is appended, so between iterations -- and once the build is
// over -- no table slot is tentative.  A ball keeps what makes it different: the check of a closed level, where the state of
// batch position c comes from, and what it stores per node beside the state.  The host side is KeptBall (rk_frontier_host.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include "rk_device.h"
#include "rk_search_dev.h"

namespace rk {

constexpr int BALL_CHECKED = 8;                     // the last level whose size is known
// states at distance 0 .. 8 from solved in the quarter-turn metric
constexpr int32_t BALL_LEVELS[BALL_CHECKED + 1] = {1, 12, 114, 1068, 10011, 93840, 878880, 8221632, 76843595};
static __constant__ int32_t D_BALL_LEVELS[BALL_CHECKED + 1] = {1, 12, 114, 1068, 10011, 93840, 878880, 8221632, 76843595};

enum {
	BB_SIZE = 0, BB_HEAD, BB_DONE, BB_STOP, BB_ITERS, BB_ERROR, BB_NPOP, BB_TOTAL, BB_EPOCH, BB_TICKET, BB_LEVEL, BB_HI,
	BB_LSTART /* [radius + 2] */, BB_COUNT = 32
};
enum { BB_STOP_NO = 0, BB_STOP_BUILT = 1, BB_STOP_ERROR = 4, BB_STOP_FULL = 5 };    // FULL: the symmetry ball only, its capacity is the caller's
enum { BB_ERR_NONE = 0, BB_ERR_CAPACITY = 1, BB_ERR_LEVEL = 2 };

struct BuildDev {
	uint32_t mask, cap1;                        // table slots - 1, capacity + 1
	int pops, radius;
	uint32_t *states; uint32_t *table;
	int32_t *ctr;
	uint32_t *slot; int32_t *rank; uint8_t *first;                   // per child of the batch (freed after the build)
	unsigned long long *chain;
};

// the depth of node idx from the level boundaries a view holds (INT32_MAX beyond radius + 1)
template <int N>
__device__ __forceinline__ int level_of(const int32_t (&lstart)[N], uint32_t idx)
{
	int depth = 0;
	#pragma unroll
	for (int l = 1; l <= N - 2; l++) depth += (int32_t)idx >= lstart[l] ? 1 : 0;
	return depth;
}

// After the pops of an iteration (or the root): the end of a level with the ball's check level_ok(level, nodes of the level),
// the end of the build, the next P.  FIT: P is cut to the pops whose children fit the pool whatever they are, and the build
// stops with BB_STOP_FULL BEFORE an iteration of which not one pop fits.  One thread.
template <bool FIT, typename Check>
__device__ __forceinline__ void bb_next(const BuildDev &d, Check &&level_ok)
{
	const int32_t size = d.ctr[BB_SIZE], head = d.ctr[BB_HEAD];
	int level = d.ctr[BB_LEVEL];
	int32_t hi = d.ctr[BB_HI];
	int stop = BB_STOP_NO;
	if (head > hi) {                                                     // every node of `level` was popped: level + 1 is complete
		level += 1;
		if (!level_ok(level, size - hi)) { d.ctr[BB_ERROR] = BB_ERR_LEVEL; stop = BB_STOP_ERROR; }
		d.ctr[BB_LSTART + level + 1] = size + 1;
		d.ctr[BB_LEVEL] = level;
		d.ctr[BB_HI] = hi = size;
	}
	if (!stop && level >= d.radius) stop = BB_STOP_BUILT;                // level `radius` is stored and never expanded
	int P = stop ? 0 : min(d.pops, hi - head + 1);
	if constexpr (FIT) {
		if (!stop) {
			const uint32_t fit = (d.cap1 - 1u - (uint32_t)size) / 12u;
			P = min(P, (int)min(fit, (uint32_t)INT32_MAX));
			if (P < 1) { d.ctr[BB_ERROR] = BB_ERR_CAPACITY; stop = BB_STOP_FULL; P = 0; }
		}
	}
	d.ctr[BB_STOP] = stop;
	d.ctr[BB_DONE] = stop ? 1 : 0;
	d.ctr[BB_NPOP] = P;
}

// counters zeroed, node 1 = the solved state with its table slot, levels 0 and 1 opened, then next().  extra(tid): the ball's
// own words, every thread, before the barrier.
template <typename Extra, typename Next>
__device__ __forceinline__ void bb_root(const BuildDev &d, Extra &&extra, Next &&next)
{
	const int tid = threadIdx.x;
	if (tid < BB_COUNT) d.ctr[tid] = 0;
	extra(tid);
	__syncthreads();
	if (tid != 0) return;
	uint32_t s[5];
	#pragma unroll
	for (int j = 0; j < 5; j++) { s[j] = SOLVED_DW[j]; d.states[5 + j] = s[j]; }
	d.table[hash_state(s) & d.mask] = 1u;
	d.ctr[BB_SIZE] = 1; d.ctr[BB_HEAD] = 1; d.ctr[BB_HI] = 1;
	d.ctr[BB_LSTART] = 1; d.ctr[BB_LSTART + 1] = 2;
	next();
}

// membership / election, one thread per child; state_of(c, out) is the state of batch position c -- the thread's own and the
// election's `other`
template <typename StateOf>
__device__ __forceinline__ void bb_expand(const BuildDev &d, StateOf &&state_of)
{
	const int P = d.ctr[BB_NPOP];
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P) return;
	uint32_t s[5];
	state_of(c, s);
	uint32_t slot = 0;
	const uint32_t e = probe_elect(d.table, d.mask, d.states, s, c, state_of, &slot);
	d.slot[c] = e == 0u ? slot : NO_SLOT;
}

__device__ __forceinline__ void bb_scan(const BuildDev &d)
{
	const int P = d.ctr[BB_NPOP];
	if (P == 0) return;                                                  // done: no ticket drawn, nothing to reset
	frontier_scan(d.slot, d.table, d.rank, d.first, d.chain, &d.ctr[BB_TICKET], (uint32_t)d.ctr[BB_EPOCH] + 1u, &d.ctr[BB_TOTAL], 12 * P);
}

// Child c, a first occurrence, becomes node size + 1 + rank[c]; its claim becomes that index.  store(idx, s) gives the state and
// writes what the ball keeps per node beside it.  False (and the error word) for an index outside the pool: an engine error.
template <typename Store>
__device__ __forceinline__ bool bb_append(const BuildDev &d, int c, Store &&store)
{
	const uint32_t idx = (uint32_t)d.ctr[BB_SIZE] + 1u + (uint32_t)d.rank[c];
	if (idx >= d.cap1) { d.ctr[BB_ERROR] = BB_ERR_CAPACITY; return false; }
	uint32_t s[5];
	store(idx, s);
	#pragma unroll
	for (int j = 0; j < 5; j++) d.states[(size_t)idx * 5 + j] = s[j];
	d.table[d.slot[c]] = idx;
	return true;
}

template <typename Next>
__device__ __forceinline__ void bb_end(const BuildDev &d, Next &&next)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const int P = d.ctr[BB_NPOP];
	if (P == 0) return;
	d.ctr[BB_ITERS] += 1;
	d.ctr[BB_TICKET] = 0;
	d.ctr[BB_EPOCH] += 1;
	if (d.ctr[BB_ERROR]) {
		d.ctr[BB_STOP] = BB_STOP_ERROR; d.ctr[BB_DONE] = 1; d.ctr[BB_NPOP] = 0;
		return;
	}
	d.ctr[BB_SIZE] += d.ctr[BB_TOTAL];
	d.ctr[BB_HEAD] += P;
	next();
}

}  // namespace rk
