// The goal ball: every state within `radius` quarter turns of the solved state, built once and kept in HBM, and what reads it --
// exact distances and shortest solutions of batches of states in one launch, and a one-sided breadth-first search from a start
// that ends at the first child the ball holds.  (rk_bibfs.hip rebuilds the solved side's ball for every search; it is the same
// for every start.)
//
// The ball (rk_ball_*) is the level-by-level build of rk_ballbuild_dev.h (counters, root, next, expand, scan, append, end) over
// raw states: the state of batch position c is recomputed from its parent, and every node is stored with its parent and its
// action -- the move AWAY from solved.  There is no depth array: a node's depth follows from its index.  The capacity is exact,
// from the level sizes of the quarter-turn Cayley graph (BALL_LEVELS), and every completed level is checked against them.
//   states  int8 (C+1, 20), parent int32 (C+1), pact uint8 (C+1), table uint32 (T = pow2 >= 2C)
// The pool is never too small for a batch unless the engine is wrong; the append checks every index all the same.
// After the build the ball is read-only:
//   k_ball_depth   one thread per query: read-only probe (probe_find), 20-byte compare, depth from the level boundaries; -1 outside
//   k_ball_solve   the same, then the walk along the parents: the inverse of every stored action leads back to solved
//
// Shortening (rk_bshorten_*): one pass over a batch of action queues, the start states not needed.  The moves a[i .. j-1] of a
// queue, applied to the solved state, give X(i, j); the distance between the queue's states s_i and s_j is the ball depth d(i, j)
// of X(i, j), and the ball's word for X(i, j) leads from s_i to s_j as well (the states are a group).  So a queue is a DAG over
// 0 .. L with an edge i -> j of weight d(i, j) for every window j - i <= W that the ball holds, and its best rewrite a shortest path:
//   k_shorten_windows   a WAVE per (queue, i), the lane is the offset: the window's moves composed by scan_moves in chunks of 64
//                       with a carried state (rk_cube_kernels.hip: k_apply_sequences_scan), probe_find, d(i, j) as one byte
//   k_shorten_dp        (rk_shorten_dev.h, rk_sym.hip launches the same) a workgroup per queue: cost[j] = min cost[i] + w(i, j),
//                       the candidates of one j reduced in parallel, ties to the largest i; cost in LDS, pred to scratch
//   k_shorten_emit      a wave per queue (shorten_emit): back along pred, then forward; an edge with d < j - i is replaced by the
//                       ball's word for X(i, j) (found again by one scan and one probe), the stored actions from node 1 down to the node
// Nothing of the ball is written.
//
// The search (rk_bsearch_*) is rk_bfs.hip's protocol from the start (node 1 of a pool of its own) with rk_bibfs.hip's level
// bookkeeping and meeting: a child the own pool holds is skipped, a child the BALL holds is the meeting -- not stored, the lowest
// batch position wins --, every other is appended.  The budget is checked before every pop; the cut is min(12 x the first
// refused pop, the lowest batch position of a meeting); nothing at or after it is stored.  A start at distance D > R has no
// state of a level k < D - R in the ball, and every hit at level D - R has ball depth exactly R: the first meeting in index and
// action order is a shortest solution.  A start that the ball holds is answered by the ball's path without a pop.  The own
// table is sized to the own pool; a reset clears it and never the ball's.
//
// The batch (rk_bsearchb_*) is S such searches in lock-step.  The kernels' bodies are __device__ functions of a FrontierDev; the single
// engine's kernels pass theirs by value, the batch's pick devs[blockIdx.y] from an array in device memory, so an iteration of all
// slots is the same four launches with S in the grid's second dimension.  Every kind of array is one block sliced per slot.  A
// slot's pool is fixed: it stops with reason 5 before an iteration that might not fit.
// The kernels of this file are the root, the expand and the walk of either form (k_bsearch_*, kb_bsearch_*): what looks at the
// ball.  The scan, the append, the end, the rehash and the batch's clear do not and are rk_frontier_dev.h's (k_fr_scan,
// k_fr_append, k_srch_end, k_fr_rehash, kb_srch_*), launched by FrontierPool and FrontierSlots (rk_frontier_host.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_ballbuild_dev.h"
#include "rk_error.h"
#include "rk_frontier_dev.h"
#include "rk_frontier_host.h"
#include "rk_shorten_dev.h"

namespace rk {

constexpr int BALL_MAX_RADIUS = BALL_CHECKED;   // the capacity is exact, so every level must be a known one

struct BallDev : BuildDev {
	int32_t *parent; uint8_t *pact;             // of every node: where it came from and by which action, the move AWAY from solved
};

// What the readers of a built ball get, by value: nothing in it changes any more.
struct BallView {
	uint32_t mask, cap1;
	int radius;
	int32_t lstart[BALL_MAX_RADIUS + 2];        // level l = lstart[l] .. lstart[l + 1] - 1; INT32_MAX beyond radius + 1
	const uint32_t *states; const int32_t *parent; const uint8_t *pact; const uint32_t *table;
};

// a closed level has the size of the graph's; P is never cut: the capacity is the sum of those sizes
__device__ __forceinline__ void ball_next(const BallDev &d)
{
	bb_next<false>(d, [](int level, int32_t nodes) { return nodes == D_BALL_LEVELS[level]; });
}

__global__ void k_ball_root(BallDev d)
{
	bb_root(d, [&](int tid) { if (tid == 0) { d.parent[1] = 0; d.pact[1] = 0; } }, [&] { ball_next(d); });
}

// the state of batch position c is recomputed from its parent
__global__ __launch_bounds__(256)
void k_ball_expand(BallDev d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int32_t head = d.ctr[BB_HEAD];
	bb_expand(d, [&](int c, uint32_t o[5]) { child_state(d.states, head + c / 12, s_act, (uint32_t)(c % 12), o); });
}

__global__ __launch_bounds__(ASCAN)
void k_ball_scan(BallDev d) { bb_scan(d); }

// every first occurrence is stored with its parent and its action
__global__ __launch_bounds__(256)
void k_ball_append(BallDev d)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = d.ctr[BB_NPOP];
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P || !d.first[c]) return;
	const int i = c / 12, a = c - 12 * i;
	const int32_t p = d.ctr[BB_HEAD] + i;
	bb_append(d, c, [&](uint32_t idx, uint32_t s[5]) {
		child_state(d.states, p, s_act, (uint32_t)a, s);
		d.parent[idx] = p;
		d.pact[idx] = (uint8_t)a;
	});
}

__global__ void k_ball_end(BallDev d) { bb_end(d, [&] { ball_next(d); }); }

// exact distance to solved of query q, -1 outside the ball: one thread per query, nothing is written but the answer
__global__ __launch_bounds__(256)
void k_ball_depth(BallView b, const uint32_t *queries, size_t n, int32_t *depth)
{
	const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (q >= n) return;
	uint32_t s[5];
	load5(queries + q * 5, s);
	const uint32_t e = probe_find(b.table, b.mask, b.states, s);
	depth[q] = e ? level_of(b.lstart, e) : -1;
}

// the shortest solution of query q: from its node along the parents, the inverse of every stored action (those lead away from
// solved); row q of `actions` (n, radius) is padded with -1, lengths[q] = -1 outside the ball
__global__ __launch_bounds__(256)
void k_ball_solve(BallView b, const uint32_t *queries, size_t n, int32_t *lengths, int8_t *actions)
{
	const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (q >= n) return;
	uint32_t s[5];
	load5(queries + q * 5, s);
	uint32_t i = probe_find(b.table, b.mask, b.states, s);
	int8_t *row = actions + q * (size_t)b.radius;
	int len = 0;
	bool ok = i != 0u;
	while (ok && i != 1u) {
		if (len >= b.radius) { ok = false; break; }                      // (a chain longer than the radius: never in a ball that passed its build)
		row[len++] = (int8_t)(b.pact[i] ^ 1);                            // cube.rev_action: the two turns of a face are a, a ^ 1
		i = (uint32_t)b.parent[i];
		ok = i >= 1u && i < b.cap1;
	}
	lengths[q] = ok ? len : -1;
	for (int k = ok ? len : 0; k < b.radius; k++) row[k] = -1;
}

// ---- shortening action queues against the ball ---------------------------------------------------------------------------------
// (the limits, shorten_compose, the DP and its kernel, the emit but for the word of a replaced edge and the argument checks are in
// rk_shorten_dev.h: rk_sym.hip's rk_sshorten runs the same ones)
// d(i, j) of every window of queue p that starts at i: wave (p, i), lane = offset inside a chunk of 64 moves.  The byte of window
// (i, j) is depth[(p * max_len + j - 1) * window + (j - i - 1)]: the row of an END j is contiguous, which is how the DP reads it.
__global__ __launch_bounds__(256)
void k_shorten_windows(BallView b, const int8_t *__restrict__ actions, const int32_t *__restrict__ len, size_t n, int max_len, int window,
                       int8_t *__restrict__ depth)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int lane = threadIdx.x & 63;
	const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (w >= n * (size_t)max_len) return;                                // (whole waves)
	const size_t p = w / (size_t)max_len;
	const int i = (int)(w - p * (size_t)max_len);
	const int L = shorten_len(len, p, max_len);
	if (i >= L) return;
	const int8_t *row = actions + p * (size_t)max_len;
	const int moves = min(window, L - i);                                // windows (i, i + 1) .. (i, i + moves)
	uint32_t s[5] = {SOLVED_DW[0], SOLVED_DW[1], SOLVED_DW[2], SOLVED_DW[3], SOLVED_DW[4]};
	uint32_t a_next = lane < moves ? (uint32_t)(uint8_t)row[i + lane] : 0xFFu;
	for (int d0 = 0; d0 < moves; d0 += 64) {
		const int nc = min(64, moves - d0);
		const uint32_t a = a_next;
		a_next = d0 + 64 + lane < moves ? (uint32_t)(uint8_t)row[i + d0 + 64 + lane] : 0xFFu;    // behind the six scan steps
		uint32_t st[5];
		shorten_compose(s_act, a, lane, nc, s, st);
		if (lane < nc) {
			const uint32_t e = probe_find(b.table, b.mask, b.states, st);
			const int k = d0 + lane;                                         // j - i - 1
			depth[(p * (size_t)max_len + (size_t)(i + k)) * (size_t)window + (size_t)k] = (int8_t)(e ? level_of(b.lstart, e) : -1);
		}
		shorten_carry(st, nc, s);                                        // into the next chunk
	}
}

// The rewritten queue of queue blockIdx.x: one wave (shorten_emit).  The word of a replaced edge is the ball's own: X(i, j) is
// probed (its level must be the stored d), then the stored actions from the node down to node 1 -- they lead away from solved, so
// the last one first.  Lane 0 writes.
__global__ __launch_bounds__(64)
void k_shorten_emit(BallView b, const int8_t *__restrict__ actions, const int32_t *__restrict__ len, int max_len, int window,
                    const int8_t *__restrict__ depth, const uint16_t *__restrict__ pred, int8_t *__restrict__ out_actions,
                    int32_t *__restrict__ out_len, int32_t *error)
{
	__shared__ u32x4 s_act[36];
	const int lane = threadIdx.x;
	stage_action_tables(s_act, lane);
	shorten_emit(s_act, actions, len, max_len, window, depth, pred, out_actions, out_len, error, [&](const uint32_t x[5], int d, int8_t *at) {
		uint32_t g = probe_find(b.table, b.mask, b.states, x);
		if (g == 0u || level_of(b.lstart, g) != d || d > b.radius) return false;
		for (int k = d - 1; k >= 0; k--) {
			if (g <= 1u || g >= b.cap1) return false;
			if (lane == 0) at[k] = (int8_t)b.pact[g];
			g = (uint32_t)b.parent[g];
		}
		return g == 1u;
	});
}

// ---- the search from a start towards the ball -------------------------------------------------------------------------------
// (the pool, the counters, the level bookkeeping and the scan, append, end and rehash bodies are in rk_frontier_dev.h: every
// breadth-first engine runs the same ones)
// ---- the bodies: what one search does in a launch, for the single engine (k_bsearch_*) and for one slot of a batch (kb_bsearch_*) ----
__device__ __forceinline__ void bsearch_root(const FrontierDev &d, const BallView &b, const uint32_t *root, int budget)
{
	const int tid = threadIdx.x;
	if (tid < S_COUNT) d.ctr[tid] = 0;
	__syncthreads();
	if (tid != 0) return;
	uint32_t s[5];
	load5(root, s);
	srch_root_store(d, s, budget, probe_find(b.table, b.mask, b.states, s));     // (a start the ball holds: nothing is popped)
}

// fan-out, the look-up in the ball (read-only), then membership / election in the own table: one thread per child
__device__ __forceinline__ void bsearch_expand(const FrontierDev &d, const BallView &b)
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
	// no state is in both pools (the start is outside the ball and nothing the ball holds is ever stored), so the order of the two
	// look-ups decides nothing; the ball first, so that a meeting child leaves no claim in the own table
	const uint32_t m = probe_find(b.table, b.mask, b.states, s);
	if (m != 0u) srch_meet(d, c, m);
	else srch_claim(d, s_act, head, c, s);
}

// The action queue of a won search: the path from the start to the popped parent and the meeting action (none of either when
// the ball holds the start itself), then the ball's path from the meeting node.  out[0] = length or -1.
__device__ __forceinline__ void bsearch_walk(const FrontierDev &d, const BallView &b, int32_t *out, int max_len)
{
	out[0] = -1;
	if (!d.ctr[F_WON]) return;
	const int p = d.ctr[F_WPARENT];
	const int ls = p != 0 ? fr_walk_up(d, p, out + 1, max_len, true) : 0;
	if (ls < 0) return;
	int len = ls;
	if (p != 0) {
		if (len < max_len) out[1 + len] = d.ctr[F_WACT];
		len++;
	}
	for (uint32_t g = (uint32_t)d.ctr[S_MEET]; g != 1u; len++) {
		if (g < 1u || g >= b.cap1 || len > ls + 1 + b.radius) return;
		if (len < max_len) out[1 + len] = b.pact[g] ^ 1;
		g = (uint32_t)b.parent[g];
	}
	out[0] = len;
}

// ---- the single engine: one search per launch (scan, append, end and rehash: rk_frontier_dev.h's k_fr_*, k_srch_end) ----
__global__ void k_bsearch_root(FrontierDev d, BallView b, const uint32_t *root, int budget) { bsearch_root(d, b, root, budget); }

__global__ __launch_bounds__(256)
void k_bsearch_expand(FrontierDev d, BallView b) { bsearch_expand(d, b); }

__global__ void k_bsearch_walk(FrontierDev d, BallView b, int32_t *out, int max_len) { if (threadIdx.x == 0 && blockIdx.x == 0) bsearch_walk(d, b, out, max_len); }

// ---- the batch: S searches in lock-step, slot blockIdx.y of `devs` per workgroup row (rk_astar.hip: kb_merge_pass) ----
// Every slot is a whole search of its own -- pool, table, counters, batch scratch, look-back words, ticket and epoch --, so a
// launch reads and writes through devs[blockIdx.y] alone.  A slot that is done, or was never started, has F_NPOP == 0: it leaves
// at that read, draws no ticket and leaves its epoch alone.  The pool of a slot never grows: the pool-full rule (srch_fit,
// BS_STOP_FULL) and the clear, scan, append and end of all slots (kb_srch_*) are rk_frontier_dev.h's, shared with rk_sym.hip's
// rk_ssearchb_*.

// row j of roots / budgets starts slot slots[j]
__global__ void kb_bsearch_root(const FrontierDev *devs, BallView b, const int32_t *slots, const uint32_t *roots, const int32_t *budgets)
{
	const FrontierDev d = devs[slots[blockIdx.y]];
	bsearch_root(d, b, roots + (size_t)blockIdx.y * 5, budgets[blockIdx.y]);
	if (threadIdx.x == 0) srch_fit(d);
}

__global__ __launch_bounds__(256)
void kb_bsearch_expand(const FrontierDev *devs, BallView b)
{
	const FrontierDev d = devs[blockIdx.y];
	if (blockIdx.x * 256 >= 12 * d.ctr[F_NPOP]) return;                  // done, never started, or a workgroup past the batch
	bsearch_expand(d, b);
}

// one thread per slot: row s of `out` (n_slots, 1 + max_len) = length or -1, then the queue
__global__ __launch_bounds__(64)
void kb_bsearch_walk(const FrontierDev *devs, BallView b, int n_slots, int32_t *out, int max_len)
{
	const int s = blockIdx.x * 64 + threadIdx.x;
	if (s >= n_slots) return;
	const FrontierDev d = devs[s];
	bsearch_walk(d, b, out + (size_t)s * (1 + max_len), max_len);
}

}  // namespace rk

using namespace rk;

struct rk_ball : KeptBall {
	BallDev d{};
	BallView view{};
};

struct rk_bsearch : FrontierPool, BallReader<rk_ball> {};

// S searches in lock-step: the slots (rk_frontier_host.h: FrontierSlots) and the ball they all read
struct rk_bsearchb : FrontierSlots, BallReader<rk_ball> {};

namespace {

size_t ball_capacity(int radius)
{
	size_t n = 0;
	for (int l = 0; l <= radius; l++) n += (size_t)BALL_LEVELS[l];
	return n;
}

}  // namespace

extern "C" {

int rk_ball_create(rk_ball_t **out, int radius, int pops)
{
	if (int e = KeptBall::check_create("rk_ball_create", out, radius, BALL_MAX_RADIUS, pops)) return e;
	rk_ball *h = new rk_ball();
	h->describe(h->d, ball_capacity(radius), radius, pops);
	*out = h;
	return RK_OK;
}

int rk_ball_destroy(rk_ball_t *h)
{
	if (int e = KeptBall::check_destroy("rk_ball_destroy", h)) return e;
	delete h;
	return RK_OK;
}

int rk_ball_build(rk_ball_t *h, int poll, void *stream)
{
	if (int e = KeptBall::check_build("rk_ball_build", h, poll)) return e;
	if (h->built) return RK_OK;
	hipStream_t st = (hipStream_t)stream;
	BallDev &d = h->d;
	const size_t C1 = h->cap + 1, K = (size_t)12 * d.pops;
	const unsigned grid = blocks(K);
	int32_t c[BB_COUNT];
	if (int e = h->run_build("rk_ball_build", "states", d, poll, st, c,
	                         [&] { const int e = h->pool.alloc(&d.parent, C1); return e ? e : h->pool.alloc(&d.pact, C1); },
	                         [&] { hipLaunchKernelGGL(k_ball_root, dim3(1), dim3(64), 0, st, d); },
	                         [&] {
		                         hipLaunchKernelGGL(k_ball_expand, dim3(grid), dim3(256), 0, st, d);
		                         hipLaunchKernelGGL(k_ball_scan, dim3(blocks(K, ASCAN)), dim3(ASCAN), 0, st, d);
		                         hipLaunchKernelGGL(k_ball_append, dim3(grid), dim3(256), 0, st, d);
		                         hipLaunchKernelGGL(k_ball_end, dim3(1), dim3(64), 0, st, d);
	                         }))
		return e;
	if (c[BB_ERROR] || c[BB_STOP] != BB_STOP_BUILT || (size_t)c[BB_SIZE] != h->cap)      // (the arrays stay until the next build clears them)
		return fail(RK_ESTATE, "rk_ball_build: engine error %d: %d states after level %d, %zu expected in all", c[BB_ERROR], c[BB_SIZE], c[BB_LEVEL], h->cap);
	h->finish_build(d, c, h->view);
	h->view.parent = d.parent; h->view.pact = d.pact;
	return RK_OK;
}

int rk_ball_status(rk_ball_t *h, long long *h_status)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_ball_status: null argument");
	h->status_words(h_status, h->d.radius, h->view.lstart);
	h_status[5] = h->attached;
	return RK_OK;
}

int rk_ball_export(rk_ball_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_ball_export: null ball");
	if (!h->built) return fail(RK_ESTATE, "rk_ball_export: build the ball first");
	if (first + count > h->cap + 1) return fail(RK_EINVAL, "rk_ball_export: rows %zu..%zu outside the pool", first, first + count);
	return export_pool_rows(h->d.states, h->d.parent, h->d.pact, first, count, h_states, h_parents, h_actions, nullptr, (hipStream_t)stream);
}

int rk_ball_depth(rk_ball_t *h, const int8_t *d_states, size_t n, int32_t *d_depth, void *stream)
{
	if (int e = KeptBall::check_queries("rk_ball_depth", "queries", h, d_states, n, d_depth)) return e;
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_ball_depth, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, h->view,
	                   reinterpret_cast<const uint32_t *>(d_states), n, d_depth);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_ball_solve(rk_ball_t *h, const int8_t *d_states, size_t n, int32_t *d_lengths, int8_t *d_actions, void *stream)
{
	if (int e = KeptBall::check_queries("rk_ball_solve", "queries", h, d_states, n, d_lengths)) return e;
	if (n == 0) return RK_OK;
	if (!d_actions && h->d.radius > 0) return fail(RK_EINVAL, "rk_ball_solve: null pointer");
	hipLaunchKernelGGL(k_ball_solve, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, h->view,
	                   reinterpret_cast<const uint32_t *>(d_states), n, d_lengths, d_actions);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

long long rk_bshorten_scratch_bytes(size_t n, int max_len, int window)
{
	if (max_len < 1 || max_len > SHORTEN_MAX_LEN || window < 1 || window > max_len)
		return fail(RK_EINVAL, "rk_bshorten_scratch_bytes: need 1 <= window <= max_len <= %d, got window %d, max_len %d", SHORTEN_MAX_LEN, window, max_len);
	if (n > SHORTEN_MAX_WAVES / (size_t)max_len) return fail(RK_EINVAL, "rk_bshorten_scratch_bytes: %zu queues of %d moves in one call", n, max_len);
	return (long long)(shorten_depth_bytes(n, max_len, window) + n * (size_t)(max_len + 1) * sizeof(uint16_t));
}

int rk_bshorten(rk_ball_t *h, const int8_t *d_actions, const int32_t *d_len, size_t n, int max_len, int window, int8_t *d_out_actions,
                int32_t *d_out_len, int32_t *d_error, void *d_scratch, size_t scratch_bytes, void *stream)
{
	if (int e = shorten_check("rk_bshorten", h, h && h->built, d_actions, d_len, n, max_len, window, d_out_actions, d_out_len, d_error, d_scratch,
	                          scratch_bytes))
		return e;
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemsetAsync(d_error, 0, sizeof(int32_t), st));
	if (n == 0) return RK_OK;
	int8_t *depth = static_cast<int8_t *>(d_scratch);
	uint16_t *pred = reinterpret_cast<uint16_t *>(depth + shorten_depth_bytes(n, max_len, window));
	hipLaunchKernelGGL(k_shorten_windows, dim3(blocks(n * (size_t)max_len, 4)), dim3(256), 0, st, h->view, d_actions, d_len, n, max_len, window, depth);
	hipLaunchKernelGGL(k_shorten_dp, dim3((unsigned)n), dim3(SHORTEN_DP_THREADS), 0, st, d_actions, d_len, max_len, window, depth, pred, d_error);
	hipLaunchKernelGGL(k_shorten_emit, dim3((unsigned)n), dim3(64), 0, st, h->view, d_actions, d_len, max_len, window, depth, pred, d_out_actions,
	                   d_out_len, d_error);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_bsearch_create(rk_bsearch_t **out, rk_ball_t *ball, size_t capacity, int pops)
{
	if (!out || !ball) return fail(RK_EINVAL, "rk_bsearch_create: null argument");
	if (int e = FrontierPool::check_create("rk_bsearch_create", capacity, pops)) return e;
	rk_bsearch *h = new rk_bsearch();
	if (int e = h->alloc(capacity, pops, S_COUNT)) { delete h; return e; }
	h->attach(ball);
	*out = h;
	return RK_OK;
}

int rk_bsearch_destroy(rk_bsearch_t *h)
{
	delete h;                                   // (lets go of the ball: BallReader)
	return RK_OK;
}

int rk_bsearch_reset(rk_bsearch_t *h, const int8_t *h_start_state, long long max_states, void *stream)
{
	if (!h || !h_start_state) return fail(RK_EINVAL, "rk_bsearch_reset: null argument");
	if (!h->ball->built) return fail(RK_ESTATE, "rk_bsearch_reset: build the ball first");
	hipStream_t st = (hipStream_t)stream;
	return h->reset(h_start_state, st, [&] {
		hipLaunchKernelGGL(k_bsearch_root, dim3(1), dim3(64), 0, st, h->d, h->ball->view, h->root_dev, budget_of(max_states));
	});
}

int rk_bsearch_run(rk_bsearch_t *h, int iterations, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bsearch_run")) return e;
	hipStream_t st = (hipStream_t)stream;
	return h->run("rk_bsearch_run", iterations, st,
	              [&](unsigned grid) { hipLaunchKernelGGL(k_bsearch_expand, dim3(grid), dim3(256), 0, st, h->d, h->ball->view); });
}

int rk_bsearch_status(rk_bsearch_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_bsearch_status: bad argument");
	int32_t c[S_COUNT];
	if (int e = h->read_ctr(c, (hipStream_t)stream)) return e;
	bsearch_status_words(c, h_status);
	return RK_OK;
}

int rk_bsearch_grow(rk_bsearch_t *h, size_t new_capacity, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bsearch_grow")) return e;
	return h->grow("rk_bsearch_grow", new_capacity, (hipStream_t)stream);
}

long long rk_bsearch_size(const rk_bsearch_t *h) { return FrontierPool::size(h); }

int rk_bsearch_export(rk_bsearch_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bsearch_export")) return e;
	return h->export_rows("rk_bsearch_export", first, count, h_states, h_parents, h_actions, nullptr, (hipStream_t)stream);
}

int rk_bsearchb_create(rk_bsearchb_t **out, rk_ball_t *ball, int n_slots, size_t capacity_per_slot, int pops)
{
	if (int e = FrontierSlots::check_create("rk_bsearchb_create", out, ball, n_slots, capacity_per_slot, pops)) return e;
	rk_bsearchb *h = new rk_bsearchb();
	if (int e = h->alloc("rk_bsearchb_create", n_slots, capacity_per_slot, pops, [] { return RK_OK; })) { delete h; return e; }
	h->attach(ball);
	*out = h;
	return RK_OK;
}

int rk_bsearchb_destroy(rk_bsearchb_t *h)
{
	delete h;
	return RK_OK;
}

int rk_bsearchb_reset(rk_bsearchb_t *h, int n, const int32_t *slots, const int8_t *h_start_states, const long long *max_states, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_bsearchb_reset: null engine");
	hipStream_t st = (hipStream_t)stream;
	return h->reset("rk_bsearchb_reset", h->ball->built, n, slots, h_start_states, max_states, st, [&] {
		hipLaunchKernelGGL(kb_bsearch_root, dim3(1, n), dim3(64), 0, st, h->devs, h->ball->view, h->slots_dev, h->roots_dev, h->budgets_dev);
	});
}

int rk_bsearchb_run(rk_bsearchb_t *h, int iterations, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_bsearchb_run: null engine");
	hipStream_t st = (hipStream_t)stream;
	return h->run("rk_bsearchb_run", h->ball->built, iterations, st,
	              [&](dim3 grid) { hipLaunchKernelGGL(kb_bsearch_expand, grid, dim3(256), 0, st, h->devs, h->ball->view); });
}

int rk_bsearchb_status(rk_bsearchb_t *h, long long *h_status, void *stream)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_bsearchb_status: null argument");
	return h->status(h_status, (hipStream_t)stream);
}

int rk_bsearchb_paths(rk_bsearchb_t *h, int32_t *h_out, int max_len, void *stream)
{
	if (!h || !h_out) return fail(RK_EINVAL, "rk_bsearchb_paths: null argument");
	hipStream_t st = (hipStream_t)stream;
	return h->paths("rk_bsearchb_paths", h->ball->built, h_out, max_len, st, [&] {
		hipLaunchKernelGGL(kb_bsearch_walk, dim3(blocks((size_t)h->n_slots, 64)), dim3(64), 0, st, h->devs, h->ball->view, h->n_slots, h->walk, max_len);
	});
}

int rk_bsearchb_export(rk_bsearchb_t *h, int slot, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_bsearchb_export: null engine");
	return h->export_rows("rk_bsearchb_export", slot, first, count, h_states, h_parents, h_actions, (hipStream_t)stream);
}

long long rk_bsearch_path(rk_bsearch_t *h, long long *h_actions, size_t max_len, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_bsearch_path")) return e;
	if (!h_actions && max_len > 0) return fail(RK_EINVAL, "rk_bsearch_path: null h_actions with max_len %zu", max_len);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_bsearch_walk, dim3(1), dim3(64), 0, st, h->d, h->ball->view, h->walk, FRONTIER_WALK_MAX);
	RK_HIP(hipGetLastError());
	int32_t len = 0;
	if (int e = read_walk(h->walk, FRONTIER_WALK_MAX, h_actions, max_len, st, &len)) return e;
	if (len < 0) return fail(RK_ESTATE, "rk_bsearch_path: the search has not met the ball (or a parent chain is broken)");
	return (long long)len;
}

}  // extern "C"
