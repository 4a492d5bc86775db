// The 48 symmetries of the cube on the device: conjugates and canonical representatives of batches of states (rk_sym_*), and
// the symmetry-reduced goal ball (rk_symball_*): one representative per orbit of the states within `radius` quarter turns of
// solved.  Conjugation relabels the actions and keeps the distance to solved (rk_sym_tables.h), so the depth of a representative
// is the depth of the up to 48 states of its orbit, and a ball of representatives reaches about two levels further than the plain
// ball of rk_ball.hip in the same memory.  It keeps no parent and no action either: a shortest solution is found by descent.
//
// Canonicalisation (rk_sym_dev.h) is a WAVE per state: lane = symmetry, 48 of 64 lanes live, the tables staged in LDS once per
// workgroup, the minimum of the 48 conjugates taken across the wave.  A kernel that asks the ball about states declares its LDS,
// makes one SymProbe (sym_probe: the staging, the barrier, the lane's symmetry) and asks sb_node / sb_level / sb_descend.
//   k_sym_canonical   waves stride over the states: representative, lowest symmetry that gives it, orbit size
//   k_sym_conjugate   one given symmetry, a thread per state (every lane reads the same table rows)
//
// The ball is the level-by-level build of rk_ballbuild_dev.h (counters, root, next, expand, scan, append, end) over
// representatives: the children of a level's representatives are canonicalised before the election.
//   states  int8 (C+1, 20), table uint32 (T = pow2 >= 2C); no parent, no action
// The election compares a child with OTHER children of the batch, one thread per child, and a canonical form takes a wave, so
// an iteration has one launch in front that writes the representatives of the batch to scratch
//   k_sb_canon    a wave per child: fan-out, canonical form, orbit size          -> cstate (12 P, 5), corbit (12 P)
//   k_sb_expand   bb_expand; the state of batch position c is cstate[c]
//   k_sb_scan     bb_scan
//   k_sb_append   bb_append from cstate; the orbit sizes of what a wave stored are added to the sum of the level
//   k_sb_end      bb_end, then sb_next
// Level check: the orbit sizes of a level add up to the level size of the quarter-turn Cayley graph; a closed level 0..8 is
// compared with BALL_LEVELS (BB_ERR_LEVEL otherwise).  Levels 9 and 10 are summed (64 bits) and reported but not compared: the
// project holds no published table for them.
// Capacity: orbit counts are not known in advance, so the pool has the size the caller asks for.  P is cut to what fits whatever
// the batch finds (size + 12 P <= C); when not even one pop fits, the build stops BEFORE the iteration with BB_STOP_FULL.  The
// append checks every index all the same.
// After the build the ball is read-only:
//   k_sb_depth    a wave per query: canonical form, read-only probe (probe_find), depth from the level boundaries; -1 outside
//   k_sb_solve    the same, then the descent: at each step the lowest action whose child lies one level nearer (12 canonical
//                 forms and probes at most), bounded by the radius; a step without such a child sets the error word
//   k_sb_child_values   k_sb_depth for the 12 n children of an ADI rollout (rk_symball_child_values): the depth as a byte and the exact
//                 value V*(depth) beside it; then k_sb_outside_count, _scan, _write compact the rows OUTSIDE the ball -- the net's
//                 batch -- in ascending order
//   k_sb_state_at the other way round, a wave per sample: (depth, rank) -> the state, through an index over the orbit sizes that is
//                 made at the first call (k_sb_orbit, _orbit_count, _orbit_scan, _orbit_base) and kept with the ball
//   k_sb_child_depths   a wave per state: the level of the state and of its 12 children, made exact within radius + 1 by parity
//
// The search (rk_ssearch_*) is rk_ball.hip's rk_bsearch_* -- a one-sided breadth-first search from a start, in a pool and table of
// its own that hold RAW states with parent and action -- with one difference: "the ball holds this child" is "the symmetry ball
// holds this child's representative".  A state lies in the plain ball of radius R exactly when its representative lies in this
// one, so the own pool, the depth, the pops and the meeting child are rk_bsearch's on a plain ball of the same radius, bit for
// bit.  The election among the children of a batch is on the raw child, so no representative goes to scratch: a canonical form
// takes a wave, the election a thread, hence one launch more than rk_bsearch, the rest is shared (rk_frontier_dev.h)
//   k_ss_probe    a wave per child: fan-out, canonical form, read-only probe of the ball  -> hit (12 P): the ball's node or 0
//   k_ss_expand   a thread per child: hit != 0 is a meeting (atomicMin on the win position, no claim), else membership / election
//                 in the own table on the raw child
//   k_fr_scan, k_fr_append, k_srch_end, k_fr_rehash   rk_frontier_dev.h's, the plain search's too; S_MEET is the node in THIS ball
//   k_ss_walk     one wave: the own path and the meeting action, then the descent from the meeting state (sb_descend)
//
// The batch (rk_ssearchb_*) is S such searches in lock-step, as rk_ball.hip's rk_bsearchb_* is of rk_bsearch_*.  The bodies of the root,
// the probe, the expand and the walk are __device__ functions of a FrontierDev (ssearch_*); the single engine's kernels pass theirs
// by value, the batch's (kb_ss_*) pick devs[blockIdx.y], so an iteration of all slots is the same five launches with S in the
// grid's second dimension.  Every kind of array is one block sliced per slot -- pool, parents, actions, table, counters, batch
// scratch, look-back words and 12 P words of `hit` --; all slots read one ball.
//   kb_ss_probe   grid (k_ss_probe's x, S): a workgroup whose first child is past 12 * F_NPOP of its slot -- done, never started, a
//                 short batch -- returns BEFORE it stages the tables; writes nothing but the slot's hit
//   kb_ss_expand  ssearch_expand behind kb_bsearch_expand's early exit
//   kb_srch_scan, kb_srch_append, kb_srch_end   rk_frontier_dev.h's, the plain batch's too: fr_scan, fr_append, srch_end behind the
//                 early exits (a slot with F_NPOP == 0 draws no ticket and leaves its epoch alone); srch_fit follows the end
//   kb_ss_root    one wave per named slot, then srch_fit; kb_srch_clear zeroes the named slots' tables and look-back words first
//   kb_ss_walk    one wave per slot (the descent needs lane = symmetry) into row s of (S, 1 + max_len)
// A slot's pool is fixed: it stops with reason 5 before an iteration that might not fit (rk_frontier_dev.h: srch_fit).  The host
// side -- the slot block, the reset's checks, the iteration loop, the status fetch, the paths buffer, the export -- is FrontierSlots
// (rk_frontier_host.h), shared with rk_bsearchb; this engine adds the hit block and the probe launch.
//
// Shortening (rk_sshorten) is rk_ball.hip's rk_bshorten -- the same contract, scratch, DP and copy rule (rk_shorten_dev.h) -- with
// d(i, j) = the depth of the REPRESENTATIVE of X(i, j), which is the plain ball's d(i, j) at the same radius, so the lengths are
// rk_bshorten's queue for queue.  There is no stored word for a replaced edge: it gets the inverse of the descent from X(i, j),
// i.e. rk_symball_solve's word reversed with every action ^ 1, which may differ from the plain ball's word of the same length.
//   k_ss_windows  a persistent grid, waves stride over the (queue, i) pairs, the tables staged once per workgroup: the windows
//                 composed with lane = offset, then one canonical form (lane = symmetry) and one probe per window
//   k_shorten_dp  rk_shorten_dev.h's, the plain ball's too
//   k_ss_emit     a wave per queue (shorten_emit): a replaced edge is composed again, canonicalised, probed, descended and written
//                 inverted
// Three launches; nothing of the ball is written.
//
// Deepening (rk_sdeepen, rk_sdeepen_*) goes on where memory ends: short words applied to a state, each result canonicalised
// and probed, nothing kept but the lowest rank that hit (rk_deepen_dev.h: the words, their ranks, the item of a wave).
//   k_sd_probe       a persistent grid, waves stride over the (state, 121 ranks) items, the tables staged once per workgroup; on
//                    the caller's states (rk_sdeepen) or on rows of a search's pool with the stored action as the last move
//   k_sd_probe_pruned  k_sd_probe with the words that an admissible bound of pattern databases rules out left unprobed
//                    (rk_sdeepen_pruned, rk_sdeepen_nodes_pruned; rk_deepen_dev.h: PdbPrune): the same lowest ranks, fewer look-ups
//   k_ss_setpops     one thread: a lower pop count for the iterations to come (the host lowers it when the pool is nearly full)
//   k_ss_deepen_walk one wave: the path to a pool node, a word from it, then the descent from the moved state
// In the batch (rk_sdeepenb_set, _frontiers, _probe, _keys, _paths) a slot whose pool is full goes on the
// same way beside the slots that still pop.  Its pool phase ends where pops = 1 would end it (rk_frontier_dev.h: S_CLIP, srch_fit).
//   kb_sd_probe        grid (k_sd_probe's x, jobs): one launch for all deepening slots, each job a node range and a word range of
//                      one slot in a round of its own; deepen_probe's body, one 64-bit key per slot instead of a word per node
//   kb_ss_deepen_walk  one wave per named slot: k_ss_deepen_walk's body (ssearch_deepen_walk)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>

#include "../../include/rubiks_hip.h"
#include "rk_deepen_dev.h"
#include "rk_frontier_dev.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_search_dev.h"
#include "rk_frontier_host.h"
#include "rk_shorten_dev.h"
#include "rk_sym_dev.h"

namespace rk {

// levels 9 and 10 as the literature is recalled to give them: used for the default capacity only, never compared
constexpr long long SB_LEVELS_UNCHECKED[2] = {717789576ll, 6701836858ll};
static_assert(BB_LSTART + SB_MAX_RADIUS + 2 <= BB_COUNT, "the level boundaries do not fit the counter block");

struct SymBallDev : BuildDev {
	unsigned long long *cover;                  // [SB_MAX_RADIUS + 1]: the orbit sizes of every level added up
	uint32_t *cstate; uint8_t *corbit;          // per child of the batch: its representative and its orbit size (freed after the build)
};

// the orbit sizes of a closed level 0..8 add up to the level's size in the graph; P is cut to what fits the caller's capacity
__device__ __forceinline__ void sb_next(const SymBallDev &d)
{
	bb_next<true>(d, [&](int level, int32_t) { return level > BALL_CHECKED || d.cover[level] == (unsigned long long)D_BALL_LEVELS[level]; });
}

__global__ void k_sb_root(SymBallDev d)
{
	bb_root(d, [&](int tid) { if (tid <= SB_MAX_RADIUS) d.cover[tid] = tid == 0 ? 1ull : 0ull; }, [&] { sb_next(d); });
}

// the representative and the orbit size of every child of the batch: waves stride over the children
__global__ __launch_bounds__(256)
void k_sb_canon(SymBallDev d)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const int K = 12 * d.ctr[BB_NPOP];
	if ((int)blockIdx.x * 4 >= K) return;                                // done, or a workgroup past the batch: nothing staged
	const SymProbe sp = sym_probe(s_sym, 256, s_act);
	const int lane = sp.lane;
	const int32_t head = d.ctr[BB_HEAD];
	for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < K; c += gridDim.x * 4) {       // (whole waves)
		const int i = c / 12, a = c - 12 * i;
		uint32_t x[5], rep[5];
		child_state(d.states, head + i, s_act, (uint32_t)a, x);
		int sym, count;
		sym_canonical(s_sym, sp.L, lane, x, rep, &sym, &count);
		if (lane < 5) d.cstate[(size_t)c * 5 + lane] = dword_of(rep, lane);
		if (lane == 5) d.corbit[c] = (uint8_t)(N_SYM / count);
	}
}

// the state of batch position c is its representative, from the scratch k_sb_canon wrote
__global__ __launch_bounds__(256)
void k_sb_expand(SymBallDev d)
{
	bb_expand(d, [&](int c, uint32_t o[5]) { load5(d.cstate + (size_t)c * 5, o); });
}

__global__ __launch_bounds__(ASCAN)
void k_sb_scan(SymBallDev d) { bb_scan(d); }

// every first occurrence is stored, and its orbit size added to the sum of the level that is being filled
__global__ __launch_bounds__(256)
void k_sb_append(SymBallDev d)
{
	const int K = 12 * d.ctr[BB_NPOP];
	if ((int)blockIdx.x * 256 >= K) return;                              // (whole workgroups: every lane of a wave reaches the sum)
	const int c = blockIdx.x * 256 + threadIdx.x;
	uint32_t orbit = 0;
	if (c < K && d.first[c] && bb_append(d, c, [&](uint32_t, uint32_t s[5]) { load5(d.cstate + (size_t)c * 5, s); }))
		orbit = d.corbit[c];                                             // (never refused: P was cut to what fits)
	#pragma unroll
	for (int m = 32; m > 0; m >>= 1) orbit += (uint32_t)__shfl_xor((int)orbit, m, 64);
	if ((threadIdx.x & 63) == 0 && orbit != 0u) atomicAdd(&d.cover[d.ctr[BB_LEVEL] + 1], (unsigned long long)orbit);
}

__global__ void k_sb_end(SymBallDev d) { bb_end(d, [&] { sb_next(d); }); }

// exact distance to solved of query q, -1 outside the ball: waves stride over the queries, nothing is written but the answer
__global__ __launch_bounds__(256)
void k_sb_depth(SymBallView b, const uint32_t *queries, size_t n, int32_t *depth)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	const SymProbe sp = sym_probe(s_sym, 256);
	for (size_t q = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (size_t)gridDim.x * 4) {
		uint32_t x[5];
		load5(queries + q * 5, x);
		const int lvl = sb_level(b, sp, x);
		if (sp.lane == 0) depth[q] = lvl;
	}
}

// the shortest solution of query q by descent; row q of `actions` (n, radius) is padded with -1, lengths[q] = -1 outside the ball
__global__ __launch_bounds__(256)
void k_sb_solve(SymBallView b, const uint32_t *queries, size_t n, int32_t *lengths, int8_t *actions, int32_t *error)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const SymProbe sp = sym_probe(s_sym, 256, s_act);
	const int lane = sp.lane;
	for (size_t q = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (size_t)gridDim.x * 4) {
		uint32_t x[5];
		load5(queries + q * 5, x);
		int8_t *row = actions + q * (size_t)b.radius;
		const int depth = sb_level(b, sp, x);
		bool ok;
		const int len = sb_descend(b, sp, x, depth, [&](int k, int a) { if (lane == 0) row[k] = (int8_t)a; }, &ok);
		if (depth >= 0 && !ok && lane == 0) *error = RK_ESTATE;
		if (lane == 0) lengths[q] = ok ? len : -1;
		for (int k = (ok ? len : 0) + lane; k < b.radius; k += 64) row[k] = -1;
	}
}

// ---- exact values of the children of an ADI rollout (rk_symball_child_values) ----
// k_sb_depth's loop with an int8 answer and V*(c) beside it: 0 at c = 0, g - (c - 1) at 1 <= c <= radius (small integers: exact
// in float32); values[q] of a row outside the ball is not touched.
__global__ __launch_bounds__(256)
void k_sb_child_values(SymBallView b, const uint32_t *states, size_t n, float g, int8_t *depth, float *values)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	const SymProbe sp = sym_probe(s_sym, 256);
	for (size_t q = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (size_t)gridDim.x * 4) {
		uint32_t x[5];
		load5(states + q * 5, x);
		const int lvl = sb_level(b, sp, x);
		if (sp.lane == 0) {
			depth[q] = (int8_t)lvl;
			if (lvl >= 0) values[q] = lvl == 0 ? 0.0f : g - (float)(lvl - 1);
		}
	}
}

// The rows outside the ball in ascending order, by a scan and not by a counter: the order is what the net's slices are cut from.
// A tile is ASCAN rows, a thread per row.  Three launches and no waiting inside any of them: the tiles' counts, their exclusive
// prefix in place by ONE workgroup (a tile count per 256 rows: 10 547 words for the 2.7 M children of a reference rollout), then
// every tile ranks its rows again (block_rank256) and writes the row index and the 20 bytes of the state at base + rank.
__global__ __launch_bounds__(ASCAN)
void k_sb_outside_count(const int8_t *depth, size_t n, int32_t *tile)
{
	__shared__ int s_wave[4];
	const size_t q = (size_t)blockIdx.x * ASCAN + threadIdx.x;
	int total;
	(void)block_rank256(q < n && depth[q] < 0, s_wave, &total);
	if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

constexpr int SB_SCAN_THREADS = 1024;

__global__ __launch_bounds__(SB_SCAN_THREADS)
void k_sb_outside_scan(int32_t *tile, int tiles, int32_t *count)
{
	__shared__ int s_sum[SB_SCAN_THREADS];
	const int t = threadIdx.x;
	const int per = (tiles + SB_SCAN_THREADS - 1) / SB_SCAN_THREADS;         // (at most 2^23 tiles: t * per stays far below 2^31)
	const int lo = min(t * per, tiles), hi = min(lo + per, tiles);
	int sum = 0;
	for (int i = lo; i < hi; i++) sum += tile[i];
	s_sum[t] = sum;
	__syncthreads();
	for (int off = 1; off < SB_SCAN_THREADS; off <<= 1) {
		const int v = t >= off ? s_sum[t - off] : 0;
		__syncthreads();
		s_sum[t] += v;
		__syncthreads();
	}
	int run = s_sum[t] - sum;
	for (int i = lo; i < hi; i++) {
		const int c = tile[i];
		tile[i] = run;
		run += c;
	}
	if (t == SB_SCAN_THREADS - 1) *count = s_sum[t];
}

__global__ __launch_bounds__(ASCAN)
void k_sb_outside_write(const int8_t *depth, const uint32_t *states, size_t n, const int32_t *tile, int32_t *rows, uint32_t *outside)
{
	__shared__ int s_wave[4];
	const size_t q = (size_t)blockIdx.x * ASCAN + threadIdx.x;
	const bool out = q < n && depth[q] < 0;
	int total;
	const int r = block_rank256(out, s_wave, &total);
	if (!out) return;
	const size_t at = (size_t)tile[blockIdx.x] + (size_t)r;                  // < the count <= n: the caller's arrays hold n rows
	rows[at] = (int32_t)q;
	uint32_t x[5];
	load5(states + q * 5, x);
	#pragma unroll
	for (int j = 0; j < 5; j++) outside[at * 5 + j] = x[j];
}

// ---- unranking the ball: the state of (depth, rank) (rk_symball_state_at) and exact depths around a state (rk_symball_child_depths) ----
// The orbit index, kept with the ball from the first rk_symball_state_at on.  Positions are nodes minus one, a tile is 256 of them:
//   orbit  one byte per position, the orbit size 48 / |stabiliser| of the node's representative; zero behind the last node up to
//          the end of the last tile, so a tile is always 64 whole dwords
//   tile   64-bit exclusive prefix of the orbit sizes per tile, tile[tiles] = the sum of all
//   base   base[l] = the orbit sizes of all nodes below level l added up, l = 0 .. radius + 1: levels are contiguous node ranges,
//          so the ranks of level l are the range base[l] .. base[l + 1] - 1 of the global cumulative
struct SymIndex {
	const uint32_t *orbit; const unsigned long long *tile;
	uint32_t tiles, len;
	unsigned long long base[SB_MAX_RADIUS + 2];
};

// the sum of the four bytes of a dword
__device__ __forceinline__ uint32_t bytes_sum(uint32_t w) { return (w & 0xFFu) + ((w >> 8) & 0xFFu) + ((w >> 16) & 0xFFu) + (w >> 24); }

// orbit[node - 1] of every node, a wave per node: the canonical form of the stored representative gives the stabiliser's size,
// and must give the representative itself at symmetry 0 -- a node that is not its own canonical form sets the error word
__global__ __launch_bounds__(256)
void k_sb_orbit(SymBallView b, uint32_t len, uint8_t *orbit, int32_t *error)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	const SymProbe sp = sym_probe(s_sym, 256);
	for (size_t p = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < (size_t)len; p += (size_t)gridDim.x * 4) {
		uint32_t x[5], rep[5];
		load5(b.states + (p + 1) * 5, x);
		int sym, count;
		sym_canonical(s_sym, sp.L, sp.lane, x, rep, &sym, &count);
		bool own = sym == 0;
		#pragma unroll
		for (int j = 0; j < 5; j++) own = own && rep[j] == x[j];
		if (sp.lane == 0) {
			orbit[p] = (uint8_t)(N_SYM / count);
			if (!own) *error = RK_ESTATE;
		}
	}
}

// the orbit sizes of a tile added up, a wave per tile: a dword per lane
__global__ __launch_bounds__(256)
void k_sb_orbit_count(const uint32_t *orbit, uint32_t tiles, unsigned long long *tile)
{
	const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= tiles) return;                                              // (whole waves)
	uint32_t sum = bytes_sum(orbit[(size_t)t * 64 + (threadIdx.x & 63)]);
	#pragma unroll
	for (int m = 32; m > 0; m >>= 1) sum += (uint32_t)__shfl_xor((int)sum, m, 64);
	if ((threadIdx.x & 63) == 0) tile[t] = sum;
}

// k_sb_outside_scan on 64-bit sums (the orbit sizes of radius 10 add up to 7.5e9): the exclusive prefix in place by ONE workgroup,
// tile[tiles] = the sum of all
__global__ __launch_bounds__(SB_SCAN_THREADS)
void k_sb_orbit_scan(unsigned long long *tile, uint32_t tiles)
{
	__shared__ unsigned long long s_sum[SB_SCAN_THREADS];
	const uint32_t t = threadIdx.x;
	const uint32_t per = (tiles + SB_SCAN_THREADS - 1) / SB_SCAN_THREADS;    // (at most 2^22 tiles: t * per stays far below 2^32)
	const uint32_t lo = min(t * per, tiles), hi = min(lo + per, tiles);
	unsigned long long sum = 0;
	for (uint32_t i = lo; i < hi; i++) sum += tile[i];
	s_sum[t] = sum;
	__syncthreads();
	for (uint32_t off = 1; off < SB_SCAN_THREADS; off <<= 1) {
		const unsigned long long v = t >= off ? s_sum[t - off] : 0ull;
		__syncthreads();
		s_sum[t] += v;
		__syncthreads();
	}
	unsigned long long run = s_sum[t] - sum;
	for (uint32_t i = lo; i < hi; i++) {
		const unsigned long long c = tile[i];
		tile[i] = run;
		run += c;
	}
	if (t == SB_SCAN_THREADS - 1) tile[tiles] = s_sum[t];
}

// base[l], l = 0 .. radius + 1, a thread per level boundary: the prefix of the boundary's tile and the bytes in front of it
__global__ __launch_bounds__(64)
void k_sb_orbit_base(SymBallView b, const uint8_t *orbit, const unsigned long long *tile, unsigned long long *base)
{
	const int l = threadIdx.x;
	if (l > b.radius + 1) return;
	const uint32_t p = (uint32_t)b.lstart[l] - 1u;                       // positions below level l (level radius + 1 starts behind the last node)
	unsigned long long sum = tile[p >> 8];                               // (p = len on a tile boundary reads tile[tiles])
	for (uint32_t q = p & ~255u; q < p; q++) sum += orbit[q];
	base[l] = sum;
}

// an inclusive prefix sum over the 64 lanes.  ALL 64 lanes call it.
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane)
{
	#pragma unroll
	for (int m = 1; m < 64; m <<= 1) {
		const uint32_t up = (uint32_t)__shfl_up((int)v, m, 64);
		if (lane >= m) v += up;
	}
	return v;
}

// Row i of `out` = the state of (depth[i], rank[i]): the k-th distinct conjugate, in ascending symmetry order, of the node of
// level depth[i] whose cumulative orbit range holds the rank.  Waves stride over the samples; everything up to the conjugates is
// the same in every lane (the wave index goes through readfirstlane, so the sample, its tile and its node are wave-uniform).
//   G = base[depth] + rank; the tile that holds G by bisection over the tiles of the level; the tile's 256 orbit bytes a dword per
//   lane, their sums scanned across the wave: the lane, then the byte, whose range holds G - tile[t] -> node j, k = what is left;
//   lane s < 48 conjugates the representative by s and is FIRST when no lower lane holds the same state; the first lanes are the
//   orbit (orbit[j] of them, anything else is RK_ESTATE), and the one with k first lanes below it writes its conjugate.
// A depth outside 0..radius or a rank outside the level sets RK_EINVAL and the row is zeroed, as is a row of a broken index.
// Nothing is written but `out` and the error word.
__global__ __launch_bounds__(256)
void k_sb_state_at(SymBallView b, SymIndex ix, const int32_t *depth, const long long *rank, size_t n, uint32_t *out, int32_t *error)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	const SymProbe sp = sym_probe(s_sym, 256);
	const int lane = sp.lane;
	for (size_t i = (size_t)blockIdx.x * 4 + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); i < n; i += (size_t)gridDim.x * 4) {
		const int d = depth[i];
		const long long r = rank[i];
		int bad = RK_OK;
		if (d < 0 || d > b.radius || r < 0 || (unsigned long long)r >= ix.base[d + 1] - ix.base[d]) bad = RK_EINVAL;
		uint32_t y[5] = {0u, 0u, 0u, 0u, 0u};
		bool writer = false;
		if (!bad) {
			const unsigned long long G = ix.base[d] + (unsigned long long)r;
			uint32_t lo = ((uint32_t)b.lstart[d] - 1u) >> 8, hi = min(((uint32_t)b.lstart[d + 1] - 2u) >> 8, ix.tiles - 1u);
			while (lo < hi) {                                                // the last tile of the level whose prefix is <= G
				const uint32_t mid = (lo + hi + 1u) >> 1;
				if (ix.tile[mid] <= G) lo = mid; else hi = mid - 1u;
			}
			const unsigned long long left = G - ix.tile[lo];                 // (>= 0: the level's first tile starts at or below base[d])
			const uint32_t w = ix.orbit[(size_t)lo * 64 + lane];
			const uint32_t mine = bytes_sum(w), incl = wave_inclusive_sum(mine, lane), excl = incl - mine;
			const unsigned long long holds = __ballot((unsigned long long)excl <= left && left < (unsigned long long)incl);
			if (holds == 0ull) {
				bad = RK_ESTATE;                                             // the tile's prefix and its bytes disagree
			} else {
				const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)holds) - 1);
				uint32_t bytes = (uint32_t)__builtin_amdgcn_readlane((int)w, src);
				uint32_t k = (uint32_t)left - (uint32_t)__builtin_amdgcn_readlane((int)excl, src);
				uint32_t j = lo * 256u + (uint32_t)src * 4u + 1u;
				while (k >= (bytes & 0xFFu)) {                               // (ends inside the dword: k < the sum of its bytes)
					k -= bytes & 0xFFu;
					bytes >>= 8;
					j++;
				}
				const uint32_t size = bytes & 0xFFu;
				if (j > ix.len) {
					bad = RK_ESTATE;
				} else {
					uint32_t x[5];
					load5(b.states + (size_t)j * 5, x);
					sym_conjugate(sp.s_sym, sp.L, x, y);
					bool first = lane < N_SYM;
					for (int t = 0; t < N_SYM - 1; t++) {
						bool same = true;
						#pragma unroll
						for (int q = 0; q < 5; q++) same = same && (uint32_t)__builtin_amdgcn_readlane((int)y[q], t) == y[q];
						if (same && t < lane) first = false;
					}
					const unsigned long long firsts = __ballot(first);
					if ((uint32_t)__popcll(firsts) != size) bad = RK_ESTATE;
					else writer = first && (uint32_t)__popcll(firsts & ((1ull << lane) - 1ull)) == k;
				}
			}
		}
		if (bad) {
			if (lane == 0) *error = bad;
			if (lane < 5) out[i * 5 + lane] = 0u;
		} else if (writer) {
			#pragma unroll
			for (int q = 0; q < 5; q++) out[i * 5 + q] = y[q];
		}
	}
}

// The exact depth of every state within radius + 1 of solved and of its twelve children, a wave per state: the level of the
// state and of each child in action order, then the parity of quarter turns -- a turn changes the distance by exactly one.
//   own level o in 0..R: a child the ball holds has its level, any other lies at o + 1 (with o < R the ball is broken: RK_ESTATE)
//   own state outside, a child inside: that child lies at R (anything else: RK_ESTATE), the state at R + 1, a child outside at R + 2
//   own state and all children outside: -1 for all thirteen
// Lane a < 12 keeps and writes child a.
__global__ __launch_bounds__(256)
void k_sb_child_depths(SymBallView b, const uint32_t *states, size_t n, int8_t *depth, int8_t *child, int32_t *error)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const SymProbe sp = sym_probe(s_sym, 256, s_act);
	const int lane = sp.lane, R = b.radius;
	for (size_t q = (size_t)blockIdx.x * 4 + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); q < n; q += (size_t)gridDim.x * 4) {
		uint32_t x[5];
		load5(states + q * 5, x);
		const int own = sb_level(b, sp, x);
		int mine = -1;
		for (int a = 0; a < N_ACTIONS; a++) {
			uint32_t y[5], tab[12];
			#pragma unroll
			for (int j = 0; j < 5; j++) y[j] = x[j];
			load_action_table(sp.s_act, (uint32_t)a, tab);
			move5(y, tab);
			const int lvl = sb_level(b, sp, y);
			if (lane == a) mine = lvl;
		}
		const bool inside = lane < N_ACTIONS && mine >= 0;
		const bool any = __ballot(inside) != 0ull;
		int d = own, c = mine;
		bool broken = false;
		if (own >= 0) {
			if (!inside) { c = own + 1; broken = own < R; }
		} else if (any) {
			d = R + 1;
			if (inside) broken = mine != R; else c = R + 2;
		}
		if (lane < N_ACTIONS) {
			child[q * N_ACTIONS + lane] = (int8_t)c;
			if (broken) *error = RK_ESTATE;
		}
		if (lane == 0) depth[q] = (int8_t)d;
	}
}

// ---- shortening action queues against the symmetry ball (rk_sshorten; the DP and everything ball-independent: rk_shorten_dev.h) ----
// d(i, j) of every window of every queue, at rk_ball.hip's k_shorten_windows' addresses: the byte of window (i, j) is
// depth[(p * max_len + j - 1) * window + (j - i - 1)].  A persistent grid: every workgroup stages s_act (576 B) and the symmetry
// tables (23 232 B) ONCE, then its four waves stride over the (queue, i) pairs.  A workgroup per four pairs, as in
// k_shorten_windows, would stage 23 KB again for a handful of probes -- most pairs of a padded batch have no window at all.
// Per pair the windows are composed as there: lane = offset, shorten_compose in chunks of 64 with the carried state, the next
// chunk's actions loaded ahead.  Then the chunk's states are taken one at a time: lane k's state is broadcast (five v_readlane),
// canonicalised with lane = symmetry as everywhere in this file (so the table reads bank as rk_sym_dev.h describes), its
// representative probed once, and lane k keeps the level.  The wave index goes through readfirstlane: the pair, the queue's
// length, every trip count and the broadcast lane are wave-uniform, so all 64 lanes reach every sym_canonical.
__global__ __launch_bounds__(256)
void k_ss_windows(SymBallView b, const int8_t *__restrict__ actions, const int32_t *__restrict__ len, size_t n, int max_len, int window,
                  int8_t *__restrict__ depth)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const SymProbe sp = sym_probe(s_sym, 256, s_act);
	const int lane = sp.lane;
	const size_t pairs = n * (size_t)max_len;
	for (size_t w = (size_t)blockIdx.x * 4 + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); w < pairs; w += (size_t)gridDim.x * 4) {
		const size_t p = w / (size_t)max_len;
		const int i = (int)(w - p * (size_t)max_len);
		const int L = shorten_len(len, p, max_len);
		if (i >= L) continue;
		const int8_t *row = actions + p * (size_t)max_len;
		const int moves = min(window, L - i);                                // windows (i, i + 1) .. (i, i + moves)
		uint32_t s[5] = {SOLVED_DW[0], SOLVED_DW[1], SOLVED_DW[2], SOLVED_DW[3], SOLVED_DW[4]};
		uint32_t a_next = lane < moves ? (uint32_t)(uint8_t)row[i + lane] : 0xFFu;
		for (int d0 = 0; d0 < moves; d0 += 64) {
			const int nc = min(64, moves - d0);
			const uint32_t a = a_next;
			a_next = d0 + 64 + lane < moves ? (uint32_t)(uint8_t)row[i + d0 + 64 + lane] : 0xFFu;    // behind the scan and the probes
			uint32_t st[5];
			shorten_compose(s_act, a, lane, nc, s, st);
			int mine = -1;
			for (int k = 0; k < nc; k++) {
				uint32_t x[5];
				#pragma unroll
				for (int j = 0; j < 5; j++) x[j] = (uint32_t)__builtin_amdgcn_readlane((int)st[j], k);
				const int lvl = sb_level(b, sp, x);
				if (lane == k) mine = lvl;
			}
			if (lane < nc) {
				const int k = d0 + lane;                                         // j - i - 1
				depth[(p * (size_t)max_len + (size_t)(i + k)) * (size_t)window + (size_t)k] = (int8_t)mine;
			}
			shorten_carry(st, nc, s);                                        // into the next chunk
		}
	}
}

// The rewritten queue of queue blockIdx.x: one wave, rk_ball.hip's k_shorten_emit (shorten_emit) but for the word of a replaced
// edge.  The ball keeps no parents, so X(i, j) is canonicalised and probed (its level must be the stored d), and the word is the
// INVERSE of the descent from X(i, j): sb_descend's step k, action a, is written as a ^ 1 at place d - 1 - k, which leads from
// solved to X(i, j), hence from s_i to s_j.  A failed descent or a level that differs is RK_ESTATE and the queue comes back as it
// is.  Everything is the same in every lane; lane 0 writes the replaced words.
__global__ __launch_bounds__(64)
void k_ss_emit(SymBallView b, const int8_t *__restrict__ actions, const int32_t *__restrict__ len, int max_len, int window,
               const int8_t *__restrict__ depth, const uint16_t *__restrict__ pred, int8_t *__restrict__ out_actions,
               int32_t *__restrict__ out_len, int32_t *error)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const SymProbe sp = sym_probe(s_sym, 64, s_act);
	shorten_emit(s_act, actions, len, max_len, window, depth, pred, out_actions, out_len, error, [&](uint32_t x[5], int d, int8_t *at) {
		if (sb_level(b, sp, x) != d) return false;
		bool down;
		const int steps = sb_descend(b, sp, x, d, [&](int k, int a) { if (sp.lane == 0) at[d - 1 - k] = (int8_t)(a ^ 1); }, &down);
		return down && steps == d;
	});
}

// ---- the search from a start towards the symmetry ball ----------------------------------------------------------------------
// (the bodies: what one search does in a launch, for the single engine (k_ss_*) and for one slot of a batch (kb_ss_*))
// One wave: node 1 = the start, whose representative is looked up in the ball (bsearch_root with that one difference).
__device__ __forceinline__ void ssearch_root(const FrontierDev &d, const SymBallView &b, const uint32_t *root, int budget)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	if (threadIdx.x < S_COUNT) d.ctr[threadIdx.x] = 0;
	const SymProbe sp = sym_probe(s_sym, 64);                            // (its barrier is behind the zeroed counters as well)
	uint32_t s[5];
	load5(root, s);
	const uint32_t e = sb_node(b, sp, s);
	if (sp.lane == 0) srch_root_store(d, s, budget, e);                  // (the ball holds the start's orbit: nothing is popped)
}

// hit[c] = the ball's node of the representative of child c of the batch, 0 when the ball does not hold it: waves stride over
// the children (k_sb_canon's grid), nothing but hit is written
__device__ __forceinline__ void ssearch_probe(const FrontierDev &d, const SymBallView &b, uint32_t *hit)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const int K = 12 * fr_pops(d);
	if ((int)blockIdx.x * 4 >= K) return;                                // done, or a workgroup past the batch: nothing staged
	const SymProbe sp = sym_probe(s_sym, 256, s_act);
	const int32_t head = d.ctr[F_HEAD];
	for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < K; c += gridDim.x * 4) {       // (whole waves)
		const int i = c / 12, a = c - 12 * i;
		uint32_t x[5];
		child_state(d.states, head + i, s_act, (uint32_t)a, x);
		const uint32_t e = sb_node(b, sp, x);
		if (sp.lane == 0) hit[c] = e;
	}
}

// a meeting child leaves no claim; any other: membership / election in the own table on the raw child (bsearch_expand)
__device__ __forceinline__ void ssearch_expand(const FrontierDev &d, const uint32_t *hit)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int P = fr_pops(d);
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= 12 * P) return;
	const uint32_t m = hit[c];
	if (m != 0u) { srch_meet(d, c, m); return; }
	const int32_t head = d.ctr[F_HEAD];
	const int i = c / 12, a = c - 12 * i;
	uint32_t s[5];
	child_state(d.states, head + i, s_act, (uint32_t)a, s);
	srch_claim(d, s_act, head, c, s);
}

// The action queue of a won search, one wave: the path from the start to the popped parent and the meeting action (none of either
// when the ball holds the start's orbit), then the descent from the meeting state.  out[0] = length, -1 when the search has not
// met or a parent chain is broken, -2 when the meeting state is not where S_MEET says or the descent finds no way on.  Every lane
// computes the same; lane 0 writes.
__device__ __forceinline__ void ssearch_walk(const FrontierDev &d, const SymBallView &b, int32_t *out, int max_len)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const SymProbe sp = sym_probe(s_sym, 64, s_act);
	const int lane = sp.lane;
	if (lane == 0) out[0] = -1;
	if (!d.ctr[F_WON]) return;
	const int p = d.ctr[F_WPARENT];
	int len = p != 0 ? fr_walk_up(d, p, out + 1, max_len, lane == 0) : 0;
	if (len < 0) return;
	uint32_t x[5];
	if (p != 0) {
		const int a = d.ctr[F_WACT];
		if ((uint32_t)a >= (uint32_t)N_ACTIONS) return;
		if (len < max_len && lane == 0) out[1 + len] = a;
		len++;
		child_state(d.states, p, s_act, (uint32_t)a, x);
	} else {
		load5(d.states + 5, x);
	}
	const uint32_t g = sb_node(b, sp, x);
	bool ok = g != 0u && g == (uint32_t)d.ctr[S_MEET];
	const int own = len;                                                 // moves before the meeting state
	if (ok) len = own + sb_descend(b, sp, x, level_of(b.lstart, g), [&](int k, int a) { if (own + k < max_len && lane == 0) out[1 + own + k] = a; }, &ok);
	if (lane == 0) out[0] = ok ? len : -2;
}

// ---- the single engine: one search per launch (scan, append, end and rehash: rk_frontier_dev.h's k_fr_*, k_srch_end) ----
__global__ __launch_bounds__(64)
void k_ss_root(FrontierDev d, SymBallView b, const uint32_t *root, int budget) { ssearch_root(d, b, root, budget); }

__global__ __launch_bounds__(256)
void k_ss_probe(FrontierDev d, SymBallView b, uint32_t *hit) { ssearch_probe(d, b, hit); }

__global__ __launch_bounds__(256)
void k_ss_expand(FrontierDev d, const uint32_t *hit) { ssearch_expand(d, hit); }

__global__ __launch_bounds__(64)
void k_ss_walk(FrontierDev d, SymBallView b, int32_t *out, int max_len) { ssearch_walk(d, b, out, max_len); }

// ---- deepening: words from a state, every result probed (rk_deepen_dev.h) ----
__global__ __launch_bounds__(256)
void k_sd_probe(SymBallView b, DeepenJob job, uint32_t *best)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	deepen_probe(b, job, sym_probe(s_sym, 256, s_act), (size_t)blockIdx.x * 4 + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), (size_t)gridDim.x * 4,
	             DeepenRanks{best});
}

// k_sd_probe with the words that an admissible bound rules out left unprobed (rk_deepen_dev.h: PdbPrune): the same `best`
__global__ __launch_bounds__(256)
void k_sd_probe_pruned(SymBallView b, DeepenJob job, uint32_t *best, PdbBound bound, unsigned long long *lookups)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	deepen_probe(b, job, sym_probe(s_sym, 256, s_act), (size_t)blockIdx.x * 4 + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), (size_t)gridDim.x * 4,
	             DeepenRanks{best}, PdbPrune{bound, b.radius, lookups});
}

// the pops of the iterations to come; results do not depend on them.  One thread.
__global__ void k_ss_setpops(FrontierDev d)
{
	if (threadIdx.x != 0 || blockIdx.x != 0 || d.ctr[F_DONE]) return;
	d.ctr[F_NPOP] = min(d.pops, d.ctr[S_HI] - d.ctr[F_HEAD] + 1);
}

// The queue start -> `node` -> word `rank` of `extra` moves -> descent, one wave, as ssearch_walk: out[0] = length, -1 when the
// parent chain is broken or the node has no such word, -2 when the ball does not hold the moved state's representative or the
// descent finds no way on.  Every lane computes the same; lane 0 writes.
__device__ __forceinline__ void ssearch_deepen_walk(const FrontierDev &d, const SymBallView &b, int node, int extra, uint32_t rank, int32_t *out, int max_len)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const SymProbe sp = sym_probe(s_sym, 64, s_act);
	const int lane = sp.lane;
	if (lane == 0) out[0] = -1;
	const int ls = fr_walk_up(d, node, out + 1, max_len, lane == 0);
	if (ls < 0) return;
	int word[DEEPEN_MAX_EXTRA];
	if (!deepen_word(extra, node == 1 ? -1 : deepen_last(d.pact[node] & PACT_ACTION), rank, word)) return;
	uint32_t x[5];
	load5(d.states + (size_t)node * 5, x);
	int len = ls;
	for (int k = 0; k < extra; k++, len++) {
		if (len < max_len && lane == 0) out[1 + len] = word[k];
		uint32_t y[5];
		deepen_move(s_act, word[k], x, y);
		#pragma unroll
		for (int j = 0; j < 5; j++) x[j] = y[j];
	}
	const uint32_t g = sb_node(b, sp, x);
	bool ok = g != 0u;
	const int own = len;
	if (ok) len = own + sb_descend(b, sp, x, level_of(b.lstart, g), [&](int k, int a) { if (own + k < max_len && lane == 0) out[1 + own + k] = a; }, &ok);
	if (lane == 0) out[0] = ok ? len : -2;
}

__global__ __launch_bounds__(64)
void k_ss_deepen_walk(FrontierDev d, SymBallView b, int node, int extra, uint32_t rank, int32_t *out, int max_len)
{
	ssearch_deepen_walk(d, b, node, extra, rank, out, max_len);
}

// ---- the batch: S searches in lock-step, slot blockIdx.y of `devs` per workgroup row (rk_ball.hip: kb_bsearch_*) ----
// Every slot is a whole search of its own -- pool, table, counters, batch scratch, look-back words, ticket, epoch and the 12 P
// words of `hit` --, so a launch reads and writes through devs[blockIdx.y] and that slot's slice of `hits` alone; the ball is read
// by all.  A slot that is done, or was never started, has F_NPOP == 0: it leaves at that read, draws no ticket and leaves its
// epoch alone.  The pool-full rule is the plain batch's (rk_frontier_dev.h: srch_fit), so fr_pops() of a slot with P > 0 is P; the
// clear, scan, append and end of all slots are the plain batch's too (kb_srch_*).

// row j of roots / budgets starts slot slots[j]: one wave per named slot
__global__ __launch_bounds__(64)
void kb_ss_root(const FrontierDev *devs, SymBallView b, const int32_t *slots, const uint32_t *roots, const int32_t *budgets, int clip)
{
	const FrontierDev d = devs[slots[blockIdx.y]];
	ssearch_root(d, b, roots + (size_t)blockIdx.y * 5, budgets[blockIdx.y]);
	if (threadIdx.x == 0) {                                              // (the thread that wrote the counters)
		d.ctr[S_CLIP] = clip;                                            // the pool-full rule of this search: srch_fit
		srch_fit(d);
	}
}

// slot blockIdx.y's children, its waves striding over them; a workgroup whose first child is past the slot's batch -- a slot that
// is done, never started, or has a short batch -- returns before the tables are staged (ssearch_probe's first lines)
__global__ __launch_bounds__(256)
void kb_ss_probe(const FrontierDev *devs, SymBallView b, uint32_t *hits)
{
	const FrontierDev d = devs[blockIdx.y];
	ssearch_probe(d, b, hits + (size_t)blockIdx.y * 12u * (size_t)d.pops);
}

__global__ __launch_bounds__(256)
void kb_ss_expand(const FrontierDev *devs, const uint32_t *hits)
{
	const FrontierDev d = devs[blockIdx.y];
	if (blockIdx.x * 256 >= 12 * d.ctr[F_NPOP]) return;                  // done, never started, or a workgroup past the batch
	ssearch_expand(d, hits + (size_t)blockIdx.y * 12u * (size_t)d.pops);
}

// one WAVE per slot (the descent needs lane = symmetry): row s of `out` (n_slots, 1 + max_len) = length, -1 or -2, then the queue
__global__ __launch_bounds__(64)
void kb_ss_walk(const FrontierDev *devs, SymBallView b, int32_t *out, int max_len)
{
	const FrontierDev d = devs[blockIdx.x];
	ssearch_walk(d, b, out + (size_t)blockIdx.x * (size_t)(1 + max_len), max_len);
}

// ---- deepening in the batch: slots whose pool is full go on by probes, all of them in one launch ----
// A job as the device reads it (rk_deepen_job_t after the host's checks).  For the probe launch: the nodes node_first ..
// node_first + node_count - 1 of slot `slot`'s pool, the words word_first .. word_first + word_count - 1 of `extra` moves, and
// the slot's key keys[key_at]; for the walk: node_first = the node, word_first = the rank.
struct SlotDeepenJob {
	int32_t slot, extra;
	uint32_t node_first, node_count, word_first, word_count, key_at, unused;
};

// Job blockIdx.y, its waves striding over the job's items as k_sd_probe's do over theirs: the same body (deepen_probe) on the rows
// of the slot's pool, the stored action as the last move, none for node 1.  What is kept is the slot's key (DeepenKey).  A slot
// has two keys and a job names the one of its round; the other is set to "none" here, where no launch of this round reads or
// lowers it, so the round that follows finds it cleared.  A workgroup past the job's items returns before the tables are staged.
// Nothing of a pool or of the ball is written.
__global__ __launch_bounds__(256)
void kb_sd_probe(const FrontierDev *devs, SymBallView b, const SlotDeepenJob *jobs, unsigned long long *keys)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const SlotDeepenJob j = jobs[blockIdx.y];
	if (blockIdx.x == 0 && threadIdx.x == 0) keys[j.key_at ^ 1u] = DEEPEN_NO_KEY;
	if ((size_t)blockIdx.x * 4 >= (size_t)j.node_count * deepen_groups(j.extra, j.word_first, j.word_count)) return;
	const FrontierDev d = devs[j.slot];
	const DeepenJob job{d.states + (size_t)j.node_first * 5, reinterpret_cast<const int8_t *>(d.pact) + j.node_first, 1 - (long long)j.node_first,
	                    j.node_count, j.extra, j.word_first, j.word_count};
	deepen_probe(b, job, sym_probe(s_sym, 256, s_act), (size_t)blockIdx.x * 4 + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), (size_t)gridDim.x * 4,
	             DeepenKey{keys + j.key_at, j.node_first});
}

// one wave per job: row blockIdx.x of `out` (n, 1 + max_len) = ssearch_deepen_walk of the job's slot, node, extra and rank
__global__ __launch_bounds__(64)
void kb_ss_deepen_walk(const FrontierDev *devs, SymBallView b, const SlotDeepenJob *jobs, int32_t *out, int max_len)
{
	const SlotDeepenJob j = jobs[blockIdx.x];
	ssearch_deepen_walk(devs[j.slot], b, (int)j.node_first, j.extra, j.word_first, out + (size_t)blockIdx.x * (size_t)(1 + max_len), max_len);
}

__global__ __launch_bounds__(256)
void k_sym_canonical(const uint32_t *states, size_t n, uint32_t *rep_out, uint8_t *sym_out, uint8_t *orbit_out)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	const SymProbe sp = sym_probe(s_sym, 256);
	const int lane = sp.lane;
	for (size_t q = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (size_t)gridDim.x * 4) {
		uint32_t x[5], rep[5];
		load5(states + q * 5, x);
		int sym, count;
		sym_canonical(s_sym, sp.L, lane, x, rep, &sym, &count);
		if (rep_out != nullptr && lane < 5) rep_out[q * 5 + lane] = dword_of(rep, lane);
		if (sym_out != nullptr && lane == 5) sym_out[q] = (uint8_t)sym;
		if (orbit_out != nullptr && lane == 6) orbit_out[q] = (uint8_t)(N_SYM / count);
	}
}

__global__ __launch_bounds__(256)
void k_sym_conjugate(const uint32_t *states, size_t n, int sym, uint32_t *out)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	sym_stage(s_sym, threadIdx.x, 256);
	__syncthreads();
	const SymLane L = sym_lane(sym);
	for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
		uint32_t x[5], y[5];
		load5(states + q * 5, x);
		sym_conjugate(s_sym, L, x, y);
		#pragma unroll
		for (int j = 0; j < 5; j++) out[q * 5 + j] = y[j];
	}
}

}  // namespace rk

using namespace rk;

struct rk_symball : KeptBall {
	SymBallDev d{};
	SymBallView view{};
	long long cover[SB_MAX_RADIUS + 1] = {};
	// the orbit index of rk_symball_state_at: made at its first call, in the ball's pool (so it goes with the ball)
	SymIndex index{};
	uint8_t *orbit = nullptr; unsigned long long *tile = nullptr;
	long long index_builds = 0, index_bytes = 0;
};

// What an engine of another translation unit that ends at a built symmetry ball takes and gives back (rk_beam.hip; declared in
// rk_sym_dev.h): the view by value and a count in `attached`, so that rk_symball_destroy refuses under it as under a search here.
namespace rk {

int symball_attach(rk_symball *ball, const char *who, SymBallView *view)
{
	if (!ball || !view) return fail(RK_EINVAL, "%s: null ball", who);
	if (!ball->built) return fail(RK_ESTATE, "%s: build the ball first", who);
	ball->attached += 1;
	*view = ball->view;
	return RK_OK;
}

void symball_detach(rk_symball *ball)
{
	if (ball) ball->attached -= 1;
}

}  // namespace rk

struct rk_ssearch : FrontierPool, BallReader<rk_symball> {
	uint32_t *hit = nullptr;                    // per child of the batch: the ball's node of its representative, or 0
	int pops_made = 0;                          // what it was created with: rk_sdeepen_set_pops lowers d.pops, a reset restores it
};

// S searches in lock-step: the slots (rk_frontier_host.h: FrontierSlots), their `hit` block and the ball they all read
struct rk_ssearchb : FrontierSlots, BallReader<rk_symball> {
	// what the host knows of a slot between a rk_sdeepenb_frontiers and the slot's next reset
	struct Front {
		int32_t lo = 0, hi = 0, size = 0;       // the newest complete level and the states stored
		bool stopped = false;                   // the slot was done at that read: its pool and its level stand still
		bool round_open = false;                // a job with new_round has chosen the slot's key since
	};
	uint32_t *hit = nullptr;                    // (n_slots, 12 x pops): slot s's words are its own
	bool clip = false;                          // rk_sdeepenb_set: the pool-full rule of the resets to come
	unsigned long long *keys = nullptr;         // (n_slots, 2): a slot's key of this round and the cleared one of the next
	SlotDeepenJob *jobs_dev = nullptr;          // (n_slots): the jobs of the launch in flight
	std::vector<SlotDeepenJob> jobs_host;       // what the copy to jobs_dev reads: left alone until jobs_sent has passed
	hipEvent_t jobs_sent = nullptr;
	std::vector<Front> front;
	std::vector<uint8_t> key_of;                // per slot: which of its two keys the current round lowers

	~rk_ssearchb() { if (jobs_sent != nullptr) (void)hipEventDestroy(jobs_sent); }

	// `jobs` to the device block, behind whatever the stream holds; the host copy of the launch before is no longer read by then
	int send_jobs(std::vector<SlotDeepenJob> &jobs, hipStream_t st)
	{
		RK_HIP(hipEventSynchronize(jobs_sent));
		jobs_host.swap(jobs);
		RK_HIP(hipMemcpyAsync(jobs_dev, jobs_host.data(), jobs_host.size() * sizeof(SlotDeepenJob), hipMemcpyHostToDevice, st));
		RK_HIP(hipEventRecord(jobs_sent, st));
		return RK_OK;
	}
};

namespace {

constexpr size_t SB_MAX_CAPACITY = 0x3FFFFFF0ull;
constexpr unsigned SYM_GRID = 2048;              // workgroups of the wave-per-state launches: eight to a CU, the tables staged once each

long long sb_level_size(int l) { return l <= BALL_CHECKED ? BALL_LEVELS[l] : SB_LEVELS_UNCHECKED[l - BALL_CHECKED - 1]; }

// the sum over the levels of ceil(level / 48 * 1.02) + 64
size_t sb_default_capacity(int radius)
{
	size_t n = 0;
	for (int l = 0; l <= radius; l++) n += (size_t)((sb_level_size(l) * 102 + 4799) / 4800) + 64;
	return n;
}

unsigned sym_grid(size_t waves) { return std::min(blocks(waves, 4), SYM_GRID); }

// the range checks of a deepening launch and the launch itself; `bound` (null: every word is looked up) prunes, `lookups` counts
int launch_deepen(const char *who, rk_symball *ball, DeepenJob job, uint32_t *best, hipStream_t st, const rk_bound *bound = nullptr,
                  unsigned long long *lookups = nullptr)
{
	if ((uintptr_t)lookups & 7u) return fail(RK_EINVAL, "%s: d_lookups must be an 8-byte aligned device pointer", who);
	if (job.extra < 1 || job.extra > DEEPEN_MAX_EXTRA) return fail(RK_EINVAL, "%s: extra %d outside 1..%d", who, job.extra, DEEPEN_MAX_EXTRA);
	if ((unsigned long long)job.n * job.word_count > DEEPEN_MAX_PROBES)
		return fail(RK_EINVAL, "%s: %zu states x %u words are more than the %llu probes of one launch", who, job.n, job.word_count, DEEPEN_MAX_PROBES);
	if (!best || ((uintptr_t)best & 3u)) return fail(RK_EINVAL, "%s: d_best must be a 4-byte aligned device pointer", who);
	const unsigned long long all = deepen_words(job.extra, -1);
	if (job.n == 0 || job.word_count == 0 || job.word_first >= all) return RK_OK;
	job.word_count = (uint32_t)std::min<unsigned long long>(job.word_count, all - job.word_first);
	const size_t items = job.n * (size_t)deepen_groups(job.extra, job.word_first, job.word_count);
	if (bound != nullptr)
		hipLaunchKernelGGL(k_sd_probe_pruned, dim3(sym_grid(items)), dim3(256), 0, st, ball->view, job, best, bound->b, lookups);
	else
		hipLaunchKernelGGL(k_sd_probe, dim3(sym_grid(items)), dim3(256), 0, st, ball->view, job, best);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

// The orbit index of a built ball, made once: the orbit bytes, the tiles' counts, their prefix and the level bases -- four launches
// and one read -- then the check that every level's orbit sizes add up to what the ball's own build reported.  Synchronises when
// it builds; a ball that has its index returns at once.  Whatever fails leaves the ball without an index.
int ensure_index(const char *who, rk_symball *h, hipStream_t st)
{
	if (h->orbit != nullptr) return RK_OK;
	const uint32_t len = (uint32_t)h->size, tiles = blocks(len, 256);
	const int levels = h->d.radius + 2;
	uint8_t *orbit = nullptr;
	unsigned long long *tile = nullptr, *base = nullptr;
	int32_t *error = nullptr;
	const auto drop = [&] {
		for (void *p : {(void *)orbit, (void *)tile, (void *)base, (void *)error}) h->pool.release(p);
	};
	int e = h->pool.alloc(&orbit, (size_t)tiles * 256);
	if (!e) e = h->pool.alloc(&tile, (size_t)tiles + 1);
	if (!e) e = h->pool.alloc(&base, (size_t)SB_MAX_RADIUS + 2);
	if (!e) e = h->pool.alloc(&error, 1);
	if (e) {
		(void)hipGetLastError();
		drop();
		return fail(RK_ECAPACITY, "%s: no device memory for the orbit index of %u orbits", who, len);
	}
	unsigned long long sums[SB_MAX_RADIUS + 2] = {};
	int32_t err = 0;
	const hipError_t he = [&]() -> hipError_t {
		RK_FILL(hipMemsetAsync(orbit, 0, (size_t)tiles * 256, st));
		RK_FILL(hipMemsetAsync(error, 0, sizeof(int32_t), st));
		hipLaunchKernelGGL(k_sb_orbit, dim3(sym_grid(len)), dim3(256), 0, st, h->view, len, orbit, error);
		hipLaunchKernelGGL(k_sb_orbit_count, dim3(blocks(tiles, 4)), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(orbit), tiles, tile);
		hipLaunchKernelGGL(k_sb_orbit_scan, dim3(1), dim3(SB_SCAN_THREADS), 0, st, tile, tiles);
		hipLaunchKernelGGL(k_sb_orbit_base, dim3(1), dim3(64), 0, st, h->view, orbit, tile, base);
		RK_FILL(hipGetLastError());
		RK_FILL(hipMemcpyAsync(sums, base, (size_t)levels * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		RK_FILL(hipMemcpyAsync(&err, error, sizeof err, hipMemcpyDeviceToHost, st));
		return hipStreamSynchronize(st);
	}();
	if (he != hipSuccess) {
		(void)hipStreamSynchronize(st);
		drop();
		return fail(RK_EHIP, "%s: the orbit index: %s", who, hipGetErrorString(he));
	}
	int wrong = -1;
	for (int l = h->d.radius; l >= 0; l--)
		if ((long long)(sums[l + 1] - sums[l]) != h->cover[l]) wrong = l;
	if (err || sums[0] != 0ull || wrong >= 0) {
		drop();
		if (err) return fail(RK_ESTATE, "%s: a node of the ball is not the canonical form of its orbit", who);
		return fail(RK_ESTATE, "%s: the orbit sizes of level %d add up to %llu in the index, the build reported %lld", who, std::max(wrong, 0),
		            sums[std::max(wrong, 0) + 1] - sums[std::max(wrong, 0)], h->cover[std::max(wrong, 0)]);
	}
	h->pool.release(base);
	h->pool.release(error);
	h->orbit = orbit;
	h->tile = tile;
	h->index = SymIndex{reinterpret_cast<const uint32_t *>(orbit), tile, tiles, len, {}};
	for (int l = 0; l < levels; l++) h->index.base[l] = sums[l];
	h->index_builds += 1;
	h->index_bytes = (long long)tiles * 256 + (long long)(tiles + 1) * (long long)sizeof(unsigned long long);
	return RK_OK;
}

}  // namespace

extern "C" {

int rk_sym_tables(uint8_t *h_actions, uint8_t *h_src, uint8_t *h_map)
{
	if (!h_actions && !h_src && !h_map) return fail(RK_EINVAL, "rk_sym_tables: null output");
	if (h_actions) memcpy(h_actions, SYM_TABLES.act, sizeof SYM_TABLES.act);
	if (h_src) memcpy(h_src, SYM_TABLES.src, sizeof SYM_TABLES.src);
	if (h_map) memcpy(h_map, SYM_TABLES.map, sizeof SYM_TABLES.map);
	return RK_OK;
}

int rk_sym_canonical(const int8_t *d_states, size_t n, int8_t *d_rep, uint8_t *d_sym, uint8_t *d_orbit, void *stream)
{
	if (int e = check_state_rows("rk_sym_canonical", d_states, n)) return e;
	if ((uintptr_t)d_rep & 3u) return fail(RK_EINVAL, "rk_sym_canonical: device pointers must be 4-byte aligned");
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_sym_canonical, dim3(sym_grid(n)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(d_states), n,
	                   reinterpret_cast<uint32_t *>(d_rep), d_sym, d_orbit);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_sym_conjugate(const int8_t *d_states, size_t n, int sym, int8_t *d_out, void *stream)
{
	if (sym < 0 || sym >= N_SYM) return fail(RK_EINVAL, "rk_sym_conjugate: symmetry %d outside 0..%d", sym, N_SYM - 1);
	if (int e = check_state_rows("rk_sym_conjugate", d_states, n)) return e;
	if (n != 0 && !d_out) return fail(RK_EINVAL, "rk_sym_conjugate: null pointer");
	if ((uintptr_t)d_out & 3u) return fail(RK_EINVAL, "rk_sym_conjugate: device pointers must be 4-byte aligned");
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_sym_conjugate, dim3(std::min(blocks(n), SYM_GRID)), dim3(256), 0, (hipStream_t)stream,
	                   reinterpret_cast<const uint32_t *>(d_states), n, sym, reinterpret_cast<uint32_t *>(d_out));
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_symball_create(rk_symball_t **out, int radius, int pops, size_t capacity)
{
	if (int e = KeptBall::check_create("rk_symball_create", out, radius, SB_MAX_RADIUS, pops)) return e;
	if (capacity == 0) capacity = sb_default_capacity(radius);
	if (capacity > SB_MAX_CAPACITY) return fail(RK_EINVAL, "rk_symball_create: capacity %zu out of range", capacity);
	rk_symball *h = new rk_symball();
	h->describe(h->d, capacity, radius, pops);
	*out = h;
	return RK_OK;
}

int rk_symball_destroy(rk_symball_t *h)
{
	if (int e = KeptBall::check_destroy("rk_symball_destroy", h)) return e;
	delete h;
	return RK_OK;
}

int rk_symball_build(rk_symball_t *h, int poll, void *stream)
{
	if (int e = KeptBall::check_build("rk_symball_build", h, poll)) return e;
	if (h->built) return RK_OK;
	hipStream_t st = (hipStream_t)stream;
	SymBallDev &d = h->d;
	const size_t K = (size_t)12 * d.pops;
	const unsigned grid = blocks(K);
	int32_t c[BB_COUNT];
	if (int e = h->run_build("rk_symball_build", "orbits", d, poll, st, c,
	                         [&] {
		                         int e = h->pool.alloc(&d.cover, SB_MAX_RADIUS + 1);
		                         if (!e) e = h->pool.alloc(&d.cstate, K * 5);
		                         return e ? e : h->pool.alloc(&d.corbit, K);
	                         },
	                         [&] { hipLaunchKernelGGL(k_sb_root, dim3(1), dim3(64), 0, st, d); },
	                         [&] {
		                         hipLaunchKernelGGL(k_sb_canon, dim3(sym_grid(K)), dim3(256), 0, st, d);
		                         hipLaunchKernelGGL(k_sb_expand, dim3(grid), dim3(256), 0, st, d);
		                         hipLaunchKernelGGL(k_sb_scan, dim3(blocks(K, ASCAN)), dim3(ASCAN), 0, st, d);
		                         hipLaunchKernelGGL(k_sb_append, dim3(grid), dim3(256), 0, st, d);
		                         hipLaunchKernelGGL(k_sb_end, dim3(1), dim3(64), 0, st, d);
	                         }))
		return e;
	unsigned long long cover[SB_MAX_RADIUS + 1];
	RK_HIP(hipMemcpyAsync(cover, d.cover, sizeof cover, hipMemcpyDeviceToHost, st));
	RK_HIP(hipStreamSynchronize(st));
	if (c[BB_STOP] != BB_STOP_BUILT || c[BB_ERROR]) {                    // the ball stays unbuilt and says how far it came; its arrays go at once
		h->size = c[BB_SIZE];
		h->iterations = c[BB_ITERS];
		h->pool.clear(); d.states = nullptr; d.table = nullptr;
		if (c[BB_STOP] == BB_STOP_FULL)
			return fail(RK_ECAPACITY, "rk_symball_build: a capacity of %zu orbits is too small for radius %d: %d orbits stored, level %d complete", h->cap,
			            d.radius, c[BB_SIZE], c[BB_LEVEL]);
		return fail(RK_ESTATE, "rk_symball_build: engine error %d: %d orbits after level %d, whose orbit sizes add up to %llu", c[BB_ERROR], c[BB_SIZE],
		            c[BB_LEVEL], cover[std::min(std::max(c[BB_LEVEL], 0), SB_MAX_RADIUS)]);
	}
	h->finish_build(d, c, h->view, d.cstate, d.corbit);
	for (int l = 0; l <= SB_MAX_RADIUS; l++) h->cover[l] = l <= d.radius ? (long long)cover[l] : 0;
	return RK_OK;
}

int rk_symball_status(rk_symball_t *h, long long *h_status)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_symball_status: null argument");
	h->status_words(h_status, h->d.radius, h->view.lstart);
	h_status[5] = (long long)h->d.mask + 1;
	for (int l = 0; l <= SB_MAX_RADIUS; l++) h_status[18 + l] = h->built ? h->cover[l] : 0;
	for (int k = 29; k < 32; k++) h_status[k] = 0;
	return RK_OK;
}

int rk_symball_export(rk_symball_t *h, size_t first, size_t count, int8_t *h_states, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_symball_export: null ball");
	if (!h->built) return fail(RK_ESTATE, "rk_symball_export: build the ball first");
	if (first + count > (size_t)h->size + 1) return fail(RK_EINVAL, "rk_symball_export: rows %zu..%zu outside the pool", first, first + count);
	if (count == 0) return RK_OK;
	if (!h_states) return fail(RK_EINVAL, "rk_symball_export: null pointer");
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemcpyAsync(h_states, h->d.states + first * 5, count * STATE_BYTES, hipMemcpyDeviceToHost, st));
	RK_HIP(hipStreamSynchronize(st));
	return RK_OK;
}

int rk_symball_depth(rk_symball_t *h, const int8_t *d_states, size_t n, int32_t *d_depth, void *stream)
{
	if (int e = KeptBall::check_queries("rk_symball_depth", "states", h, d_states, n, d_depth)) return e;
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_sb_depth, dim3(sym_grid(n)), dim3(256), 0, (hipStream_t)stream, h->view, reinterpret_cast<const uint32_t *>(d_states), n,
	                   d_depth);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_symball_solve(rk_symball_t *h, const int8_t *d_states, size_t n, int32_t *d_lengths, int8_t *d_actions, int32_t *d_error, void *stream)
{
	if (int e = KeptBall::check_queries("rk_symball_solve", "states", h, d_states, n, d_lengths)) return e;
	if (!d_error || ((uintptr_t)d_error & 3u)) return fail(RK_EINVAL, "rk_symball_solve: the error word must be a 4-byte aligned device pointer");
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemsetAsync(d_error, 0, sizeof(int32_t), st));
	if (n == 0) return RK_OK;
	if (!d_actions && h->d.radius > 0) return fail(RK_EINVAL, "rk_symball_solve: null pointer");
	hipLaunchKernelGGL(k_sb_solve, dim3(sym_grid(n)), dim3(256), 0, st, h->view, reinterpret_cast<const uint32_t *>(d_states), n, d_lengths,
	                   d_actions, d_error);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

long long rk_symball_child_values_scratch_bytes(size_t m12)
{
	if (m12 > (size_t)INT32_MAX) return fail(RK_EINVAL, "rk_symball_child_values_scratch_bytes: %zu children in one call", m12);
	return (long long)blocks(m12, ASCAN) * (long long)sizeof(int32_t);
}

int rk_symball_child_values(rk_symball_t *h, const int8_t *d_states, size_t m12, float g, int8_t *d_depth, float *d_values, int32_t *d_rows,
                            int8_t *d_outside, int32_t *d_count, void *d_scratch, size_t scratch_bytes, void *stream)
{
	const char *who = "rk_symball_child_values";
	if (!h) return fail(RK_EINVAL, "%s: null ball", who);
	if (!h->built) return fail(RK_ESTATE, "%s: build the ball first", who);
	if (m12 > (size_t)INT32_MAX) return fail(RK_EINVAL, "%s: %zu children in one call", who, m12);
	if (m12 % N_ACTIONS) return fail(RK_EINVAL, "%s: %zu children are not twelve per state", who, m12);
	if (!d_count) return fail(RK_EINVAL, "%s: null pointer", who);
	if (m12 != 0 && (!d_states || !d_depth || !d_values || !d_rows || !d_outside || !d_scratch)) return fail(RK_EINVAL, "%s: null pointer", who);
	if (((uintptr_t)d_states | (uintptr_t)d_values | (uintptr_t)d_rows | (uintptr_t)d_outside | (uintptr_t)d_count | (uintptr_t)d_scratch) & 3u)
		return fail(RK_EINVAL, "%s: device pointers must be 4-byte aligned", who);
	const unsigned tiles = blocks(m12, ASCAN);
	if (scratch_bytes < (size_t)tiles * sizeof(int32_t))
		return fail(RK_EINVAL, "%s: %zu bytes of scratch, %zu needed", who, scratch_bytes, (size_t)tiles * sizeof(int32_t));
	hipStream_t st = (hipStream_t)stream;
	if (m12 == 0) {
		RK_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st));
		return RK_OK;
	}
	const uint32_t *states = reinterpret_cast<const uint32_t *>(d_states);
	int32_t *tile = static_cast<int32_t *>(d_scratch);
	hipLaunchKernelGGL(k_sb_child_values, dim3(sym_grid(m12)), dim3(256), 0, st, h->view, states, m12, g, d_depth, d_values);
	hipLaunchKernelGGL(k_sb_outside_count, dim3(tiles), dim3(ASCAN), 0, st, d_depth, m12, tile);
	hipLaunchKernelGGL(k_sb_outside_scan, dim3(1), dim3(SB_SCAN_THREADS), 0, st, tile, (int)tiles, d_count);
	hipLaunchKernelGGL(k_sb_outside_write, dim3(tiles), dim3(ASCAN), 0, st, d_depth, states, m12, tile, d_rows, reinterpret_cast<uint32_t *>(d_outside));
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_symball_state_at(rk_symball_t *h, const int32_t *d_depth, const int64_t *d_rank, size_t n, int8_t *d_states, int32_t *d_error, void *stream)
{
	const char *who = "rk_symball_state_at";
	if (!h) return fail(RK_EINVAL, "%s: null ball", who);
	if (!h->built) return fail(RK_ESTATE, "%s: build the ball first", who);
	if (n > (size_t)INT32_MAX) return fail(RK_EINVAL, "%s: %zu samples in one launch", who, n);
	if (!d_error || (n != 0 && (!d_depth || !d_rank || !d_states))) return fail(RK_EINVAL, "%s: null pointer", who);
	if ((((uintptr_t)d_depth | (uintptr_t)d_states | (uintptr_t)d_error) & 3u) || ((uintptr_t)d_rank & 7u))
		return fail(RK_EINVAL, "%s: device pointers must be 4-byte aligned, the ranks 8-byte", who);
	hipStream_t st = (hipStream_t)stream;
	if (int e = ensure_index(who, h, st)) return e;
	RK_HIP(hipMemsetAsync(d_error, 0, sizeof(int32_t), st));
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_sb_state_at, dim3(sym_grid(n)), dim3(256), 0, st, h->view, h->index, d_depth, reinterpret_cast<const long long *>(d_rank), n,
	                   reinterpret_cast<uint32_t *>(d_states), d_error);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_symball_index_status(rk_symball_t *h, long long *h_status)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_symball_index_status: null argument");
	const bool made = h->orbit != nullptr;
	h_status[0] = h->index_builds;
	h_status[1] = made ? h->index_bytes : 0;
	h_status[2] = made ? (long long)h->index.tiles : 0;
	h_status[3] = 0;
	for (int l = 0; l < SB_MAX_RADIUS + 2; l++) h_status[4 + l] = made && l <= h->d.radius + 1 ? (long long)h->index.base[l] : 0;
	return RK_OK;
}

int rk_symball_child_depths(rk_symball_t *h, const int8_t *d_states, size_t n, int8_t *d_depth, int8_t *d_child, int32_t *d_error, void *stream)
{
	const char *who = "rk_symball_child_depths";
	if (int e = KeptBall::check_queries(who, "states", h, d_states, n, d_depth)) return e;
	if (n != 0 && !d_child) return fail(RK_EINVAL, "%s: null pointer", who);
	if (!d_error || ((uintptr_t)d_error & 3u)) return fail(RK_EINVAL, "%s: the error word must be a 4-byte aligned device pointer", who);
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemsetAsync(d_error, 0, sizeof(int32_t), st));
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_sb_child_depths, dim3(sym_grid(n)), dim3(256), 0, st, h->view, reinterpret_cast<const uint32_t *>(d_states), n, d_depth, d_child,
	                   d_error);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

long long rk_sdeepen_max_probes(void) { return (long long)DEEPEN_MAX_PROBES; }

// rk_sdeepen and rk_sdeepen_pruned (`bound` null: the former)
static int sdeepen_states(const char *who, rk_symball *ball, const rk_bound *bound, const int8_t *d_states, const int8_t *d_last, size_t n, int extra,
                          uint32_t word_first, uint32_t word_count, uint32_t *d_best, unsigned long long *d_lookups, void *stream)
{
	if (!ball) return fail(RK_EINVAL, "%s: null ball", who);
	if (!ball->built) return fail(RK_ESTATE, "%s: build the ball first", who);
	if (int e = check_state_rows(who, d_states, n)) return e;
	return launch_deepen(who, ball, DeepenJob{reinterpret_cast<const uint32_t *>(d_states), d_last, -1, n, extra, word_first, word_count}, d_best,
	                     (hipStream_t)stream, bound, d_lookups);
}

int rk_sdeepen(rk_symball_t *ball, const int8_t *d_states, const int8_t *d_last, size_t n, int extra, uint32_t word_first, uint32_t word_count,
               uint32_t *d_best, void *stream)
{
	return sdeepen_states("rk_sdeepen", ball, nullptr, d_states, d_last, n, extra, word_first, word_count, d_best, nullptr, stream);
}

int rk_sdeepen_pruned(rk_symball_t *ball, rk_bound_t *bound, const int8_t *d_states, const int8_t *d_last, size_t n, int extra, uint32_t word_first,
                      uint32_t word_count, uint32_t *d_best, unsigned long long *d_lookups, void *stream)
{
	if (!bound) return fail(RK_EINVAL, "rk_sdeepen_pruned: null bound");
	return sdeepen_states("rk_sdeepen_pruned", ball, bound, d_states, d_last, n, extra, word_first, word_count, d_best, d_lookups, stream);
}

int rk_sshorten(rk_symball_t *h, const int8_t *d_actions, const int32_t *d_len, size_t n, int max_len, int window, int8_t *d_out_actions,
                int32_t *d_out_len, int32_t *d_error, void *d_scratch, size_t scratch_bytes, void *stream)
{
	if (int e = shorten_check("rk_sshorten", h, h && h->built, d_actions, d_len, n, max_len, window, d_out_actions, d_out_len, d_error, d_scratch,
	                          scratch_bytes))
		return e;
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemsetAsync(d_error, 0, sizeof(int32_t), st));
	if (n == 0) return RK_OK;
	int8_t *depth = static_cast<int8_t *>(d_scratch);
	uint16_t *pred = reinterpret_cast<uint16_t *>(depth + shorten_depth_bytes(n, max_len, window));
	hipLaunchKernelGGL(k_ss_windows, dim3(sym_grid(n * (size_t)max_len)), dim3(256), 0, st, h->view, d_actions, d_len, n, max_len, window, depth);
	hipLaunchKernelGGL(k_shorten_dp, dim3((unsigned)n), dim3(SHORTEN_DP_THREADS), 0, st, d_actions, d_len, max_len, window, depth, pred, d_error);
	hipLaunchKernelGGL(k_ss_emit, dim3((unsigned)n), dim3(64), 0, st, h->view, d_actions, d_len, max_len, window, depth, pred, d_out_actions, d_out_len,
	                   d_error);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_ssearch_create(rk_ssearch_t **out, rk_symball_t *ball, size_t capacity, int pops)
{
	if (!out || !ball) return fail(RK_EINVAL, "rk_ssearch_create: null argument");
	if (int e = FrontierPool::check_create("rk_ssearch_create", capacity, pops)) return e;
	if (!ball->built) return fail(RK_ESTATE, "rk_ssearch_create: build the ball first");
	rk_ssearch *h = new rk_ssearch();
	int e = h->alloc(capacity, pops, S_COUNT);
	if (!e) e = h->pool.alloc(&h->hit, (size_t)12 * pops);
	if (e) { delete h; return e; }
	h->attach(ball);
	h->pops_made = pops;
	*out = h;
	return RK_OK;
}

int rk_ssearch_destroy(rk_ssearch_t *h)
{
	delete h;                                   // (lets go of the ball: BallReader)
	return RK_OK;
}

int rk_ssearch_reset(rk_ssearch_t *h, const int8_t *h_start_state, long long max_states, void *stream)
{
	if (!h || !h_start_state) return fail(RK_EINVAL, "rk_ssearch_reset: null argument");
	if (!h->ball->built) return fail(RK_ESTATE, "rk_ssearch_reset: build the ball first");
	hipStream_t st = (hipStream_t)stream;
	h->d.pops = h->pops_made;
	return h->reset(h_start_state, st, [&] {
		hipLaunchKernelGGL(k_ss_root, dim3(1), dim3(64), 0, st, h->d, h->ball->view, h->root_dev, budget_of(max_states));
	});
}

int rk_ssearch_run(rk_ssearch_t *h, int iterations, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_ssearch_run")) return e;
	hipStream_t st = (hipStream_t)stream;
	const unsigned probe_grid = sym_grid((size_t)12 * h->d.pops);
	return h->run("rk_ssearch_run", iterations, st,
	              [&](unsigned grid) {
		              hipLaunchKernelGGL(k_ss_probe, dim3(probe_grid), dim3(256), 0, st, h->d, h->ball->view, h->hit);
		              hipLaunchKernelGGL(k_ss_expand, dim3(grid), dim3(256), 0, st, h->d, h->hit);
	              });
}

int rk_ssearch_status(rk_ssearch_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_ssearch_status: bad argument");
	int32_t c[S_COUNT];
	if (int e = h->read_ctr(c, (hipStream_t)stream)) return e;
	bsearch_status_words(c, h_status);
	return RK_OK;
}

int rk_ssearch_grow(rk_ssearch_t *h, size_t new_capacity, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_ssearch_grow")) return e;
	return h->grow("rk_ssearch_grow", new_capacity, (hipStream_t)stream);
}

long long rk_ssearch_size(const rk_ssearch_t *h) { return FrontierPool::size(h); }

int rk_ssearch_export(rk_ssearch_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_ssearch_export")) return e;
	return h->export_rows("rk_ssearch_export", first, count, h_states, h_parents, h_actions, nullptr, (hipStream_t)stream);
}

long long rk_ssearch_path(rk_ssearch_t *h, long long *h_actions, size_t max_len, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_ssearch_path")) return e;
	if (!h_actions && max_len > 0) return fail(RK_EINVAL, "rk_ssearch_path: null h_actions with max_len %zu", max_len);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_ss_walk, dim3(1), dim3(64), 0, st, h->d, h->ball->view, h->walk, FRONTIER_WALK_MAX);
	RK_HIP(hipGetLastError());
	int32_t len = 0;
	if (int e = read_walk(h->walk, FRONTIER_WALK_MAX, h_actions, max_len, st, &len)) return e;
	if (len == -2) return fail(RK_ESTATE, "rk_ssearch_path: the meeting state has no way down the ball (or is not where the search met)");
	if (len < 0) return fail(RK_ESTATE, "rk_ssearch_path: the search has not met the ball (or a parent chain is broken)");
	return (long long)len;
}

int rk_sdeepen_set_pops(rk_ssearch_t *h, int pops, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_sdeepen_set_pops")) return e;
	if (pops < 1 || pops > h->pops_made) return fail(RK_EINVAL, "rk_sdeepen_set_pops: pops %d outside 1..%d", pops, h->pops_made);
	h->d.pops = pops;
	hipLaunchKernelGGL(k_ss_setpops, dim3(1), dim3(64), 0, (hipStream_t)stream, h->d);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_sdeepen_frontier(rk_ssearch_t *h, long long *h_out, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_sdeepen_frontier")) return e;
	if (!h_out) return fail(RK_EINVAL, "rk_sdeepen_frontier: null output");
	int32_t c[S_COUNT];
	if (int e = h->read_ctr(c, (hipStream_t)stream)) return e;
	h_out[0] = c[S_LO];
	h_out[1] = c[S_HI];
	return RK_OK;
}

// rk_sdeepen_nodes and rk_sdeepen_nodes_pruned (`bound` null: the former)
static int sdeepen_nodes(const char *who, rk_ssearch *h, const rk_bound *bound, int extra, size_t node_first, size_t node_count, uint32_t word_first,
                         uint32_t word_count, uint32_t *d_best, unsigned long long *d_lookups, void *stream)
{
	if (int e = FrontierPool::check_ready(h, who)) return e;
	if (!h->ball->built) return fail(RK_ESTATE, "%s: build the ball first", who);
	if (node_first < 1 || node_count > h->cap || node_first + node_count > h->cap + 1)
		return fail(RK_EINVAL, "%s: nodes %zu..%zu outside the pool", who, node_first, node_first + node_count);
	return launch_deepen(who, h->ball,
	                     DeepenJob{h->d.states + node_first * 5, reinterpret_cast<const int8_t *>(h->d.pact) + node_first, 1 - (long long)node_first,
	                               node_count, extra, word_first, word_count},
	                     d_best, (hipStream_t)stream, bound, d_lookups);
}

int rk_sdeepen_nodes(rk_ssearch_t *h, int extra, size_t node_first, size_t node_count, uint32_t word_first, uint32_t word_count, uint32_t *d_best,
                      void *stream)
{
	return sdeepen_nodes("rk_sdeepen_nodes", h, nullptr, extra, node_first, node_count, word_first, word_count, d_best, nullptr, stream);
}

int rk_sdeepen_nodes_pruned(rk_ssearch_t *h, rk_bound_t *bound, int extra, size_t node_first, size_t node_count, uint32_t word_first,
                            uint32_t word_count, uint32_t *d_best, unsigned long long *d_lookups, void *stream)
{
	if (!bound) return fail(RK_EINVAL, "rk_sdeepen_nodes_pruned: null bound");
	return sdeepen_nodes("rk_sdeepen_nodes_pruned", h, bound, extra, node_first, node_count, word_first, word_count, d_best, d_lookups, stream);
}

long long rk_sdeepen_path(rk_ssearch_t *h, long long node, int extra, uint32_t rank, long long *h_actions, size_t max_len, void *stream)
{
	if (int e = FrontierPool::check_ready(h, "rk_sdeepen_path")) return e;
	if (!h->ball->built) return fail(RK_ESTATE, "rk_sdeepen_path: build the ball first");
	if (extra < 1 || extra > DEEPEN_MAX_EXTRA) return fail(RK_EINVAL, "rk_sdeepen_path: extra %d outside 1..%d", extra, DEEPEN_MAX_EXTRA);
	if (!h_actions && max_len > 0) return fail(RK_EINVAL, "rk_sdeepen_path: null h_actions with max_len %zu", max_len);
	hipStream_t st = (hipStream_t)stream;
	int32_t c[S_COUNT];
	if (int e = h->read_ctr(c, st)) return e;
	if (node < 1 || node > c[F_SIZE]) return fail(RK_EINVAL, "rk_sdeepen_path: node %lld outside 1..%d", node, c[F_SIZE]);
	hipLaunchKernelGGL(k_ss_deepen_walk, dim3(1), dim3(64), 0, st, h->d, h->ball->view, (int)node, extra, rank, h->walk, FRONTIER_WALK_MAX);
	RK_HIP(hipGetLastError());
	int32_t len = 0;
	if (int e = read_walk(h->walk, FRONTIER_WALK_MAX, h_actions, max_len, st, &len)) return e;
	if (len == -2) return fail(RK_ESTATE, "rk_sdeepen_path: word %u of %d moves from node %lld does not lead into the ball", rank, extra, node);
	if (len < 0) return fail(RK_ESTATE, "rk_sdeepen_path: node %lld has no word %u of %d moves (or a parent chain is broken)", node, rank, extra);
	return (long long)len;
}

int rk_ssearchb_create(rk_ssearchb_t **out, rk_symball_t *ball, int n_slots, size_t capacity_per_slot, int pops)
{
	if (int e = FrontierSlots::check_create("rk_ssearchb_create", out, ball, n_slots, capacity_per_slot, pops)) return e;
	if (!ball->built) return fail(RK_ESTATE, "rk_ssearchb_create: build the ball first");
	rk_ssearchb *h = new rk_ssearchb();
	int e = h->alloc("rk_ssearchb_create", n_slots, capacity_per_slot, pops, [&] {
		int a = h->pool.alloc(&h->hit, (size_t)n_slots * 12 * (size_t)pops);
		if (!a) a = h->pool.alloc(&h->keys, (size_t)n_slots * 2);
		if (!a) a = h->pool.alloc(&h->jobs_dev, (size_t)n_slots);
		return a;
	});
	if (!e) {                                   // every key "none", so whichever of a slot's two a first round names is cleared
		hipError_t he = hipMemset(h->keys, 0xFF, (size_t)n_slots * 2 * sizeof(unsigned long long));
		if (he == hipSuccess) he = hipStreamSynchronize(nullptr);         // filled when create returns, whatever stream the first reset takes
		if (he == hipSuccess) he = hipEventCreateWithFlags(&h->jobs_sent, hipEventDisableTiming);
		if (he != hipSuccess) e = fail(RK_EHIP, "rk_ssearchb_create: %s", hipGetErrorString(he));
	}
	if (e) {
		delete h;
		return e;
	}
	h->front.resize((size_t)n_slots);
	h->key_of.assign((size_t)n_slots, 0);
	h->attach(ball);
	*out = h;
	return RK_OK;
}

int rk_ssearchb_destroy(rk_ssearchb_t *h)
{
	delete h;
	return RK_OK;
}

int rk_ssearchb_reset(rk_ssearchb_t *h, int n, const int32_t *slots, const int8_t *h_start_states, const long long *max_states, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_ssearchb_reset: null engine");
	hipStream_t st = (hipStream_t)stream;
	return h->reset("rk_ssearchb_reset", h->ball->built, n, slots, h_start_states, max_states, st, [&] {
		for (int j = 0; j < n; j++) h->front[(size_t)slots[j]] = rk_ssearchb::Front{};     // (checked by now) a new pool: its level is not known
		hipLaunchKernelGGL(kb_ss_root, dim3(1, n), dim3(64), 0, st, h->devs, h->ball->view, h->slots_dev, h->roots_dev, h->budgets_dev, h->clip ? 1 : 0);
	});
}

int rk_ssearchb_run(rk_ssearchb_t *h, int iterations, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_ssearchb_run: null engine");
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid_probe(sym_grid((size_t)12 * h->pops), h->n_slots);
	return h->run("rk_ssearchb_run", h->ball->built, iterations, st, [&](dim3 grid) {
		hipLaunchKernelGGL(kb_ss_probe, grid_probe, dim3(256), 0, st, h->devs, h->ball->view, h->hit);
		hipLaunchKernelGGL(kb_ss_expand, grid, dim3(256), 0, st, h->devs, h->hit);
	});
}

int rk_ssearchb_status(rk_ssearchb_t *h, long long *h_status, void *stream)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_ssearchb_status: null argument");
	return h->status(h_status, (hipStream_t)stream);
}

int rk_ssearchb_paths(rk_ssearchb_t *h, int32_t *h_out, int max_len, void *stream)
{
	if (!h || !h_out) return fail(RK_EINVAL, "rk_ssearchb_paths: null argument");
	hipStream_t st = (hipStream_t)stream;
	return h->paths("rk_ssearchb_paths", h->ball->built, h_out, max_len, st, [&] {
		hipLaunchKernelGGL(kb_ss_walk, dim3(h->n_slots), dim3(64), 0, st, h->devs, h->ball->view, h->walk, max_len);
	});
}

int rk_ssearchb_export(rk_ssearchb_t *h, int slot, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_ssearchb_export: null engine");
	return h->export_rows("rk_ssearchb_export", slot, first, count, h_states, h_parents, h_actions, (hipStream_t)stream);
}

int rk_sdeepenb_set(rk_ssearchb_t *h, int on)
{
	if (!h) return fail(RK_EINVAL, "rk_sdeepenb_set: null engine");
	h->clip = on != 0;
	return RK_OK;
}

int rk_sdeepenb_frontiers(rk_ssearchb_t *h, long long *h_out, void *stream)
{
	if (!h || !h_out) return fail(RK_EINVAL, "rk_sdeepenb_frontiers: null argument");
	const int32_t *c = nullptr;
	if (int e = h->ctr_host.fetch(h->d.ctr, (size_t)h->n_slots * S_COUNT, h->ctr_spare.data(), (hipStream_t)stream, &c)) return e;
	for (int s = 0; s < h->n_slots; s++, c += S_COUNT) {
		h_out[2 * s] = c[S_LO];
		h_out[2 * s + 1] = c[S_HI];
		rk_ssearchb::Front &f = h->front[(size_t)s];
		const bool open = f.stopped && f.round_open;                     // (a stopped slot stands still: a second read changes nothing)
		f = rk_ssearchb::Front{c[S_LO], c[S_HI], c[F_SIZE], c[F_DONE] != 0 && c[F_SIZE] >= 1, false};
		f.round_open = f.stopped && open;
	}
	return RK_OK;
}

int rk_sdeepenb_probe(rk_ssearchb_t *h, int n_jobs, const rk_deepen_job_t *h_jobs, void *stream)
{
	const char *who = "rk_sdeepenb_probe";
	if (!h) return fail(RK_EINVAL, "%s: null engine", who);
	if (!h->ball->built) return fail(RK_ESTATE, "%s: build the ball first", who);
	if (n_jobs < 0 || n_jobs > h->n_slots) return fail(RK_EINVAL, "%s: %d jobs for %d slots", who, n_jobs, h->n_slots);
	if (n_jobs == 0) return RK_OK;
	if (!h_jobs) return fail(RK_EINVAL, "%s: null jobs", who);
	std::vector<char> named((size_t)h->n_slots, 0);
	std::vector<SlotDeepenJob> jobs((size_t)n_jobs);
	unsigned long long probes = 0;
	size_t items = 0;
	for (int j = 0; j < n_jobs; j++) {
		const rk_deepen_job_t &q = h_jobs[j];
		if (q.slot < 0 || q.slot >= h->n_slots) return fail(RK_EINVAL, "%s: slot %d outside 0..%d", who, q.slot, h->n_slots - 1);
		if (named[q.slot]) return fail(RK_EINVAL, "%s: slot %d is named twice", who, q.slot);
		named[q.slot] = 1;
		if (q.extra < 1 || q.extra > DEEPEN_MAX_EXTRA) return fail(RK_EINVAL, "%s: extra %d of slot %d outside 1..%d", who, q.extra, q.slot, DEEPEN_MAX_EXTRA);
		const rk_ssearchb::Front &f = h->front[(size_t)q.slot];
		if (!f.stopped) return fail(RK_ESTATE, "%s: slot %d had not stopped at the last rk_sdeepenb_frontiers (or was reset since)", who, q.slot);
		if (q.node_count < 1 || q.node_first < (uint32_t)f.lo || q.node_first > (uint32_t)f.hi || q.node_count > (uint32_t)f.hi - q.node_first + 1u)
			return fail(RK_EINVAL, "%s: nodes %u.. (%u of them) outside slot %d's frontier %d..%d", who, q.node_first, q.node_count, q.slot, f.lo, f.hi);
		const uint32_t words = deepen_words(q.extra, f.lo == 1 ? -1 : 0);   // (node 1 is a level of its own and has no last move)
		if (q.word_count < 1 || q.word_first >= words || q.word_count > words - q.word_first)
			return fail(RK_EINVAL, "%s: words %u.. (%u of them) outside the %u words of %d moves of slot %d", who, q.word_first, q.word_count, words, q.extra, q.slot);
		if (!q.new_round && !f.round_open) return fail(RK_ESTATE, "%s: the first job of slot %d since its reset must start a round (new_round)", who, q.slot);
		probes += (unsigned long long)q.node_count * q.word_count;
		if (probes > DEEPEN_MAX_PROBES) return fail(RK_EINVAL, "%s: more than the %llu probes of one launch", who, DEEPEN_MAX_PROBES);
		items = std::max(items, (size_t)q.node_count * deepen_groups(q.extra, q.word_first, q.word_count));
		jobs[(size_t)j] = SlotDeepenJob{q.slot, q.extra, q.node_first, q.node_count, q.word_first, q.word_count, 0u, 0u};
	}
	for (SlotDeepenJob &job : jobs) {                                    // nothing is refused from here on
		const size_t s = (size_t)job.slot;
		if (h_jobs[&job - jobs.data()].new_round) h->key_of[s] ^= 1u;    // the key the launches before left cleared
		h->front[s].round_open = true;
		job.key_at = (uint32_t)(2 * s + h->key_of[s]);
	}
	hipStream_t st = (hipStream_t)stream;
	if (int e = h->send_jobs(jobs, st)) return e;
	hipLaunchKernelGGL(kb_sd_probe, dim3(sym_grid(items), n_jobs), dim3(256), 0, st, h->devs, h->ball->view, h->jobs_dev, h->keys);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_sdeepenb_keys(rk_ssearchb_t *h, unsigned long long *h_out, void *stream)
{
	if (!h || !h_out) return fail(RK_EINVAL, "rk_sdeepenb_keys: null argument");
	hipStream_t st = (hipStream_t)stream;
	std::vector<unsigned long long> both((size_t)h->n_slots * 2);
	RK_HIP(hipMemcpyAsync(both.data(), h->keys, both.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	RK_HIP(hipStreamSynchronize(st));
	for (size_t s = 0; s < (size_t)h->n_slots; s++) h_out[s] = h->front[s].round_open ? both[2 * s + h->key_of[s]] : DEEPEN_NO_KEY;
	return RK_OK;
}

int rk_sdeepenb_paths(rk_ssearchb_t *h, int n, const int32_t *slots, const long long *nodes, const int32_t *extras, const uint32_t *ranks,
                             int32_t *h_out, int max_len, void *stream)
{
	const char *who = "rk_sdeepenb_paths";
	if (!h) return fail(RK_EINVAL, "%s: null engine", who);
	if (n < 0 || n > h->n_slots) return fail(RK_EINVAL, "%s: %d rows for %d slots", who, n, h->n_slots);
	if (n == 0) return RK_OK;
	if (!slots || !nodes || !extras || !ranks || !h_out) return fail(RK_EINVAL, "%s: null argument", who);
	std::vector<SlotDeepenJob> jobs((size_t)n);
	for (int j = 0; j < n; j++) {
		if (slots[j] < 0 || slots[j] >= h->n_slots) return fail(RK_EINVAL, "%s: slot %d outside 0..%d", who, slots[j], h->n_slots - 1);
		const rk_ssearchb::Front &f = h->front[(size_t)slots[j]];
		if (!f.stopped) return fail(RK_ESTATE, "%s: slot %d had not stopped at the last rk_sdeepenb_frontiers (or was reset since)", who, slots[j]);
		if (nodes[j] < 1 || nodes[j] > f.size) return fail(RK_EINVAL, "%s: node %lld outside 1..%d of slot %d", who, nodes[j], f.size, slots[j]);
		if (extras[j] < 1 || extras[j] > DEEPEN_MAX_EXTRA) return fail(RK_EINVAL, "%s: extra %d outside 1..%d", who, extras[j], DEEPEN_MAX_EXTRA);
		jobs[(size_t)j] = SlotDeepenJob{slots[j], extras[j], (uint32_t)nodes[j], 1u, ranks[j], 1u, 0u, 0u};
	}
	hipStream_t st = (hipStream_t)stream;
	int sent = RK_OK;
	const int e = h->paths(who, h->ball->built, h_out, max_len, st, [&] {
		sent = h->send_jobs(jobs, st);
		if (sent == RK_OK) hipLaunchKernelGGL(kb_ss_deepen_walk, dim3(n), dim3(64), 0, st, h->devs, h->ball->view, h->jobs_dev, h->walk, max_len);
	}, n);
	return sent != RK_OK ? sent : e;
}

}  // extern "C"
