// Device-side pieces shared by the search engines (single A*, sharded A*, batched A*, breadth-first search): queue records and their order,
// the state hash, order-preserving compaction inside a workgroup, binary search in a sorted run, and the net rows, the argmax rule and
// the 64-bit counters of the engines that own their net batches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/rubiks_hip.h"
#include "rk_device.h"

namespace rk {

struct Rec { uint64_t key; uint64_t idx; };

constexpr uint32_t TENT = 0x80000000u;          // hash slot holds a batch position, not yet an index
constexpr uint32_t NO_MARK = 0xFFFFFFFFu;


__device__ __forceinline__ bool rec_less(const Rec &a, const Rec &b)
{
	return a.key < b.key || (a.key == b.key && a.idx < b.idx);
}

// float64 -> uint64 whose unsigned order is the float order.  A NaN maps below -inf or above +inf by its sign bit, in bounds but in
// no order a search could use: the A* engines end the search that meets one with ERR_NONFINITE (cost_record, rk_astar.hip).
__device__ __forceinline__ uint64_t sortable_key(double c)
{
	c = c + 0.0;                                  // -0.0 -> +0.0: Python compares them equal
	const uint64_t u = (uint64_t)__double_as_longlong(c);
	return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__host__ __device__ inline double key_to_double(uint64_t k)
{
	const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
	double d;
	memcpy(&d, &u, sizeof d);
	return d;
}

__host__ __device__ inline uint32_t hash_state(const uint32_t s[5])
{
	uint64_t h = 0x9E3779B97F4A7C15ull;
	#pragma unroll
	for (int j = 0; j < 5; j++) {
		h ^= s[j];
		h *= 0xFF51AFD7ED558CCDull;
		h ^= h >> 29;
	}
	return (uint32_t)(h ^ (h >> 32));
}

// owner rank of a state in a hash-sharded search: a remix of the hash, so that it is independent of the table slot
__host__ __device__ inline uint32_t owner_of(const uint32_t s[5], uint32_t world)
{
	const uint32_t h = hash_state(s) * 0x9E3779B1u;
	return (uint32_t)(((uint64_t)h * world) >> 32);
}

__device__ __forceinline__ void load5(const uint32_t *p, uint32_t s[5])
{
	#pragma unroll
	for (int j = 0; j < 5; j++) s[j] = p[j];
}

__device__ __forceinline__ bool equal5(const uint32_t a[5], const uint32_t *p)
{
	return ((a[0] ^ p[0]) | (a[1] ^ p[1]) | (a[2] ^ p[2]) | (a[3] ^ p[3]) | (a[4] ^ p[4])) == 0;
}

// child `a` of the stored state `parent` (s_act: the action tables staged in LDS by stage_action_tables)
__device__ __forceinline__ void child_state(const uint32_t *states, int32_t parent, const u32x4 *s_act, uint32_t a, uint32_t s[5])
{
	load5(states + (size_t)parent * 5, s);
	uint32_t tab[12];
	load_action_table(s_act, a, tab);
	move5(s, tab);
}

// Membership test + in-batch first-occurrence election through an open-addressing table of indices (T = mask + 1 slots,
// linear probing).  Child c of the batch claims an empty slot as TENT | c; children that hold the same state settle on the
// smallest position with atomicMin, so once every child has probed, a slot holds TENT | (first occurrence).  Returns the
// stored index (> 0) of a state that is already in the table, or 0 when c took part in a claim; *slot_out is that slot.
// other(c', buf): the state of batch position c' (recomputed or loaded).
template <typename Other>
__device__ __forceinline__ uint32_t probe_elect(uint32_t *table, uint32_t mask, const uint32_t *states, const uint32_t s[5], int c,
                                                Other other, uint32_t *slot_out)
{
	uint32_t slot = hash_state(s) & mask;
	for (;;) {
		// (the claim IS the probe: an empty slot -- two children in three at N = 1000 are new states -- costs one round trip to the
		//  table instead of a load and then the compare-and-swap; an occupied slot answers with its occupant either way)
		const uint32_t e = atomicCAS(&table[slot], 0u, TENT | (uint32_t)c);
		if (e == 0u) { *slot_out = slot; return 0u; }
		if (e & TENT) {
			uint32_t o[5];
			other((int)(e & ~TENT), o);
			if (((s[0] ^ o[0]) | (s[1] ^ o[1]) | (s[2] ^ o[2]) | (s[3] ^ o[3]) | (s[4] ^ o[4])) == 0u) {
				atomicMin(&table[slot], TENT | (uint32_t)c);          // all claimants hold the same state: smallest position wins
				*slot_out = slot;
				return 0u;
			}
		} else if (equal5(s, states + (size_t)e * 5)) {
			return e;
		}
		slot = (slot + 1) & mask;
	}
}

// Membership test that writes nothing: the stored index (> 0) of state s in a table that other kernels may read at the same
// time, or 0.  For a table that is final (rk_ball.hip: a built ball holds no tentative slot); a tentative slot, should one be
// met, is passed over without being followed.  The table is at most half full, so an empty slot ends every probe.
__device__ __forceinline__ uint32_t probe_find(const uint32_t *table, uint32_t mask, const uint32_t *states, const uint32_t s[5])
{
	uint32_t slot = hash_state(s) & mask;
	for (;;) {
		const uint32_t e = table[slot];
		if (e == 0u) return 0u;
		if ((e & TENT) == 0u && equal5(s, states + (size_t)e * 5)) return e;
		slot = (slot + 1) & mask;
	}
}

// After a growth (or to drop stale claims): the stored states 1..n of one pool back into its cleared table.  No slot is tentative
// then, so this is a plain insert; the slot a state lands in may differ from the one it had, which no result depends on (look-ups
// compare states).  This thread takes the indices first, first + stride, ... (the kernel passes its own 1 + x position and the
// grid's width: read in here, blockDim compiles to the general form that allows for a partial last workgroup).
__device__ __forceinline__ void rehash_pool(const uint32_t *states, uint32_t *table, uint32_t mask, int n, int first, int stride)
{
	for (int idx = first; idx <= n; idx += stride) {
		uint32_t s[5];
		load5(states + (size_t)idx * 5, s);
		uint32_t slot = hash_state(s) & mask;
		while (atomicCAS(&table[slot], 0u, (uint32_t)idx) != 0u) slot = (slot + 1) & mask;
	}
}

// ---- what the engines that own their net batches share (epsilon-greedy value search, the greedy one-step games, beam search) ----
// dword j of a state held in registers, j not known at compile time (no indexed register array)
__device__ __forceinline__ uint32_t dword_of(const uint32_t s[5], int j)
{
	return j == 0 ? s[0] : j == 1 ? s[1] : j == 2 ? s[2] : j == 3 ? s[3] : s[4];
}

// Row `row` of a net batch from state s, written by `n` threads of which this is thread `t`: (rows, 480) one-hot of 4- or 2-byte
// elements, oh[24 i + s[i]] = 1 (cube.py:265-277), in 16-byte chunks, or the 20 bytes themselves.
__device__ __forceinline__ void write_row(void *buf, int code, size_t row, const uint32_t s[5], int t, int n)
{
	if (code == RK_OH_STATES) {
		uint32_t *dst = reinterpret_cast<uint32_t *>(buf) + row * 5;
		for (int j = t; j < 5; j += n) dst[j] = dword_of(s, j);
		return;
	}
	const bool wide = code == RK_OH_F32;
	const uint32_t one_bits = wide ? 0x3F800000u : code == RK_OH_F16 ? 0x3C00u : 0x3F80u;
	const int E = wide ? 4 : 8, CPR = 480 / E, CPC = 24 / E;
	u32x4 *dst = reinterpret_cast<u32x4 *>(buf) + row * CPR;
	for (int g = t; g < CPR; g += n) {
		const int cubie = g / CPC, base = (g - cubie * CPC) * E;
		const int rel = (int)((dword_of(s, cubie >> 2) >> (8 * (cubie & 3))) & 0xFFu) - base;
		u32x4 val = {0u, 0u, 0u, 0u};
		if (wide) {
			val.x = rel == 0 ? one_bits : 0u; val.y = rel == 1 ? one_bits : 0u;
			val.z = rel == 2 ? one_bits : 0u; val.w = rel == 3 ? one_bits : 0u;
		} else if (rel >= 0 && rel < 8) {
			const uint32_t one = one_bits << (16 * (rel & 1));
			val.x = (rel >> 1) == 0 ? one : 0u; val.y = (rel >> 1) == 1 ? one : 0u;
			val.z = (rel >> 1) == 2 ? one : 0u; val.w = (rel >> 1) == 3 ? one : 0u;
		}
		dst[g] = val;
	}
}

// element i of a float32 or bfloat16 vector, widened exactly
__device__ __forceinline__ float net_out(const void *p, bool bf16, size_t i)
{
	if (!bf16) return reinterpret_cast<const float *>(p)[i];
	return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(p)[i] << 16);
}

// (v, i) beats (bv, bi) under "first index of the maximum, NaN counts as the maximum" (ndarray.argmax, torch.argmax on the CPU)
__device__ __forceinline__ bool beats(float v, int i, float bv, int bi)
{
	const bool vn = v != v, bn = bv != bv;
	if (vn != bn) return vn;
	if (!vn && v != bv) return v > bv;
	return i < bi;
}

// a 64-bit counter in words w (low half) and w + 1 of an int32 counter block (on the host: of the block's copy)
__host__ __device__ __forceinline__ long long ctr64(const int32_t *ctr, int w)
{
	return (long long)(((unsigned long long)(uint32_t)ctr[w + 1] << 32) | (uint32_t)ctr[w]);
}

__device__ __forceinline__ void set_ctr64(int32_t *ctr, int w, long long v)
{
	ctr[w] = (int32_t)(uint32_t)(unsigned long long)v;
	ctr[w + 1] = (int32_t)(uint32_t)((unsigned long long)v >> 32);
}

// ---- order-preserving compaction across workgroups in ONE launch: tickets + look-back --------------------------------
// Every workgroup draws a ticket (so that "predecessor" means "started earlier": no deadlock whatever the dispatch
// order), publishes its local total at once and then sums the totals of ALL its predecessors, 64 at a time with one wave
// (a decoupled look-back without the prefix hand-over: nobody waits for a chain, only for words that are published
// before any waiting starts).  A word is {epoch : 32 | total : 32} written with ONE 64-bit agent-scope store and polled
// with agent-scope loads; the epoch makes the words of earlier launches invisible, so nothing has to be cleared except
// the ticket counter (the engine's end-of-iteration kernel does that).  The word carries its payload itself, so no
// fence is needed (MI355X_MICROARCH.md: a naturally aligned 8-byte granule written by one store).
constexpr int ASCAN = 256;                        // threads (= items) per workgroup of these compactions

// exclusive prefix of a 0/1 predicate inside a 256-thread workgroup; *total = number of set predicates
__device__ __forceinline__ int block_rank256(bool pred, int *s_wave /* [4] */, int *total)
{
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const unsigned long long b = __ballot(pred);
	const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
	__syncthreads();                                  // s_wave may still be read from a previous call
	if (lane == 0) s_wave[wv] = __popcll(b);
	__syncthreads();
	int before = 0, tot = 0;
	#pragma unroll
	for (int w = 0; w < 4; w++) {
		const int v = s_wave[w];
		before += w < wv ? v : 0;
		tot += v;
	}
	*total = tot;
	return before + in_wave;
}

__device__ __forceinline__ int scan_ticket(int32_t *ticket_ctr, int *s_ticket)
{
	if (threadIdx.x == 0) *s_ticket = atomicAdd(ticket_ctr, 1);
	__syncthreads();
	return *s_ticket;
}

// exclusive prefix of `total` over tickets 0..b-1.  Call from ALL threads of the workgroup (it contains a barrier);
// s_base is one int of LDS.
__device__ __forceinline__ int scan_lookback(unsigned long long *words, int b, int total, uint32_t epoch, int *s_base)
{
	if (threadIdx.x == 0)
		__hip_atomic_store(&words[b], ((unsigned long long)epoch << 32) | (uint32_t)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (threadIdx.x < 64) {                           // wave 0 sums the predecessors' totals, 64 per round
		int sum = 0;
		for (int j0 = 0; j0 < b; j0 += 64) {
			const int j = j0 + (int)threadIdx.x;
			if (j < b) {
				unsigned long long w;
				for (;;) {
					w = __hip_atomic_load(&words[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if ((uint32_t)(w >> 32) == epoch) break;
					__builtin_amdgcn_s_sleep(1);
				}
				sum += (int)(uint32_t)w;
			}
		}
		#pragma unroll
		for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, 64);
		if (threadIdx.x == 0) *s_base = sum;
	}
	__syncthreads();
	return *s_base;
}

// The same for W classes at once (the sharded engine buckets records by owner rank): every thread belongs to class `cls` (none: cls >= W).
// Returns the thread's position in its class's output -- the class's total over all workgroups with smaller tickets plus the thread's rank
// inside this workgroup; afterwards s_tot[w] / s_base[w] (W ints each, LDS) hold this workgroup's total and its predecessors' sum per class.
// ALL totals are published before anybody waits, so the chain costs ONE wait on the predecessors instead of W of them back to back
// (W = 8: the sharded expand kernel spent 41 us of a 14-us job in eight dependent look-backs, benchmarks/sharded_sim8.py).
// words: W rows of `nblocks` look-back words.  Call from ALL threads of a 256-thread workgroup.
__device__ __forceinline__ int scan_lookback_classes(unsigned long long *words, int nblocks, int b, int W, uint32_t cls, uint32_t epoch,
                                                    int *s_wave /* [4] */, int *s_tot, int *s_base)
{
	// ranks inside this workgroup for all classes with ONE barrier: per wave a ballot per class (no barrier), the waves' counts in LDS
	__shared__ int s_cnt[4 * 64];
	const int lane0 = threadIdx.x & 63, wv0 = threadIdx.x >> 6;
	int my = 0;
	for (int w = 0; w < W; w++) {
		const unsigned long long bal = __ballot(cls == (uint32_t)w);
		if (lane0 == 0) s_cnt[wv0 * 64 + w] = __popcll(bal);
		if (cls == (uint32_t)w) my = __popcll(bal & ((1ull << lane0) - 1ull));
	}
	__syncthreads();
	if (cls < (uint32_t)W)
		for (int v = 0; v < wv0; v++) my += s_cnt[v * 64 + cls];
	if ((int)threadIdx.x < W) s_tot[threadIdx.x] = s_cnt[threadIdx.x] + s_cnt[64 + threadIdx.x] + s_cnt[128 + threadIdx.x] + s_cnt[192 + threadIdx.x];
	(void)s_wave;
	__syncthreads();
	if ((int)threadIdx.x < W)
		__hip_atomic_store(&words[(size_t)threadIdx.x * nblocks + b], ((unsigned long long)epoch << 32) | (uint32_t)s_tot[threadIdx.x],
		                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
	for (int w = wv; w < W; w += nw) {                // a wave per class, 64 predecessors per round
		const unsigned long long *row = words + (size_t)w * nblocks;
		int sum = 0;
		for (int j0 = 0; j0 < b; j0 += 64) {
			const int j = j0 + lane;
			if (j < b) {
				unsigned long long x;
				for (;;) {
					x = __hip_atomic_load(&row[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if ((uint32_t)(x >> 32) == epoch) break;
					__builtin_amdgcn_s_sleep(1);
				}
				sum += (int)(uint32_t)x;
			}
		}
		#pragma unroll
		for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, 64);
		if (lane == 0) s_base[w] = sum;
	}
	__syncthreads();
	return (cls < (uint32_t)W ? s_base[cls] : 0) + my;
}

// ---- a batch of K children in pop order: what the frontier pool (rk_frontier_dev.h) and the ball builds (rk_ballbuild_dev.h) scan ----
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;       // slot[c] of a child that takes part in no claim (any value with the TENT bit)

// First-occurrence flags of the batch and their exclusive prefix in batch order, one launch of ASCAN-thread workgroups: child c
// is a first occurrence iff the slot it claimed (slot[c], TENT bit clear) still holds TENT | c once every child has probed.
// Writes first[c] and rank[c] for c < K and the number of first occurrences to *total_out; `epoch` is the launch's (the
// end-of-iteration kernel resets *ticket and moves the epoch on).  Call from ALL threads of the workgroup.
__device__ __forceinline__ void frontier_scan(const uint32_t *slot, const uint32_t *table, int32_t *rank, uint8_t *first,
                                              unsigned long long *chain, int32_t *ticket, uint32_t epoch, int32_t *total_out, int K)
{
	__shared__ int s_wave[4];
	__shared__ int s_ticket, s_base;
	const int b = scan_ticket(ticket, &s_ticket);
	const int last = (K - 1) / ASCAN;
	if (b > last) return;
	const int c = b * ASCAN + threadIdx.x;
	const bool valid = c < K;
	bool fu = false;
	if (valid) {
		const uint32_t sl = slot[c];
		fu = (sl & TENT) == 0u && __hip_atomic_load(&table[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (TENT | (uint32_t)c);
	}
	int total;
	const int r = block_rank256(fu, s_wave, &total);
	const int base = scan_lookback(chain, b, total, epoch, &s_base);
	if (valid) {
		rank[c] = base + r;
		first[c] = fu ? 1 : 0;
	}
	if (b == last && threadIdx.x == 0) *total_out = base + total;
}

// The first of the P pops of a batch that the state budget refuses, P when none is: pop j runs only if size0 + (new states of
// the pops before j) < budget, and rank[12 j] is that count.  It only grows along the batch, hence the bisection.
__device__ __forceinline__ int first_refused_pop(const int32_t *rank, int P, int32_t size0, long long budget)
{
	int lo = 0, hi = P;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if ((long long)size0 + rank[12 * mid] >= budget) hi = mid; else lo = mid + 1;
	}
	return lo;
}

__device__ __forceinline__ int lower_bound_rec(const Rec *a, int n, const Rec &x)
{
	int lo = 0, hi = n;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (rec_less(a[mid], x)) lo = mid + 1; else hi = mid;
	}
	return lo;
}


}  // namespace rk
