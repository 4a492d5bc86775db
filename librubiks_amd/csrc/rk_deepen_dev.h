// Depth-first probes of the symmetry ball (rk_sdeepen, rk_sdeepen_*): short words applied to a state, every result
// canonicalised and looked up in the ball, nothing kept but the lowest rank that hit.  Shared by the launches of rk_sym.hip.
//
// Words.  A word of `extra` moves for a state whose last move was `last` (-1: none) is a sequence of actions 0..11 in which no
// action is the opposite turn (a ^ 1) of the one before it; "before the first" is `last`.  In lexicographic order of the actions
// a word is the number  rank = ((d_0 * 11 + d_1) * 11 + ...) + d_{extra-1}:  digit d_k counts the allowed actions below action k,
//   action = digit                            with no action before it (d_0 in 0..11),
//   action = digit + (digit >= (prev ^ 1))    otherwise              (digit in 0..10),
// so there are 11^extra words, 12 * 11^(extra-1) without a last move, and rank order is lexicographic order.
//
// Work.  An item is (state i, g): the ranks g * 121 .. g * 121 + 120 that share the first extra - 2 moves (extra <= 2: the one
// item g = 0 holds every rank).  A wave takes an item: the state after the shared moves is composed once, each of the up to 11
// (12) next-to-last moves once, and a probe costs one move, one canonical form (lane = symmetry, rk_sym_dev.h) and one read-only
// look-up.  Everything is the same in every lane; lane 0 does the atomicMin.  Ranks outside [word_first, word_first + word_count),
// ranks a state does not have, and ranks above the state's current best are skipped; a hit ends the item, whose later ranks are
// all above it.
//
// What is kept.  A launch on the caller's states or on one search's pool keeps a word per state, the lowest rank that hit
// (DeepenRanks).  A slot of the batch keeps ONE 64-bit key for its whole frontier, node << 32 | rank (DeepenKey): the lowest key is
// the lowest node that has a hit and that node's lowest rank, which is what the words give when they are read in node order.  A
// (node, rank) above the key is skipped, so after the first hit what is left of a round collapses to the lower nodes.
//
// Pruning.  A launch may carry an admissible bound (PdbPrune below): words behind a state that is provably too far from the
// ball are not looked up, which changes no hit and therefore nothing that is kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rk_device.h"
#include "rk_pdb_dev.h"
#include "rk_search_dev.h"
#include "rk_sym_dev.h"

namespace rk {

constexpr int DEEPEN_MAX_EXTRA = 8;
constexpr uint32_t DEEPEN_NONE = 0xFFFFFFFFu;       // d_best of a state without a hit
constexpr unsigned long long DEEPEN_NO_KEY = ~0ull;  // the key of a slot without a hit
constexpr uint32_t DEEPEN_SPAN = 121;               // ranks of an item when extra >= 3
// The most probes (states x word_count) of one launch.  Measured on the radius-10 ball (benchmarks/symball_deepen.py,
// profiles/r17_symball_deepen.json); the cap keeps a launch well under a second on a machine that others share.
constexpr unsigned long long DEEPEN_MAX_PROBES = 1ull << 28;

__host__ __device__ inline uint32_t deepen_pow11(int k)
{
	uint32_t p = 1;
	for (int j = 0; j < k; j++) p *= 11u;
	return p;
}

// words of `extra` moves behind the action `last` (-1: none)
__host__ __device__ inline uint32_t deepen_words(int extra, int last) { return (last < 0 ? 12u : 11u) * deepen_pow11(extra - 1); }

__host__ __device__ inline int deepen_action(int prev, int digit) { return prev < 0 ? digit : digit + (digit >= (prev ^ 1) ? 1 : 0); }

// a stored last action as the kernels take it: anything outside 0..11 is "none"
__host__ __device__ inline int deepen_last(int v) { return v >= 0 && v < N_ACTIONS ? v : -1; }

// The actions of word `rank` behind `last`, most significant digit first, to out[0 .. extra - 1]; false for a rank the state
// does not have.
__host__ __device__ inline bool deepen_word(int extra, int last, uint32_t rank, int *out)
{
	if (rank >= deepen_words(extra, last)) return false;
	int prev = last;
	for (int k = 0; k < extra; k++) {
		const uint32_t p = deepen_pow11(extra - 1 - k);
		const uint32_t d = rank / p;
		rank -= d * p;
		out[k] = prev = deepen_action(prev, (int)d);
	}
	return true;
}

// ranks per item (extra <= 2: every rank is below 132)
__host__ __device__ inline uint32_t deepen_span(int extra) { return extra >= 3 ? DEEPEN_SPAN : 132u; }

// the items per state of the ranks [word_first, word_first + word_count), word_count >= 1
__host__ __device__ inline uint32_t deepen_groups(int extra, uint32_t word_first, uint32_t word_count)
{
	const uint32_t span = deepen_span(extra);
	return (uint32_t)(((unsigned long long)word_first + word_count - 1u) / span) - word_first / span + 1u;
}

struct DeepenJob {
	const uint32_t *states;                     // (n, 5) dwords
	const int8_t *last;                         // (n) or null: the action that led to each state, anything outside 0..11 for none
	long long no_last;                          // the one row whose stored action is no action (a pool's node 1), -1: none
	size_t n;
	int extra;
	uint32_t word_first, word_count;
};

// What a launch keeps of its hits.  limit(i): the highest rank of state i that is still worth a probe, -1 when none is, the same
// in every lane and read through readfirstlane; lower(i, r): rank r of state i hit (one lane calls it).
struct DeepenRanks {                            // best (n): atomicMin of the ranks that hit, DEEPEN_NONE without one
	uint32_t *best;
	__device__ __forceinline__ long long limit(size_t i) const
	{
		return (long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&best[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
	}
	__device__ __forceinline__ void lower(size_t i, uint32_t r) const { atomicMin(&best[i], r); }
};

struct DeepenKey {                              // *key: atomicMin of (node_first + i) << 32 | rank over the hits, DEEPEN_NO_KEY without one
	unsigned long long *key;
	uint32_t node_first;
	__device__ __forceinline__ long long limit(size_t i) const
	{
		const unsigned long long k = __hip_atomic_load(key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const uint32_t node = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(k >> 32));
		const uint32_t rank = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)k);
		const uint32_t mine = node_first + (uint32_t)i;
		return mine < node ? (long long)DEEPEN_NONE : mine == node ? (long long)rank : -1ll;
	}
	__device__ __forceinline__ void lower(size_t i, uint32_t r) const { atomicMin(key, (unsigned long long)(node_first + (uint32_t)i) << 32 | r); }
};

__device__ __forceinline__ void deepen_move(const u32x4 *s_act, int a, const uint32_t in[5], uint32_t out[5])
{
	uint32_t tab[12];
	#pragma unroll
	for (int j = 0; j < 5; j++) out[j] = in[j];
	load_action_table(s_act, (uint32_t)a, tab);
	move5(out, tab);
}

// What a launch knows about words that cannot hit.  NoPrune: nothing, every word is looked up.  PdbPrune: an admissible bound
// (rk_pdb_dev.h) and the ball's radius R; left(s, m) says that no state of the ball lies within m moves of s, bound(s) > R + m.
// A word that hits has no such prefix -- the state after k of its e moves is at most (e - k) + R from solved --, so the hits,
// and with them everything a launch keeps, are NoPrune's.  lookups (null: not counted) += the sb_node calls of a wave, once.
struct NoPrune {
	static constexpr bool on = false;
};

struct PdbPrune {
	static constexpr bool on = true;
	PdbBound bound;
	int radius;
	unsigned long long *lookups;
	__device__ __forceinline__ bool left(const uint32_t s[5], int m) const { return pdb_bound(bound, s) > radius + m; }
	// the same for a state that every lane holds: one answer for the wave, in a scalar register
	__device__ __forceinline__ bool left_uniform(const uint32_t s[5], int m) const { return __builtin_amdgcn_readfirstlane((int)left(s, m)) != 0; }
};

// The last two moves of an item under PdbPrune.  The item's up to 132 (next-to-last, last) pairs are filtered with lane = word,
// 64 at a time: a lane makes its own two moves and asks the bound about its next-to-last state and its leaf; lanes whose rank
// is outside [lo, hi), above `best` or not a rank of the item are off.  The ballot is the pass's survivors, which the wave takes
// in ascending rank order as deepen_probe takes every word: the leaf made again in every lane, one cooperative look-up, a hit
// ends the item.  s: the state after the shared moves, prev: the move before the pair; cm x cl pairs, rank = base + dm * cl + dl.
template <typename Keep>
__device__ __forceinline__ void deepen_pairs_pruned(const SymBallView &b, const SymProbe &c, const PdbPrune &prune, const Keep &keep, size_t i, int e,
                                                    const uint32_t s[5], int prev, uint32_t cm, uint32_t cl, long long base, long long lo, long long hi,
                                                    long long best, unsigned long long &lookups)
{
	const u32x4 *s_act = c.s_act;
	const uint32_t pairs = cm * cl;
	uint32_t s1[5];
	uint32_t at = ~0u;                                               // the next-to-last move s1 holds
	int p1 = prev;
	#pragma unroll
	for (int j = 0; j < 5; j++) s1[j] = s[j];
	for (uint32_t first = 0; first < pairs; first += WAVE) {
		if (base + first >= hi || base + first > best) break;
		if (base + first + WAVE <= lo) continue;
		const uint32_t mine = first + (uint32_t)c.lane;
		const long long r = base + mine;
		bool live = mine < pairs && r >= lo && r < hi && r <= best;
		{                                                            // lane = word (a lane that is off makes pair 0's moves)
			const uint32_t w = live ? mine : 0u, dm = w / cl, dl = w - dm * cl;
			uint32_t x[5], y[5];
			int q = prev;
			if (e >= 2) {
				q = deepen_action(prev, (int)dm);
				deepen_move(s_act, q, s, x);
				live = live && !prune.left(x, 1);
			} else {
				#pragma unroll
				for (int j = 0; j < 5; j++) x[j] = s[j];
			}
			deepen_move(s_act, deepen_action(q, (int)dl), x, y);
			live = live && !prune.left(y, 0);
		}
		unsigned long long todo = __ballot(live);
		while (todo != 0ull) {                                       // (the same in every lane from here on)
			const uint32_t w = first + (uint32_t)__ffsll((long long)todo) - 1u, dm = w / cl, dl = w - dm * cl;
			todo &= todo - 1ull;
			if (e >= 2 && dm != at) {
				p1 = deepen_action(prev, (int)dm);
				deepen_move(s_act, p1, s, s1);
				at = dm;
			}
			uint32_t s2[5];
			deepen_move(s_act, deepen_action(p1, (int)dl), s1, s2);
			lookups++;
			if (sb_node(b, c, s2) != 0u) {
				if (c.lane == 0) keep.lower(i, (uint32_t)(base + w));
				return;                                              // every later rank of the item is above this one
			}
		}
	}
}

// the items wave, wave + stride, ... of the job (wave and stride in whole waves; all 64 lanes of a wave call it)
template <typename Keep, typename Prune = NoPrune>
__device__ __forceinline__ void deepen_probe(const SymBallView &b, const DeepenJob &job, const SymProbe &c, size_t wave, size_t stride, const Keep &keep,
                                             const Prune &prune = Prune{})
{
	[[maybe_unused]] unsigned long long lookups = 0;                     // (PdbPrune: the sb_node calls of this wave)
	const u32x4 *s_act = c.s_act;
	const int e = job.extra;
	const uint32_t span = deepen_span(e);
	const unsigned long long end = (unsigned long long)job.word_first + job.word_count;
	const uint32_t g_first = job.word_first / span;
	const uint32_t ng = deepen_groups(e, job.word_first, job.word_count);
	const size_t items = job.n * (size_t)ng;
	for (size_t w = wave; w < items; w += stride) {
		const size_t i = w / ng;
		const uint32_t g = g_first + (uint32_t)(w - i * ng);
		// (one address for the whole wave: through readfirstlane, so that everything that depends on them is scalar)
		const int last = job.last != nullptr && (long long)i != job.no_last ? deepen_last(__builtin_amdgcn_readfirstlane((int)job.last[i])) : -1;
		const uint32_t n0 = last < 0 ? 12u : 11u;
		const long long best = keep.limit(i);
		const long long base = (long long)g * span;
		const long long lo = max((long long)job.word_first, base), hi = min((long long)end, base + span);
		if (lo > best) continue;
		uint32_t s[5];
		load5(job.states + i * 5, s);
		int prev = last;
		bool exists = true;
		if constexpr (Prune::on)
			if (prune.left_uniform(s, e)) continue;                      // nothing of the ball within e moves of the state
		if (e >= 3) {                                                    // the shared moves: the digits of g
			uint32_t rem = g;
			for (int k = 0; k < e - 2; k++) {
				const uint32_t p = deepen_pow11(e - 3 - k);
				const uint32_t d = rem / p;
				rem -= d * p;
				if (k == 0 && d >= n0) { exists = false; break; }
				prev = deepen_action(prev, (int)d);
				uint32_t t[5];
				deepen_move(s_act, prev, s, t);
				#pragma unroll
				for (int j = 0; j < 5; j++) s[j] = t[j];
				if constexpr (Prune::on)
					if (prune.left_uniform(s, e - 1 - k)) { exists = false; break; }      // nor within the e - (k + 1) moves still to make
			}
		}
		if (!exists) continue;
		const uint32_t cm = e >= 3 ? 11u : e == 2 ? n0 : 1u;             // next-to-last moves, last moves
		const uint32_t cl = e >= 2 ? 11u : n0;
		if constexpr (Prune::on) {
			deepen_pairs_pruned(b, c, prune, keep, i, e, s, prev, cm, cl, base, lo, hi, best, lookups);
			continue;
		}
		bool hit = false;
		for (uint32_t dm = 0; dm < cm && !hit; dm++) {
			const long long r0 = base + (long long)dm * cl;
			if (r0 >= hi || r0 > best) break;
			if (r0 + cl <= lo) continue;
			uint32_t s1[5];
			int p1 = prev;
			if (e >= 2) {
				p1 = deepen_action(prev, (int)dm);
				deepen_move(s_act, p1, s, s1);
			} else {
				#pragma unroll
				for (int j = 0; j < 5; j++) s1[j] = s[j];
			}
			for (uint32_t dl = 0; dl < cl; dl++) {
				const long long r = r0 + dl;
				if (r < lo) continue;
				if (r >= hi || r > best) break;
				uint32_t s2[5];
				deepen_move(s_act, deepen_action(p1, (int)dl), s1, s2);
				if (sb_node(b, c, s2) != 0u) {                           // (the same in every lane)
					if (c.lane == 0) keep.lower(i, (uint32_t)r);
					hit = true;                                          // every later rank of the item is above r
					break;
				}
			}
		}
	}
	if constexpr (Prune::on)
		if (prune.lookups != nullptr && c.lane == 0 && lookups != 0ull) atomicAdd(prune.lookups, lookups);
}

}  // namespace rk
