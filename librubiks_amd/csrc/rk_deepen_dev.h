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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rk_device.h"
#include "rk_search_dev.h"
#include "rk_sym_dev.h"

namespace rk {

constexpr int DEEPEN_MAX_EXTRA = 8;
constexpr uint32_t DEEPEN_NONE = 0xFFFFFFFFu;       // d_best of a state without a hit
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

struct DeepenJob {
	const uint32_t *states;                     // (n, 5) dwords
	const int8_t *last;                         // (n) or null: the action that led to each state, anything outside 0..11 for none
	long long no_last;                          // the one row whose stored action is no action (a pool's node 1), -1: none
	size_t n;
	int extra;
	uint32_t word_first, word_count;
	uint32_t *best;                             // (n): atomicMin of the ranks that hit
};

__device__ __forceinline__ void deepen_move(const u32x4 *s_act, int a, const uint32_t in[5], uint32_t out[5])
{
	uint32_t tab[12];
	#pragma unroll
	for (int j = 0; j < 5; j++) out[j] = in[j];
	load_action_table(s_act, (uint32_t)a, tab);
	move5(out, tab);
}

// the items wave, wave + stride, ... of the job (wave and stride in whole waves; all 64 lanes of a wave call it)
__device__ __forceinline__ void deepen_probe(const SymBallView &b, const DeepenJob &job, const SymProbe &c, size_t wave, size_t stride)
{
	const u32x4 *s_act = c.s_act;
	const int e = job.extra;
	const uint32_t span = e >= 3 ? DEEPEN_SPAN : 132u;                   // (extra <= 2: every rank is below 132)
	const unsigned long long end = (unsigned long long)job.word_first + job.word_count;
	const uint32_t g_first = job.word_first / span;
	const uint32_t ng = (uint32_t)((end - 1) / span) - g_first + 1u;
	const size_t items = job.n * (size_t)ng;
	for (size_t w = wave; w < items; w += stride) {
		const size_t i = w / ng;
		const uint32_t g = g_first + (uint32_t)(w - i * ng);
		// (one address for the whole wave: through readfirstlane, so that everything that depends on them is scalar)
		const int last = job.last != nullptr && (long long)i != job.no_last ? deepen_last(__builtin_amdgcn_readfirstlane((int)job.last[i])) : -1;
		const uint32_t n0 = last < 0 ? 12u : 11u;
		const uint32_t best =
			(uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&job.best[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
		const unsigned long long base = (unsigned long long)g * span;
		const unsigned long long lo = max((unsigned long long)job.word_first, base), hi = min(end, base + span);
		if (lo > best) continue;
		uint32_t s[5];
		load5(job.states + i * 5, s);
		int prev = last;
		bool exists = true;
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
			}
		}
		if (!exists) continue;
		const uint32_t cm = e >= 3 ? 11u : e == 2 ? n0 : 1u;             // next-to-last moves, last moves
		const uint32_t cl = e >= 2 ? 11u : n0;
		bool hit = false;
		for (uint32_t dm = 0; dm < cm && !hit; dm++) {
			const unsigned long long r0 = base + (unsigned long long)dm * cl;
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
				const unsigned long long r = r0 + dl;
				if (r < lo) continue;
				if (r >= hi || r > best) break;
				uint32_t s2[5];
				deepen_move(s_act, deepen_action(p1, (int)dl), s1, s2);
				if (sb_node(b, c, s2) != 0u) {                           // (the same in every lane)
					if (c.lane == 0) atomicMin(&job.best[i], (uint32_t)r);
					hit = true;                                          // every later rank of the item is above r
					break;
				}
			}
		}
	}
}

}  // namespace rk
