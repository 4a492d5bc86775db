// Two-phase search (rk_twophase_*): short solutions for every legal state by IDA* into the subgroup H = <F, B, TT, DD, LL, RR>, then
// IDA* inside it -- no pool, no net.  H is the subgroup the chain's stage 3 starts in, so phase 1 = the chain's stages 1 + 2 and
// phase 2 = its stages 3 + 4, and the chain's own answer (launch 1, the unchanged rk_chain_solve) is every row's first best.
//
// COORDINATES, all BY POSITION and all taken from rk_chain_dev.h (include/rubiks_hip.h states them):
//     phase 1   twist = chain_index<1> / 495 (2 187)   flip = chain_index<0> (2 048)            slice = chain_index<1> % 495 (495)
//     phase 2   corners = chain_corner_rank (40 320)   edges = tp_edges8 (40 320, below)        places = chain_places<0> (24)
// A move's effect on a coordinate depends on the coordinate alone, so the search steps coordinates through six u16 move tables
// built at create (phase 1: 12 columns, the actions; phase 2: 8 columns, the generators F F' B B' TT DD LL RR of the chain's stage
// 3 in its order) and reads two one-byte pruning tables per child: 2 dependent loads per child instead of a 20-byte move and four
// index computations.  The tables (4 MB of pruning, 1.7 MB of moves) are meant to live in L2 / Infinity Cache.
//
// THE MOVE-PRUNING RULE (both phases; a generator is named by its action a, face a >> 1, the half turns of phase 2 by the even
// action; `last` and `last2` are the two generators before it IN THE SAME PHASE, none at a phase's start).  Generator a is skipped
//     1. if a == last ^ 1                                  (the immediate inverse),
//     2. if its face is the lower one of last's axis, (a >> 1) == (last >> 1) - 1 with last's face odd: opposite faces commute and
//        are taken lower face first,
//     3. if a == last and a is odd                         (X'X' = XX, kept as XX),
//     4. if a == last == last2                             (XXX = X'),
//     5. if a == last and a is a half turn of phase 2      (its own inverse).
// Every cheapest word can be brought into this form without growing (sort each run on one axis lower face first, write a face's
// run as X, X', XX or the half turn), so a cheapest word per element survives and each phase's first solution is optimal for it.
// Children are taken in ascending order of a.
//
// THE SEARCH of one state (tests/twophase_model.py restates it):
//     best = the chain's length L; D = the phase-1 entry of the state (the greater of its two tables)
//     while D < best: depth-first over phase-1 words of exactly D generators (child kept if depth + its entry <= D);
//         every such word ends in H and is a PHASE-1 SOLUTION, p1 = D:  found += 1; the state behind it is formed from the 20 bytes,
//         its phase-2 entry h2 read; for D2 = h2, h2 + 1, .. best - p1 - 1: depth-first over phase-2 words of cost <= D2 (child kept
//         if cost + its entry <= D2); the first child whose entry is 0 is solved: best = p1 + cost, the row is rewritten, phase 2 ends.
//         After phase 2 (solved or exhausted): stop if found == tries or D >= best, else phase 1 goes on behind that word.
//         D += 1 when the depth-first pass is exhausted.
//     WITH A CAP C ON THE PHASE-2 BOUND (rk_twophase_solve_capped, tests/twophase_cap_model.py) two conditions change and nothing
//     else: a phase-1 solution with h2 != 0 is left behind -- phase 1 goes on -- if p1 + h2 >= best OR h2 > C; and after D2 += 1
//     phase 1 goes on if p1 + D2 >= best OR D2 > C.  found still counts every phase-1 solution, h2 == 0 still ends the search.
// THE BUDGET RULE.  A node is one child evaluation: a generator that the move-pruning rule lets through at the current node, its
// three coordinates stepped and its two entries read, in either phase.  Immediately BEFORE each evaluation the state's counter is
// compared with max_nodes: if equal, the state's search ends there (reason 1 or 2); otherwise the counter goes up by one and the
// child is evaluated.  Root entries, pops, restarts and the replay of the chain's row count nothing.  So the answer is a function
// of (state, tries, max_nodes) alone -- with a cap, of (state, tries, max_nodes, C).
//
// THE KERNEL is one persistent grid of at most RK_TWOPHASE_GRID workgroups of 256.  A lane owns one state and runs the explicit-
// stack depth-first search as a UNIFORM loop: per trip one child (or one pop, or one move of the chain's row) per lane, by
// predication -- divergence costs branches, not serialised subtrees.  A lane that finishes takes the next row from a device
// counter (one atomic per wave and refill); which lane gets which row influences no output.  The stack holds generators only, a
// byte per entry in LDS (72 x 256 B per workgroup); coordinates are not stacked: a pop steps them through the inverse generator's
// column.  Vector stores only; the one atomic is the row counter.  The kernel is a template: k_twophase_search<false> is the search
// without a cap and without counts, the code rk_twophase_solve has always run; <true> compares with the cap (0xFFFFFFFF: none),
// counts the phase-2 searches it enters and writes the two counts of a row at its end.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_chain_dev.h"
#include "rk_error.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"
#include "rk_table_host.h"

namespace rk {

constexpr int TP_TABLES = 4, TP_MOVES = 6;
constexpr uint32_t TP_THREADS = 256;
constexpr uint32_t TP_STACK = 72;                       // generators a row's words can hold: max_length <= 70 is checked
constexpr uint32_t TP_TWIST = 2187, TP_FLIP = 2048, TP_SLICE = 495, TP_PLACES = 24;
constexpr uint32_t TP_SIZE[TP_TABLES] = {TP_TWIST * TP_SLICE, TP_FLIP * TP_SLICE, CHAIN_PERMS * TP_PLACES, CHAIN_PERMS * TP_PLACES};
constexpr uint32_t TP_COUNT[TP_TABLES] = {1082565u, 1013760u, 967680u, 967680u};
// move tables: twist, flip, slice (12 columns), corners, edges, places (8 columns)
constexpr uint32_t TP_MT_ROWS[TP_MOVES] = {TP_TWIST, TP_FLIP, TP_SLICE, CHAIN_PERMS, CHAIN_PERMS, TP_PLACES};
constexpr uint32_t TP_MT_COLS[TP_MOVES] = {12, 12, 12, 8, 8, 8};
constexpr uint32_t TP_PHASE2_ACTIONS = 0x55Fu;           // F F' B B' and the even action of T D L R

// the kernel's column rule for phase 2 (action a < 4: column a, else 2 + a / 2) and its face pairing, checked against the tables
constexpr bool tp_consistent()
{
	if (CHAIN.gen_count[2] != 8) return false;
	for (int j = 0; j < 8; j++) {
		if (CHAIN.gen_action[2][j] != (j < 4 ? j : 2 * (j - 2))) return false;
		if (CHAIN.gen_cost[2][j] != (j < 4 ? 1 : 2)) return false;
	}
	if (CHAIN.gen_count[0] != 12) return false;
	const Tables t = make_tables();
	for (int f = 0; f < 6; f += 2)                       // faces f and f + 1 commute
		for (int k = 0; k < 2; k++)
			for (int v = 0; v < 24; v++)
				if (t.lut[2 * f][k][t.lut[2 * f + 2][k][v]] != t.lut[2 * f + 2][k][t.lut[2 * f][k][v]]) return false;
	for (int a = 0; a < 12; a++)                         // a ^ 1 is a's inverse
		for (int k = 0; k < 2; k++)
			for (int v = 0; v < 24; v++)
				if (t.lut[a ^ 1][k][t.lut[a][k][v]] != v) return false;
	return true;
}
static_assert(tp_consistent(), "the move table does not give the generators and face pairs the two-phase kernel assumes");

// the lexicographic rank of the sequence (place of the i-th edge outside slice 0 among the eight positions outside slice 0)
__host__ __device__ __forceinline__ uint32_t tp_edges8(const uint32_t x[5])
{
	uint32_t r = 0, seen = 0;
	#pragma unroll
	for (int i = 0; i < 8; i++) {
		const uint32_t pos = (CHAIN_BYTE(x, 8 + ((CHAIN_OUTSIDE0 >> (4 * i)) & 15u)) >> 1) & 15u;
		const uint32_t place = chain_popc(0xFFFu & ~CHAIN_SLICE_MASK<0> & ((1u << pos) - 1u)) & 7u, bit = 1u << place;
		r = r * (uint32_t)(8 - i) + place - chain_popc(seen & (bit - 1u));
		seen |= bit;
	}
	return r;
}

struct TpDev {
	const uint8_t *prune[TP_TABLES];
	const uint16_t *mt[TP_MOVES];
	uint32_t goal_twist, goal_flip, goal_slice;
};

enum : uint32_t { TP_IDLE = 0, TP_REPLAY, TP_SEARCH, TP_SOL1, TP_DONE };
constexpr uint32_t TP_IMPROVED = 1u, TP_BUDGET = 2u;

__device__ __forceinline__ uint32_t tp_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

template <bool EXT>                                                 // EXT: the cap on the phase-2 bound and the two counts per row
__global__ __launch_bounds__(TP_THREADS)
void k_twophase_search(TpDev dv, const uint32_t *states, uint32_t n, uint32_t stride, uint32_t tries, unsigned long long max_nodes,
                       int32_t *lengths, int8_t *actions, int32_t *phase_lengths, int32_t *reason, long long *nodes_out, uint32_t *counter,
                       uint32_t cap, int32_t *counts)
{
	__shared__ u32x4 s_tab[36];
	__shared__ uint8_t s_stack[TP_STACK * TP_THREADS];              // entry e of this lane: s_stack[e * 256 + tid]
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	stage_action_tables(s_tab, (int)tid);
	__syncthreads();

	uint32_t mode = TP_IDLE, q = 0, c0 = 0, c1 = 0, c2 = 0;         // the row; the three coordinates of the current phase
	uint32_t root = 0, root2 = 0, root2p = 0, leaf = 0;             // packed coordinates: phase-1 root, phase-2 root (and its places), the phase-1 word's end
	uint32_t phase = 1, depth = 0, cost = 0, g = 0;                 // generators and cost behind the current node; the next action to try
	uint32_t D = 0, D2 = 0, best = 0, p1 = 0, bp1 = 0, found = 0, flags = 0, t = 0;
	unsigned long long nodes = 0;
	uint32_t entered = 0;                                           // EXT: the phase-2 searches of this row

	// the end of a state's search
	const auto finish = [&]() {
		lengths[q] = (int32_t)best;
		phase_lengths[2 * (size_t)q] = (int32_t)bp1;
		phase_lengths[2 * (size_t)q + 1] = (int32_t)(best - bp1);
		reason[q] = (flags & TP_IMPROVED) == 0u ? 2 : (flags & TP_BUDGET) != 0u ? 1 : 0;
		nodes_out[q] = (long long)nodes;
		if constexpr (EXT) {
			if (counts) {
				counts[2 * (size_t)q] = (int32_t)found;
				counts[2 * (size_t)q + 1] = (int32_t)entered;
			}
		}
		mode = TP_IDLE;
	};
	// after phase 2: phase 1 goes on behind the word that ended at `leaf` (its next trip pops), unless the search is over
	const auto resume1 = [&]() {
		if (found == tries || D >= best) {
			finish();
			return;
		}
		phase = 1;
		c0 = leaf & 4095u; c1 = (leaf >> 12) & 2047u; c2 = leaf >> 23;
		depth = D; cost = D; g = 12;
		mode = TP_SEARCH;
	};
	// the row: the first `entries` generators of the stack, a half turn of phase 2 twice, then -1 up to the length it had
	const auto write_row = [&](uint32_t entries, uint32_t old_length) {
		int8_t *row = actions + (size_t)q * stride;
		uint32_t w = 0;
		for (uint32_t e = 0; e < entries && e < TP_STACK && w < stride; e++) {
			const uint32_t a = s_stack[e * TP_THREADS + tid];
			row[w++] = (int8_t)a;
			if (e >= p1 && a >= 4u && w < stride) row[w++] = (int8_t)a;
		}
		for (; w < old_length && w < stride; w++) row[w] = (int8_t)-1;
	};

	for (;;) {
		// ---- a lane without a state takes the next row: one atomic per wave and refill ----
		if (mode == TP_IDLE) {
			const unsigned long long need = __ballot(1);
			uint32_t base = 0;
			if (lane == (uint32_t)__builtin_ctzll(need)) base = atomicAdd(counter, (uint32_t)__popcll(need));
			base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
			const unsigned long long at = (unsigned long long)base + (unsigned long long)__popcll(need & ((1ull << lane) - 1ull));
			if (at >= (unsigned long long)n) {
				mode = TP_DONE;
			} else {
				q = (uint32_t)at;
				const int32_t L = lengths[q];
				if (L < 0 || (uint32_t)L > stride) {                        // no legal state (launch 1): nothing is searched
					phase_lengths[2 * (size_t)q] = -1;
					phase_lengths[2 * (size_t)q + 1] = -1;
					reason[q] = 2;
					nodes_out[q] = 0;
					if constexpr (EXT) {
						if (counts) {
							counts[2 * (size_t)q] = 0;
							counts[2 * (size_t)q + 1] = 0;
						}
					}
				} else {
					uint32_t x[5];
					load5(states + (size_t)q * 5, x);
					const uint32_t i1 = min(chain_index<1>(x, nullptr, nullptr), TP_SIZE[0] - 1u);
					c1 = chain_index<0>(x, nullptr, nullptr);
					c0 = i1 / TP_SLICE;
					c2 = i1 - c0 * TP_SLICE;
					root = c0 | c1 << 12 | c2 << 23;
					D = tp_max(dv.prune[0][i1], dv.prune[1][c1 * TP_SLICE + c2]);
					best = (uint32_t)L;
					nodes = 0; found = 0; flags = 0; t = 0; phase = 1;
					if constexpr (EXT) entered = 0;
					mode = TP_REPLAY;
				}
			}
		}
		// ---- a phase-1 solution: the state behind the word, its phase-2 coordinates and entry ----
		if (mode == TP_SOL1) {
			found++;
			uint32_t x[5];
			load5(states + (size_t)q * 5, x);
			for (uint32_t e = 0; e < p1 && e < TP_STACK; e++) {
				uint32_t tab[12];
				load_action_table(s_tab, min((uint32_t)s_stack[e * TP_THREADS + tid], 11u), tab);
				move5(x, tab);
			}
			const uint32_t cp = min(chain_corner_rank(x), CHAIN_PERMS - 1u), ep = min(tp_edges8(x), CHAIN_PERMS - 1u);
			const uint32_t sp = min(chain_places<0>(x), TP_PLACES - 1u);
			const uint32_t h2 = tp_max(dv.prune[2][cp * TP_PLACES + sp], dv.prune[3][ep * TP_PLACES + sp]);
			if (h2 == 0u) {                                                 // the word solves the state (p1 < best: D < best)
				const uint32_t old = best;
				best = p1; bp1 = p1; flags |= TP_IMPROVED;
				write_row(p1, old);
				finish();
			} else if (p1 + h2 >= best || (EXT && h2 > cap)) {              // nothing below best behind this word, or only past the cap
				resume1();
			} else {
				if constexpr (EXT) entered++;
				phase = 2;
				root2 = cp | ep << 16;
				c0 = cp; c1 = ep; c2 = sp;
				root2p = sp;
				depth = 0; cost = 0; g = 0; D2 = h2;
				mode = TP_SEARCH;
			}
		}
		// ---- one trip: a child, a pop, or one move of the chain's row ----
		bool step = false, child = false;
		uint32_t a = 0, col = 0;
		if (mode == TP_REPLAY) {
			if ((c0 == dv.goal_twist && c1 == dv.goal_flip && c2 == dv.goal_slice) || t >= best) {
				bp1 = t;                                                    // the chain's stages 1 + 2: its row's first prefix that ends in H
				c0 = root & 4095u; c1 = (root >> 12) & 2047u; c2 = root >> 23;
				depth = 0; cost = 0; g = 0;
				if (D >= best) {                                            // no phase-1 word below best
					finish();
				} else if (D == 0u) {                                       // the state is in H: the empty word is the first phase-1 solution
					p1 = 0; leaf = root;
					mode = TP_SOL1;
				} else {
					mode = TP_SEARCH;
				}
			} else {
				a = min((uint32_t)(uint8_t)actions[(size_t)q * stride + t], 11u);
				col = a;
				step = true;
			}
		} else if (mode == TP_SEARCH) {
			const uint32_t base = phase == 2u ? p1 : 0u;
			const uint32_t e1 = min(base + depth - 1u, TP_STACK - 1u), e2 = min(base + depth - 2u, TP_STACK - 1u);
			const uint32_t last = depth > 0u ? (uint32_t)s_stack[e1 * TP_THREADS + tid] : 0xFFu;
			const uint32_t last2 = depth > 1u ? (uint32_t)s_stack[e2 * TP_THREADS + tid] : 0xFFu;
			uint32_t mask = phase == 2u ? TP_PHASE2_ACTIONS : 0xFFFu;
			if (last != 0xFFu) {
				mask &= ~(1u << (last ^ 1u));
				if (last & 2u) mask &= ~(3u << ((last & ~3u)));             // last's face is odd: not the lower face of its axis
				if ((last & 1u) != 0u || last2 == last || (phase == 2u && last >= 4u)) mask &= ~(1u << last);
			}
			mask &= ~((1u << g) - 1u);
			if (mask != 0u) {
				if (nodes == max_nodes) {
					flags |= TP_BUDGET;
					finish();
				} else {
					nodes++;
					a = (uint32_t)__builtin_ctz(mask);
					col = phase == 2u && a >= 4u ? 2u + (a >> 1) : a;
					step = child = true;
				}
			} else if (depth > 0u) {                                        // pop: through the inverse generator's column
				a = last;
				const uint32_t inv = phase == 2u && a >= 4u ? a : a ^ 1u;
				col = phase == 2u && inv >= 4u ? 2u + (inv >> 1) : inv;
				step = true;
			} else if (phase == 2u) {                                       // this bound is exhausted
				D2++;
				if (p1 + D2 >= best || (EXT && D2 > cap)) {
					resume1();
				} else {
					c0 = root2 & 0xFFFFu; c1 = root2 >> 16; c2 = root2p;
					g = 0;
				}
			} else {
				D++;
				if (D >= best) {
					finish();
				} else {
					c0 = root & 4095u; c1 = (root >> 12) & 2047u; c2 = root >> 23;
					g = 0;
				}
			}
		}
		if (step) {
			const bool two = phase == 2u;
			const uint32_t W = two ? 8u : 12u;
			const uint32_t n0 = (two ? dv.mt[3] : dv.mt[0])[c0 * W + col];
			const uint32_t n1 = (two ? dv.mt[4] : dv.mt[1])[c1 * W + col];
			const uint32_t n2 = (two ? dv.mt[5] : dv.mt[2])[c2 * W + col];
			const uint32_t ca = two && a >= 4u ? 2u : 1u;
			if (mode == TP_REPLAY) {
				c0 = n0; c1 = n1; c2 = n2;
				t++;
			} else if (!child) {
				c0 = n0; c1 = n1; c2 = n2;
				depth--; cost -= ca; g = a + 1u;
			} else {
				const uint32_t K = two ? TP_PLACES : TP_SLICE;
				const uint32_t ia = min(n0 * K + n2, (two ? TP_SIZE[2] : TP_SIZE[0]) - 1u), ib = min(n1 * K + n2, (two ? TP_SIZE[3] : TP_SIZE[1]) - 1u);
				const uint32_t h = tp_max((two ? dv.prune[2] : dv.prune[0])[ia], (two ? dv.prune[3] : dv.prune[1])[ib]);
				if (cost + ca + h <= (two ? D2 : D)) {
					// entries <= cost <= best - 1 < max_length <= TP_STACK - 2
					s_stack[min((two ? p1 : 0u) + depth, TP_STACK - 1u) * TP_THREADS + tid] = (uint8_t)a;
					c0 = n0; c1 = n1; c2 = n2;
					depth++; cost += ca; g = 0;
					if (!two) {
						if (cost == D) {                                    // depth D: its entry is 0, the word ends in H
							p1 = D;
							leaf = c0 | c1 << 12 | c2 << 23;
							mode = TP_SOL1;
						}
					} else if (h == 0u) {                                   // solved, p1 + cost < best
						const uint32_t old = best;
						best = p1 + cost; bp1 = p1; flags |= TP_IMPROVED;
						write_row(p1 + depth, old);
						resume1();
					}
				} else {
					g = a + 1u;
				}
			}
		}
		if (__all(mode == TP_DONE)) break;
	}
}

}  // namespace rk

using namespace rk;

struct rk_twophase {
	TpDev d{};
	uint8_t *d_block = nullptr;                         // the four pruning tables, the six move tables, the row counter: one allocation
	uint32_t *d_counter = nullptr;
	long long counts[TP_TABLES] = {};
	int deepest[TP_TABLES] = {};
	~rk_twophase()
	{
		if (d_block) (void)hipFree(d_block);
	}
};

namespace {

unsigned tp_grid(size_t n) { return (unsigned)std::min<size_t>((n + TP_THREADS - 1) / TP_THREADS, (size_t)RK_TWOPHASE_GRID); }

// column `col` of a phase's move tables: an action, or a generator of the chain's stage 3
HostState tp_column(const HostState &s, bool two, int col)
{
	return two ? host_generate(s, CHAIN.gen_action[2][col], CHAIN.gen_cost[2][col]) : host_move(s, col);
}

uint32_t tp_coordinate(int which, const HostState &s)
{
	const uint32_t *x = s.data();
	switch (which) {
	case 0: return chain_index<1>(x, nullptr, nullptr) / TP_SLICE;
	case 1: return chain_index<0>(x, nullptr, nullptr);
	case 2: return chain_index<1>(x, nullptr, nullptr) % TP_SLICE;
	case 3: return chain_corner_rank(x);
	case 4: return tp_edges8(x);
	default: return chain_places<0>(x);
	}
}

// One representative state per value of coordinate `which`: a closure from solved under the phase's generators, so every
// representative is a legal state (a digit or a place that the coordinate leaves out is the one the others force).  false: a value
// is out of range or not every value is reached.
bool tp_representatives(int which, std::vector<HostState> &reps)
{
	const uint32_t rows = TP_MT_ROWS[which];
	const HostState solved = host_solved();
	reps.assign(rows, solved);
	std::vector<uint8_t> have(rows, 0);
	std::vector<HostState> todo{solved};
	uint32_t v = tp_coordinate(which, solved), count = 1;
	if (v >= rows) return false;
	have[v] = 1;
	while (!todo.empty()) {
		const HostState s = todo.back();
		todo.pop_back();
		for (uint32_t col = 0; col < TP_MT_COLS[which]; col++) {
			const HostState c = tp_column(s, which >= 3, (int)col);
			v = tp_coordinate(which, c);
			if (v >= rows) return false;
			if (have[v]) continue;
			have[v] = 1;
			reps[v] = c;
			todo.push_back(c);
			count++;
		}
	}
	return count == rows;
}

bool tp_move_table(int which, std::vector<uint16_t> &mt)
{
	std::vector<HostState> reps;
	if (!tp_representatives(which, reps)) return false;
	const uint32_t cols = TP_MT_COLS[which];
	mt.assign((size_t)TP_MT_ROWS[which] * cols, 0);
	for (uint32_t v = 0; v < TP_MT_ROWS[which]; v++)
		for (uint32_t col = 0; col < cols; col++) {
			const uint32_t to = tp_coordinate(which, tp_column(reps[v], which >= 3, (int)col));
			if (to >= TP_MT_ROWS[which]) return false;
			mt[(size_t)v * cols + col] = (uint16_t)to;
		}
	return true;
}

// One pruning table over the pairs (a, b), index a * K + b: build_cost_table (rk_table_host.h) on the indices themselves, a child
// stepped through the two move tables.  Returns the deepest entry, -1 unless exactly TP_COUNT[table] entries were reached and one
// of them is 0.
int tp_build(int table, const std::vector<uint16_t> &mta, const std::vector<uint16_t> &mtb, uint32_t goal, std::vector<uint8_t> &out, long long &count)
{
	const bool two = table >= 2;
	const uint32_t K = two ? TP_PLACES : TP_SLICE, cols = two ? 8 : 12;
	const uint8_t quarter_turns[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
	const uint16_t *ma = mta.data(), *mb = mtb.data();
	return build_cost_table(
		out, TP_SIZE[table], (long long)TP_COUNT[table], (int)cols, two ? CHAIN.gen_cost[2] : quarter_turns, goal,
		[=](uint32_t index, int col) {
			const uint32_t a = index / K, b = index - a * K;
			return (uint32_t)ma[(size_t)a * cols + col] * K + mb[(size_t)b * cols + col];
		},
		[](uint32_t index) { return index; }, count);
}

// Both solve entries: phase2_cap <= 0 is no cap, d_counts may be null; without either the launch is k_twophase_search<false>.
int tp_solve(const char *who, rk_twophase_t *h, rk_chain_t *chain, const int8_t *d_states, size_t n, int tries, long long max_nodes, int phase2_cap,
             int32_t *d_lengths, int8_t *d_actions, int32_t *d_phase_lengths, int32_t *d_reason, long long *d_nodes, int32_t *d_counts,
             int32_t *d_error, void *stream)
{
	if (!h || !chain) return fail(RK_EINVAL, "%s: null handle", who);
	if (tries < 1 || max_nodes < 1) return fail(RK_EINVAL, "%s: tries %d and max_nodes %lld must be at least 1", who, tries, max_nodes);
	if (phase2_cap > (int)TP_STACK - 2) return fail(RK_EINVAL, "%s: phase2_cap %d is above the longest row, %u", who, phase2_cap, TP_STACK - 2);
	if (int e = check_state_rows(who, d_states, n)) return e;
	if (n != 0 && (!d_lengths || !d_actions || !d_phase_lengths || !d_reason || !d_nodes)) return fail(RK_EINVAL, "%s: null pointer", who);
	if (((uintptr_t)d_lengths | (uintptr_t)d_phase_lengths | (uintptr_t)d_reason | (uintptr_t)d_counts | (uintptr_t)d_error) & 3u)
		return fail(RK_EINVAL, "%s: device pointers must be 4-byte aligned", who);
	if ((uintptr_t)d_nodes & 7u) return fail(RK_EINVAL, "%s: d_nodes must be 8-byte aligned", who);
	long long chain_status[16];
	if (int e = rk_chain_status(chain, chain_status)) return e;
	const long long stride = chain_status[8];
	if (stride < 1 || stride > (long long)TP_STACK - 2)
		return fail(RK_ESTATE, "%s: the chain's rows are %lld wide, the search's stack holds %u", who, stride, TP_STACK - 2);
	if (n == 0) return RK_OK;
	hipStream_t st = (hipStream_t)stream;
	// launch 1: the chain's answer into the output rows
	if (int e = rk_chain_solve(chain, d_states, n, d_lengths, d_actions, nullptr, d_error, stream)) return e;
	// launch 2: the search
	RK_HIP(hipMemsetAsync(h->d_counter, 0, sizeof(uint32_t), st));
	const bool ext = phase2_cap > 0 || d_counts != nullptr;
	hipLaunchKernelGGL(ext ? k_twophase_search<true> : k_twophase_search<false>, dim3(tp_grid(n)), dim3(TP_THREADS), 0, st, h->d,
	                   reinterpret_cast<const uint32_t *>(d_states), (uint32_t)n, (uint32_t)stride, (uint32_t)tries, (unsigned long long)max_nodes,
	                   d_lengths, d_actions, d_phase_lengths, d_reason, d_nodes, h->d_counter, phase2_cap > 0 ? (uint32_t)phase2_cap : 0xFFFFFFFFu,
	                   d_counts);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

}  // namespace

extern "C" {

int rk_twophase_create(rk_twophase_t **out, void *stream)
{
	if (!out) return fail(RK_EINVAL, "rk_twophase_create: null out pointer");
	std::vector<uint16_t> mt[TP_MOVES];
	for (int w = 0; w < TP_MOVES; w++)
		if (!tp_move_table(w, mt[w])) return fail(RK_ESTATE, "rk_twophase_create: coordinate %d does not take every value under its generators", w);
	const HostState solved = host_solved();
	uint32_t goal[TP_MOVES];
	for (int w = 0; w < TP_MOVES; w++) goal[w] = tp_coordinate(w, solved);
	rk_twophase *h = new rk_twophase();
	std::vector<uint8_t> table[TP_TABLES];
	h->deepest[0] = tp_build(0, mt[0], mt[2], goal[0] * TP_SLICE + goal[2], table[0], h->counts[0]);
	h->deepest[1] = tp_build(1, mt[1], mt[2], goal[1] * TP_SLICE + goal[2], table[1], h->counts[1]);
	h->deepest[2] = tp_build(2, mt[3], mt[5], goal[3] * TP_PLACES + goal[5], table[2], h->counts[2]);
	h->deepest[3] = tp_build(3, mt[4], mt[5], goal[4] * TP_PLACES + goal[5], table[3], h->counts[3]);
	for (int s = 0; s < TP_TABLES; s++)
		if (h->deepest[s] < 0) {
			const long long got = h->counts[s];
			delete h;
			return fail(RK_ESTATE, "rk_twophase_create: pruning table %d reached %lld entries, not %u with one goal", s + 1, got, TP_COUNT[s]);
		}
	TableBlock block;                                                   // the pruning tables, the move tables, the row counter
	for (int s = 0; s < TP_TABLES; s++) block.add(table[s].data(), TP_SIZE[s]);
	for (int w = 0; w < TP_MOVES; w++) block.add(mt[w].data(), mt[w].size() * sizeof(uint16_t));
	block.add_zeros(16);
	if (int e = block.upload("rk_twophase_create", (hipStream_t)stream)) {
		delete h;
		return e;
	}
	for (int s = 0; s < TP_TABLES; s++) h->d.prune[s] = block.at(s);
	for (int w = 0; w < TP_MOVES; w++) h->d.mt[w] = block.at<uint16_t>(TP_TABLES + w);
	h->d_counter = block.at<uint32_t>(TP_TABLES + TP_MOVES);
	h->d_block = block.release();
	h->d.goal_twist = goal[0];
	h->d.goal_flip = goal[1];
	h->d.goal_slice = goal[2];
	*out = h;
	return RK_OK;
}

int rk_twophase_destroy(rk_twophase_t *h)
{
	delete h;
	return RK_OK;
}

int rk_twophase_status(rk_twophase_t *h, long long *h_status)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_twophase_status: null argument");
	memset(h_status, 0, 16 * sizeof(long long));
	for (int s = 0; s < TP_TABLES; s++) {
		h_status[s] = h->counts[s];
		h_status[4 + s] = (long long)h->deepest[s];
		h_status[8 + s] = (long long)TP_SIZE[s];
	}
	h_status[12] = RK_TWOPHASE_GRID;
	h_status[13] = TP_THREADS;
	h_status[14] = TP_STACK - 2;
	return RK_OK;
}

int rk_twophase_export(rk_twophase_t *h, int table, size_t first, size_t count, uint8_t *h_bytes, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_twophase_export: null handle");
	return export_table("rk_twophase_export", "table", table, TP_TABLES, h->d.prune, TP_SIZE, first, count, h_bytes, stream);
}

int rk_twophase_solve(rk_twophase_t *h, rk_chain_t *chain, const int8_t *d_states, size_t n, int tries, long long max_nodes, int32_t *d_lengths,
                      int8_t *d_actions, int32_t *d_phase_lengths, int32_t *d_reason, long long *d_nodes, int32_t *d_error, void *stream)
{
	return tp_solve("rk_twophase_solve", h, chain, d_states, n, tries, max_nodes, 0, d_lengths, d_actions, d_phase_lengths, d_reason, d_nodes, nullptr,
	                d_error, stream);
}

int rk_twophase_solve_capped(rk_twophase_t *h, rk_chain_t *chain, const int8_t *d_states, size_t n, int tries, long long max_nodes, int phase2_cap,
                             int32_t *d_lengths, int8_t *d_actions, int32_t *d_phase_lengths, int32_t *d_reason, long long *d_nodes,
                             int32_t *d_counts, int32_t *d_error, void *stream)
{
	return tp_solve("rk_twophase_solve_capped", h, chain, d_states, n, tries, max_nodes, phase2_cap, d_lengths, d_actions, d_phase_lengths, d_reason,
	                d_nodes, d_counts, d_error, stream);
}

}  // extern "C"
