// The cube group acting on 20-byte states, as tables generated at compile time from the move table (rk_tables.h).  Nothing is typed in.
//
// lut[a][kind] permutes all 24 sticker slots of a kind (corner slot 3 * pos + k, edge slot 2 * pos + k), not only the codes a cubie's
// primary sticker takes.  A state b reached from solved by a word has therefore a full action g_b on the slots -- the product of the
// word's moves -- and b[c] = g_b(home slot of c) is what the 20 bytes keep of it.  The rest follows from the cubies being rigid:
//     full[kind][p][v][k] = g_b(slot k of home p) for every b with b[p] = v
// Cubie p's stickers start at slots stride * p + k and are carried along by every action; a breadth-first walk over the 12 actions
// from solved reaches all 24 codes of the primary sticker and records where the others are.  `consistent` says that no two paths to
// a code disagreed, that every walk reached 24 codes, that a cubie's stickers always fill one position, and, for edges, that the
// walk found the closed form g_b(2 p + k) = b[p] ^ k.
//     apply(a, b)[c] = g_b(a[c]) = full[p][b[p]][k]  with a[c] = stride * p + k          (a's word, then b's)
//     inverse(b)[pos of b[p]] = inv[kind][p][b[p]] = the slot stride * p + k that g_b sends to the primary slot of that position
//
// The corner twist.  Seen from cubie 0, the stickers of a cubie at position q lie at slots 3 q + sigma(k); sigma is a rotation of
// 0 1 2 where q has the chirality of position 0 and a reflection where it has the other (chi).  tau(3 q + k) = k or -k mod 3 by
// chi[q] is zero on the home codes; an action changes tau by an amount that depends on the position alone, and the eight amounts
// add up to 0 mod 3 (both checked here), so the sum of tau over the corners of a state is the same before and after any move: 0.
#pragma once
#include <stdint.h>
#include "rk_tables.h"

namespace rk {

struct alignas(16) GroupTables {
	uint8_t full[2][12][24][3];                     // [kind][home][code][k]; corners use homes 0..7, edges k 0..1; the rest is zero
	uint8_t inv[2][12][24];                         // [kind][home][code]
	uint8_t tau[24];                                // the twist of a corner code, 0..2
	uint8_t chi[8];                                 // 1: the position has the other chirality than position 0
	// what the kernels stage in LDS: [corner home][code & 31] = full's three bytes, inv in byte 3.  Codes 24..31 repeat 16..23, as
	// lut4 (rk_device.h) reads them, so that no byte of an ill-formed row indexes past the image.
	uint32_t dev[8][32];
	uint32_t div3[6], mod3[6];                      // code / 3 and code % 3 as lut4 tables
	bool consistent;
};

constexpr GroupTables make_group_tables()
{
	const Tables t = make_tables();
	GroupTables r{};
	r.consistent = true;
	for (int kind = 0; kind < 2; kind++) {
		const int n = kind == 0 ? 3 : 2, homes = kind == 0 ? 8 : 12;
		for (int p = 0; p < homes; p++) {
			uint8_t slot[24][3] = {};
			bool known[24] = {};
			int todo[24] = {}, n_todo = 0, n_known = 1;
			for (int j = 0; j < n; j++) slot[n * p][j] = (uint8_t)(n * p + j);
			known[n * p] = true;
			todo[n_todo++] = n * p;
			while (n_todo > 0) {
				const int v = todo[--n_todo];
				for (int a = 0; a < N_ACTIONS; a++) {
					const int w = t.lut[a][kind][v];
					uint8_t moved[3] = {};
					for (int j = 0; j < n; j++) moved[j] = t.lut[a][kind][slot[v][j]];
					if (moved[0] != w) r.consistent = false;
					if (!known[w]) {
						for (int j = 0; j < n; j++) slot[w][j] = moved[j];
						known[w] = true;
						todo[n_todo++] = w;
						n_known++;
					} else {
						for (int j = 0; j < n; j++) if (slot[w][j] != moved[j]) r.consistent = false;
					}
				}
			}
			if (n_known != 24) r.consistent = false;
			for (int v = 0; v < 24; v++) {
				const int first = v / n * n;                                 // the primary slot of v's position
				int seen = 0, back = -1;
				for (int j = 0; j < n; j++) {
					r.full[kind][p][v][j] = slot[v][j];
					if (slot[v][j] / n * n != first) r.consistent = false;
					seen |= 1 << (slot[v][j] - first);
					if (slot[v][j] == first) back = n * p + j;
					if (kind == 1 && slot[v][j] != (v ^ j)) r.consistent = false;
				}
				if (seen != (1 << n) - 1 || back < 0) r.consistent = false;
				r.inv[kind][p][v] = (uint8_t)back;
			}
		}
	}
	// chirality from cubie 0, then every cubie against it
	for (int q = 0; q < 8; q++) r.chi[q] = r.full[0][0][3 * q][1] == 3 * q + 1 ? 0 : 1;
	for (int p = 0; p < 8; p++)
		for (int v = 0; v < 24; v++) {
			const int q = v / 3, s0 = r.full[0][p][v][0] - 3 * q, s1 = r.full[0][p][v][1] - 3 * q;
			const bool rotation = (s1 - s0 + 3) % 3 == 1;
			if (rotation != (r.chi[p] == r.chi[q])) r.consistent = false;
		}
	for (int v = 0; v < 24; v++) r.tau[v] = (uint8_t)(r.chi[v / 3] ? (3 - v % 3) % 3 : v % 3);
	for (int a = 0; a < N_ACTIONS; a++) {
		int sum = 0;
		for (int q = 0; q < 8; q++) {
			const int d = (r.tau[t.lut[a][0][3 * q]] - r.tau[3 * q] + 3) % 3;
			for (int k = 1; k < 3; k++)
				if ((r.tau[t.lut[a][0][3 * q + k]] - r.tau[3 * q + k] + 3) % 3 != d) r.consistent = false;
			sum += d;
		}
		if (sum % 3 != 0) r.consistent = false;
	}
	for (int p = 0; p < 8; p++)
		for (int v = 0; v < 32; v++) {
			const int u = v < 24 ? v : v - 8;
			r.dev[p][v] = (uint32_t)r.full[0][p][u][0] | (uint32_t)r.full[0][p][u][1] << 8 | (uint32_t)r.full[0][p][u][2] << 16 |
			              (uint32_t)r.inv[0][p][u] << 24;
		}
	for (int v = 0; v < 24; v++) {
		r.div3[v >> 2] |= (uint32_t)(v / 3) << (8 * (v & 3));
		r.mod3[v >> 2] |= (uint32_t)(v % 3) << (8 * (v & 3));
	}
	return r;
}

constexpr GroupTables GROUP_TABLES = make_group_tables();
static_assert(GROUP_TABLES.consistent, "the slot actions of the cubies do not fit the move tables");

// tau as 24 two-bit fields: (GROUP_TAU_BITS >> 2 v) & 3
constexpr uint64_t group_tau_bits()
{
	uint64_t b = 0;
	for (int v = 0; v < 24; v++) b |= (uint64_t)GROUP_TABLES.tau[v] << (2 * v);
	return b;
}
constexpr uint64_t GROUP_TAU_BITS = group_tau_bits();

}  // namespace rk
