// Move tables of the cube, generated at compile time from the six face definitions and placed in
// both host memory and the device's constant segment (no runtime initialisation, valid on every GPU).
//
// What the tables mean is fixed by the reference: maps.py:74-98 (face rings), maps.py:107-145
// (how a quarter turn re-codes a cubie), cube.py:330-347 + maps.py:149-156 (6x8x6 sticker cycles).
#pragma once
#include <stdint.h>

namespace rk {

constexpr int N_ACTIONS = 12;
constexpr int STATE_BYTES = 20;     // 8 corner codes + 12 edge codes (cube.py:58-65)
constexpr int STATE_DWORDS = 5;
constexpr int S686_BYTES = 288;     // 6 faces x 8 ring positions x 6 colours, int8 one-hot (cube.py:67-71)
constexpr int S686_SLOTS = 48;

struct Face { uint8_t corner[4], edge[4], fixed_ori, flip; };

// Order F, B, T, D, L, R (cube.py:30).  A positive turn moves the cubie in ring[j] to ring[j+1].
constexpr Face FACES[6] = {
	{{0, 1, 2, 3}, {0, 1, 2, 3},   0, 0},
	{{4, 7, 6, 5}, {8, 11, 10, 9}, 0, 0},
	{{0, 3, 7, 4}, {0, 7, 8, 4},   1, 1},
	{{1, 5, 6, 2}, {2, 5, 10, 6},  1, 1},
	{{0, 4, 5, 1}, {1, 4, 9, 5},   2, 0},
	{{7, 3, 2, 6}, {3, 6, 11, 7},  2, 0},
};
constexpr uint8_t NEIGHBOUR[6][4] = {{4, 3, 5, 2}, {3, 4, 2, 5}, {0, 5, 1, 4}, {5, 0, 4, 1}, {2, 1, 3, 0}, {1, 2, 0, 3}};
constexpr uint8_t STRIP[4][3] = {{6, 7, 0}, {2, 3, 4}, {4, 5, 6}, {0, 1, 2}};

struct alignas(16) Tables {
	// T[a][kind][v]: code of a cubie with code v after action a; kind 0 corner, 1 edge.  a = 2*face + (1-dir).
	uint8_t lut[N_ACTIONS][2][24];
	// rows[kind][v][a]: the same numbers regrouped so that ONE 16-byte LDS read returns the code of a cubie in
	// all 12 children (bytes 12..15 are zero).  This is the table the fan-out kernel stages in LDS.
	uint8_t rows[2][24][16];
	// per_action[a][24*kind + v]: 48-byte rows (6 dwords of corner codes, 6 of edge codes); what kernels whose
	// action differs per state stage in LDS.
	uint8_t per_action[N_ACTIONS][48];
	// 6x8x6: new[slot] = old[perm686[a][slot]], slot = 8*face + ring position
	uint8_t perm686[N_ACTIONS][S686_SLOTS];
	int8_t  solved[STATE_BYTES + 12];   // padded to 32 bytes
	int8_t  solved686[S686_BYTES];
	// 6x8x6 gather tables, ready to be copied to LDS with 16-byte loads: a state is 144 ushorts (48 slots x 3);
	// src686[a][u] = source ushort of output ushort u under action a = perm686[a][u/3]*3 + u%3
	alignas(16) uint8_t src686[N_ACTIONS][144];
	// near686[a][slot] = colour shown by `slot` in the state whose child `a` is solved (= move a^1 applied to solved)
	alignas(16) uint8_t near686[N_ACTIONS][S686_SLOTS];
};

constexpr Tables make_tables()
{
	Tables t{};
	for (int a = 0; a < N_ACTIONS; a++)
		for (int k = 0; k < 2; k++)
			for (int v = 0; v < 24; v++) t.lut[a][k][v] = (uint8_t)v;
	for (int f = 0; f < 6; f++) {
		const int p = 2 * f, n = 2 * f + 1;       // positive (dir 1) and negative (dir 0) action of face f
		for (int j = 0; j < 4; j++) {
			const int cf = FACES[f].corner[j], ct = FACES[f].corner[(j + 1) & 3];
			for (int k = 0; k < 3; k++) {
				const int kn = (k == FACES[f].fixed_ori) ? k : 3 - FACES[f].fixed_ori - k;
				t.lut[p][0][3 * cf + k] = (uint8_t)(3 * ct + kn);
				t.lut[n][0][3 * ct + kn] = (uint8_t)(3 * cf + k);
			}
			const int ef = FACES[f].edge[j], et = FACES[f].edge[(j + 1) & 3];
			for (int k = 0; k < 2; k++) {
				const int kn = k ^ FACES[f].flip;
				t.lut[p][1][2 * ef + k] = (uint8_t)(2 * et + kn);
				t.lut[n][1][2 * et + kn] = (uint8_t)(2 * ef + k);
			}
		}
	}
	for (int k = 0; k < 2; k++)
		for (int v = 0; v < 24; v++)
			for (int a = 0; a < N_ACTIONS; a++) {
				t.rows[k][v][a] = t.lut[a][k][v];
				t.per_action[a][24 * k + v] = t.lut[a][k][v];
			}
	for (int i = 0; i < 8; i++) t.solved[i] = (int8_t)(3 * i);
	for (int i = 0; i < 12; i++) t.solved[8 + i] = (int8_t)(2 * i);

	for (int f = 0; f < 6; f++) {
		uint8_t *p = t.perm686[2 * f], *q = t.perm686[2 * f + 1];
		for (int s = 0; s < S686_SLOTS; s++) p[s] = (uint8_t)s;
		for (int pos = 0; pos < 8; pos++) p[8 * f + pos] = (uint8_t)(8 * f + ((pos + 6) & 7));
		for (int k = 0; k < 4; k++)
			for (int s = 0; s < 3; s++)
				p[8 * NEIGHBOUR[f][k] + STRIP[k][s]] = (uint8_t)(8 * NEIGHBOUR[f][(k + 3) & 3] + STRIP[(k + 3) & 3][s]);
		for (int s = 0; s < S686_SLOTS; s++) q[p[s]] = (uint8_t)s;
		for (int pos = 0; pos < 8; pos++) t.solved686[(8 * f + pos) * 6 + f] = 1;
	}
	for (int a = 0; a < N_ACTIONS; a++) {
		for (int u = 0; u < 144; u++) t.src686[a][u] = (uint8_t)(t.perm686[a][u / 3] * 3 + u % 3);
		for (int slot = 0; slot < S686_SLOTS; slot++) t.near686[a][slot] = (uint8_t)(t.perm686[a ^ 1][slot] >> 3);
	}
	return t;
}

// ---- 20-byte <-> 6x8x6 (the two representations of one cube, cube.py:58-71) ----------------------------------------
// Both forms follow the same actions, so each cubie's stickers can be tracked through the 6x8x6 sticker permutation while
// its 20-byte code is tracked through the move table: starting from the solved cube, a breadth-first walk over the 12
// actions reaches every (cubie, code) pair and records which slot shows which of the cubie's colours there.  Nothing is
// typed in: the slots of a cubie position are the slots that exactly the faces holding that position move, a sticker's
// colour is the face of the slot it shows at home, and `consistent` checks that every path to a code agrees.
struct alignas(16) Repr686Tables {
	// fw[c][v]: cubie c (0..7 corners, 8..19 edges) with code v; sticker k (3 corners, 2 edges) in bits 9k..9k+8 as
	// slot (6 bits, slot = 8*face + ring position) | colour << 6
	uint32_t fw[20][24];
	// home[pos]: the slots of cubie position pos (0..7 corners, 8..19 edges), its stickers' slots at home, ascending;
	// inv[pos][c0][c1]: the cubie * 32 + code that shows colours c0, c1 at home[pos][0], home[pos][1]; 0xFFFF: none
	uint8_t  home[20][3];
	uint16_t inv[20][6][6];
	bool     consistent;
};

constexpr int face_mask_of_slot(const Tables &t, int s)
{
	int m = 0;
	for (int f = 0; f < 6; f++) if (t.perm686[2 * f][s] != s) m |= 1 << f;
	return m;
}

constexpr Repr686Tables make_repr686_tables()
{
	const Tables t = make_tables();
	Repr686Tables r{};
	r.consistent = true;
	uint8_t slot[20][24][3] = {};
	bool known[20][24] = {};
	for (int c = 0; c < 20; c++) {
		const bool corner = c < 8;
		const int pos = corner ? c : c - 8, n = corner ? 3 : 2;
		int want = 0;
		for (int f = 0; f < 6; f++)
			for (int j = 0; j < 4; j++)
				if ((corner ? FACES[f].corner[j] : FACES[f].edge[j]) == pos) want |= 1 << f;
		int k = 0;
		for (int s = 0; s < S686_SLOTS; s++)
			if (face_mask_of_slot(t, s) == want) {
				if (k < 3) r.home[c][k] = (uint8_t)s;
				k++;
			}
		if (k != n) r.consistent = false;
		const int v0 = corner ? 3 * pos : 2 * pos;
		for (int j = 0; j < n; j++) slot[c][v0][j] = r.home[c][j];
		known[c][v0] = true;
		for (bool grew = true; grew;) {
			grew = false;
			for (int v = 0; v < 24; v++) {
				if (!known[c][v]) continue;
				for (int a = 0; a < N_ACTIONS; a++) {
					const int w = t.lut[a][corner ? 0 : 1][v];
					uint8_t moved[3] = {};
					for (int j = 0; j < n; j++) moved[j] = t.perm686[a ^ 1][slot[c][v][j]];     // perm686[a ^ 1] inverts perm686[a]
					if (known[c][w]) {
						for (int j = 0; j < n; j++) if (slot[c][w][j] != moved[j]) r.consistent = false;
					} else {
						for (int j = 0; j < n; j++) slot[c][w][j] = moved[j];
						known[c][w] = grew = true;
					}
				}
			}
		}
		for (int v = 0; v < 24; v++) {
			if (!known[c][v]) r.consistent = false;
			uint32_t e = 0;
			for (int j = 0; j < n; j++) e |= (uint32_t)(slot[c][v][j] | (r.home[c][j] >> 3) << 6) << (9 * j);
			r.fw[c][v] = e;
		}
	}
	for (int p = 0; p < 20; p++)
		for (int a = 0; a < 6; a++)
			for (int b = 0; b < 6; b++) r.inv[p][a][b] = 0xFFFF;
	for (int c = 0; c < 20; c++) {
		const bool corner = c < 8;
		const int n = corner ? 3 : 2;
		for (int v = 0; v < 24; v++) {
			const int p = corner ? v / 3 : 8 + v / 2;
			int col[2] = {-1, -1};
			for (int j = 0; j < n; j++)
				for (int h = 0; h < 2; h++)
					if (slot[c][v][j] == r.home[p][h]) col[h] = r.home[c][j] >> 3;
			if (col[0] < 0 || col[1] < 0 || r.inv[p][col[0]][col[1]] != 0xFFFF) { r.consistent = false; continue; }
			r.inv[p][col[0]][col[1]] = (uint16_t)(c * 32 + v);
		}
	}
	return r;
}

}  // namespace rk
