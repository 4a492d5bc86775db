// The 48 whole-cube symmetries (24 rotations, 24 reflections) as tables, generated at compile time from the six face definitions
// and the move table (rk_tables.h); host memory and the device's constant segment hold the same bytes.  Nothing is typed in.
//
// Order.  A face is 2 * axis + side (F B | T D | L R).  Symmetry s = 8 * p + m sends axis `ax` to SYM_PERMS[p][ax] (the six
// permutations of 0 1 2 in lexicographic order) and swaps the two faces of source axis `ax` when bit `ax` of m is set: face f goes
// to 2 * SYM_PERMS[p][f / 2] + ((f & 1) ^ ((m >> (f / 2)) & 1)).  s = 0 is the identity.  s is a reflection when the parity of the
// permutation and the parity of m differ.
//
// What a symmetry does.  It relabels the actions -- act[s][a]: the turn of face f becomes a turn of the image face, in the same
// sense under a rotation and in the opposite sense under a reflection -- and the relabelling w -> act[s](w) of move sequences is an
// automorphism of the cube group that keeps the distance to solved.  The conjugate of state x (code[c] of 20 cubies) is
//     conj_s(x)[c] = map[s][c][ x[ src[s][c] ] ]                  conj_s(rotate(x, a)) = rotate(conj_s(x), act[s][a])
// src[s][c] is the cubie whose home position the symmetry carries onto the home position of c: the cubie that lies on the source
// faces of the faces c lies on.  map[s][c] re-codes it: a sequence W that puts cubie src at code v = W(home of src) becomes a
// sequence act[s](W) that puts cubie c at act[s](W)(home of c), so map[s][c] is the one bijection of the 24 codes with
//     map[home of src] = home of c          map o lut[a] = lut[act[s][a]] o map          for all 12 actions
// -- the slot bijection of the symmetry composed with the twist / flip that brings the one home onto the other.  It is filled by
// a breadth-first walk over the moves from that seed; `consistent` says that no two paths to a code disagreed, that every walk
// reached all 24 codes and that src is a permutation, for all 48 symmetries.  A wrong turning sense would contradict itself there.
#pragma once
#include <stdint.h>
#include "rk_tables.h"

namespace rk {

constexpr int N_SYM = 48;
constexpr uint8_t SYM_PERMS[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

struct alignas(16) SymTables {
	uint8_t act[N_SYM][N_ACTIONS];
	uint8_t src[N_SYM][STATE_BYTES];
	uint8_t map[N_SYM][STATE_BYTES][24];
	bool consistent;
};

constexpr int sym_face(int s, int f)
{
	return 2 * SYM_PERMS[s >> 3][f >> 1] + ((f & 1) ^ (((s & 7) >> (f >> 1)) & 1));
}

constexpr bool sym_is_reflection(int s)
{
	const uint8_t *p = SYM_PERMS[s >> 3];
	const int inversions = (p[0] > p[1]) + (p[0] > p[2]) + (p[1] > p[2]);
	const int m = s & 7;
	return ((inversions + (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1)) & 1) != 0;
}

// the faces (bit f) whose ring holds position `pos` of cubie kind `kind` (0 corner, 1 edge)
constexpr int sym_faces_of(int kind, int pos)
{
	int mask = 0;
	for (int f = 0; f < 6; f++)
		for (int j = 0; j < 4; j++)
			if ((kind == 0 ? FACES[f].corner[j] : FACES[f].edge[j]) == pos) mask |= 1 << f;
	return mask;
}

constexpr SymTables make_sym_tables()
{
	const Tables t = make_tables();
	SymTables r{};
	r.consistent = true;
	int faces_of[2][12] = {};
	for (int k = 0; k < 2; k++)
		for (int pos = 0; pos < (k == 0 ? 8 : 12); pos++) faces_of[k][pos] = sym_faces_of(k, pos);
	for (int s = 0; s < N_SYM; s++) {
		const int mirror = sym_is_reflection(s) ? 1 : 0;
		for (int a = 0; a < N_ACTIONS; a++) r.act[s][a] = (uint8_t)(2 * sym_face(s, a >> 1) + ((a & 1) ^ mirror));
		bool is_src[STATE_BYTES] = {};
		for (int c = 0; c < STATE_BYTES; c++) {
			const int k = c < 8 ? 0 : 1, n = k == 0 ? 8 : 12, pos = c - 8 * k;
			// the cubie on the source faces of c's faces
			int from = -1;
			for (int q = 0; q < n; q++) {
				int image = 0;
				for (int f = 0; f < 6; f++) if (faces_of[k][q] >> f & 1) image |= 1 << sym_face(s, f);
				if (image == faces_of[k][pos]) from = from < 0 ? q : n;          // (two candidates: not a cube)
			}
			if (from < 0 || from >= n || is_src[8 * k + from]) { r.consistent = false; continue; }
			is_src[8 * k + from] = true;
			r.src[s][c] = (uint8_t)(8 * k + from);
			// the walk: map[home of src] = home of c, map[lut[a][v]] = lut[act[a]][map[v]]
			uint8_t *map = r.map[s][c];
			bool known[24] = {};
			int todo[24] = {}, n_todo = 0, n_known = 1;
			const int stride = k == 0 ? 3 : 2;
			map[stride * from] = (uint8_t)(stride * pos);
			known[stride * from] = true;
			todo[n_todo++] = stride * from;
			while (n_todo > 0) {
				const int v = todo[--n_todo];
				for (int a = 0; a < N_ACTIONS; a++) {
					const int v2 = t.lut[a][k][v], w2 = t.lut[r.act[s][a]][k][map[v]];
					if (!known[v2]) {
						map[v2] = (uint8_t)w2;
						known[v2] = true;
						todo[n_todo++] = v2;
						n_known++;
					} else if (map[v2] != w2) {
						r.consistent = false;
					}
				}
			}
			if (n_known != 24) r.consistent = false;
		}
	}
	return r;
}

// evaluated once per compilation (a few million constexpr steps: build.py raises the compiler's step limit)
constexpr SymTables SYM_TABLES = make_sym_tables();
static_assert(SYM_TABLES.consistent, "the 48 symmetries do not fit the move tables");

}  // namespace rk
