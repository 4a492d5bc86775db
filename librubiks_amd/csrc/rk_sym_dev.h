// Device side of the symmetry tables (rk_sym_tables.h): the conjugate of a state under one symmetry and the canonical
// representative of a state's orbit -- the smallest of its 48 conjugates -- for the kernels of rk_sym.hip.
//
// Layout.  A lane works for ONE symmetry for as long as the kernel runs (canonicalisation: lane = symmetry, 48 of 64 lanes live;
// a single conjugate: every lane the same one).  What it needs of that symmetry:
//   * src, 20 bytes, in registers as v_perm_b32 selectors: x o src is two v_perm for the corners (8 bytes = the pool of one
//     v_perm) and two v_perm and a merge per dword of edges (12 bytes = a pool and a half), with no memory access at all;
//   * map, 20 rows of 24 bytes, in LDS: 20 byte reads per conjugate at row-of-the-lane + 24 c + code.  Sub-dword reads bank like
//     ds_read_b32: (address / 4) mod 32, the 32-lane halves apart.  The rows of a symmetry are 480 bytes = 120 dwords, and
//     120 = 24 mod 32 would put the 32 lanes of a half on 4 banks; a symmetry's block is therefore padded to SYM_ROW = 121
//     dwords, an odd stride: the 32 lanes of a half start on 32 different banks and differ by at most the 6 dwords of a row
//     after that, so a read meets a 2-way conflict now and then instead of an 8-way one always.  (Transposed, [c][code][symmetry], the lanes of a
//     wave would read 48 bytes of ONE row only if they held the same code, and they do not.)  With every lane on the same
//     symmetry (rk_sym_conjugate) all addresses of a read fall in one 24-byte row: 6 banks, no conflict.
// The tables are staged once per workgroup: 48 x 121 dwords = 23 232 bytes, six workgroups to a CU.
//
// The minimum of the 48 conjugates is taken dword by dword: the wave's unsigned minimum of dword j over the lanes still tied,
// the lanes that do not hold it drop out; after five rounds the lanes left are the symmetries that give the representative.
// A round is four v_min_u32 with a DPP row rotation (a row is 16 lanes: after rotations by 1, 2, 4, 8 every lane holds its
// row's minimum), four v_readlane and three scalar minima -- no LDS traffic beside the table reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rk_ballbuild_dev.h"
#include "rk_device.h"
#include "rk_search_dev.h"
#include "rk_sym_tables.h"

namespace rk {

constexpr int SYM_ROW = 121;                         // dwords of LDS per symmetry: 120 of tables and one of padding (odd stride)
constexpr int SYM_LDS_DWORDS = N_SYM * SYM_ROW + 2;   // (+ 2: a code is read as code & 31, so no byte of a state indexes past the image)

static __constant__ SymTables D_SYM = SYM_TABLES;

// what a lane keeps of its symmetry
struct SymLane {
	uint32_t sel[5];                                 // src as selectors: corners 0..7; edges minus 8: 0..11
	uint32_t row;                                    // byte offset of the symmetry's block in the staged tables
};

// all threads of the workgroup; a barrier before the first use
__device__ __forceinline__ void sym_stage(uint32_t *lds /* SYM_LDS_DWORDS */, int tid, int threads)
{
	const uint32_t *src = reinterpret_cast<const uint32_t *>(&D_SYM.map[0][0][0]);
	for (int i = tid; i < N_SYM * 120; i += threads) {
		const int s = i / 120;
		lds[s * SYM_ROW + (i - s * 120)] = src[i];
	}
}

__device__ __forceinline__ SymLane sym_lane(int s /* 0..47 */)
{
	SymLane L;
	const uint32_t *p = reinterpret_cast<const uint32_t *>(D_SYM.src[s]);
	L.sel[0] = p[0]; L.sel[1] = p[1];
	L.sel[2] = p[2] - 0x08080808u; L.sel[3] = p[3] - 0x08080808u; L.sel[4] = p[4] - 0x08080808u;
	L.row = (uint32_t)s * (SYM_ROW * 4);
	return L;
}

// y = conj_s(x) for the lane's symmetry
__device__ __forceinline__ void sym_conjugate(const uint32_t *lds, const SymLane &L, const uint32_t x[5], uint32_t y[5])
{
	uint32_t g[5];
	g[0] = bperm(x[1], x[0], L.sel[0]);
	g[1] = bperm(x[1], x[0], L.sel[1]);
	#pragma unroll
	for (int j = 2; j < 5; j++) {
		const uint32_t e = L.sel[j];
		const uint32_t lo = bperm(x[3], x[2], e & 0x07070707u);
		const uint32_t hi = bperm(0u, x[4], e & 0x03030303u);
		const uint32_t m = bperm(0u, 0u, ((e >> 3) & 0x01010101u) | 0x0C0C0C0Cu);       // 0xFF where the source is edge 8..11 (lut4)
		g[j] = (hi & m) | (lo & ~m);
	}
	const uint8_t *rows = reinterpret_cast<const uint8_t *>(lds) + L.row;
	#pragma unroll
	for (int j = 0; j < 5; j++) {
		uint32_t out = 0;
		#pragma unroll
		for (int b = 0; b < 4; b++) {
			const int c = 4 * j + b;
			out |= (uint32_t)rows[24 * c + ((g[j] >> (8 * b)) & 31u)] << (8 * b);
		}
		y[j] = out;
	}
}

template <int CTRL>
__device__ __forceinline__ uint32_t sym_dpp(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// the unsigned minimum over the 64 lanes, the same in every lane.  ALL 64 lanes call it.
__device__ __forceinline__ uint32_t sym_wave_umin(uint32_t v)
{
	v = min(v, sym_dpp<0x121>(v));                   // row_ror:1
	v = min(v, sym_dpp<0x122>(v));                   // row_ror:2
	v = min(v, sym_dpp<0x124>(v));                   // row_ror:4
	v = min(v, sym_dpp<0x128>(v));                   // row_ror:8
	const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
	const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
	return min(min(a, b), min(c, d));
}

// The canonical form of x (the same in every lane): rep = the smallest conjugate, compared as the tuple of its dwords, dword 0
// first; *sym = the lowest symmetry that gives it, *count = how many do (the orbit has 48 / count states).  ALL 64 lanes of the
// wave call it, lane l with the SymLane of symmetry l (lanes 48..63: of any symmetry; they take no part).
__device__ __forceinline__ void sym_canonical(const uint32_t *lds, const SymLane &L, int lane, const uint32_t x[5], uint32_t rep[5],
                                              int *sym, int *count)
{
	uint32_t y[5];
	sym_conjugate(lds, L, x, y);
	bool tied = lane < N_SYM;
	#pragma unroll
	for (int j = 0; j < 5; j++) {
		rep[j] = sym_wave_umin(tied ? y[j] : 0xFFFFFFFFu);
		tied = tied && y[j] == rep[j];
	}
	const unsigned long long who = __ballot(tied);
	*sym = __ffsll((long long)who) - 1;
	*count = __popcll(who);
}

// ---- what the readers of a built symmetry ball share (rk_sym.hip: the queries of rk_symball_*, the search of rk_ssearch_*) ----
constexpr int SB_MAX_RADIUS = 10;

// What the readers of a built ball get, by value.
struct SymBallView {
	uint32_t mask, cap1;
	int radius;
	int32_t lstart[SB_MAX_RADIUS + 2];          // level l = lstart[l] .. lstart[l + 1] - 1; INT32_MAX beyond radius + 1
	const uint32_t *states; const uint32_t *table;
};

// A reader in another translation unit than the ball's (rk_beam.hip): the built ball's view and a hold on its arrays, counted as
// a search's is (rk_symball_destroy refuses meanwhile), and the hold given back.  Host side, defined in rk_sym.hip.
int symball_attach(::rk_symball *ball, const char *who, SymBallView *view);
void symball_detach(::rk_symball *ball);

// What a wave needs to ask the ball about a state: the staged tables, its lane and the lane's symmetry (lane l < 48: symmetry l;
// lanes 48..63 take no part in the minimum).  s_act is null in a kernel that moves no state.
struct SymProbe {
	const uint32_t *s_sym;
	const u32x4 *s_act;
	SymLane L;
	int lane;
};

// All `threads` threads of the workgroup, once, after the kernel has declared its LDS (s_sym: SYM_LDS_DWORDS; s_act: 36 or null):
// stages the symmetry tables and, where given, the action tables, then the barrier.
__device__ __forceinline__ SymProbe sym_probe(uint32_t *s_sym, int threads, u32x4 *s_act = nullptr)
{
	sym_stage(s_sym, threadIdx.x, threads);
	if (s_act != nullptr) stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int lane = threadIdx.x & 63;
	return SymProbe{s_sym, s_act, sym_lane(min(lane, N_SYM - 1)), lane};
}

// The ball's node of the representative of x, 0 when the ball does not hold it; sb_level: its level, -1 outside the ball.  ALL 64
// lanes of a wave call these with the same x (sym_canonical); the answer is the same in every lane.
__device__ __forceinline__ uint32_t sb_node(const SymBallView &b, const SymProbe &c, const uint32_t x[5])
{
	uint32_t rep[5];
	int sym, count;
	sym_canonical(c.s_sym, c.L, c.lane, x, rep, &sym, &count);
	return probe_find(b.table, b.mask, b.states, rep);
}

__device__ __forceinline__ int sb_level(const SymBallView &b, const SymProbe &c, const uint32_t x[5])
{
	const uint32_t e = sb_node(b, c, x);
	return e ? level_of(b.lstart, e) : -1;
}

// The descent from x, a state whose representative lies at level `depth` of the ball, to the solved state: at each step the lowest
// action whose child's representative lies one level nearer, emit(step, action) for every step, x moved along.  Returns the
// steps taken; *ok = false when a state has no such child (the ball is broken) or depth is outside 0..radius.  ALL 64 lanes of a
// wave call it with the same x; everything in it is the same in every lane.
template <typename Emit>
__device__ __forceinline__ int sb_descend(const SymBallView &b, const SymProbe &c, uint32_t x[5], int depth, Emit emit, bool *ok_out)
{
	int len = 0;
	bool ok = depth >= 0 && depth <= b.radius;
	while (ok && len < depth) {                                      // (everything here is the same in every lane)
		int found = -1;
		for (int a = 0; a < N_ACTIONS && found < 0; a++) {
			uint32_t y[5], tab[12];
			#pragma unroll
			for (int j = 0; j < 5; j++) y[j] = x[j];
			load_action_table(c.s_act, (uint32_t)a, tab);
			move5(y, tab);
			if (sb_level(b, c, y) == depth - len - 1) {
				found = a;
				#pragma unroll
				for (int j = 0; j < 5; j++) x[j] = y[j];
			}
		}
		if (found < 0) { ok = false; break; }                        // a node without a child one level nearer: the ball is broken
		emit(len, found);
		len++;
	}
	*ok_out = ok;
	return len;
}

}  // namespace rk
