// Device-resident beam search guided by a value net: depth t holds a beam F_t of m_t <= B states in a fixed order, F_0 = the start;
// child c = 12 i + a is the state of member i under action a, and every depth treats its children in that order.
//
// What lives in HBM (width B, at most D depths):
//   beam    2 x B x 5 u32      F_t in half t & 1 and, while a depth commits, F_{t+1} in the other (no state of an earlier depth is kept)
//   back    (D + 1) x B u32    back[t][j] = i << 4 | a: member j of F_t is child a of member i of F_{t-1}
//   sizes   int32 (D + 1)      m_t
//   table   u32, 2^k >= 24 B   the dedup election of one depth's children (probe_elect: the lowest c of equal states wins)
//   slot, key, level   per child: the slot it claimed, its ordered 32-bit value key (0: no survivor), with a ball its ball depth
//   hist    4 x 256 int32      the radix passes of the selection;  words: the look-back words of the commit's scan
//   ctr     int32[32]          the counters: everything data-dependent that a launch needs is read from here
//   the net batch: 12 B rows, row 12 j + a = child a of member j, one-hot of the net's dtype or the 20-byte states
// A depth is [net forward, rk_beam_step]; rk_beam_step enqueues a fixed sequence of launches and nothing else:
//   ball    (with a ball) a wave per live child: the canonical form and the read-only look-up, level[c]
//   probe   a thread per child: live or dead, the goal test (or level[c]), the election, n_live and the win key (ball depth, c)
//   keys    the survivors' keys and the histogram of their top byte
//   hist    x 3: the next byte among the keys that share the bytes picked so far
//   commit  the B-th best key T from the four histograms; keys above T are taken, keys equal to T in c order while room is left:
//           an order-preserving compaction over both classes (scan_lookback_classes) writes F_{t+1} in ascending c and its back words,
//           and every child gives back the table slot it claimed
//   rows    a wave per member of F_{t+1}: its twelve rows of the next batch
//   end     one wave: the budget, the win, the depth limit, t and m_t move on; the counters of the next depth are cleared
// Every launch begins by reading the status (written by `end` alone, in a launch of its own): after a stop a replay writes nothing.
// A launch between probe and end reads whether THIS depth stops (budget, win) from counters that no launch in between writes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"
#include "rk_sym_dev.h"

namespace rk {

enum {
	W_STATUS = 0, W_T, W_M, W_MNEXT, W_NLIVE, W_WINKEY, W_TICKET, W_ERROR, W_DEPTH, W_MEET_I, W_MEET_A, W_MEET_LEVEL,
	W_EXPLORED /* 2 words */, W_BUDGET = W_EXPLORED + 2 /* 2 words */, W_COUNT = 32
};
enum { BEAM_RUNNING = 0, BEAM_SOLVED = 1, BEAM_SPENT = 2, BEAM_DEPTH = 3, BEAM_FAILED = 4, BEAM_IDLE = 5 /* a slot of the batch at rest */ };
enum { BEAM_ERR_NONE = 0, BEAM_ERR_RECORD = 1 };     // a write into back, the beam or the sizes that has no place there
constexpr int32_t NO_WIN = INT32_MAX;
constexpr int WIN_SHIFT = 20;                         // win key = ball depth << 20 | c, c < 12 * 2^16 < 2^20

struct BeamDev {
	int B, D, code, prune, has_ball;
	uint32_t mask;
	uint32_t *beam, *back, *table, *slot, *key, *root;
	int32_t *sizes, *hist, *ctr;
	int8_t *level;
	unsigned long long *words;
	void *net_in;
};

// the depth a launch works on; run = false after a stop
struct BeamNow { int t, m; bool run; };

__device__ __forceinline__ BeamNow beam_now(const BeamDev &d)
{
	BeamNow n;
	n.run = d.ctr[W_STATUS] == BEAM_RUNNING;
	n.t = d.ctr[W_T];
	n.m = min(max(d.ctr[W_M], 0), d.B);
	n.run = n.run && n.t >= 0 && n.t < d.D;
	return n;
}

// whether the depth whose probe has run stops before it selects: the budget refuses its live children, or one of them wins
__device__ __forceinline__ bool beam_stops(const BeamDev &d)
{
	return ctr64(d.ctr, W_EXPLORED) + d.ctr[W_NLIVE] > ctr64(d.ctr, W_BUDGET) || d.ctr[W_WINKEY] != NO_WIN;
}

__device__ __forceinline__ const uint32_t *beam_half(const BeamDev &d, int t) { return d.beam + (size_t)(t & 1) * d.B * 5; }

// child c = 12 i + a of depth t: dead beyond the beam and, with prune, when a undoes the action that made member i
__device__ __forceinline__ bool beam_live(const BeamDev &d, const BeamNow &n, int c, int *i_out, int *a_out)
{
	const int i = c / 12, a = c - 12 * i;
	*i_out = i; *a_out = a;
	if (i >= n.m) return false;
	if (d.prune && n.t > 0 && a == (int)((d.back[(size_t)n.t * d.B + i] & 15u) ^ 1u)) return false;
	return true;
}

// v as a 32-bit key whose unsigned order is `beats`' order of values: every NaN the one top key, -0.0 folded onto +0.0; never 0
__device__ __forceinline__ uint32_t beam_key(float v)
{
	if (v != v) return 0xFFFFFFFFu;
	const uint32_t u = __float_as_uint(v + 0.0f);
	return (u >> 31) ? ~u : (u | 0x80000000u);
}

// ---- reset ----
// one wave: the counters, F_0 = the start, and with a ball the start's own look-up (a start whose orbit the ball holds has won)
// (`start`: where the start lies now -- d.root itself, or the batch's upload, which becomes the slot's root here)
__device__ __forceinline__ void beam_root(const BeamDev &d, const SymBallView &b, const uint32_t *start, long long budget)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	if (threadIdx.x < W_COUNT) d.ctr[threadIdx.x] = 0;
	const SymProbe sp = sym_probe(s_sym, 64);
	uint32_t s[5];
	load5(start, s);
	const int level = d.has_ball ? sb_level(b, sp, s) : -1;
	if (sp.lane < 5) {
		d.beam[sp.lane] = dword_of(s, sp.lane);
		if (start != d.root) d.root[sp.lane] = dword_of(s, sp.lane);
	}
	if (sp.lane == 0) {
		d.sizes[0] = 1;
		d.ctr[W_M] = 1;
		d.ctr[W_WINKEY] = NO_WIN;
		set_ctr64(d.ctr, W_BUDGET, budget);
		if (level >= 0) {
			d.ctr[W_STATUS] = BEAM_SOLVED;
			d.ctr[W_MEET_A] = -1;
			d.ctr[W_MEET_LEVEL] = level;
		}
	}
}

__global__ __launch_bounds__(64)
void k_beam_root(BeamDev d, SymBallView b, long long budget) { beam_root(d, b, d.root, budget); }

// EVERY row of the batch: rows 0..11 the start's children, every other the solved state (the net reads all 12 B rows at every
// depth, and its first layer indexes tables with a row's bytes).  Waves stride over the rows.
// (`started` false: the solved state in rows 0..11 too, what a slot of the batch holds that was not started in this form)
__device__ __forceinline__ void beam_fill(const BeamDev &d, bool started)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int lane = threadIdx.x & 63;
	const size_t rows = (size_t)12 * d.B;
	for (size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (size_t)gridDim.x * 4) {
		uint32_t s[5] = {SOLVED_DW[0], SOLVED_DW[1], SOLVED_DW[2], SOLVED_DW[3], SOLVED_DW[4]};
		if (r < 12 && started) child_state(d.root, 0, s_act, (uint32_t)r, s);
		write_row(d.net_in, d.code, r, s, lane, 64);
	}
}

__global__ __launch_bounds__(256)
void k_beam_fill(BeamDev d) { beam_fill(d, true); }

// ---- a depth ----
// one wave: level[c] of child c < 12 m_t, if it is live
__device__ __forceinline__ void beam_ball_child(const BeamDev &d, const BeamNow &n, const SymBallView &b, const SymProbe &sp, int c)
{
	int i, a;
	if (!beam_live(d, n, c, &i, &a)) return;
	uint32_t x[5];
	child_state(beam_half(d, n.t), i, sp.s_act, (uint32_t)a, x);
	const int level = sb_level(b, sp, x);
	if (sp.lane == 0) d.level[c] = (int8_t)level;
}

__global__ __launch_bounds__(256)
void k_beam_ball(BeamDev d, SymBallView b)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const BeamNow n = beam_now(d);
	const int K = 12 * n.m;
	if (!n.run || (int)blockIdx.x * 4 >= K) return;
	const SymProbe sp = sym_probe(s_sym, 256, s_act);
	for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < K; c += gridDim.x * 4) beam_ball_child(d, n, b, sp, c);       // (whole waves)
}

__device__ __forceinline__ void beam_probe(const BeamDev &d)
{
	__shared__ u32x4 s_act[36];
	const BeamNow n = beam_now(d);
	if (!n.run) return;
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int c = blockIdx.x * 256 + threadIdx.x;
	if (c >= 12 * d.B) return;
	const uint32_t *cur = beam_half(d, n.t);
	int i, a;
	const bool live = beam_live(d, n, c, &i, &a);
	uint32_t slot = NO_SLOT;
	if (live) {
		uint32_t x[5];
		child_state(cur, i, s_act, (uint32_t)a, x);
		const int level = d.has_ball ? (int)d.level[c] : is_solved5(x) ? 0 : -1;
		if (level >= 0) atomicMin(&d.ctr[W_WINKEY], (level << WIN_SHIFT) | c);
		probe_elect(d.table, d.mask, nullptr, x, c,
		            [&](int c2, uint32_t *o) { child_state(cur, c2 / 12, s_act, (uint32_t)(c2 % 12), o); }, &slot);
	}
	d.slot[c] = slot;
	const unsigned long long alive = __ballot(live);
	if (alive != 0ull && (threadIdx.x & 63) == __ffsll((long long)alive) - 1) atomicAdd(&d.ctr[W_NLIVE], __popcll(alive));
}

__global__ __launch_bounds__(256)
void k_beam_probe(BeamDev d) { beam_probe(d); }

// the histogram of one workgroup's digits into the pass's 256 counters
__device__ __forceinline__ void beam_hist_add(int32_t *hist, int *s_h, bool mine, uint32_t digit)
{
	s_h[threadIdx.x] = 0;
	__syncthreads();
	if (mine) atomicAdd(&s_h[digit], 1);
	__syncthreads();
	if (s_h[threadIdx.x] != 0) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}

// (`out`: the net's values on the whole batch, those of this search from element `first` on)
__device__ __forceinline__ void beam_keys(const BeamDev &d, const void *out, int bf16, size_t first)
{
	__shared__ int s_h[256];
	const BeamNow n = beam_now(d);
	if (!n.run || beam_stops(d)) return;
	const int c = blockIdx.x * 256 + threadIdx.x;
	uint32_t key = 0u;
	if (c < 12 * n.m) {
		const uint32_t sl = d.slot[c];
		if (sl != NO_SLOT && d.table[sl] == (TENT | (uint32_t)c)) key = beam_key(net_out(out, bf16 != 0, first + (size_t)c));
	}
	if (c < 12 * d.B) d.key[c] = key;
	beam_hist_add(d.hist, s_h, key != 0u, key >> 24);
}

__global__ __launch_bounds__(256)
void k_beam_keys(BeamDev d, const void *out, int bf16) { beam_keys(d, out, bf16, 0); }

// The bytes of the B-th best key that the first P histograms fix, by ALL 256 threads of a workgroup (barriers inside): prefix =
// those bytes, k = how many of the keys that share them are still to be taken; all = there are at most B survivors, all are taken.
struct BeamPick { uint32_t prefix; int k; bool all; };

__device__ __forceinline__ BeamPick beam_picks(const BeamDev &d, int P)
{
	__shared__ int s_w[4], s_digit, s_k;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	BeamPick p{0u, d.B, false};
	for (int pass = 0; pass < P; pass++) {
		const int digit = 255 - (int)threadIdx.x;                           // thread order = descending digits
		const int h = d.hist[pass * 256 + digit];
		int incl = h;
		#pragma unroll
		for (int off = 1; off < 64; off <<= 1) {
			const int y = __shfl_up(incl, off, 64);
			if (lane >= off) incl += y;
		}
		if (lane == 63) s_w[wv] = incl;
		if (threadIdx.x == 0) { s_digit = 0; s_k = 0; }
		__syncthreads();
		int before = 0, total = 0;
		#pragma unroll
		for (int w = 0; w < 4; w++) { before += w < wv ? s_w[w] : 0; total += s_w[w]; }
		const int above = before + incl - h;                                // keys with a larger digit
		if (pass == 0 && total <= p.k) { p.all = true; return p; }
		if (h > 0 && above < p.k && p.k <= above + h) { s_digit = digit; s_k = p.k - above; }
		__syncthreads();
		p.prefix = (p.prefix << 8) | (uint32_t)s_digit;
		p.k = s_k;
		__syncthreads();                                                    // s_w, s_digit and s_k are written again
	}
	return p;
}

__device__ __forceinline__ void beam_hist(const BeamDev &d, int pass)
{
	__shared__ int s_h[256];
	const BeamNow n = beam_now(d);
	if (!n.run || beam_stops(d)) return;
	const BeamPick p = beam_picks(d, pass);
	if (p.all) return;
	const int c = blockIdx.x * 256 + threadIdx.x;
	const uint32_t key = c < 12 * n.m ? d.key[c] : 0u;
	const int shift = 32 - 8 * pass;
	beam_hist_add(d.hist + pass * 256, s_h, key != 0u && (key >> shift) == p.prefix, (key >> (shift - 8)) & 255u);
}

__global__ __launch_bounds__(256)
void k_beam_hist(BeamDev d, int pass) { beam_hist(d, pass); }

// (nblocks = gridDim.x: the workgroups of ONE search; the ticket, the look-back words and the epoch t + 1 are that search's own)
__device__ __forceinline__ void beam_commit(const BeamDev &d)
{
	__shared__ u32x4 s_act[36];
	__shared__ int s_wave[4], s_tot[2], s_base[2], s_ticket;
	const BeamNow n = beam_now(d);
	if (!n.run || beam_stops(d)) return;
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const BeamPick p = beam_picks(d, 4);
	const uint32_t T = p.all ? 0u : p.prefix;                               // keys above T are taken,
	const int kt = p.all ? 0 : p.k;                                         // of the keys equal to T the first kt
	const int nblocks = gridDim.x;
	const int b = scan_ticket(&d.ctr[W_TICKET], &s_ticket);
	if (b >= nblocks) return;
	const int c = b * ASCAN + threadIdx.x;
	const bool inside = c < 12 * d.B;
	const uint32_t key = inside && c < 12 * n.m ? d.key[c] : 0u;
	const uint32_t cls = key > T ? 0u : (key != 0u && key == T) ? 1u : 2u;
	scan_lookback_classes(d.words, nblocks, b, 2, cls, (uint32_t)n.t + 1u, s_wave, s_tot, s_base);
	const int base0 = s_base[0], base1 = s_base[1], tot0 = s_tot[0], tot1 = s_tot[1];
	int unused;
	const int g0 = base0 + block_rank256(cls == 0u, s_wave, &unused);       // taken-for-sure children before c
	const int g1 = base1 + block_rank256(cls == 1u, s_wave, &unused);       // children at the threshold before c
	if (cls == 0u || (cls == 1u && g1 < kt)) {
		const int j = g0 + min(g1, kt);
		if (j < 0 || j >= d.B || n.t + 1 > d.D) {                           // never write outside the beam or the back record
			d.ctr[W_ERROR] = BEAM_ERR_RECORD;
		} else {
			const int i = c / 12, a = c - 12 * i;
			uint32_t x[5];
			child_state(beam_half(d, n.t), i, s_act, (uint32_t)a, x);
			uint32_t *dst = d.beam + ((size_t)((n.t + 1) & 1) * d.B + j) * 5;
			#pragma unroll
			for (int q = 0; q < 5; q++) dst[q] = x[q];
			d.back[(size_t)(n.t + 1) * d.B + j] = ((uint32_t)i << 4) | (uint32_t)a;
		}
	}
	if (inside) {                                                           // the election is read (k_beam_keys): the slots go back
		const uint32_t sl = d.slot[c];
		if (sl != NO_SLOT && sl <= d.mask) d.table[sl] = 0u;
	}
	if (b == nblocks - 1 && threadIdx.x == 0) d.ctr[W_MNEXT] = base0 + tot0 + min(base1 + tot1, kt);
}

__global__ __launch_bounds__(ASCAN)
void k_beam_commit(BeamDev d) { beam_commit(d); }

// the twelve rows of every member of F_{t+1}, a wave per member; rows beyond 12 m_{t+1} keep the legal states they hold
__device__ __forceinline__ void beam_rows(const BeamDev &d)
{
	__shared__ u32x4 s_act[36];
	const BeamNow n = beam_now(d);
	if (!n.run || beam_stops(d) || d.ctr[W_ERROR] != BEAM_ERR_NONE) return;
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (j >= d.ctr[W_MNEXT] || j >= d.B) return;
	uint32_t s[5];
	load5(beam_half(d, n.t + 1) + (size_t)j * 5, s);
	for (uint32_t a = 0; a < 12; a++) {
		uint32_t child[5] = {s[0], s[1], s[2], s[3], s[4]}, tab[12];
		load_action_table(s_act, a, tab);
		move5(child, tab);
		write_row(d.net_in, d.code, (size_t)j * 12 + a, child, lane, 64);
	}
}

__global__ __launch_bounds__(256)
void k_beam_rows(BeamDev d) { beam_rows(d); }

// one wave: the depth's outcome.  The only writer of the status, t, m_t and the explored count.
__device__ __forceinline__ void beam_end(const BeamDev &d)
{
	const BeamNow n = beam_now(d);
	if (!n.run) return;
	const int lane = threadIdx.x;
	const int n_live = d.ctr[W_NLIVE], win = d.ctr[W_WINKEY], m_next = d.ctr[W_MNEXT], err = d.ctr[W_ERROR];
	const long long explored = ctr64(d.ctr, W_EXPLORED);
	const bool spent = explored + n_live > ctr64(d.ctr, W_BUDGET);
	if (!spent && win == NO_WIN && err == BEAM_ERR_NONE)
		for (int q = lane; q < 4 * 256; q += 64) d.hist[q] = 0;
	if (lane != 0) return;
	if (spent) { d.ctr[W_STATUS] = BEAM_SPENT; return; }
	set_ctr64(d.ctr, W_EXPLORED, explored + n_live);
	if (win != NO_WIN) {
		const int c = win & ((1 << WIN_SHIFT) - 1);
		d.ctr[W_MEET_I] = c / 12;
		d.ctr[W_MEET_A] = c % 12;
		d.ctr[W_MEET_LEVEL] = win >> WIN_SHIFT;
		d.ctr[W_DEPTH] = n.t + 1;
		d.ctr[W_STATUS] = BEAM_SOLVED;
		return;
	}
	if (err != BEAM_ERR_NONE || m_next < 0 || m_next > d.B || n.t + 1 > d.D) {
		if (err == BEAM_ERR_NONE) d.ctr[W_ERROR] = BEAM_ERR_RECORD;
		d.ctr[W_STATUS] = BEAM_FAILED;
		return;
	}
	d.sizes[n.t + 1] = m_next;
	d.ctr[W_T] = n.t + 1;
	d.ctr[W_DEPTH] = n.t + 1;
	d.ctr[W_M] = m_next;
	d.ctr[W_NLIVE] = 0;
	d.ctr[W_WINKEY] = NO_WIN;
	d.ctr[W_TICKET] = 0;
	d.ctr[W_MNEXT] = 0;
	if (n.t + 1 == d.D) d.ctr[W_STATUS] = BEAM_DEPTH;
}

__global__ __launch_bounds__(64)
void k_beam_end(BeamDev d) { beam_end(d); }

// The action queue of a won search, one wave: back upward from the winning child's parent, the winning action, then the ball's
// descent from the winning child (none of the first two when the ball holds the start's orbit).  out[0] = length, -1 when the
// search has not won, -2 when the record does not lead to the start, the winning child is not what the search said, or the
// descent finds no way on.  Every lane computes the same; lane 0 writes.
__device__ __forceinline__ void beam_walk(const BeamDev &d, const SymBallView &b, int32_t *out, int max_len)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	const SymProbe sp = sym_probe(s_sym, 64, s_act);
	const int lane = sp.lane;
	if (lane == 0) out[0] = -1;
	if (d.ctr[W_STATUS] != BEAM_SOLVED) return;
	const int t = d.ctr[W_T], a = d.ctr[W_MEET_A], level = d.ctr[W_MEET_LEVEL];
	int i = d.ctr[W_MEET_I];
	if (lane == 0) out[0] = -2;
	uint32_t x[5];
	int own = 0;
	if (a < 0) {
		load5(d.root, x);
	} else {
		if (t < 0 || t >= d.D || t + 1 > max_len || (uint32_t)i >= (uint32_t)d.B || a >= N_ACTIONS) return;
		child_state(beam_half(d, t), i, s_act, (uint32_t)a, x);
		if (lane == 0) out[1 + t] = a;
		for (int tt = t; tt >= 1; tt--) {
			const uint32_t w = d.back[(size_t)tt * d.B + i];
			if (lane == 0) out[tt] = (int)(w & 15u);
			i = (int)(w >> 4);
			if ((uint32_t)i >= (uint32_t)d.B || (w & 15u) >= (uint32_t)N_ACTIONS) return;
		}
		if (i != 0) return;                                                 // F_0 is the start alone
		own = t + 1;
	}
	bool ok;
	int len = own;
	if (d.has_ball) {
		ok = sb_level(b, sp, x) == level;
		if (ok) len = own + sb_descend(b, sp, x, level, [&](int k, int act) { if (own + k < max_len && lane == 0) out[1 + own + k] = act; }, &ok);
	} else {
		ok = is_solved5(x);
	}
	if (lane == 0) out[0] = ok ? len : -2;
}

__global__ __launch_bounds__(64)
void k_beam_walk(BeamDev d, SymBallView b, int32_t *out, int max_len) { beam_walk(d, b, out, max_len); }

// ---- S searches in lock-step (rk_beamb_*) ----
// Slot s is a whole search of its own: `base` describes slot 0, and every array of slot s lies s times its own length further on
// (the net batch: rows [12 B s, 12 B (s + 1)) of the one batch, whose values are out[12 B s ..] of the one forward).  The launches
// of a depth are the single engine's with the slot in the grid's second dimension; nothing is shared between slots but the ball.
constexpr int BEAMB_MAX_SLOTS = 1024;

struct BeamSlots {
	BeamDev base;
	int S;
	uint32_t n_words;                           // look-back words per slot
};

__device__ __forceinline__ size_t beam_row_bytes(int code) { return code == RK_OH_STATES ? 20 : code == RK_OH_F32 ? 1920 : 960; }

__device__ __forceinline__ BeamDev beam_slot(const BeamSlots &b, int s)
{
	BeamDev d = b.base;
	const size_t q = (size_t)s, B = (size_t)d.B, K = 12 * B, D1 = (size_t)d.D + 1;
	d.beam += q * 2 * B * 5; d.back += q * D1 * B; d.sizes += q * D1; d.table += q * ((size_t)d.mask + 1);
	d.slot += q * K; d.key += q * K; d.level += q * K; d.hist += q * 4 * 256; d.words += q * b.n_words; d.ctr += q * W_COUNT; d.root += q * 8;
	d.net_in = reinterpret_cast<char *>(d.net_in) + q * K * beam_row_bytes(d.code);
	return d;
}

// reset, over the n named slots (blockIdx.y indexes `slots`): what the single engine's reset clears with four memsets ...
__global__ __launch_bounds__(256)
void kb_beam_clear(BeamSlots b, const int32_t *slots)
{
	const BeamDev d = beam_slot(b, slots[blockIdx.y]);
	const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
	for (size_t i = at; i <= (size_t)d.mask; i += step) d.table[i] = 0u;
	for (size_t i = at; i < (size_t)b.n_words; i += step) d.words[i] = 0ull;
	for (size_t i = at; i < 4 * 256; i += step) d.hist[i] = 0;
	for (size_t i = at; i <= (size_t)d.D; i += step) d.sizes[i] = 0;
}

// ... its root, from the uploaded starts and budgets (slot slots[j] starts from start j) ...
__global__ __launch_bounds__(64)
void kb_beam_root(BeamSlots b, SymBallView v, const int32_t *slots, const uint32_t *starts, const long long *budgets)
{
	beam_root(beam_slot(b, slots[blockIdx.y]), v, starts + (size_t)blockIdx.y * 5, budgets[blockIdx.y]);
}

// ... and its rows
__global__ __launch_bounds__(256)
void kb_beam_fill(BeamSlots b, const int32_t *slots) { beam_fill(beam_slot(b, slots[blockIdx.y]), true); }

// every slot (blockIdx.y is the slot): the solved state in all its rows, for a batch form that was just handed out
__global__ __launch_bounds__(256)
void kb_beam_fill_solved(BeamSlots b) { beam_fill(beam_slot(b, blockIdx.y), false); }

// a thread per named slot (slots null: every slot): a running search is put to rest.  Only the status word is written.
__global__ __launch_bounds__(256)
void kb_beam_rest(BeamSlots b, const int32_t *slots, int n)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n) return;
	int32_t *ctr = beam_slot(b, slots != nullptr ? slots[j] : j).ctr;
	if (ctr[W_STATUS] == BEAM_RUNNING) ctr[W_STATUS] = BEAM_IDLE;
}

// The ball look-ups of all running slots.  The grid is (gx, S) with gx S workgroups in the order of the single engine's grid, but a
// workgroup does not belong to slot blockIdx.y: the live work -- units of four children, a wave each, of the running slots, slot
// after slot -- is dealt out over ALL workgroups, so that a few running slots among many idle ones still get the whole launch.
// A workgroup beyond the units leaves before it stages the symmetry tables.
__global__ __launch_bounds__(256)
void kb_beam_ball(BeamSlots bs, SymBallView b)
{
	__shared__ uint32_t s_sym[SYM_LDS_DWORDS];
	__shared__ u32x4 s_act[36];
	__shared__ int s_first[BEAMB_MAX_SLOTS + 1], s_w[4];                    // s_first[s]: the first unit of slot s; [S]: all units
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	int mine[4], sum = 0;
	#pragma unroll
	for (int q = 0; q < 4; q++) {
		const int s = tid * 4 + q;
		mine[q] = 0;
		if (s < bs.S) {
			const BeamNow n = beam_now(beam_slot(bs, s));
			if (n.run) mine[q] = (12 * n.m + 3) / 4;
		}
		sum += mine[q];
	}
	int incl = sum;
	#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const int y = __shfl_up(incl, off, 64);
		if (lane >= off) incl += y;
	}
	if (lane == 63) s_w[wv] = incl;
	__syncthreads();
	int before = incl - sum;
	#pragma unroll
	for (int w = 0; w < 4; w++) before += w < wv ? s_w[w] : 0;
	#pragma unroll
	for (int q = 0; q < 4; q++) {
		if (tid * 4 + q <= bs.S) s_first[tid * 4 + q] = before;                 // (slot S, if a thread has it, holds no units: the total)
		before += mine[q];
	}
	if (tid == 255 && bs.S == BEAMB_MAX_SLOTS) s_first[BEAMB_MAX_SLOTS] = before;
	__syncthreads();
	const int total = s_first[bs.S];
	const int g = blockIdx.y * gridDim.x + blockIdx.x, G = gridDim.x * gridDim.y;
	if (g >= total) return;
	const SymProbe sp = sym_probe(s_sym, 256, s_act);
	for (int u = g; u < total; u += G) {
		int lo = 0, hi = bs.S - 1;                                             // the last slot whose first unit is <= u: the one that holds u
		while (lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if (s_first[mid] <= u) lo = mid; else hi = mid - 1;
		}
		const BeamDev d = beam_slot(bs, lo);
		const BeamNow n = beam_now(d);
		const int c = (u - s_first[lo]) * 4 + wv;
		if (c < 12 * n.m) beam_ball_child(d, n, b, sp, c);
	}
}

// the other launches of a depth: the slot is blockIdx.y, and a workgroup whose slot is not running leaves at once (beam_now)
__global__ __launch_bounds__(256)
void kb_beam_probe(BeamSlots b) { beam_probe(beam_slot(b, blockIdx.y)); }

__global__ __launch_bounds__(256)
void kb_beam_keys(BeamSlots b, const void *out, int bf16) { beam_keys(beam_slot(b, blockIdx.y), out, bf16, (size_t)blockIdx.y * 12 * b.base.B); }

__global__ __launch_bounds__(256)
void kb_beam_hist(BeamSlots b, int pass) { beam_hist(beam_slot(b, blockIdx.y), pass); }

__global__ __launch_bounds__(ASCAN)
void kb_beam_commit(BeamSlots b) { beam_commit(beam_slot(b, blockIdx.y)); }

__global__ __launch_bounds__(256)
void kb_beam_rows(BeamSlots b) { beam_rows(beam_slot(b, blockIdx.y)); }

__global__ __launch_bounds__(64)
void kb_beam_end(BeamSlots b) { beam_end(beam_slot(b, blockIdx.y)); }

// a wave per slot; row s of `out` has 1 + max_len words
__global__ __launch_bounds__(64)
void kb_beam_walk(BeamSlots b, SymBallView v, int32_t *out, int max_len)
{
	beam_walk(beam_slot(b, blockIdx.y), v, out + (size_t)blockIdx.y * (1 + (size_t)max_len), max_len);
}

}  // namespace rk

using namespace rk;

struct rk_beam {
	BeamDev d{};
	SymBallView view{};
	rk_symball *ball = nullptr;
	NetBatches batch{false};                    // not cleared: rk_beam_reset writes every row before a forward reads one
	int32_t *walk = nullptr;
	int walk_max = 0;
	size_t n_words = 0;
	Landing ctr_host;
	bool ready = false;
	DevPool pool{64};

	~rk_beam() { symball_detach(ball); }
};

// S searches in lock-step: every array of rk_beam S times over (b.base: slot 0), one net batch of S x 12 B rows per form
struct rk_beamb {
	BeamSlots b{};
	SymBallView view{};
	rk_symball *ball = nullptr;
	NetBatches batch{false};                    // not cleared: the first reset or rest in a form writes every row of every slot
	bool legal = false;                         // every row of the batch holds a state in the form of b.base.code
	int32_t *walk = nullptr, *slots_dev = nullptr;
	uint32_t *starts_dev = nullptr;
	long long *budgets_dev = nullptr;
	int walk_max = 0;                           // `walk` holds S rows of 1 + walk_max words
	std::vector<int32_t> ctr_spare;
	Landing ctr_host;
	DevPool pool{64};

	~rk_beamb() { symball_detach(ball); }
};

namespace {

constexpr int BEAM_MAX_WIDTH = 1 << 16, BEAM_MAX_DEPTH = 1 << 12;
constexpr unsigned BEAM_WAVE_GRID = 2048;       // workgroups of the wave-per-child launches that stage the symmetry tables

// the twelve status words of a search from its counter block
void beam_status_words(const int32_t *c, long long *o)
{
	o[0] = c[W_STATUS]; o[1] = c[W_DEPTH]; o[2] = ctr64(c, W_EXPLORED); o[3] = c[W_M]; o[4] = c[W_ERROR];
	o[5] = c[W_MEET_I]; o[6] = c[W_MEET_A]; o[7] = c[W_MEET_LEVEL]; o[8] = ctr64(c, W_BUDGET); o[9] = c[W_T];
	o[10] = o[11] = 0;
}

}  // namespace

extern "C" {

int rk_beam_create(rk_beam_t **out, rk_symball_t *ball, int width, int max_depth, int prune_inverse)
{
	if (!out) return fail(RK_EINVAL, "rk_beam_create: null out pointer");
	if (width < 1 || width > BEAM_MAX_WIDTH) return fail(RK_EINVAL, "rk_beam_create: width %d outside 1..%d", width, BEAM_MAX_WIDTH);
	if (max_depth < 1 || max_depth > BEAM_MAX_DEPTH) return fail(RK_EINVAL, "rk_beam_create: max_depth %d outside 1..%d", max_depth, BEAM_MAX_DEPTH);
	rk_beam *h = new rk_beam();
	if (ball != nullptr) {
		if (int e = symball_attach(ball, "rk_beam_create", &h->view)) { delete h; return e; }
		h->ball = ball;
	}
	BeamDev &d = h->d;
	d.B = width; d.D = max_depth; d.code = -1; d.prune = prune_inverse ? 1 : 0; d.has_ball = ball != nullptr ? 1 : 0;
	const size_t K = (size_t)12 * width;
	d.mask = (uint32_t)(table_slots(K, 1024) - 1);
	h->n_words = 2 * (size_t)blocks(K, ASCAN);
	h->walk_max = max_depth + 1 + SB_MAX_RADIUS;
	int e = RK_OK;
	#define A(ptr, cnt) if (!e) e = h->pool.alloc(&d.ptr, (cnt))
	A(beam, (size_t)2 * width * 5); A(back, ((size_t)max_depth + 1) * width); A(sizes, (size_t)max_depth + 1); A(table, (size_t)d.mask + 1);
	A(slot, K); A(key, K); A(level, K); A(hist, 4 * 256); A(words, h->n_words); A(ctr, W_COUNT); A(root, 8);
	#undef A
	if (!e) e = h->pool.alloc(&h->walk, (size_t)h->walk_max + 8);
	if (!e) h->ctr_host.reserve(W_COUNT);
	if (e) { (void)hipGetLastError(); delete h; return fail(RK_ECAPACITY, "rk_beam_create: no device memory for a beam of %d states and %d depths", width, max_depth); }
	*out = h;
	return RK_OK;
}

int rk_beam_destroy(rk_beam_t *h)
{
	delete h;                                   // the pool and the landing buffer go with it; the ball is let go
	return RK_OK;
}

int rk_beam_net_in(rk_beam_t *h, int out_dtype, void **d_ptr, size_t *rows)
{
	if (!h || !d_ptr || !rows) return fail(RK_EINVAL, "rk_beam_net_in: null argument");
	if (out_dtype < RK_OH_F32 || out_dtype > RK_OH_STATES) return fail(RK_EINVAL, "rk_beam_net_in: unknown dtype %d", out_dtype);
	BeamDev &d = h->d;
	const size_t n = (size_t)12 * d.B;
	if (int e = h->batch.get(h->pool, out_dtype, n, &d.net_in)) return e;
	if (d.code != out_dtype) h->ready = false;  // the batch of a running search is in the other form: reset first
	d.code = out_dtype;
	*d_ptr = d.net_in;
	*rows = n;
	return RK_OK;
}

int rk_beam_reset(rk_beam_t *h, const int8_t *h_start_state, long long max_states, void *stream)
{
	if (!h || !h_start_state) return fail(RK_EINVAL, "rk_beam_reset: null argument");
	BeamDev &d = h->d;
	if (d.code < 0) return fail(RK_ESTATE, "rk_beam_reset: ask for the net batch first (rk_beam_net_in)");
	if (max_states < 0) return fail(RK_EINVAL, "rk_beam_reset: max_states %lld < 0", max_states);
	if (int e = check_cubie_codes("rk_beam_reset", "start", h_start_state, 1)) return e;
	hipStream_t st = (hipStream_t)stream;
	h->ready = false;
	RK_HIP(hipMemcpyAsync(d.root, h_start_state, STATE_BYTES, hipMemcpyHostToDevice, st));
	RK_HIP(hipMemsetAsync(d.table, 0, ((size_t)d.mask + 1) * sizeof(uint32_t), st));
	RK_HIP(hipMemsetAsync(d.words, 0, h->n_words * sizeof(unsigned long long), st));           // look-back epochs restart
	RK_HIP(hipMemsetAsync(d.hist, 0, 4 * 256 * sizeof(int32_t), st));
	RK_HIP(hipMemsetAsync(d.sizes, 0, ((size_t)d.D + 1) * sizeof(int32_t), st));
	hipLaunchKernelGGL(k_beam_root, dim3(1), dim3(64), 0, st, d, h->view, max_states);
	hipLaunchKernelGGL(k_beam_fill, dim3(std::min(blocks((size_t)12 * d.B, 4), 4096u)), dim3(256), 0, st, d);
	RK_HIP(hipGetLastError());
	RK_HIP(hipStreamSynchronize(st));           // the host buffer may go away after return
	h->ready = true;
	return RK_OK;
}

int rk_beam_step(rk_beam_t *h, const void *d_out, int dtype, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_beam_step: reset the engine first");
	int bf16 = 0;
	if (int e = check_net_out("rk_beam_step", d_out, dtype, &bf16)) return e;
	const BeamDev &d = h->d;
	hipStream_t st = (hipStream_t)stream;
	const size_t K = (size_t)12 * d.B;
	const unsigned grid = blocks(K);
	if (d.has_ball) hipLaunchKernelGGL(k_beam_ball, dim3(std::min(blocks(K, 4), BEAM_WAVE_GRID)), dim3(256), 0, st, d, h->view);
	hipLaunchKernelGGL(k_beam_probe, dim3(grid), dim3(256), 0, st, d);
	hipLaunchKernelGGL(k_beam_keys, dim3(grid), dim3(256), 0, st, d, d_out, bf16);
	for (int pass = 1; pass < 4; pass++) hipLaunchKernelGGL(k_beam_hist, dim3(grid), dim3(256), 0, st, d, pass);
	hipLaunchKernelGGL(k_beam_commit, dim3(blocks(K, ASCAN)), dim3(ASCAN), 0, st, d);
	hipLaunchKernelGGL(k_beam_rows, dim3(blocks((size_t)d.B, 4)), dim3(256), 0, st, d);
	hipLaunchKernelGGL(k_beam_end, dim3(1), dim3(64), 0, st, d);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_beam_status(rk_beam_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_beam_status: bad argument");
	int32_t c[W_COUNT];
	if (int e = h->ctr_host.read(h->d.ctr, W_COUNT, c, (hipStream_t)stream)) return e;
	beam_status_words(c, h_status);
	return RK_OK;
}

int rk_beam_export(rk_beam_t *h, int depth, long long *h_sizes, long long *h_back, size_t back_len, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_beam_export: reset the engine first");
	const BeamDev &d = h->d;
	hipStream_t st = (hipStream_t)stream;
	if (int e = export_widened(d.sizes, (size_t)d.D + 1, h_sizes, st)) return e;
	if (h_back == nullptr || back_len == 0) return RK_OK;
	if (depth < 1 || depth > d.D) return fail(RK_EINVAL, "rk_beam_export: depth %d outside 1..%d", depth, d.D);
	if (back_len > (size_t)d.B) return fail(RK_EINVAL, "rk_beam_export: %zu words of a beam of %d", back_len, d.B);
	return export_widened(d.back + (size_t)depth * d.B, back_len, h_back, st);
}

long long rk_beam_path(rk_beam_t *h, long long *h_actions, size_t max_len, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_beam_path: reset the engine first");
	if (!h_actions && max_len != 0) return fail(RK_EINVAL, "rk_beam_path: null output");
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_beam_walk, dim3(1), dim3(64), 0, st, h->d, h->view, h->walk, h->walk_max);
	RK_HIP(hipGetLastError());
	int32_t len = 0;
	if (int e = read_walk(h->walk, (size_t)h->walk_max, h_actions, max_len, st, &len)) return e;
	if (len == -1) return fail(RK_ESTATE, "rk_beam_path: the search has not won");
	if (len < 0) return fail(RK_ESTATE, "rk_beam_path: the record does not lead from the start to the winning child and on to the solved state");
	return len;
}

// ---- the batch ----
int rk_beamb_create(rk_beamb_t **out, rk_symball_t *ball, int searches, int width, int max_depth, int prune_inverse)
{
	if (!out) return fail(RK_EINVAL, "rk_beamb_create: null out pointer");
	*out = nullptr;
	if (searches < 1 || searches > BEAMB_MAX_SLOTS) return fail(RK_EINVAL, "rk_beamb_create: searches %d outside 1..%d", searches, BEAMB_MAX_SLOTS);
	if (width < 1 || width > BEAM_MAX_WIDTH) return fail(RK_EINVAL, "rk_beamb_create: width %d outside 1..%d", width, BEAM_MAX_WIDTH);
	if ((long long)searches * width > BEAM_MAX_WIDTH)
		return fail(RK_EINVAL, "rk_beamb_create: searches * width = %lld exceeds %d", (long long)searches * width, BEAM_MAX_WIDTH);
	if (max_depth < 1 || max_depth > BEAM_MAX_DEPTH) return fail(RK_EINVAL, "rk_beamb_create: max_depth %d outside 1..%d", max_depth, BEAM_MAX_DEPTH);
	rk_beamb *h = new rk_beamb();
	if (ball != nullptr) {
		if (int e = symball_attach(ball, "rk_beamb_create", &h->view)) { delete h; return e; }
		h->ball = ball;
	}
	BeamDev &d = h->b.base;
	d.B = width; d.D = max_depth; d.code = -1; d.prune = prune_inverse ? 1 : 0; d.has_ball = ball != nullptr ? 1 : 0;
	const size_t S = (size_t)searches, K = (size_t)12 * width;
	d.mask = (uint32_t)(table_slots(K, 1024) - 1);
	h->b.S = searches;
	h->b.n_words = (uint32_t)(2 * (size_t)blocks(K, ASCAN));
	h->walk_max = max_depth + 1 + SB_MAX_RADIUS;
	int e = RK_OK;
	#define A(ptr, cnt) if (!e) e = h->pool.alloc(&d.ptr, S * (cnt))
	A(beam, (size_t)2 * width * 5); A(back, ((size_t)max_depth + 1) * width); A(sizes, (size_t)max_depth + 1); A(table, (size_t)d.mask + 1);
	A(slot, K); A(key, K); A(level, K); A(hist, 4 * 256); A(words, h->b.n_words); A(ctr, W_COUNT); A(root, 8);
	#undef A
	if (!e) e = h->pool.alloc(&h->walk, S * ((size_t)h->walk_max + 1));
	if (!e) e = h->pool.alloc(&h->slots_dev, S);
	if (!e) e = h->pool.alloc(&h->starts_dev, S * 5);
	if (!e) e = h->pool.alloc(&h->budgets_dev, S);
	if (e) {
		(void)hipGetLastError();
		delete h;
		return fail(RK_ECAPACITY, "rk_beamb_create: no device memory for %d beams of %d states and %d depths", searches, width, max_depth);
	}
	std::vector<int32_t> ctr(S * W_COUNT, 0);                                  // every slot at rest
	for (size_t s = 0; s < S; s++) { ctr[s * W_COUNT + W_STATUS] = BEAM_IDLE; ctr[s * W_COUNT + W_WINKEY] = NO_WIN; }
	hipError_t he = hipMemcpy(d.ctr, ctr.data(), ctr.size() * sizeof(int32_t), hipMemcpyHostToDevice);
	if (he == hipSuccess) he = hipStreamSynchronize(nullptr);                  // the counters are in place when create returns, whatever stream the first reset takes
	if (he != hipSuccess) { delete h; return fail(RK_EHIP, "rk_beamb_create: %s", hipGetErrorString(he)); }
	h->ctr_host.reserve(S * W_COUNT);
	h->ctr_spare.resize(S * W_COUNT);
	*out = h;
	return RK_OK;
}

int rk_beamb_destroy(rk_beamb_t *h)
{
	delete h;
	return RK_OK;
}

int rk_beamb_net_in(rk_beamb_t *h, int out_dtype, void **d_ptr, size_t *rows)
{
	if (!h || !d_ptr || !rows) return fail(RK_EINVAL, "rk_beamb_net_in: null argument");
	if (out_dtype < RK_OH_F32 || out_dtype > RK_OH_STATES) return fail(RK_EINVAL, "rk_beamb_net_in: unknown dtype %d", out_dtype);
	BeamDev &d = h->b.base;
	const size_t n = (size_t)h->b.S * 12 * d.B;
	if (int e = h->batch.get(h->pool, out_dtype, n, &d.net_in)) return e;
	if (d.code != out_dtype) h->legal = false;  // rows of the other form, or of none: the next reset writes every row of every slot
	d.code = out_dtype;
	*d_ptr = d.net_in;
	*rows = n;
	return RK_OK;
}

namespace {

// the named slots of a reset or a rest: in range, none twice
static int beamb_check_slots(const char *who, const rk_beamb *h, int n, const int32_t *slots)
{
	if (n < 0 || n > h->b.S) return fail(RK_EINVAL, "%s: %d slots of %d", who, n, h->b.S);
	if (n > 0 && !slots) return fail(RK_EINVAL, "%s: null argument", who);
	std::vector<char> named((size_t)h->b.S, 0);
	for (int j = 0; j < n; j++) {
		if (slots[j] < 0 || slots[j] >= h->b.S) return fail(RK_EINVAL, "%s: slot %d outside 0..%d", who, slots[j], h->b.S - 1);
		if (named[slots[j]]) return fail(RK_EINVAL, "%s: slot %d is named twice", who, slots[j]);
		named[slots[j]] = 1;
	}
	return RK_OK;
}

// The first reset or rest after a form was handed out: EVERY row of every slot gets the solved state in that form, and a search that
// was running in the other form is put to rest -- from here on a forward reads legal rows only, whichever slots are started.
static void beamb_make_legal(rk_beamb *h, hipStream_t st)
{
	if (h->legal) return;
	const BeamDev &d = h->b.base;
	const unsigned gx = std::min(blocks((size_t)12 * d.B, 4), std::max(1u, 4096u / (unsigned)h->b.S));
	hipLaunchKernelGGL(kb_beam_rest, dim3(blocks((size_t)h->b.S)), dim3(256), 0, st, h->b, (const int32_t *)nullptr, h->b.S);
	hipLaunchKernelGGL(kb_beam_fill_solved, dim3(gx, h->b.S), dim3(256), 0, st, h->b);
	h->legal = true;
}

}  // namespace

int rk_beamb_reset(rk_beamb_t *h, int n, const int32_t *slots, const int8_t *h_start_states, const long long *max_states, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_beamb_reset: null engine");
	BeamDev &d = h->b.base;
	if (d.code < 0) return fail(RK_ESTATE, "rk_beamb_reset: ask for the net batch first (rk_beamb_net_in)");
	if (int e = beamb_check_slots("rk_beamb_reset", h, n, slots)) return e;
	if (n == 0) return RK_OK;
	if (!h_start_states || !max_states) return fail(RK_EINVAL, "rk_beamb_reset: null argument");
	for (int j = 0; j < n; j++)
		if (max_states[j] < 0) return fail(RK_EINVAL, "rk_beamb_reset: max_states %lld of slot %d < 0", max_states[j], slots[j]);
	if (int e = check_cubie_codes("rk_beamb_reset", "start", h_start_states, (size_t)n)) return e;
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemcpyAsync(h->slots_dev, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
	RK_HIP(hipMemcpyAsync(h->starts_dev, h_start_states, (size_t)n * STATE_BYTES, hipMemcpyHostToDevice, st));
	RK_HIP(hipMemcpyAsync(h->budgets_dev, max_states, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, st));
	beamb_make_legal(h, st);
	const size_t longest = std::max<size_t>((size_t)d.mask + 1, (size_t)d.D + 1);
	hipLaunchKernelGGL(kb_beam_clear, dim3(std::min(blocks(longest), 256u), n), dim3(256), 0, st, h->b, h->slots_dev);
	hipLaunchKernelGGL(kb_beam_root, dim3(1, n), dim3(64), 0, st, h->b, h->view, h->slots_dev, h->starts_dev, h->budgets_dev);
	hipLaunchKernelGGL(kb_beam_fill, dim3(std::min(blocks((size_t)12 * d.B, 4), 256u), n), dim3(256), 0, st, h->b, h->slots_dev);
	RK_HIP(hipGetLastError());
	RK_HIP(hipStreamSynchronize(st));           // the host buffers may go away after return
	return RK_OK;
}

int rk_beamb_rest(rk_beamb_t *h, int n, const int32_t *slots, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_beamb_rest: null engine");
	if (h->b.base.code < 0) return fail(RK_ESTATE, "rk_beamb_rest: ask for the net batch first (rk_beamb_net_in)");
	if (int e = beamb_check_slots("rk_beamb_rest", h, n, slots)) return e;
	hipStream_t st = (hipStream_t)stream;
	beamb_make_legal(h, st);
	if (n > 0) {
		RK_HIP(hipMemcpyAsync(h->slots_dev, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(kb_beam_rest, dim3(blocks((size_t)n)), dim3(256), 0, st, h->b, (const int32_t *)h->slots_dev, n);
	}
	RK_HIP(hipGetLastError());
	RK_HIP(hipStreamSynchronize(st));
	return RK_OK;
}

int rk_beamb_step(rk_beamb_t *h, const void *d_out, int dtype, void *stream)
{
	if (!h || !h->legal) return fail(RK_ESTATE, "rk_beamb_step: reset the engine first");
	int bf16 = 0;
	if (int e = check_net_out("rk_beamb_step", d_out, dtype, &bf16)) return e;
	const BeamDev &d = h->b.base;
	hipStream_t st = (hipStream_t)stream;
	const size_t K = (size_t)12 * d.B;
	const unsigned S = (unsigned)h->b.S;
	const dim3 grid(blocks(K), S);
	if (d.has_ball) {                           // (gx S workgroups in all, dealt out over the running slots' children)
		const unsigned gx = std::min(blocks(K, 4), std::max(1u, BEAM_WAVE_GRID / S));
		hipLaunchKernelGGL(kb_beam_ball, dim3(gx, S), dim3(256), 0, st, h->b, h->view);
	}
	hipLaunchKernelGGL(kb_beam_probe, grid, dim3(256), 0, st, h->b);
	hipLaunchKernelGGL(kb_beam_keys, grid, dim3(256), 0, st, h->b, d_out, bf16);
	for (int pass = 1; pass < 4; pass++) hipLaunchKernelGGL(kb_beam_hist, grid, dim3(256), 0, st, h->b, pass);
	hipLaunchKernelGGL(kb_beam_commit, dim3(blocks(K, ASCAN), S), dim3(ASCAN), 0, st, h->b);
	hipLaunchKernelGGL(kb_beam_rows, dim3(blocks((size_t)d.B, 4), S), dim3(256), 0, st, h->b);
	hipLaunchKernelGGL(kb_beam_end, dim3(1, S), dim3(64), 0, st, h->b);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_beamb_status(rk_beamb_t *h, long long *h_status, void *stream)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_beamb_status: null argument");
	const int32_t *c = nullptr;
	if (int e = h->ctr_host.fetch(h->b.base.ctr, (size_t)h->b.S * W_COUNT, h->ctr_spare.data(), (hipStream_t)stream, &c)) return e;
	for (int s = 0; s < h->b.S; s++, c += W_COUNT) beam_status_words(c, h_status + (size_t)s * 12);
	return RK_OK;
}

int rk_beamb_paths(rk_beamb_t *h, int32_t *h_out, int max_len, void *stream)
{
	if (!h || !h_out) return fail(RK_EINVAL, "rk_beamb_paths: null argument");
	if (max_len < 0 || max_len > h->walk_max) return fail(RK_EINVAL, "rk_beamb_paths: max_len %d outside 0..%d", max_len, h->walk_max);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(kb_beam_walk, dim3(1, h->b.S), dim3(64), 0, st, h->b, h->view, h->walk, max_len);
	RK_HIP(hipGetLastError());
	RK_HIP(hipMemcpyAsync(h_out, h->walk, (size_t)h->b.S * (1 + (size_t)max_len) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	RK_HIP(hipStreamSynchronize(st));
	return RK_OK;
}

int rk_beamb_export(rk_beamb_t *h, int slot, int depth, long long *h_sizes, long long *h_back, size_t back_len, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_beamb_export: null engine");
	const BeamDev &d = h->b.base;
	if (slot < 0 || slot >= h->b.S) return fail(RK_EINVAL, "rk_beamb_export: slot %d outside 0..%d", slot, h->b.S - 1);
	hipStream_t st = (hipStream_t)stream;
	const size_t D1 = (size_t)d.D + 1;
	if (int e = export_widened(d.sizes + (size_t)slot * D1, D1, h_sizes, st)) return e;
	if (h_back == nullptr || back_len == 0) return RK_OK;
	if (depth < 1 || depth > d.D) return fail(RK_EINVAL, "rk_beamb_export: depth %d outside 1..%d", depth, d.D);
	if (back_len > (size_t)d.B) return fail(RK_EINVAL, "rk_beamb_export: %zu words of a beam of %d", back_len, d.B);
	return export_widened(d.back + ((size_t)slot * D1 + (size_t)depth) * d.B, back_len, h_back, st);
}

}  // extern "C"
