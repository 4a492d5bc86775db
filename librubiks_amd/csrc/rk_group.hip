// The cube group on 20-byte states (rk_group_*): composition, inverse, a state seen from a goal, and the legality of a row.
//
// Definitions (rk_group_tables.h).  A state b has a full action g_b on the 24 corner slots and the 24 edge slots.
//     apply(a, b)[c]    = g_b(a[c])                       the state after b's net effect is applied to a (a's word, then b's)
//     inverse(b)        : apply(b, inverse(b)) = apply(inverse(b), b) = solved
//     relative(s, goal) = apply(inverse(goal), s)         relabels the cubies by the goal; commutes with the 12 moves
//     legal(s)          : codes in range, positions a permutation, equal permutation parities, flip sum 0 mod 2, twist sum 0 mod 3
//
// Kernels: a thread per state under a capped grid, a row in and out as five dwords, nothing indexed dynamically in registers.
//   * edges need no table, g_b(2 p + k) = b[p] ^ k: the byte pick b[p] of four codes at once is v_perm_b32 over the three edge dwords,
//     as sym_conjugate (rk_sym_dev.h) picks its sources;
//   * corners read full[p][b[p]][0..2] and inv[p][b[p]] as ONE dword of a 1 KB image staged in LDS once per workgroup (8 homes x 32
//     codes); code / 3 and code % 3 of four codes at once are lut4 over constant tables, b[p] again a v_perm_b32;
//   * inverse and relative scatter a byte to a position: a 64-bit shift into a register pair, never a store to a private array.
// Every code is used as code & 31 and every home as a value 0..7 or 0..15 that the picks above cannot exceed, so a row of arbitrary
// bytes reads the image and the operands in bounds; what it gives is unspecified.  k_group_legal is the kernel that reports such rows.
// A thread reads its operands fully before it stores, so the output may be exactly one of the operands.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_group_dev.h"
#include "rk_group_tables.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"

namespace rk {

enum GroupOp { GROUP_APPLY, GROUP_INVERSE, GROUP_RELATIVE };

struct GroupDev { uint32_t dev[8][32]; };

constexpr GroupDev make_group_dev()
{
	GroupDev d{};
	for (int p = 0; p < 8; p++)
		for (int v = 0; v < 32; v++) d.dev[p][v] = GROUP_TABLES.dev[p][v];
	return d;
}

static __constant__ GroupDev D_GROUP = make_group_dev();

// byte `pos` (0..7) of the pair |= v; a position beyond 7 cannot be given
__device__ __forceinline__ void group_put8(uint32_t &lo, uint32_t &hi, uint32_t pos, uint32_t v)
{
	const unsigned long long w = (unsigned long long)v << (8u * pos);
	lo |= (uint32_t)w;
	hi |= (uint32_t)(w >> 32);
}

// byte `pos` (0..15) of the three edge dwords |= v; positions 12..15 are dropped
__device__ __forceinline__ void group_put12(uint32_t e[3], uint32_t pos, uint32_t v)
{
	const unsigned long long w = (unsigned long long)v << (8u * (pos & 7u));
	const bool low = pos < 8u;
	e[0] |= low ? (uint32_t)w : 0u;
	e[1] |= low ? (uint32_t)(w >> 32) : 0u;
	e[2] |= low ? 0u : (uint32_t)w;
}

// y = apply(a, b): y[c] = g_b(a[c])
__device__ __forceinline__ void group_apply(const uint32_t *lds, const uint32_t a[5], const uint32_t b[5], uint32_t y[5])
{
	#pragma unroll
	for (int j = 0; j < 2; j++) {
		const uint32_t p4 = group_div3(a[j]), sh4 = group_mod3(a[j]) << 3;                   // homes 0..7, 8 k
		const uint32_t idx4 = p4 << 5 | (bperm(b[1], b[0], p4) & 0x1F1F1F1Fu);              // 32 p + b[p]: below 256 in every byte
		uint32_t out = 0;
		#pragma unroll
		for (int i = 0; i < 4; i++) {
			const uint32_t e = lds[(idx4 >> (8 * i)) & 0xFFu];
			out |= ((e >> ((sh4 >> (8 * i)) & 0xFFu)) & 0xFFu) << (8 * i);
		}
		y[j] = out;
	}
	#pragma unroll
	for (int j = 2; j < 5; j++) {
		const uint32_t sel = (a[j] >> 1) & 0x0F0F0F0Fu;                                       // homes 0..15
		const uint32_t lo = bperm(b[3], b[2], sel & 0x07070707u);
		const uint32_t hi = bperm(0u, b[4], sel & 0x03030303u);
		const uint32_t m = bperm(0u, 0u, ((sel >> 3) & 0x01010101u) | 0x0C0C0C0Cu);          // 0xFF where the home is 8..15
		y[j] = ((hi & m) | (lo & ~m)) ^ (a[j] & 0x01010101u);
	}
}

// y = relative(s, g) = apply(inverse(g), s): cubie p of g lies at position pos with inv[p][g[p]] = 3 p + k there, and s sends that slot
// to full[p][s[p]][k]; an edge to s[p] ^ k.  RELATIVE = false: y = inverse(g) (the slot itself, s is not read).
template <bool RELATIVE>
__device__ __forceinline__ void group_relative(const uint32_t *lds, const uint32_t s[5], const uint32_t g[5], uint32_t y[5])
{
	y[0] = y[1] = y[2] = y[3] = y[4] = 0u;
	#pragma unroll
	for (int j = 0; j < 2; j++) {
		const uint32_t pos4 = group_div3(g[j]);
		#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int p = 4 * j + i;
			const uint32_t back = lds[32 * p + ((g[j] >> (8 * i)) & 31u)] >> 24;              // 3 p + k
			uint32_t v = back;
			if (RELATIVE) v = (lds[32 * p + ((s[j] >> (8 * i)) & 31u)] >> (8u * (back - 3u * p))) & 0xFFu;
			group_put8(y[0], y[1], (pos4 >> (8 * i)) & 7u, v);
		}
	}
	#pragma unroll
	for (int j = 2; j < 5; j++) {
		const uint32_t k4 = g[j] & 0x01010101u, pos4 = (g[j] >> 1) & 0x0F0F0F0Fu;
		const uint32_t home4 = 0x06040200u + 0x08080808u * (uint32_t)(j - 2);                // the home codes 2 p of the dword's four edges
		const uint32_t v4 = RELATIVE ? s[j] ^ k4 : home4 | k4;
		#pragma unroll
		for (int i = 0; i < 4; i++) group_put12(y + 2, (pos4 >> (8 * i)) & 0xFFu, (v4 >> (8 * i)) & 0xFFu);
	}
}

__device__ __forceinline__ void group_stage(uint32_t *lds /* 256 */)
{
	lds[threadIdx.x] = D_GROUP.dev[threadIdx.x >> 5][threadIdx.x & 31];
	__syncthreads();
}

// out[q] = apply(a[q], b[q]) / inverse(a[q]) / relative(a[q], b[q]); b_rows = 0: row 0 of b for every q
template <int OP>
__global__ __launch_bounds__(256)
void k_group(const uint32_t *a, size_t n, const uint32_t *b, size_t b_rows, uint32_t *out)
{
	__shared__ uint32_t s_group[256];
	group_stage(s_group);
	for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
		uint32_t x[5], z[5] = {}, y[5];
		load5(a + q * 5, x);
		if (OP != GROUP_INVERSE) load5(b + (b_rows ? q * 5 : 0), z);
		if (OP == GROUP_APPLY) group_apply(s_group, x, z, y);
		else if (OP == GROUP_INVERSE) group_relative<false>(s_group, x, x, y);
		else group_relative<true>(s_group, x, z, y);
		#pragma unroll
		for (int j = 0; j < 5; j++) out[q * 5 + j] = y[j];
	}
}

// flags[q] = 1 for a legal row; stats = [count, lowest index] of the others (either may be null; stats initialised to [0, INT64_MAX]).
// The lowest illegal lane of a wave reports for the wave: its row is the wave's lowest.
__global__ __launch_bounds__(256)
void k_group_legal(const uint32_t *states, size_t n, uint8_t *flags, long long *stats)
{
	for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
		uint32_t x[5];
		load5(states + q * 5, x);
		const bool ok = group_legal(x);
		if (flags != nullptr) flags[q] = ok ? 1 : 0;
		if (stats != nullptr) {
			const unsigned long long bad = __ballot(!ok);
			if (!ok && (int)(threadIdx.x & 63) == __ffsll((long long)bad) - 1) {
				atomicAdd(reinterpret_cast<unsigned long long *>(&stats[0]), (unsigned long long)__popcll(bad));
				atomicMin(&stats[1], (long long)q);
			}
		}
	}
}

}  // namespace rk

using namespace rk;

namespace {

unsigned group_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, (size_t)RK_GROUP_GRID); }

bool group_overlap(const void *p, size_t p_bytes, const void *q, size_t q_bytes)
{
	const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
	return a < b + q_bytes && b < a + p_bytes;
}

// the output may be exactly an operand of n rows; any other overlap is a race between threads
int check_group_out(const char *who, const void *d_out, size_t n, const void *d_in, size_t in_rows)
{
	if (d_out == d_in && in_rows == n) return RK_OK;
	if (group_overlap(d_out, n * STATE_BYTES, d_in, in_rows * STATE_BYTES))
		return fail(RK_EINVAL, "%s: the output overlaps an operand without being exactly it", who);
	return RK_OK;
}

template <int OP>
int group_binary(const char *who, const int8_t *d_a, size_t n, const int8_t *d_b, size_t b_rows, int8_t *d_out, void *stream)
{
	if (int e = check_state_rows(who, d_a, n)) return e;
	if (b_rows != n && b_rows != 1) return fail(RK_EINVAL, "%s: %zu second operands for %zu states: one, or one for each", who, b_rows, n);
	if (int e = check_state_rows(who, d_b, n)) return e;
	if (int e = check_state_rows(who, d_out, n)) return e;
	if (n == 0) return RK_OK;
	if (int e = check_group_out(who, d_out, n, d_a, n)) return e;
	if (int e = check_group_out(who, d_out, n, d_b, b_rows)) return e;
	hipLaunchKernelGGL((k_group<OP>), dim3(group_grid(n)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(d_a), n,
	                   reinterpret_cast<const uint32_t *>(d_b), b_rows == n ? n : (size_t)0, reinterpret_cast<uint32_t *>(d_out));
	RK_HIP(hipGetLastError());
	return RK_OK;
}

}  // namespace

extern "C" {

int rk_group_tables(uint8_t *h_full, uint8_t *h_inv, uint8_t *h_tau)
{
	if (!h_full && !h_inv && !h_tau) return fail(RK_EINVAL, "rk_group_tables: null output");
	if (h_full) memcpy(h_full, GROUP_TABLES.full, sizeof GROUP_TABLES.full);
	if (h_inv) memcpy(h_inv, GROUP_TABLES.inv, sizeof GROUP_TABLES.inv);
	if (h_tau) memcpy(h_tau, GROUP_TABLES.tau, sizeof GROUP_TABLES.tau);
	return RK_OK;
}

int rk_group_apply(const int8_t *d_states, size_t n, const int8_t *d_effects, size_t n_effects, int8_t *d_out, void *stream)
{
	return group_binary<GROUP_APPLY>("rk_group_apply", d_states, n, d_effects, n_effects, d_out, stream);
}

int rk_group_inverse(const int8_t *d_states, size_t n, int8_t *d_out, void *stream)
{
	if (int e = check_state_rows("rk_group_inverse", d_states, n)) return e;
	if (int e = check_state_rows("rk_group_inverse", d_out, n)) return e;
	if (n == 0) return RK_OK;
	if (int e = check_group_out("rk_group_inverse", d_out, n, d_states, n)) return e;
	hipLaunchKernelGGL((k_group<GROUP_INVERSE>), dim3(group_grid(n)), dim3(256), 0, (hipStream_t)stream,
	                   reinterpret_cast<const uint32_t *>(d_states), n, (const uint32_t *)nullptr, (size_t)0, reinterpret_cast<uint32_t *>(d_out));
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_group_relative(const int8_t *d_states, size_t n, const int8_t *d_goals, size_t n_goals, int8_t *d_out, void *stream)
{
	return group_binary<GROUP_RELATIVE>("rk_group_relative", d_states, n, d_goals, n_goals, d_out, stream);
}

int rk_group_legal(const int8_t *d_states, size_t n, uint8_t *d_flags, long long *d_stats, void *stream)
{
	if (int e = check_state_rows("rk_group_legal", d_states, n)) return e;
	if (d_stats && ((uintptr_t)d_stats & 7u)) return fail(RK_EINVAL, "rk_group_legal: stats must be 8-byte aligned");
	if (n == 0) return RK_OK;
	if (!d_flags && !d_stats) return fail(RK_EINVAL, "rk_group_legal: null pointer");
	if (d_flags && group_overlap(d_flags, n, d_states, n * STATE_BYTES)) return fail(RK_EINVAL, "rk_group_legal: the flags overlap the states");
	hipLaunchKernelGGL(k_group_legal, dim3(group_grid(n)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(d_states), n,
	                   d_flags, d_stats);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

}  // extern "C"
