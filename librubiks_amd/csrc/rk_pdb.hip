// Pattern databases (rk_pdb_*): a dense table of exact distances for a partial goal -- some cubies home, the rest anywhere.
//
// A 20-byte state keeps one code per cubie and a move maps every code on its own, new[c] = lut[action][kind][old[c]], so the
// codes of any subset of cubies are closed under the 12 moves.  The selected codes are ranked to a table index (the definition is
// in include/rubiks_hip.h and DESIGN 3.59.7: partial-permutation rank and orientation word of the corners, then of the edges) and
// the table holds one byte per index: the number of quarter turns that bring the selected cubies home, 255 = not reached.
//
// The build.  The goal's entry is 0; level d is ONE sweep launch over the whole table.  A thread loads 16 consecutive entries
// with one 128-bit load and leaves at once when none equals d.  For an entry equal to d it unranks the index to the selected
// codes, applies the 12 moves through the per-action tables staged in LDS (576 bytes), ranks each child and stores d + 1 with a
// plain byte store where the child's entry still reads 255.  WHY THAT IS EXACT WITHOUT ATOMICS: before the launch every entry
// <= d is final and every other is 255.  During it the only value stored is d + 1 and only over an entry that some thread read
// as 255, i.e. over 255 or over another thread's d + 1: racing writers store the same byte, a byte store touches no neighbour,
// and the sweep only looks for == d, which no store of this launch creates or removes.  After the launch an entry is d + 1
// exactly when it was unreached and has a parent at level d: breadth-first distance, whatever the scheduling.
// The sweep also counts the entries equal to d (a wave reduction, one atomicAdd per workgroup); the host reads the count after
// each level and stops at the first empty one.  The build passes when the counts add up to the size and level 0 holds one entry.
//
// Registers.  The selected codes live packed, one byte each in selection order: corners in two dwords, edges in three (the shape move5 takes; the size cap admits seven edges at most, so the loops unroll to seven); slots past
// kc / ke hold code 0 and are never ranked.  A move is lut4 on the five dwords (move5).  Every loop over the selected cubies is
// unrolled to the maximum with a wave-uniform bound test, so nothing is indexed dynamically in registers.  A query gathers the
// selected bytes of a row with v_perm_b32 by selectors made at create: what the other bytes hold cannot matter.
//
// A bound (rk_bound_*) is the descriptors of 1..4 built tables in one handle: rk_bound_depth answers the greatest entry of a
// state over them in one launch, and the deepening probes of rk_sym.hip prune by it (rk_pdb_dev.h: pdb_bound).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_group_tables.h"
#include "rk_pdb_dev.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"
#include "rk_table_host.h"

namespace rk {

constexpr int PDB_MAX_EDGES = 10;                   // ke = 11 or 12: the parity of the edge permutation is bound to the corners'
constexpr int PDB_MAX_LEVELS = 59;                  // what rk_pdb_status has room for; no pattern comes near

constexpr uint32_t pdb_chi_bits()
{
	uint32_t b = 0;
	for (int q = 0; q < 8; q++) b |= (uint32_t)GROUP_TABLES.chi[q] << q;
	return b;
}
constexpr uint32_t PDB_CHI_BITS = pdb_chi_bits();

// the d-th free position, ascending
__device__ __forceinline__ uint32_t pdb_nth_free(uint32_t free, uint32_t d)
{
	for (; d != 0u; d--) free &= free - 1u;
	return (uint32_t)__ffs((int)free) - 1u;
}

// The packed selected codes of an index below p.size.
__device__ __forceinline__ void pdb_unrank(const PdbDesc &p, uint32_t index, uint32_t c[2], uint32_t e[3])
{
	uint32_t oe = index & ((1u << p.ke) - 1u);
	index >>= p.ke;
	uint32_t re = index % p.Pe;
	index /= p.Pe;
	uint32_t oc = index % p.Oc, rc = index / p.Oc;
	uint32_t dg[8], tw[8];
	c[0] = c[1] = e[0] = e[1] = e[2] = 0u;

	#pragma unroll
	for (int i = PDB_EDGE_SLOTS - 1; i >= 0; i--)
		if ((uint32_t)i < p.ke) {
			dg[i] = re % (uint32_t)(12 - i);
			re /= (uint32_t)(12 - i);
		}
	uint32_t used = 0;
	#pragma unroll
	for (int i = 0; i < PDB_EDGE_SLOTS; i++)
		if ((uint32_t)i < p.ke) {
			const uint32_t pos = pdb_nth_free(~used & 0xFFFu, dg[i]);
			used |= 1u << pos;
			e[i >> 2] |= (2u * pos + ((oe >> (p.ke - 1u - (uint32_t)i)) & 1u)) << (8 * (i & 3));
		}

	#pragma unroll
	for (int i = 7; i >= 0; i--) {
		if ((uint32_t)i < p.kc) {
			dg[i] = rc % (uint32_t)(8 - i);
			rc /= (uint32_t)(8 - i);
		}
		if ((uint32_t)i < p.oc_digits) {
			tw[i] = oc % 3u;
			oc /= 3u;
		}
	}
	used = 0;
	uint32_t twist = 0;
	#pragma unroll
	for (int i = 0; i < 8; i++)
		if ((uint32_t)i < p.kc) {
			const uint32_t pos = pdb_nth_free(~used & 0xFFu, dg[i]);
			used |= 1u << pos;
			uint32_t k;
			if ((uint32_t)i < p.oc_digits) {
				k = tw[i];
			} else {
				// all eight corners, the last one: the digit whose twist makes the sum 0 mod 3; tau(3 q + k) = k, or -k where q has
				// the other chirality
				const uint32_t want = (3u - twist % 3u) % 3u;
				k = (PDB_CHI_BITS >> pos) & 1u ? (3u - want) % 3u : want;
			}
			const uint32_t code = 3u * pos + k;
			twist += (uint32_t)(GROUP_TAU_BITS >> (2u * code)) & 3u;
			c[i >> 2] |= code << (8 * (i & 3));
		}
}

// a dword that has a zero byte: the classic test, exact for the question "is there one"
__device__ __forceinline__ bool pdb_has_zero_byte(uint32_t v) { return ((v - 0x01010101u) & ~v & 0x80808080u) != 0u; }

// Level d -> d + 1: see the head of this file.  count += the entries equal to d.
__global__ __launch_bounds__(256)
void k_pdb_sweep(PdbDesc p, uint32_t d, unsigned long long *count)
{
	__shared__ u32x4 s_tab[36];
	__shared__ uint32_t s_count[4];
	stage_action_tables(s_tab, (int)threadIdx.x);
	__syncthreads();
	const u32x4 *groups = reinterpret_cast<const u32x4 *>(p.table);
	const uint32_t d4 = d * 0x01010101u;
	uint32_t mine = 0;
	for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < (size_t)p.groups; g += (size_t)gridDim.x * 256) {
		const u32x4 v = groups[g];
		const uint32_t w[4] = {v.x ^ d4, v.y ^ d4, v.z ^ d4, v.w ^ d4};
		if (!(pdb_has_zero_byte(w[0]) || pdb_has_zero_byte(w[1]) || pdb_has_zero_byte(w[2]) || pdb_has_zero_byte(w[3]))) continue;
		#pragma unroll 1
		for (uint32_t j = 0; j < 16u; j++) {
			const uint32_t word = j < 4u ? w[0] : j < 8u ? w[1] : j < 12u ? w[2] : w[3];
			if (((word >> (8u * (j & 3u))) & 0xFFu) != 0u) continue;
			mine++;
			uint32_t c[2], e[3];
			pdb_unrank(p, (uint32_t)g * 16u + j, c, e);                  // below p.size: the bytes past it are 255, never d
			#pragma unroll 1
			for (uint32_t a = 0; a < (uint32_t)N_ACTIONS; a++) {
				uint32_t tab[12], s[5] = {c[0], c[1], e[0], e[1], e[2]}, child;
				load_action_table(s_tab, a, tab);
				move5(s, tab);
				pdb_rank(p, s, s + 2, child);                            // a move keeps the positions distinct and the codes below 24
				if (child < p.size && p.table[child] == PDB_UNREACHED) p.table[child] = (uint8_t)(d + 1u);
			}
		}
	}
	#pragma unroll
	for (int m = 32; m > 0; m >>= 1) mine += (uint32_t)__shfl_xor((int)mine, m, 64);
	if ((threadIdx.x & 63u) == 0u) s_count[threadIdx.x >> 6] = mine;
	__syncthreads();
	if (threadIdx.x == 0) {
		const uint32_t all = s_count[0] + s_count[1] + s_count[2] + s_count[3];
		if (all != 0u) atomicAdd(count, (unsigned long long)all);
	}
}

__global__ void k_pdb_root(PdbDesc p)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		// the goal: the selected cubies at home
		uint32_t c[2] = {0u, 0u}, e[3] = {0u, 0u, 0u}, index;
		const uint32_t home_c[2] = {SOLVED_DW[0], SOLVED_DW[1]}, home_e[3] = {SOLVED_DW[2], SOLVED_DW[3], SOLVED_DW[4]};
		const uint32_t x[5] = {home_c[0], home_c[1], home_e[0], home_e[1], home_e[2]};
		if (pdb_gather(p, x, c, e) && pdb_rank(p, c, e, index) && index < p.size) p.table[index] = 0;
	}
}

// depth[q] = the entry of row q's selected codes, -1 for a row whose selected codes are no partial pattern
__global__ __launch_bounds__(256)
void k_pdb_depth(PdbDesc p, const uint32_t *states, size_t n, int32_t *depth)
{
	for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
		uint32_t x[5], c[2], e[3], index = 0;
		load5(states + q * 5, x);
		const bool ok = pdb_gather(p, x, c, e) && pdb_rank(p, c, e, index) && index < p.size;
		depth[q] = ok ? (int32_t)p.table[index] : -1;
	}
}

// bound[q] = the greatest entry of row q over the tables of B, -1 where it has none in any of them
__global__ __launch_bounds__(256)
void k_bound_depth(PdbBound B, const uint32_t *states, size_t n, int32_t *bound)
{
	for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
		uint32_t x[5];
		load5(states + q * 5, x);
		int best = -1;
		#pragma unroll
		for (int k = 0; k < PDB_BOUND_MAX; k++)
			if (k < B.n) best = max(best, pdb_entry(B.db[k], x));
		bound[q] = best;
	}
}

// The descent: at each step the lowest action whose child's entry is one less.  `stride` = the deepest level = the row length.
__global__ __launch_bounds__(256)
void k_pdb_solve(PdbDesc p, const uint32_t *states, size_t n, uint32_t stride, int32_t *lengths, int8_t *actions, int32_t *error)
{
	__shared__ u32x4 s_tab[36];
	stage_action_tables(s_tab, (int)threadIdx.x);
	__syncthreads();
	for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
		uint32_t x[5], c[2], e[3], index = 0;
		load5(states + q * 5, x);
		const bool ok = pdb_gather(p, x, c, e) && pdb_rank(p, c, e, index) && index < p.size;
		int8_t *row = actions + q * (size_t)stride;
		uint32_t cur = ok ? (uint32_t)p.table[index] : 0u, t = 0;
		bool lost = ok && cur > stride;                                  // an unreached entry: never in a table that passed its build
		const uint32_t len = cur;
		while (ok && !lost && cur != 0u) {
			uint32_t a = 0, s[5];
			for (; a < (uint32_t)N_ACTIONS; a++) {
				uint32_t tab[12], child;
				s[0] = c[0]; s[1] = c[1]; s[2] = e[0]; s[3] = e[1]; s[4] = e[2];
				load_action_table(s_tab, a, tab);
				move5(s, tab);
				pdb_rank(p, s, s + 2, child);
				if (child < p.size && (uint32_t)p.table[child] == cur - 1u) break;
			}
			if (a == (uint32_t)N_ACTIONS) { lost = true; break; }
			c[0] = s[0]; c[1] = s[1]; e[0] = s[2]; e[1] = s[3]; e[2] = s[4];
			row[t++] = (int8_t)a;
			cur--;
		}
		if (lost) { *error = RK_ESTATE; t = 0; }
		for (; t < stride; t++) row[t] = -1;
		lengths[q] = ok && !lost ? (int32_t)len : -1;
	}
}

}  // namespace rk

using namespace rk;

struct rk_pdb {
	PdbDesc d{};
	uint8_t corners[8] = {}, edges[12] = {};
	bool built = false;
	int levels = 0;
	long long level_size[PDB_MAX_LEVELS] = {};
	unsigned long long *d_count = nullptr;

	void drop()
	{
		if (d.table) (void)hipFree(d.table);
		if (d_count) (void)hipFree(d_count);
		d.table = nullptr;
		d_count = nullptr;
	}
	~rk_pdb() { drop(); }
};

namespace {

unsigned pdb_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, (size_t)RK_PDB_GRID); }

// the cubies of a kind: ascending, below `limit`
int check_pdb_cubies(const char *kind, const uint8_t *cubies, int k, int limit)
{
	if (k < 0 || k > limit) return fail(RK_EINVAL, "rk_pdb_create: %d %s outside 0..%d", k, kind, limit);
	if (k > 0 && !cubies) return fail(RK_EINVAL, "rk_pdb_create: null pointer");
	for (int i = 0; i < k; i++) {
		if (cubies[i] >= limit) return fail(RK_EINVAL, "rk_pdb_create: %s cubie %d outside 0..%d", kind, (int)cubies[i], limit - 1);
		if (i > 0 && cubies[i] <= cubies[i - 1]) return fail(RK_EINVAL, "rk_pdb_create: the %s must ascend without repeats", kind);
	}
	return RK_OK;
}

int check_pdb_queries(const char *who, const rk_pdb *h, const void *d_states, size_t n, const void *out)
{
	if (!h) return fail(RK_EINVAL, "%s: null handle", who);
	if (!h->built) return fail(RK_ESTATE, "%s: build the table first", who);
	if (int e = check_state_rows(who, d_states, n)) return e;
	return check_state_rows(who, out, n);                                   // the output: n dwords, the same three tests
}

}  // namespace

extern "C" {

int rk_pdb_create(rk_pdb_t **out, const uint8_t *h_corners, int kc, const uint8_t *h_edges, int ke)
{
	if (!out) return fail(RK_EINVAL, "rk_pdb_create: null out pointer");
	if (int e = check_pdb_cubies("corners", h_corners, kc, 8)) return e;
	if (int e = check_pdb_cubies("edges", h_edges, ke, 12)) return e;
	if (kc + ke < 1) return fail(RK_EINVAL, "rk_pdb_create: an empty pattern");
	if (ke > PDB_MAX_EDGES)
		return fail(RK_EINVAL, "rk_pdb_create: %d edges: with more than %d the permutation parity leaves entries unreachable", ke, PDB_MAX_EDGES);
	const int oc_digits = kc == 8 ? 7 : kc;
	unsigned long long Pc = 1, Oc = 1, Pe = 1;
	for (int i = 0; i < kc; i++) Pc *= (unsigned long long)(8 - i);
	for (int i = 0; i < oc_digits; i++) Oc *= 3;
	for (int i = 0; i < ke; i++) Pe *= (unsigned long long)(12 - i);
	const unsigned long long size = Pc * Oc * Pe << ke;                  // at most 8! 3^7 P(12, 10) 2^10: far below 2^64
	if (size > RK_PDB_MAX_SIZE) return fail(RK_EINVAL, "rk_pdb_create: %llu entries are more than %llu", size, RK_PDB_MAX_SIZE);
	if (ke > PDB_EDGE_SLOTS) return fail(RK_EINVAL, "rk_pdb_create: %d edges", ke);      // (never: eight edges are past the size cap)
	rk_pdb *h = new rk_pdb();
	PdbDesc &d = h->d;
	d.size = (uint32_t)size;
	d.groups = (uint32_t)((size + 15) / 16);
	d.kc = (uint32_t)kc; d.ke = (uint32_t)ke; d.oc_digits = (uint32_t)oc_digits;
	d.Oc = (uint32_t)Oc; d.Pe = (uint32_t)Pe;
	// selector byte 12 of v_perm_b32 yields 0x00: a slot that holds no selected cubie reads as code 0
	uint8_t sc[8], lo[12], hi[12];
	memset(sc, 12, sizeof sc); memset(lo, 12, sizeof lo); memset(hi, 12, sizeof hi);
	for (int i = 0; i < kc; i++) sc[i] = h->corners[i] = h_corners[i];
	for (int i = 0; i < ke; i++) {
		h->edges[i] = h_edges[i];
		if (h_edges[i] < 8) lo[i] = h_edges[i]; else hi[i] = (uint8_t)(h_edges[i] - 8);
	}
	memcpy(d.sel_c, sc, 8); memcpy(d.sel_lo, lo, 12); memcpy(d.sel_hi, hi, 12);
	*out = h;
	return RK_OK;
}

int rk_pdb_destroy(rk_pdb_t *h)
{
	delete h;
	return RK_OK;
}

int rk_pdb_build(rk_pdb_t *h, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_pdb_build: null handle");
	if (h->built) return RK_OK;
	hipStream_t st = (hipStream_t)stream;
	PdbDesc &d = h->d;
	h->drop();
	h->levels = 0;
	memset(h->level_size, 0, sizeof h->level_size);
	const size_t bytes = (size_t)d.groups * 16;
	if (hipMalloc((void **)&d.table, bytes) != hipSuccess || hipMalloc((void **)&h->d_count, PDB_MAX_LEVELS * sizeof(unsigned long long)) != hipSuccess) {
		(void)hipGetLastError();
		h->drop();
		return fail(RK_ECAPACITY, "rk_pdb_build: no device memory for a table of %u entries", d.size);
	}
	int err = RK_OK;
	const auto run = [&]() -> int {
		RK_HIP(hipMemsetAsync(d.table, (int)PDB_UNREACHED, bytes, st));
		RK_HIP(hipMemsetAsync(h->d_count, 0, PDB_MAX_LEVELS * sizeof(unsigned long long), st));
		hipLaunchKernelGGL(k_pdb_root, dim3(1), dim3(64), 0, st, d);
		RK_HIP(hipGetLastError());
		for (int level = 0; level < PDB_MAX_LEVELS; level++) {
			unsigned long long count = 0;
			hipLaunchKernelGGL(k_pdb_sweep, dim3(pdb_grid(d.groups)), dim3(256), 0, st, d, (uint32_t)level, h->d_count + level);
			RK_HIP(hipGetLastError());
			RK_HIP(hipMemcpyAsync(&count, h->d_count + level, sizeof count, hipMemcpyDeviceToHost, st));
			RK_HIP(hipStreamSynchronize(st));
			if (count == 0) break;
			h->level_size[h->levels++] = (long long)count;
		}
		return RK_OK;
	};
	err = run();
	(void)hipFree(h->d_count);
	h->d_count = nullptr;
	long long sum = 0;
	for (int l = 0; l < h->levels; l++) sum += h->level_size[l];
	if (!err && (sum != (long long)d.size || h->level_size[0] != 1))
		err = fail(RK_ESTATE, "rk_pdb_build: %d levels hold %lld entries of %u, level 0 holds %lld", h->levels, sum, d.size, h->level_size[0]);
	if (err) {                                                           // the handle stays unbuilt; the table goes at once
		h->drop();
		return err;
	}
	h->built = true;
	return RK_OK;
}

int rk_pdb_status(rk_pdb_t *h, long long *h_status)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_pdb_status: null argument");
	memset(h_status, 0, 64 * sizeof(long long));
	h_status[0] = h->built ? 1 : 0;
	h_status[1] = (long long)h->d.size;
	h_status[2] = (long long)h->d.kc;
	h_status[3] = (long long)h->d.ke;
	if (h->built) {
		h_status[4] = h->levels;
		for (int l = 0; l < h->levels; l++) h_status[5 + l] = h->level_size[l];
	}
	return RK_OK;
}

int rk_pdb_export(rk_pdb_t *h, size_t first, size_t count, uint8_t *h_bytes, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_pdb_export: null handle");
	if (!h->built) return fail(RK_ESTATE, "rk_pdb_export: build the table first");
	return export_table("rk_pdb_export", "table", 1, 1, &h->d.table, &h->d.size, first, count, h_bytes, stream);
}

int rk_pdb_depth(rk_pdb_t *h, const int8_t *d_states, size_t n, int32_t *d_depth, void *stream)
{
	if (int e = check_pdb_queries("rk_pdb_depth", h, d_states, n, d_depth)) return e;
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_pdb_depth, dim3(pdb_grid(n)), dim3(256), 0, (hipStream_t)stream, h->d, reinterpret_cast<const uint32_t *>(d_states), n,
	                   d_depth);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_pdb_solve(rk_pdb_t *h, const int8_t *d_states, size_t n, int32_t *d_lengths, int8_t *d_actions, int32_t *d_error, void *stream)
{
	if (int e = check_pdb_queries("rk_pdb_solve", h, d_states, n, d_lengths)) return e;
	if (!d_error || ((uintptr_t)d_error & 3u)) return fail(RK_EINVAL, "rk_pdb_solve: the error word must be a 4-byte aligned device pointer");
	if (n != 0 && !d_actions) return fail(RK_EINVAL, "rk_pdb_solve: null pointer");
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemsetAsync(d_error, 0, sizeof(int32_t), st));                // every argument has passed: nothing is enqueued by a refused call
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_pdb_solve, dim3(pdb_grid(n)), dim3(256), 0, st, h->d, reinterpret_cast<const uint32_t *>(d_states), n,
	                   (uint32_t)(h->levels - 1), d_lengths, d_actions, d_error);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_bound_create(rk_bound_t **out, rk_pdb_t *const *dbs, int n)
{
	if (!out) return fail(RK_EINVAL, "rk_bound_create: null out pointer");
	if (n < 1 || n > PDB_BOUND_MAX) return fail(RK_EINVAL, "rk_bound_create: %d databases outside 1..%d", n, PDB_BOUND_MAX);
	if (!dbs) return fail(RK_EINVAL, "rk_bound_create: null pointer");
	for (int k = 0; k < n; k++) {
		if (!dbs[k]) return fail(RK_EINVAL, "rk_bound_create: database %d is null", k);
		for (int j = 0; j < k; j++)
			if (dbs[j] == dbs[k]) return fail(RK_EINVAL, "rk_bound_create: databases %d and %d are the same", j, k);
	}
	for (int k = 0; k < n; k++)
		if (!dbs[k]->built) return fail(RK_ESTATE, "rk_bound_create: build database %d first", k);
	rk_bound *h = new rk_bound();
	for (int k = 0; k < n; k++) h->b.db[k] = dbs[k]->d;
	h->b.n = n;
	*out = h;
	return RK_OK;
}

int rk_bound_destroy(rk_bound_t *h)
{
	delete h;
	return RK_OK;
}

int rk_bound_depth(rk_bound_t *h, const int8_t *d_states, size_t n, int32_t *d_bound, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_bound_depth: null handle");
	if (int e = check_state_rows("rk_bound_depth", d_states, n)) return e;
	if (int e = check_state_rows("rk_bound_depth", d_bound, n)) return e;
	if (n == 0) return RK_OK;
	hipLaunchKernelGGL(k_bound_depth, dim3(pdb_grid(n)), dim3(256), 0, (hipStream_t)stream, h->b, reinterpret_cast<const uint32_t *>(d_states), n,
	                   d_bound);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

}  // extern "C"
