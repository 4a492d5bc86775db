// Device-side pieces of the pattern databases that more than one engine uses: the descriptor of a built table, the index of the
// selected codes of a row (rk_pdb.hip builds and queries the tables with them) and the bound of a state over several tables
// (rk_pdb.hip reports it, rk_deepen_dev.h prunes the probes of rk_sym.hip by it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rk_device.h"
#include "rk_group_tables.h"

namespace rk {

constexpr int PDB_EDGE_SLOTS = 7;                   // the most edges a table of at most 2^31 entries has (eight: 5.1 G): what the loops unroll to
constexpr uint32_t PDB_UNREACHED = 255;
constexpr int PDB_BOUND_MAX = 4;                    // the most tables of a bound

struct PdbDesc {
	uint8_t *table;                                 // `groups` * 16 bytes; the bytes past `size` stay 255
	uint32_t size, groups;
	uint32_t kc, ke;
	uint32_t oc_digits;                             // corner orientation digits in the index: kc, 7 with all eight corners
	uint32_t Oc, Pe;                                // 3^oc_digits, P(12, ke)
	uint32_t sel_c[2], sel_lo[3], sel_hi[3];        // v_perm selectors: packed corners from row dwords 0..1, edges from 2..3 and from 4
};

// The built tables a bound reads, by value: db[0 .. n - 1].
struct PdbBound {
	PdbDesc db[PDB_BOUND_MAX];
	int n;
};

__device__ __forceinline__ uint32_t pdb_div3(uint32_t x)
{
	const uint32_t t[6] = {GROUP_TABLES.div3[0], GROUP_TABLES.div3[1], GROUP_TABLES.div3[2], GROUP_TABLES.div3[3], GROUP_TABLES.div3[4],
	                       GROUP_TABLES.div3[5]};
	return lut4(x, t);
}

__device__ __forceinline__ uint32_t pdb_mod3(uint32_t x)
{
	const uint32_t t[6] = {GROUP_TABLES.mod3[0], GROUP_TABLES.mod3[1], GROUP_TABLES.mod3[2], GROUP_TABLES.mod3[3], GROUP_TABLES.mod3[4],
	                       GROUP_TABLES.mod3[5]};
	return lut4(x, t);
}

// byte i of a packed array of dwords, i a compile-time constant
#define PDB_BYTE(w, i) (((w)[(i) >> 2] >> (8 * ((i) & 3))) & 0xFFu)

// The index of packed selected codes, all below 24.  false: two selected cubies of a kind share a position (the index means nothing).
__device__ __forceinline__ bool pdb_rank(const PdbDesc &p, const uint32_t c[2], const uint32_t e[3], uint32_t &index)
{
	const uint32_t pos4[2] = {pdb_div3(c[0]), pdb_div3(c[1])}, dig4[2] = {pdb_mod3(c[0]), pdb_mod3(c[1])};
	uint32_t r = 0, o = 0, seen = 0, twice = 0;
	#pragma unroll
	for (int i = 0; i < 8; i++)
		if ((uint32_t)i < p.kc) {
			const uint32_t pos = PDB_BYTE(pos4, i) & 7u, bit = 1u << pos;
			twice |= seen & bit;
			r = r * (uint32_t)(8 - i) + pos - (uint32_t)__popc(seen & (bit - 1u));
			seen |= bit;
			if ((uint32_t)i < p.oc_digits) o = o * 3u + (PDB_BYTE(dig4, i) & 3u);
		}
	uint32_t x = r * p.Oc + o;
	r = 0; o = 0; seen = 0;
	#pragma unroll
	for (int i = 0; i < PDB_EDGE_SLOTS; i++)
		if ((uint32_t)i < p.ke) {
			const uint32_t code = PDB_BYTE(e, i), pos = (code >> 1) & 15u, bit = 1u << pos;
			twice |= seen & bit;
			r = r * (uint32_t)(12 - i) + pos - (uint32_t)__popc(seen & (bit - 1u));
			seen |= bit;
			o = o * 2u + (code & 1u);
		}
	index = ((x * p.Pe + r) << p.ke) | o;
	return twice == 0u;
}

// The selected codes of a row, packed.  false: a selected code is 24 or more (or negative).
__device__ __forceinline__ bool pdb_gather(const PdbDesc &p, const uint32_t x[5], uint32_t c[2], uint32_t e[3])
{
	uint32_t high = 0;
	#pragma unroll
	for (int j = 0; j < 2; j++) {
		c[j] = bperm(x[1], x[0], p.sel_c[j]);
		high |= ((c[j] & 0x7F7F7F7Fu) + 0x68686868u) | c[j];
	}
	#pragma unroll
	for (int j = 0; j < 3; j++) {
		e[j] = bperm(x[3], x[2], p.sel_lo[j]) | bperm(0u, x[4], p.sel_hi[j]);
		high |= ((e[j] & 0x7F7F7F7Fu) + 0x68686868u) | e[j];
	}
	return (high & 0x80808080u) == 0u;
}

// The entry of state s in one table, -1 where its selected codes are no partial pattern.  The table is read only behind
// index < size.
__device__ __forceinline__ int pdb_entry(const PdbDesc &p, const uint32_t s[5])
{
	uint32_t c[2], e[3], index = 0;
	int v = -1;
	if (pdb_gather(p, s, c, e) && pdb_rank(p, c, e, index) && index < p.size) v = (int)p.table[index];
	return v;
}

// A lower bound on the quarter turns from s to solved: the greatest entry of s over the tables.  A table in which s has no
// entry, or an unreached one (255: never in a table that passed its build), counts 0, so such a state is never pruned.
__device__ __forceinline__ int pdb_bound(const PdbBound &B, const uint32_t s[5])
{
	int best = 0;
	#pragma unroll
	for (int k = 0; k < PDB_BOUND_MAX; k++)
		if (k < B.n) {
			const int v = pdb_entry(B.db[k], s);
			best = max(best, v == (int)PDB_UNREACHED ? 0 : v);
		}
	return best;
}

}  // namespace rk

// What rk_bound_create makes: the descriptors of its tables, copied.  The tables belong to their rk_pdb handles, which outlive it.
struct rk_bound {
	rk::PdbBound b{};
};
