// What the subgroup chain (rk_chain.hip) and the two-phase search (rk_twophase.hip) share: the constants read off the move table at
// compile time (ChainConsts: which faces flip an edge, which take a corner's digit off 0, the three slices, the generators of every
// stage) and the signatures BY POSITION with THE INDEX of each chain table (chain_index), one function for the host builds and
// the kernels.  include/rubiks_hip.h and DESIGN 3.59.8 define them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rk_device.h"

namespace rk {

constexpr int CHAIN_STAGES = 4;
constexpr uint32_t CHAIN_UNREACHED = 255;
constexpr uint32_t CHAIN_PERMS = 40320;             // 8!
constexpr uint32_t CHAIN_C3 = 96, CHAIN_COSETS = 420;
constexpr uint32_t CHAIN_SIZE[CHAIN_STAGES] = {2048u, 2187u * 495u, CHAIN_COSETS * 70u, CHAIN_C3 * 13824u};
constexpr uint32_t CHAIN_COUNT[CHAIN_STAGES] = {2048u, 1082565u, 29400u, 663552u};      // the cosets each build must reach

struct ChainConsts {
	bool flips[6], twists[6];                       // the face changes an edge's digit / takes a corner's digit off 0
	uint8_t slice[3][4];                            // the edges neither face of an axis moves, ascending: 0 the axis that keeps both digits,
	uint16_t slice_mask[3];                         // 1 the axis that flips edges, 2 the third
	uint8_t outside0[8];                            // the positions outside slice 0, ascending
	uint8_t gen_action[CHAIN_STAGES][12], gen_cost[CHAIN_STAGES][12];
	int gen_count[CHAIN_STAGES];
	bool consistent;
};

constexpr ChainConsts make_chain_consts()
{
	const Tables t = make_tables();
	ChainConsts c{};
	c.consistent = true;
	uint16_t moved[6] = {};
	for (int f = 0; f < 6; f++) {
		for (int v = 0; v < 24; v++)
			if ((t.lut[2 * f][1][v] & 1) != (v & 1)) c.flips[f] = true;
		for (int q = 0; q < 8; q++)
			if (t.lut[2 * f][0][3 * q] % 3 != 0) c.twists[f] = true;
		for (int e = 0; e < 12; e++)
			if (t.lut[2 * f][1][2 * e] != 2 * e) moved[f] |= (uint16_t)(1u << e);
	}
	int found[3] = {0, 0, 0};
	for (int f = 0; f < 6; f++)
		for (int g = f + 1; g < 6; g++) {
			if (moved[f] & moved[g]) continue;
			if (c.flips[f] != c.flips[g] || c.twists[f] != c.twists[g]) c.consistent = false;
			const int s = c.flips[f] ? 1 : c.twists[f] ? 2 : 0;
			found[s]++;
			c.slice_mask[s] = (uint16_t)(0xFFFu & ~(moved[f] | moved[g]));
		}
	for (int s = 0; s < 3; s++) {
		int k = 0;
		for (int e = 0; e < 12; e++)
			if (c.slice_mask[s] >> e & 1) {
				if (k < 4) c.slice[s][k] = (uint8_t)e;
				k++;
			}
		if (found[s] != 1 || k != 4) c.consistent = false;
	}
	if ((c.slice_mask[0] | c.slice_mask[1] | c.slice_mask[2]) != 0xFFFu) c.consistent = false;
	for (int p = 0, k = 0; p < 12; p++)
		if (!(c.slice_mask[0] >> p & 1) && k < 8) c.outside0[k++] = (uint8_t)p;
	for (int stage = 0; stage < CHAIN_STAGES; stage++) {
		int n = 0;
		for (int f = 0; f < 6; f++) {
			const bool quarter = stage == 0 || (stage == 1 && !c.flips[f]) || (stage == 2 && !c.flips[f] && !c.twists[f]);
			c.gen_action[stage][n] = (uint8_t)(2 * f);
			c.gen_cost[stage][n++] = quarter ? 1 : 2;
			if (quarter) {
				c.gen_action[stage][n] = (uint8_t)(2 * f + 1);
				c.gen_cost[stage][n++] = 1;
			}
		}
		c.gen_count[stage] = n;
	}
	return c;
}

constexpr ChainConsts CHAIN = make_chain_consts();
static_assert(CHAIN.consistent, "the move table does not give three axes with a slice of four edges each");

template <int S> constexpr uint32_t CHAIN_SLICE = CHAIN.slice[S][0] | CHAIN.slice[S][1] << 4 | CHAIN.slice[S][2] << 8 | CHAIN.slice[S][3] << 12;
template <int S> constexpr uint32_t CHAIN_SLICE_MASK = CHAIN.slice_mask[S];
constexpr uint32_t chain_outside0()
{
	uint32_t v = 0;
	for (int i = 0; i < 8; i++) v |= (uint32_t)CHAIN.outside0[i] << (4 * i);
	return v;
}
constexpr uint32_t CHAIN_OUTSIDE0 = chain_outside0();
template <int STAGE> constexpr int CHAIN_GENS = CHAIN.gen_count[STAGE];
template <int STAGE, int G> constexpr uint32_t CHAIN_ACTION = CHAIN.gen_action[STAGE][G];
template <int STAGE, int G> constexpr uint32_t CHAIN_COST = CHAIN.gen_cost[STAGE][G];

// byte i of a state in five dwords, i a constant once the loops are unrolled
#define CHAIN_BYTE(x, i) (((x)[(i) >> 2] >> (8 * ((i) & 3))) & 0xFFu)

__host__ __device__ __forceinline__ uint32_t chain_popc(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return (uint32_t)__popc(v);
#else
	return (uint32_t)__builtin_popcount(v);
#endif
}

// the ordinal of a set of four among the 4-subsets of 0..11, ordered by the largest element, then the next: sum of C(p_i, i + 1)
// over its elements ascending.  A set of fewer elements gives a number that means nothing; the caller guards the table read.
__host__ __device__ __forceinline__ uint32_t chain_subset(uint32_t set)
{
	uint32_t p[4];
	#pragma unroll
	for (int i = 0; i < 4; i++) {
		p[i] = set != 0u ? (uint32_t)__builtin_ctz(set) : 0u;
		set &= set - 1u;
	}
	return p[0] + p[1] * (p[1] - 1u) / 2u + p[2] * (p[2] - 1u) * (p[2] - 2u) / 6u + p[3] * (p[3] - 1u) * (p[3] - 2u) * (p[3] - 3u) / 24u;
}

// the positions that hold the four edges of slice S, as a bit set
template <int S>
__host__ __device__ __forceinline__ uint32_t chain_slice_at(const uint32_t x[5])
{
	uint32_t set = 0;
	#pragma unroll
	for (int i = 0; i < 4; i++) set |= 1u << ((CHAIN_BYTE(x, 8 + ((CHAIN_SLICE<S> >> (4 * i)) & 15u)) >> 1) & 15u);
	return set;
}

// the ordinal, among the 24 sequences in lexicographic order, of the places the edges of slice S take within the slice
template <int S>
__host__ __device__ __forceinline__ uint32_t chain_places(const uint32_t x[5])
{
	uint32_t q = 0, seen = 0;
	#pragma unroll
	for (int i = 0; i < 4; i++) {
		const uint32_t pos = (CHAIN_BYTE(x, 8 + ((CHAIN_SLICE<S> >> (4 * i)) & 15u)) >> 1) & 15u;
		const uint32_t place = chain_popc(CHAIN_SLICE_MASK<S> & ((1u << pos) - 1u)) & 3u;
		q = q * (uint32_t)(4 - i) + place - chain_popc(seen & ((1u << place) - 1u));
		seen |= 1u << place;
	}
	return q;
}

// the lexicographic rank of the corner sequence P = (position of cubie 0, .., of cubie 7); code / 3 = code * 11 >> 5 below 24
__host__ __device__ __forceinline__ uint32_t chain_corner_rank(const uint32_t x[5])
{
	uint32_t r = 0, seen = 0;
	#pragma unroll
	for (int c = 0; c < 8; c++) {
		const uint32_t pos = ((CHAIN_BYTE(x, c) * 11u) >> 5) & 7u, bit = 1u << pos;
		r = r * (uint32_t)(8 - c) + pos - chain_popc(seen & (bit - 1u));
		seen |= bit;
	}
	return r;
}

// THE INDEX of a state in the table of STAGE (include/rubiks_hip.h).  A value at or above the table's size: the state has none.
template <int STAGE>
__host__ __device__ __forceinline__ uint32_t chain_index(const uint32_t x[5], const uint16_t *coset, const uint8_t *c3)
{
	if (STAGE == 0) {
		uint32_t bits = 0;
		#pragma unroll
		for (int e = 0; e < 12; e++) {
			const uint32_t code = CHAIN_BYTE(x, 8 + e);
			bits |= (code & 1u) << ((code >> 1) & 15u);
		}
		return bits & 2047u;
	}
	if (STAGE == 1) {
		uint32_t digits = 0, ori = 0;
		#pragma unroll
		for (int c = 0; c < 8; c++) {
			const uint32_t code = CHAIN_BYTE(x, c), pos = ((code * 11u) >> 5) & 7u;
			digits |= ((code - 3u * pos) & 3u) << (2u * pos);
		}
		#pragma unroll
		for (int p = 6; p >= 0; p--) ori = ori * 3u + ((digits >> (2 * p)) & 3u);
		return ori * 495u + chain_subset(chain_slice_at<0>(x));
	}
	const uint32_t rank = chain_corner_rank(x);
	if (rank >= CHAIN_PERMS) return 0xFFFFFFFFu;
	if (STAGE == 2) {
		const uint32_t at = chain_slice_at<1>(x);
		uint32_t narrow = 0;
		#pragma unroll
		for (int i = 0; i < 8; i++) narrow |= ((at >> ((CHAIN_OUTSIDE0 >> (4 * i)) & 15u)) & 1u) << i;
		return (uint32_t)coset[rank] * 70u + chain_subset(narrow);
	}
	const uint32_t g = c3[rank];
	if (g >= CHAIN_C3) return 0xFFFFFFFFu;
	return ((g * 24u + chain_places<0>(x)) * 24u + chain_places<1>(x)) * 24u + chain_places<2>(x);
}

}  // namespace rk
