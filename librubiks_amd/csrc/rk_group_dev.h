// Device-side pieces of the cube group that more than one engine uses: code / 3 and code % 3 of four codes at once, and the legality
// of a row (rk_group.hip reports it, rk_chain.hip refuses such rows before it reads a table).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rk_device.h"
#include "rk_group_tables.h"

namespace rk {

__device__ __forceinline__ uint32_t group_div3(uint32_t x)
{
	const uint32_t t[6] = {GROUP_TABLES.div3[0], GROUP_TABLES.div3[1], GROUP_TABLES.div3[2], GROUP_TABLES.div3[3], GROUP_TABLES.div3[4],
	                       GROUP_TABLES.div3[5]};
	return lut4(x, t);
}

__device__ __forceinline__ uint32_t group_mod3(uint32_t x)
{
	const uint32_t t[6] = {GROUP_TABLES.mod3[0], GROUP_TABLES.mod3[1], GROUP_TABLES.mod3[2], GROUP_TABLES.mod3[3], GROUP_TABLES.mod3[4],
	                       GROUP_TABLES.mod3[5]};
	return lut4(x, t);
}

// A row is legal when it is reachable from solved: every code below 24, the corner positions a permutation of 0..7 and the edge
// positions one of 0..11, the two permutations of equal parity, the edge flips even in number and the corner twists 0 mod 3.
__device__ __forceinline__ bool group_legal(const uint32_t x[5])
{
	uint32_t high = 0;                                                                       // bit 7 of a byte: the code is 24 or more
	#pragma unroll
	for (int j = 0; j < 5; j++) high |= ((x[j] & 0x7F7F7F7Fu) + 0x68686868u) | x[j];
	bool ok = (high & 0x80808080u) == 0u;
	// positions seen so far, and the inversions of both permutations together: an element counts the greater positions before it
	uint32_t seen = 0, inversions = 0, twist = 0;
	#pragma unroll
	for (int j = 0; j < 2; j++) {
		const uint32_t pos4 = group_div3(x[j]);
		#pragma unroll
		for (int i = 0; i < 4; i++) {
			const uint32_t pos = (pos4 >> (8 * i)) & 7u;
			inversions += (uint32_t)__popc(seen & (0xFFFFFFFEu << pos));
			seen |= 1u << pos;
			twist += (uint32_t)(GROUP_TAU_BITS >> (2u * ((x[j] >> (8 * i)) & 31u))) & 3u;
		}
	}
	ok = ok && seen == 0xFFu;
	seen = 0;
	#pragma unroll
	for (int j = 2; j < 5; j++) {
		#pragma unroll
		for (int i = 0; i < 4; i++) {
			const uint32_t pos = (x[j] >> (8 * i + 1)) & 15u;
			inversions += (uint32_t)__popc(seen & (0xFFFFFFFEu << pos));
			seen |= 1u << pos;
		}
	}
	ok = ok && seen == 0xFFFu;
	uint32_t flips = x[2] ^ x[3] ^ x[4];
	flips ^= flips >> 16;
	flips ^= flips >> 8;
	return ok && ((inversions | flips) & 1u) == 0u && twist % 3u == 0u;
}

}  // namespace rk
