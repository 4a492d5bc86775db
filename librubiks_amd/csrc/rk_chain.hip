// The subgroup chain (rk_chain_*): a solution for EVERY legal state by four table descents -- no search, no pool, no net.
//
// Thistlethwaite's four stages restated for the 12 quarter turns.  Stage k may use only the generators that keep what stages 1..k-1
// reached, a half turn XX (the action 2 f twice, cost 2) where the quarter turn would not; it brings the state into the next
// subgroup, and its table holds, for every coset of that subgroup, the cost of the cheapest word that does so.  DESIGN 3.59.8 and
// include/rubiks_hip.h define the signatures and THE INDEX of each table; chain_index below is that definition, one function for
// the host build and the kernel.  Signatures are taken BY POSITION (the digit of the cubie AT position p, the positions that hold
// a set of cubies, the corner sequence up to relabelling the cubies by the half-turn group): only then does a move's effect on the
// signature depend on the signature alone.
//
// Everything is read off the move table at compile time (ChainConsts): which faces flip an edge, which take a corner's digit off
// 0, the three slices (the edges neither face of an axis moves), the generators of every stage.  The corner sequences of the
// half-turn group (C3, 96 of them) and the coset map (40 320 entries, 420 cosets) come from a closure at create time.
//
// The build is on the host, build_cost_table of rk_table_host.h: level d + 1 takes the cost-1 children of level d and the cost-2
// children of level d - 1 and stores only over "unreached", so a table does not depend on the visiting order; one representative
// state per coset carries the search.  The tables and the two maps go to the device as one TableBlock.
// The coset counts 2 048 / 1 082 565 / 29 400 / 663 552 are conditions: any other count is RK_ESTATE.
//
// The query is ONE launch, a thread per state under a capped grid, the per-action tables staged in LDS once per workgroup, the
// state in five dwords.  Per step a thread applies each generator of the stage, forms the child's index, reads one byte and takes
// the LOWEST generator whose entry equals the current entry minus its cost.  The generator loop is a template recursion: every
// generator's action and cost are compile-time constants, every loop bound is wave-uniform, nothing is indexed dynamically in
// registers.  The legality test of rk_group_legal runs before any table access, every table and map read is guarded by its size,
// and every descent is bounded by the stage's deepest entry.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_chain_dev.h"
#include "rk_error.h"
#include "rk_group_dev.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"
#include "rk_table_host.h"

namespace rk {

struct ChainDev {
	const uint8_t *table[CHAIN_STAGES];
	uint32_t depth[CHAIN_STAGES];                   // the deepest entry of each table
	const uint16_t *coset;                          // [rank of the corner sequence] -> its coset under C3, 0..419
	const uint8_t *c3;                              // [rank] -> its ordinal in C3, 255 outside
};

// the entry of a state, CHAIN_UNREACHED where it has none
template <int STAGE>
__device__ __forceinline__ uint32_t chain_entry(const ChainDev &d, const uint32_t x[5])
{
	const uint32_t index = chain_index<STAGE>(x, d.coset, d.c3);
	return index < CHAIN_SIZE[STAGE] ? (uint32_t)d.table[STAGE][index] : CHAIN_UNREACHED;
}

constexpr uint32_t CHAIN_NO_PICK = 0xFFu;

// Generators G, G - 1, .., 0 in turn, each overwriting the pick: the lowest that fits stays.  pick = action | cost << 4.
template <int STAGE, int G>
__device__ __forceinline__ void chain_try(const ChainDev &d, const u32x4 *s_tab, const uint32_t x[5], uint32_t cur, uint32_t &pick)
{
	if constexpr (G >= 0) {
		constexpr uint32_t a = CHAIN_ACTION<STAGE, G>, cost = CHAIN_COST<STAGE, G>;
		uint32_t tab[12], s[5] = {x[0], x[1], x[2], x[3], x[4]};
		load_action_table(s_tab, a, tab);
		move5(s, tab);
		if (cost == 2u) move5(s, tab);
		if (chain_entry<STAGE>(d, s) + cost == cur) pick = a | cost << 4;
		chain_try<STAGE, G - 1>(d, s_tab, x, cur, pick);
	}
}

// One stage's descent of state x; the actions go to row[t...].  false: the state has no entry, or an entry has no generator that
// fits (never with tables that passed their build and a legal state).
template <int STAGE>
__device__ __forceinline__ bool chain_descend(const ChainDev &d, const u32x4 *s_tab, uint32_t x[5], int8_t *row, uint32_t &t, uint32_t &length)
{
	uint32_t cur = chain_entry<STAGE>(d, x);
	if (cur > d.depth[STAGE]) return false;
	length = cur;
	for (uint32_t step = 0; step < d.depth[STAGE] && cur != 0u; step++) {
		uint32_t pick = CHAIN_NO_PICK;
		chain_try<STAGE, CHAIN_GENS<STAGE> - 1>(d, s_tab, x, cur, pick);
		if (pick == CHAIN_NO_PICK) return false;
		const uint32_t a = pick & 15u, cost = pick >> 4;
		uint32_t tab[12];
		load_action_table(s_tab, a, tab);
		move5(x, tab);
		row[t++] = (int8_t)a;
		if (cost == 2u) {
			move5(x, tab);
			row[t++] = (int8_t)a;
		}
		cur -= cost;                                                     // cost <= cur: the pick's entry + cost == cur
	}
	return cur == 0u;
}

// lengths[q] = the moves written to row q of `actions` (`stride` = the four depths added up, which no row exceeds: a stage writes
// exactly its entry's cost); -1 and no action for a row that is no legal state.  error = min(error, q) over the rows that get -1.
__global__ __launch_bounds__(256)
void k_chain_solve(ChainDev d, const uint32_t *states, size_t n, uint32_t stride, int32_t *lengths, int8_t *actions, int32_t *stage_lengths,
                   uint32_t *error)
{
	__shared__ u32x4 s_tab[36];
	stage_action_tables(s_tab, (int)threadIdx.x);
	__syncthreads();
	for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
		uint32_t x[5], t = 0, l0 = 0, l1 = 0, l2 = 0, l3 = 0;
		load5(states + q * 5, x);
		int8_t *row = actions + q * (size_t)stride;
		const bool ok = group_legal(x) && chain_descend<0>(d, s_tab, x, row, t, l0) && chain_descend<1>(d, s_tab, x, row, t, l1) &&
		                chain_descend<2>(d, s_tab, x, row, t, l2) && chain_descend<3>(d, s_tab, x, row, t, l3);
		lengths[q] = ok ? (int32_t)t : -1;
		if (stage_lengths != nullptr) {
			int32_t *out = stage_lengths + q * 4;
			out[0] = ok ? (int32_t)l0 : -1;
			out[1] = ok ? (int32_t)l1 : -1;
			out[2] = ok ? (int32_t)l2 : -1;
			out[3] = ok ? (int32_t)l3 : -1;
		}
		if (!ok && error != nullptr) atomicMin(error, (uint32_t)q);
	}
}

}  // namespace rk

using namespace rk;

struct rk_chain {
	ChainDev d{};
	uint8_t *d_block = nullptr;                         // the four tables and the two maps, one allocation
	long long counts[CHAIN_STAGES] = {};
	~rk_chain()
	{
		if (d_block) (void)hipFree(d_block);
	}
};

namespace {

unsigned chain_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, (size_t)RK_CHAIN_GRID); }

// The two corner maps.  C3: the corner sequences that the half turns reach from solved, by a closure.  coset[r]: sequences P and
// P o h, h in C3 (the cubies relabelled), share a coset -- the side on which a move, which acts on the positions, maps cosets to
// cosets --; cosets are numbered by their least rank.  false: not 96 sequences or not 420 cosets.
bool chain_corner_maps(std::vector<uint16_t> &coset, std::vector<uint8_t> &c3)
{
	std::vector<uint8_t> in_c3(CHAIN_PERMS, 0);
	std::vector<HostState> todo{host_solved()};
	in_c3[chain_corner_rank(todo[0].data())] = 1;
	while (!todo.empty()) {
		const HostState s = todo.back();
		todo.pop_back();
		for (int g = 0; g < CHAIN.gen_count[3]; g++) {
			const HostState c = host_generate(s, CHAIN.gen_action[3][g], CHAIN.gen_cost[3][g]);
			const uint32_t r = chain_corner_rank(c.data());
			if (!in_c3[r]) {
				in_c3[r] = 1;
				todo.push_back(c);
			}
		}
	}
	// every sequence by rank, eight positions each
	std::vector<uint8_t> seq((size_t)CHAIN_PERMS * 8);
	uint8_t p[8] = {0, 1, 2, 3, 4, 5, 6, 7};
	for (uint32_t r = 0; r < CHAIN_PERMS; r++, std::next_permutation(p, p + 8)) memcpy(&seq[(size_t)r * 8], p, 8);
	const auto rank_of = [](const uint8_t *q) {
		uint32_t x[5] = {0, 0, 0, 0, 0};
		for (int c = 0; c < 8; c++) x[c >> 2] |= (uint32_t)(3 * q[c]) << (8 * (c & 3));
		return chain_corner_rank(x);
	};
	c3.assign(CHAIN_PERMS, 255);
	std::vector<uint32_t> members;
	for (uint32_t r = 0; r < CHAIN_PERMS; r++)
		if (in_c3[r]) {
			if (rank_of(&seq[(size_t)r * 8]) != r) return false;
			c3[r] = (uint8_t)std::min<size_t>(members.size(), 254);
			members.push_back(r);
		}
	if (members.size() != CHAIN_C3) return false;
	coset.assign(CHAIN_PERMS, 0xFFFF);
	uint32_t cosets = 0;
	for (uint32_t r = 0; r < CHAIN_PERMS; r++) {
		if (coset[r] != 0xFFFF) continue;
		if (cosets == CHAIN_COSETS) return false;
		for (uint32_t h : members) {
			uint8_t q[8];
			for (int c = 0; c < 8; c++) q[c] = seq[(size_t)r * 8 + seq[(size_t)h * 8 + c]];
			const uint32_t other = rank_of(q);
			if (coset[other] != 0xFFFF && coset[other] != cosets) return false;
			coset[other] = (uint16_t)cosets;
		}
		cosets++;
	}
	return cosets == CHAIN_COSETS;
}

// One table: build_cost_table (rk_table_host.h) over the stage's generators, one representative state per coset.  Returns the
// deepest entry, -1 unless exactly CHAIN_COUNT[STAGE] entries were reached and one of them is 0.  The index is forced inline: the
// builder calls it at two places, and left as a call the later stages' builds take a third longer.
template <int STAGE>
int chain_build(std::vector<uint8_t> &table, const uint16_t *coset, const uint8_t *c3, long long &count)
{
	return build_cost_table(
		table, CHAIN_SIZE[STAGE], (long long)CHAIN_COUNT[STAGE], CHAIN.gen_count[STAGE], CHAIN.gen_cost[STAGE], host_solved(),
		[](const HostState &s, int g) { return host_generate(s, CHAIN.gen_action[STAGE][g], CHAIN.gen_cost[STAGE][g]); },
		[=](const HostState &s) __attribute__((always_inline)) { return chain_index<STAGE>(s.data(), coset, c3); }, count);
}

}  // namespace

extern "C" {

int rk_chain_create(rk_chain_t **out, void *stream)
{
	if (!out) return fail(RK_EINVAL, "rk_chain_create: null out pointer");
	std::vector<uint16_t> coset;
	std::vector<uint8_t> c3, table[CHAIN_STAGES];
	if (!chain_corner_maps(coset, c3))
		return fail(RK_ESTATE, "rk_chain_create: the half turns do not give %u corner sequences in %u cosets", CHAIN_C3, CHAIN_COSETS);
	rk_chain *h = new rk_chain();
	int depth[CHAIN_STAGES];
	depth[0] = chain_build<0>(table[0], coset.data(), c3.data(), h->counts[0]);
	depth[1] = chain_build<1>(table[1], coset.data(), c3.data(), h->counts[1]);
	depth[2] = chain_build<2>(table[2], coset.data(), c3.data(), h->counts[2]);
	depth[3] = chain_build<3>(table[3], coset.data(), c3.data(), h->counts[3]);
	for (int s = 0; s < CHAIN_STAGES; s++)
		if (depth[s] < 0) {
			const long long got = h->counts[s];
			delete h;
			return fail(RK_ESTATE, "rk_chain_create: the table of stage %d reached %lld cosets, not %u with one goal", s + 1, got, CHAIN_COUNT[s]);
		}
	TableBlock block;                                                   // the tables, then the maps
	for (int s = 0; s < CHAIN_STAGES; s++) block.add(table[s].data(), CHAIN_SIZE[s]);
	block.add(coset.data(), (size_t)CHAIN_PERMS * sizeof(uint16_t));
	block.add(c3.data(), CHAIN_PERMS);
	if (int e = block.upload("rk_chain_create", (hipStream_t)stream)) {
		delete h;
		return e;
	}
	for (int s = 0; s < CHAIN_STAGES; s++) {
		h->d.table[s] = block.at(s);
		h->d.depth[s] = (uint32_t)depth[s];
	}
	h->d.coset = block.at<uint16_t>(CHAIN_STAGES);
	h->d.c3 = block.at(CHAIN_STAGES + 1);
	h->d_block = block.release();
	*out = h;
	return RK_OK;
}

int rk_chain_destroy(rk_chain_t *h)
{
	delete h;
	return RK_OK;
}

int rk_chain_status(rk_chain_t *h, long long *h_status)
{
	if (!h || !h_status) return fail(RK_EINVAL, "rk_chain_status: null argument");
	memset(h_status, 0, 16 * sizeof(long long));
	for (int s = 0; s < CHAIN_STAGES; s++) {
		h_status[s] = h->counts[s];
		h_status[4 + s] = (long long)h->d.depth[s];
		h_status[8] += (long long)h->d.depth[s];
		h_status[9 + s] = (long long)CHAIN_SIZE[s];
	}
	return RK_OK;
}

int rk_chain_export(rk_chain_t *h, int stage, size_t first, size_t count, uint8_t *h_bytes, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_chain_export: null handle");
	return export_table("rk_chain_export", "stage", stage, CHAIN_STAGES, h->d.table, CHAIN_SIZE, first, count, h_bytes, stream);
}

int rk_chain_solve(rk_chain_t *h, const int8_t *d_states, size_t n, int32_t *d_lengths, int8_t *d_actions, int32_t *d_stage_lengths,
                   int32_t *d_error, void *stream)
{
	if (!h) return fail(RK_EINVAL, "rk_chain_solve: null handle");
	if (int e = check_state_rows("rk_chain_solve", d_states, n)) return e;
	if (n != 0 && (!d_lengths || !d_actions)) return fail(RK_EINVAL, "rk_chain_solve: null pointer");
	if (((uintptr_t)d_lengths | (uintptr_t)d_stage_lengths | (uintptr_t)d_error) & 3u)
		return fail(RK_EINVAL, "rk_chain_solve: device pointers must be 4-byte aligned");
	if (n == 0) return RK_OK;
	hipStream_t st = (hipStream_t)stream;
	if (d_error) RK_HIP(hipMemsetAsync(d_error, 0xFF, sizeof(int32_t), st));         // -1: no row so far
	const uint32_t stride = h->d.depth[0] + h->d.depth[1] + h->d.depth[2] + h->d.depth[3];
	hipLaunchKernelGGL(k_chain_solve, dim3(chain_grid(n)), dim3(256), 0, st, h->d, reinterpret_cast<const uint32_t *>(d_states), n, stride,
	                   d_lengths, d_actions, d_stage_lengths, reinterpret_cast<uint32_t *>(d_error));
	RK_HIP(hipGetLastError());
	return RK_OK;
}

}  // extern "C"
