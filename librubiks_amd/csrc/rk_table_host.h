// Host-side pieces shared by the table solvers (the subgroup chain rk_chain.hip, the two-phase search rk_twophase.hip and, for the
// export alone, the pattern database rk_pdb.hip): 20-byte states moved on the host, the level-by-level build of a table of exact
// costs over generators of cost 1 or 2, the one device block a solver keeps its tables in, and the export of a table's entries.
// A table-backed engine still writes itself what makes it one: its index, its generators and its kernel.  Header-only, host code
// only, nothing in here is exported; DESIGN 3.59.10.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <array>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_chain_dev.h"
#include "rk_error.h"
#include "rk_kernels.h"

namespace rk {
namespace {

// ---- a 20-byte state in five dwords, moved through host_tables() ----
typedef std::array<uint32_t, 5> HostState;

// host_tables() lives in another translation unit: asked once, not once per move (the builds make some 40 M moves)
inline const Tables &host_lut()
{
	static const Tables &t = host_tables();
	return t;
}

inline HostState host_solved()
{
	HostState s;
	memcpy(s.data(), host_lut().solved, STATE_BYTES);
	return s;
}

inline HostState host_move(const HostState &s, int action)
{
	const Tables &t = host_lut();
	uint8_t b[STATE_BYTES];
	memcpy(b, s.data(), STATE_BYTES);
	for (int i = 0; i < 8; i++) b[i] = t.lut[action][0][b[i]];
	for (int i = 8; i < STATE_BYTES; i++) b[i] = t.lut[action][1][b[i]];
	HostState out;
	memcpy(out.data(), b, STATE_BYTES);
	return out;
}

// a generator: the action once, twice (the half turn) where its cost is 2
inline HostState host_generate(const HostState &s, int action, int cost)
{
	const HostState once = host_move(s, action);
	return cost == 2 ? host_move(once, action) : once;
}

// One table of exact costs, one byte per index, over `gens` generators of cost[g] = 1 or 2 from `root` (entry 0): level d + 1 takes
// the cost-1 children of level d and the cost-2 children of level d - 1 and stores only over CHAIN_UNREACHED, so the table does not
// depend on the visiting order; one node per entry carries the search.  child(node, g) is the node behind generator g, index(node)
// its entry.  Returns the deepest entry; -1 for an index at or past `size`, a depth that would reach CHAIN_UNREACHED, or unless
// exactly `expected` entries were reached and one of them is 0.  `count` = the entries reached, in either case.
template <typename Node, typename Child, typename Index>
int build_cost_table(std::vector<uint8_t> &table, size_t size, long long expected, int gens, const uint8_t *cost, const Node &root, Child child,
                     Index index, long long &count)
{
	table.assign(size, (uint8_t)CHAIN_UNREACHED);
	count = 0;
	std::vector<Node> before, level{root}, next;                           // levels d - 1, d, d + 1
	const size_t goal = index(root);
	if (goal >= size) return -1;
	table[goal] = 0;
	count = 1;
	int d = 0;
	for (; !level.empty() || !before.empty(); d++) {
		if (d + 1 >= (int)CHAIN_UNREACHED) return -1;
		next.clear();
		for (int g = 0; g < gens; g++)
			for (const Node &s : cost[g] == 1 ? level : before) {
				const Node c = child(s, g);
				const size_t to = index(c);
				if (to >= size) return -1;
				if (table[to] != CHAIN_UNREACHED) continue;
				table[to] = (uint8_t)(d + 1);
				next.push_back(c);
			}
		count += (long long)next.size();
		before.swap(level);
		level.swap(next);
	}
	long long zeros = 0;
	for (uint8_t v : table) zeros += v == 0;
	if (count != expected || zeros != 1) return -1;
	return d - 2;                                                        // the last two levels were empty
}

// The tables of a solver as ONE device allocation: add() the host spans (a null pointer: a span of zeros), each laid out 16-byte
// aligned, then upload() allocates, copies and clears on `st` and synchronises (the host copies go out of scope); at(i) is span
// i's device address.  The block belongs to this object until release() hands it to the solver's handle.
class TableBlock {
public:
	TableBlock() = default;
	TableBlock(const TableBlock &) = delete;
	TableBlock &operator=(const TableBlock &) = delete;
	~TableBlock() { if (d_block_) (void)hipFree(d_block_); }

	void add(const void *host, size_t bytes)
	{
		spans_.push_back({host, bytes_, bytes});
		bytes_ += (bytes + 15) / 16 * 16;
	}
	void add_zeros(size_t bytes) { add(nullptr, bytes); }

	int upload(const char *who, hipStream_t st)
	{
		if (hipMalloc((void **)&d_block_, bytes_) != hipSuccess) {
			(void)hipGetLastError();
			d_block_ = nullptr;
			return fail(RK_ECAPACITY, "%s: no device memory for %zu bytes of tables", who, bytes_);
		}
		for (const Span &s : spans_) {
			if (s.host) RK_HIP(hipMemcpyAsync(d_block_ + s.at, s.host, s.bytes, hipMemcpyHostToDevice, st));
			else RK_HIP(hipMemsetAsync(d_block_ + s.at, 0, s.bytes, st));
		}
		RK_HIP(hipStreamSynchronize(st));
		return RK_OK;
	}
	template <typename T = uint8_t>
	T *at(size_t span) const { return reinterpret_cast<T *>(d_block_ + spans_[span].at); }
	uint8_t *release()
	{
		uint8_t *p = d_block_;
		d_block_ = nullptr;
		return p;
	}

private:
	struct Span { const void *host; size_t at, bytes; };
	std::vector<Span> spans_;
	size_t bytes_ = 0;
	uint8_t *d_block_ = nullptr;
};

// entries first .. first + count of table `which` (1..tables, `what` names it) of the engine's d_tables, of sizes[] entries, to the
// host; the caller has checked its handle.  The arrays are read only once `which` has passed.
inline int export_table(const char *who, const char *what, int which, int tables, const uint8_t *const *d_tables, const uint32_t *sizes, size_t first,
                        size_t count, uint8_t *h_bytes, void *stream)
{
	if (which < 1 || which > tables) return fail(RK_EINVAL, "%s: %s %d outside 1..%d", who, what, which, tables);
	const size_t size = sizes[which - 1];
	if (first > size || count > size - first) return fail(RK_EINVAL, "%s: entries %zu..%zu outside the table", who, first, first + count);
	if (count == 0) return RK_OK;
	if (!h_bytes) return fail(RK_EINVAL, "%s: null pointer", who);
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemcpyAsync(h_bytes, d_tables[which - 1] + first, count, hipMemcpyDeviceToHost, st));
	RK_HIP(hipStreamSynchronize(st));
	return RK_OK;
}

}  // namespace
}  // namespace rk
