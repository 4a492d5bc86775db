// Host-side pieces shared by the search engines (A* single / sharded / batched, MCTS, the breadth-first and ball searches, and the
// net-stepped ones: epsilon-greedy value search, the greedy games, beam search): who owns a device allocation, growing arrays in place
// as one transaction and the small read-backs every engine needs; at the end, what only the net-stepped engines share: the net batches
// an engine owns per RK_OH_* form, and the checks of the start states and of the net output that their entry points take.
// The counterpart of rk_search_dev.h; header-only, nothing in here is exported.  The host half of the breadth-first engines' pool
// and of the kept balls is rk_frontier_host.h, which only those engines include: it brings the frontier pool's kernels with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_search_dev.h"

namespace rk {
namespace {

class Growth;

inline unsigned blocks(size_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

// slots of an open-addressing table for `capacity` states (+ the unused index 0): a power of two, at most half full
inline uint64_t table_slots(size_t capacity, uint64_t floor)
{
	uint64_t t = floor;
	while (t < 2 * (uint64_t)capacity + 2) t <<= 1;
	return t;
}

// look-back words of frontier_scan (rk_search_dev.h) over the 12 x pops children of a breadth-first batch, 256 per workgroup
inline size_t frontier_scan_blocks(int pops) { return (size_t)blocks((size_t)12 * pops, 256) + 1; }

// a caller's max_states as the int32 the device counters hold
inline int budget_of(long long max_states) { return (int)std::min<long long>(std::max<long long>(max_states, 0), INT32_MAX); }

// Owns device allocations: whatever alloc() handed out is freed by release(), or with the owner.  `slack` bytes are added to
// every allocation (kernels may read a little past the last element with wide loads).
class DevPool {
public:
	explicit DevPool(size_t slack) : slack_(slack) {}
	DevPool(const DevPool &) = delete;
	DevPool &operator=(const DevPool &) = delete;
	~DevPool() { clear(); }

	template <typename T>
	int alloc(T **field, size_t count)
	{
		void *q = nullptr;
		RK_HIP(hipMalloc(&q, count * sizeof(T) + slack_));
		owned_.push_back(q);
		*field = static_cast<T *>(q);
		return RK_OK;
	}
	void release(void *p)
	{
		const auto it = std::find(owned_.begin(), owned_.end(), p);
		if (it == owned_.end()) return;
		owned_.erase(it);
		(void)hipFree(p);
	}
	void clear()
	{
		for (void *p : owned_) (void)hipFree(p);
		owned_.clear();
	}

private:
	friend class Growth;
	size_t slack_;
	std::vector<void *> owned_;
};

// inside the fill step of a Growth: hand the first HIP error to the transaction
#define RK_FILL(call) do { const hipError_t rk_fill_e_ = (call); if (rk_fill_e_ != hipSuccess) return rk_fill_e_; } while (0)

// Growing arrays in place, all or nothing.  Work on a COPY of the engine's descriptor:
//   request()  a new array for a field of the copy; the array the field held (if any) is replaced at commit
//   granted()  false if a request failed: what was taken is given back, the caller reports RK_ECAPACITY
//   fill()     the engine's copies / rehash on `st` (RK_FILL around every call), then one synchronisation; on an error the stream
//              is synchronised -- nothing may still write into what is freed next --, what was taken is given back and RK_EHIP is
//              reported as "<who>: <hip error>"
//   commit()   frees the replaced arrays and adopts the new ones; the caller then stores the copy
// Until commit() the engine is untouched; a transaction that is dropped gives back what it took.
class Growth {
public:
	Growth(DevPool &pool, const char *who) : pool_(pool), who_(who) {}
	~Growth() { give_back(); }

	template <typename T>
	void request(T **field, size_t count)
	{
		void *q = nullptr;
		if (ok_ && hipMalloc(&q, count * sizeof(T) + pool_.slack_) == hipSuccess) fresh_.push_back(q);
		else { ok_ = false; q = nullptr; }
		if (*field != nullptr) stale_.push_back(*field);
		*field = static_cast<T *>(q);
	}
	bool granted()
	{
		if (!ok_) { give_back(); (void)hipGetLastError(); }
		return ok_;
	}
	template <typename Steps>
	int fill(hipStream_t st, Steps &&steps)
	{
		hipError_t e = steps();
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e == hipSuccess) return RK_OK;
		(void)hipStreamSynchronize(st);
		give_back();
		(void)hipGetLastError();
		return fail(RK_EHIP, "%s: %s", who_, hipGetErrorString(e));
	}
	void commit()
	{
		for (void *q : stale_) pool_.release(q);
		pool_.owned_.insert(pool_.owned_.end(), fresh_.begin(), fresh_.end());
		fresh_.clear();
		stale_.clear();
	}

private:
	void give_back()
	{
		for (void *q : fresh_) (void)hipFree(q);
		fresh_.clear();
	}
	DevPool &pool_;
	const char *who_;
	std::vector<void *> fresh_, stale_;
	bool ok_ = true;
};

// Page-locked landing place of a small block of device counters: a poll is one direct copy, no staging (pageable memory costs a
// staged copy per poll).  Without page-locked memory the caller's own buffer is the landing place.
class Landing {
public:
	Landing() = default;
	Landing(const Landing &) = delete;
	Landing &operator=(const Landing &) = delete;
	~Landing() { if (pinned_ != nullptr) (void)hipHostFree(pinned_); }

	void reserve(size_t count)
	{
		if (hipHostMalloc((void **)&pinned_, count * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); pinned_ = nullptr; }
	}
	// `count` ints from `dev`, synchronising `st`; *at is where they landed (`spare`, of `count` ints, unless there is a page-locked buffer)
	int fetch(const int32_t *dev, size_t count, int32_t *spare, hipStream_t st, const int32_t **at)
	{
		int32_t *dst = pinned_ != nullptr ? pinned_ : spare;
		RK_HIP(hipMemcpyAsync(dst, dev, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
		RK_HIP(hipStreamSynchronize(st));
		*at = dst;
		return RK_OK;
	}
	// the same, into `out`
	int read(const int32_t *dev, size_t count, int32_t *out, hipStream_t st)
	{
		const int32_t *at = nullptr;
		if (int e = fetch(dev, count, out, st, &at)) return e;
		if (at != out) memcpy(out, at, count * sizeof(int32_t));
		return RK_OK;
	}
	bool pinned() const { return pinned_ != nullptr; }

private:
	int32_t *pinned_ = nullptr;
};

// A narrow device column (int32 / uint8) for a host that wants long long / double: start() enqueues the copy into a temporary (a
// null `out` asks for nothing), finish() widens it once the stream has been synchronised.
template <typename Narrow, typename Wide>
class Widened {
public:
	int start(const Narrow *dev, size_t count, Wide *out, hipStream_t st)
	{
		out_ = out;
		if (out == nullptr || count == 0) return RK_OK;
		tmp_.resize(count);
		RK_HIP(hipMemcpyAsync(tmp_.data(), dev, count * sizeof(Narrow), hipMemcpyDeviceToHost, st));
		return RK_OK;
	}
	void finish()
	{
		for (size_t i = 0; i < tmp_.size(); i++) out_[i] = (Wide)tmp_[i];
	}

private:
	std::vector<Narrow> tmp_;
	Wide *out_ = nullptr;
};

// one column on its own: copy, synchronise, widen
template <typename Narrow, typename Wide>
int export_widened(const Narrow *dev, size_t count, Wide *out, hipStream_t st)
{
	Widened<Narrow, Wide> w;
	if (int e = w.start(dev, count, out, st)) return e;
	if (out != nullptr && count != 0) RK_HIP(hipStreamSynchronize(st));
	w.finish();
	return RK_OK;
}

// What a walk kernel left in `walk`: [0] = length of the action queue or -1, then the actions root -> node.  *len is that first
// word; of a queue that exists, the first min(length, max_len, walk_max) actions go to h_actions.
inline int read_walk(const int32_t *walk, size_t walk_max, long long *h_actions, size_t max_len, hipStream_t st, int32_t *len)
{
	*len = 0;
	RK_HIP(hipMemcpyAsync(len, walk, sizeof *len, hipMemcpyDeviceToHost, st));
	RK_HIP(hipStreamSynchronize(st));
	if (*len < 0) return RK_OK;
	return export_widened(walk + 1, std::min(std::min((size_t)*len, max_len), walk_max), h_actions, st);
}

// n rows of 20-byte device states, read as dwords, as every batched entry takes them: the caller checks its handle first, then
// this, then its own arguments
inline int check_state_rows(const char *who, const void *d_rows, size_t n)
{
	if (n > (size_t)INT32_MAX) return fail(RK_EINVAL, "%s: %zu states in one launch", who, n);
	if (n != 0 && !d_rows) return fail(RK_EINVAL, "%s: null pointer", who);
	if ((uintptr_t)d_rows & 3u) return fail(RK_EINVAL, "%s: device pointers must be 4-byte aligned", who);
	return RK_OK;
}

// ---- what the net-stepped engines share (rk_egvm.hip, rk_greedy.hip, rk_beam.hip): they own the net's batch, per RK_OH_* form ----
// bytes of a batch row: the 20-byte state, or 480 one-hot elements of 4 or 2 bytes (write_row, rk_search_dev.h)
inline size_t net_row_bytes(int code) { return code == RK_OH_STATES ? 20 : code == RK_OH_F32 ? 1920 : 960; }

// The net batches of one engine input, per form (the entry point checks the code): taken from the engine's pool when a form is
// first asked for, alive as long as the pool.  `zeroed`: a fresh buffer is cleared (blocking), for an engine whose forwards read
// rows that nothing has written (code 0 is a valid cubie code, an all-zero one-hot row a harmless input).
struct NetBatches {
	bool zeroed;
	void *at[RK_OH_STATES + 1] = {};

	int get(DevPool &pool, int code, size_t rows, void **out)
	{
		if (at[code] == nullptr) {
			const size_t bytes = rows * net_row_bytes(code);
			uint8_t *p = nullptr;
			if (int e = pool.alloc(&p, bytes)) return e;
			if (zeroed) { RK_HIP(hipMemset(p, 0, bytes)); RK_HIP(hipStreamSynchronize(nullptr)); }
			at[code] = p;
		}
		*out = at[code];
		return RK_OK;
	}
	void drop(DevPool &pool, int code) { pool.release(at[code]); at[code] = nullptr; }      // (an engine with two inputs that got only the first)
};

// `n` 20-byte host states hold only cubie codes 0..23, else "<entry>: byte b of the <what> ...", for n > 1 "... of <what> i ..."
inline int check_cubie_codes(const char *entry, const char *what, const int8_t *h_states, size_t n)
{
	for (size_t i = 0; i < n * STATE_BYTES; i++) {
		if (h_states[i] >= 0 && h_states[i] < 24) continue;
		if (n == 1) return fail(RK_EINVAL, "%s: byte %zu of the %s is %d, not a cubie code", entry, i, what, (int)h_states[i]);
		return fail(RK_EINVAL, "%s: byte %zu of %s %zu is %d, not a cubie code", entry, i % STATE_BYTES, what, i / STATE_BYTES, (int)h_states[i]);
	}
	return RK_OK;
}

// a net output handed to a step: non-null, float32 or bfloat16; *bf16 = what the launch passes on (net_out, rk_search_dev.h)
inline int check_net_out(const char *entry, const void *d_out, int dtype, int *bf16)
{
	if (!d_out) return fail(RK_EINVAL, "%s: null net output", entry);
	if (dtype != RK_OH_F32 && dtype != RK_OH_BF16) return fail(RK_EINVAL, "%s: the net's output is float32 or bfloat16, got dtype %d", entry, dtype);
	*bf16 = dtype == RK_OH_BF16 ? 1 : 0;
	return RK_OK;
}

}  // namespace
}  // namespace rk
