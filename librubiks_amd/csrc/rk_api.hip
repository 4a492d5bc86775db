// C ABI of librubiks_hip.so (declared in include/rubiks_hip.h): argument validation, error reporting and the
// host-pointer conveniences.  Nothing in here computes on the CPU: every entry either launches a HIP kernel or
// fails with an error code.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <climits>

#include "../../include/rubiks_hip.h"
#include "rk_kernels.h"
#include "rk_error.h"

namespace rk {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return code;
}

}  // namespace rk

using namespace rk;

namespace {

inline bool misaligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

inline int state_bytes(int repr) { return repr == RK_REPR_2024 ? STATE_BYTES : S686_BYTES; }

int check_repr(int repr)
{
	if (repr != RK_REPR_2024 && repr != RK_REPR_686) return fail(RK_EINVAL, "unknown representation %d", repr);
	return RK_OK;
}

// Scratch for the *_host entries: grow-only device buffers cached per host thread and device, so that a small call
// (one state through cube.rotate) costs two tiny copies and a launch instead of three hipMalloc/hipFree pairs.
struct ScratchSlot { void *p = nullptr; size_t cap = 0; int device = -1; };
thread_local ScratchSlot g_scratch[8];
thread_local int g_scratch_next = 0;

struct DevBuf {
	void *p = nullptr;
	int alloc(size_t bytes)
	{
		if (g_scratch_next >= 8) return fail(RK_ESTATE, "scratch slots exhausted");
		ScratchSlot &s = g_scratch[g_scratch_next++];
		int dev = 0;
		RK_HIP(hipGetDevice(&dev));
		if (bytes < 256) bytes = 256;
		if (s.device != dev || s.cap < bytes) {
			if (s.p && s.device == dev) (void)hipFree(s.p);
			s.p = nullptr; s.cap = 0; s.device = dev;
			RK_HIP(hipMalloc(&s.p, bytes));
			s.cap = bytes;
		}
		p = s.p;
		return RK_OK;
	}
};

// resets the slot cursor when a *_host entry starts (slots are handed out in call order, so sizes stay matched)
struct ScratchScope { ScratchScope() { g_scratch_next = 0; } };

// SMALL host calls go zero-copy: one page-locked, device-mapped buffer per host thread; the inputs are placed in it with a CPU
// memcpy, the kernel reads and writes it over the bus, the outputs are copied out after ONE stream synchronisation.  A staged
// call costs two or three hipMemcpyAsync round trips around its launch (29-37 us for one state through cube.rotate /
// is_solved, profiles/r04_reference_protocol.json -- what reference code that loops over single states sees); this way it
// costs the launch and the wait (10 000 states through multi_rotate: 410 KB, about 70 us from Python against 100 with a torch
// hop and staged copies).  Larger calls keep the staged copies (the CPU memcpy into and out of the buffer, and the kernel's
// accesses over the bus, then cost more than the copy engines do).
constexpr size_t ZERO_COPY_MAX = 1u << 20;            // staged bytes (inputs + outputs) up to which a call goes this way
struct PinnedBuf { char *host = nullptr; char *dev = nullptr; int device = -1; bool tried = false; };
thread_local PinnedBuf g_pinned;

constexpr size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the buffer of this thread for the current device, or nullptr (then the caller stages through device memory as before)
PinnedBuf *pinned_buffer()
{
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
	PinnedBuf &b = g_pinned;
	if (b.host && b.device == dev) return &b;
	if (b.tried && b.device == dev) return nullptr;
	if (b.host) { (void)hipHostFree(b.host); b.host = b.dev = nullptr; }
	b.device = dev; b.tried = true;
	void *h = nullptr, *d = nullptr;
	if (hipHostMalloc(&h, ZERO_COPY_MAX + 4096, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
	if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(h); return nullptr; }
	b.host = (char *)h; b.dev = (char *)d;
	return &b;
}

// Where the parts of a host call lie in the pinned buffer: the running sum of up256(bytes), in declaration order.  The same
// numbers decide the route (fits) and give the pointers (off); nothing else computes an offset.
constexpr int MAX_PARTS = 4;
struct Layout { size_t off[MAX_PARTS]; size_t total; };
constexpr Layout layout_of(size_t b0, size_t b1 = 0, size_t b2 = 0, size_t b3 = 0)
{
	const size_t o1 = up256(b0), o2 = o1 + up256(b1), o3 = o2 + up256(b2);
	return Layout{{0, o1, o2, o3}, o3 + up256(b3)};
}
constexpr bool fits(const Layout &l) { return l.total <= ZERO_COPY_MAX; }

// multi_rotate of one 20-byte state: states, actions, out
static_assert(layout_of(20, 1, 20).off[0] == 0 && layout_of(20, 1, 20).off[1] == 256 && layout_of(20, 1, 20).off[2] == 512, "layout");
static_assert(layout_of(20, 1, 20).total == 768 && layout_of(256, 257).off[2] == 768 && layout_of(0, 20).off[1] == 0, "layout");
static_assert(layout_of(ZERO_COPY_MAX - 512, 256, 256).total == ZERO_COPY_MAX && fits(layout_of(ZERO_COPY_MAX - 512, 256, 256)), "limit fits");
static_assert(layout_of(ZERO_COPY_MAX - 512, 256, 257).total == ZERO_COPY_MAX + 256 && !fits(layout_of(ZERO_COPY_MAX - 512, 256, 257)), "one step more does not");

const long long STATS_INIT[2] = {0, LLONG_MAX};

// One *_host call: the entry declares its arrays in order (in: host bytes the kernel reads; out: bytes the kernel writes, copied
// back when the host pointer is given -- the device part exists either way), calls begin(), launches on dev(k), returns finish().
//   zero-copy  when the entry allows it, the layout fits ZERO_COPY_MAX and this thread has its pinned buffer: the inputs are
//              memcpy'd to their offsets, the kernel works on the buffer over the bus, finish() synchronises once and memcpy's
//              the wanted outputs out
//   staged     otherwise: one scratch slot per part, hipMemcpyAsync in, the launch, hipMemcpyAsync of the wanted outputs, one
//              synchronise
// finish() synchronises on either route, also when the entry's own output is a device pointer: the pinned buffer and the slots
// belong to this thread's next call from then on.
// The counters (how many solved, the first one's index) are atomics, so they stay in device memory: an entry whose caller wants
// them does not allow zero-copy, and on that route stats() is null.  On the staged route begin(.., got) seeds one more part from
// STATS_INIT and finish() reads the two raw words back into got; what the caller sees of them is the entry's business.
struct HostCall {
	struct Part { const void *in; void *out; size_t bytes; char *dev, *pinned; };
	Part part[MAX_PARTS] = {};
	int count = 0;
	hipStream_t st;
	bool zero_copy = false;
	void *d_stats = nullptr;

	explicit HostCall(void *stream) : st((hipStream_t)stream) {}
	HostCall &in(const void *h, size_t bytes) { part[count++] = Part{h, nullptr, bytes, nullptr, nullptr}; return *this; }
	HostCall &out(void *h, size_t bytes) { part[count++] = Part{nullptr, h, bytes, nullptr, nullptr}; return *this; }
	void *dev(int k) const { return part[k].dev; }
	long long *stats() const { return (long long *)d_stats; }

	int begin(bool allow_zero_copy, long long *got = nullptr)
	{
		const Layout l = layout_of(part[0].bytes, part[1].bytes, part[2].bytes, part[3].bytes);
		PinnedBuf *b = allow_zero_copy && fits(l) ? pinned_buffer() : nullptr;
		if (b) {
			zero_copy = true;
			for (Part *p = part; p < part + count; p++) {
				p->dev = b->dev + l.off[p - part];
				p->pinned = b->host + l.off[p - part];
				if (p->in && p->bytes) memcpy(p->pinned, p->in, p->bytes);
			}
			return RK_OK;
		}
		if (got) part[count++] = Part{STATS_INIT, got, sizeof STATS_INIT, nullptr, nullptr};
		ScratchScope scope;                          // slots in declaration order: a thread's cached slot sizes stay matched
		for (Part *p = part; p < part + count; p++) {
			DevBuf d;
			if (int e = d.alloc(p->bytes)) return e;
			p->dev = (char *)d.p;
		}
		if (got) d_stats = part[count - 1].dev;
		for (Part *p = part; p < part + count; p++)
			if (p->in && p->bytes) RK_HIP(hipMemcpyAsync(p->dev, p->in, p->bytes, hipMemcpyHostToDevice, st));
		return RK_OK;
	}

	int finish()
	{
		if (zero_copy) RK_HIP(hipStreamSynchronize(st));
		for (Part *p = part; p < part + count; p++) {
			if (!p->out || !p->bytes) continue;
			if (zero_copy) memcpy(p->out, p->pinned, p->bytes);
			else RK_HIP(hipMemcpyAsync(p->out, p->dev, p->bytes, hipMemcpyDeviceToHost, st));
		}
		if (!zero_copy) RK_HIP(hipStreamSynchronize(st));
		return RK_OK;
	}
};

// what expand12 and is_solved report: {how many solved, the first one's index or -1}
inline void solved_stats(long long *h_stats, const long long got[2])
{
	if (h_stats) { h_stats[0] = got[0]; h_stats[1] = got[0] ? got[1] : -1; }
}

}  // namespace

extern "C" {

int rk_version(void) { return 100; }

const char *rk_last_error(void) { return g_err; }

int rk_init(int device)
{
	int count = 0;
	RK_HIP(hipGetDeviceCount(&count));
	if (device < 0 || device >= count) return fail(RK_EINVAL, "device %d out of range (%d visible)", device, count);
	RK_HIP(hipSetDevice(device));
	hipDeviceProp_t prop;
	RK_HIP(hipGetDeviceProperties(&prop, device));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return fail(RK_EINVAL, "device %d is %s; this library only carries gfx950 code", device, prop.gcnArchName);
	(void)calibrate_pacing(false);          // once per device and process, about 4 ms; a calibration that cannot run keeps the compiled schedule
	return RK_OK;
}

int rk_tables(int repr, uint8_t *h_out)
{
	if (int e = check_repr(repr)) return e;
	if (!h_out) return fail(RK_EINVAL, "rk_tables: null output");
	const Tables &t = host_tables();
	if (repr == RK_REPR_2024) memcpy(h_out, t.lut, sizeof t.lut);
	else memcpy(h_out, t.perm686, sizeof t.perm686);
	return RK_OK;
}

int rk_face_definitions(uint8_t *h_out)
{
	if (!h_out) return fail(RK_EINVAL, "rk_face_definitions: null output");
	for (int f = 0; f < 6; f++) {
		uint8_t *o = h_out + 14 * f;
		for (int j = 0; j < 4; j++) {
			o[j] = FACES[f].corner[j];
			o[4 + j] = FACES[f].edge[j];
			o[10 + j] = NEIGHBOUR[f][j];
		}
		o[8] = FACES[f].fixed_ori;
		o[9] = FACES[f].flip;
	}
	return RK_OK;
}

int rk_solved(int repr, int8_t *h_out)
{
	if (int e = check_repr(repr)) return e;
	if (!h_out) return fail(RK_EINVAL, "rk_solved: null output");
	const Tables &t = host_tables();
	if (repr == RK_REPR_2024) memcpy(h_out, t.solved, STATE_BYTES);
	else memcpy(h_out, t.solved686, S686_BYTES);
	return RK_OK;
}

int rk_malloc(void **d_ptr, size_t bytes)
{
	if (!d_ptr) return fail(RK_EINVAL, "rk_malloc: null out pointer");
	RK_HIP(hipMalloc(d_ptr, bytes ? bytes : 16));
	return RK_OK;
}

int rk_free(void *d_ptr)
{
	RK_HIP(hipFree(d_ptr));
	return RK_OK;
}

int rk_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream)
{
	RK_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
	return RK_OK;
}

int rk_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream)
{
	RK_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
	return RK_OK;
}

int rk_memset(void *d_dst, int value, size_t bytes, void *stream)
{
	RK_HIP(hipMemsetAsync(d_dst, value, bytes, (hipStream_t)stream));
	return RK_OK;
}

int rk_stream_synchronize(void *stream)
{
	RK_HIP(hipStreamSynchronize((hipStream_t)stream));
	return RK_OK;
}

// ---- device-pointer entries ---------------------------------------------------------------------------------

int rk_multi_rotate(int repr, const int8_t *d_states, const uint8_t *d_actions, int8_t *d_out, size_t n, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (n == 0) return RK_OK;
	if (!d_states || !d_actions || !d_out) return fail(RK_EINVAL, "rk_multi_rotate: null pointer");
	if (misaligned(d_states, 4) || misaligned(d_out, 4)) return fail(RK_EINVAL, "rk_multi_rotate: state arrays must be 4-byte aligned");
	if (repr == RK_REPR_686 && (misaligned(d_out, 16) || misaligned(d_states, 16)))
		return fail(RK_EINVAL, "rk_multi_rotate: 6x8x6 state arrays must be 16-byte aligned");
	if (repr == RK_REPR_2024) launch_multi_rotate(d_states, d_actions, nullptr, d_out, n, (hipStream_t)stream);
	else {
		if (d_out == d_states) return fail(RK_EINVAL, "rk_multi_rotate: in-place not supported for the 6x8x6 representation");
		launch_rotate686(d_states, d_actions, d_out, n, false, (hipStream_t)stream);
	}
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_set_pacing(int mode)
{
	set_pace_override(mode);
	return RK_OK;
}

int rk_calibrate_pacing(int force)
{
	if (calibrate_pacing(force != 0) != 0) return fail(RK_EHIP, "rk_calibrate_pacing: no current device");
	return RK_OK;
}

int rk_get_pacing(unsigned int *tau_ps, int *source, float *h_us)
{
	get_pacing(tau_ps, source, h_us);
	return RK_OK;
}

int rk_pace_slot_of_device(int device) { return pace_slot_of_device(device); }

int rk_stream_register(void *stream)
{
	register_stream((hipStream_t)stream);
	return RK_OK;
}

int rk_stream_forget(void *stream)
{
	forget_stream((hipStream_t)stream);
	return RK_OK;
}

int rk_multi_rotate_solved(int repr, const int8_t *d_states, const uint8_t *d_actions, int8_t *d_out, uint8_t *d_flags, long long *d_stats,
                           size_t n, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (n == 0) return RK_OK;
	if (!d_states || !d_actions || !d_out) return fail(RK_EINVAL, "rk_multi_rotate_solved: null pointer");
	if (!d_flags && !d_stats) return fail(RK_EINVAL, "rk_multi_rotate_solved: flags or stats (or both) must be given");
	if (misaligned(d_states, 4) || misaligned(d_out, 4)) return fail(RK_EINVAL, "rk_multi_rotate_solved: state arrays must be 4-byte aligned");
	if (d_stats && misaligned(d_stats, 8)) return fail(RK_EINVAL, "rk_multi_rotate_solved: stats must be 8-byte aligned");
	if (repr == RK_REPR_2024) {
		launch_multi_rotate(d_states, d_actions, nullptr, d_out, n, (hipStream_t)stream, d_flags, d_stats, true);
	} else {
		// 6x8x6: the goal test reads the moved states back (two launches; the fused form exists for the 20-byte states)
		if (misaligned(d_out, 16) || misaligned(d_states, 16)) return fail(RK_EINVAL, "rk_multi_rotate_solved: 6x8x6 state arrays must be 16-byte aligned");
		if (d_out == d_states) return fail(RK_EINVAL, "rk_multi_rotate_solved: in-place not supported for the 6x8x6 representation");
		launch_rotate686(d_states, d_actions, d_out, n, false, (hipStream_t)stream);
		launch_is_solved686(d_out, d_flags, d_stats, n, (hipStream_t)stream);
	}
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_bad_actions_seen(int *h_seen, void *stream)
{
	if (!h_seen) return fail(RK_EINVAL, "rk_bad_actions_seen: null pointer");
	const int r = read_bad_actions((hipStream_t)stream);
	if (r < 0) return fail(RK_EHIP, "rk_bad_actions_seen: could not read the device flag");
	*h_seen = r;
	return RK_OK;
}

int rk_multi_rotate_fd(int repr, const int8_t *d_states, const uint8_t *d_faces, const uint8_t *d_dirs, int8_t *d_out,
                       size_t n, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (repr != RK_REPR_2024) return fail(RK_EINVAL, "rk_multi_rotate_fd: only the 20-byte representation; pass action indices for 6x8x6");
	if (n == 0) return RK_OK;
	if (!d_states || !d_faces || !d_dirs || !d_out) return fail(RK_EINVAL, "rk_multi_rotate_fd: null pointer");
	if (misaligned(d_states, 4) || misaligned(d_out, 4)) return fail(RK_EINVAL, "rk_multi_rotate_fd: state arrays must be 4-byte aligned");
	launch_multi_rotate(d_states, d_faces, d_dirs, d_out, n, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_expand12(int repr, const int8_t *d_parents, int8_t *d_children, uint8_t *d_solved, long long *d_stats, size_t n,
                void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (n == 0) return RK_OK;
	if (!d_parents || !d_children) return fail(RK_EINVAL, "rk_expand12: null pointer");
	if (misaligned(d_parents, 4)) return fail(RK_EINVAL, "rk_expand12: parents must be 4-byte aligned");
	if (misaligned(d_children, 16)) return fail(RK_EINVAL, "rk_expand12: children must be 16-byte aligned");
	if (d_solved && misaligned(d_solved, 4)) return fail(RK_EINVAL, "rk_expand12: solved flags must be 4-byte aligned");
	if (d_stats && misaligned(d_stats, 8)) return fail(RK_EINVAL, "rk_expand12: stats must be 8-byte aligned");
	if (d_stats && !d_solved && repr == RK_REPR_2024) return fail(RK_EINVAL, "rk_expand12: stats need the solved-flag output");
	if (repr == RK_REPR_2024) {
		launch_expand12(d_parents, d_children, d_solved, d_stats, n, (hipStream_t)stream);
	} else {
		if (misaligned(d_parents, 16)) return fail(RK_EINVAL, "rk_expand12: 6x8x6 parents must be 16-byte aligned");
		launch_rotate686(d_parents, nullptr, d_children, 12 * n, true, (hipStream_t)stream, d_solved, d_stats);   // flags fused: one launch
	}
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_expand12_soa(const uint32_t *d_parents, uint32_t *d_children, uint8_t *d_solved, long long *d_stats, size_t n, void *stream)
{
	if (n == 0) return RK_OK;
	if (!d_parents || !d_children) return fail(RK_EINVAL, "rk_expand12_soa: null pointer");
	if (misaligned(d_parents, 4) || misaligned(d_children, 4)) return fail(RK_EINVAL, "rk_expand12_soa: planes must be 4-byte aligned");
	if (d_stats && (!d_solved || misaligned(d_stats, 8))) return fail(RK_EINVAL, "rk_expand12_soa: stats need flags and 8-byte alignment");
	launch_expand12_soa(d_parents, d_children, d_solved, d_stats, n, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_states_to_soa(const int8_t *d_states, uint32_t *d_planes, size_t n, void *stream)
{
	if (n == 0) return RK_OK;
	if (!d_states || !d_planes || misaligned(d_states, 4) || misaligned(d_planes, 4)) return fail(RK_EINVAL, "rk_states_to_soa: bad pointer");
	launch_states_soa(d_states, d_planes, n, true, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_states_from_soa(const uint32_t *d_planes, int8_t *d_states, size_t n, void *stream)
{
	if (n == 0) return RK_OK;
	if (!d_states || !d_planes || misaligned(d_states, 4) || misaligned(d_planes, 4)) return fail(RK_EINVAL, "rk_states_from_soa: bad pointer");
	launch_states_soa(d_states, const_cast<uint32_t *>(d_planes), n, false, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

#ifdef RK_TUNING
/* Tuning hook, deliberately outside the public header: other shapes of the fan-out kernel (benchmarks/tune_expand.py). */
int rkx_expand12_variant(int variant, const int8_t *d_parents, int8_t *d_children, uint8_t *d_solved, long long *d_stats, size_t n,
                         unsigned int *d_counter, int grid_blocks, void *stream)
{
	if (!d_parents || !d_children || !d_solved || misaligned(d_children, 16)) return fail(RK_EINVAL, "rkx_expand12_variant: bad argument");
	tune_cell(d_counter);
	launch_expand12_variant(variant, d_parents, d_children, d_solved, d_stats, n, grid_blocks, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rkx_pace_debug(void *d_buf) { tune_pace_debug(d_buf); return RK_OK; }

int rkx_as_oh_variant(int tile, int grid_cap, const int8_t *d_states, void *d_out, int out_dtype, size_t n, void *stream)
{
	if (!d_states || !d_out || misaligned(d_out, 16)) return fail(RK_EINVAL, "rkx_as_oh_variant: bad argument");
	launch_as_oh_variant(tile, grid_cap, d_states, d_out, out_dtype, n, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

#endif  /* RK_TUNING */

int rk_multi_is_solved(int repr, const int8_t *d_states, uint8_t *d_flags, long long *d_stats, size_t n, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (n == 0) return RK_OK;
	if (!d_states) return fail(RK_EINVAL, "rk_multi_is_solved: null states");
	if (misaligned(d_states, 4)) return fail(RK_EINVAL, "rk_multi_is_solved: states must be 4-byte aligned");
	if (d_stats && misaligned(d_stats, 8)) return fail(RK_EINVAL, "rk_multi_is_solved: stats must be 8-byte aligned");
	if (repr == RK_REPR_686 && misaligned(d_states, 16)) return fail(RK_EINVAL, "rk_multi_is_solved: 6x8x6 states must be 16-byte aligned");
	if (repr == RK_REPR_2024) launch_multi_is_solved(d_states, d_flags, d_stats, n, (hipStream_t)stream);
	else launch_is_solved686(d_states, d_flags, d_stats, n, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_apply_sequences(int repr, const uint8_t *d_actions, int depth, int games, int with_solved, int only_last,
                       int8_t *d_out, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (repr != RK_REPR_2024) return fail(RK_EINVAL, "rk_apply_sequences: only the 20-byte representation is implemented");
	if (depth < 0 || games < 0) return fail(RK_EINVAL, "rk_apply_sequences: negative size");
	with_solved = with_solved ? 1 : 0;
	const int moves = depth - with_solved;
	if (games == 0 || (moves < 0)) return RK_OK;
	if (!only_last && moves + with_solved == 0) return RK_OK;
	if (!d_out || (moves > 0 && !d_actions)) return fail(RK_EINVAL, "rk_apply_sequences: null pointer");
	if (misaligned(d_out, 4)) return fail(RK_EINVAL, "rk_apply_sequences: output must be 4-byte aligned");
	launch_apply_sequences(d_actions, moves, games, with_solved, only_last ? 1 : 0, d_out, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_rollout_fanout(int repr, const uint8_t *d_actions, int depth, int games, int with_solved, int8_t *d_states, uint8_t *d_state_flags,
                      int8_t *d_children, uint8_t *d_child_flags, long long *d_stats, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (repr != RK_REPR_2024) return fail(RK_EINVAL, "rk_rollout_fanout: only the 20-byte representation is implemented");
	if (depth < 0 || games < 0) return fail(RK_EINVAL, "rk_rollout_fanout: negative size");
	with_solved = with_solved ? 1 : 0;
	const int moves = depth - with_solved;
	if (games == 0 || moves < 0 || moves + with_solved == 0) return RK_OK;
	if (!d_states || !d_children || !d_child_flags || (moves > 0 && !d_actions)) return fail(RK_EINVAL, "rk_rollout_fanout: null pointer");
	if (misaligned(d_states, 4) || misaligned(d_children, 16) || misaligned(d_child_flags, 4))
		return fail(RK_EINVAL, "rk_rollout_fanout: states / child flags must be 4-byte aligned, children 16-byte aligned");
	if (d_stats && misaligned(d_stats, 8)) return fail(RK_EINVAL, "rk_rollout_fanout: stats must be 8-byte aligned");
	if ((size_t)games * depth > ((size_t)1 << 31)) return fail(RK_EINVAL, "rk_rollout_fanout: more than 2^31 states");
	launch_rollout_fanout(d_actions, moves, games, with_solved, d_states, d_state_flags, d_children, d_child_flags, d_stats, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_as_oh(int repr, const int8_t *d_states, void *d_out, int out_dtype, size_t n, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (out_dtype < RK_OH_F32 || out_dtype > RK_OH_BF16) return fail(RK_EINVAL, "rk_as_oh: unknown output dtype %d", out_dtype);
	if (n == 0) return RK_OK;
	if (!d_states || !d_out) return fail(RK_EINVAL, "rk_as_oh: null pointer");
	if (misaligned(d_states, 4)) return fail(RK_EINVAL, "rk_as_oh: states must be 4-byte aligned");
	if (misaligned(d_out, 16)) return fail(RK_EINVAL, "rk_as_oh: output must be 16-byte aligned");
	if (repr == RK_REPR_2024) launch_as_oh(d_states, d_out, out_dtype, n, (hipStream_t)stream);
	else launch_as_oh686(d_states, d_out, out_dtype, n, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_as_correct686(const int8_t *d_states, float *d_out, size_t n, void *stream)
{
	if (n == 0) return RK_OK;
	if (!d_states || !d_out) return fail(RK_EINVAL, "rk_as_correct686: null pointer");
	launch_as_correct686(d_states, d_out, n, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_oh686_from2024(const int8_t *d_states20, void *d_out, int out_dtype, size_t n, void *stream)
{
	if (out_dtype != RK_OH_F32 && out_dtype != RK_OH_F16 && out_dtype != RK_OH_BF16 && out_dtype != RK_OH_I8)
		return fail(RK_EINVAL, "rk_oh686_from2024: unknown output dtype %d", out_dtype);
	if (n == 0) return RK_OK;
	if (!d_states20 || !d_out) return fail(RK_EINVAL, "rk_oh686_from2024: null pointer");
	if (misaligned(d_states20, 4)) return fail(RK_EINVAL, "rk_oh686_from2024: states must be 4-byte aligned");
	if (misaligned(d_out, 16)) return fail(RK_EINVAL, "rk_oh686_from2024: output must be 16-byte aligned");
	launch_oh686_from2024(d_states20, d_out, out_dtype, n, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_686_to2024(const int8_t *d_states686, int8_t *d_out20, long long *d_stats, size_t n, void *stream)
{
	if (n == 0) return RK_OK;
	if (!d_states686 || !d_out20) return fail(RK_EINVAL, "rk_686_to2024: null pointer");
	if (misaligned(d_states686, 16)) return fail(RK_EINVAL, "rk_686_to2024: 6x8x6 states must be 16-byte aligned");
	if (misaligned(d_out20, 4)) return fail(RK_EINVAL, "rk_686_to2024: output must be 4-byte aligned");
	if (d_stats && misaligned(d_stats, 8)) return fail(RK_EINVAL, "rk_686_to2024: stats must be 8-byte aligned");
	launch_686_to2024(d_states686, d_out20, d_stats, n, (hipStream_t)stream);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

// ---- host-pointer conveniences ------------------------------------------------------------------------------

// Each one: its checks, its parts in order, one launch on the parts' device pointers, its counter mapping (see HostCall).

int rk_multi_rotate_host(int repr, const int8_t *h_states, const uint8_t *h_actions, int8_t *h_out, size_t n, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (n == 0) return RK_OK;
	if (!h_states || !h_actions || !h_out) return fail(RK_EINVAL, "rk_multi_rotate_host: null pointer");
	for (size_t i = 0; i < n; i++)
		if (h_actions[i] >= N_ACTIONS) return fail(RK_EINVAL, "rk_multi_rotate_host: action %u at row %zu out of range", h_actions[i], i);
	const size_t sb = (size_t)state_bytes(repr);
	HostCall c(stream);
	c.in(h_states, n * sb).in(h_actions, n).out(h_out, n * sb);
	if (int e = c.begin(true)) return e;
	if (int e = rk_multi_rotate(repr, (const int8_t *)c.dev(0), (const uint8_t *)c.dev(1), (int8_t *)c.dev(2), n, stream)) return e;
	return c.finish();
}

int rk_expand12_host(int repr, const int8_t *h_parents, int8_t *h_children, uint8_t *h_solved, long long *h_stats, size_t n,
                     void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (h_stats) { h_stats[0] = 0; h_stats[1] = -1; }
	if (n == 0) return RK_OK;
	if (!h_parents || !h_children) return fail(RK_EINVAL, "rk_expand12_host: null pointer");
	const size_t sb = (size_t)state_bytes(repr);
	long long got[2];
	HostCall c(stream);
	c.in(h_parents, n * sb).out(h_children, 12 * n * sb).out(h_solved, 12 * n);
	if (int e = c.begin(!h_stats, got)) return e;
	uint8_t *d_solved = h_solved || c.stats() ? (uint8_t *)c.dev(2) : nullptr;     // the counters need the flags
	if (int e = rk_expand12(repr, (const int8_t *)c.dev(0), (int8_t *)c.dev(1), d_solved, c.stats(), n, stream)) return e;
	if (int e = c.finish()) return e;
	solved_stats(h_stats, got);
	return RK_OK;
}

int rk_multi_is_solved_host(int repr, const int8_t *h_states, uint8_t *h_flags, long long *h_stats, size_t n, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (h_stats) { h_stats[0] = 0; h_stats[1] = -1; }
	if (n == 0) return RK_OK;
	if (!h_states) return fail(RK_EINVAL, "rk_multi_is_solved_host: null pointer");
	long long got[2];
	HostCall c(stream);
	c.in(h_states, n * (size_t)state_bytes(repr)).out(h_flags, n);
	if (int e = c.begin(!h_stats, h_stats ? got : nullptr)) return e;      // the counters cost two extra copies: only when asked for
	if (int e = rk_multi_is_solved(repr, (const int8_t *)c.dev(0), (uint8_t *)c.dev(1), c.stats(), n, stream)) return e;
	if (int e = c.finish()) return e;
	solved_stats(h_stats, got);
	return RK_OK;
}

int rk_apply_sequences_host(int repr, const uint8_t *h_actions, int depth, int games, int with_solved, int only_last,
                            int8_t *h_out, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (repr != RK_REPR_2024) return fail(RK_EINVAL, "rk_apply_sequences_host: only the 20-byte representation is implemented");
	if (depth < 0 || games < 0) return fail(RK_EINVAL, "rk_apply_sequences_host: negative size");
	with_solved = with_solved ? 1 : 0;
	const int moves = depth - with_solved;
	if (games == 0 || moves < 0) return RK_OK;
	const size_t rows = only_last ? 1 : (size_t)(moves + with_solved);
	if (rows == 0) return RK_OK;
	if (!h_out || (moves > 0 && !h_actions)) return fail(RK_EINVAL, "rk_apply_sequences_host: null pointer");
	const size_t nact = (size_t)moves * games;
	for (size_t i = 0; i < nact; i++)
		if (h_actions[i] >= N_ACTIONS) return fail(RK_EINVAL, "rk_apply_sequences_host: action %u out of range", h_actions[i]);
	HostCall c(stream);
	c.in(h_actions, nact).out(h_out, (size_t)games * rows * STATE_BYTES);      // no moves: an empty part, nothing is copied
	if (int e = c.begin(true)) return e;
	if (int e = rk_apply_sequences(repr, (const uint8_t *)c.dev(0), depth, games, with_solved, only_last, (int8_t *)c.dev(1), stream)) return e;
	return c.finish();
}

int rk_as_oh_host(int repr, const int8_t *h_states, void *d_out, int out_dtype, size_t n, void *stream)
{
	if (int e = check_repr(repr)) return e;
	if (n == 0) return RK_OK;
	if (!h_states || !d_out) return fail(RK_EINVAL, "rk_as_oh_host: null pointer");
	HostCall c(stream);
	c.in(h_states, n * (size_t)state_bytes(repr));
	if (int e = c.begin(true)) return e;
	if (int e = rk_as_oh(repr, (const int8_t *)c.dev(0), d_out, out_dtype, n, stream)) return e;
	return c.finish();
}

int rk_oh686_from2024_host(const int8_t *h_states20, void *d_out, int out_dtype, size_t n, void *stream)
{
	if (out_dtype != RK_OH_F32 && out_dtype != RK_OH_F16 && out_dtype != RK_OH_BF16 && out_dtype != RK_OH_I8)
		return fail(RK_EINVAL, "rk_oh686_from2024_host: unknown output dtype %d", out_dtype);
	if (n == 0) return RK_OK;
	if (!h_states20 || !d_out) return fail(RK_EINVAL, "rk_oh686_from2024_host: null pointer");
	if (misaligned(d_out, 16)) return fail(RK_EINVAL, "rk_oh686_from2024_host: output must be 16-byte aligned");
	HostCall c(stream);
	c.in(h_states20, n * STATE_BYTES);
	if (int e = c.begin(true)) return e;
	if (int e = rk_oh686_from2024((const int8_t *)c.dev(0), d_out, out_dtype, n, stream)) return e;
	return c.finish();
}

int rk_686_to2024_host(const int8_t *h_states686, int8_t *h_out20, long long *h_stats, size_t n, void *stream)
{
	if (n == 0) return RK_OK;
	if (!h_states686 || !h_out20) return fail(RK_EINVAL, "rk_686_to2024_host: null pointer");
	long long got[2];
	HostCall c(stream);
	c.in(h_states686, n * S686_BYTES).out(h_out20, n * STATE_BYTES);
	if (int e = c.begin(false, got)) return e;       // always staged: it always counts (illegal rows, the first one's index)
	if (int e = rk_686_to2024((const int8_t *)c.dev(0), (int8_t *)c.dev(1), c.stats(), n, stream)) return e;
	if (int e = c.finish()) return e;
	if (h_stats) { h_stats[0] = got[0]; h_stats[1] = got[1]; }       // the raw words
	return RK_OK;
}

}  // extern "C"
