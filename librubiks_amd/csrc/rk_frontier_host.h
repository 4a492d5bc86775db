// The host half of the breadth-first engines that keep their whole search in HBM and of the kept balls they end at: FrontierPool
// (rk_bfs, rk_bibfs, rk_bsearch, rk_ssearch; device half rk_frontier_dev.h), FrontierSlots (the two lock-step batches of such
// searches), KeptBall (the two ball builds, rk_ballbuild_dev.h) and BallReader (a search handle's hold on its ball).  Apart from
// rk_search_host.h because it launches rk_frontier_dev.h's kernels, which have internal linkage: a file that includes this
// carries them, so only rk_bfs.hip, rk_bibfs.hip, rk_ball.hip and rk_sym.hip do.  Header-only, nothing in here is exported.
#pragma once
#include "rk_ballbuild_dev.h"
#include "rk_frontier_dev.h"
#include "rk_search_host.h"

namespace rk {
namespace {

// Rows first .. first + count - 1 of a breadth-first pool for the host: states as they are, parents widened, pact split into the
// action and the tag above it (rk_frontier_dev.h: PACT_TAG_SHIFT).  A null column asks for nothing.
inline int export_pool_rows(const uint32_t *states, const int32_t *parent, const uint8_t *pact, size_t first, size_t count, int8_t *h_states,
                            long long *h_parents, long long *h_actions, long long *h_tags, hipStream_t st)
{
	if (count == 0) return RK_OK;
	Widened<int32_t, long long> p;
	std::vector<uint8_t> pa;
	if (h_states) RK_HIP(hipMemcpyAsync(h_states, states + first * 5, count * STATE_BYTES, hipMemcpyDeviceToHost, st));
	if (int e = p.start(parent + first, count, h_parents, st)) return e;
	if (h_actions || h_tags) {
		pa.resize(count);
		RK_HIP(hipMemcpyAsync(pa.data(), pact + first, count, hipMemcpyDeviceToHost, st));
	}
	RK_HIP(hipStreamSynchronize(st));
	p.finish();
	for (size_t i = 0; i < pa.size(); i++) {
		if (h_actions) h_actions[i] = pa[i] & PACT_ACTION;
		if (h_tags) h_tags[i] = pa[i] >> PACT_TAG_SHIFT;
	}
	return RK_OK;
}

// The host half of a frontier pool (rk_frontier_dev.h): the descriptor and what the engines rk_bfs, rk_bibfs, rk_bsearch and
// rk_ssearch do with it in the same way.  An engine's handle is this plus its own members; its entries check their arguments
// and call one of these with their own name as `who`, the prefix of every error text.
constexpr size_t FRONTIER_MAX_CAPACITY = 0x3FFFFFF0ull;
constexpr int FRONTIER_MAX_POPS = 1 << 22;
constexpr int FRONTIER_MAX_COUNTERS = 32;

struct FrontierPool {
	using Kernel = void (*)(FrontierDev);

	FrontierDev d{};
	size_t cap = 0;
	uint32_t *root_dev = nullptr;
	int32_t *walk = nullptr;                    // what the walk kernel writes: FRONTIER_WALK_MAX actions behind the length
	Landing ctr_host;                           // page-locked landing place of the counter block
	int n_ctr = 0;
	bool ready = false;
	DevPool pool{64};

	static uint32_t table_mask(size_t capacity) { return (uint32_t)(table_slots(capacity, 1024) - 1); }

	// the range checks of a *_create
	static int check_create(const char *who, size_t capacity, int pops)
	{
		if (capacity < 2 || capacity > FRONTIER_MAX_CAPACITY) return fail(RK_EINVAL, "%s: capacity %zu out of range", who, capacity);
		if (pops < 1 || pops > FRONTIER_MAX_POPS) return fail(RK_EINVAL, "%s: pops %d outside 1..%d", who, pops, FRONTIER_MAX_POPS);
		return RK_OK;
	}
	// *_run, *_grow, *_export, *_path of a handle that was never reset
	static int check_ready(const FrontierPool *h, const char *who)
	{
		return h && h->ready ? RK_OK : fail(RK_ESTATE, "%s: reset the engine first", who);
	}

	// every array of a pool of `capacity` states that pops `pops` nodes per iteration and has `counters` counter words
	int alloc(size_t capacity, int pops, int counters)
	{
		cap = capacity;
		n_ctr = counters;
		d.pops = pops;
		d.cap1 = (uint32_t)(capacity + 1);
		d.mask = table_mask(capacity);
		const size_t C1 = capacity + 1, K = (size_t)12 * pops;
		int e = RK_OK;
		#define A(ptr, cnt) if (!e) e = pool.alloc(&ptr, (cnt))
		A(d.states, C1 * 5); A(d.parent, C1); A(d.pact, C1); A(d.table, (size_t)d.mask + 1); A(d.ctr, (size_t)counters);
		A(d.slot, K); A(d.rank, K); A(d.first, K); A(d.chain, frontier_scan_blocks(pops));
		A(root_dev, 8); A(walk, FRONTIER_WALK_MAX + 8);
		#undef A
		if (!e) ctr_host.reserve((size_t)counters);
		return e;
	}

	// a new search: the table and the look-back words cleared, the start on the device, then the engine's root launch
	template <typename Root>
	int reset(const int8_t *h_start_state, hipStream_t st, Root &&launch_root)
	{
		RK_HIP(hipMemsetAsync(d.table, 0, ((size_t)d.mask + 1) * sizeof(uint32_t), st));                        // the own table only
		RK_HIP(hipMemsetAsync(d.chain, 0, frontier_scan_blocks(d.pops) * sizeof(unsigned long long), st));      // look-back epochs restart
		RK_HIP(hipMemcpyAsync(root_dev, h_start_state, STATE_BYTES, hipMemcpyHostToDevice, st));
		launch_root();
		RK_HIP(hipGetLastError());
		RK_HIP(hipStreamSynchronize(st));       // the host buffer may go away after return
		ready = true;
		return RK_OK;
	}

	// `iterations` iterations: the engine's expand launch(es) on a grid of `grid` workgroups of 256, then scan, append and end.
	// The append and the end are the searches' that end at a kept ball unless the engine brings its own (rk_bibfs.hip: the side
	// tag, its level bookkeeping; rk_bfs.hip: its stopping rule).
	template <typename Expand>
	int run(const char *who, int iterations, hipStream_t st, Expand &&launch_expand, Kernel append = k_fr_append, Kernel end = k_srch_end)
	{
		if (iterations < 0) return fail(RK_EINVAL, "%s: iterations %d < 0", who, iterations);
		const size_t K = (size_t)12 * d.pops;
		const unsigned grid = blocks(K);
		for (int it = 0; it < iterations; it++) {
			launch_expand(grid);
			hipLaunchKernelGGL(k_fr_scan, dim3(blocks(K, ASCAN)), dim3(ASCAN), 0, st, d);
			hipLaunchKernelGGL(append, dim3(grid), dim3(256), 0, st, d);
			hipLaunchKernelGGL(end, dim3(1), dim3(64), 0, st, d);
		}
		RK_HIP(hipGetLastError());
		return RK_OK;
	}

	// the table cleared and every stored state entered again
	static hipError_t rebuild_table(const FrontierDev &x, size_t rows, hipStream_t st)
	{
		RK_FILL(hipMemsetAsync(x.table, 0, ((size_t)x.mask + 1) * sizeof(uint32_t), st));
		hipLaunchKernelGGL(k_fr_rehash, dim3(std::max<unsigned>(1u, std::min<unsigned>(blocks(rows), 4096u))), dim3(256), 0, st, x);
		return hipGetLastError();
	}

	// the pool, its parents and actions and its table in place at `new_capacity`, all or nothing
	int grow(const char *who, size_t new_capacity, hipStream_t st)
	{
		if (new_capacity <= cap) return new_capacity == cap ? RK_OK : fail(RK_EINVAL, "%s: %zu is below the current capacity %zu", who, new_capacity, cap);
		if (new_capacity > FRONTIER_MAX_CAPACITY) return fail(RK_EINVAL, "%s: capacity %zu out of range", who, new_capacity);
		const FrontierDev old = d;
		FrontierDev x = old;
		const size_t C1 = new_capacity + 1, C1_old = cap + 1;
		x.cap1 = (uint32_t)C1;
		x.mask = table_mask(new_capacity);
		Growth g(pool, who);
		g.request(&x.states, C1 * 5); g.request(&x.parent, C1); g.request(&x.pact, C1); g.request(&x.table, (size_t)x.mask + 1);
		if (!g.granted()) return fail(RK_ECAPACITY, "%s: no device memory for a pool of %zu states", who, new_capacity);
		const int e = g.fill(st, [&]() -> hipError_t {
			RK_FILL(hipMemcpyAsync(x.states, old.states, C1_old * STATE_BYTES, hipMemcpyDeviceToDevice, st));
			RK_FILL(hipMemcpyAsync(x.parent, old.parent, C1_old * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
			RK_FILL(hipMemcpyAsync(x.pact, old.pact, C1_old, hipMemcpyDeviceToDevice, st));
			return rebuild_table(x, C1_old, st);
		});
		if (e) return e;
		g.commit();
		d = x;
		cap = new_capacity;
		return RK_OK;
	}

	int read_ctr(int32_t *out, hipStream_t st) { return ctr_host.read(d.ctr, (size_t)n_ctr, out, st); }

	// *_size: the states stored, 0 before the first reset
	static long long size(const FrontierPool *hc)
	{
		FrontierPool *h = const_cast<FrontierPool *>(hc);
		if (!h || !h->ready) return 0;
		int32_t c[FRONTIER_MAX_COUNTERS];
		if (h->read_ctr(c, nullptr)) return RK_EHIP;
		return c[F_SIZE];
	}

	int export_rows(const char *who, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, long long *h_tags,
	                hipStream_t st)
	{
		if (first + count > cap + 1) return fail(RK_EINVAL, "%s: rows %zu..%zu outside the pool", who, first, first + count);
		return export_pool_rows(d.states, d.parent, d.pact, first, count, h_states, h_parents, h_actions, h_tags, st);
	}
};

// The host half of a kept ball (rk_ballbuild_dev.h): what rk_ball and rk_symball hold and do in the same way.  A ball's handle is
// this plus its descriptor, its view and what it reports of its own; its entries pass their own name as `who`, the prefix of
// every error text.  Creating a ball costs nothing: the arrays are made by the build.
struct KeptBall {
	size_t cap = 0;
	long long size = 0, iterations = 0;
	int attached = 0;                           // searches that hold this ball's arrays
	bool built = false;
	Landing ctr_host;
	DevPool pool{64};

	static int check_create(const char *who, const void *out, int radius, int max_radius, int pops)
	{
		if (!out) return fail(RK_EINVAL, "%s: null out pointer", who);
		if (radius < 0 || radius > max_radius) return fail(RK_EINVAL, "%s: radius %d outside 0..%d", who, radius, max_radius);
		if (pops < 1 || pops > FRONTIER_MAX_POPS) return fail(RK_EINVAL, "%s: pops %d outside 1..%d", who, pops, FRONTIER_MAX_POPS);
		return RK_OK;
	}
	static int check_destroy(const char *who, const KeptBall *h)
	{
		return h && h->attached > 0 ? fail(RK_ESTATE, "%s: %d searches still hold this ball", who, h->attached) : RK_OK;
	}
	static int check_build(const char *who, const KeptBall *h, int poll)
	{
		if (!h) return fail(RK_EINVAL, "%s: null ball", who);
		if (poll < 1) return fail(RK_EINVAL, "%s: poll %d < 1", who, poll);
		return RK_OK;
	}
	// queries: n 20-byte rows on the device, read as dwords (`rows`: what the entry calls them)
	static int check_queries(const char *who, const char *rows, const KeptBall *h, const void *d_states, size_t n, const void *out)
	{
		if (!h) return fail(RK_EINVAL, "%s: null ball", who);
		if (!h->built) return fail(RK_ESTATE, "%s: build the ball first", who);
		if (n > (size_t)INT32_MAX) return fail(RK_EINVAL, "%s: %zu %s in one launch", who, n, rows);
		if (n != 0 && (!d_states || !out)) return fail(RK_EINVAL, "%s: null pointer", who);
		if (((uintptr_t)d_states | (uintptr_t)out) & 3u) return fail(RK_EINVAL, "%s: device pointers must be 4-byte aligned", who);
		return RK_OK;
	}

	void describe(BuildDev &d, size_t capacity, int radius, int pops)
	{
		cap = capacity;
		d.pops = pops;
		d.radius = radius;
		d.cap1 = (uint32_t)(capacity + 1);
		d.mask = FrontierPool::table_mask(capacity);
	}

	// The build up to the counter block it ends with, `c` (BB_COUNT words): what a failed build left is cleared, the common arrays
	// and the ball's own (alloc_own) are made, table and look-back words cleared, the root launched, then `poll` iterations (the
	// ball's four or five launches) per read of the counters until the device says done.  Whether the build passed is the ball's
	// to judge.  `nodes`: what the ball calls what it stores.
	template <typename Alloc, typename Root, typename Iteration>
	int run_build(const char *who, const char *nodes, BuildDev &d, int poll, hipStream_t st, int32_t *c, Alloc &&alloc_own, Root &&launch_root,
	              Iteration &&launch_iteration)
	{
		const size_t K = (size_t)12 * d.pops;
		pool.clear();
		int e = RK_OK;
		#define A(ptr, cnt) if (!e) e = pool.alloc(&d.ptr, (cnt))
		A(states, (cap + 1) * 5); A(table, (size_t)d.mask + 1); A(ctr, BB_COUNT);
		A(slot, K); A(rank, K); A(first, K); A(chain, frontier_scan_blocks(d.pops));
		#undef A
		if (!e) e = alloc_own();
		if (e) { (void)hipGetLastError(); pool.clear(); return fail(RK_ECAPACITY, "%s: no device memory for a ball of %zu %s", who, cap, nodes); }
		if (!ctr_host.pinned()) ctr_host.reserve(BB_COUNT);
		RK_HIP(hipMemsetAsync(d.table, 0, ((size_t)d.mask + 1) * sizeof(uint32_t), st));
		RK_HIP(hipMemsetAsync(d.chain, 0, frontier_scan_blocks(d.pops) * sizeof(unsigned long long), st));
		launch_root();
		RK_HIP(hipGetLastError());
		for (;;) {
			if (int r = ctr_host.read(d.ctr, BB_COUNT, c, st)) return r;
			if (c[BB_DONE]) break;
			for (int it = 0; it < poll; it++) launch_iteration();
			RK_HIP(hipGetLastError());
		}
		return RK_OK;
	}

	// after a build that passed: the per-batch scratch given back, the common part of the view (the level boundaries from the
	// counters) and the sizes
	template <typename View, typename... Own>
	void finish_build(BuildDev &d, const int32_t *c, View &v, Own *&... own_scratch)
	{
		for (void *p : {(void *)d.slot, (void *)d.rank, (void *)d.first, (void *)d.chain, (void *)own_scratch...}) pool.release(p);
		d.slot = nullptr; d.rank = nullptr; d.first = nullptr; d.chain = nullptr;
		((own_scratch = nullptr), ...);
		v.mask = d.mask; v.cap1 = d.cap1; v.radius = d.radius;
		v.states = d.states; v.table = d.table;
		for (int l = 0; l < (int)(sizeof v.lstart / sizeof v.lstart[0]); l++) v.lstart[l] = l <= d.radius + 1 ? c[BB_LSTART + l] : INT32_MAX;
		size = c[BB_SIZE];
		iterations = c[BB_ITERS];
		built = true;
	}

	// status words 0..4 and 6..: built, nodes, iterations, radius, capacity; the level boundaries (0 beyond radius + 1).  Word 5 is the ball's own.
	template <int N>
	void status_words(long long *o, int radius, const int32_t (&lstart)[N]) const
	{
		o[0] = built ? 1 : 0; o[1] = size; o[2] = iterations; o[3] = radius; o[4] = (long long)cap;
		for (int l = 0; l < N; l++) o[6 + l] = built && l <= radius + 1 ? lstart[l] : 0;
	}
};

// What the handle of a search that ends at a kept ball adds for that ball: the ball counts the searches that hold its arrays and
// refuses to be destroyed under them (KeptBall::check_destroy).  A handle that was never attached lets go of nothing.
template <typename Ball>
struct BallReader {
	Ball *ball = nullptr;
	BallReader() = default;
	BallReader(const BallReader &) = delete;
	BallReader &operator=(const BallReader &) = delete;
	~BallReader() { if (ball) ball->attached -= 1; }
	void attach(Ball *b) { ball = b; b->attached += 1; }
};

// the ten status words of a search that ends at a kept ball (rk_bsearch_status, a slot of rk_bsearchb_status, rk_ssearch_status)
inline void bsearch_status_words(const int32_t *c, long long *o)
{
	o[0] = c[F_DONE]; o[1] = c[F_WON]; o[2] = c[F_SIZE]; o[3] = c[F_ITERS]; o[4] = c[S_POPPED]; o[5] = c[F_STOP]; o[6] = c[F_ERROR];
	o[7] = c[F_NPOP]; o[8] = c[S_DEPTH]; o[9] = c[S_MEET];
}

// The host half of S searches in lock-step (rk_bsearchb, rk_ssearchb), as FrontierPool is of one: a block of every kind of array,
// sliced per slot, and devs[s] on the device describes slot s.  An engine's handle is this plus its ball and its own blocks; its
// entries pass their own name as `who`, the prefix of every error text, and their root, expand and walk launches.
constexpr int FRONTIER_MAX_SLOTS = 1024;

struct FrontierSlots {
	int n_slots = 0, pops = 0;
	size_t cap = 0;                             // per slot
	uint32_t mask = 0;
	FrontierDev d{};                            // slot 0: the blocks' base addresses
	FrontierDev *devs = nullptr;
	int32_t *slots_dev = nullptr, *budgets_dev = nullptr;
	uint32_t *roots_dev = nullptr;
	int32_t *walk = nullptr;
	int walk_len = 0;                           // `walk` holds n_slots rows of 1 + walk_len words
	std::vector<int32_t> ctr_spare;
	Landing ctr_host;
	DevPool pool{64};

	// the null and range checks of a *_create
	static int check_create(const char *who, const void *out, const void *ball, int n_slots, size_t capacity_per_slot, int pops)
	{
		if (!out || !ball) return fail(RK_EINVAL, "%s: null argument", who);
		if (n_slots < 1 || n_slots > FRONTIER_MAX_SLOTS) return fail(RK_EINVAL, "%s: n_slots %d outside 1..%d", who, n_slots, FRONTIER_MAX_SLOTS);
		if (capacity_per_slot < 2 || capacity_per_slot > FRONTIER_MAX_CAPACITY) return fail(RK_EINVAL, "%s: capacity %zu out of range", who, capacity_per_slot);
		if (pops < 1 || pops > FRONTIER_MAX_POPS) return fail(RK_EINVAL, "%s: pops %d outside 1..%d", who, pops, FRONTIER_MAX_POPS);
		return RK_OK;
	}

	// every block (the engine's own through alloc_own), the table of descriptors, and counters that say "never started": F_NPOP == 0,
	// every launch passes such a slot by
	template <typename Own>
	int alloc(const char *who, int slots, size_t capacity_per_slot, int pops_, Own &&alloc_own)
	{
		n_slots = slots; pops = pops_; cap = capacity_per_slot;
		mask = FrontierPool::table_mask(capacity_per_slot);
		const size_t S = (size_t)n_slots, C1 = capacity_per_slot + 1, T = (size_t)mask + 1, K = (size_t)12 * pops, W = frontier_scan_blocks(pops);
		d.pops = pops;
		d.cap1 = (uint32_t)C1;
		d.mask = mask;
		int e = RK_OK;
		#define A(ptr, cnt) if (!e) e = pool.alloc(&d.ptr, S * (cnt))
		A(states, C1 * 5); A(parent, C1); A(pact, C1); A(table, T); A(ctr, S_COUNT);
		A(slot, K); A(rank, K); A(first, K); A(chain, W);
		#undef A
		if (!e) e = pool.alloc(&devs, S);
		if (!e) e = pool.alloc(&slots_dev, S);
		if (!e) e = pool.alloc(&budgets_dev, S);
		if (!e) e = pool.alloc(&roots_dev, S * 5);
		if (!e) e = alloc_own();
		if (e) { (void)hipGetLastError(); return fail(RK_ECAPACITY, "%s: no device memory for %d pools of %zu states", who, n_slots, capacity_per_slot); }
		std::vector<FrontierDev> table(S, d);
		for (size_t s = 0; s < S; s++) {
			FrontierDev &x = table[s];
			x.states += s * C1 * 5; x.parent += s * C1; x.pact += s * C1; x.table += s * T; x.ctr += s * S_COUNT;
			x.slot += s * K; x.rank += s * K; x.first += s * K; x.chain += s * W;
		}
		hipError_t he = hipMemcpy(devs, table.data(), S * sizeof(FrontierDev), hipMemcpyHostToDevice);
		if (he == hipSuccess) he = hipMemset(d.ctr, 0, S * S_COUNT * sizeof(int32_t));
		if (he == hipSuccess) he = hipStreamSynchronize(nullptr);          // both are in place when create returns, whatever stream the first reset takes
		if (he != hipSuccess) return fail(RK_EHIP, "%s: %s", who, hipGetErrorString(he));
		ctr_host.reserve(S * S_COUNT);
		ctr_spare.resize(S * S_COUNT);
		return RK_OK;
	}

	// slot slots[j] starts again from host state j: the checks, the uploads, the named slots' own tables and look-back words
	// cleared, then the engine's root launch over the n named slots
	template <typename Root>
	int reset(const char *who, bool ball_built, int n, const int32_t *slots, const int8_t *h_start_states, const long long *max_states, hipStream_t st,
	          Root &&launch_root)
	{
		if (!ball_built) return fail(RK_ESTATE, "%s: build the ball first", who);
		if (n < 0 || n > n_slots) return fail(RK_EINVAL, "%s: %d slots of %d", who, n, n_slots);
		if (n == 0) return RK_OK;
		if (!slots || !h_start_states || !max_states) return fail(RK_EINVAL, "%s: null argument", who);
		std::vector<char> named((size_t)n_slots, 0);
		std::vector<int32_t> budgets((size_t)n);
		for (int j = 0; j < n; j++) {
			if (slots[j] < 0 || slots[j] >= n_slots) return fail(RK_EINVAL, "%s: slot %d outside 0..%d", who, slots[j], n_slots - 1);
			if (named[slots[j]]) return fail(RK_EINVAL, "%s: slot %d is named twice", who, slots[j]);
			named[slots[j]] = 1;
			budgets[j] = budget_of(max_states[j]);
		}
		RK_HIP(hipMemcpyAsync(slots_dev, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
		RK_HIP(hipMemcpyAsync(budgets_dev, budgets.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
		RK_HIP(hipMemcpyAsync(roots_dev, h_start_states, (size_t)n * STATE_BYTES, hipMemcpyHostToDevice, st));
		const unsigned gx = std::min<unsigned>(blocks(((size_t)mask + 1) / 4), 1024u);
		hipLaunchKernelGGL(kb_srch_clear, dim3(gx, n), dim3(256), 0, st, devs, slots_dev, (int)frontier_scan_blocks(pops));   // the named slots' own tables only
		launch_root();
		RK_HIP(hipGetLastError());
		RK_HIP(hipStreamSynchronize(st));       // the host buffers may go away after return
		return RK_OK;
	}

	// `iterations` lock-step iterations of every slot: the engine's expand launch(es) on a grid of (workgroups of 256 over 12 x
	// pops children, n_slots), then scan, append and end with the slot in the grid's second dimension
	template <typename Expand>
	int run(const char *who, bool ball_built, int iterations, hipStream_t st, Expand &&launch_expand)
	{
		if (!ball_built) return fail(RK_ESTATE, "%s: build the ball first", who);
		if (iterations < 0) return fail(RK_EINVAL, "%s: iterations %d < 0", who, iterations);
		const size_t K = (size_t)12 * pops;
		const dim3 grid(blocks(K), n_slots), grid_scan(blocks(K, ASCAN), n_slots);
		for (int it = 0; it < iterations; it++) {
			launch_expand(grid);
			hipLaunchKernelGGL(kb_srch_scan, grid_scan, dim3(ASCAN), 0, st, devs);
			hipLaunchKernelGGL(kb_srch_append, grid, dim3(256), 0, st, devs);
			hipLaunchKernelGGL(kb_srch_end, dim3(1, n_slots), dim3(64), 0, st, devs);
		}
		RK_HIP(hipGetLastError());
		return RK_OK;
	}

	// bsearch_status_words of every slot, the counters read with one copy
	int status(long long *h_status, hipStream_t st)
	{
		const int32_t *c = nullptr;
		if (int e = ctr_host.fetch(d.ctr, (size_t)n_slots * S_COUNT, ctr_spare.data(), st, &c)) return e;
		for (int s = 0; s < n_slots; s++, c += S_COUNT)
			bsearch_status_words(c, h_status + (size_t)s * 10);
		return RK_OK;
	}

	// the engine's walk launch into the first `rows` rows of 1 + max_len words of `walk` (n_slots of them), then one copy to h_out
	template <typename Walk>
	int paths(const char *who, bool ball_built, int32_t *h_out, int max_len, hipStream_t st, Walk &&launch_walk, int rows = -1)
	{
		if (!ball_built) return fail(RK_ESTATE, "%s: build the ball first", who);
		if (max_len < 0 || max_len > FRONTIER_WALK_MAX) return fail(RK_EINVAL, "%s: max_len %d outside 0..%d", who, max_len, FRONTIER_WALK_MAX);
		const size_t words = (size_t)n_slots * (size_t)(1 + max_len);
		if (walk == nullptr || walk_len < max_len) {
			RK_HIP(hipStreamSynchronize(st));
			if (walk != nullptr) { pool.release(walk); walk = nullptr; }
			if (pool.alloc(&walk, words) != RK_OK) { (void)hipGetLastError(); return fail(RK_ECAPACITY, "%s: no device memory for %zu words", who, words); }
			walk_len = max_len;
		}
		launch_walk();
		RK_HIP(hipGetLastError());
		RK_HIP(hipMemcpyAsync(h_out, walk, (rows < 0 ? words : (size_t)rows * (size_t)(1 + max_len)) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
		RK_HIP(hipStreamSynchronize(st));
		return RK_OK;
	}

	int export_rows(const char *who, int slot, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions, hipStream_t st)
	{
		if (slot < 0 || slot >= n_slots) return fail(RK_EINVAL, "%s: slot %d outside 0..%d", who, slot, n_slots - 1);
		if (first + count > cap + 1) return fail(RK_EINVAL, "%s: rows %zu..%zu outside the pool", who, first, first + count);
		const size_t at = (size_t)slot * (cap + 1);
		return export_pool_rows(d.states + at * 5, d.parent + at, d.pact + at, first, count, h_states, h_parents, h_actions, nullptr, st);
	}
};

}  // namespace
}  // namespace rk
