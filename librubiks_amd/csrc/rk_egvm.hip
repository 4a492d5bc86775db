// Device-resident epsilon-greedy value maximisation (reference: librubiks/solving/agents.py:649-726), sync-free between polls.
//
// What lives in HBM (W walkers, D moves per walk, a window of R rounds of draws and records):
//   root    5 x u32           the state every walker of the round starts from                        (`state`, :667, :675)
//   cur     5 x u32 (W)       where every walker stands                                              (`states`, :686, :707)
//   visited 5 x u32 (W D)     row w D + d = walker w after d + 1 moves                               (`new_states`, :714)
//   paths   uint8 (W, D)      the action of every move                                               (`paths`, :703)
//   draws   int8 (R, D, W)    the action 0..11 where the reference acts at random (:698), -1 where it follows the policy
//   rec     int32 (R, D + 2)  per closed round: number of actions, 1 if the round ended by a solve, the actions (:670, :677)
//   ctr     int32[16] + two int64 (explored, max_states)
//   the two net batches: W rows for the policy forward, W D rows for the value forward, as one-hot rows of the net's dtype
//   or as the 20-byte states themselves
// The epsilon draws depend on nothing the device computes, so the host makes them in the reference's order (:694, :698) and
// uploads a window of rounds; everything else of a round runs here:
//   k_egvm_step        one launch per move, one wave per walker: the drawn action or the first maximum of the walker's 12 logits
//                      (ndarray.argmax, :701), the move, the goal test (:709), visited / paths, and the walker's row of the next
//                      policy batch and of the value batch (:708, :715).  A solved walker reports d W + w with one atomicMin: the
//                      reference returns at the first depth with a solved walker, and there the lowest one (:710-713).
//   k_egvm_round_end   one launch per round, one workgroup: either the solve -- its path, explored += (d + 1) W (:711), done -- or
//                      the first maximum over the W D values (torch.argmax on the CPU, :674), the new root, its path (:677),
//                      explored += W D (:716), the loop guard of :665, and the start of the next round.
// After the search is done, and after a round has a solved walker, both kernels do nothing.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"

namespace rk {

enum { E_DONE = 0, E_SOLVED, E_ROUND, E_DEPTH, E_WIN, E_TICKET, E_ERROR, E_BASE, E_NDRAW, E_SWALKER, E_SDEPTH, E_COUNT = 16 };
enum { E_BIG_EXPLORED = 0, E_BIG_MAX = 1 };
enum { EGVM_ERR_NONE = 0, EGVM_ERR_DRAWS = 1, EGVM_ERR_WALK = 2 };   // a round beyond the uploaded draws; a round closed before its walk ended

constexpr uint32_t EGVM_NO_WIN = 0x7FFFFFFFu;
constexpr int EGVM_WORDS = E_COUNT + 4;          // the counters, then two int64

struct EgvmDev {
	int W, D, R;
	int code;                                   // RK_OH_* form of the two net batches
	uint32_t *root, *cur, *visited;
	uint8_t *paths;
	int8_t *draws;
	int32_t *rec;
	int32_t *ctr;
	void *pol_in, *val_in;
};

__device__ __forceinline__ long long *egvm_big(const EgvmDev &d) { return reinterpret_cast<long long *>(d.ctr + E_COUNT); }

// The start of a round, by one workgroup: every walker on `from`, and its row of the policy batch.
__device__ __forceinline__ void egvm_restart(const EgvmDev &d, const uint32_t *from)
{
	uint32_t s[5];
	load5(from, s);
	for (int q = threadIdx.x; q < d.W * 5; q += blockDim.x) d.cur[q] = dword_of(s, q % 5);
	for (int w = threadIdx.x >> 6; w < d.W; w += blockDim.x >> 6)      // one wave per row
		write_row(d.pol_in, d.code, (size_t)w, s, threadIdx.x & 63, 64);
}

__global__ __launch_bounds__(1024)
void k_egvm_begin(EgvmDev d, const uint32_t *root_in, long long max_states)
{
	const int tid = threadIdx.x;
	if (tid < E_COUNT) d.ctr[tid] = tid == E_WIN ? (int32_t)EGVM_NO_WIN : 0;
	if (tid == 0) {
		long long *big = egvm_big(d);
		big[E_BIG_EXPLORED] = 0;
		big[E_BIG_MAX] = max_states;
		if ((long long)d.W * d.D > max_states) d.ctr[E_DONE] = 1;          // the loop guard of agents.py:665 fails at once
	}
	if (tid < 5) d.root[tid] = root_in[tid];
	egvm_restart(d, root_in);
}

// the draws of the rounds that follow: round ctr[E_ROUND] is slot 0 of the window
__global__ void k_egvm_window(EgvmDev d, int rounds)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	d.ctr[E_BASE] = d.ctr[E_ROUND];
	d.ctr[E_NDRAW] = rounds;
}

// one move of every walker: one wave per walker, four walkers per workgroup                        agents.py:692-715
__global__ __launch_bounds__(256)
void k_egvm_step(EgvmDev d, const void *logits, int bf16)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	// Nothing below changes what these reads return while the launch runs: the depth moves on only after every workgroup has drawn
	// its ticket, and a walker that solves at this depth leaves win / W == depth.
	const int depth = d.ctr[E_DEPTH];
	const uint32_t win = (uint32_t)d.ctr[E_WIN];
	const int slot = d.ctr[E_ROUND] - d.ctr[E_BASE];
	const bool idle = d.ctr[E_DONE] || d.ctr[E_ERROR] || depth >= d.D || (win != EGVM_NO_WIN && (int)(win / (uint32_t)d.W) < depth);
	const int ndraw = d.ctr[E_NDRAW];
	__syncthreads();
	if (idle) return;
	if (slot < 0 || slot >= ndraw) {
		if (blockIdx.x == 0 && threadIdx.x == 0) d.ctr[E_ERROR] = EGVM_ERR_DRAWS;
		return;
	}
	const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (w < d.W) {
		int a = d.draws[((size_t)slot * d.D + depth) * d.W + w];
		if (a < 0) {                                                        // p.argmax(axis=1)   agents.py:701
			float bv = net_out(logits, bf16 != 0, (size_t)w * 12);
			a = 0;
			#pragma unroll
			for (int k = 1; k < 12; k++) {
				const float v = net_out(logits, bf16 != 0, (size_t)w * 12 + k);
				if (beats(v, k, bv, a)) { bv = v; a = k; }
			}
		}
		uint32_t s[5], tab[12];
		load5(d.cur + (size_t)w * 5, s);
		load_action_table(s_act, (uint32_t)a, tab);
		move5(s, tab);                                                      // :706-707
		const size_t row = (size_t)w * d.D + depth;
		if (lane < 5) {
			d.cur[(size_t)w * 5 + lane] = dword_of(s, lane);
			d.visited[row * 5 + lane] = dword_of(s, lane);                  // :714
		}
		if (lane == 0) {
			d.paths[row] = (uint8_t)a;                                      // :703
			if (is_solved5(s)) atomicMin(reinterpret_cast<uint32_t *>(&d.ctr[E_WIN]), (uint32_t)depth * (uint32_t)d.W + (uint32_t)w);   // :709-713
		}
		write_row(d.pol_in, d.code, (size_t)w, s, lane, 64);                // :708
		write_row(d.val_in, d.code, row, s, lane, 64);                      // :715
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		__threadfence();
		if (atomicAdd(&d.ctr[E_TICKET], 1) == (int)gridDim.x - 1) {        // the last workgroup of the launch: the walk is one move deeper
			d.ctr[E_TICKET] = 0;
			d.ctr[E_DEPTH] = depth + 1;
		}
	}
}

// closes a round; one workgroup                                                                     agents.py:665-677
__global__ __launch_bounds__(1024)
void k_egvm_round_end(EgvmDev d, const void *values, int bf16)
{
	__shared__ float s_v[16];
	__shared__ int s_i[16];
	__shared__ int s_best;
	const int tid = threadIdx.x, W = d.W, D = d.D;
	const int done = d.ctr[E_DONE], err = d.ctr[E_ERROR], depth = d.ctr[E_DEPTH], round = d.ctr[E_ROUND];
	const uint32_t win = (uint32_t)d.ctr[E_WIN];
	const int slot = round - d.ctr[E_BASE], ndraw = d.ctr[E_NDRAW];
	__syncthreads();                                                        // every thread has read the counters before one is written
	if (done) return;
	const bool won = win != EGVM_NO_WIN;
	if (err || slot < 0 || slot >= ndraw || (!won && depth != D)) {
		if (tid == 0) {
			if (!err) d.ctr[E_ERROR] = slot < 0 || slot >= ndraw ? EGVM_ERR_DRAWS : EGVM_ERR_WALK;
			d.ctr[E_DONE] = 1;
		}
		return;
	}
	long long *big = egvm_big(d);
	int32_t *rec = d.rec + (size_t)slot * (D + 2);
	if (won) {                                                              // :669-671, :711-713
		const int w = (int)(win % (uint32_t)W), n = (int)(win / (uint32_t)W) + 1;
		for (int k = tid; k < n; k += blockDim.x) rec[2 + k] = d.paths[(size_t)w * D + k];
		if (tid == 0) {
			rec[0] = n; rec[1] = 1;
			big[E_BIG_EXPLORED] += (long long)n * W;
			d.ctr[E_SWALKER] = w; d.ctr[E_SDEPTH] = n;
			d.ctr[E_ROUND] = round + 1;
			d.ctr[E_SOLVED] = 1; d.ctr[E_DONE] = 1;
		}
		return;
	}
	// int(v.argmax())   :674 -- every thread walks its indices upwards, so a later equal value never replaces an earlier one
	const int N = W * D;
	float bv = 0.0f;
	int bi = INT_MAX;
	for (int i = tid; i < N; i += blockDim.x) {
		const float v = net_out(values, bf16 != 0, (size_t)i);
		if (bi == INT_MAX || beats(v, i, bv, bi)) { bv = v; bi = i; }
	}
	#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		const float ov = __shfl_down(bv, off, 64);
		const int oi = __shfl_down(bi, off, 64);
		if (oi != INT_MAX && (bi == INT_MAX || beats(ov, oi, bv, bi))) { bv = ov; bi = oi; }
	}
	if ((tid & 63) == 0) { s_v[tid >> 6] = bv; s_i[tid >> 6] = bi; }
	__syncthreads();
	if (tid == 0) {
		for (int k = 1; k < (int)(blockDim.x >> 6); k++)
			if (s_i[k] != INT_MAX && (bi == INT_MAX || beats(s_v[k], s_i[k], bv, bi))) { bv = s_v[k]; bi = s_i[k]; }
		s_best = bi;
	}
	__syncthreads();
	const int best = s_best, bw = best / D, bd = best - bw * D;             // :676
	for (int k = tid; k <= bd; k += blockDim.x) rec[2 + k] = d.paths[(size_t)bw * D + k];                  // :677
	const uint32_t *from = d.visited + (size_t)best * 5;
	if (tid < 5) d.root[tid] = from[tid];                                   // :675
	const long long explored = big[E_BIG_EXPLORED] + N;                     // :716 (thread 0 writes it below, after everyone has read it)
	const bool last = explored + N > big[E_BIG_MAX];                        // :665
	__syncthreads();
	if (tid == 0) {
		rec[0] = bd + 1; rec[1] = 0;
		big[E_BIG_EXPLORED] = explored;
		d.ctr[E_ROUND] = round + 1;
		d.ctr[E_DEPTH] = 0;
		d.ctr[E_TICKET] = 0;
		if (last) d.ctr[E_DONE] = 1;
	}
	if (!last) egvm_restart(d, from);
}

}  // namespace rk

using namespace rk;

struct rk_egvm {
	EgvmDev d{};
	uint32_t *root_dev = nullptr;
	// zeroed: a round that ends by a solve leaves value rows unwritten, and the value forward of that round still reads them
	NetBatches pol{true}, val{true};
	Landing ctr_host;
	bool ready = false;
	DevPool pool{64};
};

namespace {

constexpr int EGVM_MAX_WORKERS = 1 << 16, EGVM_MAX_DEPTH = 1 << 12, EGVM_MAX_ROUNDS = 1 << 12;
constexpr long long EGVM_MAX_STATES = 1ll << 22, EGVM_MAX_DRAWS = 1ll << 28;

int egvm_read(rk_egvm *h, int32_t *out, hipStream_t st) { return h->ctr_host.read(h->d.ctr, EGVM_WORDS, out, st); }

}  // namespace

extern "C" {

int rk_egvm_create(rk_egvm_t **out, int workers, int depth, int burst_rounds)
{
	if (!out) return fail(RK_EINVAL, "rk_egvm_create: null out pointer");
	if (workers < 1 || workers > EGVM_MAX_WORKERS) return fail(RK_EINVAL, "rk_egvm_create: workers %d outside 1..%d", workers, EGVM_MAX_WORKERS);
	if (depth < 1 || depth > EGVM_MAX_DEPTH) return fail(RK_EINVAL, "rk_egvm_create: depth %d outside 1..%d", depth, EGVM_MAX_DEPTH);
	if (burst_rounds < 1 || burst_rounds > EGVM_MAX_ROUNDS) return fail(RK_EINVAL, "rk_egvm_create: burst_rounds %d outside 1..%d", burst_rounds, EGVM_MAX_ROUNDS);
	const long long N = (long long)workers * depth;
	if (N > EGVM_MAX_STATES) return fail(RK_EINVAL, "rk_egvm_create: workers * depth = %lld above %lld", N, EGVM_MAX_STATES);
	if (N * burst_rounds > EGVM_MAX_DRAWS) return fail(RK_EINVAL, "rk_egvm_create: workers * depth * burst_rounds = %lld above %lld", N * burst_rounds, EGVM_MAX_DRAWS);
	rk_egvm *h = new rk_egvm();
	EgvmDev &d = h->d;
	d.W = workers; d.D = depth; d.R = burst_rounds;
	d.code = -1;
	int e = RK_OK;
	#define A(ptr, cnt) if (!e) e = h->pool.alloc(&d.ptr, (cnt))
	A(root, 8); A(cur, (size_t)workers * 5); A(visited, (size_t)N * 5); A(paths, (size_t)N); A(draws, (size_t)N * burst_rounds);
	A(rec, (size_t)burst_rounds * (depth + 2)); A(ctr, EGVM_WORDS);
	#undef A
	if (!e) e = h->pool.alloc(&h->root_dev, 8);
	if (!e) h->ctr_host.reserve(EGVM_WORDS);
	if (e) { rk_egvm_destroy(h); return e; }
	*out = h;
	return RK_OK;
}

int rk_egvm_destroy(rk_egvm_t *h)
{
	delete h;                                   // the pool and the landing buffer go with it
	return RK_OK;
}

int rk_egvm_net_in(rk_egvm_t *h, int which, int out_dtype, void **d_ptr, size_t *rows)
{
	if (!h || !d_ptr || !rows) return fail(RK_EINVAL, "rk_egvm_net_in: null argument");
	if (which != 0 && which != 1) return fail(RK_EINVAL, "rk_egvm_net_in: which is 0 (policy batch) or 1 (value batch), got %d", which);
	if (out_dtype < RK_OH_F32 || out_dtype > RK_OH_STATES) return fail(RK_EINVAL, "rk_egvm_net_in: unknown dtype %d", out_dtype);
	EgvmDev &d = h->d;
	const size_t nw = (size_t)d.W, nv = (size_t)d.W * d.D;
	void *p = nullptr, *v = nullptr;                // both batches of a form or neither
	if (int e = h->pol.get(h->pool, out_dtype, nw, &p)) return e;
	if (int e = h->val.get(h->pool, out_dtype, nv, &v)) { h->pol.drop(h->pool, out_dtype); return e; }
	if (d.code != out_dtype) h->ready = false;  // the batches of a running search are in the other form: reset first
	d.code = out_dtype;
	d.pol_in = p; d.val_in = v;
	*d_ptr = which == 0 ? d.pol_in : d.val_in;
	*rows = which == 0 ? nw : nv;
	return RK_OK;
}

int rk_egvm_reset(rk_egvm_t *h, const int8_t *h_root, long long max_states, void *stream)
{
	if (!h || !h_root) return fail(RK_EINVAL, "rk_egvm_reset: null argument");
	if (h->d.code < 0) return fail(RK_ESTATE, "rk_egvm_reset: ask for the net batches first (rk_egvm_net_in)");
	if (int e = check_cubie_codes("rk_egvm_reset", "root", h_root, 1)) return e;
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemcpyAsync(h->root_dev, h_root, STATE_BYTES, hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(k_egvm_begin, dim3(1), dim3(1024), 0, st, h->d, h->root_dev, std::max<long long>(max_states, 0));
	RK_HIP(hipGetLastError());
	RK_HIP(hipStreamSynchronize(st));       // the host buffer may go away after return
	h->ready = true;
	return RK_OK;
}

int rk_egvm_set_draws(rk_egvm_t *h, const int8_t *h_draws, int rounds, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_egvm_set_draws: reset the engine first");
	if (!h_draws) return fail(RK_EINVAL, "rk_egvm_set_draws: null draws");
	const EgvmDev &d = h->d;
	if (rounds < 1 || rounds > d.R) return fail(RK_EINVAL, "rk_egvm_set_draws: rounds %d outside 1..%d", rounds, d.R);
	const size_t n = (size_t)rounds * d.D * d.W;
	for (size_t i = 0; i < n; i++)
		if (h_draws[i] < -1 || h_draws[i] >= N_ACTIONS) return fail(RK_EINVAL, "rk_egvm_set_draws: draw %zu is %d, outside -1..11", i, (int)h_draws[i]);
	hipStream_t st = (hipStream_t)stream;
	RK_HIP(hipMemcpyAsync(d.draws, h_draws, n, hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(k_egvm_window, dim3(1), dim3(64), 0, st, d, rounds);
	RK_HIP(hipGetLastError());
	RK_HIP(hipStreamSynchronize(st));       // the host buffer may go away after return
	return RK_OK;
}

int rk_egvm_step(rk_egvm_t *h, const void *d_logits, int dtype, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_egvm_step: reset the engine first");
	int bf16 = 0;
	if (int e = check_net_out("rk_egvm_step", d_logits, dtype, &bf16)) return e;
	hipLaunchKernelGGL(k_egvm_step, dim3(blocks((size_t)h->d.W, 4)), dim3(256), 0, (hipStream_t)stream, h->d, d_logits, bf16);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_egvm_round_end(rk_egvm_t *h, const void *d_values, int dtype, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_egvm_round_end: reset the engine first");
	int bf16 = 0;
	if (int e = check_net_out("rk_egvm_round_end", d_values, dtype, &bf16)) return e;
	hipLaunchKernelGGL(k_egvm_round_end, dim3(1), dim3(1024), 0, (hipStream_t)stream, h->d, d_values, bf16);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_egvm_status(rk_egvm_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_egvm_status: bad argument");
	int32_t c[EGVM_WORDS];
	if (int e = egvm_read(h, c, (hipStream_t)stream)) return e;
	h_status[0] = c[E_DONE]; h_status[1] = c[E_SOLVED]; h_status[2] = c[E_ROUND]; h_status[3] = ctr64(c, E_COUNT + 2 * E_BIG_EXPLORED);
	h_status[4] = c[E_SOLVED] ? c[E_SWALKER] : -1; h_status[5] = c[E_SOLVED] ? c[E_SDEPTH] : -1; h_status[6] = c[E_ERROR]; h_status[7] = c[E_BASE];
	return RK_OK;
}

int rk_egvm_records(rk_egvm_t *h, long long first_round, int rounds, long long *h_out, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_egvm_records: reset the engine first");
	if (rounds < 0 || (rounds > 0 && !h_out)) return fail(RK_EINVAL, "rk_egvm_records: bad argument");
	if (rounds == 0) return RK_OK;
	hipStream_t st = (hipStream_t)stream;
	int32_t c[EGVM_WORDS];
	if (int e = egvm_read(h, c, st)) return e;
	const EgvmDev &d = h->d;
	const long long lo = c[E_BASE], hi = std::min<long long>(c[E_ROUND], lo + c[E_NDRAW]);
	if (first_round < lo || first_round + rounds > hi)
		return fail(RK_EINVAL, "rk_egvm_records: rounds %lld..%lld are not the closed rounds of the window, %lld..%lld", first_round, first_round + rounds, lo, hi);
	return export_widened(d.rec + (size_t)(first_round - lo) * (d.D + 2), (size_t)rounds * (d.D + 2), h_out, st);
}

}  // extern "C"
