// Device-resident greedy one-step games (reference: librubiks/solving/agents.py:132-169, the loop of :22-38 around them), G independent
// games advanced in lock-step, sync-free between polls.
//
// What lives in HBM (G games, at most S moves per game):
//   cur     5 x u32 (G)       the state every game stands on                                           (`state` of :31)
//   status  int32 (G)         0 running, 1 solved, 2 budget spent, 3 handed back to the host
//   steps   int32 (G)         moves made                                                               (len(self.action_queue), :32)
//   actions uint8 (G, S)      the action of every move                                                 (`action_queue`, :32)
//   ctr     int32[8]          running games, moves launched, error, and what the last reset fixed: games played, moves per game
//   the net batch: G rows (policy mode: where every game stands) or 12 G rows (value mode: row 12 g + a = child a of game g's
//   state), as one-hot rows of the net's dtype or as the 20-byte states themselves
// One launch per move (k_greedy_step), one wave per game, no wave depends on another:
//   policy mode   the first maximum of the game's 12 logits -- unless the host's argmax(softmax(logits)) (:139-140) might choose
//                 otherwise, see TIE_GAP --, the move, the goal test (:141-142), and the game's row of the next batch
//   value mode    the 12 children and their goal tests again (:157-158); the first solved child (:159-161) or the first maximum of
//                 the 12 values, NaN counting as the maximum (ndarray.argmax, :165); the 12 children of the new state as the next batch
// and in both the action record, the move count and the budget: this repository's Agent.search counts a game's moves against
// max_states before every step, so a game that is not solved after max_states moves ends with status 2.  Games that are not
// running are skipped and their rows of the batch stay as they are, so the net's batch never changes shape.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"
#include "rk_search_dev.h"
#include "rk_search_host.h"

namespace rk {

enum { Y_RUNNING = 0, Y_LAUNCHES, Y_ERROR, Y_GAMES, Y_BUDGET, Y_COUNT = 8 };
enum { GREEDY_POLICY = 0, GREEDY_VALUE = 1 };
enum { GAME_RUNNING = 0, GAME_SOLVED = 1, GAME_SPENT = 2, GAME_HANDED_BACK = 3 };
enum { GREEDY_ERR_NONE = 0, GREEDY_ERR_RECORD = 1 };     // a running game whose next move has no place in the action record

// Policy mode takes argmax(logits) where the host agent takes argmax(softmax(logits)) on the CPU.  The two can differ only when a
// smaller logit x_k at a LOWER index rounds to the same probability as the maximum m.  With d = m - x_k (float32) >= 2^-20:
//   * exp(x_k - m) <= exp(-2^-20) < 1 - 2^-20 + 2^-41, and float32 numbers just below 1 are 2^-24 apart, so an exp that is up to
//     eight ulp off still returns at most 1 - 2^-21; the maximum's own numerator is exp(0) = 1 exactly;
//   * a relative gap of 2^-21 between two numerators survives one rounded division by the same sum (a relative error of at most
//     2^-24 each), and equally one rounded multiplication by the sum's rounded reciprocal r: fl(1 r) = r, and
//     fl(e_k r) <= r (1 - 2^-21) (1 + 2^-24) < r.  The sum is between 1 and 12, so nothing is subnormal.
// So the maximum logit's probability is strictly the largest, and exact ties (d = 0) resolve to the first index either way.  A game
// with 0 < d < 2^-20 for some k is not moved: it gets status 3 and the host plays it.  So does a game whose d is NaN for some k -- a
// NaN logit, or an infinite maximum, for which the softmax is NaN in every place.
constexpr float TIE_GAP = 0x1p-20f;

struct GreedyDev {
	int G, S, mode;
	int code;                                   // RK_OH_* form of the net batch
	uint32_t *cur;
	int32_t *status, *steps;
	uint8_t *actions;
	int32_t *ctr;
	void *net_in;
};

// value mode: the 12 children of s as rows 12 g .. 12 g + 11 of the batch, by the 64 lanes of the game's wave        agents.py:157, :163
__device__ __forceinline__ void greedy_write_children(const GreedyDev &d, const u32x4 *s_act, int g, const uint32_t s[5], int lane)
{
	for (uint32_t c = 0; c < 12; c++) {
		uint32_t child[5] = {s[0], s[1], s[2], s[3], s[4]}, tab[12];
		load_action_table(s_act, c, tab);
		move5(child, tab);
		write_row(d.net_in, d.code, (size_t)g * 12 + c, child, lane, 64);
	}
}

// a game leaves the running ones (lane 0 of its wave)
__device__ __forceinline__ void greedy_end(const GreedyDev &d, int g, int status)
{
	d.status[g] = status;
	atomicSub(&d.ctr[Y_RUNNING], 1);
}

// the games of a search: one wave per game, four games per workgroup
__global__ __launch_bounds__(256)
void k_greedy_begin(GreedyDev d, const uint32_t *roots, int n_games, int budget)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	__syncthreads();
	if (blockIdx.x == 0 && threadIdx.x == 0) { d.ctr[Y_GAMES] = n_games; d.ctr[Y_BUDGET] = budget; }
	const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (g >= d.G) return;
	if (g >= n_games) {                                                     // not played: idle until the next reset
		if (lane == 0) { d.status[g] = GAME_HANDED_BACK; d.steps[g] = 0; }
		return;
	}
	uint32_t s[5];
	load5(roots + (size_t)g * 5, s);
	const bool solved = is_solved5(s);                                      // Agent.search returns before its loop (:29)
	if (lane < 5) d.cur[(size_t)g * 5 + lane] = dword_of(s, lane);
	if (lane == 0) {
		d.status[g] = solved ? GAME_SOLVED : GAME_RUNNING;
		d.steps[g] = 0;
		if (!solved) atomicAdd(&d.ctr[Y_RUNNING], 1);
	}
	if (d.mode == GREEDY_POLICY) write_row(d.net_in, d.code, (size_t)g, s, lane, 64);
	else greedy_write_children(d, s_act, g, s, lane);
}

// one move of every running game: one wave per game, four games per workgroup                       agents.py:30-35 around :138-142 / :156-166
__global__ __launch_bounds__(256)
void k_greedy_step(GreedyDev d, const void *out, int bf16)
{
	__shared__ u32x4 s_act[36];
	stage_action_tables(s_act, threadIdx.x);
	const int n_games = d.ctr[Y_GAMES], budget = d.ctr[Y_BUDGET];           // no launch of this kernel writes them
	__syncthreads();
	if (blockIdx.x == 0 && threadIdx.x == 0) d.ctr[Y_LAUNCHES] += 1;        // the only writer of this word
	const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (g >= d.G || g >= n_games) return;
	if (d.status[g] != GAME_RUNNING) return;
	const int steps = d.steps[g];
	if (steps < 0 || steps >= budget || budget > d.S) {                     // never write outside the action record
		if (lane == 0) d.ctr[Y_ERROR] = GREEDY_ERR_RECORD;
		return;
	}
	uint32_t s[5], tab[12];
	load5(d.cur + (size_t)g * 5, s);
	int a = 0;
	bool solved = false;
	if (d.mode == GREEDY_POLICY) {
		float m = net_out(out, bf16 != 0, (size_t)g * 12);
		#pragma unroll
		for (int k = 1; k < 12; k++) {
			const float v = net_out(out, bf16 != 0, (size_t)g * 12 + k);
			if (beats(v, k, m, a)) { m = v; a = k; }
		}
		bool unsure = false;                                                // see TIE_GAP
		#pragma unroll
		for (int k = 0; k < 12; k++) {
			const float gap = m - net_out(out, bf16 != 0, (size_t)g * 12 + k);
			unsure |= !(gap == 0.0f || gap >= TIE_GAP);
		}
		if (unsure) {
			if (lane == 0) greedy_end(d, g, GAME_HANDED_BACK);
			return;
		}
		load_action_table(s_act, (uint32_t)a, tab);
		move5(s, tab);                                                      // :141
		solved = is_solved5(s);                                             // :142
	} else {
		uint32_t child[5] = {s[0], s[1], s[2], s[3], s[4]};                 // lane a < 12 holds child a (:157)
		load_action_table(s_act, lane < 12 ? (uint32_t)lane : 0u, tab);
		move5(child, tab);
		const unsigned long long won = __ballot(lane < 12 && is_solved5(child));       // :158
		if (won != 0ull) {                                                  // np.where(solutions)[0][0]   :159-161
			a = __ffsll(won) - 1;
			solved = true;
		} else {                                                            // np.argmax(v)   :165
			float bv = net_out(out, bf16 != 0, (size_t)g * 12);
			#pragma unroll
			for (int k = 1; k < 12; k++) {
				const float v = net_out(out, bf16 != 0, (size_t)g * 12 + k);
				if (beats(v, k, bv, a)) { bv = v; a = k; }
			}
		}
		load_action_table(s_act, (uint32_t)a, tab);
		move5(s, tab);
	}
	const bool spent = !solved && steps + 1 >= budget;                      // `len(self) < max_states` before the next step
	if (lane < 5) d.cur[(size_t)g * 5 + lane] = dword_of(s, lane);
	if (lane == 0) {
		d.actions[(size_t)g * d.S + steps] = (uint8_t)a;                    // :32
		d.steps[g] = steps + 1;
		if (solved || spent) greedy_end(d, g, solved ? GAME_SOLVED : GAME_SPENT);
	}
	if (solved || spent) return;                                            // no forward of this game is read again
	if (d.mode == GREEDY_POLICY) write_row(d.net_in, d.code, (size_t)g, s, lane, 64);
	else greedy_write_children(d, s_act, g, s, lane);
}

}  // namespace rk

using namespace rk;

struct rk_greedy {
	GreedyDev d{};
	uint32_t *roots_dev = nullptr;
	// zeroed: the rows of games that an engine made for G does not play are read by every forward and never written
	NetBatches batch{true};
	Landing ctr_host;
	int n_games = 0, budget = 0;                                // of the last reset
	bool ready = false;
	DevPool pool{64};
};

namespace {

constexpr int GREEDY_MAX_GAMES = 1 << 16;
constexpr long long GREEDY_MAX_RECORD = 1ll << 30;

}  // namespace

extern "C" {

int rk_greedy_create(rk_greedy_t **out, int games, int max_steps, int mode)
{
	if (!out) return fail(RK_EINVAL, "rk_greedy_create: null out pointer");
	if (games < 1 || games > GREEDY_MAX_GAMES) return fail(RK_EINVAL, "rk_greedy_create: games %d outside 1..%d", games, GREEDY_MAX_GAMES);
	if (max_steps < 1) return fail(RK_EINVAL, "rk_greedy_create: max_steps %d below 1", max_steps);
	if (mode != GREEDY_POLICY && mode != GREEDY_VALUE) return fail(RK_EINVAL, "rk_greedy_create: mode is 0 (policy) or 1 (value), got %d", mode);
	const long long N = (long long)games * max_steps;
	if (N > GREEDY_MAX_RECORD) return fail(RK_EINVAL, "rk_greedy_create: games * max_steps = %lld above %lld", N, GREEDY_MAX_RECORD);
	rk_greedy *h = new rk_greedy();
	GreedyDev &d = h->d;
	d.G = games; d.S = max_steps; d.mode = mode;
	d.code = -1;
	int e = RK_OK;
	#define A(ptr, cnt) if (!e) e = h->pool.alloc(&d.ptr, (cnt))
	A(cur, (size_t)games * 5); A(status, (size_t)games); A(steps, (size_t)games); A(actions, (size_t)N); A(ctr, Y_COUNT);
	#undef A
	if (!e) e = h->pool.alloc(&h->roots_dev, (size_t)games * 5);
	if (!e) h->ctr_host.reserve(Y_COUNT);
	if (e) { rk_greedy_destroy(h); return e; }
	*out = h;
	return RK_OK;
}

int rk_greedy_destroy(rk_greedy_t *h)
{
	delete h;                                   // the pool and the landing buffer go with it
	return RK_OK;
}

int rk_greedy_net_in(rk_greedy_t *h, int out_dtype, void **d_ptr, size_t *rows)
{
	if (!h || !d_ptr || !rows) return fail(RK_EINVAL, "rk_greedy_net_in: null argument");
	if (out_dtype < RK_OH_F32 || out_dtype > RK_OH_STATES) return fail(RK_EINVAL, "rk_greedy_net_in: unknown dtype %d", out_dtype);
	GreedyDev &d = h->d;
	const size_t n = (size_t)d.G * (d.mode == GREEDY_VALUE ? 12 : 1);
	if (int e = h->batch.get(h->pool, out_dtype, n, &d.net_in)) return e;
	if (d.code != out_dtype) h->ready = false;  // the batch of a running search is in the other form: reset first
	d.code = out_dtype;
	*d_ptr = d.net_in;
	*rows = n;
	return RK_OK;
}

int rk_greedy_reset(rk_greedy_t *h, const int8_t *h_roots, int n_games, int max_states, void *stream)
{
	if (!h || !h_roots) return fail(RK_EINVAL, "rk_greedy_reset: null argument");
	GreedyDev &d = h->d;
	if (d.code < 0) return fail(RK_ESTATE, "rk_greedy_reset: ask for the net batch first (rk_greedy_net_in)");
	if (n_games < 1 || n_games > d.G) return fail(RK_EINVAL, "rk_greedy_reset: n_games %d outside 1..%d", n_games, d.G);
	if (max_states < 1 || max_states > d.S) return fail(RK_EINVAL, "rk_greedy_reset: max_states %d outside 1..%d", max_states, d.S);
	if (int e = check_cubie_codes("rk_greedy_reset", "root", h_roots, (size_t)n_games)) return e;
	hipStream_t st = (hipStream_t)stream;
	h->ready = false;
	RK_HIP(hipMemcpyAsync(h->roots_dev, h_roots, (size_t)n_games * STATE_BYTES, hipMemcpyHostToDevice, st));
	RK_HIP(hipMemsetAsync(d.ctr, 0, Y_COUNT * sizeof(int32_t), st));
	hipLaunchKernelGGL(k_greedy_begin, dim3(blocks((size_t)d.G, 4)), dim3(256), 0, st, d, h->roots_dev, n_games, max_states);
	RK_HIP(hipGetLastError());
	RK_HIP(hipStreamSynchronize(st));           // the host buffer may go away after return
	h->n_games = n_games; h->budget = max_states;
	h->ready = true;
	return RK_OK;
}

int rk_greedy_step(rk_greedy_t *h, const void *d_out, int dtype, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_greedy_step: reset the engine first");
	int bf16 = 0;
	if (int e = check_net_out("rk_greedy_step", d_out, dtype, &bf16)) return e;
	hipLaunchKernelGGL(k_greedy_step, dim3(blocks((size_t)h->d.G, 4)), dim3(256), 0, (hipStream_t)stream, h->d, d_out, bf16);
	RK_HIP(hipGetLastError());
	return RK_OK;
}

int rk_greedy_status(rk_greedy_t *h, long long *h_status, void *stream)
{
	if (!h || !h->ready || !h_status) return fail(RK_EINVAL, "rk_greedy_status: bad argument");
	int32_t c[Y_COUNT];
	if (int e = h->ctr_host.read(h->d.ctr, Y_COUNT, c, (hipStream_t)stream)) return e;
	h_status[0] = c[Y_RUNNING]; h_status[1] = c[Y_LAUNCHES]; h_status[2] = c[Y_ERROR]; h_status[3] = c[Y_GAMES]; h_status[4] = c[Y_BUDGET];
	h_status[5] = h_status[6] = h_status[7] = 0;
	return RK_OK;
}

int rk_greedy_export(rk_greedy_t *h, long long *h_status, long long *h_steps, uint8_t *h_actions, void *stream)
{
	if (!h || !h->ready) return fail(RK_ESTATE, "rk_greedy_export: reset the engine first");
	const GreedyDev &d = h->d;
	hipStream_t st = (hipStream_t)stream;
	const size_t n = (size_t)h->n_games, width = (size_t)h->budget;
	Widened<int32_t, long long> status, steps;
	if (int e = status.start(d.status, n, h_status, st)) return e;
	if (int e = steps.start(d.steps, n, h_steps, st)) return e;
	if (h_actions != nullptr)
		RK_HIP(hipMemcpy2DAsync(h_actions, width, d.actions, (size_t)d.S, width, n, hipMemcpyDeviceToHost, st));
	RK_HIP(hipStreamSynchronize(st));
	status.finish();
	steps.finish();
	return RK_OK;
}

}  // extern "C"
