// Shortening action queues against a kept ball: what rk_ball.hip's rk_bshorten and rk_sym.hip's rk_sshorten share.  A queue is a
// DAG over 0 .. L with an edge i -> j of weight d(i, j) -- the ball's depth of X(i, j), the solved state after the moves
// a[i .. j-1] -- for every window j - i <= W that the ball holds, and its best rewrite a shortest path.  A call is three launches:
//   windows   d(i, j) of every window as one byte, -1 outside the ball: byte (p * max_len + j - 1) * window + (j - i - 1)
//   dp        a workgroup per queue: cost[j] = min cost[i] + w(i, j), ties to the largest i; cost in LDS, pred to scratch
//   emit      a wave per queue: back along pred, then forward; an edge with d < j - i is replaced by the ball's word for X(i, j)
// Nothing here looks at a ball: the limits, the composition of a chunk of 64 moves onto a carried state (shorten_compose, shorten_carry), the
// DP (shorten_dp, and its kernel k_shorten_dp), the emit but for the word of a replaced edge (shorten_emit over shorten_successors,
// the reversal of the pred chain), the scratch layout and the host's argument checks (shorten_check).  A ball keeps what makes it
// different: how d(i, j) is looked up -- rk_ball.hip probes the raw state,
// rk_sym.hip its canonical representative -- and which word a replaced edge gets: the stored actions along the parents there,
// the inverse of the descent here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rubiks_hip.h"
#include "rk_device.h"
#include "rk_error.h"

namespace rk {

constexpr int SHORTEN_MAX_LEN = 1 << 12;
constexpr uint16_t SHORTEN_KEPT = 0xFFFFu;      // pred[0] of a queue that is not rewritten (an action outside 0..11, a length outside 0..max_len)
constexpr int SHORTEN_DP_THREADS = 256;

__device__ __forceinline__ int shorten_len(const int32_t *len, size_t p, int max_len)
{
	const int L = len[p];
	return L < 0 ? 0 : L > max_len ? max_len : L;
}

// One chunk of up to 64 consecutive moves, one per lane (`a`; lanes >= n hold none), applied to the carried state s: st = the
// state after the moves of lanes 0 .. lane.  An action outside 0..11 indexes no table (it counts as action 0; its queue is never
// rewritten).  All 64 lanes call it.  shorten_carry then moves s on to the state after all n (lane n - 1's st, the same in every
// lane) for the next chunk.  The two are apart because the windows kernels probe st in between: carried first, the five scalars
// of s would live across the probes.
__device__ __forceinline__ void shorten_compose(const u32x4 *s_act, uint32_t a, int lane, int n, const uint32_t s[5], uint32_t st[5])
{
	uint32_t X[12];
	if (lane < n) load_action_table(s_act, a < 12u ? a : 0u, X);
	else identity_moves(X);
	scan_moves(X, lane, lane, n);
	#pragma unroll
	for (int j = 0; j < 5; j++) st[j] = s[j];
	move5(st, X);
}

__device__ __forceinline__ void shorten_carry(const uint32_t st[5], int n, uint32_t s[5])
{
	#pragma unroll
	for (int j = 0; j < 5; j++) s[j] = (uint32_t)__builtin_amdgcn_readlane((int)st[j], n - 1);
}

// The shortest path 0 -> L of queue blockIdx.x, the whole body of a DP kernel of SHORTEN_DP_THREADS threads.  key = cost << 12 |
// (j - i - 1): the minimum is the least cost and, among equal costs, the largest i.  One barrier per j: the partial minima
// alternate between two rows, and cost[j] is read by the thread that wrote it (k = 1) or two barriers later.
__device__ __forceinline__ void shorten_dp(const int8_t *__restrict__ actions, const int32_t *__restrict__ len, int max_len, int window,
                                           const int8_t *__restrict__ depth, uint16_t *__restrict__ pred, int32_t *error)
{
	__shared__ uint16_t cost[SHORTEN_MAX_LEN + 1];
	__shared__ uint32_t part[2][SHORTEN_DP_THREADS / 64];
	const size_t p = blockIdx.x;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int L = shorten_len(len, p, max_len);
	const int8_t *row = actions + p * (size_t)max_len;
	uint16_t *pr = pred + p * (size_t)(max_len + 1);
	int bad = len[p] != L;
	for (int k = tid; k < L; k += SHORTEN_DP_THREADS) bad |= (uint8_t)row[k] >= 12u;
	if (__syncthreads_or(bad)) {                                         // reported; the queue comes back as it is
		if (tid == 0) { pr[0] = SHORTEN_KEPT; *error = RK_EINVAL; }
		return;
	}
	if (tid == 0) { cost[0] = 0; pr[0] = 0; }
	__syncthreads();
	for (int j = 1; j <= L; j++) {
		const int8_t *dj = depth + (p * (size_t)max_len + (size_t)(j - 1)) * (size_t)window;
		const int kmax = min(window, j);
		uint32_t best = 0xFFFFFFFFu;
		for (int k = tid + 1; k <= kmax; k += SHORTEN_DP_THREADS) {          // i = j - k
			const int d = dj[k - 1];
			const int wgt = d >= 0 ? d : k == 1 ? 1 : -1;                        // a single move outside the ball (radius 0) costs itself
			if (wgt >= 0) best = min(best, (((uint32_t)cost[j - k] + (uint32_t)wgt) << 12) | (uint32_t)(k - 1));
		}
		#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, off, 64));
		if (lane == 0) part[j & 1][wave] = best;
		__syncthreads();
		if (tid == 0) {
			uint32_t m = part[j & 1][0];
			#pragma unroll
			for (int v = 1; v < SHORTEN_DP_THREADS / 64; v++) m = min(m, part[j & 1][v]);
			cost[j] = (uint16_t)(m >> 12);                                   // (k = 1 is always a candidate: m is a real key)
			pr[j] = (uint16_t)(j - 1 - (int)(m & 0xFFFu));
		}
	}
}

// The DP kernel of both balls (internal linkage: this header goes into two .hip files of one library).
namespace {
__global__ __launch_bounds__(SHORTEN_DP_THREADS)
void k_shorten_dp(const int8_t *__restrict__ actions, const int32_t *__restrict__ len, int max_len, int window,
                  const int8_t *__restrict__ depth, uint16_t *__restrict__ pred, int32_t *error)
{
	shorten_dp(actions, len, max_len, window, depth, pred, error);
}
}  // namespace

// The top of an emit kernel of ONE wave: the pred chain of a queue of L moves, from L back to 0, turned into a chain of successors
// from 0 in nxt (LDS, SHORTEN_MAX_LEN + 1 entries; s_ok: one LDS word).  False when the chain is not one the DP can have written
// (never: it wrote pred[j] in j - window .. j - 1).  All 64 lanes call it and get the same answer.
__device__ __forceinline__ bool shorten_successors(const uint16_t *__restrict__ pr, int L, int window, int lane, uint16_t *nxt, int *s_ok)
{
	for (int k = lane; k <= L; k += 64) nxt[k] = pr[k];
	__syncthreads();
	if (lane == 0) {
		int good = 1;
		int j = L, i = L > 0 ? nxt[L] : 0;
		while (j > 0) {
			if (i >= j || j - i > window) { good = 0; break; }              // (never: the DP wrote pred[j] in j - window .. j - 1)
			const int ii = i > 0 ? nxt[i] : 0;
			nxt[i] = (uint16_t)j;
			j = i; i = ii;
		}
		*s_ok = good;
	}
	__syncthreads();
	return *s_ok != 0;
}

// The rewritten queue of queue blockIdx.x, the body of an emit kernel of ONE wave that has staged s_act.  Lane 0 turns the pred
// chain from L into a chain of successors from 0 (shorten_successors; its barriers are behind the kernel's staging as well), then
// the wave takes the edges in order.  An edge of weight j - i (or a single move outside the ball) is copied.  Any other is
// replaced: X(i, j) is composed again and word(x, d, at) writes the ball's d moves for x = X(i, j) to at[0 .. d - 1] -- they fit
// -- and says whether it could; x is the same in every lane and all 64 lanes call it.  A word that fails or an index out of range
// is RK_ESTATE and the queue comes back as it is.  The output is never longer than the input; every index is checked all the same.
template <typename Word>
__device__ __forceinline__ void shorten_emit(const u32x4 *s_act, const int8_t *__restrict__ actions, const int32_t *__restrict__ len, int max_len,
                                             int window, const int8_t *__restrict__ depth, const uint16_t *__restrict__ pred,
                                             int8_t *__restrict__ out_actions, int32_t *__restrict__ out_len, int32_t *error, Word &&word)
{
	__shared__ uint16_t nxt[SHORTEN_MAX_LEN + 1];
	__shared__ int s_ok;
	const size_t p = blockIdx.x;
	const int lane = threadIdx.x;
	const int L = shorten_len(len, p, max_len);
	const int8_t *row = actions + p * (size_t)max_len;
	int8_t *out = out_actions + p * (size_t)max_len;
	const uint16_t *pr = pred + p * (size_t)(max_len + 1);
	bool ok = pr[0] != SHORTEN_KEPT;
	int pos = 0;
	if (ok) {
		ok = shorten_successors(pr, L, window, lane, nxt, &s_ok);
		for (int i = 0; ok && i < L; ) {
			const int j = nxt[i], span = j - i;
			if (span < 1 || span > window || j > L) { ok = false; break; }
			const int d = depth[(p * (size_t)max_len + (size_t)(j - 1)) * (size_t)window + (size_t)(span - 1)];
			if (d < 0 || d >= span) {                                        // as short as the ball knows: copied
				if (pos + span > max_len) { ok = false; break; }
				for (int k = lane; k < span; k += 64) out[pos + k] = row[i + k];
				pos += span;
			} else if (d > 0) {
				uint32_t x[5] = {SOLVED_DW[0], SOLVED_DW[1], SOLVED_DW[2], SOLVED_DW[3], SOLVED_DW[4]};
				for (int d0 = 0; d0 < span; d0 += 64) {
					const int nc = min(64, span - d0);
					uint32_t st[5];
					shorten_compose(s_act, lane < nc ? (uint32_t)(uint8_t)row[i + d0 + lane] : 0xFFu, lane, nc, x, st);
					shorten_carry(st, nc, x);
				}
				if (pos + d > max_len || !word(x, d, out + pos)) { ok = false; break; }
				pos += d;
			}
			i = j;
		}
		if (!ok && lane == 0) *error = RK_ESTATE;                           // an engine error: the queue comes back as it is
	}
	if (!ok) {
		for (int k = lane; k < L; k += 64) out[k] = row[k];
		pos = L;
	}
	for (int k = pos + lane; k < max_len; k += 64) out[k] = -1;
	if (lane == 0) out_len[p] = pos;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
constexpr size_t SHORTEN_MAX_WAVES = (size_t)1 << 30;    // queues x max_len of one call: a wave each in rk_bshorten, four to a workgroup

// the d(i, j) bytes of a call, rounded up so that the pred rows behind them are aligned
inline size_t shorten_depth_bytes(size_t n, int max_len, int window) { return (n * (size_t)max_len * (size_t)window + 15) & ~(size_t)15; }

// The argument checks of a shortening entry `who` on a ball `h` (built: whether it is), before anything is launched.  The
// scratch has one size and one layout for both balls: rk_bshorten_scratch_bytes.
inline int shorten_check(const char *who, const void *h, bool built, const int8_t *d_actions, const int32_t *d_len, size_t n, int max_len,
                         int window, const int8_t *d_out_actions, const int32_t *d_out_len, const int32_t *d_error, const void *d_scratch,
                         size_t scratch_bytes)
{
	if (!h) return fail(RK_EINVAL, "%s: null ball", who);
	if (!built) return fail(RK_ESTATE, "%s: build the ball first", who);
	const long long need = rk_bshorten_scratch_bytes(n, max_len, window);
	if (need < 0) return (int)need;
	if (!d_error) return fail(RK_EINVAL, "%s: null pointer", who);
	if (n != 0 && (!d_actions || !d_len || !d_out_actions || !d_out_len || !d_scratch)) return fail(RK_EINVAL, "%s: null pointer", who);
	if (((uintptr_t)d_len | (uintptr_t)d_out_len | (uintptr_t)d_error) & 3u) return fail(RK_EINVAL, "%s: device pointers must be 4-byte aligned", who);
	if ((uintptr_t)d_scratch & 15u) return fail(RK_EINVAL, "%s: the scratch must be 16-byte aligned", who);
	if (n != 0 && d_actions == d_out_actions) return fail(RK_EINVAL, "%s: the output may not be the input", who);
	if (scratch_bytes < (size_t)need) return fail(RK_EINVAL, "%s: %zu bytes of scratch, %lld needed", who, scratch_bytes, need);
	return RK_OK;
}

}  // namespace rk
