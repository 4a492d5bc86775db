/*
 * rubiks_hip.h -- C ABI of librubiks_hip.so, the MI355X (gfx950) cube engine.
 *
 * The reference (peleiden/librubiks) is pure Python and has no FFI of its own; the boundary this
 * library replaces is the module surface of `librubiks.cube` (librubiks/cube/__init__.py:2) and
 * the expand-children sections of `librubiks.solving.agents`.  Each entry point below names the
 * reference function (file:line under /root/reference) whose arithmetic it performs.  The ctypes
 * stub a maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Every entry returns 0 on success or a negative RK_E* code; rk_last_error() gives the
 *     thread-local message of the last failure.  No entry ever falls back to a CPU path.
 *   - Pointers named d_* are DEVICE pointers (hipMalloc / tensor.data_ptr()); h_* are host
 *     pointers.  The library never frees or retains caller memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Device-pointer entries
 *     are stream-ordered and do not synchronise; *_host entries copy, launch, copy back and
 *     synchronise `stream` before returning.  Everything an entry launches, copies or waits for goes to
 *     its `stream` argument; an rk_*_create takes no stream and has finished its own initialisation
 *     when it returns.  One handle is driven on one stream at a time: two streams using the same
 *     handle at once is not supported (two handles on two streams are independent).
 *   - A 20-byte state is int8[20]: 8 corner codes slot*3+ori then 12 edge codes slot*2+ori
 *     (cube.py:58-65).  State arrays are dense row-major (n, 20); their base must be 4-byte
 *     aligned (always true for rows of a 256-B aligned allocation).
 *   - An action index a in [0,12) means face a/2, direction 1-(a%2) (cube.py:33-34).  PRECONDITION of the
 *     device-pointer entries: every action code is < 12.  A larger code is treated as action 0 (the kernels never
 *     index past the move table) and the result for that row is meaningless; the *_host entries check and fail
 *     with RK_EINVAL, as the reference's table indexing would raise.
 *   - repr: RK_REPR_2024 = 20-byte cubie codes, RK_REPR_686 = int8 (6,8,6) one-hot, 288 bytes
 *     (cube.py:67-71).
 */
#ifndef RUBIKS_HIP_H
#define RUBIKS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RK_REPR_2024 0
#define RK_REPR_686  1

#define RK_OK          0
#define RK_EINVAL     -1   /* bad argument (null pointer, misaligned base, unknown repr, ...) */
#define RK_EHIP       -2   /* a HIP runtime call failed; message holds hipGetErrorString */
#define RK_ECAPACITY  -3   /* an engine ran out of the capacity it was created with */
#define RK_ESTATE     -4   /* call not valid in the engine's current state */

#define RK_OH_F32  0
#define RK_OH_F16  1
#define RK_OH_BF16 2
#define RK_OH_STATES 3   /* engines only: hand the net the 20-byte states themselves (first layer fused, rk_ohl_*) */
#define RK_OH_I8   4     /* rk_oh686_from2024 only: int8 0 / 1 elements, i.e. the (6,8,6) state itself */

#define RK_OHL_GATHER 0  /* exact float32 gather-sum through an LDS-resident weight slice */
#define RK_OHL_MFMA   1  /* bf16 MFMA with the one-hot operand synthesised in registers; the form follows the batch size */
#define RK_OHL_MFMA_DIRECT 2  /* ... always the few-rows form: one 32 x 32 output tile per wave, weights straight from global memory */
#define RK_OHL_MFMA_TILED  3  /* ... always the many-rows form: a 64-column weight tile resident in LDS (same bits as the direct form) */
/* epilogue activation of the fused first layer (rk_ohl_set_epilogue) */
#define RK_OHL_ACT_NONE 0
#define RK_OHL_ACT_ELU  1  /* x > 0 ? x : alpha (exp(x) - 1)          nn.ELU, the reference's default, model.py:30 */
#define RK_OHL_ACT_RELU 2

/* ---- library ------------------------------------------------------------------------------ */
int         rk_version(void);
const char *rk_last_error(void);
/* Select `device` for the calling thread and check that it is a gfx950 part. */
int         rk_init(int device);

/* The large launches of the write-heavy kernels (fan-out, one-hot, 6x8x6 fan-out, multi_rotate) run in a PACED form: inputs read
 * first, every tile's stores released on a fixed-rate schedule.  Results never depend on it.  mode 0 switches
 * the form off for this process (the unpaced kernels run at every size), 1 on, -1 back to the environment's choice (RK_PACE,
 * default on).  bench.py uses it to time both forms on the same box in one run (`frac_ring_same_box`). */
int rk_set_pacing(int mode);
/* The fan-out's store schedule is measured once per device and process (rk_init does it; about 4 ms, 272 MB of scratch that is freed
 * again): the ring form and 2.0 / 2.1 / 2.2 / 2.4 ns per 64-parent tile on 1 Mi parents.  The compiled 2.1 ns stay unless another
 * candidate is more than 3 % faster -- a part whose HBM does not keep that schedule gets the one it does keep, the unpaced form
 * included.  rk_calibrate_pacing(force != 0) measures again.  Skipped when RK_PACE_TAU_PS, RK_PACE=0 or RK_PACE_CALIBRATE=0 say so.
 * rk_get_pacing: *tau_ps = picoseconds per tile in force on the current device (0 = unpaced), *source = 0 compiled default (not
 * calibrated yet), 1 calibrated, 2 fixed by the environment or calibration impossible; h_us (nullable, 5 floats) = measured
 * microseconds per 1 Mi-parent launch of {ring form, 2.0, 2.1, 2.2, 2.4 ns}, zeros if nothing was measured.  Any pointer may be null. */
int rk_calibrate_pacing(int force);
int rk_get_pacing(unsigned int *tau_ps, int *source, float *h_us);
/* Everything the paced forms keep is PER DEVICE (time-base cells, the measured schedule, the turn gate): this is the slot of `device` in
 * those tables -- the device's own index, or -1 for a device the tables have no room for (it runs the unpaced forms).  Pure host
 * arithmetic, no HIP call: a diagnostic, and what the CPU test pins ("two devices never share a slot"). */
int rk_pace_slot_of_device(int device);
/* Stream lifetime.  Paced launches on different streams take turns: the library remembers, per device, the
 * stream of the last paced launch and, when the next one arrives on another stream, makes it wait (event record + stream wait)
 * for that stream.  It only ever remembers a stream it may rely on: the null stream, and streams REGISTERED with
 * rk_stream_register(stream) -- the caller's promise that the stream stays alive until rk_stream_forget(stream), which must be
 * called before the stream is destroyed.  A paced launch on an unregistered stream takes no turn (it may overlap another paced
 * launch: slower, never wrong) and nothing about it is kept.  The Python shim registers torch's pooled streams, which are never
 * destroyed.  Both entries are cheap and idempotent; neither touches the stream. */
int rk_stream_register(void *stream);
int rk_stream_forget(void *stream);

/* Move tables, written to HOST memory.
 * RK_REPR_2024: uint8 (12,2,24) absolute table T[a][kind][v] = v + maps[dir][face][kind][v]
 *               (maps.py:107-145).   RK_REPR_686: uint8 (12,48) sticker-slot permutation,
 *               new[slot] = old[perm[a][slot]], slot = 8*face+pos (cube.py:330-347). */
int rk_tables(int repr, uint8_t *h_out);
/* The six face definitions the tables are generated from, in the order F, B, T, D, L, R, written to HOST memory as uint8 (6,14):
 * [0:4] ring of corner slots and [4:8] ring of side slots a positive turn cycles (ring[j] -> ring[j+1]), [8] the corner
 * orientation that stays while the other two swap, [9] 1 if the turn flips side orientations (maps.py:74-98 `Actions`), [10:14]
 * the face's four neighbours in positive direction (maps.py:149-156 `neighbors_686`).  What `librubiks.cube.maps` exposes as
 * `Actions` / `neighbors_686`; the drop-in's maps.py rebuilds both from this entry. */
int rk_face_definitions(uint8_t *h_out);
/* Solved state in HOST memory: int8[20] (cube.py:58-65) or int8[288] (cube.py:67-71). */
int rk_solved(int repr, int8_t *h_out);

/* ---- plain device memory helpers (for hosts that do not bring their own allocator) -------- */
int rk_malloc(void **d_ptr, size_t bytes);
int rk_free(void *d_ptr);
int rk_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int rk_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
int rk_memset(void *d_dst, int value, size_t bytes, void *stream);
int rk_stream_synchronize(void *stream);

/* ---- cube hot path, device pointers -------------------------------------------------------- */

/* multi_rotate (cube.py:49-52, 256-263; 686: cube.py:349-361): d_out[i] = move d_actions[i]
 * applied to d_states[i].  d_out may equal d_states. */
int rk_multi_rotate(int repr, const int8_t *d_states, const uint8_t *d_actions, int8_t *d_out,
                    size_t n, void *stream);
/* multi_rotate + multi_is_solved of the MOVED states in one launch -- the pair the reference's per-row callers always run back
 * to back (agents.py:157-159 ValueSearch, :696-703 EGVM, train.py:277-281): d_out[i] = move d_actions[i] of d_states[i] (d_out
 * may equal d_states), d_flags[i] (nullable) = d_out[i] is solved, d_stats (nullable, int64[2], initialised by the caller as for
 * rk_expand12: [0] += solved rows, [1] = min(first solved row, previous value)); at least one of the two outputs.  20-byte
 * states: 21 B read + 21 B written per state, the moved states are never read back.  (6x8x6: two launches inside.) */
int rk_multi_rotate_solved(int repr, const int8_t *d_states, const uint8_t *d_actions, int8_t *d_out, uint8_t *d_flags,
                           long long *d_stats, size_t n, void *stream);
/* Same as rk_multi_rotate with the reference's (faces, directions) pair as two uint8 arrays (20-byte states only). */
int rk_multi_rotate_fd(int repr, const int8_t *d_states, const uint8_t *d_faces, const uint8_t *d_dirs,
                       int8_t *d_out, size_t n, void *stream);
/* The device-pointer entries (rk_multi_rotate, rk_multi_rotate_solved, rk_multi_rotate_fd, rk_apply_sequences) take action
 * codes as they are: a code >= 12 is treated as action 0 -- the kernels never index past the move table -- and leaves a sticky
 * mark on the device.  This reads the mark into *h_seen (1: some launch since the last call saw such a code) and clears it
 * in ONE atomic exchange on the device, and synchronises `stream`.  The mark is per device, not per stream: it reports the
 * launches of every stream.  The host entries (rk_*_host) validate their arrays and fail with RK_EINVAL instead, like the
 * reference's table indexing raises IndexError (cube.py:33-34, 256-263). */
int rk_bad_actions_seen(int *h_seen, void *stream);

/* The 12-child fan-out `multi_rotate(repeat(S,12), *iter_actions(n))` (agents.py:277-281, :513,
 * :605; train.py:285) fused with `multi_is_solved` of the children (cube.py:88-89; agents.py:321,
 * :540; train.py:292).  d_children is (12 n, state) parent-major / action-minor and must be 16-byte
 * aligned.  d_solved (nullable) gets one byte per child.  d_stats (nullable) is int64[2] that the
 * caller zero/initialises: [0] += number of solved children, [1] = min(index of a solved child,
 * previous value) -- initialise [1] to INT64_MAX.  The statistics are meant for RARE hits (a search
 * looking for its goal): every wave that has a solved child reports with two device-scope atomics
 * on these two words, and atomics on one address complete about one every 25 ns chip-wide -- 12 M
 * states of which 4 000 are solved take 0.24 ms with d_stats and 0.04 ms without.  Use d_solved
 * when hits are common. */
int rk_expand12(int repr, const int8_t *d_parents, int8_t *d_children, uint8_t *d_solved,
                long long *d_stats, size_t n, void *stream);

/* Structure-of-arrays form of the fan-out for device-resident pipelines (same arithmetic, different layout):
 * d_parents uint32 [5][n] (plane j = bytes 4j..4j+3 of every state), d_children uint32 [12][5][n] (child a of
 * parent p has its dword j at [(a*5 + j)*n + p]), d_solved uint8 [12][n] (nullable).  Every access of a wavefront
 * is one contiguous run, so the kernel needs no LDS transpose.  d_stats as rk_expand12 (the index it reports is
 * 12 p + a).  rk_states_to_soa / rk_states_from_soa convert between (n,20) int8 rows and the five planes. */
int rk_expand12_soa(const uint32_t *d_parents, uint32_t *d_children, uint8_t *d_solved, long long *d_stats, size_t n,
                    void *stream);
int rk_states_to_soa(const int8_t *d_states, uint32_t *d_planes, size_t n, void *stream);
int rk_states_from_soa(const uint32_t *d_planes, int8_t *d_states, size_t n, void *stream);

/* multi_is_solved (cube.py:88-89).  d_flags (nullable) one byte per state; d_stats as above. */
int rk_multi_is_solved(int repr, const int8_t *d_states, uint8_t *d_flags, long long *d_stats,
                       size_t n, void *stream);

/* Move sequences from the solved state: the device half of scramble (cube.py:206-216) and
 * sequence_scrambler (cube.py:218-232).  d_actions is (depth, games) uint8, row d = d-th move of
 * every game (the layout of the reference's faces/dirs draws).  Game g emits `rows` =
 * (with_solved ? 1 : 0) + moves states, where moves = depth - with_solved: optionally the solved
 * state, then the state after each of its first `moves` moves.  If only_last != 0 just the final
 * state of each game is written (d_out is (games, state)), else d_out is (games*rows, state)
 * game-major. */
int rk_apply_sequences(int repr, const uint8_t *d_actions, int depth, int games, int with_solved,
                       int only_last, int8_t *d_out, void *stream);

/* The cube part of one Autodidactic-Iteration rollout in ONE launch (train.py:277-292): d_actions uint8 (depth, games) as for
 * rk_apply_sequences (not only_last) ->
 *   d_states        (games*depth, 20)    the states along every game's walk, game-major            (cube.py:218-232; train.py:277)
 *   d_state_flags   (games*depth) uint8  1 where such a state is solved, nullable                  (train.py:281)
 *   d_children      (12*games*depth, 20) their children, parent-major, action-minor                (train.py:285)
 *   d_child_flags   (12*games*depth) uint8 1 where a child is solved                               (train.py:292)
 *   d_stats         int64[2], nullable, as rk_expand12's: [0] += solved children, [1] = min(first solved child, previous value)
 * The same bytes as rk_apply_sequences + rk_multi_is_solved + rk_expand12, without writing the states once and reading them twice. */
int rk_rollout_fanout(int repr, const uint8_t *d_actions, int depth, int games, int with_solved, int8_t *d_states, uint8_t *d_state_flags,
                      int8_t *d_children, uint8_t *d_child_flags, long long *d_stats, void *stream);
/* as_oh (cube.py:130-133, 265-277; 686: cube.py:363-369): one-hot encode n states into
 * (n, 480) [2024] or (n, 288) [686] elements of out_dtype (RK_OH_*); d_out 16-byte aligned. */
int rk_as_oh(int repr, const int8_t *d_states, void *d_out, int out_dtype, size_t n, void *stream);

/* Fused one-hot -> first Linear of the net (cube.py:265-277 + model.py:127,150): y = as_oh(states) @ W^T + b without the
 * one-hot ever reaching HBM.  rk_ohl_create copies nn.Linear(480, H)'s weight (H, 480) row-major and bias (H), both
 * float32 or both bfloat16 (w_dtype = RK_OH_F32 / RK_OH_BF16; bias may be NULL), into the layouts the two routes use;
 * H must be a multiple of 64.  rk_ohl_forward: d_out (n, H) row-major, 16-byte aligned.
 *   RK_OHL_GATHER  y = ((b + w_0) + w_1) + ... + w_19 with float32 adds in that order (w_i = row 24 i + state[i] of W^T):
 *                  exact and reproducible; out_dtype RK_OH_F32 or RK_OH_BF16 (rounded to nearest even at the end)
 *   RK_OHL_MFMA    bf16 weights, float32 accumulation on the matrix cores, out_dtype RK_OH_BF16.  Two forms with identical
 *                  results: up to 768 rows (a search step's batch) every wave computes one output tile from weights it
 *                  reads itself; beyond, workgroups keep a weight tile in LDS.  RK_OHL_MFMA_DIRECT / _TILED force one. */
typedef struct rk_ohl rk_ohl_t;
int rk_ohl_create(rk_ohl_t **out, const void *d_weight, int w_dtype, const void *d_bias, int H, void *stream);
int rk_ohl_destroy(rk_ohl_t *h);
int rk_ohl_forward(rk_ohl_t *h, const int8_t *d_states, void *d_out, int out_dtype, size_t n, int route, void *stream);
/* Optional epilogue of every later rk_ohl_forward:  y = scale * act(x W^T + b) + shift  per output column -- the
 * activation (model.py:157) and the eval-mode BatchNorm1d (model.py:158-159: scale = gamma / sqrt(var + eps), shift =
 * beta - mean * scale) that follow the layer, computed in float32 on the accumulators.  d_scale / d_shift: H float32
 * values on the device, copied; both null = no affine part.  act RK_OHL_ACT_NONE and null pointers restore the plain layer. */
int rk_ohl_set_epilogue(rk_ohl_t *h, int act, float alpha, const float *d_scale, const float *d_shift, void *stream);
/* Training (train.py:165-179 with the layer reading states): the handle follows live parameters and gives their gradient.
 * rk_ohl_set_weights runs rk_ohl_create's layout preparation again, from d_weight (H, 480) / d_bias (H or NULL) of w_dtype, into the
 * buffers the handle already owns, in stream order: no allocation, no synchronisation (the tensors must stay alive until the stream
 * has got there), a set epilogue stays set.  A following rk_ohl_forward on any route gives, bit for bit, what a handle created on
 * those weights gives.
 * rk_ohl_backward: d_states (n, 20) int8, d_dy (n, H) float32 row-major, 16-byte aligned ->
 *     d_dw[h, 24 i + v] = sum over the rows r with code(r, i) = v of d_dy[r, h]         (H, 480) float32, nn.Linear.weight's layout
 *     d_db[h]           = sum over all rows of d_dy[r, h]                               H float32, or NULL
 * with the forward's codes (the byte read as unsigned, anything >= 24 counts as 23).  Both outputs are OVERWRITTEN: a column no row
 * selects is +0.0 whatever the buffer held, n = 0 writes zeros.  Plain float32 adds in an order that is a function of (n, H) alone
 * -- rows ascending inside a workgroup's row range (rk_ohl_backward_rows(n, H) rows each), the ranges ascending, db as the sum of cubie
 * 0's 24 bins ascending -- and no atomics: the same inputs give the same bits on every call and on every handle.  Arguments are checked
 * before any launch (RK_EINVAL: a null handle, states, dY or dW; d_dy or d_dw off 16-byte alignment).  The partial sums live in scratch
 * the handle owns, allocated at the first call that needs that much; later calls of the same or a smaller (n, H) need allocate nothing. */
int rk_ohl_set_weights(rk_ohl_t *h, const void *d_weight, int w_dtype, const void *d_bias, void *stream);
int rk_ohl_backward(rk_ohl_t *h, const int8_t *d_states, const float *d_dy, size_t n, float *d_dw, float *d_db, void *stream);
size_t rk_ohl_backward_rows(size_t n, int H);

/* The net's other end (model.py:124-125,128-129: policy_net / value_net end in activation -> Linear(K, 12) / Linear(K, 1), and the
 * engines read those 12 + 1 numbers per row): y = act(x) @ W^T + b in ONE pass over x for a last layer of M <= 16 outputs, instead of an
 * elementwise kernel over (n, K) plus a GEMM with a 12-column output.  d_x (n, K) bfloat16 with row stride ldx elements (a multiple
 * of 8, rows 16-byte aligned), d_weight (M, K) bfloat16 row-major, d_bias M bfloat16 or NULL, d_out (n, M) bfloat16 row-major.
 * K is 512, 1024 or 2048; act RK_OHL_ACT_* (alpha for ELU), applied in float32 and rounded to bfloat16 as torch's activation kernel
 * stores it; float32 accumulation (v_dot2c_f32_bf16), the result rounded to bfloat16 (nearest even). */
int rk_tail_linear(const void *d_x, size_t n, int K, size_t ldx, const void *d_weight, const void *d_bias, int M, int act, float alpha,
                   void *d_out, void *stream);

/* as_correct (cube.py:371-380): 686 one-hot int8 (n,288) -> float32 (n,48) of +1/-1. */
int rk_as_correct686(const int8_t *d_states, float *d_out, size_t n, void *stream);

/* 20-byte -> 6x8x6 (cube.py:58-71; the layout is as_oh of the 686 state, cube.py:363-369): n 20-byte states into n rows of
 * 288 elements, element 48 f + 6 p + c = 1 where ring position p of face f shows colour c (48 ones per row).  out_dtype
 * RK_OH_F32 / _F16 / _BF16 (a 6x8x6 net's input batch) or RK_OH_I8 (the int8 (6,8,6) states themselves).  The states must
 * be legal (codes < 24, each position held once); an out-of-range code is read as 0 and the row is then meaningless.
 * d_states20 4-byte, d_out 16-byte aligned; n = 0 is a no-op. */
int rk_oh686_from2024(const int8_t *d_states20, void *d_out, int out_dtype, size_t n, void *stream);
/* 6x8x6 -> 20-byte, the inverse (cube.py:58-71): n int8 (6,8,6) states (16-byte aligned) into n 20-byte states (4-byte
 * aligned).  A row that is not a well-formed one-hot (six 0 / 1 bytes with exactly one 1 per slot) showing each of the 20
 * cubies exactly once is written as twenty -1 bytes and counted: d_stats (int64[2], nullable, initialise to [0, INT64_MAX])
 * gets [0] += such rows, [1] = min(first such row, previous value), as rk_multi_is_solved's counters. */
int rk_686_to2024(const int8_t *d_states686, int8_t *d_out20, long long *d_stats, size_t n, void *stream);

/* ---- batch weighted A* (agents.py:171-413): device-resident open set / closed set ---------------------------
 * Replaces the expand-children loop of AStar.search / expand_batch / relax_seen_states.  The engine owns:
 *   states (cap+1, 20) int8, G, parents, parent_actions            (agents.py:202-205; index 0 unused, root = 1)
 *   an open-addressing hash table state -> index                    (the `indices` dict, agents.py:201)
 *   the open queue as a few sorted runs (capacities 4K, 16K, 64K ... records, K = 12 * expansions): pop = the
 *   globally smallest (cost, index) records in heappop order, push = one multi-way merge into the first run that
 *   holds the result -- O(K log) queue traffic per iteration                       (the heapq, agents.py:185)
 * and EVERY size that varies (states, nodes popped, new states, won, out of budget) in device memory, so that one
 * reference iteration (agents.py:236-252 + 254-331) is two stream-ordered calls around the net forward that PyTorch
 * owns, neither of which synchronises with the host:
 *   rk_astar_step_expand : loop guard `len + 12 N <= max_states` (:236), pop the <= N best nodes (:238-239), 12-child
 *                          fan-out (:277-282), membership + first-occurrence de-duplication in parent-major batch order
 *                          (np.unique semantics, :286-295), append the unseen states with G / parent / action
 *                          (:299-313), goal test of the new states (:321-323), and the one-hot rows of the new states
 *                          (:379) into d_onehot (12 N, 480) -- rows past the number of new states are left untouched;
 *                          out_dtype RK_OH_STATES writes the (12 N, 20) int8 states instead (first layer fused)
 *   rk_astar_step_commit : d_values (12 N) from the net; cost = lambda*G + (-value) in float64 (:383), push (:316-317),
 *                          relaxation of the already-seen children (:326-329, 333-367; skipped once won, as the
 *                          reference returns before relaxing), bookkeeping and the next pop list
 *   rk_astar_status      : synchronises; h_status[8] = done, won, n_states, iterations, open-queue length, index of the
 *                          solved state, error, nodes the next iteration pops
 * Six launches per iteration (plus merge passes when 12 N > 2048), fixed shapes: an iteration can be captured in a
 * hipGraph.  Once `done` (won, out of budget, queue empty) further steps are no-ops.  Results are identical to the
 * reference's arrays (same index numbering, G, parents, parent_actions) whenever the value net returns the same
 * numbers.  An engine handle is not thread-safe: one host thread drives it, on one stream at a time.
 *
 * NON-FINITE VALUES (the single, the batched and the sharded engine alike).  A NaN among the values of the new states that
 * get a cost record -- values[j] for j below the number of new states of the iteration (and below `rows` of
 * rk_astar_shard_push_rows), exactly the values the engine reads; either sign, quiet or signalling, float32 or a bfloat16
 * NaN -- ends THAT search with engine error 4 (the first error of a search wins): the commit that read it reports done = 1,
 * error = 4, and nothing is popped again; the other searches of a batch run on undisturbed; every rank of a sharded search
 * takes stop reason 6 with error 4 at the next rk_astar_shard_select, before any pop is counted.  A cost has to have a place
 * in the order of the open queue and a NaN has none.  +inf and -inf are ordinary values and keep their order (a cost of
 * -inf is popped first, +inf last).  Values at and beyond the count are never read: a NaN there changes nothing.  A reset
 * (rk_astar_reset, rk_astarb_reset, rk_astar_shard_reset) clears the error.
 * Engine error codes: 1 pool capacity, 2 look-back chain, 3 more new states than net rows, 4 NaN value. */
typedef struct rk_astar rk_astar_t;
int rk_astar_create(rk_astar_t **out, size_t capacity, int max_expansions);
int rk_astar_destroy(rk_astar_t *h);
int rk_astar_reset(rk_astar_t *h, const int8_t *h_start_state, double lambda, void *stream);
/* max_states of agents.py:236 (default: the capacity). */
int rk_astar_set_budget(rk_astar_t *h, long long max_states, void *stream);
/* increase_stack_size (agents.py:396-402, called from :273-274): grows the node pool to new_capacity states IN PLACE -- new
 * arrays, device-to-device copies, one kernel that rebuilds the larger hash table; the open queue's sorted runs stay as they
 * are (only the top run, which can hold the whole pool, moves to a larger buffer).  States, G, parents, actions, the open
 * queue, the next pop list and every counter survive: a search that stopped at its loop guard because the pool was its
 * budget continues after rk_astar_set_budget, and ends with the arrays of a search that started in the larger pool.  Call
 * between iterations; synchronises `stream`; a hipGraph captured from this engine must be captured again (it holds the old
 * arrays).  RK_ECAPACITY when the device has no room (the engine is untouched then). */
int rk_astar_grow(rk_astar_t *h, size_t new_capacity, void *stream);
int rk_astar_step_expand(rk_astar_t *h, void *d_onehot, int out_dtype, void *stream);
int rk_astar_step_commit(rk_astar_t *h, const float *d_values, void *stream);
/* The value vectors handed to rk_astar_step_commit / rk_astar_commit / rk_astar_shard_push are float32 (default) or, after
 * rk_astar_set_values_dtype(h, RK_OH_BF16), bfloat16 as a bf16 net emits them (same pointer arguments; bf16 -> float32 is
 * exact, so the cost lambda * G - value is the same number; saves one conversion kernel per iteration).  Sticky until changed. */
int rk_astar_set_values_dtype(rk_astar_t *h, int dtype);
int rk_astar_status(rk_astar_t *h, long long *h_status /* [8] */, void *stream);
/* The same iteration as three calls for hosts that want to feed the net exactly the new states: rk_astar_expand
 * synchronises, h_info = {popped, new, won, solved_index, n_states} (popped == 0: the engine is done -- budget, nothing open --
 * and nothing is pending: there is no iteration to commit); rk_astar_new_states_oh writes the one-hot of the
 * `new` states in index order; rk_astar_commit takes their values. */
int rk_astar_expand(rk_astar_t *h, int n_expand, long long *h_info /* [5] */, void *stream);
int rk_astar_new_states_oh(rk_astar_t *h, void *d_out, int out_dtype, void *stream);
int rk_astar_commit(rk_astar_t *h, const float *d_values, void *stream);
/* Number of stored states (len(agent), agents.py:409-410) and of open-queue entries.  Synchronise. */
long long rk_astar_size(const rk_astar_t *h);
long long rk_astar_open_size(const rk_astar_t *h);
/* Copy rows [first, first+count) of the node arrays to HOST buffers (any may be NULL): states int8 (count,20),
 * G float64, parents int64, parent_actions int64 -- the reference's dtypes (agents.py:390-393). */
int rk_astar_export(rk_astar_t *h, size_t first, size_t count, int8_t *h_states, double *h_G, long long *h_parents,
                    long long *h_parent_actions, void *stream);
/* Action indices from the root to node `index`: the parents are walked on the device (agents.py:244-251).  Returns
 * the path length (>= 0) or a negative error; writes at most `max_len` actions. */
long long rk_astar_path(rk_astar_t *h, long long index, long long *h_actions, size_t max_len, void *stream);
/* Index of a state in the closed set or 0 (the `indices` dict lookup); host state in, synchronises. */
long long rk_astar_lookup(rk_astar_t *h, const int8_t *h_state, void *stream);
/* The open queue in pop order: up to max_len (cost, index) pairs to HOST arrays; returns the count written.
 * Inspection only (gathers every run and sorts on the host). */
long long rk_astar_export_open(rk_astar_t *h, double *h_costs, long long *h_indices, size_t max_len, void *stream);
/* The node indices the NEXT iteration pops, in heappop order (agents.py:238-239). */
long long rk_astar_next_pops(rk_astar_t *h, long long *h_indices, size_t max_len, void *stream);

/* ---- device-resident breadth-first search (agents.py:92-129) ---------------------------------------------------
 * The node pool (int8 (C+1, 20), index 0 unused, root = 1), the parent index and action of every node, and an
 * open-addressing table state -> index (the `self.states` dict, :103) live in HBM.  The FIFO queue (:104, :106, :121)
 * is the pool itself in index order.  One iteration pops up to `pops` nodes and is four launches with no host
 * synchronisation: 12-child fan-out in pop order with goal flag, membership test and in-batch first-occurrence
 * election (:108-112); the prefix of first occurrences; the cut and the append (:119-121); bookkeeping.  The cut
 * reproduces the check `len(self) < max_states` before every pop (:105) and the return of a solved child before it is
 * stored (:113-118): results equal the reference's dict in insertion order.  The time limit is the caller's (checked
 * between calls, not before every pop).  An engine handle is not thread-safe. */
typedef struct rk_bfs rk_bfs_t;
/* capacity: node pool size C (>= 2); pops: the most nodes one iteration pops (the grids are sized for it). */
int rk_bfs_create(rk_bfs_t **out, size_t capacity, int pops);
int rk_bfs_destroy(rk_bfs_t *h);
/* self.states = {start: (None, None)}; queue = deque([start]) (:103-104), with max_states of :105.  The start state is
 * a host 20-byte state that is not solved (:100 is the caller's).  Clears the table; synchronises. */
int rk_bfs_reset(rk_bfs_t *h, const int8_t *h_start_state, long long max_states, void *stream);
/* max_states of :105 for the iterations that follow.  A search that stopped at its budget goes on with a larger one, as
 * if it had been started with it: the table is first rebuilt from the pool, dropping the tentative claims a cut inside
 * a batch leaves behind.  Synchronises. */
int rk_bfs_set_budget(rk_bfs_t *h, long long max_states, void *stream);
/* `iterations` iterations of the while loop of :105-121, stream-ordered, no synchronisation; iterations after the
 * search is done (won, out of budget, queue empty) are no-ops.  The caller keeps size + 12 * pops * iterations <= C
 * (rk_bfs_grow); an iteration whose children might not fit is skipped and reported as error 1. */
int rk_bfs_run(rk_bfs_t *h, int iterations, void *stream);
/* Synchronises; h_status[8] = done, won, n_states (len(agent), :128-129), iterations, queue head index, stop reason
 * (0 running, 1 won, 2 budget, 3 queue empty, 4 error), error, nodes the next iteration pops. */
int rk_bfs_status(rk_bfs_t *h, long long *h_status, void *stream);
/* Grows the node pool to new_capacity states in place between iterations: new arrays, device-to-device copies, one
 * kernel that rebuilds the larger table.  The search continues where it stood.  Synchronises `stream`; RK_ECAPACITY
 * when the device has no room (the engine is untouched then). */
int rk_bfs_grow(rk_bfs_t *h, size_t new_capacity, void *stream);
/* Number of stored states, len(self.states) (:128-129).  Synchronises. */
long long rk_bfs_size(const rk_bfs_t *h);
/* Rows [first, first+count) of the pool to HOST buffers (any may be NULL): states int8 (count, 20), parent index
 * int64 and action int64 of every node -- the values of self.states (:120) as indices (0 for the root). */
int rk_bfs_export(rk_bfs_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions,
                  void *stream);
/* The action queue of a won search (:114-117): the parents are walked on the device.  Returns its length or a negative
 * error (RK_ESTATE: not won); writes at most max_len actions. */
long long rk_bfs_path(rk_bfs_t *h, long long *h_actions, size_t max_len, void *stream);

/* ---- device-resident two-sided breadth-first search: shortest solutions (quarter-turn metric) ---------------------
 * One pool in index order holds two balls: side S around the start (node 1) and side G around the solved state (node 2).
 * f and b count their complete levels.  One level grows at a time, S if f == b, else G; its parents are popped in index
 * order, their children taken in action order 0..11.  Before every pop: n_states >= max_states ends the search (not
 * won).  A child that the growing side already holds is skipped; one that the other side holds is the meeting: the
 * search ends (won) and the child is not stored; any other is appended with its parent, action and side.  With f and b
 * complete levels every solution has at least f + b + 1 moves and a meeting in the next level has exactly that many, so
 * the first meeting is a shortest solution.  Results do not depend on `pops`.  The time limit is the caller's (checked
 * between calls).  An engine handle is not thread-safe. */
typedef struct rk_bibfs rk_bibfs_t;
/* capacity: node pool size C (>= 2, both sides together); pops: the most nodes one iteration pops. */
int rk_bibfs_create(rk_bibfs_t **out, size_t capacity, int pops);
int rk_bibfs_destroy(rk_bibfs_t *h);
/* Nodes 1 and 2, f = b = 0, with the state budget max_states.  The start is a host 20-byte state that is not solved
 * (RK_EINVAL if it is: the answer is the empty queue).  Clears the table; synchronises. */
int rk_bibfs_reset(rk_bibfs_t *h, const int8_t *h_start_state, long long max_states, void *stream);
/* `iterations` iterations, stream-ordered, no synchronisation: each pops up to `pops` parents of the level that grows
 * and never crosses a level boundary; iterations after the search is done are no-ops.  The caller keeps
 * size + 12 * pops * iterations <= C (rk_bibfs_grow); an iteration whose children might not fit is skipped and reported
 * as error 1. */
int rk_bibfs_run(rk_bibfs_t *h, int iterations, void *stream);
/* Synchronises; h_status[12] = done, won, n_states (both sides), iterations, nodes popped, stop reason (0 running,
 * 1 met, 2 budget, 3 graph exhausted, 4 error), error, nodes the next iteration pops, f, b, the meeting node (the
 * stored node of the other side that the meeting child equals; 0 if none), the side that grows (0 = S, 1 = G). */
int rk_bibfs_status(rk_bibfs_t *h, long long *h_status, void *stream);
/* Grows the node pool to new_capacity states in place between iterations, as rk_bfs_grow does. */
int rk_bibfs_grow(rk_bibfs_t *h, size_t new_capacity, void *stream);
/* Number of stored states on both sides together.  Synchronises. */
long long rk_bibfs_size(const rk_bibfs_t *h);
/* Rows [first, first+count) of the pool to HOST buffers (any may be NULL): states int8 (count, 20), parent index int64
 * (0 for nodes 1 and 2), action int64 (the move from the parent, on side G away from solved) and side int64 (0 = S,
 * 1 = G) of every node. */
int rk_bibfs_export(rk_bibfs_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions,
                    long long *h_sides, void *stream);
/* The action queue of a search that met, start -> solved: the path to the S node of the meeting, the joining move, then
 * the inverses of side G's actions from its node back to node 2; walked on the device.  Returns its length or a
 * negative error (RK_ESTATE: not met); writes at most max_len actions. */
long long rk_bibfs_path(rk_bibfs_t *h, long long *h_actions, size_t max_len, void *stream);

/* ---- the goal ball: exact distances and shortest solutions from a kept table (quarter-turn metric) -----------------
 * Every state within `radius` moves of the solved state, built once and kept in HBM.  Node 1 is the solved state, the pool
 * is in index order: a level's parents are popped in index order, never across a level boundary, their children taken in
 * action order 0..11; a child the pool holds is skipped, every other is appended with its parent and its action, the move
 * AWAY from solved.  Level `radius` is stored and never expanded.  Level l is the index range level_start[l] ..
 * level_start[l + 1] - 1, so a node's depth follows from its index.  The capacity is exact (level sizes 1, 12, 114, 1 068,
 * 10 011, 93 840, 878 880, 8 221 632, 76 843 595) and every completed level is checked against them.  The pool does not
 * depend on `pops`.  After the build the ball is read-only; any number of queries and searches may read it. */
typedef struct rk_ball rk_ball_t;
/* radius 0..8; pops: the most parents one iteration of the build pops.  Allocates nothing. */
int rk_ball_create(rk_ball_t **out, int radius, int pops);
/* RK_ESTATE while a search (rk_bsearch_*, rk_bsearchb_*) is attached to the ball. */
int rk_ball_destroy(rk_ball_t *h);
/* Builds the ball (nothing if it is built): iterations of four launches, the host looks every `poll` of them.  A level of
 * the wrong size or a state too many is an engine error (RK_ESTATE); RK_ECAPACITY when the device has no room.  Afterwards
 * no table slot is tentative.  Synchronises. */
int rk_ball_build(rk_ball_t *h, int poll, void *stream);
/* h_status[16] = built, n_states, iterations of the build, radius, capacity, attached searches, then level_start[0 ..
 * radius + 1] (zeros before the build and beyond radius + 1).  Touches no device. */
int rk_ball_status(rk_ball_t *h, long long *h_status);
/* Rows [first, first+count) of the pool to HOST buffers (any may be NULL): states int8 (count, 20), parent index int64
 * (0 for node 1) and action int64 of every node. */
int rk_ball_export(rk_ball_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions,
                   void *stream);
/* d_depth[q] = exact distance to solved of DEVICE state q of d_states int8 (n, 20), -1 for a state outside the ball.  One
 * launch, one thread per query, nothing of the ball is written; stream-ordered, no synchronisation. */
int rk_ball_depth(rk_ball_t *h, const int8_t *d_states, size_t n, int32_t *d_depth, void *stream);
/* The shortest solution of every DEVICE state of d_states: d_lengths[q] moves (-1 outside the ball), row q of d_actions
 * int8 (n, radius) holds them, padded with -1.  One launch; stream-ordered, no synchronisation. */
int rk_ball_solve(rk_ball_t *h, const int8_t *d_states, size_t n, int32_t *d_lengths, int8_t *d_actions, void *stream);

/* ---- shortening action queues against the ball (rk_bshorten_*) ----------------------------------------------------------
 * One pass over a batch of action queues; neither their start states nor a net is needed.  The moves a[i .. j-1] of a queue,
 * applied to the solved state, give a state X(i, j); cube states are a group, so the distance between the queue's states s_i
 * and s_j is the distance of X(i, j) to solved, and any word that reaches X(i, j) from solved leads from s_i to s_j.  For
 * every 0 <= i < j <= len with j - i <= window, d(i, j) is the ball depth of X(i, j) (no edge outside the ball, except that a
 * single move outside a radius-0 ball costs 1).  cost[0] = 0, cost[j] = min over i of cost[i] + d(i, j), ties to the LARGEST
 * i; along the best path a window with d(i, j) = j - i is copied, any other is replaced by the ball's word for X(i, j): the
 * stored actions from node 1 down to the node.  The output has cost[len] <= len moves and reaches the same state from any
 * start; a queue whose every window is as short as the ball knows comes back byte for byte.  Three launches: d(i, j) of all
 * windows (a wave per queue and i), the shortest path (a workgroup per queue), the rewritten queue (a wave per queue).  The
 * ball is only read. */
/* Bytes of scratch one rk_bshorten call of this shape needs: n * max_len * window for d(i, j), n * (max_len + 1) * 2 for the
 * path.  RK_EINVAL unless 1 <= window <= max_len <= 4096 and n * max_len <= 2^30.  Touches no device.  rk_sshorten (the
 * symmetry ball's pass, below) takes scratch of the same size and layout: this function serves both. */
long long rk_bshorten_scratch_bytes(size_t n, int max_len, int window);
/* DEVICE d_actions int8 (n, max_len), row q holding d_len[q] actions 0..11 (what follows is ignored; -1 by convention), to
 * d_out_actions int8 (n, max_len), padded with -1, and d_out_len int32 (n); the output may not be the input.  d_scratch:
 * 16-byte aligned, scratch_bytes >= rk_bshorten_scratch_bytes(n, max_len, window).  d_error[0] is cleared, then set to
 * RK_EINVAL if a queue holds an action outside 0..11 before its length, or a length outside 0..max_len: no such action
 * indexes a table, and that queue comes back as it is (its first min(max(len, 0), max_len) bytes) while the others are
 * rewritten.  (RK_ESTATE there: a parent chain of the ball is broken.)  RK_ESTATE if the ball is not built, RK_EINVAL for a
 * null pointer or a size out of range.  Stream-ordered, no synchronisation. */
int rk_bshorten(rk_ball_t *h, const int8_t *d_actions, const int32_t *d_len, size_t n, int max_len, int window, int8_t *d_out_actions,
                int32_t *d_out_len, int32_t *d_error, void *d_scratch, size_t scratch_bytes, void *stream);

/* ---- shortest solutions by a one-sided breadth-first search from the start that ends at the ball ------------------------
 * rk_bfs's protocol in a pool of its own (node 1 = the start), one level at a time: a child the own pool holds is skipped,
 * a child the BALL holds is the meeting -- the search ends (won), the child is not stored, the lowest batch position wins
 * --, any other is appended.  Before every pop: n_states >= max_states ends the search (not won).  A start at distance
 * D > radius meets at level D - radius in a node of ball depth `radius`, so the first meeting is a shortest solution.  A
 * start that the ball holds is answered at the reset, without a pop.  Results do not depend on `pops`.  Several searches may
 * share one ball; a handle is not thread-safe. */
typedef struct rk_bsearch rk_bsearch_t;
/* capacity: size C (>= 2) of the own pool, whose table is sized to it; attaches to `ball` (built or not). */
int rk_bsearch_create(rk_bsearch_t **out, rk_ball_t *ball, size_t capacity, int pops);
int rk_bsearch_destroy(rk_bsearch_t *h);
/* Node 1 = the host 20-byte start state, with the state budget max_states.  Clears the own table, never the ball's;
 * RK_ESTATE if the ball is not built.  Synchronises. */
int rk_bsearch_reset(rk_bsearch_t *h, const int8_t *h_start_state, long long max_states, void *stream);
/* As rk_bibfs_run. */
int rk_bsearch_run(rk_bsearch_t *h, int iterations, void *stream);
/* Synchronises; h_status[10] = done, won, n_states, iterations, nodes popped, stop reason (0 running, 1 met, 2 budget,
 * 3 graph exhausted, 4 error), error, nodes the next iteration pops, complete levels, the meeting node IN THE BALL (0 if
 * none; the start's own node when the ball holds the start). */
int rk_bsearch_status(rk_bsearch_t *h, long long *h_status, void *stream);
/* Grows the own pool to new_capacity states in place between iterations, as rk_bfs_grow does. */
int rk_bsearch_grow(rk_bsearch_t *h, size_t new_capacity, void *stream);
/* Number of stored states of the own pool.  Synchronises. */
long long rk_bsearch_size(const rk_bsearch_t *h);
/* Rows [first, first+count) of the own pool to HOST buffers (any may be NULL), as rk_bfs_export. */
int rk_bsearch_export(rk_bsearch_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions,
                      void *stream);
/* The action queue of a search that met, start -> solved: the path to the popped parent, the meeting action, then the
 * ball's path from the meeting node; walked on the device.  Returns its length or a negative error (RK_ESTATE: not met);
 * writes at most max_len actions. */
long long rk_bsearch_path(rk_bsearch_t *h, long long *h_actions, size_t max_len, void *stream);

/* ---- many such searches in lock-step (rk_bsearchb_*) --------------------------------------------------------------------
 * n_slots slots, each a whole rk_bsearch of its own -- pool, table sized to it, counters, batch scratch --, advanced by the
 * same four launches with the slot in the grid's second dimension; all read one ball.  Every slot computes exactly what
 * rk_bsearch computes for its start.  A slot that is done or was never started costs one counter read per launch.  The
 * capacity is fixed per slot: a slot whose next iteration might not fit (n_states + 12 * pops of it > capacity) stops before
 * that iteration with stop reason 5 = pool full: done, not won, no error, the other slots undisturbed. */
typedef struct rk_bsearchb rk_bsearchb_t;
/* n_slots 1..1024, capacity_per_slot >= 2, pops 1..2^22; attaches to `ball` (built or not): rk_ball_destroy refuses meanwhile. */
int rk_bsearchb_create(rk_bsearchb_t **out, rk_ball_t *ball, int n_slots, size_t capacity_per_slot, int pops);
int rk_bsearchb_destroy(rk_bsearchb_t *h);
/* Between iterations: slot slots[j] (all different, 0 .. n_slots - 1) starts again from HOST state j of h_start_states int8
 * (n, 20) with the budget max_states[j].  Clears the tables and counters of the named slots only; every other slot stays
 * exactly where it was.  A start the ball holds is answered here.  RK_ESTATE if the ball is not built.  Synchronises. */
int rk_bsearchb_reset(rk_bsearchb_t *h, int n, const int32_t *slots, const int8_t *h_start_states, const long long *max_states,
                      void *stream);
/* `iterations` iterations of all slots, four launches each; stream-ordered, no synchronisation. */
int rk_bsearchb_run(rk_bsearchb_t *h, int iterations, void *stream);
/* Synchronises; h_status (n_slots, 10): rk_bsearch_status's ten words of every slot (zeros for a slot never started), read
 * with one copy.  Stop reason 5 = pool full. */
int rk_bsearchb_status(rk_bsearchb_t *h, long long *h_status, void *stream);
/* Row s of HOST h_out int32 (n_slots, 1 + max_len): the length of slot s's action queue, or -1 if it has not met, then its
 * first max_len actions.  max_len 0..4096.  One launch, one thread per slot, and one copy.  Synchronises. */
int rk_bsearchb_paths(rk_bsearchb_t *h, int32_t *h_out, int max_len, void *stream);
/* Rows [first, first+count) of slot `slot`'s pool to HOST buffers (any may be NULL), as rk_bsearch_export. */
int rk_bsearchb_export(rk_bsearchb_t *h, int slot, size_t first, size_t count, int8_t *h_states, long long *h_parents,
                       long long *h_actions, void *stream);

/* ---- the 48 symmetries of the cube: conjugates and canonical representatives (rk_sym_*) ------------------------------------
 * A face is 2 * axis + side (F B | T D | L R).  Symmetry s = 8 * p + m sends axis ax to P[p][ax], P = the six permutations of
 * 0 1 2 in lexicographic order, and swaps the two faces of source axis ax when bit ax of m is set; s = 0 is the identity.  A
 * symmetry relabels the actions (a turn of face f becomes a turn of its image, in the opposite sense under a reflection) and the
 * relabelling keeps the distance to solved.  The conjugate of a 20-byte state x is
 *     conj_s(x)[c] = map[s][c][x[src[s][c]]]            conj_s(rotate(x, a)) = rotate(conj_s(x), actions[s][a])
 * and the canonical representative of x the smallest of its 48 conjugates, compared as the tuple of the state's five
 * little-endian dwords, dword 0 first.  All tables are derived from the face definitions and the move table at compile time. */
/* HOST: actions uint8 (48, 12), src uint8 (48, 20), map uint8 (48, 20, 24); any may be NULL, not all.  Touches no device. */
int rk_sym_tables(uint8_t *h_actions, uint8_t *h_src, uint8_t *h_map);
/* Of every DEVICE state of d_states int8 (n, 20): d_rep int8 (n, 20) the representative, d_sym uint8 (n) the lowest symmetry
 * that gives it, d_orbit uint8 (n) the size of the state's orbit = 48 / the number of symmetries that give it.  Any output may
 * be NULL.  One launch, a wave per state; stream-ordered, no synchronisation. */
int rk_sym_canonical(const int8_t *d_states, size_t n, int8_t *d_rep, uint8_t *d_sym, uint8_t *d_orbit, void *stream);
/* d_out int8 (n, 20) = conj_sym of every DEVICE state of d_states, sym 0..47.  One launch; stream-ordered. */
int rk_sym_conjugate(const int8_t *d_states, size_t n, int sym, int8_t *d_out, void *stream);

/* ---- the cube group on 20-byte states: composition, inverse, a state seen from a goal, legality (rk_group_*) ----------------
 * A move permutes all 24 sticker slots of a kind (corner slot 3 * pos + k, edge slot 2 * pos + k), so a state b reached from
 * solved by a word has a full action g_b on the slots, the product of the word's moves.
 *     apply(a, b)[c]    = g_b(a[c])                  a's word, then b's; apply(s, solved moved by m) = s moved by m
 *     inverse(b)        : apply(b, inverse(b)) = apply(inverse(b), b) = solved
 *     relative(s, goal) = apply(inverse(goal), s)    relative(goal, goal) = solved; relative(rotate(s, m), goal) =
 *                                                    rotate(relative(s, goal), m): the distance from s to goal is the depth of it
 * For an edge g_b(2 p + k) = b[p] ^ k; for a corner g_b(3 p + k) = full[0][p][b[p]][k].  All tables are derived from the move
 * table at compile time.  Every entry below that launches is ONE launch, a thread per state, stream-ordered without
 * synchronisation; n at most INT32_MAX, n = 0 does nothing; device pointers 4-byte aligned.  The output may be exactly an operand
 * of n rows (a thread reads its operands before it stores); any other overlap of the output with an operand is RK_EINVAL.  A row
 * that is no legal state is read in bounds and gives an unspecified row: rk_group_legal is the entry that reports such rows. */
#define RK_GROUP_GRID 2048   /* workgroups of 256 states a launch has at most: beyond RK_GROUP_GRID * 256 states a thread takes several */
/* HOST: full uint8 (2, 12, 24, 3) = [kind][home][code][k] the slot g_b sends slot k of cubie `home` to when b[home] = code (corners:
 * homes 0..7; edges: k 0..1; zero elsewhere), inv uint8 (2, 12, 24) the slot of cubie `home` that g_b sends to the primary slot of
 * the position of `code`, tau uint8 (24) the twist of a corner code.  Any may be NULL, not all.  Touches no device. */
int rk_group_tables(uint8_t *h_full, uint8_t *h_inv, uint8_t *h_tau);
/* d_out int8 (n, 20) = apply(state i, effect i); n_effects = n, or 1: effect 0 for every state (RK_EINVAL otherwise). */
int rk_group_apply(const int8_t *d_states, size_t n, const int8_t *d_effects, size_t n_effects, int8_t *d_out, void *stream);
int rk_group_inverse(const int8_t *d_states, size_t n, int8_t *d_out, void *stream);
/* d_out int8 (n, 20) = relative(state i, goal i), inverse and apply in one pass; n_goals = n, or 1: goal 0 for every state. */
int rk_group_relative(const int8_t *d_states, size_t n, const int8_t *d_goals, size_t n_goals, int8_t *d_out, void *stream);
/* d_flags uint8 (n): 1 where row i is a state reachable from solved -- every code below 24, the corner and the edge positions
 * permutations of equal parity, an even number of flipped edges, corner twists that add up to 0 mod 3 --, 0 elsewhere.  d_stats
 * int64[2] (8-byte aligned; initialise to [0, INT64_MAX]): += the rows that are not, min= the lowest of them, as rk_686_to2024
 * counts.  Either may be NULL, not both. */
int rk_group_legal(const int8_t *d_states, size_t n, uint8_t *d_flags, long long *d_stats, void *stream);

/* ---- pattern databases: exact distances and solutions for partial goals (rk_pdb_*) -------------------------------------------
 * A pattern is a set of kc corner cubies (0..7) and ke edge cubies (0..11), each ascending, kc + ke >= 1; its goal is those
 * cubies at their home codes (3 c, 2 e), the others anywhere.  A move maps every cubie's code on its own, so the selected codes
 * of a state are closed under the 12 moves, and their space is small enough for a dense table of one byte per entry in HBM:
 * the exact number of quarter turns that bring the selected cubies home.  THE INDEX of the selected codes, over the selected
 * cubies of a kind in order (N = 8 or 12, position = code / 3 or code / 2, digit = code % 3 or code % 2):
 *     r = 0; for i in 0..k-1: d_i = p_i - #{j < i : p_j < p_i}; r = r * (N - i) + d_i          range P(N, k) = N! / (N - k)!
 *     o = 0; for i: o = o * 3 + digit_i (edges: * 2)                                            range O_c = 3^kc, 2^ke
 *     with all 8 corners the last corner's digit is left out (O_c = 3^7): the twists tau (rk_group_tables) add up to 0 mod 3
 *     index = ((r_c * O_c + o_c) * P(12, ke) + r_e) * 2^ke + o_e                                size = P(8, kc) O_c P(12, ke) 2^ke
 * Every entry of an accepted pattern is reachable, and the build checks it.  Queries are ONE launch, a thread per state under a
 * capped grid, stream-ordered without synchronisation; n at most INT32_MAX, n = 0 does nothing; device pointers 4-byte aligned.
 * A row whose SELECTED codes are no partial pattern -- a code outside 0..23, two selected cubies of a kind on one position --
 * is answered -1 before any table access; the other bytes of a row do not matter. */
#define RK_PDB_GRID 2048     /* workgroups of 256 states a query has at most: beyond RK_PDB_GRID * 256 states a thread takes several */
#define RK_PDB_MAX_SIZE 2147483648ULL
typedef struct rk_pdb rk_pdb_t;
/* h_corners uint8 (kc), h_edges uint8 (ke): the selected cubies, ascending (either may be NULL when its count is 0).  RK_EINVAL
 * for an empty pattern, a cubie out of range or out of order, ke >= 11 (the permutation parity would leave entries unreachable)
 * or a size above RK_PDB_MAX_SIZE.  Allocates nothing. */
int rk_pdb_create(rk_pdb_t **out, const uint8_t *h_corners, int kc, const uint8_t *h_edges, int ke);
int rk_pdb_destroy(rk_pdb_t *h);
/* Builds the table (nothing if it is built): level d is one sweep over the whole table, which stores d + 1 into the unreached
 * children of every entry equal to d and counts the entries of level d; the host reads that count after every level and stops
 * at the first empty one.  RK_ECAPACITY when the device has no room; RK_ESTATE unless the level sizes add up to the size and
 * level 0 holds one entry (the table is freed and the handle stays unbuilt).  Synchronises. */
int rk_pdb_build(rk_pdb_t *h, void *stream);
/* h_status[64] = built, size, kc, ke, levels, then the level sizes at [5 .. 5 + levels - 1] (zeros before the build and beyond).
 * Touches no device. */
int rk_pdb_status(rk_pdb_t *h, long long *h_status);
/* Entries [first, first+count) of the table to HOST h_bytes uint8 (count).  Synchronises. */
int rk_pdb_export(rk_pdb_t *h, size_t first, size_t count, uint8_t *h_bytes, void *stream);
/* d_depth[q] = the exact number of quarter turns that bring the selected cubies of DEVICE state q of d_states int8 (n, 20) home,
 * -1 for a row whose selected codes are no partial pattern. */
int rk_pdb_depth(rk_pdb_t *h, const int8_t *d_states, size_t n, int32_t *d_depth, void *stream);
/* A shortest word that brings the selected cubies home, by descent -- at each step the lowest action whose child's entry is one
 * less --: d_lengths[q] moves (-1 for an invalid row), row q of d_actions int8 (n, levels - 1) holds them, padded with -1.
 * d_error[0] is cleared, then set to RK_ESTATE if a reached entry has no such child (its length is -1 then; never in a table
 * that passed its build). */
int rk_pdb_solve(rk_pdb_t *h, const int8_t *d_states, size_t n, int32_t *d_lengths, int8_t *d_actions, int32_t *d_error, void *stream);
/* A bound over several databases (rk_bound_*): a pattern's entry never exceeds the distance to solved, so the greatest entry of
 * a state over 1..4 BUILT databases is an admissible lower bound on it.  The handle copies the databases' descriptors and
 * allocates nothing on the device; the databases must outlive it.  RK_EINVAL for n outside 1..4, a null database or the same
 * database twice, RK_ESTATE for a database that is not built. */
typedef struct rk_bound rk_bound_t;
int rk_bound_create(rk_bound_t **out, rk_pdb_t *const *dbs, int n);
int rk_bound_destroy(rk_bound_t *h);
/* d_bound[q] = the greatest of the databases' rk_pdb_depth of DEVICE state q of d_states int8 (n, 20), -1 only where every
 * database answers -1.  One launch, rk_pdb_depth's limits. */
int rk_bound_depth(rk_bound_t *h, const int8_t *d_states, size_t n, int32_t *d_bound, void *stream);

/* ---- the subgroup chain: a solution for every legal state (rk_chain_*) ---------------------------------------------------------
 * Four stages, each with a table of one byte per coset: the cost of the cheapest word of the stage's generators that brings a
 * state of that coset into the next subgroup.  A generator is a quarter turn (cost 1) or the half turn XX = the action 2 f twice
 * (cost 2); generators are ordered by their first action.  position = code / 3 (edges / 2), digit = code % 3 (% 2); slice s = the
 * four edges that neither face of an axis moves: 0 the axis F B, 1 the axis T D, 2 the axis L R (all read off the move table).
 *     stage  generators                  goal                                        THE INDEX                                   size
 *     1      the 12 quarter turns        every edge digit 0                          sum over positions p = 0..10 of             2^11
 *                                                                                    (digit of the edge AT p) << p
 *     2      F F' B B' TT DD L L' R R'   every corner digit 0, slice 0 on its        (sum over p = 0..6 of (digit of the corner  3^7 * 495
 *                                        positions                                   AT p) 3^p) * 495 + subset(positions of
 *                                                                                    slice 0's edges)
 *     3      F F' B B' TT DD LL RR       in the group of the six half turns          coset(P) * 70 + subset(positions of slice   420 * 70
 *                                                                                    1's edges, counted among the eight
 *                                                                                    positions outside slice 0)
 *     4      FF BB TT DD LL RR           solved                                      ((c3(P) * 24 + q_0) * 24 + q_1) * 24 + q_2  96 * 24^3
 * subset(S) = the ordinal of a set of four among the 4-subsets ordered by the largest element, then the next: the sum of
 * C(p_i, i + 1) over its elements ascending.  P = (position of corner cubie 0, .., 7); C3 = the 96 such sequences the half turns
 * reach from solved; coset(P) = the ordinal of the class {P o h, h in C3} by its lexicographically least member (420 classes);
 * c3(P) = the ordinal of P in C3, lexicographic; q_s = the lexicographic ordinal of (place of slice s's i-th edge within slice
 * s's positions, i = 0..3).  The tables reach exactly 2 048, 1 082 565, 29 400 and 663 552 entries; the rest stay 255.
 * A solution is four descents: per step the LOWEST generator whose entry equals the current entry minus its cost.  It is not
 * optimal; rk_ball_shorten / rk_symball_shorten improve it. */
#define RK_CHAIN_GRID 2048   /* workgroups of 256 states a solve has at most: beyond RK_CHAIN_GRID * 256 states a thread takes several */
typedef struct rk_chain rk_chain_t;
/* Builds the four tables and the two corner maps (coset, c3) on the HOST -- level d + 1 takes the cost-1 children of level d and
 * the cost-2 children of level d - 1 and stores only over unreached entries -- and uploads them on `stream`.  RK_ESTATE unless C3
 * has 96 sequences in 420 cosets and every table reaches exactly the count above with one entry 0; RK_ECAPACITY when the device
 * has no room for the 2.5 MB.  Synchronises. */
int rk_chain_create(rk_chain_t **out, void *stream);
int rk_chain_destroy(rk_chain_t *h);
/* h_status[16] = the four reached counts, the four deepest entries at [4..7], max_length (their sum: the row stride of
 * rk_chain_solve) at [8], the four table sizes at [9..12].  Touches no device. */
int rk_chain_status(rk_chain_t *h, long long *h_status);
/* Entries [first, first+count) of the table of `stage` (1..4) to HOST h_bytes uint8 (count).  Synchronises. */
int rk_chain_export(rk_chain_t *h, int stage, size_t first, size_t count, uint8_t *h_bytes, void *stream);
/* ONE launch, a thread per state under a capped grid, stream-ordered without synchronisation; n at most INT32_MAX, n = 0 does
 * nothing at all; d_states, d_lengths, d_stage_lengths, d_error 4-byte aligned.  Row q of d_states int8 (n, 20): d_lengths[q] =
 * the length of its solution, whose actions are the first d_lengths[q] bytes of row q of d_actions int8 (n, max_length); the
 * bytes beyond are NOT written.  d_stage_lengths int32 (n, 4), or NULL: the cost of each stage.  A row that is no legal state
 * (rk_group_legal's test, made before any table is read) gets length -1, stage lengths -1 and no action.  d_error int32[1], or
 * NULL: set to -1, then to the lowest row that got -1. */
int rk_chain_solve(rk_chain_t *h, const int8_t *d_states, size_t n, int32_t *d_lengths, int8_t *d_actions, int32_t *d_stage_lengths,
                   int32_t *d_error, void *stream);

/* ---- two-phase search: short solutions for every legal state (rk_twophase_*) --------------------------------------------------
 * IDA* into the subgroup H = <F, B, TT, DD, LL, RR> (phase 1 = the chain's stages 1 + 2, the 12 quarter turns at cost 1), then
 * IDA* inside it (phase 2 = stages 3 + 4, the generators F F' B B' (1) TT DD LL RR (2) in the chain's stage-3 order); the chain's
 * answer is every row's first best, so an answer is never longer than rk_chain_solve's.  Four pruning tables, one byte per entry,
 * the exact cost under the phase's generators; coordinates BY POSITION as the chain's (above):
 *     table  phase  THE INDEX                                                                                    size        reached
 *     1      1      twist * 495 + slice = the index of the chain's stage 2                                       2187 * 495  1 082 565
 *     2      1      flip * 495 + slice, flip = the index of the chain's stage 1, slice = subset(positions of     2048 * 495  1 013 760
 *                   slice 0's edges)
 *     3      2      corners * 24 + places, corners = the lexicographic rank of P, places = q_0                   40320 * 24  967 680
 *     4      2      edges * 24 + places, edges = the lexicographic rank of (place of the i-th edge outside       40320 * 24  967 680
 *                   slice 0 among the eight positions outside slice 0, i = 0..7)
 * MOVE PRUNING (both phases; a generator is named by its action a, a half turn by the even action; last, last2 = the two
 * generators before it in the same phase): a is skipped if a == last ^ 1; if its face is the lower one of last's axis and last's
 * face the upper (opposite faces commute: lower face first); if a == last and a is odd (X'X' = XX); if a == last == last2 (XXX);
 * if a == last is a half turn of phase 2.  A cheapest word per element survives, so a phase's first solution is optimal for it.
 * Children are taken in ascending order of a.
 * THE SEARCH of a state: best = the chain's length; D = its phase-1 entry (the greater of tables 1 and 2); while D < best: depth-
 * first over the phase-1 words of exactly D generators (a child is kept if depth + entry <= D), each of which ends in H and is a
 * phase-1 solution p1 = D: for D2 = the phase-2 entry of the state behind it (the greater of tables 3 and 4) .. best - p1 - 1,
 * depth-first over phase-2 words (a child is kept if cost + entry <= D2) up to the first child whose entry is 0: best = p1 + cost,
 * the row is rewritten.  After the phase 2 of the `tries`-th phase-1 solution, or once D >= best, the search is over.
 * WITH A CAP C on the phase-2 bound (rk_twophase_solve_capped) two conditions change and nothing else does: a phase-1 solution
 * whose phase-2 entry h2 is not 0 is left behind, and phase 1 goes on, if p1 + h2 >= best OR h2 > C (without a cap: the first
 * alone); and when a phase-2 bound is exhausted, D2 += 1, phase 1 goes on if p1 + D2 >= best OR D2 > C.  Every phase-1 solution
 * still counts towards `tries`, and one whose h2 is 0 still ends the search.
 * THE BUDGET: a node is one child evaluation (a generator the move pruning lets through, its coordinates stepped, its two entries
 * read) in either phase.  Immediately before each evaluation the state's counter is compared with max_nodes: if equal the search
 * of that state ends, otherwise the counter goes up by one.  Nothing else counts.  The answer is a function of (state, tries,
 * max_nodes) alone; with a cap, of (state, tries, max_nodes, C). */
#define RK_TWOPHASE_GRID 1024   /* workgroups of 256 lanes the search has at most; a lane that ends a state takes the next row */
typedef struct rk_twophase rk_twophase_t;
/* Builds six u16 move tables (a coordinate under every generator) and the four pruning tables on the HOST -- level d + 1 takes the
 * cost-1 children of level d and the cost-2 children of level d - 1 and stores only over unreached entries -- and uploads them on
 * `stream` (5.6 MB).  RK_ESTATE unless every coordinate takes every value under its generators and every table reaches exactly the count
 * above with one entry 0; RK_ECAPACITY when the device has no room.  Synchronises. */
int rk_twophase_create(rk_twophase_t **out, void *stream);
int rk_twophase_destroy(rk_twophase_t *h);
/* h_status[16] = the four reached counts, the four deepest entries at [4..7], the four table sizes at [8..11], RK_TWOPHASE_GRID
 * at [12], the workgroup size at [13], the longest row the search's stack holds at [14].  Touches no device. */
int rk_twophase_status(rk_twophase_t *h, long long *h_status);
/* Entries [first, first+count) of pruning table `table` (1..4) to HOST h_bytes uint8 (count).  Synchronises. */
int rk_twophase_export(rk_twophase_t *h, int table, size_t first, size_t count, uint8_t *h_bytes, void *stream);
/* TWO launches, stream-ordered without synchronisation: rk_chain_solve(chain, d_states, n, d_lengths, d_actions, NULL, d_error)
 * with its limits and its treatment of rows that are no legal state, then the search, which replaces a row by every strictly
 * shorter answer it finds (the bytes from the new length up to the length the row had are set to -1; the bytes beyond are not
 * written).  tries >= 1, max_nodes >= 1.  d_phase_lengths int32 (n, 2): the moves of the answer before and inside H -- for a row
 * that still holds the chain's answer the cost of its stages 1 + 2 and 3 + 4 --, -1 -1 for a row that is no legal state.
 * d_reason int32 (n): 0 the search ended by itself and improved the chain's answer, 1 the budget ended it and the answer is from
 * the search, 2 the row still holds the chain's answer.  d_nodes int64 (n, 8-byte aligned): the state's counter.  One handle
 * serves one solve at a time (it owns the row counter).  RK_ESTATE if the chain's rows are wider than [14] of the status. */
int rk_twophase_solve(rk_twophase_t *h, rk_chain_t *chain, const int8_t *d_states, size_t n, int tries, long long max_nodes, int32_t *d_lengths,
                      int8_t *d_actions, int32_t *d_phase_lengths, int32_t *d_reason, long long *d_nodes, int32_t *d_error, void *stream);
/* rk_twophase_solve with a cap on the phase-2 bound (the two changed conditions above) and two counts per row.  phase2_cap <= 0:
 * no cap, every output as rk_twophase_solve's; a cap above [14] of the status is RK_EINVAL.  With a cap `tries` is no longer what
 * ends a search, so callers pass a large value.  d_counts int32 (n, 2), 4-byte aligned, or NULL: the phase-1 solutions the search
 * found and the phase-2 searches it entered (entered <= found <= tries), written once when the row's search ends; 0 0 for a row
 * that is no legal state.  Everything else is rk_twophase_solve's, which is this entry with phase2_cap 0 and d_counts NULL. */
int rk_twophase_solve_capped(rk_twophase_t *h, rk_chain_t *chain, const int8_t *d_states, size_t n, int tries, long long max_nodes, int phase2_cap,
                             int32_t *d_lengths, int8_t *d_actions, int32_t *d_phase_lengths, int32_t *d_reason, long long *d_nodes,
                             int32_t *d_counts, int32_t *d_error, void *stream);

/* ---- the symmetry-reduced goal ball: one representative per orbit (rk_symball_*) -------------------------------------------
 * The canonical representatives of the states within `radius` quarter turns of solved, built once and kept in HBM; the depth of
 * a representative is the depth of the up to 48 states of its orbit.  Node 1 is the solved state, the pool is in index order: a
 * level's representatives are popped in index order, never across a level boundary, their children taken in action order 0..11
 * and canonicalised; a representative the pool holds is skipped, every other is appended.  Level `radius` is stored and never
 * expanded; level l is the index range level_start[l] .. level_start[l + 1] - 1.  There are no parents and no actions: a
 * solution is found by descent.  The orbit sizes of every level are added up; the sums of levels 0..8 are checked against the
 * level sizes of the graph (see rk_ball_*), those of levels 9 and 10 are only reported.  The pool does not depend on `pops`. */
typedef struct rk_symball rk_symball_t;
/* radius 0..10; pops 1..2^22; capacity: orbits the pool can hold, 0 = the sum over the levels of ceil(level size / 48 * 1.02)
 * + 64.  Allocates nothing. */
int rk_symball_create(rk_symball_t **out, int radius, int pops, size_t capacity);
/* RK_ESTATE while a search (rk_ssearch_*, rk_ssearchb_*) is attached to the ball. */
int rk_symball_destroy(rk_symball_t *h);
/* Builds the ball (nothing if it is built): iterations of five launches, the host looks every `poll` of them.  An iteration pops
 * only as many representatives as fit the pool whatever their children are; when not one fits, the build stops before that
 * iteration with RK_ECAPACITY (nothing is written out of bounds, the ball stays unbuilt and its arrays are freed).  RK_ECAPACITY
 * also when the device has no room; a level whose orbit sizes do not add up is an engine error (RK_ESTATE).  Synchronises. */
int rk_symball_build(rk_symball_t *h, int poll, void *stream);
/* h_status[32] = built, orbits stored, iterations of the build, radius, capacity, table slots, level_start[0 .. 11] (zeros
 * before the build and beyond radius + 1), then at [18 .. 28] the orbit sizes of levels 0 .. 10 added up.  Touches no device. */
int rk_symball_status(rk_symball_t *h, long long *h_status);
/* Rows [first, first+count) of the pool to HOST h_states int8 (count, 20). */
int rk_symball_export(rk_symball_t *h, size_t first, size_t count, int8_t *h_states, void *stream);
/* d_depth[q] = exact distance to solved of DEVICE state q of d_states int8 (n, 20), -1 for a state outside the ball.  One
 * launch, a wave per query, nothing of the ball is written; stream-ordered, no synchronisation. */
int rk_symball_depth(rk_symball_t *h, const int8_t *d_states, size_t n, int32_t *d_depth, void *stream);
/* A shortest solution of every DEVICE state of d_states by descent -- at each step the lowest action whose child lies one level
 * nearer --: d_lengths[q] moves (-1 outside the ball), row q of d_actions int8 (n, radius) holds them, padded with -1.
 * d_error[0] is cleared, then set to RK_ESTATE if a state inside the ball has no such child (its length is -1 then; never in a
 * ball that passed its build).  One launch; stream-ordered, no synchronisation. */
int rk_symball_solve(rk_symball_t *h, const int8_t *d_states, size_t n, int32_t *d_lengths, int8_t *d_actions, int32_t *d_error,
                     void *stream);
/* Exact values for the children of an Autodidactic-Iteration rollout (train.py:301-314: the value of every child, before the
 * reward is added and the maximum over twelve siblings is taken).  d_states int8 (m12, 20) are rk_rollout_fanout's d_children
 * where they lie, m12 a multiple of 12 and at most INT32_MAX; g is the goal reward of the method (0 for reward0, else 1).  With
 * c = rk_symball_depth's answer for a row (0..radius, -1 outside the ball):
 *   d_depth   int8 (m12)      c of every row
 *   d_values  float32 (m12)   V*(0) = 0, V*(c) = g - (c - 1) for 1 <= c <= radius, written at the rows with c >= 0; the rows with
 *                             c < 0 are NOT TOUCHED (the caller scatters the net's values there)
 *   d_rows    int32 (m12)     the indices of the rows with c < 0 IN ASCENDING ORDER, the first d_count[0] entries
 *   d_outside int8 (m12, 20)  those rows' states in the same order, the first d_count[0] rows: the net's batch, no gather needed
 *   d_count   int32 (1)       how many rows lie outside the ball
 * V* is the fixed point of V(s) = max_a [r(s.a) + V(s.a)] with V(solved) = 0.  The order of d_rows is part of the contract (the
 * net's slices are cut from it): the compaction is a scan over tiles of 256 rows, not a counter.  d_scratch: device memory of
 * rk_symball_child_values_scratch_bytes(m12) bytes (one word per tile), 4-byte aligned as every other pointer.  Four launches --
 * a wave per child as rk_symball_depth, the tiles' counts, their prefix, the write --; the ball is only read.  Stream-ordered, no
 * synchronisation.  RK_EINVAL for null or misaligned pointers, m12 no multiple of 12 or above INT32_MAX, too little scratch;
 * RK_ESTATE for a ball that is not built; all before any launch. */
int rk_symball_child_values(rk_symball_t *h, const int8_t *d_states, size_t m12, float g, int8_t *d_depth, float *d_values, int32_t *d_rows,
                            int8_t *d_outside, int32_t *d_count, void *d_scratch, size_t scratch_bytes, void *stream);
/* Bytes of d_scratch for m12 children: 4 * ceil(m12 / 256); RK_EINVAL above INT32_MAX.  Touches no device. */
long long rk_symball_child_values_scratch_bytes(size_t m12);
/* Unranking the ball.  THE STATE OF (d, r), 0 <= d <= radius, 0 <= r < (the orbit sizes of level d added up, status word 18 + d),
 * is the k-th distinct conjugate, in ascending symmetry order, of the node j of level d whose cumulative orbit range holds r:
 * with the nodes of level d in index order and their orbit sizes o(j), j is the node with sum_{i < j} o(i) <= r < sum_{i <= j} o(i)
 * and k = r - sum_{i < j} o(i); the distinct conjugates of j's representative are conj_s of it for the symmetries s = 0 .. 47 in
 * that order, a conjugate that a lower symmetry gave already left out.  For every d the map r -> state is a bijection onto the
 * states at distance d from solved; like the pool it does not depend on `pops`.
 * Row i of DEVICE d_states int8 (n, 20) = the state of (d_depth[i], d_rank[i]), d_depth int32 (n), d_rank int64 (n, 8-byte
 * aligned), n at most INT32_MAX.  d_error[0] is cleared, then set to RK_EINVAL if a depth lies outside 0..radius or a rank outside
 * its level -- that row is written as zeros, every other row is right -- or to RK_ESTATE if the index contradicts the ball (never
 * after a call that passed).  One launch, a wave per sample; nothing is written but d_states and d_error; stream-ordered, no
 * synchronisation -- except in the first call on a ball, which makes the ORBIT INDEX and synchronises for it: one byte per orbit
 * (its orbit size) and a 64-bit prefix per 256 orbits, 161 MB at radius 10, kept in HBM until rk_symball_destroy.  The index is
 * made by four launches (a wave per node: the node must be its own canonical form) and accepted only if the orbit sizes of every
 * level add up to what the build reported (RK_ESTATE otherwise; RK_ECAPACITY when the device has no room; the ball stays usable
 * and without an index).  A ball that never samples allocates nothing for it. */
int rk_symball_state_at(rk_symball_t *h, const int32_t *d_depth, const int64_t *d_rank, size_t n, int8_t *d_states, int32_t *d_error,
                        void *stream);
/* h_status[16] = how often the orbit index was made (0 or 1), its bytes, its tiles, 0, then at [4 .. 15] the cumulative orbit
 * sizes below levels 0 .. 11: level d's ranks are word 4 + d .. word 5 + d of the global cumulative (zeros before the index is
 * made and beyond radius + 1).  Touches no device. */
int rk_symball_index_status(rk_symball_t *h, long long *h_status);
/* The exact distance to solved of every DEVICE state of d_states int8 (n, 20) and of its twelve children in action order:
 * d_depth int8 (n), d_child int8 (n, 12).  A quarter turn changes the distance by exactly one, so with R = radius and c =
 * rk_symball_depth's answer: a state with c >= 0 gets c, its children inside the ball their own c and the others c + 1 (= R + 1); a
 * state outside the ball with a child inside gets R + 1, its children inside R and the others R + 2; a state with no child
 * inside gets -1 thirteen times.  Every answer >= 0 is exact, and every state within R + 1 of solved gets one.  d_error[0] is
 * cleared, then set to RK_ESTATE if the levels around a state contradict the parity (never in a ball that passed its build).  One
 * launch, a wave per state, thirteen probes; the ball is only read; stream-ordered, no synchronisation.  All pointers but d_child
 * 4-byte aligned. */
int rk_symball_child_depths(rk_symball_t *h, const int8_t *d_states, size_t n, int8_t *d_depth, int8_t *d_child, int32_t *d_error,
                            void *stream);
/* Depth-first probes past the ball's radius: for every DEVICE state i of d_states int8 (n, 20) and every word of `extra` moves
 * (1..8) whose rank lies in [word_first, word_first + word_count), the word is applied to the state, the result canonicalised and
 * looked up in the ball; if the ball holds it, atomicMin(d_best[i], rank).  A word is a sequence of actions 0..11 in which no
 * action is the opposite turn (a ^ 1) of the one before it; "before the first" is d_last[i], the move that led to state i
 * (d_last NULL, or an entry outside 0..11 such as -1: the first move has all 12 choices).  Words are ranked in lexicographic
 * order of their actions, rank 0 first: 11^extra of them, 12 * 11^(extra-1) without a last action; ranks a state does not have
 * are skipped.  The caller fills d_best uint32 (n) with 0xFFFFFFFF before the first launch of a round; ranks above a state's
 * current d_best may be skipped, the result is the minimum either way.  If every state within extra - 1 moves of state i lies
 * outside the ball, a hit lies at ball depth `radius` exactly and radius + extra is the distance of state i to solved.
 * One launch -- a persistent grid, a wave per (state, 121 consecutive ranks), which share all but their last two moves --,
 * stream-ordered, no synchronisation; the ball is only read, nothing but d_best is written.  RK_EINVAL for extra outside 1..8 or
 * n * word_count above rk_sdeepen_max_probes(), RK_ESTATE for a ball that is not built. */
int rk_sdeepen(rk_symball_t *ball, const int8_t *d_states, const int8_t *d_last, size_t n, int extra, uint32_t word_first,
               uint32_t word_count, uint32_t *d_best, void *stream);
/* The most probes (n * word_count) of one rk_sdeepen / rk_sdeepen_nodes launch: 2^28, which keeps a launch well under a second
 * (benchmarks/symball_deepen.py measures a full launch).  Touches no device. */
long long rk_sdeepen_max_probes(void);
/* rk_sdeepen with its look-ups pruned by an admissible bound (rk_bound_*): d_best comes out as rk_sdeepen leaves it, bit for
 * bit.  With R the ball's radius, a word is dropped without a look-up where the bound of a state on its way shows that no state
 * of the ball lies behind it: bound > R + (moves still to make), tested at the start state, after every shared move, at the
 * next-to-last state and at the leaf.  A word that hits has no such prefix -- the state after k of its `extra` moves is at most
 * (extra - k) + R from solved, and the bound is admissible --, so the set of hits is rk_sdeepen's.  d_lookups (NULL: not
 * counted; else a DEVICE uint64, 8-byte aligned, which the caller zeroes) += the ball look-ups made, one atomic add per wave.
 * word_count counts the words ISSUED, pruned or not: rk_sdeepen's limits and return codes, plus RK_EINVAL for a null bound. */
int rk_sdeepen_pruned(rk_symball_t *ball, rk_bound_t *bound, const int8_t *d_states, const int8_t *d_last, size_t n, int extra,
                      uint32_t word_first, uint32_t word_count, uint32_t *d_best, unsigned long long *d_lookups, void *stream);
/* rk_bshorten against the symmetry ball: one pass over a batch of action queues, with rk_bshorten's contract (above) -- the
 * same arguments, limits, return codes and d_error semantics, scratch of rk_bshorten_scratch_bytes(n, max_len, window) bytes --
 * and d(i, j) = the symmetry ball's depth of X(i, j), i.e. the level of its representative.  That is the plain ball's d(i, j)
 * at the same radius, so the cost, the ties to the largest i and the copy rule give output lengths equal to rk_bshorten's
 * queue for queue; the radius may be 9 or 10.  The ball stores no word: a replaced window gets the INVERSE OF THE DESCENT --
 * with w = rk_symball_solve's word for X(i, j) (at each step the lowest action whose child's representative lies one level
 * nearer), w reversed with every action ^ 1, which leads from solved to X(i, j) and hence from s_i to s_j.  It may differ
 * from the plain ball's word for the same window; it has the same length.  d_error[0] = RK_ESTATE: a descent found no way on
 * or a level differs from the stored one (never in a ball that passed its build); that queue comes back as it is.  Three
 * launches: d(i, j) of all windows (a persistent grid, one canonical form and probe per window), the shortest path, the
 * rewritten queue.  The ball is only read.  Stream-ordered, no synchronisation. */
int rk_sshorten(rk_symball_t *h, const int8_t *d_actions, const int32_t *d_len, size_t n, int max_len, int window, int8_t *d_out_actions,
                int32_t *d_out_len, int32_t *d_error, void *d_scratch, size_t scratch_bytes, void *stream);

/* ---- shortest solutions by a one-sided breadth-first search from the start that ends at the symmetry ball (rk_ssearch_*) ----
 * rk_bsearch_* with one difference: "the ball holds this child" is "the symmetry ball holds the child's canonical
 * representative".  The own pool holds RAW states with parent and action (node 1 = the start); a child the own pool holds is
 * skipped, a child whose ORBIT the ball holds is the meeting -- the search ends (won), the child is not stored, the lowest batch
 * position wins --, any other is appended; the budget is checked before every pop.  A state lies in the plain ball of radius R
 * exactly when its representative lies in the symmetry ball of radius R, so the own pool, the complete levels, the nodes popped,
 * the iterations and the meeting child are those of rk_bsearch_* on a plain ball of the same radius; the ball's half of the
 * path is found by descent and has the same length.  An iteration is five launches: a wave per child for the canonical form and
 * the read-only probe of the ball, then rk_bsearch's four.  Entry for entry, arguments, limits, return codes and the status
 * words are rk_bsearch_*'s; several searches may share one ball; a handle is not thread-safe. */
typedef struct rk_ssearch rk_ssearch_t;
/* capacity: size C (>= 2) of the own pool, whose table is sized to it; pops 1..2^22.  RK_ESTATE if the ball is not built (the
 * search holds the built ball's arrays); attaches to `ball`: rk_symball_destroy refuses meanwhile. */
int rk_ssearch_create(rk_ssearch_t **out, rk_symball_t *ball, size_t capacity, int pops);
int rk_ssearch_destroy(rk_ssearch_t *h);
/* Node 1 = the host 20-byte start state, with the state budget max_states.  Clears the own table, never the ball's.  A start
 * whose orbit the ball holds is answered here, without a pop.  Synchronises. */
int rk_ssearch_reset(rk_ssearch_t *h, const int8_t *h_start_state, long long max_states, void *stream);
/* As rk_bsearch_run, five launches per iteration. */
int rk_ssearch_run(rk_ssearch_t *h, int iterations, void *stream);
/* Synchronises; h_status[10] as rk_bsearch_status; the meeting node is the node of the REPRESENTATIVE of the meeting child (or
 * of the start) in the symmetry ball. */
int rk_ssearch_status(rk_ssearch_t *h, long long *h_status, void *stream);
/* Grows the own pool to new_capacity states in place between iterations, as rk_bsearch_grow. */
int rk_ssearch_grow(rk_ssearch_t *h, size_t new_capacity, void *stream);
/* Number of stored states of the own pool.  Synchronises. */
long long rk_ssearch_size(const rk_ssearch_t *h);
/* Rows [first, first+count) of the own pool to HOST buffers (any may be NULL), as rk_bsearch_export. */
int rk_ssearch_export(rk_ssearch_t *h, size_t first, size_t count, int8_t *h_states, long long *h_parents, long long *h_actions,
                      void *stream);
/* The action queue of a search that met, start -> solved: the path to the popped parent, the meeting action, then the descent
 * from the meeting state through the ball -- at each step the lowest action whose child's representative lies one level nearer,
 * at most `radius` steps; walked on the device by one wave.  Returns its length or a negative error (RK_ESTATE: not met, or a
 * state on the way down has no such child); writes at most max_len actions. */
long long rk_ssearch_path(rk_ssearch_t *h, long long *h_actions, size_t max_len, void *stream);

/* Deepening: how a search whose pool is full goes on.  The pool's newest complete level is the frontier; words from its nodes
 * are probed against the ball by rk_sdeepen's launch, and the first round `extra` with a hit gives a shortest solution of
 * length (level + extra + radius).
 * rk_sdeepen_set_pops: the iterations to come pop at most `pops` nodes (1 .. the pops of rk_ssearch_create); no result depends
 * on it.  A host whose pool cannot take 12 * pops more states lowers it to complete as many levels as fit; a reset restores the
 * created value.  One launch of one thread, stream-ordered. */
int rk_sdeepen_set_pops(rk_ssearch_t *h, int pops, void *stream);
/* h_out[2] = the first and the last node of the newest complete level of the own pool (nodes behind the last are a partial next
 * level).  Reads the counters on `stream` and synchronises it, as rk_ssearch_status; call it between iterations. */
int rk_sdeepen_frontier(rk_ssearch_t *h, long long *h_out, void *stream);
/* rk_sdeepen on the pool rows node_first .. node_first + node_count - 1, d_last = the stored action of each node, none for
 * node 1; d_best[k] belongs to node node_first + k.  The rows must lie inside 1..capacity (RK_EINVAL otherwise: no launch reads
 * outside the pool's arrays), and the caller keeps them inside rk_sdeepen_frontier's range: the entry does not wait for the
 * counters, so a row behind n_states is probed as whatever bytes it holds and its d_best means nothing.  rk_sdeepen's limits
 * and return codes. */
int rk_sdeepen_nodes(rk_ssearch_t *h, int extra, size_t node_first, size_t node_count, uint32_t word_first, uint32_t word_count,
                     uint32_t *d_best, void *stream);
/* rk_sdeepen_nodes with rk_sdeepen_pruned's launch: the same d_best, fewer look-ups, d_lookups as there. */
int rk_sdeepen_nodes_pruned(rk_ssearch_t *h, rk_bound_t *bound, int extra, size_t node_first, size_t node_count, uint32_t word_first,
                            uint32_t word_count, uint32_t *d_best, unsigned long long *d_lookups, void *stream);
/* The action queue start -> `node` -> word `rank` of `extra` moves -> descent through the ball, walked by one wave as
 * rk_ssearch_path.  Returns its length or a negative error: RK_EINVAL for a node outside 1..n_states or extra outside 1..8,
 * RK_ESTATE if the node has no such word or the ball does not hold the moved state's representative.  Synchronises. */
long long rk_sdeepen_path(rk_ssearch_t *h, long long node, int extra, uint32_t rank, long long *h_actions, size_t max_len,
                                 void *stream);

/* ---- many such searches in lock-step (rk_ssearchb_*) --------------------------------------------------------------------
 * rk_bsearchb_* for rk_ssearch: n_slots slots, each a whole rk_ssearch of its own -- pool, table sized to it, counters, batch
 * scratch, the words of the probe launch --, advanced by the same five launches with the slot in the grid's second dimension;
 * all read one symmetry ball.  Every slot computes exactly what rk_ssearch computes for its start, hence what a slot of
 * rk_bsearchb computes on a plain ball of the same radius (but for the ball's half of the queue, which has the same length).  A
 * slot that is done or was never started costs one counter read per launch and stages no table.  The capacity is fixed per
 * slot, with rk_bsearchb's rule: a slot whose next iteration might not fit (n_states + 12 * pops of it > capacity) stops before
 * that iteration with stop reason 5 = pool full: done, not won, no error, the other slots undisturbed.  Entry for entry the
 * arguments, limits and return codes are rk_bsearchb_*'s. */
typedef struct rk_ssearchb rk_ssearchb_t;
/* n_slots 1..1024, capacity_per_slot 2..0x3FFFFFF0, pops 1..2^22.  RK_ESTATE if the ball is not built (nothing is made or
 * attached); attaches to `ball`: rk_symball_destroy refuses meanwhile. */
int rk_ssearchb_create(rk_ssearchb_t **out, rk_symball_t *ball, int n_slots, size_t capacity_per_slot, int pops);
int rk_ssearchb_destroy(rk_ssearchb_t *h);
/* Between iterations: slot slots[j] (all different, 0 .. n_slots - 1) starts again from HOST state j of h_start_states int8
 * (n, 20) with the budget max_states[j].  Clears the tables and counters of the named slots only; every other slot stays
 * exactly where it was.  A start whose orbit the ball holds is answered here, with nothing popped.  One wave per named slot.
 * Synchronises. */
int rk_ssearchb_reset(rk_ssearchb_t *h, int n, const int32_t *slots, const int8_t *h_start_states, const long long *max_states,
                      void *stream);
/* `iterations` iterations of all slots, five launches each; stream-ordered, no synchronisation. */
int rk_ssearchb_run(rk_ssearchb_t *h, int iterations, void *stream);
/* Synchronises; h_status (n_slots, 10): rk_ssearch_status's ten words of every slot (zeros for a slot never started), read with
 * one copy; word 9 is the node of the meeting's representative in the symmetry ball.  Stop reason 5 = pool full. */
int rk_ssearchb_status(rk_ssearchb_t *h, long long *h_status, void *stream);
/* Row s of HOST h_out int32 (n_slots, 1 + max_len): the length of slot s's action queue, then its first max_len actions; -1 for
 * a slot that has not met, -2 where rk_ssearch_path reports RK_ESTATE for a search that met (the meeting state is not where the
 * search says, or a state on the way down has no child one level nearer).  max_len 0..4096.  One launch, one wave per slot, and
 * one copy.  Synchronises. */
int rk_ssearchb_paths(rk_ssearchb_t *h, int32_t *h_out, int max_len, void *stream);
/* Rows [first, first+count) of slot `slot`'s pool to HOST buffers (any may be NULL), as rk_ssearch_export. */
int rk_ssearchb_export(rk_ssearchb_t *h, int slot, size_t first, size_t count, int8_t *h_states, long long *h_parents,
                       long long *h_actions, void *stream);

/* Deepening in the batch: a slot whose pool is full goes on from its newest complete level by rk_sdeepen's probes, beside the
 * slots that still pop; one launch serves every such slot.
 * rk_sdeepenb_set: the pool-full rule of the slots that rk_ssearchb_reset starts from now on (off at creation; no
 * launch).  On: a slot whose next iteration might not fit pops only as many nodes as surely fit, min(pops, (capacity -
 * n_states) / 12), and stops with reason 5 only when not even one does -- its pool, popped nodes and levels are then those of
 * pops = 1, whatever the engine's pops.  Off: rk_ssearchb's rule above, launch for launch.  Refuses a null engine. */
int rk_sdeepenb_set(rk_ssearchb_t *h, int on);
/* h_out (n_slots, 2) = the first and the last node of every slot's newest complete level (zeros for a slot never started).
 * Reads the counters on `stream` and synchronises it.  The engine remembers the level and the size of every slot that is done
 * at this read -- such a slot stands still until its next reset --; rk_sdeepenb_probe and rk_sdeepenb_paths check their
 * arguments against that and refuse (RK_ESTATE) a slot that was running at the last call of this entry or was reset since. */
int rk_sdeepenb_frontiers(rk_ssearchb_t *h, long long *h_out, void *stream);
/* A job of rk_sdeepenb_probe: the words word_first .. word_first + word_count - 1 of `extra` moves behind the nodes node_first ..
 * node_first + node_count - 1 of slot `slot`, each node's stored action as its last move (none for node 1).  new_round != 0:
 * the slot's key is "none" before this launch lowers it; 0: the key goes on from the launches before. */
typedef struct rk_deepen_job {
	int32_t slot, extra;
	uint32_t node_first, node_count, word_first, word_count;
	uint32_t new_round, reserved;
} rk_deepen_job_t;
/* One launch over n_jobs HOST jobs, stream-ordered, no synchronisation: every result is canonicalised and looked up in the ball,
 * and a slot keeps ONE 64-bit key, the lowest (node << 32 | rank) that hit -- the lowest node with a hit and that node's
 * lowest word.  A (node, rank) above the slot's key is skipped.  Jobs of one launch may be in different rounds.  Nothing of a
 * pool or of the ball is written.  Checked on the host before anything runs, RK_EINVAL with no launch and no key changed:
 * n_jobs outside 0..n_slots, null jobs, a slot out of range or named twice, extra outside 1..8, a node range that is empty or
 * not inside the slot's frontier as rk_sdeepenb_frontiers last read it, a word range that is empty or not inside the words of
 * `extra` moves (12 * 11^(extra-1) for a frontier that is node 1, else 11^extra), and more than rk_sdeepen_max_probes() probes
 * (the sum of node_count * word_count) in the launch.  RK_ESTATE: the ball is not built, a slot was not done at the last
 * rk_sdeepenb_frontiers or was reset since, or a slot's first job since its reset does not set new_round. */
int rk_sdeepenb_probe(rk_ssearchb_t *h, int n_jobs, const rk_deepen_job_t *h_jobs, void *stream);
/* h_out[n_slots] = every slot's key of its current round, all ones for none (and for a slot without a round).  Synchronises.
 * Refuses null arguments. */
int rk_sdeepenb_keys(rk_ssearchb_t *h, unsigned long long *h_out, void *stream);
/* Row j of HOST h_out int32 (n, 1 + max_len): rk_sdeepen_path for slot slots[j], node nodes[j], extras[j] moves, word ranks[j]
 * -- the length, then the first max_len actions; -1 when the node has no such word or a parent chain is broken, -2 when the
 * word does not lead into the ball.  One launch, one wave per row, one copy.  Synchronises.  RK_EINVAL with no launch: null
 * arguments, n outside 0..n_slots, a slot out of range, a node outside 1..n_states of its slot, extra outside 1..8, max_len
 * outside 0..4096; RK_ESTATE for a slot that rk_sdeepenb_probe would refuse for the same reason. */
int rk_sdeepenb_paths(rk_ssearchb_t *h, int n, const int32_t *slots, const long long *nodes, const int32_t *extras,
                             const uint32_t *ranks, int32_t *h_out, int max_len, void *stream);

/* ---- device-resident epsilon-greedy value maximisation (agents.py:649-726) ---------------------------------------
 * W = workers walkers take D = depth moves from a root (:692-715); the visited state with the best value becomes the next
 * root (:673-677) until a walker is solved (:710-713) or another round would pass max_states (:665).  The root, the
 * walkers, the W D visited states, their actions, a window of `burst_rounds` rounds of drawn actions and of per-round
 * records, the counters and the two net batches live in HBM.  A round is D times [policy forward, rk_egvm_step] and once
 * [value forward, rk_egvm_round_end], stream-ordered with no host synchronisation; the epsilon draws (:694, :698) depend on
 * nothing the device computes and are uploaded ahead by the caller, in the reference's order.  Steps and round ends after
 * the search is done, and steps after a round has a solved walker, are no-ops.  An engine handle is not thread-safe. */
typedef struct rk_egvm rk_egvm_t;
/* workers 1..65536, depth 1..4096, workers * depth <= 2^22; burst_rounds (1..4096): rounds of draws and records held at once. */
int rk_egvm_create(rk_egvm_t **out, int workers, int depth, int burst_rounds);
int rk_egvm_destroy(rk_egvm_t *h);
/* The batch the engine writes for the net: which = 0 the policy batch (*rows = W: where every walker stands, states_oh of
 * :687, :708), which = 1 the value batch (*rows = W D, row w D + d = walker w after d + 1 moves: new_states_oh of :715), as
 * (rows, 480) one-hot rows of out_dtype (RK_OH_F32 / _F16 / _BF16; cube.py:265-277) or, with RK_OH_STATES, the (rows, 20)
 * int8 states themselves.  The engine owns both (zeroed when made, 16-byte aligned, alive until rk_egvm_destroy) and writes
 * them in the form asked for last; asking for another form needs a new rk_egvm_reset.  Call before rk_egvm_reset. */
int rk_egvm_net_in(rk_egvm_t *h, int which, int out_dtype, void **d_ptr, size_t *rows);
/* `state` of :658-667: a host 20-byte state that is not solved (:662 is the caller's), with max_states of :665.  Puts every
 * walker on it and writes the policy batch.  Synchronises. */
int rk_egvm_reset(rk_egvm_t *h, const int8_t *h_root, long long max_states, void *stream);
/* The draws of the next `rounds` (<= burst_rounds) rounds, int8 (rounds, D, W) on the host: the action 0..11 where the
 * reference acts at random (:694, :698), -1 where it follows the policy (:700-701).  The first of them belongs to the round
 * that is open when the call is made; records of earlier rounds are gone after it.  Synchronises. */
int rk_egvm_set_draws(rk_egvm_t *h, const int8_t *h_draws, int rounds, void *stream);
/* One move of every walker (:694-715): d_logits (W, 12) contiguous, float32 or bfloat16 (dtype RK_OH_F32 / RK_OH_BF16), the
 * policy head on the policy batch; a walker without a drawn action takes the first maximum of its row, a NaN counting as
 * the maximum (ndarray.argmax, :701).  Moves, tests the goal (:709), stores state and action (:703, :714) and writes the
 * walker's rows of both net batches.  No synchronisation. */
int rk_egvm_step(rk_egvm_t *h, const void *d_logits, int dtype, void *stream);
/* Closes the round: with a solved walker, the first depth and there the lowest walker (:710-713), its path (:670) and
 * explored += (d + 1) W (:711), done; else d_values (W D) contiguous, float32 or bfloat16, the value head on the value batch:
 * the first maximum (torch.argmax on the CPU, :674) is the next root (:675), its path is recorded (:677), explored += W D
 * (:716), and the search is done when explored + W D > max_states (:665), else the next round starts.  No synchronisation. */
int rk_egvm_round_end(rk_egvm_t *h, const void *d_values, int dtype, void *stream);
/* Synchronises; h_status[8] = done, solved, rounds closed, explored states (len(agent), :711, :716), the solved walker and
 * its depth (:713; -1 while unsolved), error (0 none, 1 a round beyond the uploaded draws, 2 a round closed before its walk
 * ended), first round of the window of draws. */
int rk_egvm_status(rk_egvm_t *h, long long *h_status, void *stream);
/* The records of closed rounds first_round .. first_round + rounds - 1 of the current window, int64 (rounds, D + 2) on the
 * host: the number n of actions the round appended to the action queue (:670, :677), 1 if it ended by a solve, then the n
 * actions (the rest of a row is undefined).  Synchronises. */
int rk_egvm_records(rk_egvm_t *h, long long first_round, int rounds, long long *h_out, void *stream);

/* ---- device-resident greedy one-step games (agents.py:132-169 inside the loop of :22-38), G games in lock-step ----
 * Every game is one PolicySearch (greedy) or ValueSearch search: a move per step until the state is solved or the game has
 * made max_states moves (this repository's Agent.search counts the moves of the running search against max_states; in the
 * reference len(self) stays 0 until search returns).  The games' states, status (0 running, 1 solved, 2 budget spent,
 * 3 handed back), move counts, actions, the counters and the net batch live in HBM.  A move of all games is
 * [net forward, rk_greedy_step], stream-ordered with no host synchronisation; games that are not running are skipped and
 * their rows of the batch stay as they are.  An engine handle is not thread-safe. */
typedef struct rk_greedy rk_greedy_t;
/* games 1..65536, max_steps >= 1 (the most moves a game may make: the width of the action record), games * max_steps <= 2^30;
 * mode 0 = policy (agents.py:138-142 with sample_policy false), 1 = value (:156-166). */
int rk_greedy_create(rk_greedy_t **out, int games, int max_steps, int mode);
int rk_greedy_destroy(rk_greedy_t *h);
/* The batch the engine writes for the net: *rows = G in policy mode (row g: where game g stands), 12 G in value mode (row
 * 12 g + a: child a of game g's state), as (rows, 480) one-hot rows of out_dtype (RK_OH_F32 / _F16 / _BF16; cube.py:265-277)
 * or, with RK_OH_STATES, the (rows, 20) int8 states themselves.  The engine owns it (zeroed when made, 16-byte aligned, alive
 * until rk_greedy_destroy) and writes the form asked for last; asking for another form needs a new rk_greedy_reset.  Call
 * before rk_greedy_reset. */
int rk_greedy_net_in(rk_greedy_t *h, int out_dtype, void **d_ptr, size_t *rows);
/* n_games (1..games) host 20-byte states, each with a budget of max_states (1..max_steps) moves.  A root that is solved ends
 * at once with status 1 and 0 moves (:29); games n_games.. of the engine stay idle.  Writes the first batch.  Synchronises. */
int rk_greedy_reset(rk_greedy_t *h, const int8_t *h_roots, int n_games, int max_states, void *stream);
/* One move of every running game.  d_out is the net's output on the batch, contiguous, float32 or bfloat16 (dtype RK_OH_F32 /
 * RK_OH_BF16, widened exactly).  Policy mode: (G, 12) logits; the action is the first maximum of the game's row, but a game
 * with a logit less than 2^-20 below the maximum, a NaN logit or an infinite maximum -- where argmax(softmax(logits)) on the
 * host (:139-140) might choose otherwise -- is not moved and gets status 3.  Value mode: (12 G) values; the first solved
 * child (:159-161), else the first maximum, a NaN counting as the maximum (ndarray.argmax, :165).  Then the move, the goal
 * test, the action record, status 1 or -- after max_states moves -- 2, and the game's rows of the next batch.  No
 * synchronisation. */
int rk_greedy_step(rk_greedy_t *h, const void *d_out, int dtype, void *stream);
/* Synchronises; h_status[8] = running games, moves launched since the reset, error (0 none, 1 a running game without room in
 * its action record), games and max_states of the reset, three zeros. */
int rk_greedy_status(rk_greedy_t *h, long long *h_status, void *stream);
/* The games of the last reset to HOST buffers (any may be NULL): status int64 (n_games), moves made int64 (n_games), actions
 * uint8 (n_games, max_states) of which the first `moves made` of a row are defined.  Synchronises. */
int rk_greedy_export(rk_greedy_t *h, long long *h_status, long long *h_steps, uint8_t *h_actions, void *stream);

/* ---- device-resident beam search guided by a value net (rk_beam_*), optionally ending at the symmetry ball ----
 * Depth t holds a beam F_t of m_t <= width states in a fixed order, F_0 = the start; child c = 12 i + a is the state of member i
 * under action a.  A depth: (1) with prune_inverse, child (i, a) is dead when a is the inverse (action ^ 1) of the action that
 * made member i; rows beyond 12 m_t are dead; (2) with n_live live children, explored + n_live > max_states stops the search
 * (status 2), else explored += n_live; (3) the live child that is solved -- with a ball: whose orbit the ball holds -- with the
 * least (ball depth, c) wins (status 1); (4) of live children with equal states the lowest c survives (no dedup across depths);
 * (5) the best min(width, survivors) by value -- larger first, any NaN above every number, -0.0 equal to +0.0, ties to the lower
 * c -- form F_{t+1}, stored in ascending c, back[t+1][j] = i << 4 | a; (6) t + 1 == max_depth stops the search (status 3).
 * A depth is [net forward, rk_beam_step], stream-ordered with no host synchronisation; after a stop a step writes nothing.
 * The engine keeps the current beam, the back record, the sizes and the net batch in HBM.  A handle is not thread-safe. */
typedef struct rk_beam rk_beam_t;
/* width 1..65536, max_depth 1..4096; ball NULL or a BUILT symmetry ball (RK_ESTATE otherwise), to which the engine attaches:
 * rk_symball_destroy refuses meanwhile.  RK_ECAPACITY when the device has no room. */
int rk_beam_create(rk_beam_t **out, rk_symball_t *ball, int width, int max_depth, int prune_inverse);
int rk_beam_destroy(rk_beam_t *h);
/* The batch the engine writes for the net: *rows = 12 width, row 12 j + a = child a of member j, as (rows, 480) one-hot rows of
 * out_dtype (RK_OH_F32 / _F16 / _BF16) or, with RK_OH_STATES, the (rows, 20) int8 states themselves.  The engine owns it (16-byte
 * aligned, alive until rk_beam_destroy) and writes the form asked for last; asking for another form needs a new rk_beam_reset.
 * Call before rk_beam_reset. */
int rk_beam_net_in(rk_beam_t *h, int out_dtype, void **d_ptr, size_t *rows);
/* F_0 = the host 20-byte start state, with the state budget max_states (>= 0).  Writes EVERY row of the batch: the start's
 * twelve children, then the solved state in all others (the net reads all rows at every depth).  With a ball, a start whose
 * orbit the ball holds has won here (status 1, meeting action -1) and no depth runs.  Synchronises. */
int rk_beam_reset(rk_beam_t *h, const int8_t *h_start_state, long long max_states, void *stream);
/* One depth.  d_out: the net's values on the batch, (12 width) contiguous, float32 or bfloat16 (dtype RK_OH_F32 / RK_OH_BF16,
 * widened exactly).  A fixed sequence of launches; everything data-dependent is read from device counters.  No synchronisation. */
int rk_beam_step(rk_beam_t *h, const void *d_out, int dtype, void *stream);
/* Synchronises; h_status[12] = status (0 running, 1 won, 2 budget, 3 depth limit, 4 engine error), depths run, states explored,
 * size of the current beam, error (0 none, 1 a write that had no place in the beam or the back record: not made), the winning
 * child's member i, its action a (-1: the start itself) and its ball depth, the budget, the depth of the current beam, two zeros. */
int rk_beam_status(rk_beam_t *h, long long *h_status, void *stream);
/* To HOST buffers (either may be NULL): h_sizes int64 (max_depth + 1), m_t per depth (0 beyond the depths run); h_back int64
 * (back_len <= width): the first back_len back words of depth `depth` (1..max_depth).  Synchronises. */
int rk_beam_export(rk_beam_t *h, int depth, long long *h_sizes, long long *h_back, size_t back_len, void *stream);
/* The action queue of a search that won, start -> solved: back upward from the winning child's parent (one wave), the winning
 * action, then the ball's descent from the winning child -- at each step the lowest action whose child's representative lies
 * one level nearer.  Returns its length or a negative error (RK_ESTATE: not won, or the record is broken); writes at most
 * max_len actions.  Synchronises. */
long long rk_beam_path(rk_beam_t *h, long long *h_actions, size_t max_len, void *stream);

/* ---- beam searches of many states in lock-step (rk_beamb_*) ----
 * `searches` slots, each a whole rk_beam search of its own (beam, back record, sizes, dedup table, histograms, look-back words,
 * counters, root); all share width, max_depth, prune_inverse and the ball, and differ in start, budget, depth reached and status.
 * One net batch of searches x 12 width rows per form: slot s owns rows [12 width s, 12 width (s + 1)), and its values are
 * d_out[12 width s ..] of the one forward.  A depth of all slots is [net forward, rk_beamb_step].  A slot is running (status 0),
 * stopped as rk_beam_status says (1..4), or at rest (5): never started, or put to rest.  After a slot stops a step writes nothing
 * of it.  Every slot gets what rk_beam_* gives its start alone.  A handle is not thread-safe. */
typedef struct rk_beamb rk_beamb_t;
/* searches 1..1024, width 1..65536, searches * width <= 65536, max_depth 1..4096 (RK_EINVAL before anything is allocated); ball as
 * for rk_beam_create.  Every slot is at rest.  RK_ECAPACITY when the device has no room. */
int rk_beamb_create(rk_beamb_t **out, rk_symball_t *ball, int searches, int width, int max_depth, int prune_inverse);
int rk_beamb_destroy(rk_beamb_t *h);
/* As rk_beam_net_in: *rows = searches x 12 width.  After a form is handed out that is not the one the engine writes, the next
 * rk_beamb_reset or rk_beamb_rest first writes the solved state into EVERY row of every slot in that form and puts every running
 * slot to rest: a slot that was not started in the current form holds legal rows and is not running. */
int rk_beamb_net_in(rk_beamb_t *h, int out_dtype, void **d_ptr, size_t *rows);
/* Slot slots[j] (all different, 0..searches-1) starts again from host state j (20 bytes each, cubie codes checked before anything
 * is enqueued) with the budget max_states[j] >= 0: its counters, F_0, the ball look-up of the start (inside the ball: won here,
 * meeting action -1), table, look-back words, histograms and sizes cleared, all its 12 width rows written (the start's children,
 * then the solved state).  Nothing of any other slot is touched, so it may run between two steps while other slots are
 * mid-search.  A fixed number of copies and launches per call, whatever n.  Synchronises. */
int rk_beamb_reset(rk_beamb_t *h, int n, const int32_t *slots, const int8_t *h_start_states, const long long *max_states, void *stream);
/* The named slots that are running are put to rest (status 5) without a search; a stopped slot keeps its result.  Only the status
 * word is written.  Synchronises. */
int rk_beamb_rest(rk_beamb_t *h, int n, const int32_t *slots, void *stream);
/* One depth of every running slot.  d_out: the net's values on the whole batch, (searches x 12 width) contiguous, float32 or
 * bfloat16.  rk_beam_step's sequence of launches (nine with a ball, eight without) with the slot in the grid's second dimension,
 * nothing else.  RK_ESTATE before the first reset or rest in the current form.  No synchronisation. */
int rk_beamb_step(rk_beamb_t *h, const void *d_out, int dtype, void *stream);
/* Synchronises; h_status (searches, 12): rk_beam_status's words of every slot, read with one copy. */
int rk_beamb_status(rk_beamb_t *h, long long *h_status, void *stream);
/* One launch, a wave per slot; h_out int32 (searches, 1 + max_len), max_len <= max_depth + 1 + 10: word 0 the length of the slot's
 * action queue (rk_beam_path's), -1 for a slot that has not won, -2 when the record does not lead home or the queue is longer than
 * max_len; then the actions.  Synchronises. */
int rk_beamb_paths(rk_beamb_t *h, int32_t *h_out, int max_len, void *stream);
/* rk_beam_export of one slot. */
int rk_beamb_export(rk_beamb_t *h, int slot, int depth, long long *h_sizes, long long *h_back, size_t back_len, void *stream);

/* ---- batched A*: S independent searches in lock-step, no host synchronisation inside an iteration -------------
 * Every search is a complete rk_astar_* engine (agents.py:171-413: its own pool, hash table, open queue, counter block);
 * the batch launches the same kernels with a second grid dimension (search), so one iteration of ALL searches is the
 * six launches of one search around one net forward on the padded (S * 12 N, 480) batch -- capturable in a hipGraph:
 *   rk_astarb_step_expand : loop guard + pop + fan-out + membership / first-occurrence / append + goal test for every
 *                           search, then the net's rows of the new states into d_onehot: search s owns rows
 *                           s * 12 N ... (one-hot of out_dtype, or the 20-byte states with RK_OH_STATES); rows past a
 *                           search's new states keep what they held
 *   rk_astarb_step_commit : d_values (S * 12 N) from the net (float32, or bfloat16 after rk_astarb_set_values_dtype);
 *                           cost, push, relaxation, bookkeeping, next pop lists
 *   rk_astarb_status      : synchronises; h_status (S, 7) int64 = done, won (2 = start already solved), n_states,
 *                           iterations, open-queue length, index of the solved state, error (the codes of rk_astar_status;
 *                           4 = a NaN value ended this search alone, see NON-FINITE VALUES at rk_astar_create)
 * h_max_states of rk_astarb_reset: per-search state budgets (null = the capacity). */
typedef struct rk_astarb rk_astarb_t;
int rk_astarb_create(rk_astarb_t **out, int n_searches, size_t capacity_per_search, int max_expansions);
int rk_astarb_destroy(rk_astarb_t *h);
int rk_astarb_reset(rk_astarb_t *h, const int8_t *h_start_states, const long long *h_max_states, double lambda, void *stream);
int rk_astarb_set_values_dtype(rk_astarb_t *h, int dtype, void *stream);
int rk_astarb_step_expand(rk_astarb_t *h, void *d_onehot, int out_dtype, void *stream);
/* The same step with the net's rows COMPACTED across the searches: only the NEW states of every search, one search after
 * the other (each search's first row rounded up to a multiple of 4 rows), and their total copied asynchronously into
 * (pinned) host memory at h_total.  The caller waits for the count (an event recorded behind this call), runs the net on
 * that many rows and commits values laid out the same way: the net never sees a padded row -- what the sequential
 * `AStar` does for a float32 net (agents.py:315, :369-383 evaluate exactly the new states).  One host wait per iteration;
 * not capturable in a hipGraph (the batch size varies). */
int rk_astarb_step_expand_compact(rk_astarb_t *h, void *d_rows, int out_dtype, int *h_total, void *stream);
int rk_astarb_step_commit(rk_astarb_t *h, const float *d_values, void *stream);
int rk_astarb_status(rk_astarb_t *h, long long *h_status, void *stream);
int rk_astarb_export(rk_astarb_t *h, int search, size_t first, size_t count, int8_t *h_states, double *h_G,
                     long long *h_parents, long long *h_parent_actions, void *stream);
long long rk_astarb_path(rk_astarb_t *h, int search, long long index, long long *h_actions, size_t max_len, void *stream);

/* ---- hash-sharded A* across the GPUs of a node (BASELINE config 5; no counterpart in the reference) ------------
 * One engine per GPU/rank holds the states it owns, owner(state) = rk_shard_owner(state, world).  An iteration is two
 * collectives with fixed-size device buffers and no host synchronisation in between:
 *   all-gather   rk_astar_shard_gather_ptr: 8 + N doubles per rank = {pool size, won, solved index, error, candidates,
 *                seconds since the reset on the rank's DEVICE clock (rank 0's decides "out of time"), 0, 0, the rank's N cheapest
 *                open costs ascending, +inf} -- the engine writes all of it, the host nothing: the iteration is capturable
 *   rk_astar_shard_select (gathered)  identical stop decision on every rank (won / budget / a pool could overflow /
 *                time / error / nothing open) and the global top-N by (cost, rank, position); expands this rank's share
 *                and buckets the 32-byte child records by owner (stable) into d_send
 *   all-to-all   equal splits of rk_astar_shard_block_bytes() per peer: {32-byte header = record count, offer count;
 *                12 N records of 32 B; 12 N shortcut offers of 16 B} -- counts travel inside the blocks
 *   rk_astar_shard_insert (d_recv)  applies the offers received (relaxation case 2 of the PREVIOUS iteration on the
 *                parents' owner), then membership / first-occurrence / append / goal test / relaxation case 1 in arrival
 *                order and the one-hot rows of the new states (12 N rows at most: all ranks together pop N nodes)
 *   rk_astar_shard_push  values -> cost, push; builds this iteration's offers into d_send for the next all-to-all;
 *                bookkeeping, next candidates, next all-gather contribution
 * rk_astar_shard_decision (synchronises) lets the host learn the stop decision -- every iteration or every few.
 * After a stop without a win: one more select + all-to-all, then rk_astar_shard_flush applies the pending offers.
 * With world = 1 (send buffer = receive buffer) this reproduces the single-GPU engine exactly.
 * librubiks_amd/solving/sharded.py is the driver. */
int rk_astar_create_sharded(rk_astar_t **out, size_t capacity, int max_expansions, int rank, int world);
int rk_shard_owner(const int8_t *h_state, int world);
long long rk_astar_shard_block_bytes(const rk_astar_t *h);
long long rk_astar_shard_gather_len(const rk_astar_t *h);
void *rk_astar_shard_gather_ptr(rk_astar_t *h);
/* Make the engine write its all-gather contribution into caller memory (8 + N doubles, 8-byte aligned). */
int rk_astar_shard_bind(rk_astar_t *h, void *d_gather);
int rk_astar_shard_reset(rk_astar_t *h, const int8_t *h_start_state, double lambda, void *d_send, void *stream);
int rk_astar_shard_select(rk_astar_t *h, const void *d_gathered, double time_limit, double max_states, void *d_send, void *stream);
/* h_out[8] = {stop reason (0 none, 1 won, 2 budget, 3 capacity, 4 time, 5 nothing open, 6 error), winner rank, winner
 * index, total states, this rank's pops, iterations, this rank's states, the largest error code any rank reported (1 pool
 * capacity, 2 look-back chain, 3 more new states than net rows: rk_astar_shard_push_rows, 4 a NaN among the values a rank
 * read: see NON-FINITE VALUES at rk_astar_create)}. */
int rk_astar_shard_decision(rk_astar_t *h, long long *h_out, void *stream);
int rk_astar_shard_insert(rk_astar_t *h, const void *d_recv, void *d_send, void *d_onehot, int out_dtype, void *stream);
/* Between insert and push: asynchronous copy of this iteration's new-state count (<= 12 N: all ranks together pop at most N
 * nodes) into (pinned) host memory; does not synchronise.  Lets the driver run the net on the rows that exist instead of
 * on the whole padded batch (librubiks_amd/solving/sharded.py). */
int rk_astar_shard_new_count(rk_astar_t *h, int *h_out, void *stream);
int rk_astar_shard_push(rk_astar_t *h, const float *d_values, const void *d_recv, void *d_send, void *stream);
/* The same with the promise the driver can actually keep without a host round trip: d_values holds the net's values of the FIRST
 * `rows` new states only (0 < rows <= 12 N; a rank expects 12 N / world new states, the driver evaluates a fixed number a little
 * above that).  An iteration with more new states than rows sets error 3 in this rank's all-gather contribution: every rank stops
 * together at the next rk_astar_shard_select with stop reason 6 and h_out[7] = 3, and the driver repeats the search with
 * rows = 12 N.  Nothing is copied to the host and nothing waits: insert -> net(rows) -> push_rows is a fixed-shape sequence. */
int rk_astar_shard_push_rows(rk_astar_t *h, const float *d_values, int rows, const void *d_recv, void *d_send, void *stream);
int rk_astar_shard_flush(rk_astar_t *h, const void *d_recv, void *stream);
int rk_astar_shard_clear_send(rk_astar_t *h, void *d_send, int records, int offers, void *stream);
/* h_out = {parent rank, parent index, action} of node `index` on this rank (for the cross-rank path walk). */
int rk_astar_shard_parent(rk_astar_t *h, long long index, long long *h_out, void *stream);
/* Rows [first, first+count) of the parents' owner ranks (int64, HOST): with rk_astar_export's states / G / parents / actions
 * the whole shard of this rank. */
int rk_astar_shard_export_ranks(rk_astar_t *h, size_t first, size_t count, long long *h_parent_ranks, void *stream);

/* ---- transport of the hash-sharded search over RCCL / xGMI, for callers without torch.distributed ----------------
 * No counterpart in the reference (single process); SURVEY.md 8(b) `rk_comm_*`.  One communicator per process (= per GPU,
 * the device current at rk_comm_create).  Rank 0 calls rk_comm_unique_id and hands the RK_COMM_ID_BYTES bytes to the other
 * ranks by any means (file, socket, MPI); every rank then calls rk_comm_create with the same bytes (a collective call).
 * The three transfers are exactly what rk_astar_shard_* needs, on the engine's own fixed-size DEVICE buffers, enqueued on
 * the caller's stream and ordered with the engine's kernels (nothing synchronises):
 *   rk_comm_all_gather   bytes_per_rank from every rank, rank-major, into d_recv (world * bytes_per_rank)
 *   rk_comm_all_to_all   block p of d_send goes to rank p, block q of d_recv comes from rank q (equal blocks: the record
 *                        and offer counts travel inside them, rk_astar_shard_block_bytes); d_send != d_recv
 *   rk_comm_broadcast    in place, from `root` (the three integers of one hop of the path walk)
 * librccl is opened at first use (RK_RCCL_LIB overrides the name); RK_EHIP with RCCL's message if a call fails.
 * librubiks_amd/solving/sharded.py::RcclTransport drives ShardedAStar through these; torch.distributed stays the default. */
#define RK_COMM_ID_BYTES 128
typedef struct rk_comm rk_comm_t;
int rk_comm_unique_id(void *out_128_bytes);
int rk_comm_create(rk_comm_t **out, const void *id_128_bytes, int rank, int world);
int rk_comm_destroy(rk_comm_t *c);
int rk_comm_rank(const rk_comm_t *c);
int rk_comm_world(const rk_comm_t *c);
int rk_comm_all_gather(rk_comm_t *c, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);
int rk_comm_all_to_all(rk_comm_t *c, const void *d_send, void *d_recv, size_t bytes_per_peer, void *stream);
int rk_comm_broadcast(rk_comm_t *c, void *d_buf, size_t bytes, int root, void *stream);

/* ---- Monte Carlo tree search (agents.py:415-645): T independent trees, all state in HBM ----------------------
 * Replaces MCTS.expand_leaf / find_leaf for a whole batch of searches (the reference runs one tree at a time).
 * Per tree the engine owns the reference's arrays: states, neighbors (cap,12), leaves, P, V, N, W, L
 * (agents.py:419-427; index 0 unused, root = 1), a hash table state -> index, and the current path
 * (indices_visited / actions_taken, agents.py:474-475).  One wavefront serves one tree.
 * One simulation of every live tree (agents.py:476-490) = two stream-ordered calls around the net forward:
 *   rk_mcts_expand        loop guard `len + 12 <= max_states` (:476); the leaf's 12 children (:513), membership and
 *                         new indices in action order (:517-529), neighbor links both ways and leaf flag (:533-536),
 *                         goal test of ALL children, first solved wins (:540-543).  Leaves the 12 children of every
 *                         tree in a (T*12, 20) buffer.
 *   rk_mcts_children_oh   one-hot of that buffer, (T*12, 480): the fixed-shape net batch (out_dtype RK_OH_STATES: the
 *                         (T*12, 20) int8 states themselves, for a net whose first layer is fused, rk_ohl_*)
 *   rk_mcts_backup_select P, V of the new children (:556-557), W[leaf] = V[neighbors], W[new] = v, max-backup of
 *                         max(v_new) along the path (:559-562), N += 1 once per distinct (node, action) of the path,
 *                         virtual loss cleared (:567-570); then, unless the tree just solved, the next descent
 *                         `find_leaf` (:575-595): U = c P sqrt(sum N)/(1+N), Q = W - L, first argmax, L += nu on both
 *                         ends of the chosen edge.  d_probs (T*12, 12) are softmaxed policy rows, d_values (T*12).
 * Nothing synchronises, shapes are fixed and finished trees are skipped on the device, so a simulation step can be
 * captured in a hipGraph and replayed.  float64 statistics, no fused multiply-add: identical to NumPy. */
typedef struct rk_mcts rk_mcts_t;
int rk_mcts_create(rk_mcts_t **out, int n_trees, size_t capacity_per_tree, size_t max_path);
int rk_mcts_destroy(rk_mcts_t *h);
/* h_start_states (T,20) host; h_max_states (T) host or NULL (= capacity); c exploration constant, nu virtual loss. */
int rk_mcts_reset(rk_mcts_t *h, const int8_t *h_start_states, const long long *h_max_states, double c, double nu, void *stream);
/* One-hot of the T root states (T, 480) for the net; then hand back softmaxed policy (T,12) and value (T). */
int rk_mcts_roots_oh(rk_mcts_t *h, void *d_out, int out_dtype, void *stream);
int rk_mcts_set_root_pv(rk_mcts_t *h, const float *d_probs, const float *d_values, void *stream);
int rk_mcts_expand(rk_mcts_t *h, void *stream);
/* rk_mcts_expand and hipGraphs: whether the path's leaf still has to be expanded is decided ON THE DEVICE (a per-tree word the
 * expanding kernel sets and the backup consumes).  Called eagerly, rk_mcts_expand skips its launch when the previous backup +
 * select call has expanded ahead; called on a stream that is being captured it always records the kernel, which leaves at once
 * for trees that are expanded already -- so a step captured at ANY point (straight after rk_mcts_reset, or in the middle of
 * a search) replays correctly from any state.  A captured step may also leave rk_mcts_expand out altogether once expand-ahead
 * is on and one eager step has run (what MCTSBatch does: one launch less per replay); a backup that finds no expansion pending
 * stops its tree with error 3 in rk_mcts_status instead of backing up stale children.
 * Expand ahead: with sim_limit != 0 the backup + select launch ends by expanding the leaf it has just found (the first half
 * of the NEXT simulation's expand_leaf, agents.py:505-543), and the rk_mcts_expand call that follows it is then a no-op
 * without a launch: one launch and its dependent start-up less per simulation, same order of steps (select, expand, net,
 * backup).  sim_limit > 0: only while the simulation just backed up has a number below sim_limit (so that a search of
 * sim_limit simulations ends exactly where the reference's would); < 0: always; 0 (default): off.  A driver that stops for
 * another reason (time) sets the limit to 0 and runs one more step, which completes the pending expansions. */
int rk_mcts_set_expand_ahead(rk_mcts_t *h, long long sim_limit);
int rk_mcts_children_oh(rk_mcts_t *h, void *d_out, int out_dtype, void *stream);
int rk_mcts_backup_select(rk_mcts_t *h, const float *d_probs, const float *d_values, void *stream);
/* The same step from the net's RAW outputs: d_logits, T*12 rows of 12 logits `logits_stride` elements apart, and d_values,
 * T*12 values `values_stride` elements apart (12 and 1 for separate contiguous heads; 13 and 13 for one (T*12, 13) tensor of
 * merged heads with d_values = d_logits + 12 elements), both float32 (dtype RK_OH_F32) or both bfloat16 (RK_OH_BF16); the
 * softmax of agents.py:551 (exp(x - max) / sum in float32) runs inside the kernel, which saves the conversion, softmax and
 * copy kernels of every simulation. */
int rk_mcts_backup_select_logits(rk_mcts_t *h, const void *d_logits, int logits_stride, const void *d_values, int values_stride,
                                 int dtype, void *stream);
/* The same for the trees first_tree ... first_tree + n_trees - 1 only; d_logits / d_values hold THEIR n_trees*12 rows (row 0 = child
 * 0 of tree first_tree; their children lie at rk_mcts_children() + first_tree*12*20 bytes).  Trees are independent searches
 * (agents.py:415-645 runs one at a time), so a step may advance the batch in parts, on different streams: while one part's
 * latency-bound descent runs, the other part's net forward has the chip (MCTSBatch overlap_halves).  Every tree still sees exactly
 * the reference's sequence select, expand, net, backup. */
int rk_mcts_backup_select_logits_range(rk_mcts_t *h, int first_tree, int n_trees, const void *d_logits, int logits_stride,
                                       const void *d_values, int values_stride, int dtype, void *stream);
/* Device pointer to the (T*12, 20) int8 child states of the pending simulation (what rk_mcts_children_oh encodes): a net
 * whose first layer reads states (rk_ohl_forward) can take them where they lie. */
const int8_t *rk_mcts_children(rk_mcts_t *h);
/* Synchronises.  h_status is (T, 6) int64: done, solved, n_states, simulations, path_len, error (1: path longer than max_path,
 * 2: broken neighbour link, 3: backup without a pending expansion, 4: a NaN in the value, or a NaN or an infinity among the 12
 * priors -- after the softmax of the logits entries, so a +inf logit counts and a -inf logit does not --, of a NEW child or of a
 * root: that tree stops (done = 1) before anything of the simulation is written; infinite values are accepted, and the rows of
 * children that are already in the tree are not looked at). */
int rk_mcts_status(rk_mcts_t *h, long long *h_status, void *stream);
/* Rows [first, first+count) of one tree's arrays to HOST buffers in the reference's dtypes (any may be NULL):
 * states int8 (count,20), neighbors int64 (count,12), leaves uint8, P/W/L float64 (count,12), V float64, N int64. */
int rk_mcts_export(rk_mcts_t *h, int tree, size_t first, size_t count, int8_t *h_states, long long *h_neighbors,
                   uint8_t *h_leaves, double *h_P, double *h_V, long long *h_N, double *h_W, double *h_L, void *stream);
/* The tree's action queue: the solving actions if it solved (agents.py:483), else the actions of its current
 * descent (agents.py:492).  Also the visited node indices if h_nodes != NULL.  Returns the number of actions. */
long long rk_mcts_path(rk_mcts_t *h, int tree, long long *h_actions, long long *h_nodes, size_t max_len, void *stream);

/* increase_stack_size (agents.py:450-460, called from :503-504): every tree's pool grows to new_capacity states (and the path
 * arrays to new_max_path entries) IN PLACE: new arrays, device-to-device copies, the hash tables rebuilt by one kernel.
 * h_max_states (T, host, nullable = new_capacity) are the new state budgets; a tree that had stopped only at the loop guard
 * `len + 12 <= max_states` (agents.py:476) and has room again continues with the expansion it was about to do.  Synchronises;
 * a hipGraph captured from this engine must be captured again. */
int rk_mcts_grow(rk_mcts_t *h, size_t new_capacity, size_t new_max_path, const long long *h_max_states, void *stream);
/* The graph post-processing of a solved search (agents.py:483-486) on the device, for every tree that has solved:
 * _complete_graph (agents.py:597-611: every leaf linked, both ways, to those of its 12 children that are in the graph -- one
 * launch: fan-out, hash probe, neighbour writes) and the breadth-first search of _shorten_action_queue (agents.py:613-633)
 * from the root to the solved state's index, one workgroup per tree, level by level in the reference's queue order (so the
 * path found is the reference's, not just one of the same length).  Stream-ordered; rk_mcts_export afterwards shows the
 * completed `neighbors`.  rk_mcts_graph_path (synchronises) returns the shortened action queue of `tree` -- its length, or -1
 * when there is none (tree not solved: the queue of rk_mcts_path stands). */
int rk_mcts_search_graph(rk_mcts_t *h, void *stream);
long long rk_mcts_graph_path(rk_mcts_t *h, int tree, long long *h_actions, size_t max_len, void *stream);

/* ---- host-pointer conveniences (allocate scratch, copy, launch, copy back, synchronise) ----
 * What reference code sees when it calls cube.rotate / multi_rotate / is_solved / scramble with NumPy arrays
 * (cube.py:41-56, :85-89, :206-216).  SMALL calls -- inputs and outputs together up to 1 MiB, i.e. about 25 000 20-byte
 * states through rk_multi_rotate_host or 3 800 parents through rk_expand12_host, without h_stats -- go ZERO-COPY: the arrays
 * pass through one page-locked, device-mapped buffer per host thread, the kernel reads and writes it over the bus, and the
 * call costs one launch and one stream synchronisation (one state: 17-21 us from Python against 29-37 us with staged copies,
 * profiles/r04_reference_protocol.json, r04_latency.json).  Larger calls, and calls that want the counters (atomics, kept in
 * device memory), stage through device scratch as before.  Results are the same either way. */
int rk_multi_rotate_host(int repr, const int8_t *h_states, const uint8_t *h_actions, int8_t *h_out,
                         size_t n, void *stream);
int rk_expand12_host(int repr, const int8_t *h_parents, int8_t *h_children, uint8_t *h_solved,
                     long long *h_stats, size_t n, void *stream);
int rk_multi_is_solved_host(int repr, const int8_t *h_states, uint8_t *h_flags, long long *h_stats,
                            size_t n, void *stream);
int rk_apply_sequences_host(int repr, const uint8_t *h_actions, int depth, int games, int with_solved,
                            int only_last, int8_t *h_out, void *stream);
/* cube.as_oh as reference code calls it (cube.py:130-133, :265-277): states from HOST memory, the one-hot written to DEVICE
 * memory (`d_out`, 16-byte aligned, n x 480 or n x 288 elements of `out_dtype`), where the net reads it.  Synchronises. */
int rk_as_oh_host(int repr, const int8_t *h_states, void *d_out, int out_dtype, size_t n, void *stream);
/* rk_oh686_from2024 from HOST states (cube.py:58-71, 363-369), the rows written to DEVICE memory; synchronises. */
int rk_oh686_from2024_host(const int8_t *h_states20, void *d_out, int out_dtype, size_t n, void *stream);
/* rk_686_to2024 from HOST states into HOST memory (cube.py:58-71); h_stats (nullable) receives [count, first index] of the
 * illegal rows ([0, INT64_MAX] when there are none); synchronises. */
int rk_686_to2024_host(const int8_t *h_states686, int8_t *h_out20, long long *h_stats, size_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RUBIKS_HIP_H */
