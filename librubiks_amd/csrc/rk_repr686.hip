// The two cube representations into each other on the device (cube.py:58-71, 363-369):
//   k_oh686_from2024  20-byte states -> the 6x8x6 one-hot of each, as int8 (the (6,8,6) state itself) or as the net's f32 / f16 /
//                     bf16 input: out[r][48 f + 6 p + colour] = 1 for the colour slot (f, p) shows.  The search engines keep their
//                     states in 20 bytes; a net trained on 6x8x6 gets its batch from this kernel, in the one launch that is
//                     both the conversion and the encoding.
//   k_686_to2024      (6,8,6) int8 states -> 20-byte states, counting the rows that are not a well-formed one-hot showing each
//                     of the 20 cubies exactly once (those rows are written as -1 bytes).
// The (cubie, code) <-> (slot, colour) tables are built at compile time from the face definitions (rk_tables.h).
//
// k_oh686_from2024 reads 20 B and writes 288 / 576 / 1 152 B per row: a store stream.  A workgroup takes a tile of 64 rows: the
// tile's 1 280 B come in as dwords, one thread per (row, cubie) scatters the cubie's 2-3 colours into a 48-byte colour row in LDS,
// and the workgroup then writes the tile's output -- contiguous in memory -- as consecutive 16-byte chunks, so every store
// instruction of a wave covers 1 KiB without a gap.
#include "rk_device.h"
#include "rk_kernels.h"

namespace rk {

static __constant__ Repr686Tables D_R686 = make_repr686_tables();
static_assert(make_repr686_tables().consistent, "20-byte and 6x8x6 move tables do not describe the same cube");

namespace {

template <int KIND> struct One686;                                 // bits of 1.0 in the output element
template <> struct One686<RK686_I8>   { static constexpr uint32_t bits = 0x01u, eb = 1; };
template <> struct One686<RK686_F32>  { static constexpr uint32_t bits = 0x3F800000u, eb = 4; };
template <> struct One686<RK686_F16>  { static constexpr uint32_t bits = 0x3C00u, eb = 2; };
template <> struct One686<RK686_BF16> { static constexpr uint32_t bits = 0x3F80u, eb = 2; };

constexpr int R686_TILE = 64;

// element e of a row (e = 6 slot + colour) is 1 where the slot shows that colour
template <int KIND>
__device__ __forceinline__ uint32_t elem686(const uint8_t *col, int e)
{
	return col[e / 6] == (uint8_t)(e % 6) ? One686<KIND>::bits : 0u;
}

}  // namespace

template <int KIND>
__global__ __launch_bounds__(256)
void k_oh686_from2024(const uint32_t *__restrict__ states, u32x4 *__restrict__ out, size_t n, size_t n_tiles)
{
	constexpr int EB = One686<KIND>::eb, E = 16 / EB, CH = S686_BYTES * EB / 16;      // elements per chunk, chunks per row
	__shared__ uint32_t s_fw[20 * 24];
	__shared__ uint32_t s_in[R686_TILE * STATE_DWORDS];
	__shared__ uint8_t s_col[R686_TILE * S686_SLOTS];
	for (int i = threadIdx.x; i < 20 * 24; i += 256) s_fw[i] = (&D_R686.fw[0][0])[i];
	for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		const size_t first = tile * R686_TILE;
		const int rows = (int)(n - first < (size_t)R686_TILE ? n - first : (size_t)R686_TILE);
		__syncthreads();                                           // the previous tile's colour rows are written out
		for (int q = threadIdx.x; q < rows * STATE_DWORDS; q += 256) s_in[q] = states[first * STATE_DWORDS + q];
		__syncthreads();
		for (int q = threadIdx.x; q < rows * 20; q += 256) {
			const int r = q / 20, c = q % 20;
			uint32_t v = (s_in[r * STATE_DWORDS + c / 4] >> (8 * (c % 4))) & 0xFFu;
			v = v < 24 ? v : 0;                                    // an out-of-range code stays inside the table (the row is meaningless)
			const uint32_t e = s_fw[c * 24 + v];
			uint8_t *col = s_col + r * S686_SLOTS;
			col[e & 63] = (uint8_t)((e >> 6) & 7);
			col[(e >> 9) & 63] = (uint8_t)((e >> 15) & 7);
			if (c < 8) col[(e >> 18) & 63] = (uint8_t)((e >> 24) & 7);
		}
		__syncthreads();
		u32x4 *dst = out + first * CH;
		for (int q = threadIdx.x; q < rows * CH; q += 256) {
			const uint8_t *col = s_col + (q / CH) * S686_SLOTS;
			const int e0 = (q % CH) * E;
			u32x4 w;
			if (EB == 4) {
				w.x = elem686<KIND>(col, e0);     w.y = elem686<KIND>(col, e0 + 1);
				w.z = elem686<KIND>(col, e0 + 2); w.w = elem686<KIND>(col, e0 + 3);
			} else if (EB == 2) {
				w.x = elem686<KIND>(col, e0)     | elem686<KIND>(col, e0 + 1) << 16;
				w.y = elem686<KIND>(col, e0 + 2) | elem686<KIND>(col, e0 + 3) << 16;
				w.z = elem686<KIND>(col, e0 + 4) | elem686<KIND>(col, e0 + 5) << 16;
				w.w = elem686<KIND>(col, e0 + 6) | elem686<KIND>(col, e0 + 7) << 16;
			} else {
				uint32_t d[4];
				#pragma unroll
				for (int k = 0; k < 4; k++)
					d[k] = elem686<KIND>(col, e0 + 4 * k) | elem686<KIND>(col, e0 + 4 * k + 1) << 8 |
					       elem686<KIND>(col, e0 + 4 * k + 2) << 16 | elem686<KIND>(col, e0 + 4 * k + 3) << 24;
				w = u32x4{d[0], d[1], d[2], d[3]};
			}
			dst[q] = w;
		}
	}
}

// One thread per row; the workgroup's 64 rows come in through LDS with 16-byte loads.  A row is legal when every slot holds exactly
// one 1 among six 0 / 1 bytes and the colours at the 20 cubie positions name each cubie once; stats = [count, first index] of the
// rows that are not (nullable; initialise to [0, INT64_MAX]).
__global__ __launch_bounds__(256)
void k_686_to2024(const u32x4 *__restrict__ states, uint32_t *__restrict__ out, long long *__restrict__ stats, size_t n)
{
	constexpr int Q = S686_BYTES / 16;                               // 18 chunks per row
	__shared__ u32x4 s_row[R686_TILE * Q];
	__shared__ uint8_t s_col[R686_TILE][S686_SLOTS + 16];
	const size_t n_tiles = (n + R686_TILE - 1) / R686_TILE;
	for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		const size_t first = tile * R686_TILE;
		const int rows = (int)(n - first < (size_t)R686_TILE ? n - first : (size_t)R686_TILE);
		__syncthreads();
		for (int q = threadIdx.x; q < rows * Q; q += 256) s_row[q] = states[first * Q + q];
		__syncthreads();
		const int r = threadIdx.x;
		if (r >= rows) continue;
		const uint8_t *row = reinterpret_cast<const uint8_t *>(s_row + r * Q);
		uint8_t *col = s_col[r];
		bool ok = true;
		for (int s = 0; s < S686_SLOTS; s++) {
			int ones = 0, which = 0;
			#pragma unroll
			for (int k = 0; k < 6; k++) {
				const uint8_t b = row[6 * s + k];
				ok = ok && b <= 1;
				ones += b;
				which = b ? k : which;
			}
			ok = ok && ones == 1;
			col[s] = (uint8_t)which;
		}
		uint32_t code[20] = {};
		uint32_t seen = 0;
		for (int p = 0; p < 20 && ok; p++) {
			const uint32_t q = D_R686.inv[p][col[D_R686.home[p][0]]][col[D_R686.home[p][1]]];
			if (q == 0xFFFFu) { ok = false; break; }
			const uint32_t c = q >> 5, v = q & 31;
			const uint32_t e = D_R686.fw[c][v];
			if (c < 8 && col[(e >> 18) & 63] != ((e >> 24) & 7)) ok = false;     // the corner's third colour
			seen |= 1u << c;
			code[c] = v;
		}
		ok = ok && seen == 0xFFFFFu;
		uint32_t *dst = out + (first + r) * STATE_DWORDS;
		#pragma unroll
		for (int d = 0; d < STATE_DWORDS; d++)
			dst[d] = ok ? (code[4 * d] | code[4 * d + 1] << 8 | code[4 * d + 2] << 16 | code[4 * d + 3] << 24) : 0xFFFFFFFFu;
		if (!ok && stats != nullptr) {
			atomicAdd(reinterpret_cast<unsigned long long *>(&stats[0]), 1ull);
			atomicMin(&stats[1], (long long)(first + r));
		}
	}
}

void launch_oh686_from2024(const int8_t *states, void *out, int kind, size_t n, hipStream_t st)
{
	const size_t n_tiles = (n + R686_TILE - 1) / R686_TILE;
	const unsigned grid = (unsigned)(n_tiles < 8192 ? n_tiles : 8192);
	#define RK_GO(K) hipLaunchKernelGGL((k_oh686_from2024<K>), dim3(grid), dim3(256), 0, st, (const uint32_t *)states, (u32x4 *)out, n, n_tiles)
	switch (kind) {
	case RK686_F32: RK_GO(RK686_F32); break;
	case RK686_F16: RK_GO(RK686_F16); break;
	case RK686_BF16: RK_GO(RK686_BF16); break;
	default: RK_GO(RK686_I8); break;
	}
	#undef RK_GO
}

void launch_686_to2024(const int8_t *states, int8_t *out, long long *stats, size_t n, hipStream_t st)
{
	const size_t n_tiles = (n + R686_TILE - 1) / R686_TILE;
	const unsigned grid = (unsigned)(n_tiles < 8192 ? n_tiles : 8192);
	hipLaunchKernelGGL(k_686_to2024, dim3(grid), dim3(256), 0, st, (const u32x4 *)states, (uint32_t *)out, stats, n);
}

}  // namespace rk
