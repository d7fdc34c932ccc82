// attn_tile.hip — decode attention for the verify step of speculative decoding that reads each key ONCE for all rows (include/hqq_hip.h,
// hqq_hip_attn_decode_tiled), gfx950.
//
// hqq_hip_attn_decode_shared (block.hip) is the one-row kernel with the row as blockIdx.z: each of the R rows streams the whole K and V of its head.
// Here one workgroup serves (query head, split) for ALL rows: its query tile is the R queries of the head padded to the 16 rows of an MFMA, and the
// keys [k0, k1) of [0, n_max) — n_max = 1 + the largest clamped position, chunk = ceil(n_max / S) — go through the matrix cores once, flash-decoding style.
//
//   blocks   a wave owns blocks of 32 keys, dealt round-robin over the TILE_WAVES waves; no workgroup barrier inside the loop (a wave's LDS image is its own)
//   S^T      = K . Q^T with v_mfma_f32_16x16x32: A = 16 keys (lane l: key l & 15, dims 32 c + 8 (l >> 4) ..), B = the query tile (row l & 15, the same dims;
//            HD / 32 fragments kept in registers for the whole kernel).  The accumulator holds per lane 4 keys (4 (l >> 4) + r) of ONE query row (l & 15), so a
//            row's maximum and sum over the block are this lane's 8 values and two __shfl_xor (16, 32)
//   mask     key j of row i scores -inf when j > pos[i] or j >= k1, BEFORE the maximum: its probability is exactly 0
//   (m, l, O) per row: m_new = max(m, block max); alpha = exp(m - m_new); p = exp(s - m_new); l = l alpha + sum p; O = O alpha + P V.  A row that has seen no
//            key yet (m_new = -inf) subtracts 0 instead: p = 0, alpha = 0, and it keeps m = -inf, l = 0, O = 0 (exp(-inf - -inf) would be NaN)
//   O^T      = V^T . P^T: the two S^T accumulator tiles of the block, rounded to T, ARE the B operand — lane l holds row l & 15, and its element e stands for
//            key 16 (e >> 2) + 4 (l >> 4) + (e & 3), a permutation of the k index that A follows: A = V^T, lane l: dim l & 15 of the 16-dim tile, those 8 keys.
//            V is row-major by key: the block is staged through LDS (16-byte global loads, rows of keys >= k1 REPLACED BY ZERO: 0 * NaN is NaN inside an MFMA
//            and the cache beyond n_max may hold anything) and read transposed with ds_read_b64_tr_b16.  O stays in fp32 VGPRs, HD / 16 tiles
//   end      the waves' (m, l, O) are merged through LDS in wave order (no atomics); S == 1: out[i] = T(O / l) for i < rows; S > 1: the share's record goes
//            to ((i n_heads + h) S + sp) of the one-row kernels' workspace layout and attn_combine_kernel (block.hip) finishes over rows * n_heads heads
//   body     the algorithm is stated in attn_tile_core.h (attn_tile_body) over a tile and a K / V row source; attn_gqa.hip and attn_prefill.hip place other
//            tiles on it.  This file keeps the tile of a verify step: the rows' queries, positions and outputs
//   host     attn_check / attn_launch (attn_decode_core.h) and tile_launch (attn_tile_core.h) behind the entry's own check, the row limit
//
// Loads: a key row >= k1 is never read (K rows are clamped to k1 - 1 and masked, V rows are not loaded), so nothing at or beyond n_max <= L is touched.
// Padding rows (i >= rows) read no query memory — their fragment is zero, their position -1: every key masked — and write nothing.
// exp is expf under -ffp-contract=off, the function and flags tests/_router_cases.py's EXP_ULPS was measured with (tests/_tile_cases.py derives the band).
#include "block_math.h"
#include "attn_decode_core.h"
#include "attn_tile_core.h"

namespace hqq {

// the tile of a verify step: row i of the R rows of query head h; its split record is that of head i n_heads + h
template <int HD>
struct RowTile {
  int rows;
  const uint16_t* qh;   // q + h HD
  uint16_t* oh;         // out + h HD
  float* wh;            // ws + (h S + sp) (HD + 2)
  int64_t qstride, wstride;   // n_heads HD; n_heads S (HD + 2)
  __device__ __forceinline__ const uint16_t* q(int i) const { return qh + i * qstride; }
  __device__ __forceinline__ uint16_t* out(int i) const { return oh + i * qstride; }
  __device__ __forceinline__ float* rec(int i) const { return wh + i * wstride; }
};

// the tile body (attn_tile_core.h) on the cache of ONE sequence (served: Src = DenseKV<HD>), the rows' own positions
template <int HD, bool BF, class Src>
__global__ __launch_bounds__(TILE_WAVES * 64) void attn_tile_kernel(const uint16_t* __restrict__ q, const Src src, const int64_t* __restrict__ pos, int rows,
                                                                    uint16_t* __restrict__ out, int n_heads, int n_kv, int L, float scaling, int S,
                                                                    float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int h = blockIdx.x, sp = blockIdx.y, kvh = h / (n_heads / n_kv);
  const int row = threadIdx.x & 15;
  // a position outside [0, L) attends as if at the last slot (the one-row kernels' rule)
  int n_max = 0, pr = -1;
  for (int i = 0; i < rows; ++i) {
    const int64_t p_raw = pos[i];
    const int p = (p_raw >= 0 && p_raw < L) ? static_cast<int>(p_raw) : L - 1;
    n_max = p + 1 > n_max ? p + 1 : n_max;
    pr = i == row ? p : pr;
  }
  const auto kv = src.at(static_cast<int64_t>(kvh) * L);
  const RowTile<HD> tile{rows, q + static_cast<int64_t>(h) * HD, out + static_cast<int64_t>(h) * HD,
                         S > 1 ? ws + (static_cast<int64_t>(h) * S + sp) * (HD + 2) : nullptr, static_cast<int64_t>(n_heads) * HD, static_cast<int64_t>(n_heads) * S * (HD + 2)};
  attn_tile_body<HD, BF>(smem, tile, n_max, pr, sp, S, scaling, kv);
}

extern "C" {

int hqq_hip_attn_decode_tiled(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, int64_t rows, void* out, int64_t n_heads,
                              int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const char* who = "hqq_hip_attn_decode_tiled";
  clear_stale_error();
  // this entry's own: the rows are one MFMA tile (first: the shared front would take up to a batch's count of them)
  if (rows < 1 || rows > TILE_ROWS) { set_error("%s: rows must be 1..%d (got %lld)", who, TILE_ROWS, (long long)rows); return HQQ_ERR_SHAPE; }
  const AttnCall c{who, rows, n_heads, n_kv_heads, head_dim, cache_len, dtype, splits, workspace, workspace_bytes, out, stream};
  if (const int rc = attn_check(c, {q, k_cache, v_cache, pos_dev, out}, {q, k_cache, v_cache, out})) return rc;
  return attn_launch(c, [&](auto HDc, auto BFc) {
    constexpr int HD = decltype(HDc)::value;
    using Src = DenseKV<HD>;
    return tile_launch<&attn_tile_kernel<HD, decltype(BFc)::value, Src>, HD>(c, c.grid(1), static_cast<const uint16_t*>(q),
                                                                               Src{static_cast<const uint16_t*>(k_cache), static_cast<const uint16_t*>(v_cache)}, pos_dev,
                                                                               static_cast<int>(rows), static_cast<uint16_t*>(out), static_cast<int>(n_heads),
                                                                               static_cast<int>(n_kv_heads), static_cast<int>(cache_len), scaling, c.S(), c.ws());
  });
}

}  // extern "C"

}  // namespace hqq
