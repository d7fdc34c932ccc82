// attn_gqa.hip — decode attention that reads each key ONCE per KV-head group (include/hqq_hip.h, hqq_hip_attn_decode_gqa_batched and
// hqq_hip_attn_decode_gqa_kvq_batched), gfx950.
//
// The one-row kernels (attn_decode_kernel in block.hip, attn_decode_kvq_kernel in kv_cache.hip) hand a workgroup one QUERY head: on a grouped-query model the
// G = n_heads / n_kv_heads heads of a group each stream — and on the quantised cache each rebuild — the same K and V rows of their KV head.  Here the grid is
// (n_kv_heads, splits, sequences): workgroup (kvh, sp, b) takes heads kvh G .. kvh G + G - 1 of sequence b as the rows of one MFMA query tile, padded to 16, and
// runs attn_tile_body (attn_tile_core.h; the algorithm is described at the head of attn_tile.hip) over share sp of keys [0, pos[b]]: every key is read, and a
// packed key rebuilt, once per group.
//   tile     row u is head kvh G + u: its query q[b][kvh G + u], its output out[b][kvh G + u], its split record ((b n_heads + kvh G + u) S + sp) of the one-row
//            kernels' workspace layout, so that attn_combine_kernel (block.hip) finishes a split call as it finishes theirs.  Padding rows (u >= G) hold a zero
//            fragment, read no query memory and write nothing
//   position all rows share pos[b], clamped as the one-row kernels clamp it (outside [0, L): the last slot); chunk = ceil((pos[b] + 1) / S), empty shares allowed
//   source   attn_gqa_kernel<HD, BF, Src> on DenseKV (attn_tile_core.h) or PackedKV (kv_load.h): everything behind the source is the one body, so the quantised
//            entry has the bits of the dense one on kv_dequantize's tensors with the same splits
//   host     attn_check / attn_launch / tile_launch behind the entries' own checks: 1 <= G <= 16, then kv_check for the packed entry
// Nothing at or beyond pos[b] + 1 of a sequence's cache is read (the body never asks the source for a row >= k1), in levels or in meta.  No atomics, no allocation.
// Compiled with attn_tile.hip's flags.
#include "block_math.h"
#include "attn_decode_core.h"
#include "attn_tile_core.h"
#include "kv_load.h"

namespace hqq {

// the tile of a KV group: row u is query head h0 + u of the workgroup's sequence (qb / ob: that sequence's q / out; wb: its records at share sp)
template <int HD>
struct GroupTile {
  int rows;
  const uint16_t* qb;   // q + (b n_heads + h0) HD
  uint16_t* ob;         // out + (b n_heads + h0) HD
  float* wb;            // ws + ((b n_heads + h0) S + sp) (HD + 2)
  int wstride;          // S (HD + 2)
  __device__ __forceinline__ const uint16_t* q(int u) const { return qb + u * HD; }
  __device__ __forceinline__ uint16_t* out(int u) const { return ob + u * HD; }
  __device__ __forceinline__ float* rec(int u) const { return wb + static_cast<int64_t>(u) * wstride; }
};

template <int HD>
__device__ __forceinline__ GroupTile<HD> group_tile(const uint16_t* q, uint16_t* out, float* ws, int n_heads, int n_kv, int S) {
  const int G = n_heads / n_kv, kvh = blockIdx.x, sp = blockIdx.y;
  const int64_t h0 = static_cast<int64_t>(blockIdx.z) * n_heads + static_cast<int64_t>(kvh) * G;   // the group's first head among all sequences'
  return GroupTile<HD>{G, q + h0 * HD, out + h0 * HD, S > 1 ? ws + (h0 * S + sp) * (HD + 2) : nullptr, S * (HD + 2)};
}

// a position outside [0, L) attends as if at the last slot (the one-row kernels' rule)
__device__ __forceinline__ int group_pos(const int64_t* __restrict__ pos, int L) {
  const int64_t p_raw = pos[blockIdx.z];
  return (p_raw >= 0 && p_raw < L) ? static_cast<int>(p_raw) : L - 1;
}

template <int HD, bool BF, class Src>
__global__ __launch_bounds__(TILE_WAVES * 64) void attn_gqa_kernel(const uint16_t* __restrict__ q, const Src src, const int64_t* __restrict__ pos,
                                                                   uint16_t* __restrict__ out, int n_heads, int n_kv, int L, float scaling, int S,
                                                                   float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const GroupTile<HD> tile = group_tile<HD>(q, out, ws, n_heads, n_kv, S);
  const int p = group_pos(pos, L);
  const auto kv = src.at((static_cast<int64_t>(blockIdx.z) * n_kv + blockIdx.x) * L);   // the sequence's rows of this KV head
  attn_tile_body<HD, BF>(smem, tile, p + 1, (static_cast<int>(threadIdx.x) & 15) < tile.rows ? p : -1, blockIdx.y, S, scaling, kv);
}

// the entries' own check, before the shared front: the group is one MFMA tile
static inline int gqa_check(const char* who, int64_t n_heads, int64_t n_kv_heads) {
  if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads) return 0;   // (attn_check answers these)
  const int64_t G = n_heads / n_kv_heads;
  if (G > TILE_ROWS) { set_error("%s: not covered: G = n_heads / n_kv_heads = %lld (1..%d query heads per KV head)", who, (long long)G, TILE_ROWS); return HQQ_ERR_UNSUPPORTED; }
  return 0;
}

// a grouped launch on source `src`: the grid is (n_kv_heads, splits, sequences)
template <int HD, bool BF, class Src>
static inline int gqa_launch(const AttnCall& c, const void* q, const Src& src, const int64_t* pos_dev, float scaling) {
  const dim3 grid(static_cast<unsigned>(c.n_kv_heads), static_cast<unsigned>(c.splits), static_cast<unsigned>(c.rows));
  return tile_launch<&attn_gqa_kernel<HD, BF, Src>, HD>(c, grid, static_cast<const uint16_t*>(q), src, pos_dev, static_cast<uint16_t*>(c.out), static_cast<int>(c.n_heads),
                                                        static_cast<int>(c.n_kv_heads), static_cast<int>(c.cache_len), scaling, c.S(), c.ws());
}

extern "C" {

int hqq_hip_attn_decode_gqa_batched(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads,
                                    int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* who = "hqq_hip_attn_decode_gqa_batched";
  clear_stale_error();
  if (const int rc = gqa_check(who, n_heads, n_kv_heads)) return rc;
  const AttnCall c{who, batch, n_heads, n_kv_heads, head_dim, cache_len, dtype, splits, workspace, workspace_bytes, out, stream};
  if (const int rc = attn_check(c, {q, k_cache, v_cache, pos_dev, out}, {q, k_cache, v_cache, out})) return rc;
  return attn_launch(c, [&](auto HDc, auto BFc) {
    constexpr int HD = decltype(HDc)::value;
    return gqa_launch<HD, decltype(BFc)::value>(c, q, DenseKV<HD>{static_cast<const uint16_t*>(k_cache), static_cast<const uint16_t*>(v_cache)}, pos_dev, scaling);
  });
}

int hqq_hip_attn_decode_gqa_kvq_batched(int nbits, const void* q, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale,
                                        const void* v_zero, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim,
                                        int64_t group_size, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  const char* who = "hqq_hip_attn_decode_gqa_kvq_batched";
  clear_stale_error();
  if (const int rc = gqa_check(who, n_heads, n_kv_heads)) return rc;
  if (const int rc = kv_check(who, nbits, head_dim, group_size, cache_len, dtype)) return rc;   // (the cache's coverage rule answers with its own code)
  const AttnCall c{who, batch, n_heads, n_kv_heads, head_dim, cache_len, dtype, splits, workspace, workspace_bytes, out, stream};
  if (const int rc = attn_check(c, {q, kq, k_scale, k_zero, vq, v_scale, v_zero, pos_dev, out}, {q, kq, vq, out})) return rc;
  int rc = 0;
  kv_dispatch(head_dim, nbits, c.bf(), [&](auto HDc, auto NBc, auto BFc) {
    constexpr int HD = decltype(HDc)::value;
    constexpr bool BF = decltype(BFc)::value;
    rc = gqa_launch<HD, BF>(c, q, PackedKV<HD, decltype(NBc)::value, BF>::of(kq, k_scale, k_zero, vq, v_scale, v_zero, group_size), pos_dev, scaling);
  });
  return attn_finish(c, rc);
}

}  // extern "C"

}  // namespace hqq
