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
//   loaders  dense: plain 16-byte loads of the sequence's cache rows.  Quantised: kv_load8 (kv_load.h) on the six buffers — everything behind a loader is the one
//            body, so the quantised entry has the bits of the dense one on kv_dequantize's tensors with the same splits
//   host     attn_check / attn_launch (attn_decode_core.h) behind the entries' own checks: 1 <= G <= 16, then kv_check for the packed entry
// Nothing at or beyond pos[b] + 1 of a sequence's cache is read (the body never asks a loader for a row >= k1), in levels or in meta.  No atomics, no allocation.
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

template <int HD, bool BF>
__global__ __launch_bounds__(TILE_WAVES * 64) void attn_gqa_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                                   const int64_t* __restrict__ pos, uint16_t* __restrict__ out, int n_heads, int n_kv, int L,
                                                                   float scaling, int S, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const GroupTile<HD> tile = group_tile<HD>(q, out, ws, n_heads, n_kv, S);
  const int p = group_pos(pos, L);
  const int64_t r0 = (static_cast<int64_t>(blockIdx.z) * n_kv + blockIdx.x) * L;
  const uint16_t* K = kc + r0 * HD;
  const uint16_t* V = vc + r0 * HD;
  auto krow = [&](int ch, int j) -> u32x4 { return *reinterpret_cast<const u32x4*>(K + static_cast<int64_t>(j) * HD + 8 * ch); };
  auto vrow = [&](int ch, int j) -> u32x4 { return *reinterpret_cast<const u32x4*>(V + static_cast<int64_t>(j) * HD + 8 * ch); };
  attn_tile_body<HD, BF>(smem, tile, p + 1, (static_cast<int>(threadIdx.x) & 15) < tile.rows ? p : -1, blockIdx.y, S, scaling, krow, vrow);
}

template <int HD, int NBITS, bool BF>
__global__ __launch_bounds__(TILE_WAVES * 64) void attn_gqa_kvq_kernel(const uint16_t* __restrict__ q, const uint8_t* __restrict__ kq, const uint16_t* __restrict__ ks,
                                                                       const uint16_t* __restrict__ kz, const uint8_t* __restrict__ vq, const uint16_t* __restrict__ vs,
                                                                       const uint16_t* __restrict__ vz, const int64_t* __restrict__ pos, uint16_t* __restrict__ out,
                                                                       int n_heads, int n_kv, int L, int gs_shift, float scaling, int S, float* __restrict__ ws) {
  constexpr int RB = HD * NBITS / 8;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const GroupTile<HD> tile = group_tile<HD>(q, out, ws, n_heads, n_kv, S);
  const int p = group_pos(pos, L);
  const int NG = HD >> gs_shift;   // (scale, zero) pairs per row
  const int64_t r0 = (static_cast<int64_t>(blockIdx.z) * n_kv + blockIdx.x) * L;
  kq += r0 * RB; vq += r0 * RB;
  ks += r0 * NG; kz += r0 * NG; vs += r0 * NG; vz += r0 * NG;
  auto krow = [&](int ch, int j) -> u32x4 {
    const int64_t r = j;
    return kv_load8<HD, NBITS, BF>(kq + r * RB, ks + r * NG, kz + r * NG, ch, gs_shift);
  };
  auto vrow = [&](int ch, int j) -> u32x4 {
    const int64_t r = j;
    return kv_load8<HD, NBITS, BF>(vq + r * RB, vs + r * NG, vz + r * NG, ch, gs_shift);
  };
  attn_tile_body<HD, BF>(smem, tile, p + 1, (static_cast<int>(threadIdx.x) & 15) < tile.rows ? p : -1, blockIdx.y, S, scaling, krow, vrow);
}

// the entries' own check, before the shared front: the group is one MFMA tile
static inline int gqa_check(const char* who, int64_t n_heads, int64_t n_kv_heads) {
  if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads) return 0;   // (attn_check answers these)
  const int64_t G = n_heads / n_kv_heads;
  if (G > TILE_ROWS) { set_error("%s: not covered: G = n_heads / n_kv_heads = %lld (1..%d query heads per KV head)", who, (long long)G, TILE_ROWS); return HQQ_ERR_UNSUPPORTED; }
  return 0;
}

// the grid of a grouped launch: (n_kv_heads, splits, sequences)
static inline dim3 gqa_grid(const AttnCall& c) { return dim3(static_cast<unsigned>(c.n_kv_heads), static_cast<unsigned>(c.splits), static_cast<unsigned>(c.rows)); }

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
    constexpr auto kern = &attn_gqa_kernel<decltype(HDc)::value, decltype(BFc)::value>;
    constexpr int lds = tile_lds_bytes<decltype(HDc)::value>();
    static LdsRaised raised;   // (one per instantiation)
    if (const int rc = attn_raise_lds(raised, reinterpret_cast<const void*>(kern), lds, lds, who)) return rc;
    hipLaunchKernelGGL(kern, gqa_grid(c), dim3(TILE_WAVES * 64), lds, as_stream(stream), static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k_cache),
                       static_cast<const uint16_t*>(v_cache), pos_dev, static_cast<uint16_t*>(out), static_cast<int>(n_heads), static_cast<int>(n_kv_heads),
                       static_cast<int>(cache_len), scaling, c.S(), c.ws());
    return 0;
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
  const int gs_shift = group_size == 64 ? 6 : 5;
  return attn_launch(c, [&](auto HDc, auto BFc) {
    auto go = [&](auto NBc) {
      constexpr auto kern = &attn_gqa_kvq_kernel<decltype(HDc)::value, decltype(NBc)::value, decltype(BFc)::value>;
      constexpr int lds = tile_lds_bytes<decltype(HDc)::value>();
      static LdsRaised raised;   // (one per instantiation)
      if (const int rc = attn_raise_lds(raised, reinterpret_cast<const void*>(kern), lds, lds, who)) return rc;
      hipLaunchKernelGGL(kern, gqa_grid(c), dim3(TILE_WAVES * 64), lds, as_stream(stream), static_cast<const uint16_t*>(q), static_cast<const uint8_t*>(kq),
                         static_cast<const uint16_t*>(k_scale), static_cast<const uint16_t*>(k_zero), static_cast<const uint8_t*>(vq),
                         static_cast<const uint16_t*>(v_scale), static_cast<const uint16_t*>(v_zero), pos_dev, static_cast<uint16_t*>(out), static_cast<int>(n_heads),
                         static_cast<int>(n_kv_heads), static_cast<int>(cache_len), gs_shift, scaling, c.S(), c.ws());
      return 0;
    };
    return nbits == 8 ? go(std::integral_constant<int, 8>{}) : go(std::integral_constant<int, 4>{});
  });
}

}  // extern "C"

}  // namespace hqq
