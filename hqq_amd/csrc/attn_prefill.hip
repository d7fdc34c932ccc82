// attn_prefill.hip — causal attention of a PROMPT that reads only the causal part of the static cache (include/hqq_hip.h, hqq_hip_attn_prefill and
// hqq_hip_attn_prefill_kvq), gfx950.
//
// The model's own prefill scores the T rows of a prompt against all L slots of the static cache under a [T, L] mask — and on the quantised cache dequantises all L
// slots of every layer first.  Here a prompt is a stack of attn_tile.hip's tiles: the grid is (n_heads, ceil(T / 16)), and workgroup (h, j) takes rows
// 16 j .. min(16 j + 15, T - 1) of query head h — 16 consecutive positions — as the rows of one MFMA query tile and runs attn_tile_body (attn_tile_core.h; the
// algorithm is described at the head of attn_tile.hip) over keys [0, n_max), n_max = pos0 + min(16 j + 16, T): each key is read once for the tile.
//   tile     row i is position pos0 + 16 j + i: its query q + (16 j + i) q_row_stride + h q_head_stride (strides in elements, so HF's [1, H, T, hd] view of the
//            projection's [T, H hd] output goes in as it is), its output out[16 j + i][h] of the dense [T, n_heads, hd] that o_proj takes.  Its causal limit is its
//            own position; padding rows of the last tile (-1: every key masked) hold a zero fragment, read no query memory and write nothing
//   share    ONE per tile (sp = 0, S = 1): no split, no workspace, no merging launch, the record slot of the tile struct is never used.  Measured
//            (profiles/prefill_attn_summary.md): level with SDPA on the whole cache at 128 / 512 tokens, but NOT enough for long prompts — at 8192 tokens 2.97 ms per
//            block against 1.47 on the dense cache, 5.2 - 6.3 against 1.5 on the quantised one: 16-row tiles re-read K and V T / 16 times
//   order    the tiles with the most keys take the lowest block indices, so the long ones start first (a supposition about the tail, not a measured result)
//   source   attn_prefill_kernel<HD, BF, Src> on DenseKV (attn_tile_core.h) or PackedKV (kv_load.h): everything behind the source is the one body, so the
//            quantised entry has the bits of the dense one on kv_dequantize's tensors
//   host     attn_check / attn_launch / tile_launch behind the entries' own checks: T >= 1, pos0 >= 0, pos0 + T <= cache_len (a prompt that does not fit is an
//            error: there is no "attend at the last slot" rule here), strides that keep every query row 16-byte aligned; then kv_check for the packed entry
// Rows 16 j .. of head h have the bits of hqq_hip_attn_decode_tiled on those queries with pos = pos0 + 16 j + i and splits = 1: the same body, n_max and deal of
// blocks to waves.  Nothing at or beyond pos0 + T is read (the body never asks the source for a row >= n_max), in levels, meta or dense rows.  No atomics, no allocation.
// NOT built here: sharing between the query heads of a KV group (tiles are per query head, so the G heads of a group re-read the same K and V rows; a tile of
// G heads x 16 / G positions is the follow-up), query tiles of more than 16 rows for very long prompts, and several sequences per launch.
// Compiled with attn_tile.hip's flags.
#include "block_math.h"
#include "attn_decode_core.h"
#include "attn_tile_core.h"
#include "kv_load.h"

namespace hqq {

// the tile of a prompt: row i is position pos0 + 16 j + i of query head h (q0 / o0: that head's row 16 j of q / out)
template <int HD>
struct PrefillTile {
  int rows;
  const uint16_t* q0;   // q + 16 j q_row_stride + h q_head_stride
  uint16_t* o0;         // out + (16 j n_heads + h) HD
  int64_t qstride, ostride;   // q_row_stride; n_heads HD
  __device__ __forceinline__ const uint16_t* q(int i) const { return q0 + i * qstride; }
  __device__ __forceinline__ uint16_t* out(int i) const { return o0 + i * ostride; }
  __device__ __forceinline__ float* rec(int) const { return nullptr; }   // (S == 1: never asked)
};

// where workgroup (h, j) stands: its first row t0 = 16 j, its tile, and n_max / this lane's causal limit through the references
template <int HD>
__device__ __forceinline__ PrefillTile<HD> prefill_tile(const uint16_t* q, int64_t qrs, int64_t qhs, uint16_t* out, int pos0, int T, int n_heads, int& n_max, int& pr) {
  const int h = blockIdx.x;
  const int j = gridDim.y - 1 - blockIdx.y;   // the longest tiles first
  const int t0 = TILE_ROWS * j;
  const int rows = T - t0 < TILE_ROWS ? T - t0 : TILE_ROWS;
  const int row = static_cast<int>(threadIdx.x) & 15;
  n_max = pos0 + t0 + rows;
  pr = row < rows ? pos0 + t0 + row : -1;
  return PrefillTile<HD>{rows, q + t0 * qrs + h * qhs, out + (static_cast<int64_t>(t0) * n_heads + h) * HD, qrs, static_cast<int64_t>(n_heads) * HD};
}

template <int HD, bool BF, class Src>
__global__ __launch_bounds__(TILE_WAVES * 64) void attn_prefill_kernel(const uint16_t* __restrict__ q, int64_t qrs, int64_t qhs, const Src src, int pos0, int T,
                                                                       uint16_t* __restrict__ out, int n_heads, int n_kv, int L, float scaling) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int n_max, pr;
  const PrefillTile<HD> tile = prefill_tile<HD>(q, qrs, qhs, out, pos0, T, n_heads, n_max, pr);
  const int kvh = blockIdx.x / (n_heads / n_kv);
  const auto kv = src.at(static_cast<int64_t>(kvh) * L);
  attn_tile_body<HD, BF>(smem, tile, n_max, pr, 0, 1, scaling, kv);
}

// the entries' own checks, before the shared front: the prompt fits the cache and every query row is 16-byte aligned
static inline int prefill_check(const char* who, int64_t pos0, int64_t T, int64_t cache_len, int64_t q_row_stride, int64_t q_head_stride) {
  if (T < 1 || pos0 < 0 || cache_len < 1 || pos0 > cache_len || T > cache_len - pos0) {
    set_error("%s: rows at positions %lld .. %lld do not fit a cache of %lld (T >= 1, pos0 >= 0, pos0 + T <= cache_len)", who, (long long)pos0,
              (long long)(pos0 + T - 1), (long long)cache_len);
    return HQQ_ERR_SHAPE;
  }
  if (q_row_stride < 0 || q_head_stride < 0 || q_row_stride % 8 || q_head_stride % 8) {
    set_error("%s: q_row_stride %lld / q_head_stride %lld must be non-negative multiples of 8 elements", who, (long long)q_row_stride, (long long)q_head_stride);
    return HQQ_ERR_ALIGN;
  }
  return 0;
}

// a prompt's launch on source `src`: the grid is (n_heads, tiles of 16 rows); c.rows: the prompt's
template <int HD, bool BF, class Src>
static inline int prefill_launch(const AttnCall& c, const void* q, int64_t q_row_stride, int64_t q_head_stride, const Src& src, int64_t pos0, float scaling) {
  const dim3 grid(static_cast<unsigned>(c.n_heads), static_cast<unsigned>((c.rows + TILE_ROWS - 1) / TILE_ROWS));
  return tile_launch<&attn_prefill_kernel<HD, BF, Src>, HD>(c, grid, static_cast<const uint16_t*>(q), q_row_stride, q_head_stride, src, static_cast<int>(pos0),
                                                            static_cast<int>(c.rows), static_cast<uint16_t*>(c.out), static_cast<int>(c.n_heads),
                                                            static_cast<int>(c.n_kv_heads), static_cast<int>(c.cache_len), scaling);
}

extern "C" {

int hqq_hip_attn_prefill(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_cache, const void* v_cache, int64_t pos0, int64_t T, void* out,
                         int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, void* stream) {
  const char* who = "hqq_hip_attn_prefill";
  clear_stale_error();
  if (const int rc = prefill_check(who, pos0, T, cache_len, q_row_stride, q_head_stride)) return rc;
  const AttnCall c{who, T, n_heads, n_kv_heads, head_dim, cache_len, dtype, 1, nullptr, 0, out, stream};   // (rows: the prompt's; one share)
  if (const int rc = attn_check(c, {q, k_cache, v_cache, out}, {q, k_cache, v_cache, out})) return rc;
  return attn_launch(c, [&](auto HDc, auto BFc) {
    constexpr int HD = decltype(HDc)::value;
    return prefill_launch<HD, decltype(BFc)::value>(c, q, q_row_stride, q_head_stride, DenseKV<HD>{static_cast<const uint16_t*>(k_cache), static_cast<const uint16_t*>(v_cache)},
                                                    pos0, scaling);
  });
}

int hqq_hip_attn_prefill_kvq(int nbits, const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* kq, const void* k_scale, const void* k_zero,
                             const void* vq, const void* v_scale, const void* v_zero, int64_t pos0, int64_t T, void* out, int64_t n_heads, int64_t n_kv_heads,
                             int64_t head_dim, int64_t group_size, int64_t cache_len, float scaling, int dtype, void* stream) {
  const char* who = "hqq_hip_attn_prefill_kvq";
  clear_stale_error();
  if (const int rc = prefill_check(who, pos0, T, cache_len, q_row_stride, q_head_stride)) return rc;
  if (const int rc = kv_check(who, nbits, head_dim, group_size, cache_len, dtype)) return rc;   // (the cache's coverage rule answers with its own code)
  const AttnCall c{who, T, n_heads, n_kv_heads, head_dim, cache_len, dtype, 1, nullptr, 0, out, stream};
  if (const int rc = attn_check(c, {q, kq, k_scale, k_zero, vq, v_scale, v_zero, out}, {q, kq, vq, out})) return rc;
  int rc = 0;
  kv_dispatch(head_dim, nbits, c.bf(), [&](auto HDc, auto NBc, auto BFc) {
    constexpr int HD = decltype(HDc)::value;
    constexpr bool BF = decltype(BFc)::value;
    rc = prefill_launch<HD, BF>(c, q, q_row_stride, q_head_stride, PackedKV<HD, decltype(NBc)::value, BF>::of(kq, k_scale, k_zero, vq, v_scale, v_zero, group_size), pos0,
                                scaling);
  });
  return attn_finish(c, rc);
}

}  // extern "C"

}  // namespace hqq
