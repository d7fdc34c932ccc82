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
//   host     the kernel is this file's own algorithm; its entry point goes through the host front of every decode-attention call (attn_decode_core.h: the
//            argument checks, the (head_dim, dtype) dispatch, the combine launch) and keeps only the row limit and its LDS size
//
// Loads: a key row >= k1 is never read (K rows are clamped to k1 - 1 and masked, V rows are not loaded), so nothing at or beyond n_max <= L is touched.
// Padding rows (i >= rows) read no query memory — their fragment is zero, their position -1: every key masked — and write nothing.
// exp is expf under -ffp-contract=off, the function and flags tests/_router_cases.py's EXP_ULPS was measured with (tests/_tile_cases.py derives the band).
#include "block_math.h"
#include "attn_decode_core.h"

namespace hqq {

constexpr int TILE_WAVES = 8, TILE_ROWS = 16, TILE_KEYS = 32;

typedef short tile_s4 __attribute__((ext_vector_type(4)));
typedef _Float16 tile_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 tile_b8 __attribute__((ext_vector_type(8)));

// bytes between two key rows of a wave's V image: 32 bytes of padding put the 4 rows of a transposed read's block, and the two blocks of a 32-lane half, on different banks
template <int HD>
constexpr int tile_vstride() { return HD * 2 + 32; }
template <int HD>
constexpr int tile_lds_bytes() { return TILE_WAVES * TILE_KEYS * tile_vstride<HD>() + TILE_WAVES * TILE_ROWS * 2 * 4; }

template <int HD, bool BF>
__global__ __launch_bounds__(TILE_WAVES * 64) void attn_tile_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                                    const int64_t* __restrict__ pos, int rows, uint16_t* __restrict__ out, int n_heads, int n_kv, int L,
                                                                    float scaling, int S, float* __restrict__ ws) {
  using E = El<BF>;
  constexpr int NC = HD / 32, NT = HD / 16, VS = tile_vstride<HD>(), IMG = TILE_KEYS * VS;
  static_assert(IMG >= TILE_ROWS * HD * 4, "a wave's V image also parks its output tile [16][HD] fp32 for the merge");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float* stat = reinterpret_cast<float*>(smem + TILE_WAVES * IMG);   // [wave][row][m, l]
  const int h = blockIdx.x, sp = blockIdx.y, kvh = h / (n_heads / n_kv);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, g = lane >> 4;
  // a position outside [0, L) attends as if at the last slot (the one-row kernels' rule)
  int n_max = 0, pr = -1;
  for (int i = 0; i < rows; ++i) {
    const int64_t p_raw = pos[i];
    const int p = (p_raw >= 0 && p_raw < L) ? static_cast<int>(p_raw) : L - 1;
    n_max = p + 1 > n_max ? p + 1 : n_max;
    pr = i == row ? p : pr;
  }
  const int chunk = (n_max + S - 1) / S;
  const int k0 = sp * chunk, k1 = (k0 + chunk < n_max) ? k0 + chunk : n_max;
  const int klim = pr < k1 - 1 ? pr : k1 - 1;   // the last key this lane's row takes from this share
  const int nb = k1 > k0 ? (k1 - k0 + TILE_KEYS - 1) / TILE_KEYS : 0;
  const uint16_t* K = kc + static_cast<int64_t>(kvh) * L * HD;
  const uint16_t* V = vc + static_cast<int64_t>(kvh) * L * HD;
  uint8_t* img = smem + wave * IMG;

  u32x4 qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    qf[c] = u32x4{0u, 0u, 0u, 0u};
    if (row < rows) qf[c] = *reinterpret_cast<const u32x4*>(q + (static_cast<int64_t>(row) * n_heads + h) * HD + 32 * c + 8 * g);
  }
  auto mfma = [&](const u32x4& A, const u32x4& B, f32x4 C) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tile_b8, A), __builtin_bit_cast(tile_b8, B), C, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(tile_h8, A), __builtin_bit_cast(tile_h8, B), C, 0, 0, 0);
  };
  float m = -INFINITY, l = 0.f;
  f32x4 o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int b = wave; b < nb; b += TILE_WAVES) {   // (wave-uniform: every lane of the wave is active at the transposed reads)
    const int j0 = k0 + TILE_KEYS * b;
    u32x4 kf[2][NC];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = j0 + 16 * t + row;
      const uint16_t* kr = K + static_cast<int64_t>(key < k1 ? key : k1 - 1) * HD + 8 * g;
#pragma unroll
      for (int c = 0; c < NC; ++c) kf[t][c] = *reinterpret_cast<const u32x4*>(kr + 32 * c);
    }
    // the V block: 32 rows of HD / 8 16-byte chunks, HD / 16 chunks per lane, consecutive lanes on consecutive chunks
    u32x4 vf[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int x = lane + 64 * u, vr = x / (HD / 8), ch = x % (HD / 8);
      vf[u] = u32x4{0u, 0u, 0u, 0u};
      if (j0 + vr < k1) vf[u] = *reinterpret_cast<const u32x4*>(V + static_cast<int64_t>(j0 + vr) * HD + 8 * ch);
    }
    float s[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c) acc = mfma(kf[t][c], qf[c], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) s[4 * t + r] = (j0 + 16 * t + 4 * g + r <= klim) ? acc[r] * scaling : -INFINITY;
    }
    float bm = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7])));
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float m_new = fmaxf(m, bm);
    const float m_sub = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = expf(m - m_sub);
    float p[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] = expf(s[e] - m_sub);
    float ps = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = m_new;
    u32x4 pf;
#pragma unroll
    for (int e = 0; e < 4; ++e) pf[e] = static_cast<uint32_t>(E::r(p[2 * e])) | (static_cast<uint32_t>(E::r(p[2 * e + 1])) << 16);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[t][r] *= alpha;
    // V through the wave's own LDS image (the LDS operations of a wave execute in order: the fences only keep the compiler from moving them)
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int x = lane + 64 * u, vr = x / (HD / 8), ch = x % (HD / 8);
      *reinterpret_cast<u32x4*>(img + vr * VS + 16 * ch) = vf[u];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // transposed read: lane 4 qq + pp of a 16-lane group gives the address of row qq, columns 4 pp .. of a 4 x 16 block and receives column (lane & 15) of
    // its 4 rows: block rows = keys 4 g .. 4 g + 3 (then 16 + 4 g ..), columns = the 16 dims of tile t
    const uint8_t* tr = img + (4 * g + (row >> 2)) * VS + 8 * (row & 3);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const tile_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tile_s4*)(tr + 32 * t));
      const tile_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tile_s4*)(tr + 16 * VS + 32 * t));
      const u32x2 lo2 = __builtin_bit_cast(u32x2, lo), hi2 = __builtin_bit_cast(u32x2, hi);
      const uint32_t a0 = lo2[0], a1 = lo2[1], a2 = hi2[0], a3 = hi2[1];
      o[t] = mfma(u32x4{a0, a1, a2, a3}, pf, o[t]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  // ---- merge the waves' (m, l, O) in wave order.  A wave parks its tile [row][HD] fp32 in its own image; lane (row, g) holds dims 16 t + 4 g + r ----
  {
    float* oi = reinterpret_cast<float*>(img);
#pragma unroll
    for (int t = 0; t < NT; ++t) *reinterpret_cast<f32x4*>(oi + row * HD + 16 * t + 4 * g) = o[t];
    if (g == 0) { stat[(wave * TILE_ROWS + row) * 2] = m; stat[(wave * TILE_ROWS + row) * 2 + 1] = l; }
  }
  __syncthreads();
  for (int e = tid; e < rows * HD; e += TILE_WAVES * 64) {
    const int i = e / HD, d = e - i * HD;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < TILE_WAVES; ++w) mm = fmaxf(mm, stat[(w * TILE_ROWS + i) * 2]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < TILE_WAVES; ++w) {
      const float lw = stat[(w * TILE_ROWS + i) * 2 + 1];
      const float wt = lw > 0.f ? expf(stat[(w * TILE_ROWS + i) * 2] - mm) : 0.f;   // (a wave without a visible key: m = -inf, l = 0, O = 0)
      num = fmaf(wt, reinterpret_cast<const float*>(smem + w * IMG)[i * HD + d], num);
      den = fmaf(wt, lw, den);
    }
    if (S == 1) {
      out[(static_cast<int64_t>(i) * n_heads + h) * HD + d] = E::r(num / den);
    } else {   // (a share wholly behind the row's position: max -inf, sum 0, output 0 — the record attn_combine_kernel gives weight 0)
      float* rec = ws + ((static_cast<int64_t>(i) * n_heads + h) * S + sp) * (HD + 2);
      rec[2 + d] = num;
      if (d == 0) { rec[0] = mm; rec[1] = den; }
    }
  }
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
    constexpr auto kern = &attn_tile_kernel<decltype(HDc)::value, decltype(BFc)::value>;
    constexpr int lds = tile_lds_bytes<decltype(HDc)::value>();
    static LdsRaised raised;   // (one per instantiation)
    if (const int rc = attn_raise_lds(raised, reinterpret_cast<const void*>(kern), lds, lds, who)) return rc;
    hipLaunchKernelGGL(kern, c.grid(1), dim3(TILE_WAVES * 64), lds, as_stream(stream), static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(k_cache),
                       static_cast<const uint16_t*>(v_cache), pos_dev, static_cast<int>(rows), static_cast<uint16_t*>(out), static_cast<int>(n_heads),
                       static_cast<int>(n_kv_heads), static_cast<int>(cache_len), scaling, c.S(), c.ws());
    return 0;
  });
}

}  // extern "C"

}  // namespace hqq
