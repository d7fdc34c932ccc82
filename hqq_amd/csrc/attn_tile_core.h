// attn_tile_core.h — the MFMA query-tile attention, stated once: a kernel is a PLACEMENT (attn_tile.hip, attn_gqa.hip, attn_prefill.hip) times a row SOURCE
// (DenseKV here, PackedKV in kv_load.h), and each hands attn_tile_body what differs.
//   tile    where tile row t's query, output and split record live (a struct with rows, q(t), out(t), rec(t)); the positions arrive as n_max (1 + the largest
//           clamped position of the tile) and pr (the clamped position of THIS lane's row, -1 for a padding row: every key masked)
//   source  a POD kernel argument; at(r0) gives the rows of one (sequence, KV head) from row r0 of the cache, with k(ch, j) / v(ch, j) -> u32x4: a lane's 8 dims
//           (chunk ch of HD / 8) of key / value row j as T.  Lane (row, g) takes chunks 4 c + g of its key; a V block is chunk x % (HD / 8) of row x / (HD / 8)
// The algorithm is described at the head of attn_tile.hip.  Translation units that use the body are compiled with -ffp-contract=off (expf under the flags its
// error was measured with).
#pragma once
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

// ---- the dense cache as a row source: plain 16-byte loads of rows of HD values ----
template <int HD>
struct DenseKV {
  const uint16_t* kc;
  const uint16_t* vc;
  struct Rows {
    const uint16_t* K;
    const uint16_t* V;
    __device__ __forceinline__ u32x4 k(int ch, int j) const { return *reinterpret_cast<const u32x4*>(K + static_cast<int64_t>(j) * HD + 8 * ch); }
    __device__ __forceinline__ u32x4 v(int ch, int j) const { return *reinterpret_cast<const u32x4*>(V + static_cast<int64_t>(j) * HD + 8 * ch); }
  };
  __device__ __forceinline__ Rows at(int64_t r0) const { return Rows{kc + r0 * HD, vc + r0 * HD}; }
};

// ---- the attention of one workgroup (TILE_WAVES * 64 threads) over share sp of keys [0, n_max) for the rows of `tile`, keys and values from `kv` (a source's rows);
//      smem: tile_lds_bytes<HD>() ----
template <int HD, bool BF, class Tile, class Rows>
__device__ __forceinline__ void attn_tile_body(uint8_t* smem, const Tile& tile, int n_max, int pr, int sp, int S, float scaling, const Rows& kv) {
  // (the two loaders as closures, not kv.k / kv.v called in place: in place, the compiler hoists one address computation elsewhere and the dense grouped kernels
  //  lose the instruction-for-instruction identity that profiles/attn_tile_family_parity.md records)
  auto krow = [&](int ch, int j) -> u32x4 { return kv.k(ch, j); };
  auto vrow = [&](int ch, int j) -> u32x4 { return kv.v(ch, j); };
  using E = El<BF>;
  constexpr int NC = HD / 32, NT = HD / 16, VS = tile_vstride<HD>(), IMG = TILE_KEYS * VS;
  static_assert(IMG >= TILE_ROWS * HD * 4, "a wave's V image also parks its output tile [16][HD] fp32 for the merge");
  float* stat = reinterpret_cast<float*>(smem + TILE_WAVES * IMG);   // [wave][row][m, l]
  const int rows = tile.rows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, g = lane >> 4;
  const int chunk = (n_max + S - 1) / S;
  const int k0 = sp * chunk, k1 = (k0 + chunk < n_max) ? k0 + chunk : n_max;
  const int klim = pr < k1 - 1 ? pr : k1 - 1;   // the last key this lane's row takes from this share
  const int nb = k1 > k0 ? (k1 - k0 + TILE_KEYS - 1) / TILE_KEYS : 0;
  uint8_t* img = smem + wave * IMG;

  u32x4 qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    qf[c] = u32x4{0u, 0u, 0u, 0u};
    if (row < rows) qf[c] = *reinterpret_cast<const u32x4*>(tile.q(row) + 32 * c + 8 * g);
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
      const int kj = key < k1 ? key : k1 - 1;
#pragma unroll
      for (int c = 0; c < NC; ++c) kf[t][c] = krow(4 * c + g, kj);
    }
    // the V block: 32 rows of HD / 8 16-byte chunks, HD / 16 chunks per lane, consecutive lanes on consecutive chunks
    u32x4 vf[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int x = lane + 64 * u, vr = x / (HD / 8), ch = x % (HD / 8);
      vf[u] = u32x4{0u, 0u, 0u, 0u};
      if (j0 + vr < k1) vf[u] = vrow(ch, j0 + vr);
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
      tile.out(i)[d] = E::r(num / den);
    } else {   // (a share wholly behind the row's position: max -inf, sum 0, output 0 — the record attn_combine_kernel gives weight 0)
      float* rec = tile.rec(i);
      rec[2 + d] = num;
      if (d == 0) { rec[0] = mm; rec[1] = den; }
    }
  }
}

// ---- the launch of one instantiation of the family: Kern's LDS limit raised once per device (tile_lds_bytes<HD>() passes 48 KiB at head_dim 128 and 256), then the
//      workgroups of TILE_WAVES waves.  0 or the error code with c.who's message ----
template <auto Kern, int HD, class... Args>
static inline int tile_launch(const AttnCall& c, dim3 grid, Args... args) {
  constexpr int lds = tile_lds_bytes<HD>();
  static LdsRaised raised;   // (one per instantiation)
  if (const int rc = attn_raise_lds(raised, reinterpret_cast<const void*>(Kern), lds, lds, c.who)) return rc;
  hipLaunchKernelGGL(Kern, grid, dim3(TILE_WAVES * 64), lds, as_stream(c.stream), args...);
  return 0;
}

}  // namespace hqq
