// dgrad_common.h — what the two backward-through-weights kernels share (gemm_dgrad.hip: axis-1 layers, gemm_dgrad_axis0.hip: axis-0 layers): the tile
// constants, the 4 x 4 byte transpose of the container, the A operand of g, one slab's rebuild + MFMAs on meta given PER K OF THE LANE, and the fixed
// reduce tree + store.  The container is the same [N / per, K] byte array on both axes (byte [p, k] holds rows p + slab * N / per); only where the
// constants live differs, so each kernel builds the meta pairs its own way and everything else is one definition.
#pragma once
#include "axis0_common.h"

namespace hqq {

constexpr int DG_WAVES = 8;             // waves per workgroup: the N walk is dealt out over them
constexpr int DG_KT = 64;               // k per output tile: 4 per lane of a 16-lane group
constexpr int DG_BT = 4;                // 16-row tiles of g per workgroup
constexpr int DG_PASS_M = 16 * DG_BT;
constexpr int DG_STEP = 32;             // packed rows per step: 8 per lane group

typedef f32x4 dg_red_t[4 * DG_BT][64];  // one wave's partial tile in LDS; the reduce buffer is dg_red_t[DG_WAVES / 2] = 64 KiB

// 4 x 4 byte transpose: in[r] = bytes (k0..k3) of row r  ->  out[i] = byte i of rows (0, 1, 2, 3)
static __device__ __forceinline__ u32x4 dg_transpose(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3) {
  const uint32_t a = __builtin_amdgcn_perm(r1, r0, 0x05010400u);   // (r0b0, r1b0, r0b1, r1b1)
  const uint32_t b = __builtin_amdgcn_perm(r1, r0, 0x07030602u);   // (r0b2, r1b2, r0b3, r1b3)
  const uint32_t c = __builtin_amdgcn_perm(r3, r2, 0x05010400u);
  const uint32_t d = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
  return u32x4{__builtin_amdgcn_perm(c, a, 0x05040100u), __builtin_amdgcn_perm(c, a, 0x07060302u),
               __builtin_amdgcn_perm(d, b, 0x05040100u), __builtin_amdgcn_perm(d, b, 0x07060302u)};
}

// the lane's rows of g for one step: per slab and live 16-row tile, g[m, slab * Np + pc .. + 7] in the order the rebuilt quads have (permute_x8); rows
// past M and lane groups past the end of the container contribute zeros
template <int PER, int NBT>
static __device__ __forceinline__ void dg_load_g(const uint16_t* const (&grow)[NBT], const bool (&mv)[NBT], int Np, int pc, bool live,
                                                 u32x4 (&ga)[PER][NBT]) {
#pragma unroll
  for (int j = 0; j < PER; ++j)
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
      u32x4 v = ld16(grow[bt] + static_cast<int64_t>(j) * Np + pc);
      if (!(live && mv[bt])) v = u32x4{0u, 0u, 0u, 0u};
      ga[j][bt] = permute_x8(v);
    }
}

// one slab of one step.  tlo / thi: the transposed bytes of rows 0..3 / 4..7 (dword i = k i of the lane).  zp / sp [h][2 i + b]: (zero, scale) of k i for
// the rows (4 h + b, 4 h + b + 2), low half the first — the pairs rebuild_* takes.  Rebuilds the lane's 8 rows x 4 k of slab SL, then 4 MFMAs (one per k
// of the lane) per live tile of g
template <int NBITS, bool BF16, int SL, int NBT>
static __device__ __forceinline__ void dg_slab(const u32x4& tlo, const u32x4& thi, const uint32_t (&zp)[2][8], const uint32_t (&sp)[2][8],
                                               const u32x4 (&ga)[8 / NBITS][NBT], f32x4 (&acc)[NBT][4], uint32_t magic) {
  u32x4 lo0, lo1, hi0, hi1;   // lo0 = k 0, 1 of rows 0..3; lo1 = k 2, 3 of rows 0..3; hi*: rows 4..7
  if constexpr (!BF16) {
    half2_t zz[2][8], ss[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 8; ++i) { zz[h][i] = as_h2(zp[h][i]); ss[h][i] = as_h2(sp[h][i]); }
    h8_t a0, a1;
    rebuild_f16<NBITS, SL>(tlo, zz[0], ss[0], a0, a1, magic);
    lo0 = __builtin_bit_cast(u32x4, a0); lo1 = __builtin_bit_cast(u32x4, a1);
    rebuild_f16<NBITS, SL>(thi, zz[1], ss[1], a0, a1, magic);
    hi0 = __builtin_bit_cast(u32x4, a0); hi1 = __builtin_bit_cast(u32x4, a1);
  } else {
    bf16x8_t a0, a1;
    rebuild_bf16<NBITS, SL>(tlo, zp[0], sp[0], a0, a1);
    lo0 = __builtin_bit_cast(u32x4, a0); lo1 = __builtin_bit_cast(u32x4, a1);
    rebuild_bf16<NBITS, SL>(thi, zp[1], sp[1], a0, a1);
    hi0 = __builtin_bit_cast(u32x4, a0); hi1 = __builtin_bit_cast(u32x4, a1);
  }
  // B operand of output column k0 + 4 c + i: rows (0, 2, 1, 3, 4, 6, 5, 7) of the lane's eight
  const u32x4 bq[4] = {u32x4{lo0[0], lo0[1], hi0[0], hi0[1]}, u32x4{lo0[2], lo0[3], hi0[2], hi0[3]},
                       u32x4{lo1[0], lo1[1], hi1[0], hi1[1]}, u32x4{lo1[2], lo1[3], hi1[2], hi1[3]}};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
      if constexpr (!BF16)
        acc[bt][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, ga[SL][bt]), __builtin_bit_cast(h8_t, bq[i]), acc[bt][i], 0, 0, 0);
      else
        acc[bt][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ga[SL][bt]), __builtin_bit_cast(bf16x8_t, bq[i]), acc[bt][i], 0, 0, 0);
    }
}

// the eight partial tiles, added through LDS in a fixed tree — wave w += wave w + 4, then + 2, then + 1: ((0+4)+(2+6)) + ((1+5)+(3+7)) —, rounded once
// and stored by wave 0.  D[m][c] of MFMA i: lane (c, o) holds rows m0 + 16 bt + 4 o + reg, column kl + i: 4 consecutive k per row, 8-byte stores; rows
// past M are never stored.  Called by every wave of the workgroup
template <bool BF16, int NBT>
static __device__ __forceinline__ void dg_reduce_store(f32x4 (&acc)[NBT][4], dg_red_t* red, uint16_t* __restrict__ dx, int M, int K, int m0, int kl,
                                                       int wave, int lane) {
#pragma unroll
  for (int half = DG_WAVES / 2; half >= 1; half >>= 1) {
    if (wave >= half && wave < 2 * half) {
#pragma unroll
      for (int bt = 0; bt < NBT; ++bt)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wave - half][4 * bt + i][lane] = acc[bt][i];
    }
    __syncthreads();
    if (wave < half) {
#pragma unroll
      for (int bt = 0; bt < NBT; ++bt)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[bt][i] += red[wave][4 * bt + i][lane];
    }
    __syncthreads();
  }
  if (wave != 0) return;
  const int o = lane >> 4;
#pragma unroll
  for (int bt = 0; bt < NBT; ++bt)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int m = m0 + 16 * bt + 4 * o + rg;
      if (m < M) {
        uint16_t h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (BF16) h[i] = f32_to_bf16(acc[bt][i][rg]);
          else h[i] = __builtin_bit_cast(uint16_t, static_cast<half_t>(acc[bt][i][rg]));
        }
        const u32x2 v = {static_cast<uint32_t>(h[0]) | (static_cast<uint32_t>(h[1]) << 16), static_cast<uint32_t>(h[2]) | (static_cast<uint32_t>(h[3]) << 16)};
        *reinterpret_cast<u32x2*>(dx + static_cast<int64_t>(m) * K + kl) = v;
      }
    }
}

}  // namespace hqq
