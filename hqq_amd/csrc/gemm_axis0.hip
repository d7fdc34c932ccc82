// gemm_axis0.hip — layers quantised along axis 0 at 17..256 activation rows (hqq_hip_gemm_axis0): fused unpack -> dequantize -> GEMM, gfx950.
//
// Replaces, for short prompts and wide batches, the chain HQQLinear.forward runs for axis-0 layers (hqq/core/quantize.py:880-898): the dequantise
// kernel writes the whole fp16 weight, a GEMM reads it back (72 MB moved for a 4096 x 4096 int4 layer that holds 8 MB of packed bytes + 1 MB of meta).
//
// The decode kernel (gemv_axis0.hip) carried to several B tiles; layout, classes, rebuild and reduce are its own (axis0_common.h).  A wave owns
// (class r, a block of up to 16 * NBITS packed rows of the class, a K split of whole 64-k units, a PASS of up to 64 activation rows).  Per unit it
// fetches its 16 k of the class's (scale, zero) row ONCE, rebuilds every packed row of its block against them (rebuild_f16 / rebuild_bf16: the bits
// of hqq_hip_dequantize) and contracts each rebuilt A operand against up to FOUR 16-column B tiles of x: TB * PER * 4 f32x4 accumulators = 128
// registers at every width.  The number of live B tiles (rows of the pass / 16, rounded up) is wave-uniform and picks one of four unrolled bodies;
// rows past M in the last tile are zero in B and never stored.  The loads of unit u + 1 are issued before the arithmetic of unit u.
// Registers as compiled for gfx950 (the four bodies share one kernel, so every launch is allocated for the 4-tile body): 256 VGPRs + 129 (1 bit) ..
// 209 (8 bit) AGPRs, no scratch — the accumulators plus two units of loads do not fit the 128 registers of 4 waves / SIMD, the kernel runs ONE wave
// per SIMD and hides HBM latency with the one-unit prefetch only.  profiles/axis0_gemm_summary.md holds what that costs against the composed route.
// M > 64: further passes as more work items (pass index between the class and the split, so the passes of one (class, split) are dispatched
// together and the packed rows they re-stream — loaded non-temporal only when there is one pass — come out of L2 / MALL).
// Every output (m, n) is one chain of MFMA accumulations over k in unit order, whatever tile or pass the row lands in: a row's bits do not depend
// on the rows it travels with.
//
// Split-K: the plan g0_plan() is a function of (nbits, N, K, group_size) and the number of passes only.  Splits are added until ~2048 waves exist,
// capped so that the fp32 partial sums of one FULL pass set (splits * 64 passes rows * N * 4 bytes) do not exceed the packed weight bytes
// (N K nbits / 8): splits <= K nbits / (2048 passes).  4096 x 4096 int4, group_size 64, 64 rows: 64 classes x 1 block x 8 splits = 512 waves,
// 8 MiB of partial sums against 8 MiB of packed bytes (the decode kernel's plan would give 32 splits, 32 MiB); at 256 rows 2 splits, 8 MiB.
// Partial sums are parked in the caller's workspace past the counter head (untouched) as [split][n][m] — m fastest, so the 16 lanes of an MFMA
// column group store 64 contiguous bytes; a second launch sums the splits in split order, rounds once, adds the bias with one more rounding
// (a0_sum_splits / a0_finish) and transposes 32 x 32 tiles through LDS to y[m][n].
// The workspace query is sized with the ONE-pass split count (the largest any pass count gives), so it is linear in M.
// x is read per wave straight from L2 (no LDS staging): neighbouring work items are neighbouring classes of one (pass, split) and hit the same lines.
#include "axis0_common.h"

namespace hqq {

constexpr int G0_WAVES = 1;             // waves per workgroup: a work item fills a SIMD's register file (one wave per SIMD), so single-wave workgroups spread
                                        // a few hundred items over all CUs instead of stacking four on one
constexpr int G0_BT = 4;                // B tiles of 16 activation rows per pass
constexpr int G0_PASS_M = 16 * G0_BT;   // activation rows per pass
constexpr int G0_TARGET_WAVES = 2048;   // ~8 waves per CU before K is split further
constexpr int G0_MAX_SPLITS = 64;
constexpr int G0_MIN_M = HQQ_GEMV_MAX_M + 1;

struct G0Plan {
  int S, P, nblocks, splits, upc, units, passes;
  int64_t items;
};

static G0Plan g0_plan(int nbits, int64_t N, int64_t K, int64_t gs, int passes) {
  G0Plan p;
  const int per = 8 / nbits;
  p.S = static_cast<int>(N / gs);
  p.P = static_cast<int>(gs / per);
  const int rows_per_block = 16 * nbits;
  p.nblocks = (p.P + rows_per_block - 1) / rows_per_block;
  p.units = static_cast<int>(K / A0_KU);
  p.passes = passes;
  const int64_t base = static_cast<int64_t>(p.S) * p.nblocks * passes;
  int64_t sp = (G0_TARGET_WAVES + base - 1) / base;
  const int64_t cap = K * nbits / (8 * 4 * G0_PASS_M * static_cast<int64_t>(passes));   // partial sums <= packed bytes
  if (sp > cap) sp = cap;
  if (sp > G0_MAX_SPLITS) sp = G0_MAX_SPLITS;
  if (sp > p.units) sp = p.units;
  if (sp < 1) sp = 1;
  p.upc = static_cast<int>((p.units + sp - 1) / sp);
  p.splits = (p.units + p.upc - 1) / p.upc;
  p.items = base * p.splits;
  return p;
}

static inline int g0_passes(int64_t M) { return static_cast<int>((M + G0_PASS_M - 1) / G0_PASS_M); }

// the registers one 64-k unit arrives in: the packed rows of the block, the class's meta, NBT tiles of x
template <int TB, int NBT>
struct G0Unit {
  u32x4 w[TB], s0, s1, z0, z1, x0[NBT], x1[NBT];
};

// every slab of one packed 16-byte vector against the same meta: rebuild once, then one MFMA pair per slab and B tile
template <int NBITS, int SL, int NBT>
struct G0Slabs {
  static constexpr int PER = 8 / NBITS;
  static __device__ __forceinline__ void f16(const u32x4& w, const half2_t (&zz)[8], const half2_t (&ss)[8], const h8_t (&b0)[NBT], const h8_t (&b1)[NBT],
                                             f32x4 (&acc)[PER][NBT], uint32_t magic) {
    h8_t a0, a1;
    rebuild_f16<NBITS, SL>(w, zz, ss, a0, a1, magic);
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) acc[SL][bt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0[bt], acc[SL][bt], 0, 0, 0);
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) acc[SL][bt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1[bt], acc[SL][bt], 0, 0, 0);
    if constexpr (SL + 1 < PER) G0Slabs<NBITS, SL + 1, NBT>::f16(w, zz, ss, b0, b1, acc, magic);
  }
  static __device__ __forceinline__ void bf16(const u32x4& w, const uint32_t (&zz)[8], const uint32_t (&ss)[8], const bf16x8_t (&b0)[NBT],
                                              const bf16x8_t (&b1)[NBT], f32x4 (&acc)[PER][NBT]) {
    bf16x8_t a0, a1;
    rebuild_bf16<NBITS, SL>(w, zz, ss, a0, a1);
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) acc[SL][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0[bt], acc[SL][bt], 0, 0, 0);
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) acc[SL][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1[bt], acc[SL][bt], 0, 0, 0);
    if constexpr (SL + 1 < PER) G0Slabs<NBITS, SL + 1, NBT>::bf16(w, zz, ss, b0, b1, acc);
  }
};

// one work item with NBT live B tiles (rows m0 .. m0 + 16 NBT - 1, those past M zero and unstored), by the calling wave
template <int NBITS, bool BF16, int NBT>
__device__ __forceinline__ void g0_item(const uint16_t* __restrict__ x, const uint8_t* __restrict__ Wq, const uint16_t* __restrict__ scale,
                                        const uint16_t* __restrict__ zero, float* __restrict__ part, int M, int N, int K, int S, int P, int b, int r,
                                        int split, int m0, int upc, int units, bool once) {
  constexpr int PER = 8 / NBITS;
  constexpr int TB = NBITS;   // tiles of 16 packed rows per wave: TB * 16 * PER = 128 output rows
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, g = lane >> 4;
  const int t0 = b * 16 * TB;
  const int ntiles = (P - t0 + 15) / 16 < TB ? (P - t0 + 15) / 16 : TB;
  const uint8_t* wrow[TB];
#pragma unroll
  for (int tl = 0; tl < TB; ++tl) {
    int t = t0 + 16 * tl + col;
    t = t < P ? t : P - 1;   // rows past the class (P not a multiple of 16): a valid address, results never stored
    wrow[tl] = Wq + static_cast<int64_t>(r + static_cast<int64_t>(t) * S) * K + 16 * g;
  }
  const uint16_t* srow = scale + static_cast<int64_t>(r) * K + 16 * g;
  const uint16_t* zrow = zero + static_cast<int64_t>(r) * K + 16 * g;
  bool mv[NBT];
  const uint16_t* xrow[NBT];
#pragma unroll
  for (int bt = 0; bt < NBT; ++bt) {
    const int m = m0 + 16 * bt + col;
    mv[bt] = m < M;
    xrow[bt] = x + static_cast<int64_t>(mv[bt] ? m : 0) * K + 16 * g;   // rows past M: a valid address, zeroed below
  }
  const uint32_t magic = 0x64006400u;
  f32x4 acc[TB][PER][NBT];
#pragma unroll
  for (int tl = 0; tl < TB; ++tl)
#pragma unroll
    for (int j = 0; j < PER; ++j)
#pragma unroll
      for (int bt = 0; bt < NBT; ++bt) acc[tl][j][bt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int u0 = split * upc;
  const int u1 = u0 + upc < units ? u0 + upc : units;
  auto fetch = [&](int u, G0Unit<TB, NBT>& f) {
    const int k = u * A0_KU;
#pragma unroll
    for (int tl = 0; tl < TB; ++tl)   // one pass: every packed byte is read once, non-temporal; several: the later passes should find it in L2 / MALL
      f.w[tl] = tl < ntiles ? (once ? ld16_nt(wrow[tl] + k) : ld16(wrow[tl] + k)) : u32x4{0u, 0u, 0u, 0u};
    f.s0 = ld16(srow + k); f.s1 = ld16(srow + k + 8);
    f.z0 = ld16(zrow + k); f.z1 = ld16(zrow + k + 8);
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) { f.x0[bt] = ld16(xrow[bt] + k); f.x1[bt] = ld16(xrow[bt] + k + 8); }
  };
  G0Unit<TB, NBT> nxt;
  fetch(u0, nxt);
  for (int u = u0; u < u1; ++u) {
    const G0Unit<TB, NBT> cur = nxt;
    fetch(u + 1 < u1 ? u + 1 : u, nxt);   // (the last unit is fetched twice: no branch round the loads)
    const u32x4 s0 = permute_x8(cur.s0), s1 = permute_x8(cur.s1), z0 = permute_x8(cur.z0), z1 = permute_x8(cur.z1);
    u32x4 x0[NBT], x1[NBT];
#pragma unroll
    for (int bt = 0; bt < NBT; ++bt) {
      x0[bt] = cur.x0[bt]; x1[bt] = cur.x1[bt];
      if (!mv[bt]) { x0[bt] = u32x4{0u, 0u, 0u, 0u}; x1[bt] = x0[bt]; }
      x0[bt] = permute_x8(x0[bt]);
      x1[bt] = permute_x8(x1[bt]);
    }
    if constexpr (!BF16) {
      half2_t zz[8], ss[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { zz[i] = as_h2(z0[i]); zz[4 + i] = as_h2(z1[i]); ss[i] = as_h2(s0[i]); ss[4 + i] = as_h2(s1[i]); }
      h8_t b0[NBT], b1[NBT];
#pragma unroll
      for (int bt = 0; bt < NBT; ++bt) { b0[bt] = __builtin_bit_cast(h8_t, x0[bt]); b1[bt] = __builtin_bit_cast(h8_t, x1[bt]); }
#pragma unroll
      for (int tl = 0; tl < TB; ++tl)
        if (tl < ntiles) G0Slabs<NBITS, 0, NBT>::f16(cur.w[tl], zz, ss, b0, b1, acc[tl], magic);
    } else {
      uint32_t zz[8], ss[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { zz[i] = z0[i]; zz[4 + i] = z1[i]; ss[i] = s0[i]; ss[4 + i] = s1[i]; }
      bf16x8_t b0[NBT], b1[NBT];
#pragma unroll
      for (int bt = 0; bt < NBT; ++bt) { b0[bt] = __builtin_bit_cast(bf16x8_t, x0[bt]); b1[bt] = __builtin_bit_cast(bf16x8_t, x1[bt]); }
#pragma unroll
      for (int tl = 0; tl < TB; ++tl)
        if (tl < ntiles) G0Slabs<NBITS, 0, NBT>::bf16(cur.w[tl], zz, ss, b0, b1, acc[tl]);
    }
  }
  // D[i][m]: lane l holds row m0 + 16 bt + (l & 15) and packed rows t0 + 16 tl + 4 (l >> 4) + reg; output row n = r + (t + slab P) S.
  // Parked as part[split][n][m]: the 16 lanes of a group write 16 consecutive floats
  float* out = part + static_cast<int64_t>(split) * M * N;
#pragma unroll
  for (int tl = 0; tl < TB; ++tl) {
    if (tl >= ntiles) break;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int t = t0 + 16 * tl + 4 * g + rg;
      if (t < P) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          float* o = out + (r + static_cast<int64_t>(t + j * P) * S) * M + m0 + col;
#pragma unroll
          for (int bt = 0; bt < NBT; ++bt)
            if (mv[bt]) o[16 * bt] = acc[tl][j][bt][rg];
        }
      }
    }
  }
}

template <int NBITS, bool BF16>
__global__ __launch_bounds__(G0_WAVES * 64) void gemm_axis0_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ Wq,
                                                                  const uint16_t* __restrict__ scale, const uint16_t* __restrict__ zero,
                                                                  float* __restrict__ part, int M, int N, int K, int S, int P, int nblocks, int upc,
                                                                  int units, int passes, int64_t items) {
  // (the wave index through readfirstlane: everything that picks the item, and the number of live B tiles, is then scalar)
  const int64_t item = static_cast<int64_t>(blockIdx.x) * G0_WAVES + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (item >= items) return;
  const int b = static_cast<int>(item % nblocks);
  int64_t rest = item / nblocks;
  const int r = static_cast<int>(rest % S);
  rest /= S;
  const int pass = static_cast<int>(rest % passes);
  const int split = static_cast<int>(rest / passes);
  const int m0 = pass * G0_PASS_M;
  const int rows = M - m0 < G0_PASS_M ? M - m0 : G0_PASS_M;
  switch ((rows + 15) / 16) {
    case 1: g0_item<NBITS, BF16, 1>(x, Wq, scale, zero, part, M, N, K, S, P, b, r, split, m0, upc, units, passes == 1); break;
    case 2: g0_item<NBITS, BF16, 2>(x, Wq, scale, zero, part, M, N, K, S, P, b, r, split, m0, upc, units, passes == 1); break;
    case 3: g0_item<NBITS, BF16, 3>(x, Wq, scale, zero, part, M, N, K, S, P, b, r, split, m0, upc, units, passes == 1); break;
    default: g0_item<NBITS, BF16, 4>(x, Wq, scale, zero, part, M, N, K, S, P, b, r, split, m0, upc, units, passes == 1); break;
  }
}

// y[m, n] = round(sum over splits of part[split][n][m], in split order) (+ bias, one more rounding): a 32 x 32 tile per workgroup, read along m,
// transposed through LDS, written along n
constexpr int G0_RT = 32;
template <bool BF16>
__global__ __launch_bounds__(256) void gemm_axis0_reduce_kernel(const float* __restrict__ part, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
                                                                int M, int N, int splits) {
  __shared__ uint16_t tile[G0_RT][G0_RT + 2];
  const int n0 = blockIdx.x * G0_RT, m0 = blockIdx.y * G0_RT;
  const int lo = threadIdx.x & (G0_RT - 1), hi = threadIdx.x >> 5;   // 256 threads: 32 x 8
  const int64_t MN = static_cast<int64_t>(M) * N;
#pragma unroll
  for (int q = 0; q < G0_RT / 8; ++q) {
    const int n = n0 + hi + 8 * q, m = m0 + lo;
    if (n < N && m < M) tile[hi + 8 * q][lo] = a0_finish<BF16>(a0_sum_splits(part, MN, static_cast<int64_t>(n) * M + m, splits), bias, n);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < G0_RT / 8; ++q) {
    const int n = n0 + lo, m = m0 + hi + 8 * q;
    if (n < N && m < M) y[static_cast<int64_t>(m) * N + n] = tile[lo][hi + 8 * q];
  }
}

// a0_validate's checks for 17..256 rows; the partial-sum area is checked with the most splits THIS plan gives (one pass), not with the cap
static int g0_validate(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts) {
  if (const int rc = a0_validate_rows("hqq_hip_gemm_axis0", G0_MIN_M, HQQ_GEMM_AXIS0_MAX_M, 1, nbits, M, N, K, group_size, dtype, opts)) return rc;
  if (M * N * g0_plan(nbits, N, K, group_size, 1).splits > INT32_MAX) { set_error("hqq_hip_gemm_axis0: size overflow"); return HQQ_ERR_SHAPE; }
  return 0;
}

}  // namespace hqq

using namespace hqq;

extern "C" size_t hqq_hip_gemm_axis0_workspace_bytes(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype) {
  if (g0_validate(nbits, M, N, K, group_size, dtype, 0)) return 0;
  const G0Plan one = g0_plan(nbits, N, K, group_size, 1);   // the most splits any pass count gives: the size is linear in M
  return WS_COUNTER_BYTES + ((static_cast<size_t>(one.splits) * M * N * sizeof(float) + 15) & ~static_cast<size_t>(15));
}

extern "C" int hqq_hip_gemm_axis0(int nbits, const void* x, const void* Wq, const void* scale, const void* zero, const void* bias, void* y,
                                  int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  clear_stale_error();
  if (const int rc = g0_validate(nbits, M, N, K, group_size, dtype, opts)) return rc;
  if (!x || !Wq || !scale || !zero || !y) { set_error("hqq_hip_gemm_axis0: null argument"); return HQQ_ERR_SHAPE; }
  if (!aligned16(x) || !aligned16(Wq) || !aligned16(scale) || !aligned16(zero)) { set_error("hqq_hip_gemm_axis0: pointers must be 16-byte aligned"); return HQQ_ERR_ALIGN; }
  const size_t need = hqq_hip_gemm_axis0_workspace_bytes(nbits, M, N, K, group_size, dtype);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("hqq_hip_gemm_axis0: needs %zu bytes of 16-byte aligned workspace (got %zu)", need, workspace_bytes);
    return HQQ_ERR_WORKSPACE;
  }
  const G0Plan p = g0_plan(nbits, N, K, group_size, g0_passes(M));
  if (p.splits > g0_plan(nbits, N, K, group_size, 1).splits) { set_error("hqq_hip_gemm_axis0: plan exceeds the workspace"); return HQQ_ERR_WORKSPACE; }   // (never: splits do not grow with the passes)
  float* part = reinterpret_cast<float*>(static_cast<uint8_t*>(workspace) + WS_COUNTER_BYTES);
  hipStream_t st = as_stream(stream);
  const int grid = static_cast<int>((p.items + G0_WAVES - 1) / G0_WAVES);
  const auto* xs = static_cast<const uint16_t*>(x);
  const auto* ws = static_cast<const uint8_t*>(Wq);
  const auto* ss = static_cast<const uint16_t*>(scale);
  const auto* zs = static_cast<const uint16_t*>(zero);
  const int Mi = static_cast<int>(M), Ni = static_cast<int>(N), Ki = static_cast<int>(K);
#define HQQ_G0_LAUNCH(NB, BF)                                                                                                            \
  hipLaunchKernelGGL((gemm_axis0_kernel<NB, BF>), dim3(grid), dim3(G0_WAVES * 64), 0, st, xs, ws, ss, zs, part, Mi, Ni, Ki, p.S, p.P, \
                     p.nblocks, p.upc, p.units, p.passes, p.items)
  if (dtype == HQQ_BF16) {
    if (nbits == 4) HQQ_G0_LAUNCH(4, true); else HQQ_G0_LAUNCH(2, true);
  } else {
    switch (nbits) {
      case 8: HQQ_G0_LAUNCH(8, false); break;
      case 4: HQQ_G0_LAUNCH(4, false); break;
      case 2: HQQ_G0_LAUNCH(2, false); break;
      default: HQQ_G0_LAUNCH(1, false); break;
    }
  }
#undef HQQ_G0_LAUNCH
  if (const int rc = check_launch("hqq_hip_gemm_axis0")) return rc;
  const dim3 rgrid(static_cast<unsigned>((N + G0_RT - 1) / G0_RT), static_cast<unsigned>((M + G0_RT - 1) / G0_RT));
  if (dtype == HQQ_BF16)
    hipLaunchKernelGGL(gemm_axis0_reduce_kernel<true>, rgrid, dim3(256), 0, st, part, static_cast<const uint16_t*>(bias), static_cast<uint16_t*>(y), Mi, Ni, p.splits);
  else
    hipLaunchKernelGGL(gemm_axis0_reduce_kernel<false>, rgrid, dim3(256), 0, st, part, static_cast<const uint16_t*>(bias), static_cast<uint16_t*>(y), Mi, Ni, p.splits);
  return check_launch("hqq_hip_gemm_axis0");
}
