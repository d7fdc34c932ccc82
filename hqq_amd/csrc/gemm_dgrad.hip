// gemm_dgrad.hip — the backward-through-weights product of an axis-1 layer (hqq_hip_gemm_dgrad): dx[M,K] = g[M,N] . dequantize(Wq)[N,K], fused
// unpack -> dequantize -> GEMM, gfx950.
//
// Replaces, for the gradient with respect to a layer's input, the chain _MatmulNoCache.backward runs (hqq/core/quantize.py:477-479, 534-553): the
// dequantise kernel writes the whole fp16 / bf16 weight (2 N K bytes), torch.matmul reads it back.
//
// Layout.  The container is [N / per, K] bytes, contiguous along k; byte [p, k] holds the levels of output rows p + slab * N / per in its bit fields.  The
// contraction runs along n, the strided direction.  No LDS transpose: a lane (c = lane & 15, o = lane >> 4) loads ONE dword (4 k: k0 + 4 c .. + 3) from each
// of the EIGHT packed rows p0 + 8 o .. + 7 of a 32-row step and transposes the 4 x 4 byte blocks in registers (8 v_perm_b32 per 32 bytes, shared by every
// bit field), so that dword i holds byte i of four rows.  rebuild_f16 / rebuild_bf16 (axis0_common.h: the bits of hqq_hip_dequantize, per-element meta)
// turn dword i of slab s into the weights of output column k0 + 4 c + i for four rows of the contraction, in the order (r0, r2, r1, r3); two such quads are
// the B operand of one 16x16x32 MFMA.  The A operand is g[m, slab * N / per + p0 + 8 o .. + 7], one 16-byte load, its halves put in the same order
// (permute_x8).  MFMA i (i = 0..3) of a slab therefore accumulates D[m][c] for output column k0 + 4 c + i: contraction order and column numbering of an
// MFMA are both free as long as the two operands agree.  A lane ends up with 4 consecutive k of 4 rows per 16-row tile: 8-byte stores.
// (scale, zero) of a lane's four k are ONE group per row (16 | group_size): element (slab * N / per + p) * (K / group_size) + (k0 + 4 c) / group_size.
//
// Work.  A workgroup of 8 waves owns the output tile (64 rows of g, 64 k) and walks ALL of N: wave w takes the 32-row steps w, w + 8, ...; the eight partial
// tiles are added through LDS in a fixed tree ((0+4)+(2+6)) + ((1+5)+(3+7)), wave 0 rounds once and stores.  No atomics, no workspace; an output's bits
// depend on (N, nbits) and its own row of g only — not on M, nor on the rows it travels with.  The number of live 16-row tiles (1..4) is uniform over the
// workgroup and picks one of four unrolled bodies; rows past M are zero in A and never stored.  A ragged last step (N / per any multiple of 8: 8, 16 or 24 rows left) has the
// lane groups past the end read a valid address and contribute zeros through A.
// Every k tile streams its own 64-byte column of the container and one meta element per row and slab; every further 64 rows of g stream them again (from L2 /
// MALL), so the rebuild is repeated M / 64 times: a library GEMM on the dequantised weight overtakes this kernel as M grows (profiles/dgrad_summary.md).
#include "dgrad_common.h"

namespace hqq {

// the meta of four rows as the pairs rebuild_* wants them: (row 0, row 2) against bytes (0, 2) of a transposed dword, (row 1, row 3) against bytes (1, 3)
static __device__ __forceinline__ void dg_pair(const uint16_t (&v)[4], uint32_t& p02, uint32_t& p13) {
  p02 = static_cast<uint32_t>(v[0]) | (static_cast<uint32_t>(v[2]) << 16);
  p13 = static_cast<uint32_t>(v[1]) | (static_cast<uint32_t>(v[3]) << 16);
}

// every slab of one step: the slab's meta (one group per row: the same pair at each of the lane's four k), then dg_slab (dgrad_common.h)
template <int NBITS, bool BF16, int SL, int NBT>
struct DgSlabs {
  static constexpr int PER = 8 / NBITS;
  static __device__ __forceinline__ void run(const u32x4& tlo, const u32x4& thi, const uint16_t (&z)[PER][8], const uint16_t (&s)[PER][8],
                                             const u32x4 (&ga)[PER][NBT], f32x4 (&acc)[NBT][4], uint32_t magic) {
    uint32_t zp[2][2], sp[2][2];   // [rows 0..3 / 4..7][(0,2) / (1,3)]
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint16_t zq[4] = {z[SL][4 * h], z[SL][4 * h + 1], z[SL][4 * h + 2], z[SL][4 * h + 3]};
      const uint16_t sq[4] = {s[SL][4 * h], s[SL][4 * h + 1], s[SL][4 * h + 2], s[SL][4 * h + 3]};
      dg_pair(zq, zp[h][0], zp[h][1]);
      dg_pair(sq, sp[h][0], sp[h][1]);
    }
    uint32_t zz[2][8], ss[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 8; ++i) { zz[h][i] = zp[h][i & 1]; ss[h][i] = sp[h][i & 1]; }
    dg_slab<NBITS, BF16, SL, NBT>(tlo, thi, zz, ss, ga, acc, magic);
    if constexpr (SL + 1 < PER) DgSlabs<NBITS, BF16, SL + 1, NBT>::run(tlo, thi, z, s, ga, acc, magic);
  }
};

// one output tile (rows m0 .. m0 + 16 NBT - 1, columns k0 .. k0 + 63) by the calling workgroup
template <int NBITS, bool BF16, int NBT>
__device__ __forceinline__ void dg_tile(const uint16_t* __restrict__ g, const uint8_t* __restrict__ Wq, const uint16_t* __restrict__ scale,
                                        const uint16_t* __restrict__ zero, uint16_t* __restrict__ dx, int M, int N, int K, int Np, int G, int gs, int k0,
                                        int m0, dg_red_t* red) {
  constexpr int PER = 8 / NBITS;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int c = lane & 15, o = lane >> 4;
  const int kl = k0 + 4 * c;
  const int64_t kg = kl / gs;
  const int steps = (Np + DG_STEP - 1) / DG_STEP;
  bool mv[NBT];
  const uint16_t* grow[NBT];
#pragma unroll
  for (int bt = 0; bt < NBT; ++bt) {
    const int m = m0 + 16 * bt + c;
    mv[bt] = m < M;
    grow[bt] = g + static_cast<int64_t>(mv[bt] ? m : 0) * N;   // rows past M: a valid address, zeroed below
  }
  const uint32_t magic = 0x64006400u;
  f32x4 acc[NBT][4];
#pragma unroll
  for (int bt = 0; bt < NBT; ++bt)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[bt][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int st = wave; st < steps; st += DG_WAVES) {
    const int p = st * DG_STEP + 8 * o;
    const bool live = p < Np;          // (Np % 8 == 0: a lane's eight rows are all inside or all outside)
    const int pc = live ? p : 0;       // outside: a valid address, its products zeroed through A
    uint32_t w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r] = *reinterpret_cast<const uint32_t*>(Wq + static_cast<int64_t>(pc + r) * K + kl);
    uint16_t z[PER][8], s[PER][8];
#pragma unroll
    for (int j = 0; j < PER; ++j)
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int64_t mi = (static_cast<int64_t>(j) * Np + pc + r) * G + kg;
        z[j][r] = zero[mi];
        s[j][r] = scale[mi];
      }
    u32x4 ga[PER][NBT];
    dg_load_g<PER, NBT>(grow, mv, Np, pc, live, ga);
    const u32x4 tlo = dg_transpose(w[0], w[1], w[2], w[3]);
    const u32x4 thi = dg_transpose(w[4], w[5], w[6], w[7]);
    DgSlabs<NBITS, BF16, 0, NBT>::run(tlo, thi, z, s, ga, acc, magic);
  }

  dg_reduce_store<BF16, NBT>(acc, red, dx, M, K, m0, kl, wave, lane);
}

template <int NBITS, bool BF16>
__global__ __launch_bounds__(DG_WAVES * 64) void gemm_dgrad_kernel(const uint16_t* __restrict__ g, const uint8_t* __restrict__ Wq,
                                                                  const uint16_t* __restrict__ scale, const uint16_t* __restrict__ zero,
                                                                  uint16_t* __restrict__ dx, int M, int N, int K, int Np, int G, int gs, int ktiles) {
  __shared__ dg_red_t red[DG_WAVES / 2];   // 64 KiB: the partial tiles of four waves
  // k tiles fastest: the workgroups in flight together share their rows of g and neighbouring 64-byte columns of the container
  const int k0 = static_cast<int>(blockIdx.x % ktiles) * DG_KT;
  const int m0 = static_cast<int>(blockIdx.x / ktiles) * DG_PASS_M;
  const int rows = M - m0 < DG_PASS_M ? M - m0 : DG_PASS_M;
  switch ((rows + 15) / 16) {
    case 1: dg_tile<NBITS, BF16, 1>(g, Wq, scale, zero, dx, M, N, K, Np, G, gs, k0, m0, red); break;
    case 2: dg_tile<NBITS, BF16, 2>(g, Wq, scale, zero, dx, M, N, K, Np, G, gs, k0, m0, red); break;
    case 3: dg_tile<NBITS, BF16, 3>(g, Wq, scale, zero, dx, M, N, K, Np, G, gs, k0, m0, red); break;
    default: dg_tile<NBITS, BF16, 4>(g, Wq, scale, zero, dx, M, N, K, Np, G, gs, k0, m0, red); break;
  }
}

// what the kernel covers, checked before anything is launched: 0, or an HQQ_ERR_* with the message set
static int dg_validate(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype) {
  const char* who = "hqq_hip_gemm_dgrad";
  if (nbits != 8 && nbits != 4 && nbits != 3 && nbits != 2 && nbits != 1) { set_error("%s: nbits=%d", who, nbits); return HQQ_ERR_NBITS; }
  if (nbits == 3 || nbits == 1) { set_error("%s: %d-bit containers are not covered (8 / 4 / 2)", who, nbits); return HQQ_ERR_UNSUPPORTED; }
  if (dtype == HQQ_F32) { set_error("%s: fp32 is not covered (fp16 / bf16)", who); return HQQ_ERR_UNSUPPORTED; }
  if (dtype != HQQ_F16 && dtype != HQQ_BF16) { set_error("%s: dtype %d", who, dtype); return HQQ_ERR_DTYPE; }
  if (M < 1) { set_error("%s: M=%lld is not covered (at least 1 row)", who, (long long)M); return HQQ_ERR_UNSUPPORTED; }
  if (N < 1 || K < 1 || group_size < 1) { set_error("%s: bad N/K/group_size", who); return HQQ_ERR_SHAPE; }
  const int per = 8 / nbits;
  if (group_size % 16 || K % group_size || K % DG_KT || N % (8 * per)) {
    set_error("%s: not covered: needs group_size %% 16 == 0, K %% group_size == 0, K %% %d == 0, N %% %d == 0 (N=%lld K=%lld gs=%lld)", who, DG_KT,
              8 * per, (long long)N, (long long)K, (long long)group_size);
    return HQQ_ERR_UNSUPPORTED;
  }
  // (N / per) * K packed bytes, N K / gs meta elements, M N and M K activations, the grid: everything the kernel indexes stays in range
  const int64_t tiles = (K / DG_KT) * ((M + DG_PASS_M - 1) / DG_PASS_M);
  if (N > INT32_MAX || K > INT32_MAX || M > INT32_MAX || (N / per) * K > static_cast<int64_t>(UINT32_MAX) || N * (K / group_size) > INT32_MAX ||
      tiles > INT32_MAX) {
    set_error("%s: size overflow", who);
    return HQQ_ERR_SHAPE;
  }
  return 0;
}

}  // namespace hqq

using namespace hqq;

extern "C" int hqq_hip_gemm_dgrad_covers(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype) {
  return dg_validate(nbits, M, N, K, group_size, dtype) == 0 ? 1 : 0;
}

extern "C" int hqq_hip_gemm_dgrad(int nbits, const void* g, const void* Wq, const void* scale, const void* zero, void* dx, int64_t M, int64_t N,
                                  int64_t K, int64_t group_size, int dtype, void* stream) {
  if (const int rc = dg_validate(nbits, M, N, K, group_size, dtype)) return rc;
  clear_stale_error();
  if (!g || !Wq || !scale || !zero || !dx) { set_error("hqq_hip_gemm_dgrad: null argument"); return HQQ_ERR_SHAPE; }
  if (!aligned16(g) || !aligned16(Wq) || !aligned16(dx)) { set_error("hqq_hip_gemm_dgrad: g / Wq / dx must be 16-byte aligned"); return HQQ_ERR_ALIGN; }
  const int per = 8 / nbits;
  const int ktiles = static_cast<int>(K / DG_KT);
  const int grid = static_cast<int>(ktiles * ((M + DG_PASS_M - 1) / DG_PASS_M));
  const int Mi = static_cast<int>(M), Ni = static_cast<int>(N), Ki = static_cast<int>(K), Np = static_cast<int>(N / per);
  const int G = static_cast<int>(K / group_size), gs = static_cast<int>(group_size);
  hipStream_t st = as_stream(stream);
  const auto* gp = static_cast<const uint16_t*>(g);
  const auto* ws = static_cast<const uint8_t*>(Wq);
  const auto* ss = static_cast<const uint16_t*>(scale);
  const auto* zs = static_cast<const uint16_t*>(zero);
  auto* out = static_cast<uint16_t*>(dx);
#define HQQ_DG_LAUNCH(NB, BF) \
  hipLaunchKernelGGL((gemm_dgrad_kernel<NB, BF>), dim3(grid), dim3(DG_WAVES * 64), 0, st, gp, ws, ss, zs, out, Mi, Ni, Ki, Np, G, gs, ktiles)
  if (dtype == HQQ_BF16) {
    switch (nbits) {
      case 8: HQQ_DG_LAUNCH(8, true); break;
      case 4: HQQ_DG_LAUNCH(4, true); break;
      default: HQQ_DG_LAUNCH(2, true); break;
    }
  } else {
    switch (nbits) {
      case 8: HQQ_DG_LAUNCH(8, false); break;
      case 4: HQQ_DG_LAUNCH(4, false); break;
      default: HQQ_DG_LAUNCH(2, false); break;
    }
  }
#undef HQQ_DG_LAUNCH
  return check_launch("hqq_hip_gemm_dgrad");
}
