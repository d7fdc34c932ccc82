// gemm_dgrad_axis0.hip — the backward-through-weights product of an AXIS-0 layer (hqq_hip_gemm_dgrad_axis0): dx[M,K] = g[M,N] . dequantize(Wq, axis=0)[N,K],
// fused unpack -> dequantize -> GEMM, gfx950.
//
// Replaces, for the gradient with respect to the input of a layer quantised along axis 0 (the reference's only training configuration: ATEN_BACKPROP,
// hqq/core/quantize.py:930), dequantise (2 N K bytes written) + torch.matmul (read back).
//
// Everything but the constants is gemm_dgrad.hip's (dgrad_common.h): the container is the same [N / per, K] byte array, a lane (c = lane & 15,
// o = lane >> 4) takes 8 packed rows x 4 k of a 32-row step, transposes the bytes in registers, rebuilds each slab with rebuild_f16 / rebuild_bf16 and feeds
// 4 MFMAs per slab and 16-row tile of g; 8 waves deal out the N walk and are added in the fixed tree ((0+4)+(2+6)) + ((1+5)+(3+7)).  The same contract
// follows: the weights are the bits of hqq_hip_dequantize(axis = 0), fp32 accumulation, one rounding, no atomics, no workspace, an output row's bits
// depend on (N, nbits) and its own row of g only, rows past M are never stored.
//
// Meta.  With Nr = N / group_size, element (n, k) uses constant (n % Nr) * K + k: scale and zero are [Nr, K], contiguous along k.  N / per is a multiple
// of Nr, so EVERY slab of a packed byte [p, k] uses the constant (p % Nr, k): a lane loads 8 bytes of zero and 8 of scale (its four k) per packed row, turns
// them once per step into the (row b, row b + 2) pairs per k that rebuild_* takes, and every slab and every tile of g reuses them.  Nr is arbitrary (172
// for 11008 / 64, 3, 1): the meta row of the lane's first packed row is p % Nr (one division per step) and each further row steps it by one with a wrap
// to 0, so the eight rows may wrap once, several times (Nr < 8) or always (Nr = 1).
//
// Meta traffic.  A k tile's Nr x 64 meta pairs are read group_size / per times each (int4, gs 64: 4 B of meta per packed byte, against 0.0625 B on axis 1),
// so where the walk takes them from matters.  Two ways were built and measured against each other (profiles/dgrad_axis0_summary.md): plain 8-byte global
// loads served by L1 / L2, and the tile's meta slab — zero[Nr][64] and scale[Nr][64], Nr x 256 B — staged ONCE per workgroup in LDS, under the reduce
// buffer (which is not live until the walk is over).  THE STAGED FORM STAYED: int4, gs 64, fp16 on an MI355X it is 1.20x / 1.32x / 1.22x / 1.25x / 1.26x
// faster at 1 / 16 / 64 / 256 / 1024 rows on 4096 x 4096 (14.9 against 17.9 us at one row) and 1.16x to 1.39x on the other two shapes.  Staged rows are
// 144 bytes apart, so that the 128-byte reads of two lane groups whose meta rows are 8 apart fall on different halves of the banks.  It holds while both
// slabs fit the 64 KiB buffer, Nr <= 227; a layer with more meta rows (N / group_size > 227: e.g. N = 4096 at group_size 16) takes the global-load form —
// same arithmetic, same bits.
#include "dgrad_common.h"

namespace hqq {

constexpr int DG0_LDS_ROW = DG_KT + 8;                            // staged rows are 144 bytes apart: the four lane groups' 128-byte reads fall on both bank halves
constexpr int DG0_LDS_MAX_NR = 65536 / (2 * 2 * DG0_LDS_ROW);    // zero + scale slabs inside the 64 KiB reduce buffer

// k d (0..3) of the lane's rows (b, b + 2) out of their 8-byte loads: the pair rebuild_* takes for dword d, bytes (b, b + 2)
static __device__ __forceinline__ uint32_t dg0_pair(const u32x2& ra, const u32x2& rb, int d) {
  return __builtin_amdgcn_perm(rb[d >> 1], ra[d >> 1], (d & 1) ? 0x07060302u : 0x05040100u);
}

template <int NBITS, bool BF16, int SL, int NBT>
struct Dg0Slabs {
  static constexpr int PER = 8 / NBITS;
  static __device__ __forceinline__ void run(const u32x4& tlo, const u32x4& thi, const uint32_t (&zp)[2][8], const uint32_t (&sp)[2][8],
                                             const u32x4 (&ga)[PER][NBT], f32x4 (&acc)[NBT][4], uint32_t magic) {
    dg_slab<NBITS, BF16, SL, NBT>(tlo, thi, zp, sp, ga, acc, magic);
    if constexpr (SL + 1 < PER) Dg0Slabs<NBITS, BF16, SL + 1, NBT>::run(tlo, thi, zp, sp, ga, acc, magic);
  }
};

// one output tile (rows m0 .. m0 + 16 NBT - 1, columns k0 .. k0 + 63) by the calling workgroup
template <int NBITS, bool BF16, int NBT, bool STAGE>
__device__ __forceinline__ void dg0_tile(const uint16_t* __restrict__ g, const uint8_t* __restrict__ Wq, const uint16_t* __restrict__ scale,
                                         const uint16_t* __restrict__ zero, uint16_t* __restrict__ dx, int M, int N, int K, int Np, int Nr, int k0,
                                         int m0, dg_red_t* red) {
  constexpr int PER = 8 / NBITS;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int c = lane & 15, o = lane >> 4;
  const int kl = k0 + 4 * c;
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

  // STAGE: zero[Nr][k0 .. k0 + 63] then scale[...] at the bottom of the reduce buffer, rows DG0_LDS_ROW elements apart; otherwise global loads per step
  uint16_t* const lz = reinterpret_cast<uint16_t*>(red);
  uint16_t* const ls = lz + Nr * DG0_LDS_ROW;
  if constexpr (STAGE) {
    for (int i = threadIdx.x; i < Nr * 16; i += DG_WAVES * 64) {   // 16 8-byte pieces per row
      const int row = i >> 4, pc4 = 4 * (i & 15);
      *reinterpret_cast<u32x2*>(lz + row * DG0_LDS_ROW + pc4) = *reinterpret_cast<const u32x2*>(zero + static_cast<int64_t>(row) * K + k0 + pc4);
      *reinterpret_cast<u32x2*>(ls + row * DG0_LDS_ROW + pc4) = *reinterpret_cast<const u32x2*>(scale + static_cast<int64_t>(row) * K + k0 + pc4);
    }
    __syncthreads();
  }

  for (int st = wave; st < steps; st += DG_WAVES) {
    const int p = st * DG_STEP + 8 * o;
    const bool live = p < Np;          // (Np % 8 == 0: a lane's eight rows are all inside or all outside)
    const int pc = live ? p : 0;       // outside: a valid address, its products zeroed through A
    uint32_t w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r] = *reinterpret_cast<const uint32_t*>(Wq + static_cast<int64_t>(pc + r) * K + kl);
    u32x2 zv[8], sv[8];
    int mr = pc % Nr;                  // the meta row of packed row pc + r is (pc + r) % Nr: stepped, wrapping as often as Nr asks
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if constexpr (STAGE) {
        zv[r] = *reinterpret_cast<const u32x2*>(lz + mr * DG0_LDS_ROW + 4 * c);
        sv[r] = *reinterpret_cast<const u32x2*>(ls + mr * DG0_LDS_ROW + 4 * c);
      } else {
        const int64_t mi = static_cast<int64_t>(mr) * K + kl;
        zv[r] = *reinterpret_cast<const u32x2*>(zero + mi);
        sv[r] = *reinterpret_cast<const u32x2*>(scale + mi);
      }
      mr = mr + 1 == Nr ? 0 : mr + 1;
    }
    u32x4 ga[PER][NBT];
    dg_load_g<PER, NBT>(grow, mv, Np, pc, live, ga);
    uint32_t zp[2][8], sp[2][8];       // [rows 0..3 / 4..7][2 d + b]: k d of rows (4 h + b, 4 h + b + 2)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int d = i >> 1, b = i & 1;
        zp[h][i] = dg0_pair(zv[4 * h + b], zv[4 * h + b + 2], d);
        sp[h][i] = dg0_pair(sv[4 * h + b], sv[4 * h + b + 2], d);
      }
    const u32x4 tlo = dg_transpose(w[0], w[1], w[2], w[3]);
    const u32x4 thi = dg_transpose(w[4], w[5], w[6], w[7]);
    Dg0Slabs<NBITS, BF16, 0, NBT>::run(tlo, thi, zp, sp, ga, acc, magic);
  }

  if constexpr (STAGE) __syncthreads();   // the reduce buffer lies over the staged meta: every wave has finished reading it
  dg_reduce_store<BF16, NBT>(acc, red, dx, M, K, m0, kl, wave, lane);
}

template <int NBITS, bool BF16, bool STAGE>
__global__ __launch_bounds__(DG_WAVES * 64) void gemm_dgrad_axis0_kernel(const uint16_t* __restrict__ g, const uint8_t* __restrict__ Wq,
                                                                        const uint16_t* __restrict__ scale, const uint16_t* __restrict__ zero,
                                                                        uint16_t* __restrict__ dx, int M, int N, int K, int Np, int Nr, int ktiles) {
  __shared__ dg_red_t red[DG_WAVES / 2];   // 64 KiB: the partial tiles of four waves
  // k tiles fastest: the workgroups in flight together share their rows of g and neighbouring 64-byte columns of the container
  const int k0 = static_cast<int>(blockIdx.x % ktiles) * DG_KT;
  const int m0 = static_cast<int>(blockIdx.x / ktiles) * DG_PASS_M;
  const int rows = M - m0 < DG_PASS_M ? M - m0 : DG_PASS_M;
  switch ((rows + 15) / 16) {
    case 1: dg0_tile<NBITS, BF16, 1, STAGE>(g, Wq, scale, zero, dx, M, N, K, Np, Nr, k0, m0, red); break;
    case 2: dg0_tile<NBITS, BF16, 2, STAGE>(g, Wq, scale, zero, dx, M, N, K, Np, Nr, k0, m0, red); break;
    case 3: dg0_tile<NBITS, BF16, 3, STAGE>(g, Wq, scale, zero, dx, M, N, K, Np, Nr, k0, m0, red); break;
    default: dg0_tile<NBITS, BF16, 4, STAGE>(g, Wq, scale, zero, dx, M, N, K, Np, Nr, k0, m0, red); break;
  }
}

// what the kernel covers, checked before anything is launched: 0, or an HQQ_ERR_* with the message set
static int dg0_validate(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype) {
  const char* who = "hqq_hip_gemm_dgrad_axis0";
  if (nbits != 8 && nbits != 4 && nbits != 3 && nbits != 2 && nbits != 1) { set_error("%s: nbits=%d", who, nbits); return HQQ_ERR_NBITS; }
  if (nbits == 3 || nbits == 1) { set_error("%s: %d-bit containers are not covered (8 / 4 / 2)", who, nbits); return HQQ_ERR_UNSUPPORTED; }
  if (dtype == HQQ_F32) { set_error("%s: fp32 is not covered (fp16 / bf16)", who); return HQQ_ERR_UNSUPPORTED; }
  if (dtype != HQQ_F16 && dtype != HQQ_BF16) { set_error("%s: dtype %d", who, dtype); return HQQ_ERR_DTYPE; }
  if (M < 1) { set_error("%s: M=%lld is not covered (at least 1 row)", who, (long long)M); return HQQ_ERR_UNSUPPORTED; }
  if (N < 1 || K < 1 || group_size < 1) { set_error("%s: bad N/K/group_size", who); return HQQ_ERR_SHAPE; }
  const int per = 8 / nbits;
  if (group_size % 16 || N % group_size || K % DG_KT || N % (8 * per)) {
    set_error("%s: not covered: needs group_size %% 16 == 0, N %% group_size == 0, K %% %d == 0, N %% %d == 0 (N=%lld K=%lld gs=%lld)", who, DG_KT,
              8 * per, (long long)N, (long long)K, (long long)group_size);
    return HQQ_ERR_UNSUPPORTED;
  }
  // (N / per) * K packed bytes, (N / gs) * K meta elements, M N and M K activations (64-bit row offsets), the grid: everything the kernel indexes stays in range
  const int64_t tiles = (K / DG_KT) * ((M + DG_PASS_M - 1) / DG_PASS_M);
  if (N > INT32_MAX || K > INT32_MAX || M > INT32_MAX || (N / per) * K > static_cast<int64_t>(UINT32_MAX) || (N / group_size) * K > INT32_MAX ||
      tiles > INT32_MAX) {
    set_error("%s: size overflow", who);
    return HQQ_ERR_SHAPE;
  }
  return 0;
}

}  // namespace hqq

using namespace hqq;

extern "C" int hqq_hip_gemm_dgrad_axis0_covers(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype) {
  return dg0_validate(nbits, M, N, K, group_size, dtype) == 0 ? 1 : 0;
}

extern "C" int hqq_hip_gemm_dgrad_axis0(int nbits, const void* g, const void* Wq, const void* scale, const void* zero, void* dx, int64_t M, int64_t N,
                                        int64_t K, int64_t group_size, int dtype, void* stream) {
  if (const int rc = dg0_validate(nbits, M, N, K, group_size, dtype)) return rc;
  clear_stale_error();
  if (!g || !Wq || !scale || !zero || !dx) { set_error("hqq_hip_gemm_dgrad_axis0: null argument"); return HQQ_ERR_SHAPE; }
  if (!aligned16(g) || !aligned16(Wq) || !aligned16(dx) || !aligned16(scale) || !aligned16(zero)) {
    set_error("hqq_hip_gemm_dgrad_axis0: g / Wq / scale / zero / dx must be 16-byte aligned");
    return HQQ_ERR_ALIGN;
  }
  const int per = 8 / nbits;
  const int ktiles = static_cast<int>(K / DG_KT);
  const int grid = static_cast<int>(ktiles * ((M + DG_PASS_M - 1) / DG_PASS_M));
  const int Mi = static_cast<int>(M), Ni = static_cast<int>(N), Ki = static_cast<int>(K), Np = static_cast<int>(N / per);
  const int Nr = static_cast<int>(N / group_size);
  const bool stage = Nr <= DG0_LDS_MAX_NR;   // the meta slab of a k tile fits under the reduce buffer
  hipStream_t st = as_stream(stream);
  const auto* gp = static_cast<const uint16_t*>(g);
  const auto* ws = static_cast<const uint8_t*>(Wq);
  const auto* ss = static_cast<const uint16_t*>(scale);
  const auto* zs = static_cast<const uint16_t*>(zero);
  auto* out = static_cast<uint16_t*>(dx);
#define HQQ_DG0_LAUNCH(NB, BF)                                                                                                                              \
  do {                                                                                                                                                      \
    if (stage) hipLaunchKernelGGL((gemm_dgrad_axis0_kernel<NB, BF, true>), dim3(grid), dim3(DG_WAVES * 64), 0, st, gp, ws, ss, zs, out, Mi, Ni, Ki, Np, Nr, ktiles);  \
    else hipLaunchKernelGGL((gemm_dgrad_axis0_kernel<NB, BF, false>), dim3(grid), dim3(DG_WAVES * 64), 0, st, gp, ws, ss, zs, out, Mi, Ni, Ki, Np, Nr, ktiles);  \
  } while (0)
  if (dtype == HQQ_BF16) {
    switch (nbits) {
      case 8: HQQ_DG0_LAUNCH(8, true); break;
      case 4: HQQ_DG0_LAUNCH(4, true); break;
      default: HQQ_DG0_LAUNCH(2, true); break;
    }
  } else {
    switch (nbits) {
      case 8: HQQ_DG0_LAUNCH(8, false); break;
      case 4: HQQ_DG0_LAUNCH(4, false); break;
      default: HQQ_DG0_LAUNCH(2, false); break;
    }
  }
#undef HQQ_DG0_LAUNCH
  return check_launch("hqq_hip_gemm_dgrad_axis0");
}
