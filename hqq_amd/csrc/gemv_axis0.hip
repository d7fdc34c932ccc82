// gemv_axis0.hip — the decode kernel for layers quantised along axis 0 (hqq_hip_gemv_axis0): fused unpack -> dequantize -> GEMV, gfx950.
//
// Replaces, for axis=0 layers, the chain HQQLinear.forward runs for them (hqq/core/quantize.py:183-199, :880-898): the dequantise kernel writes
// the whole fp16 weight, torch.matmul reads it back.  One pass over the packed bytes and the meta instead.
//
// Layout.  axis 0 views the level matrix as [gs, C], C = N K / gs, one (scale, zero) per COLUMN.  For the byte containers the packed bytes
// of that view are the axis-1 packed bytes of the same [N, K] matrix: byte (p, k), p < N / per, holds W[p + s N / per, k] in slab s.  With
// gs | N and S = N / gs, weight W[n, k] uses meta column (n mod S) K + k: the meta is an [S, K] matrix, output rows n = r (mod S) share meta
// row r — the "class" r — and so do the `per` rows of one packed byte (N / per is a multiple of S).
//
// Work.  A wave owns (class r, a block of up to 16 * NBITS packed rows of the class = 128 output rows, a K-split of whole 64-k units).  Per
// unit a lane fetches 16 k of its (scale, zero) row and of x ONCE and rebuilds the weights of every packed row of its block against them:
// each meta element leaves HBM once per call (the blocks of one class are neighbouring waves when the class has more than 128 rows).
// Contraction: mfma_f32_16x16x32_{f16,bf16} with A = 16 packed rows of the class (lane l: row l & 15, k octet l >> 4) and B = x (column
// m = l & 15, up to 16 activation rows, zero padded), one MFMA pair per unit and slab.  A lane group's 16 k are its own 16 consecutive
// bytes of the row (one 16-byte load), kept in the byte-pair order of biased_levels (decode_common.h) in A, B and the meta alike.
// Weights: round(round(q - z) * s) in the compute dtype, the two roundings of Quantizer.dequantize — bit-identical to hqq_hip_dequantize.
// Split-K: every wave parks its fp32 partial sums in the caller's workspace (past the counter head, which stays untouched); a second
// launch sums the splits in split order, rounds once and adds the bias (one more rounding): deterministic, shape-only split rule.
// Grouped (hqq_hip_gemv_axis0_grouped): up to three layers on the same x — q|k|v, gate|up — as ONE contraction launch over their concatenated work
// items and ONE reduce launch; each layer keeps its own plan and partial-sum area, so its output is the single-layer call's bit for bit.  The
// reduce can finish gate|up as silu(gate) * up (HQQ_BLOCK_SILU, block_math.h's silu_mul_el on the two rounded outputs).
#include "axis0_common.h"
#include "block_math.h"

namespace hqq {

constexpr int A0_WAVES = 4;             // waves per workgroup (independent work items, no LDS)
constexpr int A0_TARGET_WAVES = 2048;   // ~8 waves per CU before K is split further
constexpr int A0_MAX_SPLITS = 64;

struct A0Plan {
  int S, P, nblocks, splits, upc, units;
  int64_t items;
};

static A0Plan a0_plan(int nbits, int64_t N, int64_t K, int64_t gs) {
  A0Plan p;
  const int per = 8 / nbits;
  p.S = static_cast<int>(N / gs);
  p.P = static_cast<int>(gs / per);
  const int rows_per_block = 16 * nbits;   // NBITS tiles of 16 packed rows: 128 output rows whatever the width
  p.nblocks = (p.P + rows_per_block - 1) / rows_per_block;
  p.units = static_cast<int>(K / A0_KU);
  const int64_t base = static_cast<int64_t>(p.S) * p.nblocks;
  int64_t sp = (A0_TARGET_WAVES + base - 1) / base;
  if (sp > A0_MAX_SPLITS) sp = A0_MAX_SPLITS;
  if (sp > p.units) sp = p.units;
  if (sp < 1) sp = 1;
  p.upc = static_cast<int>((p.units + sp - 1) / sp);
  p.splits = (p.units + p.upc - 1) / p.upc;
  p.items = base * p.splits;
  return p;
}

// one work item — (class, block of the class, K split) number `item` of ONE layer's plan — by the calling wave: shared by the single-layer kernel
// and the grouped one, so that a layer's partial sums are the same bits in either
template <int NBITS, bool BF16>
__device__ __forceinline__ void a0_item(const uint16_t* __restrict__ x, const uint8_t* __restrict__ Wq, const uint16_t* __restrict__ scale,
                                        const uint16_t* __restrict__ zero, float* __restrict__ part, int M, int N, int K, int S, int P, int nblocks,
                                        int upc, int units, int64_t item) {
  constexpr int PER = 8 / NBITS;
  constexpr int TB = NBITS;   // tiles of 16 packed rows per wave: TB * 16 * PER = 128 output rows
  const int lane = threadIdx.x & 63;
  const int b = static_cast<int>(item % nblocks);
  const int64_t rest = item / nblocks;
  const int r = static_cast<int>(rest % S);
  const int split = static_cast<int>(rest / S);
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
  const bool mv = col < M;
  const uint16_t* xrow = x + static_cast<int64_t>(mv ? col : 0) * K + 16 * g;
  const uint32_t magic = 0x64006400u;
  f32x4 acc[TB][PER];
#pragma unroll
  for (int tl = 0; tl < TB; ++tl)
#pragma unroll
    for (int j = 0; j < PER; ++j) acc[tl][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int u0 = split * upc;
  const int u1 = u0 + upc < units ? u0 + upc : units;
  for (int u = u0; u < u1; ++u) {
    const int k = u * A0_KU;
    u32x4 w[TB];
#pragma unroll
    for (int tl = 0; tl < TB; ++tl) w[tl] = tl < ntiles ? ld16_nt(wrow[tl] + k) : u32x4{0u, 0u, 0u, 0u};
    const u32x4 s0 = permute_x8(ld16(srow + k)), s1 = permute_x8(ld16(srow + k + 8));
    const u32x4 z0 = permute_x8(ld16(zrow + k)), z1 = permute_x8(ld16(zrow + k + 8));
    u32x4 x0 = ld16(xrow + k), x1 = ld16(xrow + k + 8);
    if (!mv) { x0 = u32x4{0u, 0u, 0u, 0u}; x1 = x0; }
    x0 = permute_x8(x0);
    x1 = permute_x8(x1);
    if constexpr (!BF16) {
      half2_t zz[8], ss[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { zz[i] = as_h2(z0[i]); zz[4 + i] = as_h2(z1[i]); ss[i] = as_h2(s0[i]); ss[4 + i] = as_h2(s1[i]); }
      const h8_t b0 = __builtin_bit_cast(h8_t, x0), b1 = __builtin_bit_cast(h8_t, x1);
#pragma unroll
      for (int tl = 0; tl < TB; ++tl)
        if (tl < ntiles) A0Slabs<NBITS, 0>::f16(w[tl], zz, ss, b0, b1, acc[tl], magic);
    } else {
      uint32_t zz[8], ss[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { zz[i] = z0[i]; zz[4 + i] = z1[i]; ss[i] = s0[i]; ss[4 + i] = s1[i]; }
      const bf16x8_t b0 = __builtin_bit_cast(bf16x8_t, x0), b1 = __builtin_bit_cast(bf16x8_t, x1);
#pragma unroll
      for (int tl = 0; tl < TB; ++tl)
        if (tl < ntiles) A0Slabs<NBITS, 0>::bf16(w[tl], zz, ss, b0, b1, acc[tl]);
    }
  }
  // D[i][m]: lane l holds m = l & 15 and packed rows t0 + 16 tl + 4 (l >> 4) + reg; output row n = r + (t + slab P) S
  if (!mv) return;
  float* out = part + (static_cast<int64_t>(split) * M + col) * N;
#pragma unroll
  for (int tl = 0; tl < TB; ++tl) {
    if (tl >= ntiles) break;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int t = t0 + 16 * tl + 4 * g + rg;
      if (t < P) {
#pragma unroll
        for (int j = 0; j < PER; ++j) out[r + static_cast<int64_t>(t + j * P) * S] = acc[tl][j][rg];
      }
    }
  }
}

template <int NBITS, bool BF16>
__global__ __launch_bounds__(A0_WAVES * 64) void gemv_axis0_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ Wq,
                                                                  const uint16_t* __restrict__ scale, const uint16_t* __restrict__ zero,
                                                                  float* __restrict__ part, int M, int N, int K, int S, int P, int nblocks,
                                                                  int upc, int units, int64_t items) {
  const int64_t item = static_cast<int64_t>(blockIdx.x) * A0_WAVES + (threadIdx.x >> 6);
  if (item >= items) return;
  a0_item<NBITS, BF16>(x, Wq, scale, zero, part, M, N, K, S, P, nblocks, upc, units, item);
}

// hqq_hip_gemv_axis0_grouped: the work items of up to A0_MAX_GROUP layers that read the same x, concatenated.  Item i belongs to the first layer whose
// running total `end` exceeds it and is item i - (the previous layer's end) of that layer's OWN plan (a0_plan of the layer alone)
constexpr int A0_MAX_GROUP = 3;
struct A0Member {
  const uint8_t* Wq;
  const uint16_t* scale;
  const uint16_t* zero;
  float* part;      // the layer's own partial-sum area [splits, M, N]
  int64_t end;      // work items of this layer and the ones before it (layers past n_layers repeat the total)
  int N, S, P, nblocks, upc, splits;
};
struct A0Group {
  A0Member l[A0_MAX_GROUP];
};

template <int NBITS, bool BF16>
__global__ __launch_bounds__(A0_WAVES * 64) void gemv_axis0_grouped_kernel(const uint16_t* __restrict__ x, const A0Group g, int M, int K, int units) {
  // (the wave index through readfirstlane: the member is then picked with scalar loads from the kernel arguments)
  const int64_t item = static_cast<int64_t>(blockIdx.x) * A0_WAVES + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (item >= g.l[A0_MAX_GROUP - 1].end) return;
  int li = 0;
  int64_t first = 0;
  if (item >= g.l[0].end) { li = 1; first = g.l[0].end; }
  if (item >= g.l[1].end) { li = 2; first = g.l[1].end; }
  const A0Member& m = g.l[li];
  a0_item<NBITS, BF16>(x, m.Wq, m.scale, m.zero, m.part, M, m.N, K, m.S, m.P, m.nblocks, m.upc, units, item - first);
}

// y[m, n] = round(sum over splits, in split order) (+ bias)
template <bool BF16>
__global__ __launch_bounds__(256) void gemv_axis0_reduce_kernel(const float* __restrict__ part, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
                                                                int M, int N, int splits) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t MN = static_cast<int64_t>(M) * N;
  if (i >= MN) return;
  const float s = a0_sum_splits(part, MN, i, splits);
  y[i] = a0_finish<BF16>(s, bias, static_cast<int>(i % N));
}

// the grouped call's reduce, one launch for every member.  Plain: blockIdx.y is the member, finished as gemv_axis0_reduce_kernel finishes a layer.
// SILU (two members of equal N, hence equal plans): thread i finishes gate[i] and up[i] as above — both rounded to the compute dtype — and writes
// y[0][i] = silu_mul_el(gate, up), the bits hqq_hip_silu_mul gives on the two separately written outputs
struct A0ReduceMember {
  const float* part;
  const uint16_t* bias;
  uint16_t* y;
  int N, splits;
};
struct A0ReduceGroup {
  A0ReduceMember l[A0_MAX_GROUP];
};

template <bool BF16, bool SILU>
__global__ __launch_bounds__(256) void gemv_axis0_grouped_reduce_kernel(const A0ReduceGroup g, int M) {
  const A0ReduceMember& m = g.l[SILU ? 0 : blockIdx.y];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t MN = static_cast<int64_t>(M) * m.N;
  if (i >= MN) return;
  const int n = static_cast<int>(i % m.N);
  const uint16_t a = a0_finish<BF16>(a0_sum_splits(m.part, MN, i, m.splits), m.bias, n);
  if constexpr (SILU) {
    const uint16_t u = a0_finish<BF16>(a0_sum_splits(g.l[1].part, MN, i, g.l[1].splits), g.l[1].bias, n);
    m.y[i] = silu_mul_el<BF16>(a, u);
  } else {
    m.y[i] = a;
  }
}

// what the kernel covers, checked before anything is launched: 0, or an HQQ_ERR_* with the message set
static int a0_validate(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts) {
  return a0_validate_rows("hqq_hip_gemv_axis0", 1, HQQ_GEMV_MAX_M, A0_MAX_SPLITS, nbits, M, N, K, group_size, dtype, opts);
}

// the grouped call: every member must be a layer hqq_hip_gemv_axis0 covers (a0_validate names the first that is not), then the flags
static int a0g_validate(int nbits, int n_layers, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype, uint32_t opts, uint32_t flags) {
  if (n_layers < 1 || n_layers > A0_MAX_GROUP) { set_error("hqq_hip_gemv_axis0_grouped: n_layers=%d outside [1,%d]", n_layers, A0_MAX_GROUP); return HQQ_ERR_SHAPE; }
  if (!N) { set_error("hqq_hip_gemv_axis0_grouped: null argument"); return HQQ_ERR_SHAPE; }
  for (int i = 0; i < n_layers; ++i)
    if (const int rc = a0_validate(nbits, M, N[i], K, group_size, dtype, opts)) return rc;
  if (flags & ~HQQ_BLOCK_SILU) {
    set_error("hqq_hip_gemv_axis0_grouped: flags 0x%x are not covered (0 or HQQ_BLOCK_SILU)", flags);
    return HQQ_ERR_UNSUPPORTED;
  }
  if ((flags & HQQ_BLOCK_SILU) && (n_layers != 2 || N[0] != N[1])) {
    set_error("hqq_hip_gemv_axis0_grouped: HQQ_BLOCK_SILU is not covered here: it takes two layers (gate, up) of equal N");
    return HQQ_ERR_UNSUPPORTED;
  }
  return 0;
}

// bytes of one member's partial-sum area (what hqq_hip_gemv_axis0_workspace_bytes adds to the counter head for the layer alone)
static size_t a0_part_bytes(const A0Plan& p, int64_t M, int64_t N) {
  return (static_cast<size_t>(p.splits) * M * N * sizeof(float) + 15) & ~static_cast<size_t>(15);
}

}  // namespace hqq

using namespace hqq;

extern "C" size_t hqq_hip_gemv_axis0_workspace_bytes(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype) {
  if (a0_validate(nbits, M, N, K, group_size, dtype, 0)) return 0;
  const A0Plan p = a0_plan(nbits, N, K, group_size);
  return WS_COUNTER_BYTES + a0_part_bytes(p, M, N);
}

extern "C" int hqq_hip_gemv_axis0(int nbits, const void* x, const void* Wq, const void* scale, const void* zero, const void* bias, void* y,
                                  int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  clear_stale_error();
  if (const int rc = a0_validate(nbits, M, N, K, group_size, dtype, opts)) return rc;
  if (!x || !Wq || !scale || !zero || !y) { set_error("hqq_hip_gemv_axis0: null argument"); return HQQ_ERR_SHAPE; }
  if (!aligned16(x) || !aligned16(Wq) || !aligned16(scale) || !aligned16(zero)) { set_error("hqq_hip_gemv_axis0: pointers must be 16-byte aligned"); return HQQ_ERR_ALIGN; }
  const size_t need = hqq_hip_gemv_axis0_workspace_bytes(nbits, M, N, K, group_size, dtype);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("hqq_hip_gemv_axis0: needs %zu bytes of 16-byte aligned workspace (got %zu)", need, workspace_bytes);
    return HQQ_ERR_WORKSPACE;
  }
  const A0Plan p = a0_plan(nbits, N, K, group_size);
  float* part = reinterpret_cast<float*>(static_cast<uint8_t*>(workspace) + WS_COUNTER_BYTES);
  hipStream_t st = as_stream(stream);
  const int grid = static_cast<int>((p.items + A0_WAVES - 1) / A0_WAVES);
  const auto* xs = static_cast<const uint16_t*>(x);
  const auto* ws = static_cast<const uint8_t*>(Wq);
  const auto* ss = static_cast<const uint16_t*>(scale);
  const auto* zs = static_cast<const uint16_t*>(zero);
  const int Mi = static_cast<int>(M), Ni = static_cast<int>(N), Ki = static_cast<int>(K);
#define HQQ_A0_LAUNCH(NB, BF)                                                                                                            \
  hipLaunchKernelGGL((gemv_axis0_kernel<NB, BF>), dim3(grid), dim3(A0_WAVES * 64), 0, st, xs, ws, ss, zs, part, Mi, Ni, Ki, p.S, p.P, \
                     p.nblocks, p.upc, p.units, p.items)
  if (dtype == HQQ_BF16) {
    if (nbits == 4) HQQ_A0_LAUNCH(4, true); else HQQ_A0_LAUNCH(2, true);
  } else {
    switch (nbits) {
      case 8: HQQ_A0_LAUNCH(8, false); break;
      case 4: HQQ_A0_LAUNCH(4, false); break;
      case 2: HQQ_A0_LAUNCH(2, false); break;
      default: HQQ_A0_LAUNCH(1, false); break;
    }
  }
#undef HQQ_A0_LAUNCH
  if (const int rc = check_launch("hqq_hip_gemv_axis0")) return rc;
  const int64_t MN = M * N;
  const int rgrid = static_cast<int>((MN + 255) / 256);
  if (dtype == HQQ_BF16)
    hipLaunchKernelGGL(gemv_axis0_reduce_kernel<true>, dim3(rgrid), dim3(256), 0, st, part, static_cast<const uint16_t*>(bias), static_cast<uint16_t*>(y), Mi, Ni, p.splits);
  else
    hipLaunchKernelGGL(gemv_axis0_reduce_kernel<false>, dim3(rgrid), dim3(256), 0, st, part, static_cast<const uint16_t*>(bias), static_cast<uint16_t*>(y), Mi, Ni, p.splits);
  return check_launch("hqq_hip_gemv_axis0");
}

extern "C" size_t hqq_hip_gemv_axis0_grouped_workspace_bytes(int nbits, int n_layers, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype,
                                                            uint32_t flags) {
  if (a0g_validate(nbits, n_layers, N, M, K, group_size, dtype, 0, flags)) return 0;
  size_t bytes = WS_COUNTER_BYTES;
  for (int i = 0; i < n_layers; ++i) bytes += a0_part_bytes(a0_plan(nbits, N[i], K, group_size), M, N[i]);
  return bytes;
}

extern "C" int hqq_hip_gemv_axis0_grouped(int nbits, int n_layers, const void* x, const void* const* Wq, const void* const* scale, const void* const* zero,
                                          const void* const* bias, void* const* y, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype,
                                          uint32_t opts, uint32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  clear_stale_error();
  if (const int rc = a0g_validate(nbits, n_layers, N, M, K, group_size, dtype, opts, flags)) return rc;
  const bool silu = flags & HQQ_BLOCK_SILU;
  if (!x || !Wq || !scale || !zero || !y) { set_error("hqq_hip_gemv_axis0_grouped: null argument"); return HQQ_ERR_SHAPE; }
  if (!aligned16(x)) { set_error("hqq_hip_gemv_axis0_grouped: pointers must be 16-byte aligned"); return HQQ_ERR_ALIGN; }
  for (int i = 0; i < n_layers; ++i) {
    if (!Wq[i] || !scale[i] || !zero[i] || (!y[i] && !(silu && i == 1))) { set_error("hqq_hip_gemv_axis0_grouped: null argument (layer %d)", i); return HQQ_ERR_SHAPE; }
    if (!aligned16(Wq[i]) || !aligned16(scale[i]) || !aligned16(zero[i])) {
      set_error("hqq_hip_gemv_axis0_grouped: pointers must be 16-byte aligned (layer %d)", i);
      return HQQ_ERR_ALIGN;
    }
  }
  const size_t need = hqq_hip_gemv_axis0_grouped_workspace_bytes(nbits, n_layers, N, M, K, group_size, dtype, flags);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("hqq_hip_gemv_axis0_grouped: needs %zu bytes of 16-byte aligned workspace (got %zu)", need, workspace_bytes);
    return HQQ_ERR_WORKSPACE;
  }
  A0Group g;
  A0ReduceGroup rg;
  uint8_t* area = static_cast<uint8_t*>(workspace) + WS_COUNTER_BYTES;
  int64_t items = 0, max_mn = 0;
  for (int i = 0; i < A0_MAX_GROUP; ++i) {
    A0Member& m = g.l[i];
    A0ReduceMember& r = rg.l[i];
    if (i >= n_layers) {   // never selected: no item reaches `end`, no reduce workgroup carries the index
      m = A0Member{nullptr, nullptr, nullptr, nullptr, items, 0, 1, 1, 1, 1, 1};
      r = A0ReduceMember{nullptr, nullptr, nullptr, 0, 0};
      continue;
    }
    const A0Plan p = a0_plan(nbits, N[i], K, group_size);
    items += p.items;
    m = A0Member{static_cast<const uint8_t*>(Wq[i]), static_cast<const uint16_t*>(scale[i]), static_cast<const uint16_t*>(zero[i]),
                 reinterpret_cast<float*>(area), items, static_cast<int>(N[i]), p.S, p.P, p.nblocks, p.upc, p.splits};
    r = A0ReduceMember{m.part, bias ? static_cast<const uint16_t*>(bias[i]) : nullptr, static_cast<uint16_t*>(y[i]), m.N, p.splits};
    area += a0_part_bytes(p, M, N[i]);
    if (M * N[i] > max_mn) max_mn = M * N[i];
  }
  hipStream_t st = as_stream(stream);
  const int grid = static_cast<int>((items + A0_WAVES - 1) / A0_WAVES);
  const auto* xs = static_cast<const uint16_t*>(x);
  const int Mi = static_cast<int>(M), Ki = static_cast<int>(K), units = static_cast<int>(K / A0_KU);
#define HQQ_A0G_LAUNCH(NB, BF) hipLaunchKernelGGL((gemv_axis0_grouped_kernel<NB, BF>), dim3(grid), dim3(A0_WAVES * 64), 0, st, xs, g, Mi, Ki, units)
  if (dtype == HQQ_BF16) {
    if (nbits == 4) HQQ_A0G_LAUNCH(4, true); else HQQ_A0G_LAUNCH(2, true);
  } else {
    switch (nbits) {
      case 8: HQQ_A0G_LAUNCH(8, false); break;
      case 4: HQQ_A0G_LAUNCH(4, false); break;
      case 2: HQQ_A0G_LAUNCH(2, false); break;
      default: HQQ_A0G_LAUNCH(1, false); break;
    }
  }
#undef HQQ_A0G_LAUNCH
  if (const int rc = check_launch("hqq_hip_gemv_axis0_grouped")) return rc;
  const dim3 rgrid(static_cast<unsigned>((max_mn + 255) / 256), silu ? 1u : static_cast<unsigned>(n_layers));
  if (dtype == HQQ_BF16) {
    if (silu) hipLaunchKernelGGL((gemv_axis0_grouped_reduce_kernel<true, true>), rgrid, dim3(256), 0, st, rg, Mi);
    else hipLaunchKernelGGL((gemv_axis0_grouped_reduce_kernel<true, false>), rgrid, dim3(256), 0, st, rg, Mi);
  } else {
    if (silu) hipLaunchKernelGGL((gemv_axis0_grouped_reduce_kernel<false, true>), rgrid, dim3(256), 0, st, rg, Mi);
    else hipLaunchKernelGGL((gemv_axis0_grouped_reduce_kernel<false, false>), rgrid, dim3(256), 0, st, rg, Mi);
  }
  return check_launch("hqq_hip_gemv_axis0_grouped");
}
