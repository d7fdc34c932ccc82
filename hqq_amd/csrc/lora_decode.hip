// lora_decode.hip — the adapter term of UN-MERGED LoRA layers in the decode step (hqq_hip_lora_shrink + hqq_hip_lora_expand), gfx950.
//
// For a group of 1 .. HQQ_GEMV_MAX_GROUP layers that read the same activation rows x[M, K] (q | k | v, gate | up, or one layer), each with A_l [K, r_l],
// B_l [r_l, N_l], a host float s_l and an output y_l [M, N_l] that already holds the base layer's result:
//     t_l[m, j] = sum_k x[m, k] * A_l[k, j]                     fp32
//     u_l[m, n] = s_l * sum_j t_l[m, j] * B_l[j, n]             fp32
//     y_l[m, n] = rnd(y_l[m, n] + rnd(u_l[m, n]))               rnd: one round-to-nearest-even to the compute dtype
// The two roundings are HQQLinearLoRA.forward's `out + forward_lora(x).to(x_dtype)` (hqq/core/peft.py:150-165).  t and u stay in fp32: for fp32 adapters
// that is the reference's arithmetic up to summation order; for fp16 / bf16 adapters the reference ALSO rounds t, t @ B and the product with s to the
// adapter's dtype and this file does not — the same value with fewer roundings (include/hqq_hip.h and README say so too).
//
// What it replaces: per adapted linear, two torch matmuls, a scale, a cast and an add — five eager launches behind every GEMV of the decode step.
// Here a GROUP costs two short launches behind its base launch, whatever the number of adapted layers in it.
//
// shrink.  K is cut into slices of ld_kslice(r) = 256 / 512 / 1024 k (r <= 64 / <= 128 / <= 256: a workgroup's share of A stays at 16K .. 64K elements
// and the number of partials the expand sums stays bounded).  Workgroup (slice i, layer l) — blockIdx.x, blockIdx.y — of 256 threads walks its slice in
// chunks of LD_KC = 256 k: the chunk of x is staged ONCE into LDS as fp32, [k][row] (16-byte loads of 8 elements; rows past M and k past the slice
// are staged as zeros), then thread (jj = tid % RJ, kk = tid / RJ), RJ = the power of two >= r, owns column jj and the k = kk, kk + KL, kk + 2 KL ...
// of the chunk (KL = 256 / RJ): lanes run along j first, then along k, so a wave reads whole consecutive rows of A.  One fmaf per (row, k) into the
// row's accumulator, rows from LDS with ds_read_b128 (the same address across the lanes of one k: a broadcast).  The KL accumulators of a column are
// then summed through LDS in kk order and the slice's partial t goes to the caller's workspace, [layer][slice][M][r_l] fp32.  No float atomics, no
// arrival counters; every partial is written before the expand reads it, so the workspace needs no clearing.
// expand.  Workgroup (tile, layer) of 256 threads owns LD_EN = 256 columns n.  It first sums the S partials of its layer in slice order into LDS
// ([j][row], rows past M zero), then thread n forms u over j = 0 .. r - 1 in ascending order — B read coalesced along n, t as ds_read_b128 broadcasts —
// and performs the read-modify-write of y.
//
// Summation order.  The slice size, RJ / KL, the order inside a slice (chunk by chunk; within a chunk a thread's k ascending; then kk ascending), the
// slice order and the order over j are functions of (K, r_l) alone.  The row count only picks how many accumulators a thread carries (template MR =
// 1 / 4 / 8 / 16 >= M): every row's chain of fmaf / adds is the same sequence in each instantiation.  So two calls give the same bits, and row m of an
// M-row call has the bits of a one-row call on that row alone — the property of every *_batched kernel of this library.
//
// Loads of A and B are one element per lane (ranks are arbitrary, 1 .. 256, and a row of A is r elements long): a wave still covers contiguous
// memory.  Both kernels move K r + r N adapter elements once (0.25 - 3 MB at 7B shapes) and are latency-bound; the aim is two short launches.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any instantiation):
//   lora_shrink_kernel<MR = 1 / 4 / 8 / 16, *>      VGPRs 28 / 40 / 58 / 92        SGPRs 54 - 56   LDS 2048 / 8192 / 16384 / 32768 B   8 / 8 / 8 / 5 waves per SIMD
//   lora_expand_kernel<MR = 1 / 4 / 8 / 16, *, *>   VGPRs 15 / 28-32 / 48-52 / 64-69   SGPRs 28 - 29   LDS 1024 / 4096 / 8192 / 16384 B
#include "hqq_common.h"

namespace hqq {

constexpr int LD_THREADS = 256;
constexpr int LD_KC = 256;               // k per staged chunk of x
constexpr int LD_EN = 256;               // columns per expand workgroup: one per thread
constexpr int LD_MAX_R = 256;
constexpr int LD_MAX_M = HQQ_GEMV_MAX_M;
constexpr int64_t LD_MAX_DIM = int64_t(1) << 24;   // K and N_l: every flat index of a launch but A's and B's (64-bit) fits 32 bits

// k per slice, the number of slices and the column stride RJ: functions of (K, r) alone (host and device agree through the kernel arguments)
static inline int ld_kslice(int64_t r) { return r <= 64 ? 256 : (r <= 128 ? 512 : 1024); }
static inline int ld_slices(int64_t K, int64_t r) { return static_cast<int>((K + ld_kslice(r) - 1) / ld_kslice(r)); }
static inline int ld_rj(int64_t r) { int p = 1; while (p < r) p <<= 1; return p; }
static inline int ld_rows(int64_t M) { return M <= 1 ? 1 : (M <= 4 ? 4 : (M <= 8 ? 8 : 16)); }

// adapter element -> fp32
template <int LDT>
static __device__ __forceinline__ float ld_load(const void* p, int64_t i) {
  if constexpr (LDT == HQQ_F32) return static_cast<const float*>(p)[i];
  else if constexpr (LDT == HQQ_F16) return static_cast<float>(static_cast<const half_t*>(p)[i]);
  else return bf16_to_f32(static_cast<const uint16_t*>(p)[i]);
}
static __device__ __forceinline__ float ld_act(uint16_t bits, bool bf16) {
  return bf16 ? bf16_to_f32(bits) : static_cast<float>(__builtin_bit_cast(half_t, bits));
}

struct LdShrinkMember {
  const void* A;
  float* part;          // the layer's partials [slices][M][r]
  int r, rj, rj_log2, ks, slices;
};
struct LdShrinkGroup {
  LdShrinkMember l[HQQ_GEMV_MAX_GROUP];
};

template <int MR, int LDT>
__global__ __launch_bounds__(LD_THREADS) void lora_shrink_kernel(const uint16_t* __restrict__ x, const LdShrinkGroup g, int M, int K, int bf16) {
  const LdShrinkMember& m = g.l[blockIdx.y];
  const int slice = blockIdx.x;
  if (slice >= m.slices) return;
  __shared__ __attribute__((aligned(16))) float xs[LD_KC * MR];     // [k][row]
  __shared__ float red[LD_THREADS * MR];                            // [kk][row][jj]
  const int tid = threadIdx.x;
  const int r = m.r, RJ = m.rj, KL = LD_THREADS >> m.rj_log2;
  const int jj = tid & (RJ - 1), kk = tid >> m.rj_log2;
  const int k0 = slice * m.ks;
  const int kend = k0 + m.ks < K ? k0 + m.ks : K;                   // a multiple of 8, as k0 and every chunk start are
  const bool col = jj < r;

  float acc[MR];
#pragma unroll
  for (int mm = 0; mm < MR; ++mm) acc[mm] = 0.f;

  for (int kc = k0; kc < kend; kc += LD_KC) {
    // x[0 .. MR)[kc .. kc + 256) -> xs, eight elements per load; rows >= M and k >= kend as zeros
    for (int v = tid; v < (LD_KC / 8) * MR; v += LD_THREADS) {
      const int mq = v >> 5, kq = (v & 31) * 8;
      u32x4 raw = {0u, 0u, 0u, 0u};
      if (mq < M && kc + kq < kend) raw = *reinterpret_cast<const u32x4*>(x + static_cast<int64_t>(mq) * K + kc + kq);
#pragma unroll
      for (int c = 0; c < 8; ++c) xs[(kq + c) * MR + mq] = ld_act(static_cast<uint16_t>(raw[c >> 1] >> (16 * (c & 1))), bf16 != 0);
    }
    __syncthreads();
    if (col) {
#pragma unroll 4
      for (int kq = kk; kq < LD_KC; kq += KL) {
        const int k = kc + kq;
        const float a = k < kend ? ld_load<LDT>(m.A, static_cast<int64_t>(k) * r + jj) : 0.f;
        if constexpr (MR == 1) {
          acc[0] = __builtin_fmaf(xs[kq], a, acc[0]);
        } else {
#pragma unroll
          for (int q = 0; q < MR / 4; ++q) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(&xs[kq * MR + 4 * q]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[4 * q + c] = __builtin_fmaf(xv[c], a, acc[4 * q + c]);
          }
        }
      }
    }
    __syncthreads();
  }

  // the KL accumulators of (row, column) summed in kk order
#pragma unroll
  for (int mm = 0; mm < MR; ++mm) red[((kk * MR + mm) << m.rj_log2) + jj] = acc[mm];
  __syncthreads();
  float* part = m.part + static_cast<int64_t>(slice) * M * r;
  for (int o = tid; o < MR * RJ; o += LD_THREADS) {
    const int mm = o >> m.rj_log2, j = o & (RJ - 1);
    if (mm >= M || j >= r) continue;
    float s = red[(mm << m.rj_log2) + j];
    for (int q = 1; q < KL; ++q) s = s + red[((q * MR + mm) << m.rj_log2) + j];
    part[mm * r + j] = s;
  }
}

struct LdExpandMember {
  const void* B;
  const float* part;    // the layer's partials [slices][M][r]
  uint16_t* y;
  float s;
  int r, N, slices;
};
struct LdExpandGroup {
  LdExpandMember l[HQQ_GEMV_MAX_GROUP];
};

template <int MR, int LDT, typename T>
__global__ __launch_bounds__(LD_THREADS) void lora_expand_kernel(const LdExpandGroup g, int M) {
  const LdExpandMember& m = g.l[blockIdx.y];
  const int n0 = static_cast<int>(blockIdx.x) * LD_EN;
  if (n0 >= m.N) return;
  __shared__ __attribute__((aligned(16))) float ts[LD_MAX_R * MR];   // [j][row]
  const int tid = threadIdx.x;
  const int r = m.r, N = m.N, Mr = M * r;
  // t = the S partials in slice order; rows >= M as zeros
  for (int o = tid; o < MR * r; o += LD_THREADS) {
    float s = 0.f;
    if (o < Mr) {
      s = m.part[o];
      for (int i = 1; i < m.slices; ++i) s = s + m.part[static_cast<int64_t>(i) * Mr + o];
    }
    const int mm = o / r, j = o - mm * r;
    ts[j * MR + mm] = s;
  }
  __syncthreads();
  const int n = n0 + tid;
  if (n >= N) return;
  float acc[MR];
#pragma unroll
  for (int mm = 0; mm < MR; ++mm) acc[mm] = 0.f;
#pragma unroll 4
  for (int j = 0; j < r; ++j) {
    const float b = ld_load<LDT>(m.B, static_cast<int64_t>(j) * N + n);
    if constexpr (MR == 1) {
      acc[0] = __builtin_fmaf(ts[j], b, acc[0]);
    } else {
#pragma unroll
      for (int q = 0; q < MR / 4; ++q) {
        const f32x4 tv = *reinterpret_cast<const f32x4*>(&ts[j * MR + 4 * q]);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[4 * q + c] = __builtin_fmaf(tv[c], b, acc[4 * q + c]);
      }
    }
  }
  T* y = reinterpret_cast<T*>(m.y);
#pragma unroll
  for (int mm = 0; mm < MR; ++mm) {
    if (mm < M) {
      const T u = CD<T>::from_f32(m.s * acc[mm]);                                  // forward_lora(x).to(x_dtype)
      const int64_t i = static_cast<int64_t>(mm) * N + n;
      y[i] = CD<T>::from_f32(CD<T>::to_f32(y[i]) + CD<T>::to_f32(u));              // out + ...: one rounding
    }
  }
}

// what the two kernels cover, checked before anything is launched: 0, or an HQQ_ERR_* with the message set.  N may be null (the shrink has no N)
static int ld_validate(const char* who, int n_layers, const int64_t* N, const int64_t* r, int64_t M, int64_t K, int dtype, int a_dtype, int b_dtype) {
  if (n_layers < 1 || n_layers > HQQ_GEMV_MAX_GROUP) {
    set_error("%s: %d layers are not covered (1 .. %d per group)", who, n_layers, HQQ_GEMV_MAX_GROUP);
    return HQQ_ERR_UNSUPPORTED;
  }
  if (!r) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (dtype == HQQ_F32) { set_error("%s: fp32 activations are not covered (fp16 / bf16)", who); return HQQ_ERR_UNSUPPORTED; }
  if (dtype != HQQ_F16 && dtype != HQQ_BF16) { set_error("%s: dtype %d", who, dtype); return HQQ_ERR_DTYPE; }
  for (const int ldt : {a_dtype, b_dtype})
    if (ldt != HQQ_F32 && ldt != HQQ_F16 && ldt != HQQ_BF16) { set_error("%s: adapter dtype %d", who, ldt); return HQQ_ERR_DTYPE; }
  if (a_dtype != b_dtype) { set_error("%s: A (dtype %d) and B (dtype %d) of different dtypes are not covered", who, a_dtype, b_dtype); return HQQ_ERR_UNSUPPORTED; }
  if (M < 1 || M > LD_MAX_M) { set_error("%s: %lld rows are not covered (1 .. %d)", who, (long long)M, LD_MAX_M); return HQQ_ERR_UNSUPPORTED; }
  if (K < 8 || K % 8 || K > LD_MAX_DIM) { set_error("%s: K=%lld is not covered (a multiple of 8, 8 .. 2^24)", who, (long long)K); return HQQ_ERR_UNSUPPORTED; }
  for (int i = 0; i < n_layers; ++i) {
    if (r[i] < 1 || r[i] > LD_MAX_R) { set_error("%s: rank %lld (layer %d) is not covered (1 .. %d)", who, (long long)r[i], i, LD_MAX_R); return HQQ_ERR_UNSUPPORTED; }
    if (N && (N[i] < 8 || N[i] % 8 || N[i] > LD_MAX_DIM)) {
      set_error("%s: N=%lld (layer %d) is not covered (a multiple of 8, 8 .. 2^24)", who, (long long)N[i], i);
      return HQQ_ERR_UNSUPPORTED;
    }
  }
  return 0;
}

static size_t ld_workspace_bytes(int n_layers, const int64_t* r, int64_t M, int64_t K) {
  size_t floats = 0;
  for (int i = 0; i < n_layers; ++i) floats += static_cast<size_t>(ld_slices(K, r[i])) * M * r[i];
  return (floats * sizeof(float) + 15) & ~static_cast<size_t>(15);
}

static bool ld_misaligned(const void* p, int dt) { return (reinterpret_cast<uintptr_t>(p) & (dt == HQQ_F32 ? 3u : 1u)) != 0; }

// ---- the ROUTED pair (hqq_hip_lora_shrink_routed + hqq_hip_lora_expand_routed): one adapter per ROW, picked on the device ---------------------------------
// A_bank[l] is [n_adapters, K, r_l], B_bank[l] [n_adapters, r_l, N_l], scaling_dev[l] fp32 [n_adapters] and slot_dev int64 [M], all in device memory: row m
// takes adapter slot[m], and a row whose slot lies outside [0, n_adapters) takes none — its y is not written, no adapter byte is read for it and its partials
// are neither written nor read.  The kernels are the two above with a third grid dimension over the ROWS: workgroup (slice or tile, layer, z) serves the
// adapter of row z — if row z selects one and no earlier row selects the same (ld_lead: at most 16 scalar loads and compares; every other workgroup retires
// at once) — for ALL the rows that select it (a bit mask, wave-uniform), and a row's accumulator takes the fmaf only under that mask.  A row therefore runs
// exactly the chain of the kernels above — the chunk order, a thread's ascending k, the kk order, the slice order, ascending j, one fmaf per term (the zero
// term past the end of a slice included), the two roundings — with its adapter's elements and no term from another: the bits of a one-row call with that
// adapter.  An adapter no row selects is never addressed; one that several rows select is streamed once per workgroup; distinct adapters run side by side
// (the grids above fill a fraction of the device: 16 slices x 3 layers at K = 4096).
// The first design walked the distinct adapters one after the other INSIDE workgroup (slice, layer), x staged once for all of them: the same bits, but the
// launch grew with every further adapter (profiles/lora_bank_summary.md keeps the comparison), so the grid dimension is the one kept.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any instantiation): LDS as the kernels above;
//   lora_shrink_routed_kernel<MR = 1 / 4 / 8 / 16, *>      VGPRs 26 / 38 / 56 / 90   SGPRs 58 / 66 / 72 / 90   8 / 8 / 8 / 5 waves per SIMD
//   lora_expand_routed_kernel<MR = 1 / 4 / 8 / 16, *, *>   VGPRs 17 / 28 / 44 / 71   SGPRs 32 / 40 / 48 / 64   8 / 8 / 8 / 7 waves per SIMD
constexpr int64_t LD_MAX_ADAPTERS = 256;

// whether workgroup z serves an adapter: row z selects one and is the first row to select it; then a_id = that adapter, mask = the rows that select it.
// Every operand is wave-uniform (scalar loads of the M <= 16 slots)
static __device__ __forceinline__ bool ld_lead(const int64_t* __restrict__ slot, int M, int n_adapters, int z, int& a_id, unsigned& mask) {
  const int64_t s = slot[z];
  if (s < 0 || s >= n_adapters) return false;
  unsigned m = 0u;
  for (int mm = 0; mm < M; ++mm) m |= (slot[mm] == s ? 1u : 0u) << mm;
  if (m & ((1u << z) - 1u)) return false;
  a_id = static_cast<int>(s);
  mask = m;
  return true;
}

template <int MR, int LDT>
__global__ __launch_bounds__(LD_THREADS) void lora_shrink_routed_kernel(const uint16_t* __restrict__ x, const LdShrinkGroup g, const int64_t* __restrict__ slot,
                                                                         int n_adapters, int M, int K, int bf16) {
  const LdShrinkMember& m = g.l[blockIdx.y];
  const int slice = blockIdx.x;
  if (slice >= m.slices) return;
  int a_id = 0;
  unsigned mask = 0u;
  if (!ld_lead(slot, M, n_adapters, static_cast<int>(blockIdx.z), a_id, mask)) return;
  __shared__ __attribute__((aligned(16))) float xs[LD_KC * MR];     // [k][row]
  __shared__ float red[LD_THREADS * MR];                            // [kk][row][jj]
  const int tid = threadIdx.x;
  const int r = m.r, RJ = m.rj, KL = LD_THREADS >> m.rj_log2;
  const int jj = tid & (RJ - 1), kk = tid >> m.rj_log2;
  const int k0 = slice * m.ks;
  const int kend = k0 + m.ks < K ? k0 + m.ks : K;
  const bool col = jj < r;
  const int64_t a0 = a_id * (static_cast<int64_t>(K) * r) + jj;     // this adapter's A, column jj

  float acc[MR];
#pragma unroll
  for (int mm = 0; mm < MR; ++mm) acc[mm] = 0.f;

  for (int kc = k0; kc < kend; kc += LD_KC) {
    // the rows of the mask only: the others' x is not read (their accumulators are not touched either)
    for (int v = tid; v < (LD_KC / 8) * MR; v += LD_THREADS) {
      const int mq = v >> 5, kq = (v & 31) * 8;
      u32x4 raw = {0u, 0u, 0u, 0u};
      if (((mask >> mq) & 1u) && kc + kq < kend) raw = *reinterpret_cast<const u32x4*>(x + static_cast<int64_t>(mq) * K + kc + kq);
#pragma unroll
      for (int c = 0; c < 8; ++c) xs[(kq + c) * MR + mq] = ld_act(static_cast<uint16_t>(raw[c >> 1] >> (16 * (c & 1))), bf16 != 0);
    }
    __syncthreads();
    if (col) {
#pragma unroll 4
      for (int kq = kk; kq < LD_KC; kq += KL) {
        const int k = kc + kq;
        const float a = k < kend ? ld_load<LDT>(m.A, a0 + static_cast<int64_t>(k) * r) : 0.f;
        if constexpr (MR == 1) {
          acc[0] = __builtin_fmaf(xs[kq], a, acc[0]);               // (MR == 1: the mask is row 0)
        } else {
#pragma unroll
          for (int q = 0; q < MR / 4; ++q) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(&xs[kq * MR + 4 * q]);
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if ((mask >> (4 * q + c)) & 1u) acc[4 * q + c] = __builtin_fmaf(xv[c], a, acc[4 * q + c]);
          }
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int mm = 0; mm < MR; ++mm) red[((kk * MR + mm) << m.rj_log2) + jj] = acc[mm];
  __syncthreads();
  float* part = m.part + static_cast<int64_t>(slice) * M * r;
  for (int o = tid; o < MR * RJ; o += LD_THREADS) {
    const int mm = o >> m.rj_log2, j = o & (RJ - 1);
    if (j >= r || !((mask >> mm) & 1u)) continue;                   // (the mask holds rows < M only)
    float s = red[(mm << m.rj_log2) + j];
    for (int q = 1; q < KL; ++q) s = s + red[((q * MR + mm) << m.rj_log2) + j];
    part[mm * r + j] = s;
  }
}

struct LdExpandRoutedMember {
  const void* B;
  const float* part;    // the layer's partials [slices][M][r]
  uint16_t* y;
  const float* s;       // [n_adapters], device memory
  int r, N, slices;
};
struct LdExpandRoutedGroup {
  LdExpandRoutedMember l[HQQ_GEMV_MAX_GROUP];
};

template <int MR, int LDT, typename T>
__global__ __launch_bounds__(LD_THREADS) void lora_expand_routed_kernel(const LdExpandRoutedGroup g, const int64_t* __restrict__ slot, int n_adapters, int M) {
  const LdExpandRoutedMember& m = g.l[blockIdx.y];
  const int n0 = static_cast<int>(blockIdx.x) * LD_EN;
  if (n0 >= m.N) return;
  int a_id = 0;
  unsigned mask = 0u;
  if (!ld_lead(slot, M, n_adapters, static_cast<int>(blockIdx.z), a_id, mask)) return;
  __shared__ __attribute__((aligned(16))) float ts[LD_MAX_R * MR];   // [j][row]
  const int tid = threadIdx.x;
  const int r = m.r, N = m.N, Mr = M * r;
  // t = the S partials in slice order, for the rows of the mask; every other row as zeros (its partials are not read)
  for (int o = tid; o < MR * r; o += LD_THREADS) {
    const int mm = o / r, j = o - mm * r;
    float s = 0.f;
    if ((mask >> mm) & 1u) {
      s = m.part[o];
      for (int i = 1; i < m.slices; ++i) s = s + m.part[static_cast<int64_t>(i) * Mr + o];
    }
    ts[j * MR + mm] = s;
  }
  __syncthreads();
  const int n = n0 + tid;
  if (n >= N) return;
  const float sc = m.s[a_id];
  const int64_t b0 = a_id * (static_cast<int64_t>(r) * N) + n;      // this adapter's B, column n
  float acc[MR];
#pragma unroll
  for (int mm = 0; mm < MR; ++mm) acc[mm] = 0.f;
#pragma unroll 4
  for (int j = 0; j < r; ++j) {
    const float b = ld_load<LDT>(m.B, b0 + static_cast<int64_t>(j) * N);
    if constexpr (MR == 1) {
      acc[0] = __builtin_fmaf(ts[j], b, acc[0]);
    } else {
#pragma unroll
      for (int q = 0; q < MR / 4; ++q) {
        const f32x4 tv = *reinterpret_cast<const f32x4*>(&ts[j * MR + 4 * q]);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if ((mask >> (4 * q + c)) & 1u) acc[4 * q + c] = __builtin_fmaf(tv[c], b, acc[4 * q + c]);
      }
    }
  }
  T* y = reinterpret_cast<T*>(m.y);
#pragma unroll
  for (int mm = 0; mm < MR; ++mm) {
    if ((mask >> mm) & 1u) {
      const T u = CD<T>::from_f32(sc * acc[mm]);
      const int64_t i = static_cast<int64_t>(mm) * N + n;
      y[i] = CD<T>::from_f32(CD<T>::to_f32(y[i]) + CD<T>::to_f32(u));
    }
  }
}

static int ld_validate_routed(const char* who, int n_layers, const int64_t* N, const int64_t* r, int64_t n_adapters, int64_t M, int64_t K, int dtype, int lora_dtype) {
  if (const int rc = ld_validate(who, n_layers, N, r, M, K, dtype, lora_dtype, lora_dtype)) return rc;
  if (n_adapters < 1 || n_adapters > LD_MAX_ADAPTERS) {
    set_error("%s: %lld adapters are not covered (1 .. %lld per bank)", who, (long long)n_adapters, (long long)LD_MAX_ADAPTERS);
    return HQQ_ERR_UNSUPPORTED;
  }
  return 0;
}

}  // namespace hqq

using namespace hqq;

extern "C" int hqq_hip_lora_decode_covers(int n_layers, const int64_t* N, const int64_t* r, int64_t M, int64_t K, int dtype, int a_dtype, int b_dtype) {
  if (!N) { set_error("hqq_hip_lora_decode_covers: null argument"); return 0; }
  return ld_validate("hqq_hip_lora_decode", n_layers, N, r, M, K, dtype, a_dtype, b_dtype) == 0 ? 1 : 0;
}

extern "C" size_t hqq_hip_lora_decode_workspace_bytes(int n_layers, const int64_t* r, int64_t M, int64_t K) {
  if (ld_validate("hqq_hip_lora_decode_workspace_bytes", n_layers, nullptr, r, M, K, HQQ_F16, HQQ_F32, HQQ_F32)) return 0;
  return ld_workspace_bytes(n_layers, r, M, K);
}

extern "C" int hqq_hip_lora_shrink(int n_layers, const void* x, const void* const* A, const int64_t* r, int64_t M, int64_t K, int dtype, int lora_dtype,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "hqq_hip_lora_shrink";
  if (const int rc = ld_validate(who, n_layers, nullptr, r, M, K, dtype, lora_dtype, lora_dtype)) return rc;
  clear_stale_error();
  if (!x || !A) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (!aligned16(x)) { set_error("%s: x must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  for (int i = 0; i < n_layers; ++i) {
    if (!A[i]) { set_error("%s: null argument (layer %d)", who, i); return HQQ_ERR_SHAPE; }
    if (ld_misaligned(A[i], lora_dtype)) { set_error("%s: A must be aligned to its element size (layer %d)", who, i); return HQQ_ERR_ALIGN; }
  }
  const size_t need = ld_workspace_bytes(n_layers, r, M, K);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("%s: needs %zu bytes of 16-byte aligned workspace (got %zu)", who, need, workspace_bytes);
    return HQQ_ERR_WORKSPACE;
  }
  LdShrinkGroup g;
  float* area = static_cast<float*>(workspace);
  int max_slices = 0;
  for (int i = 0; i < HQQ_GEMV_MAX_GROUP; ++i) {
    if (i >= n_layers) { g.l[i] = LdShrinkMember{nullptr, nullptr, 1, 1, 0, LD_KC, 0}; continue; }   // never selected: blockIdx.y < n_layers
    const int rj = ld_rj(r[i]), S = ld_slices(K, r[i]);
    int lg = 0;
    while ((1 << lg) < rj) ++lg;
    g.l[i] = LdShrinkMember{A[i], area, static_cast<int>(r[i]), rj, lg, ld_kslice(r[i]), S};
    area += static_cast<size_t>(S) * M * r[i];
    if (S > max_slices) max_slices = S;
  }
  hipStream_t st = as_stream(stream);
  const dim3 grid(static_cast<unsigned>(max_slices), static_cast<unsigned>(n_layers));
  const auto* xs = static_cast<const uint16_t*>(x);
  const int Mi = static_cast<int>(M), Ki = static_cast<int>(K), bf = dtype == HQQ_BF16 ? 1 : 0;
#define HQQ_LD_SHRINK(MR, LDT) hipLaunchKernelGGL((lora_shrink_kernel<MR, LDT>), grid, dim3(LD_THREADS), 0, st, xs, g, Mi, Ki, bf)
#define HQQ_LD_SHRINK_ROWS(LDT)                     \
  switch (ld_rows(M)) {                             \
    case 1: HQQ_LD_SHRINK(1, LDT); break;           \
    case 4: HQQ_LD_SHRINK(4, LDT); break;           \
    case 8: HQQ_LD_SHRINK(8, LDT); break;           \
    default: HQQ_LD_SHRINK(16, LDT); break;         \
  }
  if (lora_dtype == HQQ_F32) { HQQ_LD_SHRINK_ROWS(HQQ_F32) } else if (lora_dtype == HQQ_F16) { HQQ_LD_SHRINK_ROWS(HQQ_F16) } else { HQQ_LD_SHRINK_ROWS(HQQ_BF16) }
#undef HQQ_LD_SHRINK_ROWS
#undef HQQ_LD_SHRINK
  return check_launch(who);
}

extern "C" int hqq_hip_lora_expand(int n_layers, const void* workspace, size_t workspace_bytes, const void* const* B, const float* scaling, void* const* y,
                                   const int64_t* N, const int64_t* r, int64_t M, int64_t K, int dtype, int lora_dtype, void* stream) {
  const char* who = "hqq_hip_lora_expand";
  if (!N) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (const int rc = ld_validate(who, n_layers, N, r, M, K, dtype, lora_dtype, lora_dtype)) return rc;
  clear_stale_error();
  if (!B || !scaling || !y) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  for (int i = 0; i < n_layers; ++i) {
    if (!B[i] || !y[i]) { set_error("%s: null argument (layer %d)", who, i); return HQQ_ERR_SHAPE; }
    if (ld_misaligned(B[i], lora_dtype) || ld_misaligned(y[i], dtype)) {
      set_error("%s: B and y must be aligned to their element size (layer %d)", who, i);
      return HQQ_ERR_ALIGN;
    }
  }
  const size_t need = ld_workspace_bytes(n_layers, r, M, K);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("%s: needs %zu bytes of 16-byte aligned workspace (got %zu)", who, need, workspace_bytes);
    return HQQ_ERR_WORKSPACE;
  }
  LdExpandGroup g;
  const float* area = static_cast<const float*>(workspace);
  int64_t max_n = 0;
  for (int i = 0; i < HQQ_GEMV_MAX_GROUP; ++i) {
    if (i >= n_layers) { g.l[i] = LdExpandMember{nullptr, nullptr, nullptr, 0.f, 1, 0, 0}; continue; }   // never selected: blockIdx.y < n_layers
    const int S = ld_slices(K, r[i]);
    g.l[i] = LdExpandMember{B[i], area, static_cast<uint16_t*>(y[i]), scaling[i], static_cast<int>(r[i]), static_cast<int>(N[i]), S};
    area += static_cast<size_t>(S) * M * r[i];
    if (N[i] > max_n) max_n = N[i];
  }
  hipStream_t st = as_stream(stream);
  const dim3 grid(static_cast<unsigned>((max_n + LD_EN - 1) / LD_EN), static_cast<unsigned>(n_layers));
  const int Mi = static_cast<int>(M);
#define HQQ_LD_EXPAND(MR, LDT, T) hipLaunchKernelGGL((lora_expand_kernel<MR, LDT, T>), grid, dim3(LD_THREADS), 0, st, g, Mi)
#define HQQ_LD_EXPAND_ROWS(LDT, T)                  \
  switch (ld_rows(M)) {                             \
    case 1: HQQ_LD_EXPAND(1, LDT, T); break;        \
    case 4: HQQ_LD_EXPAND(4, LDT, T); break;        \
    case 8: HQQ_LD_EXPAND(8, LDT, T); break;        \
    default: HQQ_LD_EXPAND(16, LDT, T); break;      \
  }
#define HQQ_LD_EXPAND_LDT(T) \
  if (lora_dtype == HQQ_F32) { HQQ_LD_EXPAND_ROWS(HQQ_F32, T) } else if (lora_dtype == HQQ_F16) { HQQ_LD_EXPAND_ROWS(HQQ_F16, T) } else { HQQ_LD_EXPAND_ROWS(HQQ_BF16, T) }
  if (dtype == HQQ_BF16) { HQQ_LD_EXPAND_LDT(bf16_t) } else { HQQ_LD_EXPAND_LDT(half_t) }
#undef HQQ_LD_EXPAND_LDT
#undef HQQ_LD_EXPAND_ROWS
#undef HQQ_LD_EXPAND
  return check_launch(who);
}

extern "C" int hqq_hip_lora_routed_covers(int n_layers, const int64_t* N, const int64_t* r, int64_t n_adapters, int64_t M, int64_t K, int dtype, int lora_dtype) {
  if (!N) { set_error("hqq_hip_lora_routed_covers: null argument"); return 0; }
  return ld_validate_routed("hqq_hip_lora_routed", n_layers, N, r, n_adapters, M, K, dtype, lora_dtype) == 0 ? 1 : 0;
}

extern "C" int hqq_hip_lora_shrink_routed(int n_layers, const void* x, const void* const* A_bank, const int64_t* r, int64_t n_adapters, const int64_t* slot_dev,
                                          int64_t M, int64_t K, int dtype, int lora_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "hqq_hip_lora_shrink_routed";
  if (const int rc = ld_validate_routed(who, n_layers, nullptr, r, n_adapters, M, K, dtype, lora_dtype)) return rc;
  clear_stale_error();
  if (!x || !A_bank || !slot_dev) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (!aligned16(x)) { set_error("%s: x must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  if (reinterpret_cast<uintptr_t>(slot_dev) & 7u) { set_error("%s: slot_dev must be 8-byte aligned", who); return HQQ_ERR_ALIGN; }
  for (int i = 0; i < n_layers; ++i) {
    if (!A_bank[i]) { set_error("%s: null argument (layer %d)", who, i); return HQQ_ERR_SHAPE; }
    if (ld_misaligned(A_bank[i], lora_dtype)) { set_error("%s: A_bank must be aligned to its element size (layer %d)", who, i); return HQQ_ERR_ALIGN; }
  }
  const size_t need = ld_workspace_bytes(n_layers, r, M, K);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("%s: needs %zu bytes of 16-byte aligned workspace (got %zu)", who, need, workspace_bytes);
    return HQQ_ERR_WORKSPACE;
  }
  LdShrinkGroup g;
  float* area = static_cast<float*>(workspace);
  int max_slices = 0;
  for (int i = 0; i < HQQ_GEMV_MAX_GROUP; ++i) {
    if (i >= n_layers) { g.l[i] = LdShrinkMember{nullptr, nullptr, 1, 1, 0, LD_KC, 0}; continue; }   // never selected: blockIdx.y < n_layers
    const int rj = ld_rj(r[i]), S = ld_slices(K, r[i]);
    int lg = 0;
    while ((1 << lg) < rj) ++lg;
    g.l[i] = LdShrinkMember{A_bank[i], area, static_cast<int>(r[i]), rj, lg, ld_kslice(r[i]), S};
    area += static_cast<size_t>(S) * M * r[i];
    if (S > max_slices) max_slices = S;
  }
  hipStream_t st = as_stream(stream);
  const dim3 grid(static_cast<unsigned>(max_slices), static_cast<unsigned>(n_layers), static_cast<unsigned>(M));   // z: the row whose adapter the workgroup serves
  const auto* xs = static_cast<const uint16_t*>(x);
  const int Mi = static_cast<int>(M), Ki = static_cast<int>(K), bf = dtype == HQQ_BF16 ? 1 : 0, na = static_cast<int>(n_adapters);
#define HQQ_LD_SHRINK(MR, LDT) hipLaunchKernelGGL((lora_shrink_routed_kernel<MR, LDT>), grid, dim3(LD_THREADS), 0, st, xs, g, slot_dev, na, Mi, Ki, bf)
#define HQQ_LD_SHRINK_ROWS(LDT)                     \
  switch (ld_rows(M)) {                             \
    case 1: HQQ_LD_SHRINK(1, LDT); break;           \
    case 4: HQQ_LD_SHRINK(4, LDT); break;           \
    case 8: HQQ_LD_SHRINK(8, LDT); break;           \
    default: HQQ_LD_SHRINK(16, LDT); break;         \
  }
  if (lora_dtype == HQQ_F32) { HQQ_LD_SHRINK_ROWS(HQQ_F32) } else if (lora_dtype == HQQ_F16) { HQQ_LD_SHRINK_ROWS(HQQ_F16) } else { HQQ_LD_SHRINK_ROWS(HQQ_BF16) }
#undef HQQ_LD_SHRINK_ROWS
#undef HQQ_LD_SHRINK
  return check_launch(who);
}

extern "C" int hqq_hip_lora_expand_routed(int n_layers, const void* workspace, size_t workspace_bytes, const void* const* B_bank, const float* const* scaling_dev,
                                          void* const* y, const int64_t* N, const int64_t* r, int64_t n_adapters, const int64_t* slot_dev, int64_t M, int64_t K,
                                          int dtype, int lora_dtype, void* stream) {
  const char* who = "hqq_hip_lora_expand_routed";
  if (!N) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (const int rc = ld_validate_routed(who, n_layers, N, r, n_adapters, M, K, dtype, lora_dtype)) return rc;
  clear_stale_error();
  if (!B_bank || !scaling_dev || !y || !slot_dev) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (reinterpret_cast<uintptr_t>(slot_dev) & 7u) { set_error("%s: slot_dev must be 8-byte aligned", who); return HQQ_ERR_ALIGN; }
  for (int i = 0; i < n_layers; ++i) {
    if (!B_bank[i] || !y[i] || !scaling_dev[i]) { set_error("%s: null argument (layer %d)", who, i); return HQQ_ERR_SHAPE; }
    if (ld_misaligned(B_bank[i], lora_dtype) || ld_misaligned(y[i], dtype) || ld_misaligned(scaling_dev[i], HQQ_F32)) {
      set_error("%s: B_bank, scaling_dev and y must be aligned to their element size (layer %d)", who, i);
      return HQQ_ERR_ALIGN;
    }
  }
  const size_t need = ld_workspace_bytes(n_layers, r, M, K);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("%s: needs %zu bytes of 16-byte aligned workspace (got %zu)", who, need, workspace_bytes);
    return HQQ_ERR_WORKSPACE;
  }
  LdExpandRoutedGroup g;
  const float* area = static_cast<const float*>(workspace);
  int64_t max_n = 0;
  for (int i = 0; i < HQQ_GEMV_MAX_GROUP; ++i) {
    if (i >= n_layers) { g.l[i] = LdExpandRoutedMember{nullptr, nullptr, nullptr, nullptr, 1, 0, 0}; continue; }   // never selected: blockIdx.y < n_layers
    const int S = ld_slices(K, r[i]);
    g.l[i] = LdExpandRoutedMember{B_bank[i], area, static_cast<uint16_t*>(y[i]), scaling_dev[i], static_cast<int>(r[i]), static_cast<int>(N[i]), S};
    area += static_cast<size_t>(S) * M * r[i];
    if (N[i] > max_n) max_n = N[i];
  }
  hipStream_t st = as_stream(stream);
  const dim3 grid(static_cast<unsigned>((max_n + LD_EN - 1) / LD_EN), static_cast<unsigned>(n_layers), static_cast<unsigned>(M));
  const int Mi = static_cast<int>(M), na = static_cast<int>(n_adapters);
#define HQQ_LD_EXPAND(MR, LDT, T) hipLaunchKernelGGL((lora_expand_routed_kernel<MR, LDT, T>), grid, dim3(LD_THREADS), 0, st, g, slot_dev, na, Mi)
#define HQQ_LD_EXPAND_ROWS(LDT, T)                  \
  switch (ld_rows(M)) {                             \
    case 1: HQQ_LD_EXPAND(1, LDT, T); break;        \
    case 4: HQQ_LD_EXPAND(4, LDT, T); break;        \
    case 8: HQQ_LD_EXPAND(8, LDT, T); break;        \
    default: HQQ_LD_EXPAND(16, LDT, T); break;      \
  }
#define HQQ_LD_EXPAND_LDT(T) \
  if (lora_dtype == HQQ_F32) { HQQ_LD_EXPAND_ROWS(HQQ_F32, T) } else if (lora_dtype == HQQ_F16) { HQQ_LD_EXPAND_ROWS(HQQ_F16, T) } else { HQQ_LD_EXPAND_ROWS(HQQ_BF16, T) }
  if (dtype == HQQ_BF16) { HQQ_LD_EXPAND_LDT(bf16_t) } else { HQQ_LD_EXPAND_LDT(half_t) }
#undef HQQ_LD_EXPAND_LDT
#undef HQQ_LD_EXPAND_ROWS
#undef HQQ_LD_EXPAND
  return check_launch(who);
}
