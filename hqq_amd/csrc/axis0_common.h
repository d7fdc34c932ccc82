// axis0_common.h — what the axis-0 kernels share (gemv_axis0.hip: 1..16 rows, gemm_axis0.hip: 17..256 rows): the argument checks, the bit-identical
// two-rounding weight rebuild, the MFMA pair per slab, and the split-order sum + finish of the reduce launches.  One definition, so that both kernels
// rebuild the bits of hqq_hip_dequantize(axis = 0) and finish an output the same way.
#pragma once
#include "decode_common.h"

namespace hqq {

constexpr int A0_KU = 64;               // k per unit: 16 per lane group

static __device__ __forceinline__ u32x4 ld16(const void* p) { return *reinterpret_cast<const u32x4*>(p); }
static __device__ __forceinline__ u32x4 ld16_nt(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }

// fp16: the 16 weights of slab SL of one packed 16-byte vector, (q - z) then * s per element, as two MFMA A operands
template <int NBITS, int SL>
__device__ __forceinline__ void rebuild_f16(const u32x4& w, const half2_t (&zz)[8], const half2_t (&ss)[8], h8_t& a0, h8_t& a1, uint32_t magic) {
  constexpr int sh = NBITS * (8 / NBITS - 1 - SL);
  constexpr float inv = 1.0f / static_cast<float>(1 << sh);
  const half2_t k1 = {static_cast<half_t>(inv), static_cast<half_t>(inv)};
  const half2_t k2 = {static_cast<half_t>(-1024.0f * inv), static_cast<half_t>(-1024.0f * inv)};
  half2_t q[8];
  uint32_t o[8];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    q[2 * d] = biased_levels<NBITS, SL>(w[d], magic);            // bytes (4d+0, 4d+2)
    q[2 * d + 1] = biased_levels<NBITS, SL>(w[d] >> 8, magic);   // bytes (4d+1, 4d+3)
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = __builtin_elementwise_fma(q[i], k1, k2);   // exact integer level
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = q[i] - zz[i];                               // rounding 1
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = __builtin_bit_cast(uint32_t, q[i] * ss[i]);   // rounding 2
  a0 = __builtin_bit_cast(h8_t, u32x4{o[0], o[1], o[2], o[3]});
  a1 = __builtin_bit_cast(h8_t, u32x4{o[4], o[5], o[6], o[7]});
}

// bf16: the same through fp32 (gfx950 has no packed bf16 arithmetic): q - z in fp32, rounded to bf16, times s (exact in fp32), rounded again
template <int NBITS, int SL>
__device__ __forceinline__ void rebuild_bf16(const u32x4& w, const uint32_t (&zz)[8], const uint32_t (&ss)[8], bf16x8_t& a0, bf16x8_t& a1) {
  constexpr int sh = NBITS * (8 / NBITS - 1 - SL);
  constexpr uint32_t mask = (NBITS == 8) ? 0xFFu : ((1u << NBITS) - 1u);
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int d = i >> 1, b0 = i & 1;                  // bytes (4d + b0, 4d + b0 + 2)
    const float q0 = static_cast<float>((w[d] >> (8 * b0 + sh)) & mask);
    const float q1 = static_cast<float>((w[d] >> (8 * b0 + 16 + sh)) & mask);
    const f32x2_t dq = {q0 - __uint_as_float(zz[i] << 16), q1 - __uint_as_float(zz[i] & 0xFFFF0000u)};
    const bf16x2_t dr = __builtin_convertvector(dq, bf16x2_t);                                           // rounding 1
    const uint32_t du = __builtin_bit_cast(uint32_t, dr);
    const f32x2_t pw = {__uint_as_float(du << 16) * __uint_as_float(ss[i] << 16),
                        __uint_as_float(du & 0xFFFF0000u) * __uint_as_float(ss[i] & 0xFFFF0000u)};   // exact: two 8-bit significands
    o[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(pw, bf16x2_t));                          // rounding 2
  }
  a0 = __builtin_bit_cast(bf16x8_t, u32x4{o[0], o[1], o[2], o[3]});
  a1 = __builtin_bit_cast(bf16x8_t, u32x4{o[4], o[5], o[6], o[7]});
}

// every slab of one packed 16-byte vector against the same meta and x: rebuild, then one MFMA pair per slab
template <int NBITS, int SL>
struct A0Slabs {
  static constexpr int PER = 8 / NBITS;
  static __device__ __forceinline__ void f16(const u32x4& w, const half2_t (&zz)[8], const half2_t (&ss)[8], const h8_t& b0, const h8_t& b1,
                                             f32x4 (&acc)[PER], uint32_t magic) {
    h8_t a0, a1;
    rebuild_f16<NBITS, SL>(w, zz, ss, a0, a1, magic);
    acc[SL] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0, acc[SL], 0, 0, 0);
    acc[SL] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, acc[SL], 0, 0, 0);
    if constexpr (SL + 1 < PER) A0Slabs<NBITS, SL + 1>::f16(w, zz, ss, b0, b1, acc, magic);
  }
  static __device__ __forceinline__ void bf16(const u32x4& w, const uint32_t (&zz)[8], const uint32_t (&ss)[8], const bf16x8_t& b0, const bf16x8_t& b1,
                                              f32x4 (&acc)[PER]) {
    bf16x8_t a0, a1;
    rebuild_bf16<NBITS, SL>(w, zz, ss, a0, a1);
    acc[SL] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[SL], 0, 0, 0);
    acc[SL] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[SL], 0, 0, 0);
    if constexpr (SL + 1 < PER) A0Slabs<NBITS, SL + 1>::bf16(w, zz, ss, b0, b1, acc);
  }
};

// the partial sums of output i over the splits, in split order.  The loads of eight splits are issued together (independent), then added in split
// order: a thread is one chain of dependent adds, not of dependent round trips to memory
static __device__ __forceinline__ float a0_sum_splits(const float* __restrict__ part, int64_t MN, int64_t i, int splits) {
  float s = 0.f;
  int c = 0;
  for (; c + 8 <= splits; c += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = part[(c + j) * MN + i];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; c < splits; ++c) s += part[c * MN + i];
  return s;
}

// round(s) (+ bias: `out += bias` on the rounded result, quantize.py:896-897), as raw bits of the compute dtype
template <bool BF16>
static __device__ __forceinline__ uint16_t a0_finish(float s, const uint16_t* __restrict__ bias, int n) {
  if constexpr (BF16) {
    uint16_t o = f32_to_bf16(s);
    if (bias) o = f32_to_bf16(bf16_to_f32(o) + bf16_to_f32(bias[n]));
    return o;
  } else {
    half_t o = static_cast<half_t>(s);
    if (bias) o = o + __builtin_bit_cast(half_t, bias[n]);
    return __builtin_bit_cast(uint16_t, o);
  }
}


// what an axis-0 kernel named `who` covers for min_m..max_m activation rows, checked before anything is launched: 0, or an HQQ_ERR_* with the message set.
// max_splits: the most K splits the kernel's plan gives (its fp32 partial sums, M N per split, stay within 32-bit offsets)
static inline int a0_validate_rows(const char* who, int min_m, int max_m, int max_splits, int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size,
                                   int dtype, uint32_t opts) {
  if (opts & ~HQQ_OPT_ALL) { set_error("%s: unknown option bits 0x%x", who, opts & ~HQQ_OPT_ALL); return HQQ_ERR_SHAPE; }
  if (nbits != 8 && nbits != 4 && nbits != 3 && nbits != 2 && nbits != 1) { set_error("%s: nbits=%d", who, nbits); return HQQ_ERR_NBITS; }
  if (nbits == 3) { set_error("%s: 3-bit containers are not covered", who); return HQQ_ERR_UNSUPPORTED; }
  if (dtype == HQQ_F32) { set_error("%s: fp32 is not covered (fp16 / bf16)", who); return HQQ_ERR_UNSUPPORTED; }
  if (dtype != HQQ_F16 && dtype != HQQ_BF16) { set_error("%s: dtype %d", who, dtype); return HQQ_ERR_DTYPE; }
  if (dtype == HQQ_BF16 && nbits != 4 && nbits != 2) { set_error("%s: bf16 with nbits=%d is not covered (4 / 2)", who, nbits); return HQQ_ERR_UNSUPPORTED; }
  if (M < 1 || N < 1 || K < 1 || group_size < 1) { set_error("%s: bad M/N/K/group_size", who); return HQQ_ERR_SHAPE; }
  if (M > max_m) { set_error("%s: M=%lld is not covered (at most %d rows)", who, (long long)M, max_m); return HQQ_ERR_UNSUPPORTED; }
  if (M < min_m) { set_error("%s: M=%lld is not covered (at least %d rows)", who, (long long)M, min_m); return HQQ_ERR_UNSUPPORTED; }
  if (group_size % 16 || N % group_size || K % A0_KU) {
    set_error("%s: not covered: needs group_size %% 16 == 0, N %% group_size == 0, K %% %d == 0 (N=%lld K=%lld gs=%lld)", who, A0_KU,
              (long long)N, (long long)K, (long long)group_size);
    return HQQ_ERR_UNSUPPORTED;
  }
  // (N / per) * K packed bytes and N K / gs meta elements per layer, M N fp32 partial sums per split: 32-bit offsets stay in range
  if (N > INT32_MAX || K > INT32_MAX || (N / (8 / nbits)) * K > static_cast<int64_t>(UINT32_MAX) || (N / group_size) * K > INT32_MAX ||
      M * N * max_splits > INT32_MAX) {
    set_error("%s: size overflow", who);
    return HQQ_ERR_SHAPE;
  }
  return 0;
}

}  // namespace hqq
