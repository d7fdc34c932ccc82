// kv_load.h — what every reader of the quantised KV cache shares (format: the head of kv_cache.hip): the rebuild of a lane's 8 dims of a stored row to T, the cache
// as a row source of the tile attention (attn_tile_core.h), its one coverage rule and its dispatch.  Translation units that use kv_load8 are compiled with
// -ffp-contract=off: CD<T>::dequant's two roundings stay separate.
#pragma once
#include "hqq_common.h"
#include "block_math.h"
#include "attn_decode_core.h"

namespace hqq {

// ---- a lane's 8 dims of a stored row, rebuilt to T: the packed bytes (4 bits: lanes ch and ch + LPK / 2 read the SAME 8 bytes, high / low nibbles),
//      the group's scale and zero, CD<T>::dequant ----
template <int HD, int NBITS, bool BF>
__device__ __forceinline__ u32x4 kv_load8(const uint8_t* __restrict__ qrow, const uint16_t* __restrict__ srow, const uint16_t* __restrict__ zrow, int ch, int gs_shift) {
  constexpr int LPK = HD / 8;
  uint32_t b0, b1;
  int sh = 0;
  uint32_t mask = 0xFFu;
  if constexpr (NBITS == 8) {
    const u32x2 b = *reinterpret_cast<const u32x2*>(qrow + ch * 8);
    b0 = b[0]; b1 = b[1];
  } else {
    const bool low = ch >= LPK / 2;
    const u32x2 b = *reinterpret_cast<const u32x2*>(qrow + (low ? ch - LPK / 2 : ch) * 8);
    b0 = b[0]; b1 = b[1];
    sh = low ? 0 : 4;
    mask = 0xFu;
  }
  const int g = (ch * 8) >> gs_shift;
  const uint16_t s = srow[g], z = zrow[g];
  if constexpr (!BF && NBITS == 4) {
    // fp16 nibbles, two dims per instruction: 0x6400 | q is the half 1024 + q (q < 1024), and (1024 + q) - 1024 is exact, so the pair (half(q_lo), half(q_hi)) costs one
    // byte shuffle and one packed subtraction instead of two bit-field extracts and two integer-to-float-to-half conversions; then CD<half_t>::dequant's two roundings
    // as packed half operations (v_pk_add_f16 / v_pk_mul_f16 round as their scalar forms do): the same bits.  Measured (tools/kvq_bench.py, B = 16, 16384 positions):
    // 432 us against 519 for the scalar form.  At 8 bits the scalar form stays: a byte converts in ONE instruction (v_cvt_f32_ubyteN), and the packed form measured slower
    // there (489 us against 464)
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const uint32_t t0 = (b0 >> sh) & (mask * 0x01010101u), t1 = (b1 >> sh) & (mask * 0x01010101u);   // a level per byte
    const h2 k1024 = {static_cast<_Float16>(1024.f), static_cast<_Float16>(1024.f)};
    const _Float16 zh = __builtin_bit_cast(_Float16, z), sh_ = __builtin_bit_cast(_Float16, s);
    const h2 z2 = {zh, zh}, s2 = {sh_, sh_};
    u32x4 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t w = (e < 2 ? t0 : t1) >> (16 * (e & 1));
      const uint32_t pair = (w & 0xFFu) | ((w & 0xFF00u) << 8) | 0x64006400u;
      const h2 qh = __builtin_bit_cast(h2, pair) - k1024;
      const h2 d = qh - z2;
      const h2 r = d * s2;
      out[e] = __builtin_bit_cast(uint32_t, r);
    }
    return out;
  }
  uint16_t o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t w = e < 4 ? b0 : b1;
    const float q = static_cast<float>((w >> (8 * (e & 3) + sh)) & mask);
    if constexpr (BF) o[e] = CD<bf16_t>::dequant(q, bf16_t{z}, bf16_t{s}).v;
    else o[e] = __builtin_bit_cast(uint16_t, CD<half_t>::dequant(q, __builtin_bit_cast(half_t, z), __builtin_bit_cast(half_t, s)));
  }
  u32x4 out;
#pragma unroll
  for (int e = 0; e < 4; ++e) out[e] = static_cast<uint32_t>(o[2 * e]) | (static_cast<uint32_t>(o[2 * e + 1]) << 16);
  return out;
}

// ---- the six buffers as a row source of the tile family (attn_tile_core.h states what a source is): row j of a (sequence, KV head) rebuilt to T as it is loaded.
//      The row index is widened signed, the code these kernels always had (kv_cache.hip's widen_t was tuned for the one-row kernels) ----
template <int HD, int NBITS, bool BF>
struct PackedKV {
  const uint8_t* kq;
  const uint16_t* ks;
  const uint16_t* kz;
  const uint8_t* vq;
  const uint16_t* vs;
  const uint16_t* vz;
  int gs_shift;
  static constexpr int RB = HD * NBITS / 8;   // bytes of levels per row
  struct Rows {
    const uint8_t* kq;
    const uint16_t* ks;
    const uint16_t* kz;
    const uint8_t* vq;
    const uint16_t* vs;
    const uint16_t* vz;
    int NG, gs_shift;   // NG: (scale, zero) pairs per row
    __device__ __forceinline__ u32x4 k(int ch, int j) const {
      const int64_t r = j;
      return kv_load8<HD, NBITS, BF>(kq + r * RB, ks + r * NG, kz + r * NG, ch, gs_shift);
    }
    __device__ __forceinline__ u32x4 v(int ch, int j) const {
      const int64_t r = j;
      return kv_load8<HD, NBITS, BF>(vq + r * RB, vs + r * NG, vz + r * NG, ch, gs_shift);
    }
  };
  __device__ __forceinline__ Rows at(int64_t r0) const {
    const int NG = HD >> gs_shift;
    return Rows{kq + r0 * RB, ks + r0 * NG, kz + r0 * NG, vq + r0 * RB, vs + r0 * NG, vz + r0 * NG, NG, gs_shift};
  }
  // an entry point's six buffers and group size (32 / 64: kv_check) as the source
  static PackedKV of(const void* kq, const void* ks, const void* kz, const void* vq, const void* vs, const void* vz, int64_t group_size) {
    using u8 = const uint8_t*;
    using u16 = const uint16_t*;
    return PackedKV{static_cast<u8>(kq), static_cast<u16>(ks), static_cast<u16>(kz), static_cast<u8>(vq), static_cast<u16>(vs), static_cast<u16>(vz), group_size == 64 ? 6 : 5};
  }
};

// the one coverage rule of the quantised cache (hqq_hip_kv_covers); 0 where covered, else the error code with `who`'s message
static inline int kv_check(const char* who, int nbits, int64_t head_dim, int64_t group_size, int64_t cache_len, int dtype) {
  if (dtype != HQQ_F16 && dtype != HQQ_BF16) { set_error("%s: not covered: fp16 / bf16 only (dtype %d)", who, dtype); return HQQ_ERR_UNSUPPORTED; }
  if (nbits != 8 && nbits != 4) { set_error("%s: not covered: nbits %d (8 / 4)", who, nbits); return HQQ_ERR_UNSUPPORTED; }
  if (head_dim != 64 && head_dim != 128 && head_dim != 256) { set_error("%s: not covered: head_dim %lld (64 / 128 / 256)", who, (long long)head_dim); return HQQ_ERR_UNSUPPORTED; }
  if ((group_size != 32 && group_size != 64) || head_dim % group_size || (nbits == 4 && 2 * group_size > head_dim)) {
    set_error("%s: not covered: group_size %lld (32 / 64 dividing head_dim, 2 * group_size <= head_dim at 4 bits)", who, (long long)group_size);
    return HQQ_ERR_UNSUPPORTED;
  }
  if (cache_len < 1 || cache_len > 30000) { set_error("%s: not covered: cache_len %lld outside [1, 30000]", who, (long long)cache_len); return HQQ_ERR_UNSUPPORTED; }
  return 0;
}

// f(HD, NBITS, BF) as integral constants, for a covered head_dim and width
template <class F>
static inline void kv_dispatch(int64_t hd, int nbits, bool bf, F&& f) {
  attn_dispatch(hd, bf, [&](auto HDc, auto BFc) { if (nbits == 8) f(HDc, std::integral_constant<int, 8>{}, BFc); else f(HDc, std::integral_constant<int, 4>{}, BFc); });
}

}  // namespace hqq
