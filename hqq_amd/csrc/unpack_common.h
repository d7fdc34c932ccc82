// unpack_common.h — the container layout of BitPack.pack_* (hqq/core/bitpack.py:14-144), shared by the kernels that read a level out of the reference's
// flat container: bitpack.hip (unpack / dequantize) and lora_merge.hip.  Together with CD<T>::dequant (hqq_common.h) this is the whole weight rebuild of
// hqq_hip_dequantize: level -> round_T(round_T(q - z) * s).
//
// Layout: the packed tensor is flat.  With n packed containers, slab s of the unpacked matrix is the flat range [s * n, (s + 1) * n), and container i
// holds unpacked elements {s * n + i}, slab 0 in its most significant field.
#pragma once
#include <type_traits>

#include "hqq_common.h"

namespace hqq {

template <int NBITS> struct Pk {
  static constexpr int per = (NBITS == 3) ? 10 : 8 / NBITS;
  static constexpr uint32_t mask = (NBITS == 8) ? 0xFFu : ((1u << NBITS) - 1u);
  using container_t = typename std::conditional<NBITS == 3, uint32_t, uint8_t>::type;   // 3-bit: ten levels in an int32
  // shift of slab s inside the container (slab 0 most significant)
  static __device__ __forceinline__ int shift(int s) { return (NBITS == 3) ? (27 - 3 * s) : NBITS * (per - 1 - s); }
  // the level of slab s in container w
  static __device__ __forceinline__ uint32_t level(uint32_t w, int s) { return (w >> shift(s)) & mask; }
};

}  // namespace hqq
