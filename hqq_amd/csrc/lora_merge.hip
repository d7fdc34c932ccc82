// lora_merge.hip — merge a LoRA adapter into a layer's weight (hqq_hip_lora_merge): out[N,K] = dequantize(Wq) + ((A @ B) * scaling)^T, fused
// unpack -> dequantize -> rank-r product -> add, one launch, gfx950.
//
// Replaces the chain HQQLinearLoRA.merge_and_quantize composes from torch ops (hqq/core/peft.py:167-190): a K x K identity pushed through the layer's
// forward for the base weight, a K x N fp32 A @ B, scaled, transposed, cast and added in place — about eight passes over N x K and an fp32 transient of
// that size.  Here the packed bytes, the meta and the two thin factors are read once and the merged weight is written once.
//
// Arithmetic (the contract of include/hqq_hip.h, restated by tests/_merge_cases.py): the base weight is the bits of hqq_hip_dequantize — the same
// Pk<NBITS>::level and CD<T>::dequant (unpack_common.h, hqq_common.h) —; the product is a plain fp32 sum over j = 0 .. r - 1 IN THAT ORDER of separately
// rounded products (no FMA: this file is built with contraction off; no MFMA, no atomics, no split over j), then rounded as the torch statements round:
// to the adapter's dtype (the matmul's result), times `scaling` and to the adapter's dtype again, to the compute dtype (.to(W.dtype)), and one more
// rounding for the add.  An output's bits therefore depend on its own row of B, its own row of A and its own base weight only.
//
// Work.  A workgroup of 256 threads owns the output tile (64 n, 128 k).  Lanes run along k: thread (tx = tid & 15, ty = tid >> 4) holds k0 + 8 tx .. + 7
// of the four rows n0 + ty + 16 i, 32 fp32 accumulators, and ends with one 16-byte store per row (a wave writes four 256-byte row segments).  A and B are
// staged through LDS in chunks of 32 j, converted to fp32 on the way, the accumulators stay in registers across chunks.  LDS layouts are chosen for the
// reads of the inner loop: As[j] keeps the first halves (4 k) of the 16 threads' runs side by side, then the second halves, so that each ds_read_b128 of
// a 16-lane group covers one 256-byte bank row; Bs[j] keeps a thread's four rows side by side (one ds_read_b128, the same address across a group: broadcast).
// The epilogue finds an element's container and meta from its flat index e = n K + k: slab e / n_p, container e % n_p; meta e / group_size (axis 1) or
// e % (N K / group_size) (axis 0) — one division per row and thread, then a walk; eight containers and their meta come in vector loads wherever the run
// stays inside one slab / one group and the addresses allow it.  Partial tiles: rows past N and columns past K are staged as zeros and never stored.
#include "unpack_common.h"

namespace hqq {

constexpr int LM_THREADS = 256;
constexpr int LM_TK = 128;              // k per tile: 8 per thread, 16 threads
constexpr int LM_TN = 64;               // n per tile: 4 per thread, 16 thread rows
constexpr int LM_JC = 32;               // j per LDS chunk
constexpr int LM_AS = LM_TK + 4;        // row stride of As in floats: 16-byte aligned rows, and the staging writes (lanes along j) spread over 8 banks
constexpr int LM_MAX_R = 256;

// adapter element -> fp32 (ldt is uniform over the launch)
static __device__ __forceinline__ float lm_load(const void* p, int64_t i, int ldt) {
  if (ldt == HQQ_F32) return static_cast<const float*>(p)[i];
  if (ldt == HQQ_F16) return static_cast<float>(static_cast<const half_t*>(p)[i]);
  return bf16_to_f32(static_cast<const uint16_t*>(p)[i]);
}
// round to the adapter's dtype and back
static __device__ __forceinline__ float lm_round(float v, int ldt) {
  if (ldt == HQQ_F32) return v;
  if (ldt == HQQ_F16) return static_cast<float>(static_cast<half_t>(v));
  return bf16_to_f32(f32_to_bf16(v));
}

template <typename T> static __device__ __forceinline__ uint16_t lm_bits(T v);
template <> __device__ __forceinline__ uint16_t lm_bits<half_t>(half_t v) { return __builtin_bit_cast(uint16_t, v); }
template <> __device__ __forceinline__ uint16_t lm_bits<bf16_t>(bf16_t v) { return v.v; }

static __device__ __forceinline__ bool lm_aligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

// q = e / d, rem = e % d; `small`: every flat index of the launch fits 32 bits
static __device__ __forceinline__ void lm_divmod(int64_t e, int64_t d, bool small, int64_t& q, int64_t& rem) {
  if (small) {
    const uint32_t qq = static_cast<uint32_t>(e) / static_cast<uint32_t>(d);
    q = qq;
    rem = static_cast<uint32_t>(e) - qq * static_cast<uint32_t>(d);
  } else {
    q = e / d;
    rem = e - q * d;
  }
}

// eight 16-bit values from p: one 16-byte load where the address allows it
template <typename T>
static __device__ __forceinline__ void lm_load8(const T* p, T (&v)[8]) {
  static_assert(sizeof(T) == 2, "16-bit compute dtypes");
  if (lm_aligned(p, 15)) {
    const u32x4 x = *reinterpret_cast<const u32x4*>(p);
    __builtin_memcpy(v, &x, 16);
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = p[c];
  }
}

// the base weights of flat elements e0 .. e0 + cnt - 1 (cnt <= 8; the rest of w is zero and unused).  NBITS == 0: a dense base in T
template <int NBITS, typename T>
static __device__ __forceinline__ void lm_base(const void* __restrict__ Wq, const T* __restrict__ scale, const T* __restrict__ zero, int64_t e0, int cnt,
                                               int axis, int64_t n_p, int64_t gs, int64_t R, bool small, T (&w)[8]) {
  if constexpr (NBITS == 0) {
    const T* W = static_cast<const T*>(Wq) + e0;
    if (cnt == 8) {
      lm_load8(W, w);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) w[c] = c < cnt ? W[c] : T{};
    }
  } else {
    using P = Pk<NBITS>;
    using CT = typename P::container_t;
    const CT* pk = static_cast<const CT*>(Wq);
    int64_t s, i, mi, mrem = 0;
    lm_divmod(e0, n_p, small, s, i);
    if (axis == 1) lm_divmod(e0, gs, small, mi, mrem);
    else { int64_t unused; lm_divmod(e0, R, small, unused, mi); }
    if (cnt == 8 && i + 8 <= n_p) {
      // the eight levels sit in eight consecutive containers, in the same field
      uint32_t lv[8];
      if constexpr (sizeof(CT) == 1) {
        if (lm_aligned(pk + i, 7)) {
          const u32x2 x = *reinterpret_cast<const u32x2*>(pk + i);
#pragma unroll
          for (int c = 0; c < 8; ++c) lv[c] = x[c >> 2] >> (8 * (c & 3));
        } else {
#pragma unroll
          for (int c = 0; c < 8; ++c) lv[c] = pk[i + c];
        }
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) lv[c] = pk[i + c];
      }
      const int sh = P::shift(static_cast<int>(s));
#pragma unroll
      for (int c = 0; c < 8; ++c) lv[c] = (lv[c] >> sh) & P::mask;
      if (axis == 1 && mrem + 8 <= gs) {          // one group
        const T z = zero[mi], sc = scale[mi];
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c] = CD<T>::dequant(static_cast<float>(lv[c]), z, sc);
        return;
      }
      if (axis == 0 && mi + 8 <= R) {             // eight consecutive groups
        T z[8], sc[8];
        lm_load8(zero + mi, z);
        lm_load8(scale + mi, sc);
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c] = CD<T>::dequant(static_cast<float>(lv[c]), z[c], sc[c]);
        return;
      }
      // the run crosses a group edge (axis 1) or the end of the meta row (axis 0): walk the meta
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        w[c] = CD<T>::dequant(static_cast<float>(lv[c]), zero[mi], scale[mi]);
        if (axis == 1) { if (++mrem == gs) { mrem = 0; ++mi; } }
        else if (++mi == R) mi = 0;
      }
      return;
    }
    // the general walk: a partial run, or one that crosses a slab edge
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < cnt) w[c] = CD<T>::dequant(static_cast<float>(P::level(pk[i], static_cast<int>(s))), zero[mi], scale[mi]);
      else w[c] = T{};
      if (c + 1 < cnt) {
        if (++i == n_p) { i = 0; ++s; }
        if (axis == 1) { if (++mrem == gs) { mrem = 0; ++mi; } }
        else if (++mi == R) mi = 0;
      }
    }
  }
}

template <int NBITS, typename T>
__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(const void* __restrict__ Wq, const T* __restrict__ scale, const T* __restrict__ zero,
                                                               const void* __restrict__ A, const void* __restrict__ B, float scaling,
                                                               T* __restrict__ out, int N, int K, int r, int ldt, int axis, int64_t n_p, int64_t gs,
                                                               int64_t R, int ktiles, int small, int vec_store) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float As[LM_JC][LM_AS];
  __shared__ __attribute__((aligned(16))) float Bs[LM_JC][LM_TN];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  // k tiles fastest: the workgroups in flight together share their rows of B
  const int k0 = static_cast<int>(blockIdx.x % ktiles) * LM_TK;
  const int n0 = static_cast<int>(blockIdx.x / ktiles) * LM_TN;

  float acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[i][c] = 0.f;

  for (int j0 = 0; j0 < r; j0 += LM_JC) {
    const int jc = r - j0 < LM_JC ? r - j0 : LM_JC;
    // A[k0 .. k0 + 127, j0 .. j0 + jc - 1], j fastest as in memory; column of k: (second half of its 8-run) * 64 + (run) * 4 + (k & 3)
    for (int q = tid; q < LM_TK * jc; q += LM_THREADS) {
      const int kk = jc == LM_JC ? q >> 5 : q / jc;
      const int jj = q - kk * jc;
      const int k = k0 + kk;
      As[jj][((kk >> 2) & 1) * 64 + (kk >> 3) * 4 + (kk & 3)] = k < K ? lm_load(A, static_cast<int64_t>(k) * r + j0 + jj, ldt) : 0.f;
    }
    // B[j0 .. j0 + jc - 1, n0 .. n0 + 63], n fastest; column of row n0 + ty + 16 i: 4 ty + i
    for (int q = tid; q < jc * LM_TN; q += LM_THREADS) {
      const int jj = q >> 6, nn = q & 63;
      const int n = n0 + nn;
      Bs[jj][(nn & 15) * 4 + (nn >> 4)] = n < N ? lm_load(B, static_cast<int64_t>(j0 + jj) * N + n, ldt) : 0.f;
    }
    __syncthreads();
    for (int jj = 0; jj < jc; ++jj) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(&As[jj][4 * tx]);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(&As[jj][64 + 4 * tx]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[jj][4 * ty]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float p0 = a0[c] * b[i];   // rounded on its own: contraction is off
          const float p1 = a1[c] * b[i];
          acc[i][c] = acc[i][c] + p0;
          acc[i][4 + c] = acc[i][4 + c] + p1;
        }
    }
    __syncthreads();
  }

  const int kb = k0 + 8 * tx;
  if (kb >= K) return;
  const int cnt = K - kb < 8 ? K - kb : 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty + 16 * i;
    if (n >= N) continue;
    const int64_t e0 = static_cast<int64_t>(n) * K + kb;
    T w[8];
    lm_base<NBITS, T>(Wq, scale, zero, e0, cnt, axis, n_p, gs, R, small != 0, w);
    uint16_t o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float m = lm_round(acc[i][c], ldt);             // the matmul's result in the adapter's dtype
      const float s = lm_round(m * scaling, ldt);           // * scaling, in the adapter's dtype
      const T d = CD<T>::from_f32(s);                       // .to(W.dtype)
      o[c] = lm_bits<T>(CD<T>::from_f32(CD<T>::to_f32(w[c]) + CD<T>::to_f32(d)));   // W += d
    }
    uint16_t* dst = reinterpret_cast<uint16_t*>(out) + e0;
    if (vec_store && cnt == 8) {
      u32x4 v;
      __builtin_memcpy(&v, o, 16);
      *reinterpret_cast<u32x4*>(dst) = v;
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < cnt) dst[c] = o[c];
    }
  }
}

// what the kernel covers, checked before anything is launched: 0, or an HQQ_ERR_* with the message set.  nbits == 0: the dense base
static int lm_validate(int nbits, int64_t N, int64_t K, int64_t group_size, int axis, int dtype, int lora_dtype, int64_t r) {
  const char* who = "hqq_hip_lora_merge";
  if (nbits != 0 && !per_of(nbits)) { set_error("%s: nbits=%d not in {8,4,3,2,1} (0: a dense base)", who, nbits); return HQQ_ERR_NBITS; }
  if (dtype == HQQ_F32) { set_error("%s: an fp32 compute dtype is not covered (fp16 / bf16)", who); return HQQ_ERR_UNSUPPORTED; }
  if (dtype != HQQ_F16 && dtype != HQQ_BF16) { set_error("%s: dtype %d", who, dtype); return HQQ_ERR_DTYPE; }
  if (lora_dtype != HQQ_F32 && lora_dtype != HQQ_F16 && lora_dtype != HQQ_BF16) { set_error("%s: adapter dtype %d", who, lora_dtype); return HQQ_ERR_DTYPE; }
  if (r < 1 || r > LM_MAX_R) { set_error("%s: rank %lld is not covered (1 .. %d)", who, (long long)r, LM_MAX_R); return HQQ_ERR_UNSUPPORTED; }
  if (N < 1 || K < 1) { set_error("%s: bad N / K (%lld x %lld)", who, (long long)N, (long long)K); return HQQ_ERR_SHAPE; }
  if (N > INT32_MAX || K > INT32_MAX || ((K + LM_TK - 1) / LM_TK) * ((N + LM_TN - 1) / LM_TN) > INT32_MAX) {
    set_error("%s: size overflow", who);
    return HQQ_ERR_SHAPE;
  }
  if (nbits == 0) return 0;
  // the packed base: what hqq_hip_dequantize accepts
  const int64_t total = N * K;
  if (group_size <= 0 || total % group_size || (axis != 0 && axis != 1)) {
    set_error("%s: N*K=%lld not divisible by group_size=%lld, or bad axis %d", who, (long long)total, (long long)group_size, axis);
    return HQQ_ERR_SHAPE;
  }
  const int64_t urows = (axis == 1) ? total / group_size : group_size;
  if (hqq_hip_packed_rows(nbits, urows) < 0) { set_error("%s: %lld unpacked rows not packable at %d bits", who, (long long)urows, nbits); return HQQ_ERR_SHAPE; }
  return 0;
}

template <int NBITS, typename T>
static void lm_launch(int grid, hipStream_t st, const void* Wq, const void* scale, const void* zero, const void* A, const void* B, float scaling, void* out,
                      int N, int K, int r, int ldt, int axis, int64_t n_p, int64_t gs, int64_t R, int ktiles, int small, int vec_store) {
  hipLaunchKernelGGL((lora_merge_kernel<NBITS, T>), dim3(grid), dim3(LM_THREADS), 0, st, Wq, static_cast<const T*>(scale), static_cast<const T*>(zero), A, B,
                     scaling, static_cast<T*>(out), N, K, r, ldt, axis, n_p, gs, R, ktiles, small, vec_store);
}

}  // namespace hqq

using namespace hqq;

extern "C" int hqq_hip_lora_merge_covers(int nbits, int64_t N, int64_t K, int64_t group_size, int axis, int dtype, int lora_dtype, int64_t r) {
  return lm_validate(nbits, N, K, group_size, axis, dtype, lora_dtype, r) == 0 ? 1 : 0;
}

extern "C" int hqq_hip_lora_merge(int nbits, const void* Wq, const void* scale, const void* zero, const void* A, const void* B, float scaling, void* out,
                                  int64_t N, int64_t K, int64_t group_size, int axis, int dtype, int lora_dtype, int64_t r, void* stream) {
  if (const int rc = lm_validate(nbits, N, K, group_size, axis, dtype, lora_dtype, r)) return rc;
  clear_stale_error();
  const char* who = "hqq_hip_lora_merge";
  if (!Wq || !A || !B || !out || (nbits != 0 && (!scale || !zero))) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  const uintptr_t lmask = lora_dtype == HQQ_F32 ? 3 : 1, wmask = nbits == 0 ? 1 : (nbits == 3 ? 3 : 0);
  auto misaligned = [](const void* p, uintptr_t mask) { return p && (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
  if (misaligned(A, lmask) || misaligned(B, lmask) || misaligned(Wq, wmask) || misaligned(scale, 1) || misaligned(zero, 1) || misaligned(out, 1)) {
    set_error("%s: pointers must be aligned to their element size", who);
    return HQQ_ERR_ALIGN;
  }
  const int64_t total = N * K;
  int64_t n_p = 1, gs = 1, R = 1;
  if (nbits != 0) {
    R = total / group_size;
    gs = group_size;
    const int64_t urows = (axis == 1) ? R : group_size, ucols = (axis == 1) ? group_size : R;
    n_p = hqq_hip_packed_rows(nbits, urows) * ucols;
  }
  const int ktiles = static_cast<int>((K + LM_TK - 1) / LM_TK);
  const int grid = static_cast<int>(ktiles * ((N + LM_TN - 1) / LM_TN));
  const int small = total <= static_cast<int64_t>(UINT32_MAX) ? 1 : 0;
  const int vec_store = (aligned16(out) && K % 8 == 0) ? 1 : 0;
  hipStream_t st = as_stream(stream);
#define HQQ_LM_LAUNCH(NB, T) \
  lm_launch<NB, T>(grid, st, Wq, scale, zero, A, B, scaling, out, static_cast<int>(N), static_cast<int>(K), static_cast<int>(r), lora_dtype, axis, n_p, gs, R, \
                   ktiles, small, vec_store)
#define HQQ_LM_BITS(T)                      \
  switch (nbits) {                          \
    case 0: HQQ_LM_LAUNCH(0, T); break;     \
    case 8: HQQ_LM_LAUNCH(8, T); break;     \
    case 4: HQQ_LM_LAUNCH(4, T); break;     \
    case 3: HQQ_LM_LAUNCH(3, T); break;     \
    case 2: HQQ_LM_LAUNCH(2, T); break;     \
    default: HQQ_LM_LAUNCH(1, T); break;    \
  }
  if (dtype == HQQ_BF16) { HQQ_LM_BITS(bf16_t) } else { HQQ_LM_BITS(half_t) }
#undef HQQ_LM_BITS
#undef HQQ_LM_LAUNCH
  return check_launch(who);
}
