// moe_router.hip — the router of a mixture-of-experts block at decode sizes (include/hqq_hip.h, hqq_hip_moe_router): ONE launch for what
// MixtralTopKRouter / Qwen3MoeTopKRouter compute in five or six torch launches (F.linear, softmax, topk, sum, div, Qwen3-MoE's cast):
//     l[t, e] = fp32(rnd(x_t . W_e));  p = softmax(l) in fp32;  sel = the k largest l, descending, equal logits by ascending e;  w = p[sel] (/ their sum) (rounded to T)
// and it writes idx [T_, k] int64 and weights [T_, k] float32 — what hqq_hip_moe_gate_up / hqq_hip_moe_down (moe.hip) read — with no cast launch in between.
//
// One workgroup per row, RT_WAVES waves.  Phase 1: a wave takes RT_U experts at a time (e = wave + RT_WAVES u): lane `lane` walks the 16-byte chunks
// c = lane, lane + 64, ... of x_t and of each W_e, eight fused multiply-adds per chunk into ONE fp32 accumulator per expert (a product of two T values is exact
// in fp32, so each step rounds once), then wave_sum() — a balanced tree over the lanes.  The order of a logit's summation is a function of H alone: a row's
// result does not depend on T_, on the other rows, on E or on which wave computed it.  The logit is rounded to T and kept in LDS as fp32.
// Phase 2, wave 0 alone: lane `lane` holds the logits e = lane + 64 j (j < 4); max over the wave; exp(l - max) into LDS; the denominator is their sum in
// ASCENDING e, one addition after the other (every lane computes it from LDS broadcasts: no cross-lane step whose order could vary); k selection passes, each a
// wave-wide maximum over a 32-bit key (the order-preserving 16-bit image of the logit, then lowest id first) by DPP steps, as wave_sum().  No atomics, no workspace, nothing waits on another workgroup.
// A NaN logit compares as the largest (torch.topk's rule), NaNs among themselves by ascending id; -0 equals +0.
#include "block_math.h"
#include "decode_common.h"

namespace hqq {

constexpr int RT_WAVES = 16;
constexpr int RT_THREADS = 64 * RT_WAVES;
constexpr int RT_U = 4;          // experts a wave carries through one pass over x_t
constexpr int RT_MAX_T = 16;     // = moe.hip's MOE_MAX_T
constexpr int RT_MAX_K = 8;
constexpr int RT_MAX_E = 256;
constexpr int RT_SLOTS = RT_MAX_E / 64;   // logits per lane in phase 2
constexpr int64_t RT_MAX_H = 65536;

// the order the selection decides on, as 16 bits: NaN above everything, then descending order with -0 == +0.  The logit is a value of T, and T's sign-magnitude
// pattern orders like an unsigned integer once the sign is folded in
template <bool BF>
__device__ __forceinline__ uint32_t rt_order_key(float l) {
  if (l != l) return 0xFFFFu;
  if (l == 0.f) l = 0.f;   // -0 -> +0
  const uint32_t u = El<BF>::r(l);   // (exact: l came from a value of T)
  return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}

// f over the 64 lanes, the result in every lane (uniform: it comes back through SGPRs) — wave_sum()'s steps with another operation: four DPP steps inside
// each row of 16, then the four row results.  f is associative and commutative on what it is given here (an integer maximum; fmaxf without NaNs)
template <class F>
__device__ __forceinline__ int rt_wave_reduce(int v, F f) {
  auto step = [&](int x, auto ctrl) { return f(x, __builtin_amdgcn_update_dpp(0, x, decltype(ctrl)::value, 0xF, 0xF, true)); };
  v = step(v, std::integral_constant<int, 0xB1>{});    // quad_perm [1,0,3,2]
  v = step(v, std::integral_constant<int, 0x4E>{});    // quad_perm [2,3,0,1]
  v = step(v, std::integral_constant<int, 0x141>{});   // row_half_mirror
  v = step(v, std::integral_constant<int, 0x140>{});   // row_mirror
  const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16), r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
  return f(f(r0, r1), f(r2, r3));
}

__device__ __forceinline__ uint32_t rt_wave_max(uint32_t v) {
  return static_cast<uint32_t>(rt_wave_reduce(static_cast<int>(v), [](int a, int b) { return static_cast<int>(static_cast<uint32_t>(a) > static_cast<uint32_t>(b) ? a : b); }));
}

__device__ __forceinline__ float rt_wave_fmax(float v) {
  return __builtin_bit_cast(float, rt_wave_reduce(__builtin_bit_cast(int, v), [](int a, int b) {
    return __builtin_bit_cast(int, fmaxf(__builtin_bit_cast(float, a), __builtin_bit_cast(float, b)));
  }));
}

template <bool BF>
__global__ __launch_bounds__(RT_THREADS) void moe_router_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ W, int64_t* __restrict__ idx,
                                                                float* __restrict__ wts, uint16_t* __restrict__ logits, int k, int E, int H, int renorm,
                                                                int round_w) {
  using El_ = El<BF>;
  __shared__ __attribute__((aligned(16))) float lg[RT_MAX_E];   // the logits, rounded to T, as fp32
  __shared__ __attribute__((aligned(16))) float ex[RT_MAX_E];   // exp(l - max)
  const int t = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const uint16_t* xr = x + static_cast<size_t>(t) * H;
  const int nchunks = H >> 3;
  for (int e0 = wave; e0 < E; e0 += RT_WAVES * RT_U) {   // (wave-uniform)
    const uint16_t* wr[RT_U];
    float acc[RT_U];
#pragma unroll
    for (int u = 0; u < RT_U; ++u) {
      const int e = e0 + RT_WAVES * u;
      wr[u] = W + static_cast<size_t>(e < E ? e : e0) * H;   // a pass's spare slots read expert e0 again; their sums are dropped
      acc[u] = 0.f;
    }
    for (int c = lane; c < nchunks; c += 64) {
      const size_t k0 = static_cast<size_t>(c) << 3;
      const u32x4 xv = *reinterpret_cast<const u32x4*>(xr + k0);
      u32x4 wv[RT_U];
#pragma unroll
      for (int u = 0; u < RT_U; ++u) wv[u] = *reinterpret_cast<const u32x4*>(wr[u] + k0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = El_::f(static_cast<uint16_t>(xv[j] & 0xFFFFu)), x1 = El_::f(static_cast<uint16_t>(xv[j] >> 16));
#pragma unroll
        for (int u = 0; u < RT_U; ++u) {
          acc[u] = __builtin_fmaf(x0, El_::f(static_cast<uint16_t>(wv[u][j] & 0xFFFFu)), acc[u]);
          acc[u] = __builtin_fmaf(x1, El_::f(static_cast<uint16_t>(wv[u][j] >> 16)), acc[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RT_U; ++u) {
      const float s = wave_sum(acc[u]);
      const int e = e0 + RT_WAVES * u;
      if (lane == 0 && e < E) {
        const uint16_t r = El_::r(s);
        lg[e] = El_::f(r);
        if (logits) logits[static_cast<size_t>(t) * E + e] = r;
      }
    }
  }
  __syncthreads();
  if (wave == 0) {   // (no barrier below this line)
    float l[RT_SLOTS];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < RT_SLOTS; ++j) {
      const int e = lane + 64 * j;
      l[j] = e < E ? lg[e] : -INFINITY;
      m = fmaxf(m, l[j]);   // (a NaN is passed over here and comes back through exp: the whole row's weights are NaN, as torch's softmax gives)
    }
    m = rt_wave_fmax(m);
#pragma unroll
    for (int j = 0; j < RT_SLOTS; ++j) {
      const int e = lane + 64 * j;
      if (e < E) ex[e] = expf(l[j] - m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    float den = 0.f;
    for (int e = 0; e < E; ++e) den += ex[e];   // ascending e, the same in every lane
    uint32_t key[RT_SLOTS];
#pragma unroll
    for (int j = 0; j < RT_SLOTS; ++j) {
      const int e = lane + 64 * j;
      key[j] = e < E ? (rt_order_key<BF>(l[j]) << 16) | static_cast<uint32_t>(1023 - e) : 0u;   // 0: no candidate
    }
    int sel_e = 0;      // lane s keeps slot s
    float sel_p = 0.f;
    float p[RT_MAX_K];
#pragma unroll
    for (int s = 0; s < RT_MAX_K; ++s) {
      p[s] = 0.f;
      if (s < k) {   // (uniform)
        uint32_t best = key[0];
#pragma unroll
        for (int j = 1; j < RT_SLOTS; ++j) best = key[j] > best ? key[j] : best;
        best = rt_wave_max(best);
        const int e = (1023 - static_cast<int>(best & 0xFFFFu)) & (RT_MAX_E - 1);   // k <= E: a candidate is left (the mask keeps the LDS read inside ex[] whatever happens)
#pragma unroll
        for (int j = 0; j < RT_SLOTS; ++j)
          if (lane + 64 * j == e) key[j] = 0u;
        p[s] = ex[e] / den;
        if (lane == s) sel_e = e;
      }
    }
    if (renorm) {
      float sum = 0.f;
#pragma unroll
      for (int s = 0; s < RT_MAX_K; ++s)
        if (s < k) sum += p[s];   // s ascending
#pragma unroll
      for (int s = 0; s < RT_MAX_K; ++s) p[s] = p[s] / sum;
    }
#pragma unroll
    for (int s = 0; s < RT_MAX_K; ++s)
      if (lane == s) sel_p = p[s];
    if (round_w) sel_p = El_::f(El_::r(sel_p));
    if (lane < k) {
      idx[static_cast<size_t>(t) * k + lane] = sel_e;
      wts[static_cast<size_t>(t) * k + lane] = sel_p;
    }
  }
}

static int router_validate(const char* who, int64_t T, int64_t k, int64_t E, int64_t H, int dtype) {
  if (dtype == HQQ_F32) { set_error("%s: fp32 activations are not covered (fp16 / bf16)", who); return HQQ_ERR_UNSUPPORTED; }
  if (dtype != HQQ_F16 && dtype != HQQ_BF16) { set_error("%s: dtype %d", who, dtype); return HQQ_ERR_DTYPE; }
  if (T < 1 || T > RT_MAX_T) { set_error("%s: %lld rows are not covered (1 .. %d)", who, (long long)T, RT_MAX_T); return HQQ_ERR_UNSUPPORTED; }
  if (k < 1 || k > RT_MAX_K) { set_error("%s: %lld experts per token are not covered (1 .. %d)", who, (long long)k, RT_MAX_K); return HQQ_ERR_UNSUPPORTED; }
  if (E < k || E > RT_MAX_E) { set_error("%s: %lld experts are not covered (k = %lld .. %d)", who, (long long)E, (long long)k, RT_MAX_E); return HQQ_ERR_UNSUPPORTED; }
  if (H < 8 || H % 8 || H > RT_MAX_H) { set_error("%s: H=%lld is not covered (a multiple of 8, 8 .. %lld)", who, (long long)H, (long long)RT_MAX_H); return HQQ_ERR_UNSUPPORTED; }
  return 0;
}

}  // namespace hqq

using namespace hqq;

extern "C" int hqq_hip_moe_router_covers(int64_t T, int64_t k, int64_t E, int64_t H, int dtype) {
  return router_validate("hqq_hip_moe_router", T, k, E, H, dtype) == 0 ? 1 : 0;
}

extern "C" int hqq_hip_moe_router(const void* x, const void* W, void* idx, void* weights, void* logits, int64_t T, int64_t k, int64_t E, int64_t H, int renorm,
                                  int round_weights, int dtype, void* stream) {
  const char* who = "hqq_hip_moe_router";
  if (const int rc = router_validate(who, T, k, E, H, dtype)) return rc;
  clear_stale_error();
  if (!x || !W || !idx || !weights) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (!aligned16(x) || !aligned16(W)) { set_error("%s: x and W must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  if ((reinterpret_cast<uintptr_t>(idx) & 7u) || (reinterpret_cast<uintptr_t>(weights) & 3u) || (reinterpret_cast<uintptr_t>(logits) & 1u)) {
    set_error("%s: idx, weights and logits must be aligned to their element size", who);
    return HQQ_ERR_ALIGN;
  }
  hipStream_t st = as_stream(stream);
#define HQQ_MOE_RT(BF)                                                                                                                                  \
  hipLaunchKernelGGL((moe_router_kernel<BF>), dim3(static_cast<unsigned>(T)), dim3(RT_THREADS), 0, st, static_cast<const uint16_t*>(x),                   \
                     static_cast<const uint16_t*>(W), static_cast<int64_t*>(idx), static_cast<float*>(weights), static_cast<uint16_t*>(logits),          \
                     static_cast<int>(k), static_cast<int>(E), static_cast<int>(H), renorm ? 1 : 0, round_weights ? 1 : 0)
  if (dtype == HQQ_BF16) HQQ_MOE_RT(true); else HQQ_MOE_RT(false);
#undef HQQ_MOE_RT
  return check_launch(who);
}
