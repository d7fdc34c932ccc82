// moe.hip — the routed expert MLP of a mixture-of-experts block at decode sizes (include/hqq_hip.h, hqq_hip_moe_*): two launches for
//     out[t] = sum over the token's slots of w[t, s] * down_e(silu(gate_e(x_t)) * up_e(x_t)),   e = idx[t, s]
// over expert stacks quantised along axis 1 (core/moe.py HQQExperts: one dense buffer per role and kind, expert-major).  Only the packed bytes of
// the SELECTED experts are read: the expert id comes from device memory, the kernel forms base + e * stride itself — no host read, no host loop.
//
// Work items.  A packed output row pn of a [N, K] layer is K consecutive bytes that hold the levels of the `per` output rows pn + S * N / per
// (slab S, slab 0 most significant: the BitPack layout).  One wave per
//     gate_up:  (packed row of gate AND up, token, slot)   -> a[t, s, n_S] = silu_mul_el(rnd(x . Wg[n_S]), rnd(x . Wu[n_S]))
//     down:     (packed row of down, token)                -> walks the token's slots in ascending (expert id, slot) and combines in the epilogue
// A lane takes 16-byte chunks (16 k-values x per rows) c = lane, lane + 64, ...; its fp32 partial sums are added over the wave by wave_sum().  The
// order of a row's summation is a function of K alone: a token's result does not depend on T or on the other tokens.
// Weights are rebuilt with CD<T>::dequant — the function the dequantise kernel itself calls (bitpack.hip): the same two roundings, the same bits,
// whatever the zero-points and scales are (no hqq_hip_meta_check premise).  The MFMA rebuilds of decode_common.h would lift the VALU ceiling this
// scalar form has; profiles/moe_summary.md has what it reaches.
//
// Grid order: blockIdx.x walks the packed rows, blockIdx.y the (token, slot) pairs / the tokens.  Tokens that share an expert are NOT grouped: their
// waves rebuild the same weights again (the bytes come from L2 / the memory-side cache when the waves run close together).  The alternative — a wave per
// (packed row, expert) that finds its pairs with ballots over idx, rebuilds a chunk once for up to four pairs, and a down launch that walks the experts in
// ascending id with lane t holding token t's sum — was built and measured slower at every point but Mixtral's same-experts routing from 4 tokens on
// (profiles/moe_grouping_ab.md): it gives up the parallelism over tokens that the down launch needs.  Not taken.
#include "block_math.h"
#include "decode_common.h"

namespace hqq {

constexpr int MOE_WAVES = 4;   // waves (packed rows) per workgroup
constexpr int MOE_THREADS = 64 * MOE_WAVES;
constexpr int MOE_MAX_T = 16;
constexpr int MOE_MAX_K = 8;
constexpr int MOE_MAX_E = 256;
constexpr int64_t MOE_MAX_DIM = 65536;

struct MoeLayer {          // one role's stacks
  const uint8_t* Wq;       // [E][N K / per] bytes
  const uint16_t* scale;   // [E][N K / gs]
  const uint16_t* zero;    // [E][N K / gs]
};

template <bool BF> struct MoeT { using type = half_t; };
template <> struct MoeT<true> { using type = bf16_t; };

template <bool BF>
__device__ __forceinline__ typename MoeT<BF>::type moe_raw(uint16_t v) {
  if constexpr (BF) return bf16_t{v};
  else return __builtin_bit_cast(half_t, v);
}

// this lane's fp32 partial sums of the `per` rows of one packed row (K bytes at Wrow; the constants of slab S, group g at sc / ze[S * slab_stride + g])
// against the K activations at xr
template <int NBITS, bool BF>
__device__ __forceinline__ void moe_row_dot(const uint8_t* __restrict__ Wrow, const uint16_t* __restrict__ sc, const uint16_t* __restrict__ ze,
                                            const uint16_t* __restrict__ xr, int K, int gs, size_t slab_stride, int lane, float (&acc)[8 / NBITS]) {
  constexpr int PER = 8 / NBITS;
  constexpr uint32_t MASK = (1u << NBITS) - 1u;
  using T = typename MoeT<BF>::type;
  const int nchunks = K >> 4;
  for (int c = lane; c < nchunks; c += 64) {
    const size_t k0 = static_cast<size_t>(c) << 4;
    const u32x4 wv = *reinterpret_cast<const u32x4*>(Wrow + k0);
    const u32x4 x0 = *reinterpret_cast<const u32x4*>(xr + k0);
    const u32x4 x1 = *reinterpret_cast<const u32x4*>(xr + k0 + 8);
    const int g = static_cast<int>(k0) / gs;   // (gs % 16 == 0: a chunk lies inside one group)
    float xf[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xf[2 * j] = El<BF>::f(static_cast<uint16_t>(x0[j] & 0xFFFFu));
      xf[2 * j + 1] = El<BF>::f(static_cast<uint16_t>(x0[j] >> 16));
      xf[8 + 2 * j] = El<BF>::f(static_cast<uint16_t>(x1[j] & 0xFFFFu));
      xf[8 + 2 * j + 1] = El<BF>::f(static_cast<uint16_t>(x1[j] >> 16));
    }
#pragma unroll
    for (int S = 0; S < PER; ++S) {
      const int sh = NBITS * (PER - 1 - S);
      const T z = moe_raw<BF>(ze[S * slab_stride + g]);
      const T s = moe_raw<BF>(sc[S * slab_stride + g]);
      float a = acc[S];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t q = (wv[j >> 2] >> (8 * (j & 3) + sh)) & MASK;
        const float w = CD<T>::to_f32(CD<T>::dequant(static_cast<float>(q), z, s));
        a = __builtin_fmaf(xf[j], w, a);
      }
      acc[S] = a;
    }
  }
}

// a[t, s, n] for the `per` rows of one packed row of gate and of up.  grid (ceil(I / per / MOE_WAVES), T * k)
template <int NBITS, bool BF>
__global__ __launch_bounds__(MOE_THREADS) void moe_gate_up_kernel(const uint16_t* __restrict__ x, const int64_t* __restrict__ idx, MoeLayer gate, MoeLayer up,
                                                                  uint16_t* __restrict__ a, int kslots, int E, int H, int I, int gs) {
  constexpr int PER = 8 / NBITS;
  const int lane = threadIdx.x & 63;
  const int NP = I / PER;   // packed rows of one expert
  const int pn = blockIdx.x * MOE_WAVES + (threadIdx.x >> 6);
  if (pn >= NP) return;
  const int pair = blockIdx.y;   // t * k + s
  const int64_t e = idx[pair];
  if (e < 0 || e >= E) return;   // nothing read, nothing written: hqq_hip_moe_down skips the slot as well
  const int t = pair / kslots;
  const int G = H / gs;
  const size_t wo = static_cast<size_t>(e) * (static_cast<size_t>(I) * H / PER) + static_cast<size_t>(pn) * H;
  const size_t mo = static_cast<size_t>(e) * (static_cast<size_t>(I) * G) + static_cast<size_t>(pn) * G;
  const size_t slab = static_cast<size_t>(NP) * G;   // slab S holds row pn + S * NP: its constants are S * NP * G further on
  const uint16_t* xr = x + static_cast<size_t>(t) * H;
  float ag[PER], au[PER];
#pragma unroll
  for (int S = 0; S < PER; ++S) { ag[S] = 0.f; au[S] = 0.f; }
  moe_row_dot<NBITS, BF>(gate.Wq + wo, gate.scale + mo, gate.zero + mo, xr, H, gs, slab, lane, ag);
  moe_row_dot<NBITS, BF>(up.Wq + wo, up.scale + mo, up.zero + mo, xr, H, gs, slab, lane, au);
#pragma unroll
  for (int S = 0; S < PER; ++S) { ag[S] = wave_sum(ag[S]); au[S] = wave_sum(au[S]); }
  if (lane == 0) {
    uint16_t* ar = a + static_cast<size_t>(pair) * I;
#pragma unroll
    for (int S = 0; S < PER; ++S) ar[pn + S * NP] = silu_mul_el<BF>(El<BF>::r(ag[S]), El<BF>::r(au[S]));
  }
}

// out[t, n] for the `per` rows of one packed row of down: the token's slots in ascending (expert id, slot), combined as HF's loop over the experts hit
// and its index_add_ combine them.  grid (ceil(H / per / MOE_WAVES), T)
template <int NBITS, bool BF>
__global__ __launch_bounds__(MOE_THREADS) void moe_down_kernel(const uint16_t* __restrict__ a, const int64_t* __restrict__ idx, const float* __restrict__ rw,
                                                               MoeLayer down, uint16_t* __restrict__ out, int kslots, int E, int H, int I, int gs) {
  constexpr int PER = 8 / NBITS;
  using El_ = El<BF>;
  const int lane = threadIdx.x & 63;
  const int NP = H / PER;
  const int pn = blockIdx.x * MOE_WAVES + (threadIdx.x >> 6);
  if (pn >= NP) return;
  const int t = blockIdx.y;
  const int G = I / gs;
  const size_t slab = static_cast<size_t>(NP) * G;
  // key of slot s: e * MOE_MAX_K + s for a valid id (ascending key = ascending expert, ties by ascending slot); -1: skipped
  int key[MOE_MAX_K];
#pragma unroll
  for (int s = 0; s < MOE_MAX_K; ++s) {
    key[s] = -1;
    if (s < kslots) {
      const int64_t e = idx[t * kslots + s];
      if (e >= 0 && e < E) key[s] = static_cast<int>(e) * MOE_MAX_K + s;
    }
  }
  uint16_t res[PER];
#pragma unroll
  for (int S = 0; S < PER; ++S) res[S] = 0;   // torch.zeros_like
  int prev = -1;
  for (int rank = 0; rank < kslots; ++rank) {
    int cur = 0x7FFFFFFF;
#pragma unroll
    for (int s = 0; s < MOE_MAX_K; ++s)
      if (key[s] > prev && key[s] < cur) cur = key[s];
    if (cur == 0x7FFFFFFF) break;   // (fewer valid slots than k)
    prev = cur;
    const int e = cur / MOE_MAX_K, s = cur % MOE_MAX_K;
    const size_t wo = static_cast<size_t>(e) * (static_cast<size_t>(H) * I / PER) + static_cast<size_t>(pn) * I;
    const size_t mo = static_cast<size_t>(e) * (static_cast<size_t>(H) * G) + static_cast<size_t>(pn) * G;
    float acc[PER];
#pragma unroll
    for (int S = 0; S < PER; ++S) acc[S] = 0.f;
    moe_row_dot<NBITS, BF>(down.Wq + wo, down.scale + mo, down.zero + mo, a + static_cast<size_t>(t * kslots + s) * I, I, gs, slab, lane, acc);
    const float w = rw[t * kslots + s];
#pragma unroll
    for (int S = 0; S < PER; ++S) {
      const uint16_t d = El_::r(wave_sum(acc[S]));                  // F.linear's output, in T
      res[S] = El_::add(res[S], El_::r_prod(El_::f(d), w));          // (d * w) is an fp32 value, .to(T) rounds it, index_add_ adds in T
    }
  }
  if (lane == 0) {
    uint16_t* orow = out + static_cast<size_t>(t) * H;
#pragma unroll
    for (int S = 0; S < PER; ++S) orow[pn + S * NP] = res[S];
  }
}

static int moe_validate(const char* who, int nbits, int64_t T, int64_t k, int64_t E, int64_t H, int64_t I, int64_t gs, int dtype) {
  if (nbits != 8 && nbits != 4 && nbits != 3 && nbits != 2 && nbits != 1) { set_error("%s: nbits=%d not in {8,4,3,2,1}", who, nbits); return HQQ_ERR_NBITS; }
  if (nbits != 4 && nbits != 2) { set_error("%s: %d-bit experts are not covered (4 and 2)", who, nbits); return HQQ_ERR_UNSUPPORTED; }
  if (dtype == HQQ_F32) { set_error("%s: fp32 activations are not covered (fp16 / bf16)", who); return HQQ_ERR_UNSUPPORTED; }
  if (dtype != HQQ_F16 && dtype != HQQ_BF16) { set_error("%s: dtype %d", who, dtype); return HQQ_ERR_DTYPE; }
  if (T < 1 || T > MOE_MAX_T) { set_error("%s: %lld tokens are not covered (1 .. %d)", who, (long long)T, MOE_MAX_T); return HQQ_ERR_UNSUPPORTED; }
  if (k < 1 || k > MOE_MAX_K) { set_error("%s: %lld experts per token are not covered (1 .. %d)", who, (long long)k, MOE_MAX_K); return HQQ_ERR_UNSUPPORTED; }
  if (E < 1 || E > MOE_MAX_E) { set_error("%s: %lld experts are not covered (1 .. %d)", who, (long long)E, MOE_MAX_E); return HQQ_ERR_UNSUPPORTED; }
  const int per = 8 / nbits;
  if (H < 64 || H % 64 || H % (8 * per) || H > MOE_MAX_DIM) { set_error("%s: H=%lld is not covered (a multiple of 64, 64 .. %lld)", who, (long long)H, (long long)MOE_MAX_DIM); return HQQ_ERR_UNSUPPORTED; }
  if (I < 64 || I % 64 || I % (8 * per) || I > MOE_MAX_DIM) { set_error("%s: I=%lld is not covered (a multiple of 64, 64 .. %lld)", who, (long long)I, (long long)MOE_MAX_DIM); return HQQ_ERR_UNSUPPORTED; }
  if (gs < 16 || gs % 16 || H % gs || I % gs) {
    set_error("%s: group_size=%lld is not covered (a multiple of 16 that divides H=%lld and I=%lld)", who, (long long)gs, (long long)H, (long long)I);
    return HQQ_ERR_UNSUPPORTED;
  }
  // per-expert strides in bytes: H I / per of packed levels, 2 H I / group_size of constants — 16-byte multiples, so that every expert's rows stay aligned
  if ((H * I / per) % 16 || (2 * H * I / gs) % 16) { set_error("%s: per-expert strides of H=%lld, I=%lld, group_size=%lld are not 16-byte multiples", who, (long long)H, (long long)I, (long long)gs); return HQQ_ERR_UNSUPPORTED; }
  return 0;
}

static bool moe_layer_bad(const char* who, const void* Wq, const void* scale, const void* zero) {
  if (!Wq || !scale || !zero) { set_error("%s: null argument", who); return true; }
  return false;
}

}  // namespace hqq

using namespace hqq;

extern "C" int hqq_hip_moe_covers(int nbits, int64_t T, int64_t k, int64_t E, int64_t H, int64_t I, int64_t group_size, int dtype) {
  return moe_validate("hqq_hip_moe", nbits, T, k, E, H, I, group_size, dtype) == 0 ? 1 : 0;
}

extern "C" int hqq_hip_moe_gate_up(int nbits, const void* x, const void* idx, const void* gate_Wq, const void* gate_scale, const void* gate_zero,
                                   const void* up_Wq, const void* up_scale, const void* up_zero, void* a, int64_t T, int64_t k, int64_t E, int64_t H,
                                   int64_t I, int64_t group_size, int dtype, void* stream) {
  const char* who = "hqq_hip_moe_gate_up";
  if (const int rc = moe_validate(who, nbits, T, k, E, H, I, group_size, dtype)) return rc;
  clear_stale_error();
  if (!x || !idx || !a) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (moe_layer_bad(who, gate_Wq, gate_scale, gate_zero) || moe_layer_bad(who, up_Wq, up_scale, up_zero)) return HQQ_ERR_SHAPE;
  for (const void* p : {x, gate_Wq, gate_scale, gate_zero, up_Wq, up_scale, up_zero, static_cast<const void*>(a)})
    if (!aligned16(p)) { set_error("%s: x, a and the stacks must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  if (reinterpret_cast<uintptr_t>(idx) & 7u) { set_error("%s: idx must be aligned to its element size", who); return HQQ_ERR_ALIGN; }
  const MoeLayer g{static_cast<const uint8_t*>(gate_Wq), static_cast<const uint16_t*>(gate_scale), static_cast<const uint16_t*>(gate_zero)};
  const MoeLayer u{static_cast<const uint8_t*>(up_Wq), static_cast<const uint16_t*>(up_scale), static_cast<const uint16_t*>(up_zero)};
  const int per = 8 / nbits;
  const dim3 grid(static_cast<unsigned>((I / per + MOE_WAVES - 1) / MOE_WAVES), static_cast<unsigned>(T * k));
  hipStream_t st = as_stream(stream);
#define HQQ_MOE_GU(NB, BF)                                                                                                                    \
  hipLaunchKernelGGL((moe_gate_up_kernel<NB, BF>), grid, dim3(MOE_THREADS), 0, st, static_cast<const uint16_t*>(x), static_cast<const int64_t*>(idx), g, u, \
                     static_cast<uint16_t*>(a), static_cast<int>(k), static_cast<int>(E), static_cast<int>(H), static_cast<int>(I), static_cast<int>(group_size))
  if (nbits == 4) { if (dtype == HQQ_BF16) HQQ_MOE_GU(4, true); else HQQ_MOE_GU(4, false); }
  else { if (dtype == HQQ_BF16) HQQ_MOE_GU(2, true); else HQQ_MOE_GU(2, false); }
#undef HQQ_MOE_GU
  return check_launch(who);
}

extern "C" int hqq_hip_moe_down(int nbits, const void* a, const void* idx, const void* weights, const void* down_Wq, const void* down_scale,
                                const void* down_zero, void* out, int64_t T, int64_t k, int64_t E, int64_t H, int64_t I, int64_t group_size, int dtype,
                                void* stream) {
  const char* who = "hqq_hip_moe_down";
  if (const int rc = moe_validate(who, nbits, T, k, E, H, I, group_size, dtype)) return rc;
  clear_stale_error();
  if (!a || !idx || !weights || !out) { set_error("%s: null argument", who); return HQQ_ERR_SHAPE; }
  if (moe_layer_bad(who, down_Wq, down_scale, down_zero)) return HQQ_ERR_SHAPE;
  for (const void* p : {a, down_Wq, down_scale, down_zero, static_cast<const void*>(out)})
    if (!aligned16(p)) { set_error("%s: a, out and the stacks must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  if ((reinterpret_cast<uintptr_t>(idx) & 7u) || (reinterpret_cast<uintptr_t>(weights) & 3u)) { set_error("%s: idx and weights must be aligned to their element size", who); return HQQ_ERR_ALIGN; }
  const MoeLayer d{static_cast<const uint8_t*>(down_Wq), static_cast<const uint16_t*>(down_scale), static_cast<const uint16_t*>(down_zero)};
  const int per = 8 / nbits;
  const dim3 grid(static_cast<unsigned>((H / per + MOE_WAVES - 1) / MOE_WAVES), static_cast<unsigned>(T));
  hipStream_t st = as_stream(stream);
#define HQQ_MOE_DN(NB, BF)                                                                                                                          \
  hipLaunchKernelGGL((moe_down_kernel<NB, BF>), grid, dim3(MOE_THREADS), 0, st, static_cast<const uint16_t*>(a), static_cast<const int64_t*>(idx),    \
                     static_cast<const float*>(weights), d, static_cast<uint16_t*>(out), static_cast<int>(k), static_cast<int>(E), static_cast<int>(H), \
                     static_cast<int>(I), static_cast<int>(group_size))
  if (nbits == 4) { if (dtype == HQQ_BF16) HQQ_MOE_DN(4, true); else HQQ_MOE_DN(4, false); }
  else { if (dtype == HQQ_BF16) HQQ_MOE_DN(2, true); else HQQ_MOE_DN(2, false); }
#undef HQQ_MOE_DN
  return check_launch(who);
}
