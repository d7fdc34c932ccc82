// kv_cache.hip — a quantised static KV cache (8 / 4 bits per element) and the decode-step kernels that write and read it, gfx950, fp16 and bf16.
//
// The format is this library's own, one rule per (sequence, kv head, position) row r of head_dim values, keys (after the rotary embedding) and values alike:
//   Quantizer.quantize(r.view(head_dim / gs, gs), nbits, group_size=gs, axis=1, optimize=False, round_zero=False, channel_wise=True)
// (hqq/core/quantize.py:102-154: the row in fp32, min / max per group, scale = max_v / (max - min) as reciprocal() * max_v, 1 where the range is <= 1e-4,
// clamped to 2e4, zero = -min * scale, levels = clamp(rint(W * scale + zero), 0, max_v) with the product and the sum rounded separately, the stored scale
// 1 / scale), scale and zero then cast to the compute dtype T.  No solver runs: a row's result depends on no other row, so a token is quantised when it is
// written and never touched again.  8 bits: byte i of a row is level i.  4 bits: byte i is level[i] << 4 | level[i + head_dim / 2] (BitPack.pack_4bit_u8 on
// the [head_dim / gs, gs] level matrix).  Per layer: kq / vq [B, n_kv, L, head_dim * nbits / 8] uint8, k_scale / k_zero / v_scale / v_zero [B, n_kv, L, head_dim / gs] of T.
// Dequantisation is round_T(round_T(q - zero) * scale), the two roundings of Quantizer.dequantize (CD<T>::dequant).
//   kv_quantize            dense rows [B, n_kv, T, head_dim] -> positions start .. start + T - 1 of the six buffers (prefill, and the composed route's update)
//   kv_dequantize          positions 0 .. n - 1 of the six buffers -> dense [B, n_kv, n, head_dim] (the composed route, the tests)
//   rope_kvq_cache         rope_cache_kernel's work (block.hip) with the rotated key and the value row quantised on chip instead of stored densely
//   attn_decode_kvq        the decode attention's one body (attn_decode_core.h) on loaders that read a packed row and rebuild it to T: what runs behind the
//                          rebuild is the text attn_decode_kernel (block.hip) runs, so the output has the bits of attn_decode on the dequantised cache with the same splits
// In every kernel a LANE holds 8 consecutive dims of a row (LPK = head_dim / 8 lanes per row, whole rows within a wave); gs is 32 or 64, so a lane's 8 dims
// share one (scale, zero) pair.  Compiled with -ffp-contract=off: the reference's product and sum round separately.
#include "hqq_common.h"
#include "block_math.h"
#include "attn_decode_core.h"
#include "kv_load.h"

namespace hqq {

// ---- a lane's 8 dims x of a row, quantised with the gs / 8 lanes of its group (shuffles: every lane of the wave calls this, `store` says whether it writes) ----
template <int HD, int NBITS, bool BF>
__device__ __forceinline__ void kv_quant_store8(const u32x4& x, int ch, int gs, bool store, uint8_t* __restrict__ qrow, uint16_t* __restrict__ srow,
                                                uint16_t* __restrict__ zrow) {
  using E = El<BF>;
  constexpr int LPK = HD / 8;
  constexpr float maxv = NBITS == 8 ? 255.f : 15.f;
  float w[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t u = x[e];
    w[2 * e] = E::f(static_cast<uint16_t>(u & 0xFFFFu));
    w[2 * e + 1] = E::f(static_cast<uint16_t>(u >> 16));
  }
  float mn = w[0], mx = w[0];
#pragma unroll
  for (int e = 1; e < 8; ++e) { mn = fminf(mn, w[e]); mx = fmaxf(mx, w[e]); }
  for (int off = 1; off < gs / 8; off <<= 1) { mn = fminf(mn, __shfl_xor(mn, off, 64)); mx = fmaxf(mx, __shfl_xor(mx, off, 64)); }
  const float denom = mx - mn;
  float sc = (1.0f / denom) * maxv;            // Tensor.__rtruediv__: reciprocal() * max_v, two roundings (quantize.hip)
  if (fabsf(denom) <= 1e-4f) sc = 1.0f;
  sc = (sc > 2e4f) ? 2e4f : sc;                // clamp(max=2e4) keeps a NaN, as torch.clamp does
  float ze = (-mn) * sc;
  asm("" : "+v"(ze));                          // (an fp32 VALUE before it is cast to T below: no single-rounding mixed-precision multiply, block_math.h r_prod)
  uint32_t lv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float q = w[e] * sc;
    q = q + ze;
    q = rintf(q);
    q = fminf(fmaxf(q, 0.f), maxv);            // (a NaN level packs as 0, as in quantize.hip)
    lv[e] = static_cast<uint32_t>(q);
  }
  if constexpr (NBITS == 8) {
    u32x2 b;
    b[0] = lv[0] | (lv[1] << 8) | (lv[2] << 16) | (lv[3] << 24);
    b[1] = lv[4] | (lv[5] << 8) | (lv[6] << 16) | (lv[7] << 24);
    if (store) *reinterpret_cast<u32x2*>(qrow + ch * 8) = b;
  } else {
    uint32_t nib = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) nib |= lv[e] << (4 * e);
    const uint32_t other = __shfl_xor(nib, LPK / 2, 64);   // the levels of dims i + HD / 2 (for the lanes of the first half)
    u32x2 b;
    b[0] = 0; b[1] = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t byte = (lv[e] << 4) | ((other >> (4 * e)) & 0xFu);
      if (e < 4) b[0] |= byte << (8 * e);
      else b[1] |= byte << (8 * (e - 4));
    }
    if (store && ch < LPK / 2) *reinterpret_cast<u32x2*>(qrow + ch * 8) = b;
  }
  if (store && (ch * 8) % gs == 0) {
    float inv = 1.0f / sc;                     // quantize.py:154
    asm("" : "+v"(inv));
    srow[(ch * 8) / gs] = E::r(inv);
    zrow[(ch * 8) / gs] = E::r(ze);
  }
}

// ---- dense rows -> the six buffers.  blockIdx.y: 0 keys, 1 values.  Source strides in elements (a row's head_dim values are consecutive).
//      Row (b, h, t) goes to position (pos ? pos[b * pos_stride] : start) + t; a position outside [0, L) writes nothing ----
template <int HD, int NBITS, bool BF>
__global__ __launch_bounds__(256) void kv_quantize_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int64_t ksb, int64_t ksh, int64_t kst,
                                                          int64_t vsb, int64_t vsh, int64_t vst, int n_kv, int T, int64_t rows, int gs, int64_t start,
                                                          const int64_t* __restrict__ pos, int pos_stride, uint8_t* __restrict__ kq, uint16_t* __restrict__ ks,
                                                          uint16_t* __restrict__ kz, uint8_t* __restrict__ vq, uint16_t* __restrict__ vs, uint16_t* __restrict__ vz, int L) {
  constexpr int LPK = HD / 8, RPB = 256 / LPK, RB = HD * NBITS / 8;
  const int tid = threadIdx.x, sub = tid / LPK, ch = tid - sub * LPK;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * RPB + sub;
  const bool live = r < rows;
  const int64_t rr = live ? r : rows - 1;   // (the shuffles need every lane of a row group: rows past the end are computed on the last row and dropped)
  const int64_t bh = rr / T, t = rr - bh * T, b = bh / n_kv, h = bh - b * n_kv;
  const bool is_v = blockIdx.y != 0;
  const uint16_t* src = is_v ? v + b * vsb + h * vsh + t * vst : k + b * ksb + h * ksh + t * kst;
  const u32x4 x = reinterpret_cast<const u32x4*>(src)[ch];
  const int64_t p = (pos ? pos[b * pos_stride] : start) + t;
  const bool store = live && p >= 0 && p < L;
  const int64_t d = bh * L + (store ? p : 0);
  const int G = HD / gs;
  kv_quant_store8<HD, NBITS, BF>(x, ch, gs, store, pick(is_v, vq, kq) + d * RB, pick(is_v, vs, ks) + d * G, pick(is_v, vz, kz) + d * G);
}

// ---- positions 0 .. n - 1 of the six buffers -> dense [B * n_kv, n, HD].  blockIdx.y: 0 keys, 1 values ----
template <int HD, int NBITS, bool BF>
__global__ __launch_bounds__(256) void kv_dequantize_kernel(const uint8_t* __restrict__ kq, const uint16_t* __restrict__ ks, const uint16_t* __restrict__ kz,
                                                            const uint8_t* __restrict__ vq, const uint16_t* __restrict__ vs, const uint16_t* __restrict__ vz,
                                                            int64_t rows, int n, int L, int gs_shift, uint16_t* __restrict__ k_out, uint16_t* __restrict__ v_out) {
  constexpr int LPK = HD / 8, RPB = 256 / LPK, RB = HD * NBITS / 8;
  const int tid = threadIdx.x, sub = tid / LPK, ch = tid - sub * LPK;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * RPB + sub;
  if (r >= rows) return;
  const int64_t bh = r / n, t = r - bh * n, d = bh * L + t;
  const int G = HD >> gs_shift;
  const bool is_v = blockIdx.y != 0;
  const u32x4 o = kv_load8<HD, NBITS, BF>(pick(is_v, vq, kq) + d * RB, pick(is_v, vs, ks) + d * G, pick(is_v, vz, kz) + d * G, ch, gs_shift);
  reinterpret_cast<u32x4*>(pick(is_v, v_out, k_out) + r * HD)[ch] = o;
}

// ---- rope_cache_kernel (block.hip) with a quantised cache write.  blockIdx.x < qblocks: the query heads, one thread per (head, i < HD / 2), rope_cache_kernel's
//      arithmetic and q_out bits.  blockIdx.x - qblocks: a KV head — HD / 2 threads rotate the new key into LDS, then wave 0 quantises that row and wave 1 the
//      value row (kv_quant_store8: the bits kv_quantize gives for the dense row).  blockIdx.y: the sequence.  A position outside [0, L) writes nothing ----
template <int HD, int NBITS, bool BF>
__global__ __launch_bounds__(256) void rope_kvq_cache_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                             const uint16_t* __restrict__ cosv, const uint16_t* __restrict__ sinv, const int64_t* __restrict__ pos,
                                                             uint16_t* __restrict__ q_out, uint8_t* __restrict__ kq, uint16_t* __restrict__ ks, uint16_t* __restrict__ kz,
                                                             uint8_t* __restrict__ vq, uint16_t* __restrict__ vs, uint16_t* __restrict__ vz, int n_heads, int n_kv, int gs,
                                                             int L, int qblocks) {
  constexpr int half = HD / 2, LPK = HD / 8, RB = HD * NBITS / 8;
  __shared__ __attribute__((aligned(16))) uint16_t krot[HD];
  const int64_t row = blockIdx.y;
  const int tid = threadIdx.x;
  cosv += row * HD;
  sinv += row * HD;
  if (static_cast<int>(blockIdx.x) < qblocks) {
    const int id = blockIdx.x * 256 + tid;
    if (id >= n_heads * half) return;
    const int head = id / half, i = id - head * half;
    const uint16_t* src = q + (row * n_heads + head) * HD;
    uint16_t o1, o2;
    rope_pair<BF>(src[i], src[i + half], cosv[i], cosv[i + half], sinv[i], sinv[i + half], o1, o2);
    uint16_t* dst = q_out + (row * n_heads + head) * HD;
    dst[i] = o1;
    dst[i + half] = o2;
    return;
  }
  const int kh = blockIdx.x - qblocks;
  if (tid < half) {
    const uint16_t* src = k + (row * n_kv + kh) * HD;
    uint16_t o1, o2;
    rope_pair<BF>(src[tid], src[tid + half], cosv[tid], cosv[tid + half], sinv[tid], sinv[tid + half], o1, o2);
    krot[tid] = o1;
    krot[tid + half] = o2;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  if (wave >= 2) return;
  const int64_t p = pos[row];
  const bool ok = p >= 0 && p < L;   // rope_cache_kernel's rule: a position outside the cache writes nothing
  const int ch = lane % LPK;
  const bool store = ok && lane < LPK;   // (the other lanes of the wave repeat the row: the shuffles of a group stay among lanes that hold it)
  const bool is_v = wave == 1;
  const u32x4 x = is_v ? reinterpret_cast<const u32x4*>(v + (row * n_kv + kh) * HD)[ch] : reinterpret_cast<const u32x4*>(krot)[ch];
  const int64_t d = (row * n_kv + kh) * L + (ok ? p : 0);
  const int G = HD / gs;
  kv_quant_store8<HD, NBITS, BF>(x, ch, gs, store, pick(is_v, vq, kq) + d * RB, pick(is_v, vs, ks) + d * G, pick(is_v, vz, kz) + d * G);
}

// ---- decode attention on the six buffers: attn_decode_kernel<HD, false, BF>'s front (block.hip) with loaders that rebuild a packed row to T (kv_load8: the bytes
//      and the meta of row j); the phases behind them are attn_decode_body (attn_decode_core.h), the text the dense kernel runs.  Rows beyond pos are never read,
//      in levels or in meta ----
template <int HD, int NBITS, bool BF>
__global__ __launch_bounds__(512) void attn_decode_kvq_kernel(const uint16_t* __restrict__ q, const uint8_t* __restrict__ kq, const uint16_t* __restrict__ ks,
                                                              const uint16_t* __restrict__ kz, const uint8_t* __restrict__ vq, const uint16_t* __restrict__ vs,
                                                              const uint16_t* __restrict__ vz, const int64_t* __restrict__ pos, uint16_t* __restrict__ out, int n_heads,
                                                              int n_kv, int L, int gs_shift, float scaling, int S, float* __restrict__ ws) {
  constexpr int RB = HD * NBITS / 8;
  const int G = HD >> gs_shift;
  const int h = blockIdx.x, sp = blockIdx.y, rep = n_heads / n_kv, kvh = h / rep;
  {
    const int64_t row = blockIdx.z;
    q += row * n_heads * HD;
    out += row * n_heads * HD;
    const int64_t r0 = (row * n_kv + kvh) * L;
    kq += r0 * RB; vq += r0 * RB;
    ks += r0 * G; kz += r0 * G; vs += r0 * G; vz += r0 * G;
    pos += row;
    if (S > 1) ws += row * n_heads * S * (HD + 2);
  }
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const AttnLds<HD> lds(smem);
  const int tid = threadIdx.x;
  const int64_t p_raw = pos[0];
  const int p0 = (p_raw >= 0 && p_raw < L) ? static_cast<int>(p_raw) : L - 1;   // the dense kernel's rule: a position outside the cache attends as if at the last slot
  if (tid < HD / 8) reinterpret_cast<u32x4*>(lds.qs)[tid] = reinterpret_cast<const u32x4*>(q + static_cast<int64_t>(h) * HD)[tid];
  // (how a row index, never negative, is widened for the 64-bit row offsets.  8 bits: as unsigned, which costs the loops no sign registers — with the signed
  //  extension <64, 8, fp16> took 65 VGPRs where the phases written out in this kernel took 64, a wave per SIMD less.  4 bits: signed, the code this kernel
  //  always had — the unsigned form measured 3 - 7 % slower there.  profiles/attn_refactor_parity.md)
  using widen_t = std::conditional_t<NBITS == 8, uint32_t, int>;
  auto krow = [&](int ch, int j) -> u32x4 {
    const int64_t r = static_cast<widen_t>(j);
    return kv_load8<HD, NBITS, BF>(kq + r * RB, ks + r * G, kz + r * G, ch, gs_shift);
  };
  auto vrow = [&](int ch, int j) -> u32x4 {
    const int64_t r = static_cast<widen_t>(j);
    return kv_load8<HD, NBITS, BF>(vq + r * RB, vs + r * G, vz + r * G, ch, gs_shift);
  };
  attn_decode_body<HD, BF>(lds, h, sp, p0 + 1, S, scaling, out, ws, krow, vrow);
}

}  // namespace hqq

using namespace hqq;

typedef const uint16_t* cu16;
typedef uint16_t* u16;
typedef const uint8_t* cu8;
typedef uint8_t* u8;

static inline bool kv_batch_ok(int64_t batch, const char* who) {
  if (batch >= 1 && batch <= 65535) return true;
  set_error("%s: batch %lld outside [1, 65535]", who, (long long)batch);
  return false;
}

static int attn_kvq_run(const char* who, int nbits, const void* q, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale,
                        const void* v_zero, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t group_size,
                        int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace, size_t workspace_bytes, void* stream) {
  clear_stale_error();
  if (const int rc = kv_check(who, nbits, head_dim, group_size, cache_len, dtype)) return rc;   // (first: the cache's coverage rule answers with its own code)
  const AttnCall c{who, batch, n_heads, n_kv_heads, head_dim, cache_len, dtype, splits, workspace, workspace_bytes, out, stream};
  if (const int rc = attn_check(c, {q, kq, k_scale, k_zero, vq, v_scale, v_zero, pos_dev, out}, {q, kq, vq, out})) return rc;
  const int lds = attn_lds_launch(c.HD(), cache_len, c.S());   // (the dense kernel's layout and size)
  const int gs_shift = group_size == 64 ? 6 : 5;
  int rc = 0;
  kv_dispatch(head_dim, nbits, c.bf(), [&](auto HDc, auto NBc, auto BFc) {
    constexpr auto kern = &attn_decode_kvq_kernel<decltype(HDc)::value, decltype(NBc)::value, decltype(BFc)::value>;
    static LdsRaised raised;   // (one per instantiation)
    if ((rc = attn_raise_lds(raised, reinterpret_cast<const void*>(kern), lds, ATTN_LDS_MAX, who))) return;
    hipLaunchKernelGGL(kern, c.grid(batch), dim3(512), lds, as_stream(stream), static_cast<cu16>(q), static_cast<cu8>(kq), static_cast<cu16>(k_scale),
                       static_cast<cu16>(k_zero), static_cast<cu8>(vq), static_cast<cu16>(v_scale), static_cast<cu16>(v_zero), pos_dev, static_cast<u16>(out),
                       static_cast<int>(n_heads), static_cast<int>(n_kv_heads), static_cast<int>(cache_len), gs_shift, scaling, c.S(), c.ws());
  });
  return attn_finish(c, rc);
}

extern "C" {

int hqq_hip_kv_covers(int nbits, int64_t head_dim, int64_t group_size, int64_t cache_len, int dtype) {
  return kv_check("hqq_hip_kv_covers", nbits, head_dim, group_size, cache_len, dtype) == 0 ? 1 : 0;
}

int hqq_hip_kv_quantize(int nbits, const void* k, const void* v, const int64_t* k_strides, const int64_t* v_strides, int64_t batch, int64_t n_kv_heads, int64_t T_,
                        int64_t head_dim, int64_t group_size, int64_t start, const int64_t* pos_dev, int64_t pos_stride, void* kq, void* k_scale, void* k_zero, void* vq,
                        void* v_scale, void* v_zero, int64_t cache_len, int dtype, void* stream) {
  const char* who = "hqq_hip_kv_quantize";
  clear_stale_error();
  if (const int rc = kv_check(who, nbits, head_dim, group_size, cache_len, dtype)) return rc;
  if (!kv_batch_ok(batch, who)) return HQQ_ERR_SHAPE;
  if (!k || !v || !k_strides || !v_strides || !kq || !k_scale || !k_zero || !vq || !v_scale || !v_zero || n_kv_heads < 1 || n_kv_heads > INT32_MAX || T_ < 1 ||
      T_ > cache_len || (pos_stride != 0 && pos_stride != 1) || (!pos_dev && (start < 0 || start + T_ > cache_len))) {
    set_error("%s: bad arguments (1 <= T <= cache_len; a host start with start + T <= cache_len, or device positions with stride 0 / 1)", who);
    return HQQ_ERR_SHAPE;
  }
  for (int i = 0; i < 3; ++i)
    if (k_strides[i] < 0 || v_strides[i] < 0 || k_strides[i] % 8 || v_strides[i] % 8) { set_error("%s: source strides must be non-negative multiples of 8 elements", who); return HQQ_ERR_ALIGN; }
  if (!aligned16(k) || !aligned16(v) || !aligned16(kq) || !aligned16(vq)) { set_error("%s: the sources and the level buffers must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  const int64_t rows = batch * n_kv_heads * T_;
  const int64_t rpb = 256 / (head_dim / 8);
  const int64_t blocks = (rows + rpb - 1) / rpb;
  if (blocks > INT32_MAX) { set_error("%s: too many rows", who); return HQQ_ERR_SHAPE; }
  kv_dispatch(head_dim, nbits, dtype == HQQ_BF16, [&](auto HDc, auto NBc, auto BFc) {
    hipLaunchKernelGGL((kv_quantize_kernel<decltype(HDc)::value, decltype(NBc)::value, decltype(BFc)::value>), dim3(static_cast<unsigned>(blocks), 2), dim3(256), 0,
                       as_stream(stream), static_cast<cu16>(k), static_cast<cu16>(v), k_strides[0], k_strides[1], k_strides[2], v_strides[0], v_strides[1], v_strides[2],
                       static_cast<int>(n_kv_heads), static_cast<int>(T_), rows, static_cast<int>(group_size), start, pos_dev, static_cast<int>(pos_stride),
                       static_cast<u8>(kq), static_cast<u16>(k_scale), static_cast<u16>(k_zero), static_cast<u8>(vq), static_cast<u16>(v_scale), static_cast<u16>(v_zero),
                       static_cast<int>(cache_len));
  });
  return check_launch(who);
}

int hqq_hip_kv_dequantize(int nbits, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale, const void* v_zero, int64_t batch,
                          int64_t n_kv_heads, int64_t cache_len, int64_t n, int64_t head_dim, int64_t group_size, void* k_out, void* v_out, int dtype, void* stream) {
  const char* who = "hqq_hip_kv_dequantize";
  clear_stale_error();
  if (const int rc = kv_check(who, nbits, head_dim, group_size, cache_len, dtype)) return rc;
  if (!kv_batch_ok(batch, who)) return HQQ_ERR_SHAPE;
  if (!kq || !k_scale || !k_zero || !vq || !v_scale || !v_zero || !k_out || !v_out || n_kv_heads < 1 || n_kv_heads > INT32_MAX || n < 1 || n > cache_len) {
    set_error("%s: bad arguments (1 <= n <= cache_len)", who);
    return HQQ_ERR_SHAPE;
  }
  if (!aligned16(kq) || !aligned16(vq) || !aligned16(k_out) || !aligned16(v_out)) { set_error("%s: the level buffers and the outputs must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  const int64_t rows = batch * n_kv_heads * n;
  const int64_t rpb = 256 / (head_dim / 8);
  const int64_t blocks = (rows + rpb - 1) / rpb;
  if (blocks > INT32_MAX) { set_error("%s: too many rows", who); return HQQ_ERR_SHAPE; }
  kv_dispatch(head_dim, nbits, dtype == HQQ_BF16, [&](auto HDc, auto NBc, auto BFc) {
    hipLaunchKernelGGL((kv_dequantize_kernel<decltype(HDc)::value, decltype(NBc)::value, decltype(BFc)::value>), dim3(static_cast<unsigned>(blocks), 2), dim3(256), 0,
                       as_stream(stream), static_cast<cu8>(kq), static_cast<cu16>(k_scale), static_cast<cu16>(k_zero), static_cast<cu8>(vq), static_cast<cu16>(v_scale),
                       static_cast<cu16>(v_zero), rows, static_cast<int>(n), static_cast<int>(cache_len), group_size == 64 ? 6 : 5, static_cast<u16>(k_out),
                       static_cast<u16>(v_out));
  });
  return check_launch(who);
}

int hqq_hip_rope_kvq_cache_batched(int nbits, const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t batch,
                                   void* q_out, void* kq, void* k_scale, void* k_zero, void* vq, void* v_scale, void* v_zero, int64_t n_heads, int64_t n_kv_heads,
                                   int64_t head_dim, int64_t group_size, int64_t cache_len, int dtype, void* stream) {
  const char* who = "hqq_hip_rope_kvq_cache_batched";
  clear_stale_error();
  if (const int rc = kv_check(who, nbits, head_dim, group_size, cache_len, dtype)) return rc;
  if (!kv_batch_ok(batch, who)) return HQQ_ERR_SHAPE;
  if (!q || !k || !v || !cos || !sin || !pos_dev || !q_out || !kq || !k_scale || !k_zero || !vq || !v_scale || !v_zero || n_heads < 1 || n_kv_heads < 1 ||
      (n_heads + n_kv_heads) * head_dim > INT32_MAX) { set_error("%s: bad arguments", who); return HQQ_ERR_SHAPE; }
  if (!aligned16(v) || !aligned16(kq) || !aligned16(vq)) { set_error("%s: v and the level buffers must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  const int64_t qblocks = (n_heads * (head_dim / 2) + 255) / 256;
  if (qblocks + n_kv_heads > INT32_MAX) { set_error("%s: too many heads", who); return HQQ_ERR_SHAPE; }
  kv_dispatch(head_dim, nbits, dtype == HQQ_BF16, [&](auto HDc, auto NBc, auto BFc) {
    hipLaunchKernelGGL((rope_kvq_cache_kernel<decltype(HDc)::value, decltype(NBc)::value, decltype(BFc)::value>),
                       dim3(static_cast<unsigned>(qblocks + n_kv_heads), static_cast<unsigned>(batch)), dim3(256), 0, as_stream(stream), static_cast<cu16>(q),
                       static_cast<cu16>(k), static_cast<cu16>(v), static_cast<cu16>(cos), static_cast<cu16>(sin), pos_dev, static_cast<u16>(q_out), static_cast<u8>(kq),
                       static_cast<u16>(k_scale), static_cast<u16>(k_zero), static_cast<u8>(vq), static_cast<u16>(v_scale), static_cast<u16>(v_zero),
                       static_cast<int>(n_heads), static_cast<int>(n_kv_heads), static_cast<int>(group_size), static_cast<int>(cache_len), static_cast<int>(qblocks));
  });
  return check_launch(who);
}

int hqq_hip_attn_decode_kvq(int nbits, const void* q, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale, const void* v_zero,
                            const int64_t* pos_dev, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t group_size, int64_t cache_len, float scaling,
                            int dtype, int64_t splits, void* workspace, size_t workspace_bytes, void* stream) {
  return attn_kvq_run("hqq_hip_attn_decode_kvq", nbits, q, kq, k_scale, k_zero, vq, v_scale, v_zero, pos_dev, 1, out, n_heads, n_kv_heads, head_dim, group_size, cache_len,
                      scaling, dtype, splits, workspace, workspace_bytes, stream);
}

int hqq_hip_attn_decode_kvq_batched(int nbits, const void* q, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale,
                                    const void* v_zero, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim,
                                    int64_t group_size, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace, size_t workspace_bytes, void* stream) {
  return attn_kvq_run("hqq_hip_attn_decode_kvq_batched", nbits, q, kq, k_scale, k_zero, vq, v_scale, v_zero, pos_dev, batch, out, n_heads, n_kv_heads, head_dim, group_size,
                      cache_len, scaling, dtype, splits, workspace, workspace_bytes, stream);
}

}  // extern "C"
