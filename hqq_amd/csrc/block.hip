// block.hip — the steps either side of the fused GEMVs in a decode step, gfx950, fp16 and bf16.
//
// The reference's headline number is the tok/s of its generate loop (hqq/utils/generation_hf.py:117-540, Readme.md:153): HF's decoder
// block around HQQLinear.forward — RMSNorm, rotary embedding, KV-cache update, SiLU(gate) * up, the residual adds — is ~25 small
// eager kernels per block, 79 % of a bs = 1 token once the linears are fused.  Three kernels replace twenty of them;
// each restates the HF module's arithmetic rounding for rounding, so that the fused loop emits the same tokens (T = the model's dtype):
//   add_rmsnorm   h += delta (one rounding: `residual + hidden_states`), then LlamaRMSNorm: fp32 x * rsqrt(mean(x^2) + eps) -> T -> weight * (a product in T)
//   rope_cache    apply_rotary_pos_emb: (q * cos) + (rotate_half(q) * sin) with three roundings to T, k likewise, and the StaticCache
//                 update (k_rot / v written at cache_position, read from device memory: graph-replay safe)
//   silu_mul      LlamaMLP: act_fn(gate) * up — silu in fp32 (x / (1 + exp(-x))), rounded to T, then the product in T
//   qknorm_rope_cache  Qwen3Attention: q_norm / k_norm (Qwen3RMSNorm per head: LlamaRMSNorm's roundings over head_dim elements), then rope_cache — the one
//                 op by which Qwen3's decoder block differs from Llama's (opt-in, FusedLlamaStep(qk_norm=True))
//   bias_rope_cache  Qwen2Attention: q_proj / k_proj / v_proj carry a bias — `out += bias` on the rounded matmul result, one rounding in T —, then rope_cache:
//                 the one op by which Qwen2's decoder block differs from Llama's (opt-in, FusedLlamaStep(qkv_bias=True); the q|k|v launch stays bias-free)
// T = fp16: native half arithmetic.  T = bf16: float arithmetic + one round-to-nearest-even per op, which is how torch evaluates bf16 elementwise ops.
// And one that does NOT restate a kernel bit for bit (opt-in, FusedLlamaStep(attention="hip")):
//   attn_decode   softmax(q K^T * scaling) V for ONE query per head over the static KV cache's first pos + 1 positions, fp32 scores / softmax /
//                 accumulation, one rounding of the output: what F.scaled_dot_product_attention computes for a decode step, within
//                 rounding of it (SDPA's flash kernel blocks the keys and rounds P to T; this one does neither) — 8 us instead of the
//                 12-15 us the library's prefill-shaped kernel takes for a single query (profiles/r04_e2e_kernel_times.txt)
// Compiled with -ffp-contract=off: a fused multiply-add would remove a rounding HF's separate ops make.
#include "hqq_common.h"
#include "block_math.h"
#include "attn_decode_core.h"

namespace hqq {

// ---- h (+= delta), xn = weight * T(float(h) * rsqrt(mean(float(h)^2) + eps)): one workgroup of 512 threads per row.
//      Rows of up to 512 * 8 * RPT elements stay in registers between the two passes (every load is issued before the reduction: the kernel is
//      one memory round trip + one barrier long); longer rows take the generic two-pass path ----
template <int RPT, bool BF>   // RPT: 16-byte chunks per thread held in registers; 0: re-read
__global__ __launch_bounds__(512) void add_rmsnorm_kernel(uint16_t* __restrict__ h, const uint16_t* __restrict__ delta, const uint16_t* __restrict__ weight, float eps,
                                                          uint16_t* __restrict__ xn, int H) {
  using E = El<BF>;
  __shared__ float part[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint16_t* hr = h + static_cast<int64_t>(blockIdx.x) * H;
  const uint16_t* dr = delta ? delta + static_cast<int64_t>(blockIdx.x) * H : nullptr;
  uint16_t* xr = xn + static_cast<int64_t>(blockIdx.x) * H;
  constexpr int NR = RPT > 0 ? RPT : 1;
  u32x4 hv[NR], wv[NR];
  float sum = 0.f;
  if constexpr (RPT > 0) {
    u32x4 dv[NR];
#pragma unroll
    for (int c = 0; c < NR; ++c) {
      const int i = (c * 512 + tid) * 8;
      if (i < H) {
        hv[c] = *reinterpret_cast<const u32x4*>(hr + i);
        if (dr) dv[c] = *reinterpret_cast<const u32x4*>(dr + i);
        wv[c] = *reinterpret_cast<const u32x4*>(weight + i);
      }
    }
#pragma unroll
    for (int c = 0; c < NR; ++c) {
      const int i = (c * 512 + tid) * 8;
      if (i < H) {
        uint16_t* hp = reinterpret_cast<uint16_t*>(&hv[c]);
        if (dr) {
          const uint16_t* dp = reinterpret_cast<const uint16_t*>(&dv[c]);
#pragma unroll
          for (int j = 0; j < 8; ++j) hp[j] = E::add(hp[j], dp[j]);   // residual + hidden_states, one rounding
          *reinterpret_cast<u32x4*>(hr + i) = hv[c];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = E::f(hp[j]); sum += f * f; }
      }
    }
  } else {
    for (int i = tid * 8; i < H; i += 512 * 8) {
      u32x4 v = *reinterpret_cast<const u32x4*>(hr + i);
      uint16_t* hp = reinterpret_cast<uint16_t*>(&v);
      if (dr) {
        const u32x4 dv = *reinterpret_cast<const u32x4*>(dr + i);
        const uint16_t* dp = reinterpret_cast<const uint16_t*>(&dv);
#pragma unroll
        for (int j = 0; j < 8; ++j) hp[j] = E::add(hp[j], dp[j]);
        *reinterpret_cast<u32x4*>(hr + i) = v;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float f = E::f(hp[j]); sum += f * f; }
    }
  }
  // wave sum (shuffles), then the eight waves through LDS, fixed order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  const float total = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
  const float r = rsqrtf(total / static_cast<float>(H) + eps);
  if constexpr (RPT > 0) {
#pragma unroll
    for (int c = 0; c < NR; ++c) {
      const int i = (c * 512 + tid) * 8;
      if (i < H) {
        const uint16_t* hp = reinterpret_cast<const uint16_t*>(&hv[c]);
        const uint16_t* wp = reinterpret_cast<const uint16_t*>(&wv[c]);
        u32x4 ov;
        uint16_t* op = reinterpret_cast<uint16_t*>(&ov);
#pragma unroll
        for (int j = 0; j < 8; ++j) op[j] = E::mul(wp[j], E::r_prod(E::f(hp[j]), r));
        *reinterpret_cast<u32x4*>(xr + i) = ov;
      }
    }
  } else {
    for (int i = tid * 8; i < H; i += 512 * 8) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(hr + i);
      const u32x4 w = *reinterpret_cast<const u32x4*>(weight + i);
      const uint16_t* hp = reinterpret_cast<const uint16_t*>(&v);
      const uint16_t* wp = reinterpret_cast<const uint16_t*>(&w);
      u32x4 ov;
      uint16_t* op = reinterpret_cast<uint16_t*>(&ov);
#pragma unroll
      for (int j = 0; j < 8; ++j) op[j] = E::mul(wp[j], E::r_prod(E::f(hp[j]), r));
      *reinterpret_cast<u32x4*>(xr + i) = ov;
    }
  }
}

// ---- rotary embedding of q and k, KV-cache write.  One thread per (head, i < hd / 2): elements i and i + hd / 2 of a head.
//      blockIdx.y: the sequence of a batch (hqq_hip_rope_cache_batched) — every tensor advances by one sequence's extent, the arithmetic is the same.
//      cache_row: the elements between two rows' caches, n_kv * cache_len * hd; 0 (hqq_hip_rope_cache_shared): the rows are positions of ONE sequence
//      and write into the one cache [n_kv, cache_len, hd], each at its own pos ----
template <bool BF>
__global__ __launch_bounds__(256) void rope_cache_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                         const uint16_t* __restrict__ cosv, const uint16_t* __restrict__ sinv, const int64_t* __restrict__ pos,
                                                         uint16_t* __restrict__ q_out, uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache,
                                                         int n_heads, int n_kv, int hd, int cache_len, int64_t cache_row) {
  const int half = hd / 2;
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = (n_heads + n_kv) * half;
  if (id >= total) return;
  const int64_t row = blockIdx.y;
  q += row * n_heads * hd;
  q_out += row * n_heads * hd;
  k += row * n_kv * hd;
  v += row * n_kv * hd;
  cosv += row * hd;
  sinv += row * hd;
  pos += row;
  k_cache += row * cache_row;
  v_cache += row * cache_row;
  const int head = id / half, i = id - head * half;
  const bool is_k = head >= n_heads;
  const uint16_t* src = is_k ? k + static_cast<int64_t>(head - n_heads) * hd : q + static_cast<int64_t>(head) * hd;
  uint16_t o1, o2;
  rope_pair<BF>(src[i], src[i + half], cosv[i], cosv[i + half], sinv[i], sinv[i + half], o1, o2);
  if (!is_k) {
    q_out[static_cast<int64_t>(head) * hd + i] = o1;
    q_out[static_cast<int64_t>(head) * hd + i + half] = o2;
  } else {
    const int64_t p = pos[0];
    if (p < 0 || p >= cache_len) return;   // a position outside the cache writes nothing (HF's StaticCache index_copy_ raises a device assert there)
    const int kh = head - n_heads;
    uint16_t* kd = k_cache + (static_cast<int64_t>(kh) * cache_len + p) * hd;
    uint16_t* vd = v_cache + (static_cast<int64_t>(kh) * cache_len + p) * hd;
    kd[i] = o1;
    kd[i + half] = o2;
    const uint16_t* vs = v + static_cast<int64_t>(kh) * hd;
    vd[i] = vs[i];
    vd[i + half] = vs[i + half];
  }
}

// ---- rope_cache_kernel with the three projection biases added in front (Qwen2Attention: q_proj / k_proj / v_proj have a bias, shared by every sequence):
//      q' = q + q_bias, k' = k + k_bias, v' = v + v_bias, each ONE rounding to T — the decode kernels' `out += bias` on the rounded matmul result
//      (gemv_kernel.inc, skinny.hip) —, then rope_pair on q' / k' and the cache write of k' / v'.  rope_cache_kernel's geometry: one thread per
//      (head, i < hd / 2), blockIdx.y the sequence; no LDS, no workspace ----
template <bool BF>
__global__ __launch_bounds__(256) void bias_rope_cache_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                              const uint16_t* __restrict__ q_bias, const uint16_t* __restrict__ k_bias, const uint16_t* __restrict__ v_bias,
                                                              const uint16_t* __restrict__ cosv, const uint16_t* __restrict__ sinv, const int64_t* __restrict__ pos,
                                                              uint16_t* __restrict__ q_out, uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache,
                                                              int n_heads, int n_kv, int hd, int cache_len) {
  using E = El<BF>;
  const int half = hd / 2;
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = (n_heads + n_kv) * half;
  if (id >= total) return;
  const int64_t row = blockIdx.y;
  q += row * n_heads * hd;
  q_out += row * n_heads * hd;
  k += row * n_kv * hd;
  v += row * n_kv * hd;
  cosv += row * hd;
  sinv += row * hd;
  pos += row;
  k_cache += row * n_kv * cache_len * hd;
  v_cache += row * n_kv * cache_len * hd;
  const int head = id / half, i = id - head * half;
  const bool is_k = head >= n_heads;
  const int64_t off = static_cast<int64_t>(is_k ? head - n_heads : head) * hd;   // the head's first element in a row of q (k / v): the bias index too
  const uint16_t* src = (is_k ? k : q) + off;
  const uint16_t* bias = (is_k ? k_bias : q_bias) + off;
  const uint16_t x1 = E::add(src[i], bias[i]), x2 = E::add(src[i + half], bias[i + half]);
  uint16_t o1, o2;
  rope_pair<BF>(x1, x2, cosv[i], cosv[i + half], sinv[i], sinv[i + half], o1, o2);
  if (!is_k) {
    q_out[off + i] = o1;
    q_out[off + i + half] = o2;
  } else {
    const int64_t p = pos[0];
    if (p < 0 || p >= cache_len) return;   // rope_cache_kernel's rule: a position outside the cache writes nothing
    const int kh = head - n_heads;
    uint16_t* kd = k_cache + (static_cast<int64_t>(kh) * cache_len + p) * hd;
    uint16_t* vd = v_cache + (static_cast<int64_t>(kh) * cache_len + p) * hd;
    kd[i] = o1;
    kd[i + half] = o2;
    vd[i] = E::add(v[off + i], v_bias[off + i]);
    vd[i + half] = E::add(v[off + i + half], v_bias[off + i + half]);
  }
}

// ---- per-head RMSNorm of q and k (Qwen3Attention's q_norm / k_norm), then rope_cache_kernel's rotary embedding and KV-cache write, one launch.
//      One WAVE per (sequence, head), four waves per workgroup; blockIdx.y: the sequence.  Lane l holds the rotary pairs i = l + 64 j < HD / 2:
//      elements i and i + HD / 2 of its head (HD = 64: lanes 32..63 hold nothing and add zeros).  The fp32 sum of squares is each lane's own
//      elements in index order, then a butterfly of shuffles: a fixed order, the same bits on every call.  No LDS, no workspace.
//      Qwen3RMSNorm's roundings (add_rmsnorm_kernel's): fp32 x * rsqrt(mean(x^2) + eps) -> T -> weight * (a product in T); rope_pair on those values ----
template <int HD, bool BF>
__global__ __launch_bounds__(256) void qknorm_rope_cache_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                                const uint16_t* __restrict__ q_weight, const uint16_t* __restrict__ k_weight, float q_eps, float k_eps,
                                                                const uint16_t* __restrict__ cosv, const uint16_t* __restrict__ sinv, const int64_t* __restrict__ pos,
                                                                uint16_t* __restrict__ q_out, uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache,
                                                                int n_heads, int n_kv, int cache_len) {
  using E = El<BF>;
  constexpr int half = HD / 2, NP = (half + 63) / 64;
  const int lane = threadIdx.x & 63;
  const int head = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (head >= n_heads + n_kv) return;   // (a whole wave leaves: the shuffles below never miss a lane)
  const int64_t row = blockIdx.y;
  const bool is_k = head >= n_heads;
  const int kh = head - n_heads;
  const uint16_t* src = is_k ? k + (row * n_kv + kh) * HD : q + (row * n_heads + head) * HD;
  const uint16_t* w = is_k ? k_weight : q_weight;
  cosv += row * HD;
  sinv += row * HD;
  uint16_t x1[NP], x2[NP];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int i = lane + 64 * j;
    const bool live = i < half;
    x1[j] = live ? src[i] : static_cast<uint16_t>(0);
    x2[j] = live ? src[i + half] : static_cast<uint16_t>(0);
    const float f1 = E::f(x1[j]), f2 = E::f(x2[j]);
    sum += f1 * f1;
    sum += f2 * f2;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  const float r = rsqrtf(sum / static_cast<float>(HD) + (is_k ? k_eps : q_eps));
  uint16_t* dst;
  if (!is_k) {
    dst = q_out + (row * n_heads + head) * HD;
  } else {
    const int64_t p = pos[row];
    if (p < 0 || p >= cache_len) return;   // rope_cache_kernel's rule: a position outside the cache writes nothing
    const int64_t slot = ((row * n_kv + kh) * cache_len + p) * HD;
    dst = k_cache + slot;
    const uint16_t* vs = v + (row * n_kv + kh) * HD;
    uint16_t* vd = v_cache + slot;
    for (int e = lane; e < HD; e += 64) vd[e] = vs[e];
  }
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int i = lane + 64 * j;
    if (i < half) {
      const uint16_t n1 = E::mul(w[i], E::r_prod(E::f(x1[j]), r));
      const uint16_t n2 = E::mul(w[i + half], E::r_prod(E::f(x2[j]), r));
      uint16_t o1, o2;
      rope_pair<BF>(n1, n2, cosv[i], cosv[i + half], sinv[i], sinv[i + half], o1, o2);
      dst[i] = o1;
      dst[i + half] = o2;
    }
  }
}

// ---- out = T(silu(gate)) * up ----
template <bool BF>
__global__ __launch_bounds__(256) void silu_mul_kernel(const uint16_t* __restrict__ g, const uint16_t* __restrict__ u, uint16_t* __restrict__ out, int64_t n) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) * 8;
  if (i >= n) return;
  const u32x4 gv = *reinterpret_cast<const u32x4*>(g + i);
  const u32x4 uv = *reinterpret_cast<const u32x4*>(u + i);
  const uint16_t* gp = reinterpret_cast<const uint16_t*>(&gv);
  const uint16_t* up = reinterpret_cast<const uint16_t*>(&uv);
  u32x4 ov;
  uint16_t* op = reinterpret_cast<uint16_t*>(&ov);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    op[j] = silu_mul_el<BF>(gp[j], up[j]);
  }
  *reinterpret_cast<u32x4*>(out + i) = ov;
}

// ---- decode attention on the dense cache: one workgroup of 512 threads per (query head, share of the keys).  The kernel is the front of attn_decode_body
//      (attn_decode_core.h: scores + maximum, exp + sum, P V + merge + output or record — one body, two loaders: this kernel's read dense rows, the
//      quantised cache's, kv_cache.hip, rebuild packed ones): it finds its sequence, clamps the position, puts the query into LDS and states how a key /
//      value row is loaded.  Keys beyond pos are never read.
//      ROPE = true (hqq_hip_rope_attn_decode): q, k, v are the RAW projections; the workgroup applies the rotary embedding to its query and to its
//      KV head's new key itself (rope_cache_kernel's arithmetic, rounding for rounding), uses the new key / value from LDS for position pos — the
//      cache is only read below pos, so no workgroup depends on another's write — and the first query head of each KV head writes them to the cache.
//      blockIdx.z: the sequence of a batch (the *_batched entry points) — its own q / k / v rows, cache [n_kv, L, HD], position and output row;
//      its records are those of head b n_heads + h.
//      cache_row: the elements between two sequences' caches, n_kv * L * HD; 0 (hqq_hip_attn_decode_shared, ROPE = false only): the rows are queries of ONE
//      sequence on the one cache [n_kv, L, HD], row i attending over its own pos[i] + 1 keys — everything else, and so every bit of a row, is unchanged ----
template <int HD, bool ROPE, bool BF>
__global__ __launch_bounds__(512) void attn_decode_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc_in, const uint16_t* __restrict__ vc_in,
                                                          const int64_t* __restrict__ pos, uint16_t* __restrict__ out, int n_heads, int n_kv, int L, float scaling,
                                                          const uint16_t* __restrict__ k_raw, const uint16_t* __restrict__ v_raw, const uint16_t* __restrict__ cosv,
                                                          const uint16_t* __restrict__ sinv, uint16_t* __restrict__ kc_out, uint16_t* __restrict__ vc_out,
                                                          int S, float* __restrict__ ws, int64_t cache_row) {
  {
    const int64_t row = blockIdx.z;
    q += row * n_heads * HD;
    out += row * n_heads * HD;
    kc_in += row * cache_row;
    vc_in += row * cache_row;
    pos += row;
    if constexpr (ROPE) {
      k_raw += row * n_kv * HD;
      v_raw += row * n_kv * HD;
      cosv += row * HD;
      sinv += row * HD;
      kc_out += row * cache_row;
      vc_out += row * cache_row;
    }
    if (S > 1) ws += row * n_heads * S * (HD + 2);
  }
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const AttnLds<HD> lds(smem);
  uint16_t* const qs = lds.qs;
  uint16_t* const knew = qs + HD;
  uint16_t* const vnew = qs + 2 * HD;
  const int h = blockIdx.x, sp = blockIdx.y, rep = n_heads / n_kv, kvh = h / rep;
  const int tid = threadIdx.x;
  // a position outside [0, L) must not index the cache or the score buffer (sized from L): attend as if at the last slot, write nothing
  const int64_t p_raw = pos[0];
  const bool p_ok = p_raw >= 0 && p_raw < L;
  const int p0 = p_ok ? static_cast<int>(p_raw) : L - 1;
  const uint16_t* __restrict__ K = kc_in + static_cast<int64_t>(kvh) * L * HD;
  const uint16_t* __restrict__ V = vc_in + static_cast<int64_t>(kvh) * L * HD;
  if constexpr (ROPE) {
    // thread t < HD / 2: elements t and t + HD / 2 of the query; HD / 2 <= t < HD: of the new key; HD <= t < HD + HD / 8: a 16-byte chunk of the new value
    constexpr int half = HD / 2;
    if (tid < HD) {
      const bool is_k = tid >= half;
      const int i = is_k ? tid - half : tid;
      const uint16_t* src = is_k ? k_raw + static_cast<int64_t>(kvh) * HD : q + static_cast<int64_t>(h) * HD;
      uint16_t o1, o2;
      rope_pair<BF>(src[i], src[i + half], cosv[i], cosv[i + half], sinv[i], sinv[i + half], o1, o2);
      uint16_t* dst = is_k ? knew : qs;
      dst[i] = o1;
      dst[i + half] = o2;
      if (is_k && h % rep == 0 && sp == 0 && p_ok) {
        uint16_t* kd = kc_out + (static_cast<int64_t>(kvh) * L + p0) * HD;
        kd[i] = o1;
        kd[i + half] = o2;
      }
    } else if (tid < HD + HD / 8) {
      const int c = tid - HD;
      const u32x4 vv = reinterpret_cast<const u32x4*>(v_raw + static_cast<int64_t>(kvh) * HD)[c];
      reinterpret_cast<u32x4*>(vnew)[c] = vv;
      if (h % rep == 0 && sp == 0 && p_ok) reinterpret_cast<u32x4*>(vc_out + (static_cast<int64_t>(kvh) * L + p0) * HD)[c] = vv;
    }
  } else {
    if (tid < HD / 8) reinterpret_cast<u32x4*>(qs)[tid] = reinterpret_cast<const u32x4*>(q + static_cast<int64_t>(h) * HD)[tid];
  }
  // the rows of the dense cache; ROPE: the new key / value from LDS — their cache row is being written by another workgroup
  auto row = [&](const uint16_t* __restrict__ base, const uint16_t* fresh, int ch, int j) -> u32x4 {
    const uint16_t* r = (ROPE && j == p0) ? fresh : base + static_cast<int64_t>(j) * HD;
    return reinterpret_cast<const u32x4*>(r)[ch];
  };
  attn_decode_body<HD, BF>(lds, h, sp, p0 + 1, S, scaling, out, ws, [&](int ch, int j) { return row(K, knew, ch, j); }, [&](int ch, int j) { return row(V, vnew, ch, j); });
}

// ---- the S shares of a head, merged in split order: out = sum_s e^(m_s - m) o_s / sum_s e^(m_s - m) l_s ----
template <bool BF>
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* __restrict__ ws, uint16_t* __restrict__ out, int S, int HD) {
  using E = El<BF>;
  const int h = blockIdx.x, d = threadIdx.x;
  if (d >= HD) return;
  const float* rec = ws + static_cast<int64_t>(h) * S * (HD + 2);
  float m = -INFINITY;
  for (int s_ = 0; s_ < S; ++s_) m = fmaxf(m, rec[s_ * (HD + 2)]);
  float num = 0.f, den = 0.f;
  for (int s_ = 0; s_ < S; ++s_) {
    const float* r_ = rec + s_ * (HD + 2);
    const float w = r_[1] > 0.f ? __expf(r_[0] - m) : 0.f;
    num = fmaf(w, r_[2 + d], num);
    den = fmaf(w, r_[1], den);
  }
  out[static_cast<int64_t>(h) * HD + d] = E::r(num / den);
}

// ---- the per-token work either side of the decoder blocks (hqq/utils/generation_hf.py:405-540: the embedding lookup, the rotary table row and the causal mask of one
//      query in front; argmax, token hand-over and position increment behind), one launch each instead of nine small torch kernels.  Pure copies and compares:
//      bit-identical to the torch ops they replace.
//      token_prologue: h = embed[tok]; cos = cos_tab[pos]; sin = sin_tab[pos]; mask[i] = i <= pos ? 0 : -inf (mask == null: the caller's attention needs none).
//      A token / position outside the tables reads the last row (the torch ops would trap; the host checks positions, utils/generation.py).
//      blockIdx.y: the sequence of a batch (hqq_hip_token_prologue_batched): tok / pos element, h [H], cos / sin [hd] and mask [L] row of its own ----
__global__ __launch_bounds__(256) void token_prologue_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ pos, const uint16_t* __restrict__ embed, int64_t vocab, int H,
                                                             const uint16_t* __restrict__ cos_tab, const uint16_t* __restrict__ sin_tab, int64_t L, int hd,
                                                             uint16_t* __restrict__ h, uint16_t* __restrict__ cos_o, uint16_t* __restrict__ sin_o, uint16_t* __restrict__ mask,
                                                             uint16_t zero_bits, uint16_t ninf_bits) {
  {
    const int64_t row = blockIdx.y;
    tok += row;
    pos += row;
    h += row * H;
    if (cos_tab) { cos_o += row * hd; sin_o += row * hd; }
    if (mask) mask += row * L;
  }
  int64_t t = tok[0], p = pos[0];
  t = t < 0 ? 0 : (t >= vocab ? vocab - 1 : t);
  const int64_t pr = p < 0 ? 0 : (p >= L ? L - 1 : p);
  const int nb = static_cast<int>(gridDim.x), b = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const u32x4* src = reinterpret_cast<const u32x4*>(embed + t * H);
  for (int i = b * 256 + tid; i < H / 8; i += nb * 256) reinterpret_cast<u32x4*>(h)[i] = src[i];
  if (b == 0 && cos_tab) {
    for (int i = tid; i < hd; i += 256) { cos_o[i] = cos_tab[pr * hd + i]; sin_o[i] = sin_tab[pr * hd + i]; }
  }
  if (mask) {
    for (int64_t i = b * 256 + tid; i < L; i += static_cast<int64_t>(nb) * 256) mask[i] = i <= p ? zero_bits : ninf_bits;
  }
}

// argmax_advance: next = the FIRST index of the largest logit (torch.argmax's tie and NaN rule: the first NaN wins over every number, -0 == +0, +-inf are ordinary values), written to next_tok and tok, pos += 1.  One workgroup:
// 1024 threads keep (value, index) of their strided share in index order, then a fixed tree in LDS.  blockIdx.x: the sequence of a batch
// (hqq_hip_argmax_advance_batched): logits row, next_tok / tok / pos element of its own.
template <bool BF>
__global__ __launch_bounds__(1024) void argmax_advance_kernel(const uint16_t* __restrict__ logits, int n, int64_t* __restrict__ next_tok, int64_t* __restrict__ tok, int64_t* __restrict__ pos) {
  using E = El<BF>;
  __shared__ float bv[1024];
  __shared__ int bi[1024];
  const int tid = static_cast<int>(threadIdx.x);
  {
    const int64_t row = blockIdx.x;
    logits += row * n;
    next_tok += row;
    if (tok) tok += row;
    if (pos) pos += row;
  }
  // torch.argmax's order: a NaN is the maximum (the FIRST NaN wins), otherwise the greatest value, the earliest index on a tie
  auto better = [](float v, int i, float bvv, int bii) {
    if (bii == 0x7fffffff) return true;
    if (v != v) return !(bvv != bvv) || i < bii;
    if (bvv != bvv) return false;
    return v > bvv || (v == bvv && i < bii);
  };
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int i = tid; i < n; i += 1024) {
    const float v = E::f(logits[i]);
    if (better(v, i, best, idx)) { best = v; idx = i; }
  }
  bv[tid] = best; bi[tid] = idx;
  __syncthreads();
  for (int s_ = 512; s_ > 0; s_ >>= 1) {
    if (tid < s_) {
      const float v = bv[tid + s_];
      const int j = bi[tid + s_];
      if (j != 0x7fffffff && better(v, j, bv[tid], bi[tid])) { bv[tid] = v; bi[tid] = j; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t w = bi[0] == 0x7fffffff ? 0 : bi[0];
    next_tok[0] = w;
    if (tok) tok[0] = w;
    if (pos) pos[0] += 1;
  }
}

}  // namespace hqq

using namespace hqq;

static inline bool block_dtype_ok(int dtype, const char* who) {
  if (dtype == HQQ_F16 || dtype == HQQ_BF16) return true;
  set_error("%s: fp16 / bf16 only (dtype %d)", who, dtype);
  return false;
}
typedef const uint16_t* cu16;
typedef uint16_t* u16;

extern "C" {

int hqq_hip_add_rmsnorm(void* h, const void* delta, const void* weight, float eps, void* xn_out, int64_t rows, int64_t H, int dtype, void* stream) {
  clear_stale_error();
  if (!block_dtype_ok(dtype, "hqq_hip_add_rmsnorm")) return HQQ_ERR_UNSUPPORTED;
  if (!h || !weight || !xn_out || rows < 1 || H < 8 || H % 8 || rows > INT32_MAX || H > INT32_MAX) { set_error("hqq_hip_add_rmsnorm: bad arguments (H must be a multiple of 8)"); return HQQ_ERR_SHAPE; }
  if (!aligned16(h) || !aligned16(weight) || !aligned16(xn_out) || (delta && !aligned16(delta))) { set_error("hqq_hip_add_rmsnorm: pointers must be 16-byte aligned"); return HQQ_ERR_ALIGN; }
#define HQQ_NORM_GO(RPTV, BFV)                                                                                                                   \
  hipLaunchKernelGGL((add_rmsnorm_kernel<RPTV, BFV>), dim3(static_cast<unsigned>(rows)), dim3(512), 0, as_stream(stream), static_cast<u16>(h), static_cast<cu16>(delta), \
                     static_cast<cu16>(weight), eps, static_cast<u16>(xn_out), static_cast<int>(H))
  if (dtype == HQQ_BF16) {
    if (H <= 512 * 8) HQQ_NORM_GO(1, true);
    else if (H <= 512 * 8 * 2) HQQ_NORM_GO(2, true);
    else HQQ_NORM_GO(0, true);
  } else {
    if (H <= 512 * 8) HQQ_NORM_GO(1, false);
    else if (H <= 512 * 8 * 2) HQQ_NORM_GO(2, false);
    else HQQ_NORM_GO(0, false);
  }
#undef HQQ_NORM_GO
  return check_launch("hqq_hip_add_rmsnorm");
}

}  // extern "C"

// the batch count of a *_batched call: one grid dimension (y / z) of up to 65535 sequences
static inline bool batch_ok(int64_t batch, const char* who) {
  if (batch >= 1 && batch <= 65535) return true;
  set_error("%s: batch %lld outside [1, 65535]", who, (long long)batch);
  return false;
}

static int rope_cache_run(const char* who, bool shared, const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t batch, void* q_out,
                          void* k_cache, void* v_cache, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream) {
  clear_stale_error();
  if (!block_dtype_ok(dtype, who)) return HQQ_ERR_UNSUPPORTED;
  if (!batch_ok(batch, who)) return HQQ_ERR_SHAPE;
  if (!q || !k || !v || !cos || !sin || !pos_dev || !q_out || !k_cache || !v_cache || n_heads < 1 || n_kv_heads < 1 || head_dim < 2 || head_dim % 2 || cache_len < 1 ||
      (n_heads + n_kv_heads) * head_dim > INT32_MAX || cache_len > INT32_MAX) { set_error("%s: bad arguments", who); return HQQ_ERR_SHAPE; }
  const int64_t total = (n_heads + n_kv_heads) * (head_dim / 2);
  const int64_t cache_row = shared ? 0 : n_kv_heads * cache_len * head_dim;
#define HQQ_ROPE_GO(BFV)                                                                                                                          \
  hipLaunchKernelGGL(rope_cache_kernel<BFV>, dim3(static_cast<unsigned>((total + 255) / 256), static_cast<unsigned>(batch)), dim3(256), 0, as_stream(stream), \
                     static_cast<cu16>(q), static_cast<cu16>(k),                                                                                  \
                     static_cast<cu16>(v), static_cast<cu16>(cos), static_cast<cu16>(sin), pos_dev, static_cast<u16>(q_out), static_cast<u16>(k_cache),  \
                     static_cast<u16>(v_cache), static_cast<int>(n_heads), static_cast<int>(n_kv_heads), static_cast<int>(head_dim), static_cast<int>(cache_len), cache_row)
  if (dtype == HQQ_BF16) HQQ_ROPE_GO(true);
  else HQQ_ROPE_GO(false);
#undef HQQ_ROPE_GO
  return check_launch(who);
}

extern "C" {

int hqq_hip_rope_cache(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, void* q_out, void* k_cache,
                       void* v_cache, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream) {
  return rope_cache_run("hqq_hip_rope_cache", false, q, k, v, cos, sin, pos_dev, 1, q_out, k_cache, v_cache, n_heads, n_kv_heads, head_dim, cache_len, dtype, stream);
}

int hqq_hip_rope_cache_batched(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t batch, void* q_out,
                               void* k_cache, void* v_cache, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream) {
  return rope_cache_run("hqq_hip_rope_cache_batched", false, q, k, v, cos, sin, pos_dev, batch, q_out, k_cache, v_cache, n_heads, n_kv_heads, head_dim, cache_len, dtype, stream);
}

int hqq_hip_rope_cache_shared(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t rows, void* q_out,
                              void* k_cache, void* v_cache, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream) {
  return rope_cache_run("hqq_hip_rope_cache_shared", true, q, k, v, cos, sin, pos_dev, rows, q_out, k_cache, v_cache, n_heads, n_kv_heads, head_dim, cache_len, dtype, stream);
}

int hqq_hip_qknorm_rope_cache_batched(const void* q, const void* k, const void* v, const void* q_weight, const void* k_weight, float q_eps, float k_eps, const void* cos,
                                      const void* sin, const int64_t* pos_dev, int64_t batch, void* q_out, void* k_cache, void* v_cache, int64_t n_heads,
                                      int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream) {
  const char* who = "hqq_hip_qknorm_rope_cache_batched";
  clear_stale_error();
  if (!block_dtype_ok(dtype, who)) return HQQ_ERR_UNSUPPORTED;
  if (!batch_ok(batch, who)) return HQQ_ERR_SHAPE;
  if (!q || !k || !v || !q_weight || !k_weight || !cos || !sin || !pos_dev || !q_out || !k_cache || !v_cache || n_heads < 1 || n_kv_heads < 1 || head_dim < 2 ||
      head_dim % 2 || cache_len < 1 || !(q_eps >= 0.f) || !(k_eps >= 0.f) || n_heads > INT32_MAX || n_kv_heads > INT32_MAX || head_dim > INT32_MAX ||
      (n_heads + n_kv_heads) * head_dim > INT32_MAX || cache_len > INT32_MAX) {
    set_error("%s: bad arguments (head_dim even, eps >= 0)", who);
    return HQQ_ERR_SHAPE;
  }
  if (head_dim != 64 && head_dim != 128 && head_dim != 256) { set_error("%s: head_dim %lld not covered (64 / 128 / 256)", who, (long long)head_dim); return HQQ_ERR_UNSUPPORTED; }
  // (2-byte loads and stores, a wave's lanes on consecutive elements: no alignment beyond the element's is asked for)
  const dim3 grid(static_cast<unsigned>((n_heads + n_kv_heads + 3) / 4), static_cast<unsigned>(batch));
#define HQQ_QKN_GO(HDV, BFV)                                                                                                                     \
  hipLaunchKernelGGL((qknorm_rope_cache_kernel<HDV, BFV>), grid, dim3(256), 0, as_stream(stream), static_cast<cu16>(q), static_cast<cu16>(k), static_cast<cu16>(v), \
                     static_cast<cu16>(q_weight), static_cast<cu16>(k_weight), q_eps, k_eps, static_cast<cu16>(cos), static_cast<cu16>(sin), pos_dev,    \
                     static_cast<u16>(q_out), static_cast<u16>(k_cache), static_cast<u16>(v_cache), static_cast<int>(n_heads), static_cast<int>(n_kv_heads), \
                     static_cast<int>(cache_len))
  const bool bf = dtype == HQQ_BF16;
  if (head_dim == 64) { if (bf) HQQ_QKN_GO(64, true); else HQQ_QKN_GO(64, false); }
  else if (head_dim == 128) { if (bf) HQQ_QKN_GO(128, true); else HQQ_QKN_GO(128, false); }
  else { if (bf) HQQ_QKN_GO(256, true); else HQQ_QKN_GO(256, false); }
#undef HQQ_QKN_GO
  return check_launch(who);
}

int hqq_hip_bias_rope_cache_batched(const void* q, const void* k, const void* v, const void* q_bias, const void* k_bias, const void* v_bias, const void* cos,
                                    const void* sin, const int64_t* pos_dev, int64_t batch, void* q_out, void* k_cache, void* v_cache, int64_t n_heads,
                                    int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream) {
  const char* who = "hqq_hip_bias_rope_cache_batched";
  clear_stale_error();
  if (!block_dtype_ok(dtype, who)) return HQQ_ERR_UNSUPPORTED;
  if (!batch_ok(batch, who)) return HQQ_ERR_SHAPE;
  if (!q || !k || !v || !q_bias || !k_bias || !v_bias || !cos || !sin || !pos_dev || !q_out || !k_cache || !v_cache || n_heads < 1 || n_kv_heads < 1 || head_dim < 2 ||
      head_dim % 2 || cache_len < 1 || n_heads > INT32_MAX || n_kv_heads > INT32_MAX || head_dim > INT32_MAX || (n_heads + n_kv_heads) * head_dim > INT32_MAX ||
      cache_len > INT32_MAX) {
    set_error("%s: bad arguments (all three biases are required, head_dim even)", who);
    return HQQ_ERR_SHAPE;
  }
  const int64_t total = (n_heads + n_kv_heads) * (head_dim / 2);
#define HQQ_BROPE_GO(BFV)                                                                                                                         \
  hipLaunchKernelGGL(bias_rope_cache_kernel<BFV>, dim3(static_cast<unsigned>((total + 255) / 256), static_cast<unsigned>(batch)), dim3(256), 0, as_stream(stream), \
                     static_cast<cu16>(q), static_cast<cu16>(k), static_cast<cu16>(v), static_cast<cu16>(q_bias), static_cast<cu16>(k_bias),          \
                     static_cast<cu16>(v_bias), static_cast<cu16>(cos), static_cast<cu16>(sin), pos_dev, static_cast<u16>(q_out), static_cast<u16>(k_cache), \
                     static_cast<u16>(v_cache), static_cast<int>(n_heads), static_cast<int>(n_kv_heads), static_cast<int>(head_dim), static_cast<int>(cache_len))
  if (dtype == HQQ_BF16) HQQ_BROPE_GO(true);
  else HQQ_BROPE_GO(false);
#undef HQQ_BROPE_GO
  return check_launch(who);
}

int hqq_hip_silu_mul(const void* gate, const void* up, void* out, int64_t n, int dtype, void* stream) {
  clear_stale_error();
  if (!block_dtype_ok(dtype, "hqq_hip_silu_mul")) return HQQ_ERR_UNSUPPORTED;
  if (!gate || !up || !out || n < 8 || n % 8) { set_error("hqq_hip_silu_mul: bad arguments (n must be a multiple of 8)"); return HQQ_ERR_SHAPE; }
  if (!aligned16(gate) || !aligned16(up) || !aligned16(out)) { set_error("hqq_hip_silu_mul: pointers must be 16-byte aligned"); return HQQ_ERR_ALIGN; }
  const dim3 grid(static_cast<unsigned>((n / 8 + 255) / 256));
  if (dtype == HQQ_BF16) hipLaunchKernelGGL(silu_mul_kernel<true>, grid, dim3(256), 0, as_stream(stream), static_cast<cu16>(gate), static_cast<cu16>(up), static_cast<u16>(out), n);
  else hipLaunchKernelGGL(silu_mul_kernel<false>, grid, dim3(256), 0, as_stream(stream), static_cast<cu16>(gate), static_cast<cu16>(up), static_cast<u16>(out), n);
  return check_launch("hqq_hip_silu_mul");
}

static int attn_decode_run(const char* who, bool rope, bool shared, const void* q, const void* k_raw, const void* v_raw, const void* cosv, const void* sinv, const int64_t* pos_dev,
                           int64_t batch, void* k_cache, void* v_cache, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling,
                           int dtype, int64_t splits, void* workspace, size_t workspace_bytes, void* stream) {
  clear_stale_error();
  const AttnCall c{who, batch, n_heads, n_kv_heads, head_dim, cache_len, dtype, splits, workspace, workspace_bytes, out, stream};
  if (const int rc = attn_check(c, {q, k_cache, v_cache, pos_dev, out}, {q, k_cache, v_cache, out})) return rc;
  // this runner's own: the raw projections and the rotary tables of the ROPE kernel, which has no shared-cache form
  if (rope && (shared || !k_raw || !v_raw || !cosv || !sinv)) { set_error("%s: bad arguments (k, v, cos and sin are required)", who); return HQQ_ERR_SHAPE; }
  if (rope && (!aligned16(k_raw) || !aligned16(v_raw))) { set_error("%s: k and v must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  const int64_t cache_row = shared ? 0 : n_kv_heads * cache_len * head_dim;   // (shared: every row's queries on the one cache)
  const int lds = attn_lds_launch(c.HD(), cache_len, c.S());
  return attn_launch(c, [&](auto HDc, auto BFc) {
    auto go = [&](auto RPc) {
      constexpr auto kern = &attn_decode_kernel<decltype(HDc)::value, decltype(RPc)::value, decltype(BFc)::value>;
      static LdsRaised raised;   // (one per instantiation)
      if (const int rc = attn_raise_lds(raised, reinterpret_cast<const void*>(kern), lds, ATTN_LDS_MAX, who)) return rc;
      hipLaunchKernelGGL(kern, c.grid(batch), dim3(512), lds, as_stream(stream), static_cast<cu16>(q), static_cast<cu16>(k_cache), static_cast<cu16>(v_cache), pos_dev,
                         static_cast<u16>(out), static_cast<int>(n_heads), static_cast<int>(n_kv_heads), static_cast<int>(cache_len), scaling, static_cast<cu16>(k_raw),
                         static_cast<cu16>(v_raw), static_cast<cu16>(cosv), static_cast<cu16>(sinv), static_cast<u16>(k_cache), static_cast<u16>(v_cache), c.S(), c.ws(),
                         cache_row);
      return 0;
    };
    return rope ? go(std::true_type{}) : go(std::false_type{});
  });
}

size_t hqq_hip_attn_decode_workspace_bytes(int64_t n_heads, int64_t head_dim, int64_t splits) {
  return splits > 1 ? static_cast<size_t>(n_heads) * static_cast<size_t>(splits) * static_cast<size_t>(head_dim + 2) * sizeof(float) : 0;
}

int hqq_hip_attn_decode(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, void* out, int64_t n_heads, int64_t n_kv_heads,
                        int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace, size_t workspace_bytes, void* stream) {
  return attn_decode_run("hqq_hip_attn_decode", false, false, q, nullptr, nullptr, nullptr, nullptr, pos_dev, 1, const_cast<void*>(k_cache), const_cast<void*>(v_cache), out,
                         n_heads, n_kv_heads, head_dim, cache_len, scaling, dtype, splits, workspace, workspace_bytes, stream);
}

int hqq_hip_rope_attn_decode(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, void* k_cache, void* v_cache, void* out,
                             int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                             size_t workspace_bytes, void* stream) {
  return attn_decode_run("hqq_hip_rope_attn_decode", true, false, q, k, v, cos, sin, pos_dev, 1, k_cache, v_cache, out, n_heads, n_kv_heads, head_dim, cache_len, scaling, dtype,
                         splits, workspace, workspace_bytes, stream);
}

int hqq_hip_attn_decode_batched(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads,
                                int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return attn_decode_run("hqq_hip_attn_decode_batched", false, false, q, nullptr, nullptr, nullptr, nullptr, pos_dev, batch, const_cast<void*>(k_cache),
                         const_cast<void*>(v_cache), out, n_heads, n_kv_heads, head_dim, cache_len, scaling, dtype, splits, workspace, workspace_bytes, stream);
}

int hqq_hip_rope_attn_decode_batched(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t batch, void* k_cache,
                                     void* v_cache, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype,
                                     int64_t splits, void* workspace, size_t workspace_bytes, void* stream) {
  return attn_decode_run("hqq_hip_rope_attn_decode_batched", true, false, q, k, v, cos, sin, pos_dev, batch, k_cache, v_cache, out, n_heads, n_kv_heads, head_dim, cache_len,
                         scaling, dtype, splits, workspace, workspace_bytes, stream);
}

int hqq_hip_attn_decode_shared(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, int64_t rows, void* out, int64_t n_heads,
                               int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return attn_decode_run("hqq_hip_attn_decode_shared", false, true, q, nullptr, nullptr, nullptr, nullptr, pos_dev, rows, const_cast<void*>(k_cache),
                         const_cast<void*>(v_cache), out, n_heads, n_kv_heads, head_dim, cache_len, scaling, dtype, splits, workspace, workspace_bytes, stream);
}

}  // extern "C"

// the merging launch of a split decode-attention call over `heads` records; shared with the quantised-cache attention (kv_cache.hip), whose shares are these records
void hqq::launch_attn_combine(const float* ws, void* out, int64_t heads, int S, int HD, bool bf, hipStream_t st) {
  const dim3 cgrid(static_cast<unsigned>(heads));
  if (bf) hipLaunchKernelGGL(attn_combine_kernel<true>, cgrid, dim3(256), 0, st, ws, static_cast<u16>(out), S, HD);
  else hipLaunchKernelGGL(attn_combine_kernel<false>, cgrid, dim3(256), 0, st, ws, static_cast<u16>(out), S, HD);
}

static int token_prologue_run(const char* who, const int64_t* tok_dev, const int64_t* pos_dev, int64_t batch, const void* embed, int64_t vocab, int64_t H, const void* cos_tab,
                              const void* sin_tab, int64_t L, int64_t head_dim, void* h, void* cos, void* sin, void* mask, int dtype, void* stream) {
  clear_stale_error();
  if (!block_dtype_ok(dtype, who)) return HQQ_ERR_UNSUPPORTED;
  if (!batch_ok(batch, who)) return HQQ_ERR_SHAPE;
  if (!tok_dev || !pos_dev || !embed || !h || vocab < 1 || H < 8 || H % 8 || H > INT32_MAX || L < 1 || (cos_tab && (!sin_tab || !cos || !sin || head_dim < 1 || head_dim > INT32_MAX))) {
    set_error("%s: bad arguments (H a multiple of 8; cos / sin tables and outputs come together)", who);
    return HQQ_ERR_SHAPE;
  }
  if (!aligned16(embed) || !aligned16(h)) { set_error("%s: embed / h must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  const uint16_t ninf = dtype == HQQ_BF16 ? 0xFF80u : 0xFC00u;
  const int64_t work = (mask ? L : 0) > H / 8 ? (mask ? L : 0) : H / 8;
  const unsigned blocks = static_cast<unsigned>(work / 256 < 1 ? 1 : (work / 256 > 64 ? 64 : work / 256));
  hipLaunchKernelGGL(token_prologue_kernel, dim3(blocks, static_cast<unsigned>(batch)), dim3(256), 0, as_stream(stream), tok_dev, pos_dev, static_cast<cu16>(embed), vocab,
                     static_cast<int>(H), static_cast<cu16>(cos_tab), static_cast<cu16>(sin_tab), L, static_cast<int>(head_dim), static_cast<u16>(h), static_cast<u16>(cos),
                     static_cast<u16>(sin), static_cast<u16>(mask), static_cast<uint16_t>(0), ninf);
  return check_launch(who);
}

static int argmax_advance_run(const char* who, const void* logits, int64_t batch, int64_t n, int dtype, int64_t* next_tok_dev, int64_t* tok_dev, int64_t* pos_dev, void* stream) {
  clear_stale_error();
  if (!block_dtype_ok(dtype, who)) return HQQ_ERR_UNSUPPORTED;
  if (!batch_ok(batch, who)) return HQQ_ERR_SHAPE;
  if (!logits || !next_tok_dev || n < 1 || n > INT32_MAX - 1) { set_error("%s: bad arguments", who); return HQQ_ERR_SHAPE; }
  const dim3 grid(static_cast<unsigned>(batch));
  if (dtype == HQQ_BF16) hipLaunchKernelGGL(argmax_advance_kernel<true>, grid, dim3(1024), 0, as_stream(stream), static_cast<cu16>(logits), static_cast<int>(n), next_tok_dev, tok_dev, pos_dev);
  else hipLaunchKernelGGL(argmax_advance_kernel<false>, grid, dim3(1024), 0, as_stream(stream), static_cast<cu16>(logits), static_cast<int>(n), next_tok_dev, tok_dev, pos_dev);
  return check_launch(who);
}

extern "C" {

int hqq_hip_token_prologue(const int64_t* tok_dev, const int64_t* pos_dev, const void* embed, int64_t vocab, int64_t H, const void* cos_tab, const void* sin_tab, int64_t L,
                           int64_t head_dim, void* h, void* cos, void* sin, void* mask, int dtype, void* stream) {
  return token_prologue_run("hqq_hip_token_prologue", tok_dev, pos_dev, 1, embed, vocab, H, cos_tab, sin_tab, L, head_dim, h, cos, sin, mask, dtype, stream);
}

int hqq_hip_token_prologue_batched(const int64_t* tok_dev, const int64_t* pos_dev, int64_t batch, const void* embed, int64_t vocab, int64_t H, const void* cos_tab,
                                   const void* sin_tab, int64_t L, int64_t head_dim, void* h, void* cos, void* sin, void* mask, int dtype, void* stream) {
  return token_prologue_run("hqq_hip_token_prologue_batched", tok_dev, pos_dev, batch, embed, vocab, H, cos_tab, sin_tab, L, head_dim, h, cos, sin, mask, dtype, stream);
}

int hqq_hip_argmax_advance(const void* logits, int64_t n, int dtype, int64_t* next_tok_dev, int64_t* tok_dev, int64_t* pos_dev, void* stream) {
  return argmax_advance_run("hqq_hip_argmax_advance", logits, 1, n, dtype, next_tok_dev, tok_dev, pos_dev, stream);
}

int hqq_hip_argmax_advance_batched(const void* logits, int64_t batch, int64_t n, int dtype, int64_t* next_tok_dev, int64_t* tok_dev, int64_t* pos_dev, void* stream) {
  return argmax_advance_run("hqq_hip_argmax_advance_batched", logits, batch, n, dtype, next_tok_dev, tok_dev, pos_dev, stream);
}

}  // extern "C"
