// attn_decode_core.h — the one-row decode attention, stated once: its LDS layout, its device body and the host front of every decode-attention entry point.
//   device  attn_decode_body<HD, BF>: phases 1-3 over two row loaders.  attn_decode_kernel (block.hip) hands it loaders that read the dense cache,
//           attn_decode_kvq_kernel (kv_cache.hip) loaders that rebuild a packed row to T (kv_load8).  Everything behind a loader is this one text, so the
//           quantised-cache attention has the bits of the dense one on the dequantised cache by construction.
//   host    attn_check / attn_launch: the argument checks, the (head_dim, dtype) dispatch, the combine launch and the LDS-limit raise that block.hip,
//           kv_cache.hip and attn_tile.hip share; a runner keeps the checks that are its own.
// Translation units that use the body are compiled with -ffp-contract=off (block_math.h).
#pragma once
#include <initializer_list>

#include "block_math.h"

namespace hqq {

// ---- limits of every decode-attention entry point ----
constexpr int ATTN_MAX_KEYS = 30000, ATTN_MAX_SPLITS = 64, ATTN_MAX_ROWS = 65535;   // cache_len, splits, sequences / rows (one grid dimension)

// ---- the dynamic LDS block of the one-row kernels, in bytes: [16] fp32 reduction scratch | [HD] x 3 of T: the query, then (ROPE) the new key and the new
//      value — the quantised-cache kernel keeps the two unused slots, so both kernels ask for the same bytes | [8][HD] fp32, a partial output per wave |
//      [keys] fp32 scores, then probabilities ----
constexpr int attn_lds_qs() { return 16 * 4; }
constexpr int attn_lds_part(int HD) { return attn_lds_qs() + HD * 3 * 2; }
constexpr int attn_lds_sc(int HD) { return attn_lds_part(HD) + 8 * HD * 4; }
constexpr int attn_lds_bytes(int HD, int keys) { return attn_lds_sc(HD) + keys * 4; }
// what a launch asks for (the keys of the longest share + 8) and the limit its kernels are raised to above 48 KiB
inline int attn_lds_launch(int HD, int64_t cache_len, int S) { return attn_lds_bytes(HD, static_cast<int>((cache_len + S - 1) / S + 8)); }
constexpr int ATTN_LDS_MAX = attn_lds_bytes(256, ATTN_MAX_KEYS);

template <int HD>
struct AttnLds {
  float* red;
  uint16_t* qs;
  float* part;
  float* sc;
  __device__ __forceinline__ explicit AttnLds(uint8_t* smem)
      : red(reinterpret_cast<float*>(smem)), qs(reinterpret_cast<uint16_t*>(smem + attn_lds_qs())), part(reinterpret_cast<float*>(smem + attn_lds_part(HD))),
        sc(reinterpret_cast<float*>(smem + attn_lds_sc(HD))) {}
};

// ---- decode attention of workgroup (head h, share sp) over the n visible keys: 512 threads, the query already in lds.qs (the body's first barrier publishes
//      it).  krow(ch, j) / vrow(ch, j): a lane's 8 dims (16 bytes, chunk ch of the row's HD / 8) of key / value row j as T.
//      Phase 1: a wave instruction covers KPW = 512 / HD whole key rows (LPK = HD / 8 lanes per row; v_dot2 into fp32, the LPK partial dot products of a row
//      added by shuffles), scores into LDS, workgroup maximum.  Phase 2: exp(s - max) in place, workgroup sum.  Phase 3: the same row-per-lane-group walk over
//      the values, o += p V[j]; the row groups of a wave are added by shuffles, the 8 waves' partial vectors in wave order.  Deterministic: no atomics, fixed
//      orders.  Rows at or beyond n are never asked of a loader.
//      S > 1 (long caches): the workgroup attends over keys [k0, k1), a 1 / S share of the n visible ones, and parks (max, sum, unnormalised output) in record
//      h S + sp of ws; attn_combine_kernel (block.hip) merges the S shares in split order.  One workgroup per head streams 1.3 TB/s: 48 us at 4096 keys; eight
//      per head 19 (the 64 MB of cache at 3.4 TB/s + the two launches).  out / ws: those of this workgroup's sequence ----
template <int HD, bool BF, class KRow, class VRow>
__device__ __forceinline__ void attn_decode_body(const AttnLds<HD>& lds, int h, int sp, int n, int S, float scaling, uint16_t* __restrict__ out, float* __restrict__ ws,
                                                 KRow krow, VRow vrow) {
  using E = El<BF>;
  float* const red = lds.red;
  float* const part = lds.part;
  float* const sc = lds.sc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = (n + S - 1) / S;
  const int k0 = sp * chunk, k1 = (k0 + chunk < n) ? k0 + chunk : n;
  __syncthreads();
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  typedef __bf16 b2 __attribute__((ext_vector_type(2)));
  // phase 1 (a lane per key read 64 different lines per instruction and thrashed the L1: whole rows per instruction are 1 KiB of consecutive memory)
  constexpr int LPK = HD / 8, KPW = 64 / LPK, STEP = 8 * KPW;
  const int sub = lane / LPK, ch = lane - sub * LPK;
  const u32x4 qf = reinterpret_cast<const u32x4*>(lds.qs)[ch];
  auto score = [&](const u32x4& kv) -> float {
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t qe = qf[e], ke = kv[e];   // (a bit_cast of an ext-vector ELEMENT reads element 0: copy to a scalar first)
      if constexpr (BF) acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(b2, qe), __builtin_bit_cast(b2, ke), acc, false);
      else acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, qe), __builtin_bit_cast(h2, ke), acc, false);
    }
#pragma unroll
    for (int off = 1; off < LPK; off <<= 1) acc += __shfl_xor(acc, off, 64);
    return acc * scaling;
  };
  float mx = -INFINITY;
  {
    int j = k0 + wave * KPW + sub;
    for (; j + 3 * STEP < k1; j += 4 * STEP) {
      u32x4 k4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) k4[u] = krow(ch, j + u * STEP);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float sv = score(k4[u]);
        if (ch == 0) sc[j + u * STEP - k0] = sv;
        mx = fmaxf(mx, sv);
      }
    }
    // (the shuffles of score() need every lane of a row group: rows past the end are computed on row k1 - 1 and dropped)
    for (; j - sub < k1; j += STEP) {
      const bool live = j < k1;
      const float sv = score(krow(ch, live ? j : k1 - 1));
      if (live) {
        if (ch == 0) sc[j - k0] = sv;
        mx = fmaxf(mx, sv);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < 8; ++w) mx = fmaxf(mx, red[w]);
  // phase 2
  float sum = 0.f;
  for (int j = tid; j < k1 - k0; j += 512) {
    const float pj = __expf(sc[j] - mx);
    sc[j] = pj;
    sum += pj;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0) red[8 + wave] = sum;
  __syncthreads();
  sum = ((red[8] + red[9]) + (red[10] + red[11])) + ((red[12] + red[13]) + (red[14] + red[15]));
  // phase 3: a wave takes rows k0 + KPW wave + sub, stepping 8 KPW, four instructions in flight
  float o8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o8[e] = 0.f;
  auto fold = [&](const u32x4& v, float pj) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t w = v[e];   // (element copied to a scalar before its halves are taken)
      o8[2 * e] = fmaf(pj, E::f(static_cast<uint16_t>(w & 0xFFFFu)), o8[2 * e]);
      o8[2 * e + 1] = fmaf(pj, E::f(static_cast<uint16_t>(w >> 16)), o8[2 * e + 1]);
    }
  };
  int j = k0 + wave * KPW + sub;
  for (; j + 3 * STEP < k1; j += 4 * STEP) {
    u32x4 v4[4];
    float p4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { v4[u] = vrow(ch, j + u * STEP); p4[u] = sc[j + u * STEP - k0]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) fold(v4[u], p4[u]);
  }
  for (; j < k1; j += STEP) fold(vrow(ch, j), sc[j - k0]);
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] += __shfl_xor(o8[e], off, 64);
  if (sub == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) part[wave * HD + ch * 8 + e] = o8[e];
  }
  __syncthreads();
  if (tid < HD) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) t += part[w * HD + tid];
    if (S == 1) {
      out[static_cast<int64_t>(h) * HD + tid] = E::r(t / sum);
    } else {
      float* rec = ws + (static_cast<int64_t>(h) * S + sp) * (HD + 2);   // (an empty share leaves max = -inf, sum = 0, output 0)
      rec[2 + tid] = t;
      if (tid == 0) { rec[0] = mx; rec[1] = sum; }
    }
  }
}

// ---- the host front ----
// one decode-attention call as its entry point received it; rows: the sequences of a *_batched call, the rows of a *_shared / *_tiled one (1 otherwise)
struct AttnCall {
  const char* who;
  int64_t rows, n_heads, n_kv_heads, head_dim, cache_len;
  int dtype;
  int64_t splits;
  void* workspace;
  size_t workspace_bytes;
  void* out;
  void* stream;
  int HD() const { return static_cast<int>(head_dim); }
  int S() const { return static_cast<int>(splits); }
  bool bf() const { return dtype == HQQ_BF16; }
  float* ws() const { return static_cast<float*>(workspace); }
  dim3 grid(int64_t z) const { return dim3(static_cast<unsigned>(n_heads), static_cast<unsigned>(splits), static_cast<unsigned>(z)); }
};

// the checks every entry shares, 0 or the error code with c.who's message: `need` must not be null, `align` must be 16-byte aligned.  A runner with a stricter
// rule of its own (kv_check, the tiled kernel's rows) applies it first, so its code is the one a caller sees
static inline int attn_check(const AttnCall& c, std::initializer_list<const void*> need, std::initializer_list<const void*> align) {
  const char* who = c.who;
  if (c.dtype != HQQ_F16 && c.dtype != HQQ_BF16) { set_error("%s: fp16 / bf16 only (dtype %d)", who, c.dtype); return HQQ_ERR_UNSUPPORTED; }
  if (c.rows < 1 || c.rows > ATTN_MAX_ROWS) { set_error("%s: batch %lld outside [1, %d]", who, (long long)c.rows, ATTN_MAX_ROWS); return HQQ_ERR_SHAPE; }
  bool ok = c.n_heads >= 1 && c.n_kv_heads >= 1 && c.n_heads % c.n_kv_heads == 0 && c.cache_len >= 1 && c.cache_len <= ATTN_MAX_KEYS && c.n_heads <= INT32_MAX &&
            c.rows * c.n_heads <= INT32_MAX;
  for (const void* p : need) ok = ok && p;
  if (!ok) { set_error("%s: bad arguments (a null pointer, cache_len outside [1, %d], or n_heads no multiple of n_kv_heads)", who, ATTN_MAX_KEYS); return HQQ_ERR_SHAPE; }
  if (c.head_dim != 64 && c.head_dim != 128 && c.head_dim != 256) { set_error("%s: head_dim %lld not covered (64 / 128 / 256)", who, (long long)c.head_dim); return HQQ_ERR_UNSUPPORTED; }
  for (const void* p : align)
    if (!aligned16(p)) { set_error("%s: q, out and the caches must be 16-byte aligned", who); return HQQ_ERR_ALIGN; }
  if (c.splits < 1 || c.splits > ATTN_MAX_SPLITS) { set_error("%s: splits must be 1..%d (got %lld)", who, ATTN_MAX_SPLITS, (long long)c.splits); return HQQ_ERR_SHAPE; }
  // (the records of rows * n_heads heads: hqq_hip_attn_decode_workspace_bytes(rows * n_heads, ...))
  if (c.splits > 1 && (!c.workspace || c.workspace_bytes < static_cast<size_t>(c.rows * c.n_heads) * c.S() * (c.HD() + 2) * sizeof(float))) {
    set_error("%s: %lld splits need a workspace of hqq_hip_attn_decode_workspace_bytes(rows * n_heads, ...) bytes", who, (long long)c.splits);
    return HQQ_ERR_SHAPE;
  }
  return 0;
}

// f(HD, BF) as integral constants, for a covered head_dim
template <class F>
static inline void attn_dispatch(int64_t hd, bool bf, F&& f) {
  auto on_bf = [&](auto HDc) { if (bf) f(HDc, std::true_type{}); else f(HDc, std::false_type{}); };
  if (hd == 64) on_bf(std::integral_constant<int, 64>{});
  else if (hd == 128) on_bf(std::integral_constant<int, 128>{});
  else on_bf(std::integral_constant<int, 256>{});
}

// a launch of `lds` dynamic bytes above the default 48 KiB needs kern's limit raised (to lds_max, once per device); raised: static in the caller, one per instantiation
static inline int attn_raise_lds(LdsRaised& raised, const void* kern, int lds, int lds_max, const char* who) {
  return lds > 48 * 1024 ? raise_lds_limit(raised, kern, lds_max, who) : 0;
}

// behind the attention kernel's launch (rc: what starting it gave): the shares of a split call (records of head r n_heads + h, the offset of output row r,
// head h in a dense [rows, n_heads, HD] output) are merged, and the launches checked
static inline int attn_finish(const AttnCall& c, int rc) {
  if (rc) return rc;
  if (c.S() > 1) launch_attn_combine(c.ws(), c.out, c.rows * c.n_heads, c.S(), c.HD(), c.bf(), as_stream(c.stream));
  return check_launch(c.who);
}

// a checked call's launches: launch(HDc, BFc) -> 0 or an error code starts the attention kernel of that instantiation, then attn_finish.  (A call on the
// quantised cache dispatches on the width too: kv_dispatch in kv_load.h, then attn_finish)
template <class Launch>
static inline int attn_launch(const AttnCall& c, Launch&& launch) {
  int rc = 0;
  attn_dispatch(c.head_dim, c.bf(), [&](auto HDc, auto BFc) { rc = launch(HDc, BFc); });
  return attn_finish(c, rc);
}

}  // namespace hqq
