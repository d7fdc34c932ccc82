/*
 * include/hqq_hip.h — C ABI of libhqq_hip.so, the MI355X (gfx950) implementation of HQQ's two hot paths.
 *
 * Boundary rules:
 *   - plain pointers and sizes only; no torch / ATen types cross this ABI.
 *   - the caller owns every buffer (inputs, outputs, workspace); the library never allocates or
 *     frees device memory, keeps no pointer after a call returns and holds no per-process mode:
 *     whatever selects a kernel variant is a per-call `opts` bit (HQQ_OPT_*); no environment
 *     variable is read.
 *   - every function enqueues on the given hipStream_t (passed as void*; NULL = legacy default
 *     stream) and returns immediately; there is no host synchronisation inside.
 *   - return value: 0 on success; >0 a hipError_t from the launch; <0 an argument error
 *     (HQQ_ERR_*).  hqq_hip_last_error() gives a thread-local message.  Nothing throws.
 *   - device pointers must be 16-byte aligned and dense (contiguous).
 *
 * Each entry point cites the reference interface it replaces (mobiusml/hqq v0.2.8.post1):
 * the pybind module `hqq_aten` (hqq/kernels/hqq_aten_cuda.cpp:57-73) and the PyTorch code of
 * hqq/core/{bitpack,quantize,optimize}.py that HQQBackend.PYTORCH runs.
 */
#ifndef HQQ_HIP_H
#define HQQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HQQ_HIP_ABI_VERSION 9

/* element types of activations / meta / outputs ("compute_dtype" in the reference) */
enum { HQQ_F32 = 0, HQQ_F16 = 1, HQQ_BF16 = 2, HQQ_U8 = 3 };

/* argument errors */
enum {
  HQQ_ERR_NBITS = -1,      /* nbits not in {8,4,3,2,1}                                   */
  HQQ_ERR_SHAPE = -2,      /* sizes inconsistent with the packing / group size            */
  HQQ_ERR_DTYPE = -3,      /* dtype code not supported by this entry point                */
  HQQ_ERR_UNSUPPORTED = -4,/* valid HQQ configuration this kernel does not cover (caller decides what to do) */
  HQQ_ERR_WORKSPACE = -5,  /* workspace too small / NULL                                  */
  HQQ_ERR_ALIGN = -6       /* pointer not 16-byte aligned                                 */
};

int hqq_hip_abi_version(void);
const char* hqq_hip_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * BitPack  — hqq/core/bitpack.py:14-144 ; hqq_aten.unpack_{8,4,3,2,1}bit_* (hqq_aten_cuda.cpp:57-73,
 * kernels hqq_aten_cuda_kernel.cu:81-106,159-188,244-276,337-374).
 * Layout: `per` row-slabs of the unpacked [rows, cols] matrix share one packed element, slab 0
 * most significant: per = 1/2/4/8 for 8/4/2/1-bit into uint8, per = 10 for 3-bit into int32 with
 * rows zero padded to 10*ceil(rows/10).
 * ------------------------------------------------------------------------------------------- */
/* rows of the packed tensor for `rows` unpacked rows; HQQ_ERR_SHAPE if rows % per != 0 (torch raises there) */
int64_t hqq_hip_packed_rows(int nbits, int64_t rows);

/* U [rows, cols] uint8 (in_dtype HQQ_U8) or float32 holding integers (HQQ_F32, the solver's W_q)
 * -> out [packed_rows, cols] uint8 / int32(3-bit).  BitPack.pack_* */
int hqq_hip_pack(int nbits, const void* U, int in_dtype, int64_t rows, int64_t cols, void* out, void* stream);

/* packed [packed_rows, cols] -> out [per*packed_rows, cols] of out_dtype (HQQ_U8/F16/BF16/F32).
 * BitPack.unpack_*(W_q, dtype) ; hqq_aten.unpack_* */
int hqq_hip_unpack(int nbits, const void* packed, int64_t packed_rows, int64_t cols, void* out, int out_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Quantizer.dequantize — hqq/core/quantize.py:183-199 ; hqq_aten.dequantize(W_q, scale, zero, N, K,
 * group_size, nbits, axis, packing) (hqq_aten_cuda.cpp:32-54, axis=0 only there; both axes here).
 *   out[N,K] = ((unpack(Wq)[:N*K/gs] - zero) * scale).reshape(N,K), two roundings in `dtype`.
 * scale/zero: [N*K/group_size] elements of `dtype`.  group_size = elements per (scale,zero).
 * axis=1: unpacked matrix is [N*K/gs, gs];  axis=0: [gs, N*K/gs].
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_dequantize(int nbits, const void* Wq, const void* scale, const void* zero, void* out,
                       int64_t N, int64_t K, int64_t group_size, int axis, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * HQQLinear.forward (quantize.py:880-898 forward_pytorch / matmul; patching.py:82-86) fused:
 *   y[M,N] = x[M,K] @ dequantize(Wq)^T (+ bias[N]),  axis=1 layout, dequantised weights bit-identical
 *   to hqq_hip_dequantize, fp32 accumulation, one rounding to `dtype` (+ one for the bias add).
 * hqq_hip_gemv : small M (decode), HBM-bandwidth bound (MFMA only as a free dot-product unit).  1 <= M <= HQQ_GEMV_MAX_M
 * hqq_hip_gemm : large M (prefill), MFMA f16/bf16.                          any M >= 1
 * hqq_hip_forward picks one of the two by M; the routes below say which kernel serves a call.  Anything uncovered -> HQQ_ERR_UNSUPPORTED
 * (the caller may compose hqq_hip_dequantize + its own GEMM).
 * Workspace: launches of 5..64 rows that split K, and 3-bit launches of >= 19 MB of packed weights, park fp32 partial sums (and
 * arrival counters) in a caller-owned workspace of hqq_hip_gemv_workspace_bytes(...) bytes (0 = this call needs none; then
 * workspace may be NULL).  Contract: 16-byte aligned device memory, not shared by calls that may run concurrently.  Only its first
 * 256 KiB — the arrival counters — must be ZERO when a call starts: the caller clears them once when allocating the buffer, and every
 * call leaves them zero again (only HQQ_ROUTE_SKINNY uses them; every other route keeps out of them).  What lies behind them is
 * unspecified on entry and on return: every call writes each partial sum before it reads it, so no result depends on what the buffer
 * held — routes may alternate on one buffer.  A larger workspace than asked for is fine: one buffer sized for the largest launch serves
 * a whole model.
 *
 * Routes: which kernel serves a call.  One planner in the library decides it for every entry point and query; hqq_hip_forward_route asks it
 * for hqq_hip_forward (n_layers = 1) or a group (hqq_hip_gemv_grouped / hqq_hip_gemm_grouped) without launching: a route, or the negative
 * HQQ_ERR_* the call returns (message in hqq_hip_last_error()).  The 3-bit stream layout is asked as itself (nbits 3, HQQ_OPT_W3S).
 *   1 ROWWISE      1..4 rows (FACTORED 1..16, 8 per launch); nbits 8/4/2/1, fp16 (bf16: 4/2), gs % 16 == 0, K % 16 == 0, x fits LDS
 *   2 ROWWISE_W3S  1..4;  stream layout, fp16 / bf16, gs 64, N % 2 == 0
 *   3 GEMV3_ROWS   1..4;  3-bit container, fp16, gs 64, a row's groups within one slab, x fits LDS
 *   4 GEMV3_SLABS  the same layers from 19 MB of packed weights (HQQ_OPT_GEMV3_ROWWISE / _SLABS force one); workspace
 *   5 MFMA16       5..16, exact weights; nbits 8/4/2/1, fp16, K % 64 == 0
 *   6 SKINNY       5..64 (FACTORED 9..64); nbits 8/4/2 or stream layout, fp16 / bf16, gs 64, K % 256 == 0, K >= 512; workspace
 *   7 GEMM_PIPE    beyond; nbits 8/4/2 or stream layout, fp16 / bf16, gs 64, K % 128 == 0, (N / per) % 4 == 0; workspace
 *   8 GEMM_TILE    beyond, or with HQQ_OPT_GEMM_REGTILE / _CLASSIC; nbits 4/2, fp16, gs % 16 == 0, K % 64 == 0, N % (4 per) == 0
 * Every route needs N % per == 0.  hqq_hip_gemv serves 1-6, hqq_hip_gemm 7-8; hqq_hip_forward takes hqq_hip_gemv up to HQQ_GEMV_MAX_M rows
 * (3-bit: 4) and on skinny shapes.  "workspace": parks partial sums when the plan splits K.
 * ------------------------------------------------------------------------------------------- */
enum { HQQ_ROUTE_ROWWISE = 1, HQQ_ROUTE_ROWWISE_W3S, HQQ_ROUTE_GEMV3_ROWS, HQQ_ROUTE_GEMV3_SLABS, HQQ_ROUTE_MFMA16, HQQ_ROUTE_SKINNY,
       HQQ_ROUTE_GEMM_PIPE, HQQ_ROUTE_GEMM_TILE };
int hqq_hip_forward_route(int nbits, int n_layers, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype, uint32_t opts);
#define HQQ_GEMV_MAX_M 16
#define HQQ_GEMV_MAX_M_SKINNY 64   /* HQQ_ROUTE_SKINNY */
#define HQQ_GEMV_MAX_GROUP 4
/* per-call options */
#define HQQ_OPT_FACTORED       1u   /* decode arithmetic: the group affine map is factored out of the dot product and applied in fp32
                                       (no per-weight fp16 rounding: NOT the reference's weights; results differ from it by less than its
                                       own weight-rounding noise).  M <= 8.  Default (bit clear): every weight is rebuilt as
                                       round16(round16(q - z) * s), bit-identical to hqq_hip_dequantize / Quantizer.dequantize. */
#define HQQ_OPT_META_SCALABLE  2u   /* the caller asserts hqq_hip_meta_check() returned 0 failing groups for EVERY layer of the call: the
                                       exact rebuild may then use its three-op form (same bits, ~25 % less VALU work).  fp16. */
#define HQQ_OPT_GEMV3_ROWWISE  4u   /* 3-bit decode: force the row-per-wave kernel (tests / tuning) */
#define HQQ_OPT_GEMV3_SLABS    8u   /* 3-bit decode: force the slab-sharing kernel (needs workspace) */
#define HQQ_OPT_GEMM_REGTILE  16u   /* prefill: the register-tile variant of the fused GEMM */
#define HQQ_OPT_GEMM_CLASSIC  32u   /* fused GEMM: the plain output-tile kernels for every M (tests / tuning; default: the pipelined split-K
                                       kernel up to 1024 rows) */
#define HQQ_OPT_SKINNY_KS(n) ((uint32_t)(n) << 24)   /* 5..64 rows, and the split-K fused GEMM: force n K-splits (tuning; 0 = built-in rule) */
#define HQQ_OPT_GEMM_NARROW  64u   /* pipelined fused GEMM: force 4 waves per workgroup (64 packed rows per tile) — tuning */
#define HQQ_OPT_GEMM_WIDE   128u   /* pipelined fused GEMM: force 8 waves per workgroup (128 packed rows per tile) — tuning */
#define HQQ_OPT_GEMM_NOHYBRID 256u  /* pipelined fused GEMM: never split only the last round of tiles (tuning) */
#define HQQ_OPT_SKINNY_WIDE 512u  /* 5..64 rows: force the 64-packed-row tile for launches the 32-row tile would serve (tests / tuning) */
#define HQQ_OPT_W3S        1024u  /* nbits = 3: Wq is the 3-bit STREAM layout written by hqq_hip_w3s_pack (below), not the reference container */
#define HQQ_OPT_ALL (2047u | (255u << 24))
/* Which groups of a layer can NOT take the three-op exact rebuild: (zero, scale) pairs for which zero * 2^-J is inexact in fp16,
 * |zero| > 2^15 or scale * 2^J overflows (J = 9 - bit offset of the row's slab).  Writes the count to *fail_count (device memory,
 * uint32; the call clears it first).  Run once per layer when it is prepared; pass HQQ_OPT_META_SCALABLE only if it came out 0.
 * scale / zero as in hqq_hip_dequantize, axis = 1, fp16.  (No reference counterpart: the reference always does two torch ops.) */
int hqq_hip_meta_check(int nbits, const void* scale, const void* zero, int64_t N, int64_t K, int64_t group_size, int dtype,
                       uint32_t* fail_count, void* stream);
/* ---------------------------------------------------------------------------------------------
 * The 3-bit STREAM layout (ABI 5; csrc/w3s.h).  BitPack.pack_3bit_32 (hqq/core/bitpack.py:69-91) ORs ten row slabs of the level
 * matrix into one int32 with a slab height that is not a multiple of a row's groups: a word mixes ten unrelated output rows.  Like
 * every optimised backend of the reference (hqq/backends/torchao.py:202-241, marlin.py:74-123: re-layout when a layer is patched),
 * HQQLinearHIP converts the container ONCE into [N/2, K/16, 3] uint32 — packed row p = output rows p and p + N/2, 12 bytes = 16 k of
 * both, exactly 3 bits per level — which the decode / GEMM kernels stream like a 4-bit layer (pass HQQ_OPT_W3S with nbits = 3).
 * scale / zero are unchanged.  hqq_hip_w3s_unpack restores the reference's container bit for bit (state_dict(), dequantize()).
 * Needs group_size 64 layers: N % 2 == 0, K % 64 == 0.  Wq_ref: [ceil(N K / 640), 64] int32; w3s: N K 3 / 8 bytes.
 * hqq_hip_w3s_meta_check: hqq_hip_meta_check for a layer in this layout (every group: zero 2^-9 exact, scale 2^9 finite), fp16.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_w3s_pack(const void* Wq_ref, void* w3s_out, int64_t N, int64_t K, void* stream);
int hqq_hip_w3s_unpack(const void* w3s, void* Wq_ref_out, int64_t N, int64_t K, void* stream);
int hqq_hip_w3s_meta_check(const void* scale, const void* zero, int64_t N, int64_t K, uint32_t* fail_count, void* stream);
size_t hqq_hip_gemv_workspace_bytes(int nbits, int n_layers, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype, uint32_t opts);
int hqq_hip_gemv(int nbits, const void* x, const void* Wq, const void* scale, const void* zero, const void* bias,
                 void* y, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace, size_t workspace_bytes,
                 void* stream);
/* Horizontal fusion of up to HQQ_GEMV_MAX_GROUP layers that consume the SAME activation rows x[M,K] (q/k/v, gate/up,
 * experts of one token ...): one launch streams all their packed rows; layer i writes y[i][M, N[i]].  Every per-layer
 * argument is a host array of n_layers device pointers / sizes (read during the call, not kept); bias may be NULL or
 * hold NULL entries.  All layers share K, group_size, nbits and dtype.  hqq_hip_gemv is the n_layers = 1 case.
 * (The reference has no counterpart: HQQLinear.forward is per layer, quantize.py:880-898.) */
int hqq_hip_gemv_grouped(int nbits, int n_layers, const void* x, const void* const* Wq, const void* const* scale,
                         const void* const* zero, const void* const* bias, void* const* y, const int64_t* N,
                         int64_t M, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace, size_t workspace_bytes,
                         void* stream);
/* ---------------------------------------------------------------------------------------------
 * One exchange point of a column-sharded decode step (ABI 4; csrc/exchange.hip), one activation row, without a collective library.
 * The reference has no multi-GPU path for HQQLinear.forward (quantize.py:880-898); the shard is SURVEY.md section 8e's: rank r holds the
 * packed-row block r of every layer and computes, per slab s, the output columns s N/per + [r n', (r + 1) n'), n' = N / (per P).
 * This call stores the rank's slices y_loc[j] ([1, N_loc[j]], local slab-major order) straight into EVERY rank's full row of layer j
 * at those columns — peers' rows are device pointers the caller obtained with hipIpcOpenMemHandle (stores travel over xGMI) — writes
 * the exchange's generation (how often this point has been used: counted on the device, so it counts under graph replay too) into this rank's
 * flag word of every rank's flag block and waits until all `world` flag words of its own block have reached it.  Flags only grow: one that
 * arrives after a wait gave up cannot satisfy the next use of the point.  When the
 * kernel has finished, this rank's full rows are complete and in the reference's column order; the next kernel in stream order may
 * read them.  Capturable.  One launch, `world` workgroups.
 *   full    [world * n_layers] pointers: full[p * n_layers + j] = rank p's [1, N_loc[j] * world] row of layer j (p == rank: local)
 *   flags   [world] pointers: rank p's flag block of THIS point: HQQ_EXCHANGE_MAX_RANKS + 1 uint32 words (a flag word per rank, then the
 *           rank's own launch-ticket word), all zero before the first use and only reset collectively (every rank, between two barriers);
 *           fine-grained / uncached device memory is the right kind for them and for the rows (peers write while a local kernel polls)
 *   status  one local uint32: a wait that gives up after spin_limit polls (0 = 4 Mi, seconds) writes 1 + the missing rank there
 *           and returns — outputs of that exchange undefined, reported, never a hang; sticky until the caller clears it
 * Re-use rule: consecutive exchanges on a stream must alternate between at least two points (flag block + rows); a decoder block
 * has four.  Every rank must issue the same sequence of points.  dtype F16 / BF16; nbits picks `per` (3-bit shards: per = 1).
 * ------------------------------------------------------------------------------------------- */
#define HQQ_EXCHANGE_MAX_RANKS 16
#define HQQ_EXCHANGE_MAX_ROWS 64   /* ABI 6: M activation rows per exchange (a decode batch): y_loc[j] is [M, N_loc[j]], the full row sets [M, N_loc[j] * world]; row m of a
                                      rank's slab run lands at the same columns of the peers' row m (strided slab writes), so a batch needs no un-permute either */
int hqq_hip_exchange(int n_layers, const void* const* y_loc, const int64_t* N_loc, int64_t M, int nbits, int dtype, int world, int rank,
                     void* const* full, void* const* flags, void* status, uint32_t spin_limit, void* stream);
/* ---------------------------------------------------------------------------------------------
 * The steps either side of the GEMVs in a decode step (ABI 5; csrc/block.hip).  The reference's headline is the
 * tok/s of its generate loop (hqq/utils/generation_hf.py:117-540, Readme.md:153), whose decoder block around HQQLinear.forward is HF's
 * eager code: ~25 small kernels per block.  These three restate the HF modules' arithmetic rounding for rounding (transformers
 * models/llama/modeling_llama.py: LlamaRMSNorm.forward, apply_rotary_pos_emb, LlamaMLP.forward; cache_utils.StaticLayer.update), fp16 or bf16 (T below; bf16 ops = float arithmetic + one rounding per op, as torch evaluates them):
 *   hqq_hip_add_rmsnorm  h[rows, H] += delta (if delta != NULL: the residual add, one rounding), then xn = weight * T(float(h) * rsqrt(mean(h^2) + eps))
 *   hqq_hip_rope_cache   q_out[n_heads, hd] = (q * cos) + (rotate_half(q) * sin); the same for k, written with v into the caches
 *                        [n_kv_heads, cache_len, hd] at position *pos_dev (device memory: the call is graph-replay safe)
 *   hqq_hip_silu_mul     out[n] = T(silu(gate)) * up
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_add_rmsnorm(void* h, const void* delta, const void* weight, float eps, void* xn_out, int64_t rows, int64_t H, int dtype, void* stream);
int hqq_hip_rope_cache(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, void* q_out, void* k_cache,
                       void* v_cache, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream);
int hqq_hip_silu_mul(const void* gate, const void* up, void* out, int64_t n, int dtype, void* stream);
/* hqq_hip_rope_cache for `batch` sequences (batch convention: hqq_hip_token_prologue_batched below): q / q_out [batch, n_heads, hd],
 * k / v [batch, n_kv_heads, hd], cos / sin [batch, hd], caches [batch, n_kv_heads, cache_len, hd] (HF's StaticCache tensors of that batch), pos_dev
 * int64[batch]; sequence b's key / value go to its own cache row at pos_dev[b]; a position outside [0, cache_len) writes nothing, as in the batch-1 call. */
int hqq_hip_rope_cache_batched(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t batch, void* q_out,
                               void* k_cache, void* v_cache, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream);
/* hqq_hip_rope_cache_batched with a per-head RMSNorm of q and k in front of the rotary embedding: what Qwen3Attention.forward does between its
 * projections and the cache update (transformers models/qwen3/modeling_qwen3.py: query_states = q_norm(q_proj(x).view(..., head_dim)), key_states =
 * k_norm(...), then apply_rotary_pos_emb and past_key_values.update).  Qwen3RMSNorm.forward's roundings, per head of head_dim elements:
 * n = weight * T(float(x) * rsqrt(mean(x^2) + eps)), the product in T — q_weight / k_weight [head_dim] in T, q_eps / k_eps the two modules' own
 * variance_epsilon (>= 0) —; hqq_hip_rope_cache's arithmetic on n; v is copied unchanged.  Shapes, positions and the rule for a position outside
 * [0, cache_len) (nothing is written to the caches, q_out still is) as hqq_hip_rope_cache_batched.  The fp32 sum of squares is taken in a fixed order:
 * two calls on the same inputs give the same bits.  head_dim 64 / 128 / 256 (other even values: HQQ_ERR_UNSUPPORTED; odd: HQQ_ERR_SHAPE), fp16 / bf16
 * (other dtypes: HQQ_ERR_UNSUPPORTED); element-aligned pointers suffice.  Every check is made before anything is launched.
 * The symbol was added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits. */
int hqq_hip_qknorm_rope_cache_batched(const void* q, const void* k, const void* v, const void* q_weight, const void* k_weight, float q_eps, float k_eps, const void* cos,
                                      const void* sin, const int64_t* pos_dev, int64_t batch, void* q_out, void* k_cache, void* v_cache, int64_t n_heads,
                                      int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream);
/* hqq_hip_rope_cache_batched with the three projection biases added in front: what Qwen2Attention.forward's biased q_proj / k_proj / v_proj give on top
 * of bias-free linear launches (transformers models/qwen2/modeling_qwen2.py).  q' = q + q_bias, k' = k + k_bias, v' = v + v_bias — q_bias
 * [n_heads * head_dim], k_bias / v_bias [n_kv_heads * head_dim], dense, in T, shared by every sequence, all three required.  Rounding contract: each add
 * is ONE rounding in T, the `out += bias` the decode kernels make on a rounded matmul result (a native half add for fp16; bf16: the fp32 sum of the two
 * values rounded to nearest even); then hqq_hip_rope_cache's arithmetic on q' / k'; v' goes to the cache.  The result is bit for bit that of
 * hqq_hip_gemv_grouped with the biases followed by hqq_hip_rope_cache_batched.  Shapes, positions and the rule for a position outside [0, cache_len)
 * (nothing is written to the caches, q_out still is) as hqq_hip_rope_cache_batched.  Any even head_dim (odd or < 2: HQQ_ERR_SHAPE), fp16 / bf16 (other
 * dtypes: HQQ_ERR_UNSUPPORTED); element-aligned pointers suffice; no workspace; deterministic.  Every check is made before anything is launched.
 * The symbol was added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits. */
int hqq_hip_bias_rope_cache_batched(const void* q, const void* k, const void* v, const void* q_bias, const void* k_bias, const void* v_bias, const void* cos,
                                    const void* sin, const int64_t* pos_dev, int64_t batch, void* q_out, void* k_cache, void* v_cache, int64_t n_heads,
                                    int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream);
/* The per-token work either side of the decoder blocks (ABI 7; hqq/utils/generation_hf.py:405-540: embedding lookup, the rotary table's row, the causal mask of one query in
 * front; argmax, token hand-over, position increment behind) as ONE launch each — copies and compares only, bit-identical to the torch ops they replace:
 *   hqq_hip_token_prologue  h[H] = embed[*tok_dev]; cos / sin [head_dim] = cos_tab / sin_tab [L, head_dim] row *pos_dev (tables NULL: skipped);
 *                           mask[L] = i <= *pos_dev ? 0 : -inf (mask NULL: skipped).  A token / position outside the tables is CLAMPED to the last row (torch's index ops would raise; the caller validates).
 *   hqq_hip_argmax_advance  *next_tok_dev = the FIRST index of the largest of logits[n], a NaN counting as the largest (torch.argmax's order); *tok_dev = the same (NULL: skipped); *pos_dev += 1 (NULL: skipped) */
int hqq_hip_token_prologue(const int64_t* tok_dev, const int64_t* pos_dev, const void* embed, int64_t vocab, int64_t H, const void* cos_tab, const void* sin_tab, int64_t L,
                           int64_t head_dim, void* h, void* cos, void* sin, void* mask, int dtype, void* stream);
int hqq_hip_argmax_advance(const void* logits, int64_t n, int dtype, int64_t* next_tok_dev, int64_t* tok_dev, int64_t* pos_dev, void* stream);
/* The same for a BATCH of `batch` independent sequences (1 <= batch <= 65535), one decode step of each — the glue of a batched decode step
 * (hqq_amd.utils.llama_fused.FusedLlamaBatchStep).  tok_dev / pos_dev: int64[batch] on the device; every other tensor is dense and row-major per
 * sequence.  Row b of each call gives exactly the bits the batch-1 call gives for sequence b alone (same kernel, same per-row arithmetic; the row is
 * a grid index).  Argument checks as the batch-1 calls, plus batch; all of them before anything is launched.
 *   hqq_hip_token_prologue_batched  hqq_hip_token_prologue per row: h [batch, H] = embed[tok[b]]; cos / sin [batch, head_dim] = the tables' row pos[b];
 *                                   mask [batch, L] = i <= pos[b] ? 0 : -inf
 *   hqq_hip_argmax_advance_batched  hqq_hip_argmax_advance per row, one workgroup each: logits [batch, n]; next_tok[b], tok[b] = the argmax of row b; pos[b] += 1 */
int hqq_hip_token_prologue_batched(const int64_t* tok_dev, const int64_t* pos_dev, int64_t batch, const void* embed, int64_t vocab, int64_t H, const void* cos_tab,
                                   const void* sin_tab, int64_t L, int64_t head_dim, void* h, void* cos, void* sin, void* mask, int dtype, void* stream);
int hqq_hip_argmax_advance_batched(const void* logits, int64_t batch, int64_t n, int dtype, int64_t* next_tok_dev, int64_t* tok_dev, int64_t* pos_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The decoder block's launches with those steps FOLDED IN (ABI 6; csrc/gemv_block.hip): hqq_hip_gemv_grouped for ONE activation row whose
 * prologue / epilogue does what hqq_hip_add_rmsnorm / hqq_hip_silu_mul / the residual add did as launches of their own — LlamaDecoderLayer.forward
 * (transformers models/llama/modeling_llama.py) around HQQLinear.forward (hqq/core/quantize.py:880-898) becomes 4 launches + rotary / attention:
 *   HQQ_BLOCK_NORM                   x is the RESIDUAL STREAM h [1, K]; every workgroup computes norm_weight * T(float(h) * rsqrt(mean(h^2) + eps))
 *                                    itself (LlamaRMSNorm, hqq_hip_add_rmsnorm's roundings; fp32 sum of squares in a fixed order) and contracts the
 *                                    layers with that; y[i] [1, N[i]] as hqq_hip_gemv_grouped writes them (q|k|v)
 *   HQQ_BLOCK_NORM | HQQ_BLOCK_SILU  one layer in the PAIRED layout — the level matrix of gate on top of the level matrix of up, packed as ONE layer of
 *                                    N = 2 x intermediate rows (hqq_amd.ops.pair_layers), so that a packed row holds gate row n and up row n —:
 *                                    y[0] [1, N / 2] = T(silu(T(gate[n]))) * T(up[n]) (LlamaMLP.forward; hqq_hip_silu_mul's roundings); gate / up are not stored
 *   HQQ_BLOCK_RESID                  one layer, x its input as usual; y[0] is the residual stream: h[n] = h[n] + T(result[n]) (o_proj, down_proj)
 * fp16 / bf16; nbits 4 / 2, or 3 with HQQ_OPT_W3S; group_size 64; exact weights (HQQ_OPT_META_SCALABLE honoured); K <= 8192 for the NORM forms.
 * No bias (the Llama linears have none), no workspace.  Same streaming loop, launch geometry and weights as hqq_hip_gemv.
 * ------------------------------------------------------------------------------------------- */
#define HQQ_BLOCK_NORM  1u
#define HQQ_BLOCK_RESID 2u
#define HQQ_BLOCK_SILU  4u
#define HQQ_BLOCK_ROPE  8u
/*   HQQ_BLOCK_NORM | HQQ_BLOCK_ROPE  the q | k | v group (n_layers = 3) with hqq_hip_rope_cache in its epilogue.  q and k in the ROTARY-PAIRED row order
 *                                    (hqq_amd.ops.rotary_pair_layout: element i < head_dim / 2 of head h is row h head_dim / 2 + i, its partner i + head_dim / 2
 *                                    row N / 2 + h head_dim / 2 + i — BitPack's row slabs then hold both in one packed row), v as it is.  y[0] = q_out
 *                                    [n_heads, head_dim] (rotated, natural order), y[1] / y[2] = the key / value caches [n_kv_heads, cache_len, head_dim]: the
 *                                    rotated key and the value are written at position *rope->pos (device memory: graph-replay safe; outside the cache: nothing).
 *                                    apply_rotary_pos_emb / StaticLayer.update, rounding for rounding as hqq_hip_rope_cache.  rope: NULL without the flag. */
typedef struct {
  const void* cos;       /* [head_dim] of the position, the compute dtype */
  const void* sin;
  const int64_t* pos;    /* device memory */
  int64_t head_dim, cache_len;
} hqq_rope_t;
int hqq_hip_gemv_block(int nbits, int n_layers, const void* x, const void* norm_weight, float eps, const void* const* Wq, const void* const* scale,
                       const void* const* zero, void* const* y, const int64_t* N, int64_t K, int64_t group_size, int dtype, uint32_t opts, uint32_t flags,
                       const hqq_rope_t* rope, void* stream);

/* Decode attention for ONE query per head over a static KV cache (opt-in: hqq_amd.utils.llama_fused.FusedLlamaStep(attention="hip")).
 * Replaces, in the reference's generate loop (hqq/utils/generation_hf.py:117-540), HF's call of F.scaled_dot_product_attention for a decode step:
 *   out[h, :] = softmax_j(q[h, :] . k_cache[h / (n_heads / n_kv_heads), j, :] * scaling) . v_cache[..., j, :]   over j = 0 .. pos_dev[0]
 * fp32 scores, softmax and accumulation, one rounding of the output: WITHIN ROUNDING of SDPA's result, not bit-identical to it (its flash
 * kernel blocks the keys and rounds the probabilities to the tensors' dtype) — which is why the default decode step keeps HF's attention function.
 * q [n_heads, head_dim] (rotary already applied), k_cache / v_cache [n_kv_heads, cache_len, head_dim], out [n_heads, head_dim]; fp16 / bf16;
 * head_dim 64 / 128 / 256; cache_len <= 30000; pos_dev: the query's position in device memory (graph-replay safe). */
int hqq_hip_attn_decode(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, void* out, int64_t n_heads, int64_t n_kv_heads,
                        int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace, size_t workspace_bytes, void* stream);
/* splits: 1 = one workgroup per query head (caches of up to ~1000 positions: 3.5-5.5 us); > 1 (at most 64): every head's visible keys are shared
 * out over `splits` workgroups whose (max, sum, output) records a second small launch merges in split order (long caches: 48 -> 19 us at 4096
 * positions with 8) — `workspace` then holds hqq_hip_attn_decode_workspace_bytes(n_heads, head_dim, splits) bytes (caller-owned, no initialisation). */
size_t hqq_hip_attn_decode_workspace_bytes(int64_t n_heads, int64_t head_dim, int64_t splits);
/* The same with hqq_hip_rope_cache folded in: q / k / v are the RAW projections ([n_heads, head_dim], [n_kv_heads, head_dim] twice), cos / sin
 * [head_dim]; every workgroup rotates its query and its KV head's new key (hqq_hip_rope_cache's arithmetic, rounding for rounding), takes the new
 * key / value from on-chip memory for position pos and reads the cache only below it; the new key / value are written to the cache (by one workgroup
 * per KV head) for the following steps: the cache ends up bit-identical to what hqq_hip_rope_cache writes. */
int hqq_hip_rope_attn_decode(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, void* k_cache, void* v_cache,
                             void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits,
                             void* workspace, size_t workspace_bytes, void* stream);
/* hqq_hip_attn_decode / hqq_hip_rope_attn_decode for `batch` sequences: q, k / v and out [batch, ...] of the batch-1 shapes, caches
 * [batch, n_kv_heads, cache_len, head_dim], cos / sin [batch, head_dim], pos_dev int64[batch]; sequence b attends over its own first pos_dev[b] + 1
 * keys.  `splits` holds for the whole launch (the caller picks it from the LARGEST position): a sequence with fewer visible keys than splits leaves
 * the surplus shares empty (max -inf, sum 0), and the merging launch gives them weight 0 — as the batch-1 kernels already do (a share past the
 * last key reads nothing).  workspace: hqq_hip_attn_decode_workspace_bytes(batch * n_heads, head_dim, splits) bytes. */
int hqq_hip_attn_decode_batched(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads,
                                int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                                size_t workspace_bytes, void* stream);
int hqq_hip_rope_attn_decode_batched(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t batch, void* k_cache,
                                     void* v_cache, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype,
                                     int64_t splits, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Speculative greedy decoding by prompt lookup (opt-in: hqq_amd.utils.llama_fused.FusedLlamaStep(batch = R, verify = True),
 * GraphedGreedyDecoder(speculate = "ngram")): R consecutive positions of ONE sequence — the last committed token and R - 1 guessed ones — go through
 * one pass over the weights, and the model's own argmax decides how many guesses stand.  Under greedy decoding the output is the greedy output.
 * The four symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 *
 * hqq_hip_rope_cache_shared: hqq_hip_rope_cache_batched for `rows` rows of one sequence.  q / q_out [rows, n_heads, hd], k / v [rows, n_kv_heads, hd],
 *   cos / sin [rows, hd], pos_dev int64[rows]; the caches are ONE sequence's [n_kv_heads, cache_len, hd] (a batch-1 StaticCache's tensors).  Row i's rotated
 *   key and its value go to slot pos_dev[i]; q_out[i] has the bits of the batch-1 hqq_hip_rope_cache call on row i; a position outside [0, cache_len)
 *   writes nothing.  CONTRACT: the positions of one call are distinct.  Rows with equal positions race for that slot: its contents are then unspecified
 *   (some mixture of those rows' keys and values; never anything outside the slot).  Checks as hqq_hip_rope_cache_batched.
 * hqq_hip_attn_decode_shared: hqq_hip_attn_decode_batched for `rows` queries of one sequence against that one cache [n_kv_heads, cache_len, hd]: row i
 *   attends over keys [0, pos_dev[i]].  The same kernel, splits, workspace layout (hqq_hip_attn_decode_workspace_bytes(rows * n_heads, ...)) and merging
 *   launch; only the cache's row stride is zero.  Row i is BIT-IDENTICAL to hqq_hip_attn_decode on the same cache with row i's query and position and the
 *   same `splits`.  No rotary-fused form exists: row i reads keys that other rows write in the same step, so the write is a launch of its own
 *   (hqq_hip_rope_cache_shared).  Every key is read once per row, not once per call.
 * hqq_hip_spec_propose: the n-gram proposer, one workgroup.  hist_dev int64[cap]: the sequence's tokens; *p_dev: the index of the last committed one.
 *   rows R in 2..16, ngram_max N in 0..4 (anything else: HQQ_ERR_SHAPE; 1 <= cap < 2^31).  Writes tok_dev[R], pos_dev[R]: tok[0] = hist[p], pos[i] = p + i
 *   (not clamped: past the cache the kernels above skip their writes and hqq_hip_token_prologue_batched clamps its table rows).  Drafts: take the largest
 *   n <= min(N, p) for which some e in [n - 1, p - 1] has hist[e - n + 1 .. e] == hist[p - n + 1 .. p]; among those the largest e; draft i (1 .. R - 1) is
 *   ext[e + i], where ext[m] = hist[m] for m <= p and ext[m] = draft[m - p] beyond (the periodic extension of a loop of period p - e).  No match, or
 *   N = 0: every draft is hist[p].  A *p_dev outside [0, cap) reads nothing and gives tok = 0.  Any draft is legal — only speed depends on it —, but the
 *   rule is fixed so that a host restatement can be compared bit for bit.
 * hqq_hip_spec_accept: one wave.  g_dev[R]: the rows' argmax (hqq_hip_argmax_advance_batched(logits, g, NULL, NULL)); tok_dev[R]: what the rows were
 *   fed; device scalars *p_dev, *last_dev (the index of the last token to emit), *eos_dev (-1: none), *done_dev, and the counters *steps_dev / *tokens_dev.
 *   If *done != 0 or p >= last (or p < 0 or last >= cap: nothing could be committed in bounds), NOTHING changes — replays after the end are harmless.
 *   Otherwise a is the largest value in 0 .. R - 1 with tok[i] == g[i - 1] for all 1 <= i <= a and p + a + 1 <= last; if some g[i] == eos with i <= a,
 *   a is cut to the first such i and *done = 1.  Then hist[p + 1 + i] = g[i] for i = 0 .. a, p += a + 1, steps += 1, tokens += a + 1.
 * Both are plain integer work: no atomics, no workspace, fixed orders; every argument is checked before the launch (HQQ_ERR_SHAPE).
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_rope_cache_shared(const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t rows, void* q_out,
                              void* k_cache, void* v_cache, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, int dtype, void* stream);
int hqq_hip_attn_decode_shared(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, int64_t rows, void* out, int64_t n_heads,
                               int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                               size_t workspace_bytes, void* stream);
int hqq_hip_spec_propose(const int64_t* hist_dev, int64_t cap, const int64_t* p_dev, int64_t rows, int64_t ngram_max, int64_t* tok_dev, int64_t* pos_dev, void* stream);
int hqq_hip_spec_accept(const int64_t* g_dev, const int64_t* tok_dev, int64_t rows, int64_t* hist_dev, int64_t cap, int64_t* p_dev, const int64_t* last_dev,
                        const int64_t* eos_dev, int64_t* done_dev, int64_t* steps_dev, int64_t* tokens_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * hqq_hip_attn_decode_tiled (csrc/attn_tile.hip): hqq_hip_attn_decode_shared's arguments, limits and semantics — `rows` (1 .. 16) queries of ONE sequence
 * against its dense caches [n_kv_heads, cache_len, hd], q / out [rows, n_heads * hd], pos_dev int64[rows]; row i attends over keys [0, pos_dev[i]], positions in
 * any order, a position outside [0, cache_len) attends as if at cache_len - 1; fp16 / bf16, hd 64 / 128 / 256, cache_len <= 30000, splits <= 64 and the
 * workspace of hqq_hip_attn_decode_workspace_bytes(rows * n_heads, hd, splits) bytes — with ANOTHER kernel and ANOTHER contract (opt-in:
 * FusedLlamaStep(verify = True, verify_attention = "tile")).  One workgroup per (query head, split) serves all rows: the keys [k0, k1) of [0, n_max),
 * n_max = 1 + the largest clamped position, chunk = ceil(n_max / splits), are read from memory ONCE for all rows and go through the matrix cores as
 * flash-decoding does it: blocks of 32 keys, fp32 scores, a running (max, sum, output) per row, the probabilities ROUNDED TO THE TENSORS' DTYPE for the
 * product with V, fp32 accumulation, the waves' and the splits' shares merged in fixed order (the splits by the one-row kernels' merging launch).
 * Added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * CONTRACT.  Deterministic: the same bits call to call (no atomics, fixed orders).  Row i's output depends on its own query, pos_dev[i], the cache, `rows`,
 *   `splits` and n_max, and on NO other row's query (the columns of the score tile do not mix).  It is NOT bit-identical to hqq_hip_attn_decode: it lies within
 *   a derived band of float64 attention (tests/_tile_cases.py derives it term by term).  Cache rows from n_max on may hold anything (NaN, Inf, rejected
 *   guesses): no key row >= the workgroup's k1 is read, so nothing at or beyond n_max is.  Rows i >= `rows` of the 16-row tile read no query memory and write nothing.
 *   rows outside 1 .. 16, a missing or short workspace: HQQ_ERR_SHAPE, nothing is launched.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_attn_decode_tiled(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, int64_t rows, void* out, int64_t n_heads,
                              int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                              size_t workspace_bytes, void* stream);

/* workspace of hqq_hip_forward / hqq_hip_gemm for one layer at M rows (0 = none needed, workspace may be NULL): what the call's route parks
 * (the routes table above marks the ones that need workspace).  Same contract. */
size_t hqq_hip_forward_workspace_bytes(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts);
/* introspection (host arithmetic only): how the pipelined fused GEMM would run this shape — out8 = {waves per workgroup, tokens per tile,
 * feature tiles, token tiles, K splits, steps per split, tiles that run unsplit before the split ones, workgroups}; HQQ_ERR_UNSUPPORTED
 * when another kernel serves the shape */
int hqq_hip_gemm_plan(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts, int* out8);
size_t hqq_hip_gemm_workspace_bytes(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts);   /* hqq_hip_gemm called directly, any M */
/* 1 when, for this shape, the fused kernels behind hqq_hip_forward are measured faster on MI355X than hqq_hip_dequantize + a library
 * GEMM on the result (the caller's alternative beyond the decode routes), else 0: a speed hint, never a correctness matter.  Always 1 up to
 * HQQ_GEMV_MAX_M rows; beyond, 1 on the skinny route and on the pipelined route while it is ahead (to 2560 rows). */
int hqq_hip_forward_prefers_fused(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype);
int hqq_hip_gemm(int nbits, const void* x, const void* Wq, const void* scale, const void* zero, const void* bias,
                 void* y, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace, size_t workspace_bytes,
                 void* stream);
/* hqq_hip_gemm for a GROUP of 1..HQQ_GEMV_MAX_GROUP layers that read the same x[M, K] (q | k | v, gate | up of a decoder block — hqq/utils/patching.py:82-86 calls them
 * one by one): ONE launch of the pipelined fused GEMM over the layers' concatenated feature tiles (+ one split-K reduce), y[i][M, N[i]] per layer (ABI 8).
 * Every layer must be one hqq_hip_gemm serves on the pipelined kernel (hqq_hip_gemm_grouped_covers = 1: fp16 / bf16, nbits 8 / 4 / 2 or the 3-bit stream
 * layout with HQQ_OPT_W3S, group_size 64, K % 128 == 0, (N / per) % 4 == 0); opts (incl. HQQ_OPT_META_SCALABLE) apply to the whole group.  The K split is chosen
 * for the group's total width, so a row may differ in the last bit from the same layer launched alone (another association of the same fp32 sums).
 * Workspace: hqq_hip_gemm_grouped_workspace_bytes (same contract as hqq_hip_forward's). */
int hqq_hip_gemm_grouped_covers(int nbits, int n_layers, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype, uint32_t opts);
size_t hqq_hip_gemm_grouped_workspace_bytes(int nbits, int n_layers, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype, uint32_t opts);
int hqq_hip_gemm_grouped(int nbits, int n_layers, const void* x, const void* const* Wq, const void* const* scale, const void* const* zero, const void* const* bias,
                         void* const* y, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace, size_t workspace_bytes,
                         void* stream);
/* HQQLinear.matmul on already dequantised weights (quantize.py:880-882: torch.matmul(x, W.t())): y[M,N] = x[M,K] . Wd[N,K]^T (+ bias[N]),
 * fp16 / bf16, fp32 accumulation, one rounding (+ one for the bias add).  The GEMM half of the long-prompt route: hqq_hip_dequantize rebuilds
 * a layer's weights once, this contracts them with any number of tokens (csrc/gemm_dense.hip: 256 x 256 x 64 tiles, all operands by LDS-DMA,
 * four phases per K tile).  K % 64 == 0, N % 4 == 0; no workspace. */
int hqq_hip_gemm_dense(const void* x, const void* Wd, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int dtype, void* stream);
/* hqq_hip_gemv for M it covers, hqq_hip_gemm otherwise; workspace: hqq_hip_forward_workspace_bytes with the same M */
int hqq_hip_forward(int nbits, const void* x, const void* Wq, const void* scale, const void* zero, const void* bias,
                    void* y, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * HQQLinear.forward for layers quantised along AXIS 0 (quantize.py:104-116, :880-898), decode sizes: y[M,N] = x[M,K] . dequantize(Wq)^T (+ bias[N])
 * in one pass over the packed bytes and the meta (csrc/gemv_axis0.hip).  Wq: the reference's axis-0 container of the byte widths — the [gs, N K / gs]
 * level matrix packed — which holds the same bytes as the axis-1 container of [N, K]; scale / zero: the reference's [1, N K / gs] meta, flat
 * (weight W[n, k] uses element (n mod (N / gs)) K + k).  Weights rebuilt bit-identically to hqq_hip_dequantize(axis = 0), fp32 accumulation, one
 * rounding to dtype (+ one for the bias add).  Covered: nbits 8 / 4 / 2 / 1 in fp16, 4 / 2 in bf16; group_size % 16 == 0 with N % group_size == 0
 * (group_size = N is the reference's group_size=None); K % 64 == 0; 1 <= M <= HQQ_GEMV_MAX_M.  Anything else: HQQ_ERR_UNSUPPORTED ("not covered").
 * opts: bits outside HQQ_OPT_ALL are an argument error; none changes this kernel (its weights are always the exact ones).
 * Workspace: hqq_hip_gemv_axis0_workspace_bytes(...) bytes, never 0 — fp32 partial sums of the K splits, parked past the counter head of the
 * decode workspace (same contract as hqq_hip_gemv_workspace_bytes; this call leaves the counters untouched).  Two launches: the contraction and a
 * reduce that sums the splits in a fixed order (deterministic; the split depends on the shape only).
 * ------------------------------------------------------------------------------------------- */
size_t hqq_hip_gemv_axis0_workspace_bytes(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype);
int hqq_hip_gemv_axis0(int nbits, const void* x, const void* Wq, const void* scale, const void* zero, const void* bias, void* y,
                       int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace, size_t workspace_bytes,
                       void* stream);
/* hqq_hip_gemv_axis0 for 1 <= n_layers <= 3 axis-0 layers that consume the SAME activation rows x[M, K] (q|k|v, gate|up), in one contraction launch
 * and one reduce launch.  Per-layer arguments are host arrays of n_layers entries as in hqq_hip_gemv_grouped (read during the call, not kept;
 * bias may be NULL or hold NULL entries); the layers share K, group_size, nbits and dtype, each has its own N[i], and each must be a layer
 * hqq_hip_gemv_axis0 covers (same error codes; validated before anything is launched).  The layers' work items are concatenated, every layer keeps
 * the K split it has on its own and its partial sums are added in split order: y[i] holds the bits a hqq_hip_gemv_axis0 call on layer i gives.
 * flags: 0, or HQQ_BLOCK_SILU (below) — n_layers == 2 with N[0] == N[1] (gate, up): the reduce finishes both outputs as above (rounded to dtype, bias
 * added with one more rounding) and writes only y[0][m, n] = T(silu(gate)) * up, the bits hqq_hip_silu_mul gives on the two outputs of the unflagged
 * call; y[1] is not read.  Every other flag, and HQQ_BLOCK_SILU on another group: HQQ_ERR_UNSUPPORTED.
 * Workspace: hqq_hip_gemv_axis0_grouped_workspace_bytes(...) — the counter head (untouched) plus the sum of the layers' partial-sum areas, i.e. of
 * hqq_hip_gemv_axis0_workspace_bytes(layer i) minus the head; 0 where the call would be refused.
 * The two symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits. */
size_t hqq_hip_gemv_axis0_grouped_workspace_bytes(int nbits, int n_layers, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype,
                                                  uint32_t flags);
int hqq_hip_gemv_axis0_grouped(int nbits, int n_layers, const void* x, const void* const* Wq, const void* const* scale, const void* const* zero,
                               const void* const* bias, void* const* y, const int64_t* N, int64_t M, int64_t K, int64_t group_size, int dtype,
                               uint32_t opts, uint32_t flags, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * HQQLinear.forward for layers quantised along AXIS 0 at 17 .. HQQ_GEMM_AXIS0_MAX_M activation rows (short prompts, batches wider than the decode
 * kernel's): y[M,N] = x[M,K] . dequantize(Wq)^T (+ bias[N]) in one pass over the packed bytes and the meta per 64 rows (csrc/gemm_axis0.hip).  What it
 * replaces is hqq/core/quantize.py:880-898 as HQQLinear runs it for these layers: Quantizer.dequantize writes the whole fp16 / bf16 weight, torch.matmul
 * reads it back, `out += bias`.  Arguments, layout, weights (the bits of hqq_hip_dequantize(axis = 0)), rounding (fp32 accumulation, one rounding, one
 * more for the bias) and coverage are hqq_hip_gemv_axis0's, except for the rows: HQQ_GEMV_MAX_M < M <= HQQ_GEMM_AXIS0_MAX_M, anything else
 * HQQ_ERR_UNSUPPORTED ("not covered").  A row's output bits do not depend on the contents or order of the other
 * rows of the call (they depend on M only through the number of 64-row passes, which sets the K split).
 * Workspace: hqq_hip_gemm_axis0_workspace_bytes(...) bytes — the counter head (untouched) plus fp32 partial sums of the K splits; linear in M, 0 where
 * the call would be refused.  Two launches: the contraction and a reduce that sums the splits in split order (deterministic; the split depends on
 * nbits, N, K, group_size and the number of 64-row passes only).
 * The two symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
#define HQQ_GEMM_AXIS0_MAX_M 256
size_t hqq_hip_gemm_axis0_workspace_bytes(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype);
int hqq_hip_gemm_axis0(int nbits, const void* x, const void* Wq, const void* scale, const void* zero, const void* bias, void* y,
                       int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype, uint32_t opts, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * The backward of HQQLinear with respect to its input for layers quantised along AXIS 1: dx[M,K] = g[M,N] . dequantize(Wq)[N,K] in one launch
 * (csrc/gemm_dgrad.hip).  What it replaces is the backward of the reference's autograd functions (hqq/core/quantize.py:477-479, 534-553):
 * Quantizer.dequantize writes the whole fp16 / bf16 weight (2 N K bytes), torch.matmul(grad, W) reads it back.
 * g [M,N] and dx [M,K] dense, row-major, in `dtype`; Wq the byte container [N / per, K]; scale / zero N K / group_size elements of `dtype` (the axis-1
 * layout of hqq_hip_dequantize).  Weights are the bits of hqq_hip_dequantize (two roundings in `dtype`); fp32 accumulation over n, one rounding; no bias
 * (it has no part in dx).  Deterministic: an output tile belongs to one workgroup that walks all of N — no atomics, no workspace —, and a row's output
 * bits depend on that row of g only, not on M or on the rows it travels with.
 * Covers: nbits 8 / 4 / 2 (byte containers), HQQ_F16 / HQQ_BF16, group_size % 16 == 0, K % group_size == 0, K % 64 == 0, N % (8 per) == 0 (a lane contracts 8 packed rows), M >= 1,
 * sizes within 32-bit offsets.  Anything else valid (3-bit, 1-bit, fp32, other shapes): HQQ_ERR_UNSUPPORTED ("not covered"), message in
 * hqq_hip_last_error(); hqq_hip_gemm_dgrad_covers answers the same question (1 / 0) without launching.  g, Wq, dx 16-byte aligned.
 * The two symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_gemm_dgrad_covers(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype);
int hqq_hip_gemm_dgrad(int nbits, const void* g, const void* Wq, const void* scale, const void* zero, void* dx, int64_t M, int64_t N, int64_t K,
                       int64_t group_size, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same product for layers quantised along AXIS 0: dx[M,K] = g[M,N] . dequantize(Wq, axis = 0)[N,K] in one launch (csrc/gemm_dgrad_axis0.hip) —
 * the backward of the reference's only training backend (ATEN_BACKPROP, hqq/core/quantize.py:930), which serves axis 0 and nothing else.
 * g [M,N] and dx [M,K] dense, row-major, in `dtype`; Wq the byte container [N / per, K] (the same bytes as on axis 1: byte [p, k] holds rows
 * p + slab N / per); scale / zero N K / group_size elements of `dtype` in the axis-0 layout of hqq_hip_dequantize: with Nr = N / group_size, element
 * (n, k) uses constant (n % Nr) K + k.  The contract is hqq_hip_gemm_dgrad's: weights are the bits of hqq_hip_dequantize(axis = 0) (two roundings in
 * `dtype`); fp32 accumulation over n in the same fixed order, one rounding; no bias.  Deterministic: no atomics, no workspace; a row's output bits depend
 * on (N, nbits) and that row of g only, not on M or on the rows it travels with; rows past M are never stored.  Runs on `stream`, graph-capturable.
 * Covers: nbits 8 / 4 / 2 (byte containers), HQQ_F16 / HQQ_BF16, group_size % 16 == 0, N % group_size == 0 (group_size = N: one group per column),
 * K % 64 == 0, N % (8 per) == 0, M >= 1, sizes within 32-bit offsets (HQQ_ERR_SHAPE, "size overflow", past them).  Anything else valid (3-bit, 1-bit,
 * fp32, other shapes): HQQ_ERR_UNSUPPORTED ("not covered"), message in hqq_hip_last_error(); hqq_hip_gemm_dgrad_axis0_covers answers the same question
 * (1 / 0) without launching.  Every check is made before anything is launched and needs no GPU.  g, Wq, scale, zero, dx 16-byte aligned.
 * The two symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_gemm_dgrad_axis0_covers(int nbits, int64_t M, int64_t N, int64_t K, int64_t group_size, int dtype);
int hqq_hip_gemm_dgrad_axis0(int nbits, const void* g, const void* Wq, const void* scale, const void* zero, void* dx, int64_t M, int64_t N, int64_t K,
                             int64_t group_size, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Merge a LoRA adapter into a layer's weight in one launch (csrc/lora_merge.hip): out[N,K] = dequantize(Wq) + ((A @ B) * scaling)^T, ready for
 * hqq_hip_quantize.  What it replaces is the torch composition of HQQLinearLoRA.merge_and_quantize (hqq/core/peft.py:167-190): an identity pushed
 * through the forward for the base weight, a K x N fp32 matmul, scaled, transposed, cast, added in place.
 * With T the compute dtype (`dtype`) and L the adapter's (`lora_dtype`), for every n < N, k < K:
 *     w         = hqq_hip_dequantize's value at [n, k]                 (its bits: two roundings in T)
 *     acc       = 0.f;  for j = 0 .. r-1 in this order:  acc = fadd_rn(acc, fmul_rn(float(A[k, j]), float(B[j, n])))
 *     m         = round_L(acc)                                          (the matmul's result in L; the identity for fp32)
 *     s         = round_L(float(m) * scaling)
 *     d         = round_T(s)                                            (.to(W.dtype))
 *     out[n, k] = round_T(float(w) + float(d))                          (W += ...: one rounding in T)
 * The multiply and the add are separate IEEE fp32 operations: no FMA, no MFMA, no atomics, no split over j — the result can be restated exactly on
 * the host and two calls on the same inputs give the same bits.
 * A [K, r] and B [r, N] dense, row-major, in L (HQQ_F32 / HQQ_F16 / HQQ_BF16); out [N, K] dense in T (HQQ_F16 / HQQ_BF16).
 * Base weight, packed form: Wq, scale, zero, N, K, group_size, axis exactly as hqq_hip_dequantize takes them, every (nbits, axis, group_size, N, K) it
 * accepts (8 / 4 / 3 / 2 / 1 bits, both axes); what it refuses with HQQ_ERR_NBITS / HQQ_ERR_SHAPE is refused here with the same code.
 * Base weight, dense form: nbits == 0 — Wq is a dense [N, K] weight in T and takes the place of w; scale, zero, group_size and axis are not read.
 * 1 <= r <= 256 and T fp16 / bf16; an fp32 T or another rank: HQQ_ERR_UNSUPPORTED ("not covered"); hqq_hip_lora_merge_covers answers the same
 * question (1 / 0) without launching.  Every check is made before anything is launched and needs no GPU.  No workspace; runs on `stream`; pointers
 * need the alignment of their elements only (16-byte stores and vector loads are used where the addresses allow); partial tiles on either edge are
 * handled, nothing outside out[N, K] is written.
 * The two symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_lora_merge_covers(int nbits, int64_t N, int64_t K, int64_t group_size, int axis, int dtype, int lora_dtype, int64_t r);
int hqq_hip_lora_merge(int nbits, const void* Wq, const void* scale, const void* zero, const void* A, const void* B, float scaling, void* out,
                       int64_t N, int64_t K, int64_t group_size, int axis, int dtype, int lora_dtype, int64_t r, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The adapter term of UN-MERGED LoRA layers in the decode step, two launches per group (csrc/lora_decode.hip).  For a group of
 * 1 .. HQQ_GEMV_MAX_GROUP layers that read the same activation rows x[M, K] — each with A_l [K, r_l], B_l [r_l, N_l], a host float scaling[l] and an
 * output y_l [M, N_l] that already holds the base layer's result (hqq_hip_gemv* / hqq_hip_gemv_grouped wrote it) — what HQQLinearLoRA.forward adds
 * (hqq/core/peft.py:150-165, `out + forward_lora(x).to(x_dtype)`), with T the compute dtype (`dtype`):
 *     t_l[m, j] = sum_k float(x[m, k]) * float(A_l[k, j])                  fp32     hqq_hip_lora_shrink  -> workspace
 *     u_l[m, n] = scaling[l] * sum_j t_l[m, j] * float(B_l[j, n])          fp32     hqq_hip_lora_expand, which then does
 *     y_l[m, n] = round_T(float(y_l[m, n]) + float(round_T(u_l[m, n])))             the read-modify-write of y
 * t and u stay in fp32.  For fp32 adapters that is the reference's arithmetic up to summation order.  For fp16 / bf16 adapters the reference also
 * rounds t, t @ B and the product with scaling to the adapter's dtype, and these kernels do NOT: the same value with fewer roundings (a deliberate
 * deviation: results differ from HQQLinearLoRA.forward's in the last bits of T).
 * Summation: K is cut into slices of 256 / 512 / 1024 k (r_l <= 64 / <= 128 / <= 256); slice i of layer l writes its partial t to
 * workspace[layer][slice][M][r_l] (fp32, layers one after the other); the expand sums the partials in slice order and forms u over j = 0 .. r_l - 1 in
 * ascending order.  The slice count, the order inside a slice and the order over j are functions of (K, r_l) alone — never of M, the row, a pointer
 * or anything read from the device; fused multiply-adds for the products, plain fp32 adds for the partials; no atomics, no arrival counters.  Two calls give the same
 * bits, and row m of an M-row call has the bits of a one-row call on that row.
 * Covered: x / y fp16 or bf16 (an fp32 T: HQQ_ERR_UNSUPPORTED); A_l and B_l all HQQ_F32, all HQQ_F16 or all HQQ_BF16 (`lora_dtype`), dense, row-major;
 * 1 <= M <= HQQ_GEMV_MAX_M; 1 <= r_l <= 256 (the ranks hqq_hip_lora_merge takes: what can be merged can be decoded un-merged); K % 8 == 0,
 * N_l % 8 == 0 (both up to 2^24); r_l, N_l and scaling[l] may differ per layer.  Anything else: HQQ_ERR_UNSUPPORTED with a message, before anything
 * is launched and without a GPU.  hqq_hip_lora_decode_covers answers the same question (1 / 0, A's and B's dtype given separately: they must agree).
 * Workspace: hqq_hip_lora_decode_workspace_bytes(n_layers, r, M, K) bytes (pure host arithmetic; 0 where the call would be refused), caller-owned,
 * 16-byte aligned, not shared by calls that may run concurrently; a larger one is fine.  It holds anything on entry: the shrink writes every partial
 * the expand of the same (r, M, K) reads, so it needs no clearing; HQQ_ERR_WORKSPACE when it is missing or too small.
 * The per-layer host arrays (A, B, y, N, r, scaling) are read during the call and not kept.  x must be 16-byte aligned; A, B, y to their element size.
 * Nothing outside y_l[M, N_l] and the stated part of the workspace is written.
 * The four symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_lora_decode_covers(int n_layers, const int64_t* N, const int64_t* r, int64_t M, int64_t K, int dtype, int a_dtype, int b_dtype);
size_t hqq_hip_lora_decode_workspace_bytes(int n_layers, const int64_t* r, int64_t M, int64_t K);
int hqq_hip_lora_shrink(int n_layers, const void* x, const void* const* A, const int64_t* r, int64_t M, int64_t K, int dtype, int lora_dtype,
                        void* workspace, size_t workspace_bytes, void* stream);
int hqq_hip_lora_expand(int n_layers, const void* workspace, size_t workspace_bytes, const void* const* B, const float* scaling, void* const* y,
                        const int64_t* N, const int64_t* r, int64_t M, int64_t K, int dtype, int lora_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same adapter term with ONE ADAPTER PER ROW, picked on the device from a bank of stacked adapters (csrc/lora_decode.hip): several adapters served
 * over one quantised base in one pass, and an adapter changed between calls without touching a captured graph.
 *     A_bank[l]        [n_adapters, K, r_l]       dense, `lora_dtype`                    B_bank[l]   [n_adapters, r_l, N_l]   dense, `lora_dtype`
 *     scaling_dev[l]   fp32 [n_adapters]          in DEVICE memory                       slot_dev    int64 [M]                in DEVICE memory
 * The host arrays of pointers (A_bank, B_bank, scaling_dev, y, N, r) are read during the call and not kept; slot_dev and scaling_dev[l] are read by the
 * kernels only — no host read, so the pair can be captured in a graph and replayed after the slots, a scaling or an adapter's elements were rewritten
 * in place.
 *   1. Row m with slot_dev[m] = a in [0, n_adapters): y_l[m, :] gets the bits hqq_hip_lora_shrink + hqq_hip_lora_expand give that row alone with
 *      A_bank[l][a], B_bank[l][a] and the float scaling_dev[l][a] — the slice size, the order inside a slice, the slice order, ascending j, one fused
 *      multiply-add per term and the two final roundings are theirs, functions of (K, r_l) alone.  Every row keeps its own chain: no term of another row's
 *      adapter enters it, not even a zero one.
 *   2. Row m with any other slot value (-1 is the documented "no adapter"; also >= n_adapters, other negatives): y_l[m, :] is not written and no
 *      adapter byte is read for the row; its partials in the workspace are neither written nor read.
 *   3. An adapter that no row selects is not read (it may hold anything, NaN included); one that several rows select is read once per workgroup.
 *   4. No atomics, no arrival counters: the same bits call after call, whatever the workspace held.
 * Covered: what hqq_hip_lora_shrink / hqq_hip_lora_expand cover, and 1 <= n_adapters <= 256; hqq_hip_lora_routed_covers answers 1 / 0.  The workspace
 * is theirs: hqq_hip_lora_decode_workspace_bytes(n_layers, r, M, K) bytes, layout [layer][slice][M][r_l].  x and the workspace 16-byte aligned, slot_dev
 * 8-byte aligned, everything else to its element size.  Nothing outside the selected rows of y_l and their part of the workspace is written.
 * The three symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_lora_routed_covers(int n_layers, const int64_t* N, const int64_t* r, int64_t n_adapters, int64_t M, int64_t K, int dtype, int lora_dtype);
int hqq_hip_lora_shrink_routed(int n_layers, const void* x, const void* const* A_bank, const int64_t* r, int64_t n_adapters, const int64_t* slot_dev,
                               int64_t M, int64_t K, int dtype, int lora_dtype, void* workspace, size_t workspace_bytes, void* stream);
int hqq_hip_lora_expand_routed(int n_layers, const void* workspace, size_t workspace_bytes, const void* const* B_bank, const float* const* scaling_dev,
                               void* const* y, const int64_t* N, const int64_t* r, int64_t n_adapters, const int64_t* slot_dev, int64_t M, int64_t K,
                               int dtype, int lora_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The routed expert MLP of a mixture-of-experts block at decode sizes (csrc/moe.hip) — what transformers' fused experts modules compute
 * (MixtralExperts.forward and its copies: gate_up_proj [E, 2I, H], down_proj [E, H, I], SiLU) over experts quantised along axis 1, in two launches
 * without a host read of the routing.  With T the compute dtype (`dtype`), rnd = round to T, e = idx[t, s]:
 *     hqq_hip_moe_gate_up   a[t, s, n] = rnd(rnd(silu32(rnd(x_t . Wg_e[n]))) * rnd(x_t . Wu_e[n]))                     a [T_, k, I], caller-owned
 *     hqq_hip_moe_down      d[t, s, n] = rnd(a[t, s] . Wd_e[n]);  out[t, n]: acc = 0, then for the token's slots in ascending (e, s):
 *                           acc = rnd(acc + rnd(fp32(d[t, s, n]) * w[t, s]))   (the product is an fp32 value first)      out [T_, H]
 * — the order in which HF's loop over the experts hit and its index_add_ visit a token's slots.  Dot products accumulate in fp32 (fused multiply-adds
 * in a fixed order that depends on K alone, then a fixed wave reduction): two calls give the same bits and a token's result does not depend on T_ or on
 * the other tokens.  Weights are rebuilt exactly as hqq_hip_dequantize rebuilds them (the same two roundings in T), for any zero-points and scales.
 *   x [T_, H] of T; idx [T_, k] int64 and weights [T_, k] float32 ON THE DEVICE; an id outside [0, E) contributes nothing and nothing is read for it
 *   (its part of `a` is left unwritten).  Stacks, expert-major and dense: *_Wq [E, N K / per] bytes in the layout of hqq_hip_pack applied to each expert's
 *   [N K / group_size, group_size] levels, *_scale / *_zero [E, N K / group_size] of T; gate and up: N = I, K = H; down: N = H, K = I.
 * Covered: nbits 4 and 2; fp16 / bf16; 1 <= T_ <= 16, 1 <= k <= 8, 1 <= E <= 256; H % 64 == 0, I % 64 == 0 (both up to 65536); group_size % 16 == 0
 * dividing H and I; per-expert strides that are 16-byte multiples.  Anything else (8 / 3 / 1 bits, fp32, other shapes): HQQ_ERR_UNSUPPORTED with a message,
 * before anything is launched and without a GPU; axis 0, a bias and view_as_float have no argument here.  hqq_hip_moe_covers answers the same question (1 / 0).
 * x, a, out and the stacks 16-byte aligned; idx and weights to their element size.  No workspace; nothing outside a[T_, k, I] / out[T_, H] is written.
 * The three symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_moe_covers(int nbits, int64_t T_, int64_t k, int64_t E, int64_t H, int64_t I, int64_t group_size, int dtype);
int hqq_hip_moe_gate_up(int nbits, const void* x, const void* idx, const void* gate_Wq, const void* gate_scale, const void* gate_zero,
                        const void* up_Wq, const void* up_scale, const void* up_zero, void* a, int64_t T_, int64_t k, int64_t E, int64_t H,
                        int64_t I, int64_t group_size, int dtype, void* stream);
int hqq_hip_moe_down(int nbits, const void* a, const void* idx, const void* weights, const void* down_Wq, const void* down_scale,
                     const void* down_zero, void* out, int64_t T_, int64_t k, int64_t E, int64_t H, int64_t I, int64_t group_size, int dtype,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * The router of a mixture-of-experts block at decode sizes (csrc/moe_router.hip): what MixtralTopKRouter / Qwen3MoeTopKRouter compute (F.linear, softmax,
 * topk, sum, div and Qwen3-MoE's cast), in ONE launch for T_ rows.  With T the compute dtype (`dtype`) and rnd = round to T:
 *     l[t, e] = fp32(rnd(x_t . W_e))                              x [T_, H] of T, W [E, H] of T, dense, row-major
 *     p[t, e] = exp(l[t, e] - max_e l) / sum_e exp(l - max)       in fp32; the sum over e in ascending order, one addition after the other
 *     sel     = the k experts of largest l[t, .], in descending l; EQUAL LOGITS BY ASCENDING e
 *     w[t, s] = p[t, sel_s], divided by sum_s p[t, sel_s] (s ascending) if `renorm`, then rounded to T and widened back to fp32 if `round_weights`
 *               (Qwen3-MoE's `.to(router_logits.dtype)`)
 * The dot product accumulates in fp32: lane i of a wave takes the 8-element chunks i, i + 64, ... of the row, one fused multiply-add per element in
 * ascending index into one accumulator, and the 64 partial sums are added as a balanced binary tree in lane order — an order that depends on H alone.
 * Selection is decided ON THE LOGITS (softmax is monotone) and the order among equal values — lower id first — is this library's own rule: torch.topk
 * leaves it unspecified, so it is not inherited from anything.  -0 equals +0.  A NaN logit compares as the largest (as in torch.topk), NaNs among
 * themselves by ascending id; every weight of a row that has one is NaN (as torch's softmax gives).
 * The one deviation from HF: F.linear rounds the same dot product to T in a summation order of its own, so a logit can differ from HF's by an ulp of T, and
 * a row whose k-th and (k+1)-th logits are that close can route differently.
 *   idx [T_, k] int64, weights [T_, k] float32 — what hqq_hip_moe_gate_up / hqq_hip_moe_down read; logits [T_, E] of T, or NULL to skip them.
 * Two calls give the same bits; a row's result does not depend on T_ or on the other rows.  No atomics, no workspace; nothing outside the three outputs
 * is written.
 * Covered: fp16 / bf16; 1 <= T_ <= 16; 1 <= k <= 8; k <= E <= 256; H % 8 == 0, 8 <= H <= 65536.  Anything else: HQQ_ERR_UNSUPPORTED with a message, before
 * anything is launched and without a GPU; hqq_hip_moe_router_covers answers the same question (1 / 0).  x and W 16-byte aligned, the outputs to their
 * element size (HQQ_ERR_ALIGN otherwise, as everywhere in this header).
 * The two symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_moe_router_covers(int64_t T_, int64_t k, int64_t E, int64_t H, int dtype);
int hqq_hip_moe_router(const void* x, const void* W, void* idx, void* weights, void* logits, int64_t T_, int64_t k, int64_t E, int64_t H, int renorm,
                       int round_weights, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A quantised static KV cache, 8 or 4 bits per element, and the decode-step launches that write and read it (csrc/kv_cache.hip).
 * The format, this library's own — one rule per (sequence, kv head, position) row r of head_dim values, keys (after the rotary embedding) and values alike:
 *     Quantizer.quantize(r.view(head_dim / gs, gs), nbits, group_size=gs, axis=1, optimize=False, round_zero=False, channel_wise=True)
 * (hqq/core/quantize.py:102-154, as hqq_hip_quantize computes it without its solver), scale and zero then cast to the compute dtype T (`dtype`).  A row depends
 * on no other row: it is quantised when it is written and never touched again.
 *   8 bits: byte i of a row is level i.  4 bits: byte i is level[i] << 4 | level[i + head_dim / 2] (BitPack.pack_4bit_u8 on the [head_dim / gs, gs] levels).
 *   kq, vq [batch, n_kv_heads, cache_len, head_dim * nbits / 8] uint8; k_scale, k_zero, v_scale, v_zero [batch, n_kv_heads, cache_len, head_dim / gs] of T.
 *   dequantised value: round_T(round_T(q - zero) * scale), the two roundings of Quantizer.dequantize.
 * Covered (hqq_hip_kv_covers: 1 / 0, pure host arithmetic; every entry point refuses the rest with HQQ_ERR_UNSUPPORTED "not covered" before anything is launched):
 * fp16 / bf16; nbits 8 / 4; head_dim 64 / 128 / 256; gs 32 / 64 dividing head_dim, 2 gs <= head_dim at 4 bits; 1 <= cache_len <= 30000.
 * The reference's arithmetic has no guard for a scale or zero beyond T's range (a group of near-equal values far from 0 in fp16 stores an infinite zero), and
 * none is added.  Level buffers and dense rows 16-byte aligned (HQQ_ERR_ALIGN otherwise).  No atomics, no workspace but the attention's: two calls give the same bits.
 *
 * hqq_hip_kv_quantize: dense rows k, v [batch, n_kv_heads, T_, head_dim] of T — strides in ELEMENTS of the first three dimensions in k_strides / v_strides
 *   (host int64[3], multiples of 8; a row's head_dim values are consecutive) — into positions p .. p + T_ - 1 of sequence b's rows, p = `start` (host) when
 *   pos_dev is NULL, else pos_dev[b * pos_stride] (device int64; pos_stride 0: one position for every sequence, 1: one each).  A position outside
 *   [0, cache_len) writes nothing; nothing but the addressed positions is written.
 * hqq_hip_kv_dequantize: positions 0 .. n - 1 of every (sequence, kv head) -> dense k_out, v_out [batch, n_kv_heads, n, head_dim] of T.
 * hqq_hip_rope_kvq_cache_batched: hqq_hip_rope_cache_batched's work — the same rotary arithmetic and the same q_out bits — with the rotated key and the value
 *   row quantised on chip and stored at pos_dev[b]: the stored bits are those of hqq_hip_rope_cache_batched into a dense cache followed by hqq_hip_kv_quantize
 *   of that row.  A position outside [0, cache_len) writes nothing to the buffers (q_out still is).  v 16-byte aligned.
 * hqq_hip_attn_decode_kvq / _batched: hqq_hip_attn_decode / _batched on the six buffers.  Each row is rebuilt to T as it is loaded, and everything behind the
 *   rebuild keeps the dense kernel's order (dot products, shuffles, score buffer, max / sum, accumulation, split records, the merging launch): the output is
 *   BIT-IDENTICAL to hqq_hip_attn_decode_batched on hqq_hip_kv_dequantize's tensors with the same `splits`.  Nothing at or beyond position pos + 1 is read, in
 *   levels or in meta.  splits / workspace: hqq_hip_attn_decode_workspace_bytes, the dense kernel's contract.
 * The seven symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_kv_covers(int nbits, int64_t head_dim, int64_t group_size, int64_t cache_len, int dtype);
int hqq_hip_kv_quantize(int nbits, const void* k, const void* v, const int64_t* k_strides, const int64_t* v_strides, int64_t batch, int64_t n_kv_heads, int64_t T_,
                        int64_t head_dim, int64_t group_size, int64_t start, const int64_t* pos_dev, int64_t pos_stride, void* kq, void* k_scale, void* k_zero, void* vq,
                        void* v_scale, void* v_zero, int64_t cache_len, int dtype, void* stream);
int hqq_hip_kv_dequantize(int nbits, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale, const void* v_zero, int64_t batch,
                          int64_t n_kv_heads, int64_t cache_len, int64_t n, int64_t head_dim, int64_t group_size, void* k_out, void* v_out, int dtype, void* stream);
int hqq_hip_rope_kvq_cache_batched(int nbits, const void* q, const void* k, const void* v, const void* cos, const void* sin, const int64_t* pos_dev, int64_t batch,
                                   void* q_out, void* kq, void* k_scale, void* k_zero, void* vq, void* v_scale, void* v_zero, int64_t n_heads, int64_t n_kv_heads,
                                   int64_t head_dim, int64_t group_size, int64_t cache_len, int dtype, void* stream);
int hqq_hip_attn_decode_kvq(int nbits, const void* q, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale, const void* v_zero,
                            const int64_t* pos_dev, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t group_size, int64_t cache_len, float scaling,
                            int dtype, int64_t splits, void* workspace, size_t workspace_bytes, void* stream);
int hqq_hip_attn_decode_kvq_batched(int nbits, const void* q, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale,
                                    const void* v_zero, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim,
                                    int64_t group_size, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * hqq_hip_attn_decode_gqa_batched / hqq_hip_attn_decode_gqa_kvq_batched (csrc/attn_gqa.hip): the arguments, layouts, limits and workspace of
 * hqq_hip_attn_decode_batched / hqq_hip_attn_decode_kvq_batched — `batch` sequences, q / out [batch, n_heads * hd], dense caches [batch, n_kv_heads, cache_len, hd]
 * or the six buffers of the quantised cache, pos_dev int64[batch]; sequence b attends over keys [0, pos_dev[b]], a position outside [0, cache_len) as if at
 * cache_len - 1; fp16 / bf16, hd 64 / 128 / 256, cache_len <= 30000, splits <= 64 with hqq_hip_attn_decode_workspace_bytes(batch * n_heads, hd, splits) bytes —
 * with ANOTHER kernel and ANOTHER contract (opt-in: FusedLlamaStep(gqa_attention = "group")).  The grid is (n_kv_heads, splits, batch): one workgroup serves the
 * G = n_heads / n_kv_heads query heads of a KV group as the rows of one 16-row MFMA query tile (hqq_hip_attn_decode_tiled's tile with the heads of a group in
 * the place of the rows of a verify step; csrc/attn_tile_core.h is the one text both run), so every key and value row is read from memory — and on the quantised
 * cache rebuilt — ONCE per group instead of once per query head.  Share sp of a split call covers keys [sp chunk, min((sp + 1) chunk, n)), n = pos + 1,
 * chunk = ceil(n / splits); its records have the one-row kernels' layout and are merged by their merging launch.
 * Added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * CONTRACT.  hqq_hip_attn_decode_tiled's: deterministic (no atomics, fixed orders); a head's output depends on its own query, its sequence's position and cache
 *   and `splits`, on NO other head's or sequence's query; within tests/_tile_cases.py's band of float64 attention, NOT bit-identical to hqq_hip_attn_decode_batched.
 *   On one sequence it IS bit-identical to hqq_hip_attn_decode_tiled on the transposed problem (rows = G, n_heads = n_kv_heads, every position equal, the same
 *   splits), and the quantised entry to the dense one on hqq_hip_kv_dequantize's tensors.  Nothing at or beyond pos_dev[b] + 1 of a sequence's cache is read,
 *   in levels or in meta.  The 16 - G padding rows of a tile read no query memory and write nothing.  No allocation.
 *   G > 16: HQQ_ERR_UNSUPPORTED (the message names G), then the quantised cache's coverage rule (hqq_hip_kv_covers: HQQ_ERR_UNSUPPORTED), then the checks of
 *   hqq_hip_attn_decode_batched with their codes; nothing is launched after an error.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_attn_decode_gqa_batched(const void* q, const void* k_cache, const void* v_cache, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads,
                                    int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace,
                                    size_t workspace_bytes, void* stream);
int hqq_hip_attn_decode_gqa_kvq_batched(int nbits, const void* q, const void* kq, const void* k_scale, const void* k_zero, const void* vq, const void* v_scale,
                                        const void* v_zero, const int64_t* pos_dev, int64_t batch, void* out, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim,
                                        int64_t group_size, int64_t cache_len, float scaling, int dtype, int64_t splits, void* workspace, size_t workspace_bytes,
                                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * hqq_hip_attn_prefill / hqq_hip_attn_prefill_kvq (csrc/attn_prefill.hip): causal attention of the T rows of ONE sequence's prompt against its static cache —
 * dense caches [n_kv_heads, cache_len, hd], or the six buffers [n_kv_heads, cache_len, .] of the quantised cache — that reads only the causal part of it
 * (opt-in: GraphedGreedyDecoder(prefill_attention = "hip")).  Query row t of head h is at q + t q_row_stride + h q_head_stride (strides in ELEMENTS, hd dense;
 * both multiples of 8) and stands at position pos0 + t: it attends over keys [0, pos0 + t].  The keys and values of the T rows are already in the cache when the
 * call runs.  out is dense [T, n_heads, hd].  pos0 and T are host integers (a prefill is not graph-captured).  fp16 / bf16, hd 64 / 128 / 256,
 * n_heads a multiple of n_kv_heads, cache_len <= 30000; the packed entry is additionally bounded by hqq_hip_kv_covers.
 * The grid is (n_heads, ceil(T / 16)): workgroup (h, j) serves rows 16 j .. min(16 j + 15, T - 1) of head h as the rows of hqq_hip_attn_decode_tiled's 16-row MFMA
 * query tile (csrc/attn_tile_core.h is the one text), each with its own causal limit, over keys [0, n_max), n_max = pos0 + min(16 j + 16, T), in ONE share: no
 * split, no workspace, no merging launch.  Tiles are per query head: the heads of a KV group re-read the same K and V rows.
 * The two symbols were added without raising HQQ_HIP_ABI_VERSION: nothing that existed at version 9 changed its signature, constants or bits.
 * CONTRACT.  (a) rows 16 j .. of head h are bit-identical to hqq_hip_attn_decode_tiled on those queries with pos = pos0 + 16 j + i and splits = 1; (b) every row
 *   lies within tests/_tile_cases.py's band of float64 attention (c_acc(n_max, 1)); (c) the packed entry is bit-identical to the dense one on
 *   hqq_hip_kv_dequantize's tensors; (d) nothing at or beyond pos0 + T is read, in levels, meta or dense rows (it may hold NaN); (e) row i depends on no query of
 *   a row > i and on no FINITE key / value at a position > pos0 + i (a masked V row inside the tile's range is multiplied by an exact 0); (f) deterministic, and
 *   the bits do not depend on q's strides; (g) it does NOT produce the bits of a softmax-then-matmul in the tensors' dtype (SDPA): the probabilities are rounded to
 *   the tensors' dtype before the product with V, and the keys are blocked.  Padding rows of the last tile read no query memory and write nothing.
 *   There is no position clamping: T < 1, pos0 < 0 or pos0 + T > cache_len is HQQ_ERR_SHAPE; a stride that is negative or no multiple of 8: HQQ_ERR_ALIGN; then
 *   (packed entry) the quantised cache's coverage rule, then hqq_hip_attn_decode_batched's checks with their codes; nothing is launched after an error.
 * ------------------------------------------------------------------------------------------- */
int hqq_hip_attn_prefill(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_cache, const void* v_cache, int64_t pos0, int64_t T, void* out,
                         int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t cache_len, float scaling, int dtype, void* stream);
int hqq_hip_attn_prefill_kvq(int nbits, const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* kq, const void* k_scale, const void* k_zero,
                             const void* vq, const void* v_scale, const void* v_zero, int64_t pos0, int64_t T, void* out, int64_t n_heads, int64_t n_kv_heads,
                             int64_t head_dim, int64_t group_size, int64_t cache_len, float scaling, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Quantizer.quantize + optimize_weights_proximal_legacy + BitPack.pack_* in one call
 * (quantize.py:75-180, optimize.py:96-108, 201-255), axis=1, channel_wise=True.
 *   W          [N*K] of w_dtype (F32/F16/BF16); promoted to float32 (`tensor.float()`, quantize.py:102)
 *   max_v      round(2^nbits - 1)  (quantize.py:121);  pack_bits the container width {8,4,3,2,1}
 *   Wq_out     packed weights, layout of hqq_hip_pack
 *   scale_out  [N*K/gs] float32 = 1/scale (quantize.py:154) ; zero_out [N*K/gs] float32
 *   info_out   int32[2] on the device: {iterations run, stop iteration index}  (may be NULL)
 * The solver runs in float32 — the reference's CPU precision (optimize.py:231); packed levels, zero and scale equal the
 * reference's CPU path bit for bit.  The reference's GPU path solves in fp16 and differs from its own CPU
 * result: hqq_hip_quantize_solver (ABI 9) below computes either.
 * ------------------------------------------------------------------------------------------- */
size_t hqq_hip_quantize_workspace_bytes(int64_t numel, int64_t group_size, int iters);
int hqq_hip_quantize(const void* W, int w_dtype, int64_t numel, int64_t group_size, int max_v, int pack_bits,
                     int round_zero, int optimize, int iters, float beta, float lp_norm,
                     void* Wq_out, float* scale_out, float* zero_out, int32_t* info_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* hqq_hip_quantize with the solver's precision chosen per call (ABI 9): solver_dtype HQQ_F32 is hqq_hip_quantize itself, bit for bit;
 * HQQ_F16 is the reference's GPU solver (optimize.py:231: fp16 when the device is "cuda"): after the float32 min/max initialisation W,
 * scale and zero are cast to fp16 and every op of the loop rounds once to fp16, the error means are compared as fp16, the final
 * levels use the float32 W with the fp16 scale / zero (optimize.py:254), and scale_out / zero_out are fp16 (quantize.py:154 computes
 * 1/scale in fp16).  Equal to the reference's fp16 solver as PyTorch's CPU kernels run it (their float32 summation order for the means);
 * torch-ROCm's own reduction order is not restated.  A group whose W * scale overflows fp16 gets a NaN zero, and its NaN error stops
 * the whole layer after one iteration, as in the reference; its levels are then not defined (the reference's cast of NaN to uint8
 * is platform-defined).  Any other solver_dtype: HQQ_ERR_DTYPE (checked before anything touches the device).  Same workspace size. */
int hqq_hip_quantize_solver(const void* W, int w_dtype, int64_t numel, int64_t group_size, int max_v, int pack_bits,
                            int round_zero, int optimize, int iters, float beta, float lp_norm, int solver_dtype,
                            void* Wq_out, void* scale_out, void* zero_out, int32_t* info_out,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The same with axis=0 (quantize.py:104-116): W is viewed as [group_size, numel/group_size] and every COLUMN is a group (min/max,
 * scale, zero and the solver's mean run down the rows).  Wq_out: the packed [packed_rows(group_size), numel/group_size] tensor
 * (row slabs of the [group_size, C] level matrix share a byte / word, as BitPack.pack_* packs it); scale_out / zero_out
 * [numel/group_size] float32.  Same workspace size as hqq_hip_quantize. */
int hqq_hip_quantize_axis0(const void* W, int w_dtype, int64_t numel, int64_t group_size, int max_v, int pack_bits,
                           int round_zero, int optimize, int iters, float beta, float lp_norm,
                           void* Wq_out, float* scale_out, float* zero_out, int32_t* info_out,
                           void* workspace, size_t workspace_bytes, void* stream);
/* hqq_hip_quantize_axis0 with solver_dtype HQQ_F32 / HQQ_F16, as hqq_hip_quantize_solver (ABI 9) */
int hqq_hip_quantize_axis0_solver(const void* W, int w_dtype, int64_t numel, int64_t group_size, int max_v, int pack_bits,
                                  int round_zero, int optimize, int iters, float beta, float lp_norm, int solver_dtype,
                                  void* Wq_out, void* scale_out, void* zero_out, int32_t* info_out,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* optimize_weights_proximal_legacy called on its own (optimize.py:208-255; `Quantizer.optimize_weights`): the same solver, started from the
 * CALLER's scale and zero instead of the group's min / max.  W viewed as [numel / group_size, group_size] (axis 1: a group per row) or
 * [group_size, numel / group_size] (axis 0: a group per column); scale_in / zero_in one float32 per group (scale as the quantiser uses it,
 * NOT inverted).  levels_out: the final W_q = clamp(rint(W * scale + zero), 0, max_v) as uint8 in W's view; zero_out: the solved zero per
 * group (scale is returned unchanged by the reference).  iters = 1 is one optimize_weights_proximal_legacy_step (optimize.py:201-206):
 * zero_out is then that step's new zero-point.  workspace: hqq_hip_quantize_workspace_bytes(numel, group_size, iters) + 4 bytes
 * per group. */
int hqq_hip_optimize(const void* W, int w_dtype, int64_t numel, int64_t group_size, int axis, int max_v, const float* scale_in, const float* zero_in,
                     int iters, float beta, float lp_norm, void* levels_out, float* zero_out, int32_t* info_out,
                     void* workspace, size_t workspace_bytes, void* stream);
/* hqq_hip_optimize with solver_dtype HQQ_F32 / HQQ_F16, as hqq_hip_quantize_solver (ABI 9): scale_in / zero_in stay float32 (cast to fp16
 * inside, as optimize.py:232-234 casts them), zero_out is fp16 with HQQ_F16.  Same workspace size as hqq_hip_optimize. */
int hqq_hip_optimize_solver(const void* W, int w_dtype, int64_t numel, int64_t group_size, int axis, int max_v, const float* scale_in,
                            const float* zero_in, int iters, float beta, float lp_norm, int solver_dtype, void* levels_out, void* zero_out,
                            int32_t* info_out, void* workspace, size_t workspace_bytes, void* stream);

/* channel_wise=False (quantize.py:114-116, 146): one scale and one zero for the WHOLE [rows, cols] tensor from its min and max, no
 * solver; the levels are packed in the tensor's own shape — Wq_out [packed_rows(rows), cols].  scale_out / zero_out: one float32 each
 * (scale already inverted, quantize.py:154).  cols % 8 == 0, rows * cols < 2^31.  workspace: HQQ_QUANTIZE_TENSOR_WS_BYTES. */
#define HQQ_QUANTIZE_TENSOR_WS_BYTES 16384
int hqq_hip_quantize_tensor(const void* W, int w_dtype, int64_t rows, int64_t cols, int max_v, int pack_bits, int round_zero,
                            void* Wq_out, float* scale_out, float* zero_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HQQ_HIP_H */
