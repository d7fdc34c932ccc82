// spec.hip — the two integer kernels of speculative greedy decoding by prompt lookup (include/hqq_hip.h, hqq_hip_spec_*), gfx950.
//
// One speculative step verifies R consecutive positions of ONE sequence in a single pass over the weights (FusedLlamaStep(batch = R, verify = True)):
// row 0 is the last committed token, rows 1 .. R - 1 are guesses.  The guesses come from the sequence itself — the continuation of the latest earlier
// occurrence of its last n-gram (HF's prompt_lookup_num_tokens, vLLM's ngram proposer) — and the model's own argmax decides how many of them stand:
//   spec_propose   hist, p -> tok[R], pos[R]      (one workgroup)
//   spec_accept    the rows' argmax g[R], tok[R] -> hist, p, done, the counters      (one wave)
// Both read and write the loop state in device memory, so the captured step carries it forward by itself.  Plain integer work: no atomics, no
// workspace, fixed orders; tests/_spec_cases.py restates both rules on the host (propose_ref / accept_ref) and the GPU tests compare bit for bit.
#include "hqq_common.h"

namespace hqq {

constexpr int SPEC_MAX_ROWS = 16, SPEC_MAX_NGRAM = 4, SPEC_THREADS = 256;

// ---- tok[0] = hist[p], pos[i] = p + i, tok[1 .. R - 1] = the drafts.  Thread t looks at the end positions e = t, t + 256, ... < p and counts how many
//      tokens hist[e], hist[e - 1], ... equal hist[p], hist[p - 1], ... (up to N, e + 1 and p of them: a match of n tokens ends at e >= n - 1); per n it
//      keeps the largest such e.  The four maxima are reduced by shuffles and through LDS, then thread 0 takes the largest n that matched anywhere, the
//      largest e among its matches, and copies the continuation ext[e + i] — hist up to p, the drafts themselves beyond (a loop of period p - e).
//      A p outside [0, cap) reads nothing: every token is 0 ----
__global__ __launch_bounds__(SPEC_THREADS) void spec_propose_kernel(const int64_t* __restrict__ hist, int64_t cap, const int64_t* __restrict__ p_dev, int R, int N,
                                                                    int64_t* __restrict__ tok, int64_t* __restrict__ pos) {
  __shared__ int best_w[SPEC_THREADS / 64][SPEC_MAX_NGRAM];
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int64_t p64 = p_dev[0];
  if (tid < R) pos[tid] = p64 + tid;
  if (p64 < 0 || p64 >= cap) {   // (the whole workgroup leaves: no barrier is missed)
    if (tid < R) tok[tid] = 0;
    return;
  }
  const int p = static_cast<int>(p64);
  const int nmax = N < p ? N : p;
  int64_t tail[SPEC_MAX_NGRAM];   // hist[p - j]
#pragma unroll
  for (int j = 0; j < SPEC_MAX_NGRAM; ++j) tail[j] = j < nmax ? hist[p - j] : 0;
  int best[SPEC_MAX_NGRAM];
#pragma unroll
  for (int j = 0; j < SPEC_MAX_NGRAM; ++j) best[j] = -1;
  if (nmax > 0) {
    for (int e = tid; e < p; e += SPEC_THREADS) {   // ascending: the last hit per n is the largest e
      const int lim = e + 1 < nmax ? e + 1 : nmax;
      bool run = true;
#pragma unroll
      for (int j = 0; j < SPEC_MAX_NGRAM; ++j) {
        run = run && j < lim && hist[e - j] == tail[j];
        if (run) best[j] = e;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SPEC_MAX_NGRAM; ++j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(best[j], off, 64);
      best[j] = o > best[j] ? o : best[j];
    }
    if (lane == 0) best_w[wave][j] = best[j];
  }
  __syncthreads();
  if (tid != 0) return;
  int e = -1;
  for (int j = SPEC_MAX_NGRAM - 1; j >= 0 && e < 0; --j)
    for (int w = 0; w < SPEC_THREADS / 64; ++w) e = best_w[w][j] > e ? best_w[w][j] : e;
  const int64_t t0 = hist[p];
  int64_t d[SPEC_MAX_ROWS];
  d[0] = t0;
  for (int i = 1; i < R; ++i) {
    const int m = e + i;   // (e < p: m - p <= i - 1, a draft already made)
    d[i] = e < 0 ? t0 : (m <= p ? hist[m] : d[m - p]);
  }
  for (int i = 0; i < R; ++i) tok[i] = d[i];
}

// ---- one wave.  Lane i < R holds g[i] and tok[i].  ok: bit i set where row i's input token is what the model emitted for the position before it (bit 0
//      always: row 0 is committed); the accepted prefix is the run of set bits from bit 0, a + 1 long, cut to last - p tokens and at the first EOS in it.
//      Lanes 0 .. a commit their g, lane 0 advances p, done and the counters.  Frozen (done, p >= last, or a p / last outside the history): nothing changes ----
__global__ __launch_bounds__(64) void spec_accept_kernel(const int64_t* __restrict__ g, const int64_t* __restrict__ tok, int R, int64_t* __restrict__ hist, int64_t cap,
                                                         int64_t* __restrict__ p_dev, const int64_t* __restrict__ last_dev, const int64_t* __restrict__ eos_dev,
                                                         int64_t* __restrict__ done_dev, int64_t* __restrict__ steps_dev, int64_t* __restrict__ tokens_dev) {
  const int lane = static_cast<int>(threadIdx.x);
  const int64_t p = p_dev[0], last = last_dev[0], eos = eos_dev[0];
  if (done_dev[0] != 0 || p >= last || p < 0 || last >= cap) return;   // (uniform: the whole wave leaves)
  const bool live = lane < R;
  const int64_t gi = live ? g[lane] : 0;
  const bool ok = live && (lane == 0 || tok[lane] == g[lane - 1]);
  const unsigned long long okm = __ballot(ok);                  // bit 0 is set; bits >= R are clear
  int a = __builtin_ctzll(~okm) - 1;                            // the run of ones from bit 0 is a + 1 long
  const int64_t room = last - p - 1;                            // p + a + 1 <= last
  if (a > room) a = static_cast<int>(room);
  const unsigned long long eosm = __ballot(live && gi == eos) & ((2ull << a) - 1ull);
  const bool ended = eosm != 0ull;
  if (ended) a = __builtin_ctzll(eosm);
  if (lane <= a) hist[p + 1 + lane] = gi;                       // (p + 1 + a <= last < cap)
  if (lane == 0) {
    p_dev[0] = p + a + 1;
    if (ended) done_dev[0] = 1;
    steps_dev[0] += 1;
    tokens_dev[0] += a + 1;
  }
}

}  // namespace hqq

using namespace hqq;

extern "C" {

int hqq_hip_spec_propose(const int64_t* hist_dev, int64_t cap, const int64_t* p_dev, int64_t rows, int64_t ngram_max, int64_t* tok_dev, int64_t* pos_dev, void* stream) {
  const char* who = "hqq_hip_spec_propose";
  clear_stale_error();
  if (!hist_dev || !p_dev || !tok_dev || !pos_dev || cap < 1 || cap > INT32_MAX || rows < 2 || rows > SPEC_MAX_ROWS || ngram_max < 0 || ngram_max > SPEC_MAX_NGRAM) {
    set_error("%s: bad arguments (rows 2..16, ngram_max 0..4, 1 <= cap < 2^31)", who);
    return HQQ_ERR_SHAPE;
  }
  hipLaunchKernelGGL(spec_propose_kernel, dim3(1), dim3(SPEC_THREADS), 0, as_stream(stream), hist_dev, cap, p_dev, static_cast<int>(rows), static_cast<int>(ngram_max),
                     tok_dev, pos_dev);
  return check_launch(who);
}

int hqq_hip_spec_accept(const int64_t* g_dev, const int64_t* tok_dev, int64_t rows, int64_t* hist_dev, int64_t cap, int64_t* p_dev, const int64_t* last_dev,
                        const int64_t* eos_dev, int64_t* done_dev, int64_t* steps_dev, int64_t* tokens_dev, void* stream) {
  const char* who = "hqq_hip_spec_accept";
  clear_stale_error();
  if (!g_dev || !tok_dev || !hist_dev || !p_dev || !last_dev || !eos_dev || !done_dev || !steps_dev || !tokens_dev || cap < 1 || cap > INT32_MAX || rows < 2 ||
      rows > SPEC_MAX_ROWS) {
    set_error("%s: bad arguments (rows 2..16, 1 <= cap < 2^31, every pointer required)", who);
    return HQQ_ERR_SHAPE;
  }
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(64), 0, as_stream(stream), g_dev, tok_dev, static_cast<int>(rows), hist_dev, cap, p_dev, last_dev, eos_dev, done_dev,
                     steps_dev, tokens_dev);
  return check_launch(who);
}

}  // extern "C"
