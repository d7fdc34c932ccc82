// glue_ulp.hip — the largest errors of the device's expf and rsqrtf against float64, in fp32 ulps, over the arguments the decode step's glue kernels
// (csrc/block.hip: silu_mul, add_rmsnorm) can form (needs an MI355X): tests/_glue_cases.py takes EXPF_SEEN_ULPS / RSQRTF_SEEN_ULPS from this program's
// output, which is kept in profiles/glue_ulp.txt.  Stand-alone, run once by hand, built with the flags of csrc/block.hip:
//     python tests/_glue_cases.py tools/glue_rms_args.bin     (the fp32 arguments var + eps of the RMSNorm cases; optional)
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/glue_ulp.hip -o tools/glue_ulp.bin && tools/glue_ulp.bin tools/glue_rms_args.bin
//   expf:   silu_mul forms expf(-x) for x a value of T; EVERY finite fp16 and bf16 pattern is swept (2 * 65,536 less the non-finite ones), so the figure is a
//           bound, not a sample.  Reported apart: results that are normal fp32 numbers; results below 2^-126 (ulp floored at 2^-149; the kernel adds them to 1,
//           where they vanish); arguments whose float64 exp rounds to infinity in fp32 (the device must return +inf there: silu_mul's -0).
//   rsqrtf: add_rmsnorm forms rsqrtf(var + eps); 2^22 log-uniform arguments in [2^-30, 2^30] and the arguments of the test cases (the file above).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <random>
__global__ void k_exp(const float* in, float* out, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) out[i] = expf(in[i]); }
__global__ void k_rsq(const float* in, float* out, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) out[i] = rsqrtf(in[i]); }

static bool run(bool rsq, const std::vector<float>& h, std::vector<float>& o) {
  const int n = (int)h.size();
  float *din = nullptr, *dout = nullptr;
  o.resize(n);
  if (hipMalloc(&din, n * 4) != hipSuccess || hipMalloc(&dout, n * 4) != hipSuccess) { printf("alloc failed\n"); return false; }
  if (hipMemcpy(din, h.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) { printf("copy failed\n"); return false; }
  if (rsq) k_rsq<<<(n + 255) / 256, 256>>>(din, dout, n);
  else k_exp<<<(n + 255) / 256, 256>>>(din, dout, n);
  if (hipMemcpy(o.data(), dout, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return false; }
  (void)hipFree(din);
  (void)hipFree(dout);
  return true;
}

static double ulp32(double want) {   // the fp32 ulp at |want|, floored at 2^-149
  int e;
  std::frexp(want, &e);
  return std::ldexp(1.0, (e - 24 < -149) ? -149 : e - 24);
}

static float widen(uint16_t bits, bool bf) {
  uint32_t u;
  if (bf) u = (uint32_t)bits << 16;
  else {
    const uint32_t s = (bits >> 15) & 1u, ex = (bits >> 10) & 31u, m = bits & 1023u;
    if (ex == 31) u = (s << 31) | 0x7f800000u | (m << 13);
    else if (ex == 0) { const float f = std::ldexp((float)m, -24); std::memcpy(&u, &f, 4); u |= s << 31; }
    else u = (s << 31) | ((ex + 112u) << 23) | (m << 13);
  }
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int main(int argc, char** argv) {
  // ---- expf(-x), x every finite value of fp16 and of bf16 ----
  for (int bf = 0; bf < 2; ++bf) {
    std::vector<float> h, o;
    for (int b = 0; b < 65536; ++b) { const float x = widen((uint16_t)b, bf != 0); if (std::isfinite(x)) h.push_back(-x); }
    if (!run(false, h, o)) return 1;
    double w_norm = 0, w_sub = 0; float at_norm = 0, at_sub = 0; int n_over = 0, bad_over = 0, n_norm = 0, n_sub = 0;
    const double over = std::ldexp(2.0 - std::ldexp(1.0, -24), 127);   // float64 values from here on round to +inf in fp32
    for (size_t i = 0; i < h.size(); ++i) {
      const double want = std::exp((double)h[i]);
      if (want >= over) { ++n_over; if (!(std::isinf(o[i]) && o[i] > 0)) ++bad_over; continue; }
      const double err = std::fabs((double)o[i] - want) / ulp32(want);
      if (want >= std::ldexp(1.0, -126)) { ++n_norm; if (err > w_norm) { w_norm = err; at_norm = h[i]; } }
      else { ++n_sub; if (err > w_sub) { w_sub = err; at_sub = h[i]; } }
    }
    printf("EXPF %s normal results n=%d worst=%.4f ulps at arg=%.9g | results below 2^-126 n=%d worst=%.4f ulps(2^-149) at arg=%.9g | overflowing args n=%d not +inf=%d\n",
           bf ? "bf16" : "fp16", n_norm, w_norm, at_norm, n_sub, w_sub, at_sub, n_over, bad_over);
  }
  // ---- rsqrtf ----
  {
    std::vector<float> h, o;
    std::mt19937_64 g(1);
    std::uniform_real_distribution<double> u(-30.0, 30.0);
    for (int i = 0; i < (1 << 22); ++i) h.push_back((float)std::exp2(u(g)));
    const size_t n_sampled = h.size();
    if (argc > 1) {
      FILE* f = fopen(argv[1], "rb");
      if (!f) { printf("cannot open %s\n", argv[1]); return 1; }
      float v;
      while (fread(&v, 4, 1, f) == 1) h.push_back(v);
      fclose(f);
    }
    if (!run(true, h, o)) return 1;
    double worst[2] = {0, 0}; float at[2] = {0, 0};
    for (size_t i = 0; i < h.size(); ++i) {
      const double want = 1.0 / std::sqrt((double)h[i]);
      const double err = std::fabs((double)o[i] - want) / ulp32(want);
      const int s = i < n_sampled ? 0 : 1;
      if (err > worst[s]) { worst[s] = err; at[s] = h[i]; }
    }
    printf("RSQRTF sampled n=%zu worst=%.4f ulps at arg=%.9g | case arguments n=%zu worst=%.4f ulps at arg=%.9g\n", n_sampled, worst[0], at[0],
           h.size() - n_sampled, worst[1], at[1]);
  }
  return 0;
}
