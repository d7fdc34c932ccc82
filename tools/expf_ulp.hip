// expf_ulp.hip — the largest error of the device's expf against float64 exp, in ulps, over the arguments the router kernel can form (needs an MI355X):
// tests/_router_cases.py takes its EXP_SEEN_ULPS from this program's output.  Built with the flags of csrc/moe_router.hip:
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/expf_ulp.hip -o tools/expf_ulp.bin && tools/expf_ulp.bin
// -DEXPF_FN=__expf measures the fast intrinsic the decode-attention kernels' merging launch calls (csrc/block.hip, the same flags): tests/_tile_cases.py takes its
// FAST_EXP_SEEN_ULPS from that run.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#include <random>
#ifndef EXPF_FN
#define EXPF_FN expf
#endif
__global__ void k(const float* in, float* out, int n) { int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) out[i] = EXPF_FN(in[i]); }
int main() {
  std::vector<float> h;
  const int N1 = 1 << 22;
  for (int i = 0; i < N1; ++i) h.push_back(-32.0f * (float)i / (float)N1);
  for (int i = 0; i < N1; ++i) h.push_back(-1.0f * (float)i / (float)N1);
  std::mt19937_64 g(1);
  std::uniform_real_distribution<double> u(std::log(std::ldexp(1.0, -20)), std::log(88.0));
  for (int i = 0; i < (1 << 20); ++i) h.push_back(-(float)std::exp(u(g)));
  const int n = (int)h.size();
  float *din, *dout;
  if (hipMalloc(&din, n * 4) != hipSuccess || hipMalloc(&dout, n * 4) != hipSuccess) { printf("alloc failed\n"); return 1; }
  if (hipMemcpy(din, h.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) { printf("copy failed\n"); return 1; }
  k<<<(n + 255) / 256, 256>>>(din, dout, n);
  std::vector<float> o(n);
  if (hipMemcpy(o.data(), dout, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
  double worst = 0, worst_normal = 0; float at = 0, at_normal = 0;   // (_normal: among the results that are normal fp32 numbers; a flushed subnormal counts 2^23 ulps and more)
  for (int i = 0; i < n; ++i) {
    const double want = std::exp((double)h[i]);
    int e; std::frexp(want, &e);
    double ulp = std::ldexp(1.0, e - 24);
    if (e - 24 < -149) ulp = std::ldexp(1.0, -149);
    const double err = std::fabs((double)o[i] - want) / ulp;
    if (err > worst) { worst = err; at = h[i]; }
    if (want >= std::ldexp(1.0, -126) && err > worst_normal) { worst_normal = err; at_normal = h[i]; }
  }
  printf("EXP_ULP n=%d worst=%.4f ulps at x=%.9g\n", n, worst, at);
  printf("EXP_ULP_NORMAL worst=%.4f ulps at x=%.9g\n", worst_normal, at_normal);
  return 0;
}
