// fp64 FMA rate of the whole device from a register-only loop: every lane runs K independent
// chains of v_fma_f64, enough waves to fill every SIMD.  Prints one JSON line.
//   hipcc -O3 --offload-arch=gfx950 tools/fma_rate.hip -o tools/fma_rate && ./tools/fma_rate
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

constexpr int K = 8;

__global__ __launch_bounds__(256) void chains(double* out, int n) {
  double a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = threadIdx.x * 1e-3 + k;
  const double b = 0.999999, c = 1e-7;
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) a[k] = __builtin_fma(a[k], b, c);
  }
  double s = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) s += a[k];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

int main() {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) {
    std::fprintf(stderr, "no HIP device\n");
    return 1;
  }
  const int blocks = prop.multiProcessorCount * 8, threads = 256, n = 8192, reps = 9;
  double* out;
  if (hipMalloc(&out, sizeof(double) * blocks * threads) != hipSuccess) return 1;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  std::vector<float> ms(reps);
  for (int r = -2; r < reps; ++r) {   // two warm-up launches
    hipEventRecord(e0);
    hipLaunchKernelGGL(chains, dim3(blocks), dim3(threads), 0, 0, out, n);
    hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) return 1;
    if (r >= 0) hipEventElapsedTime(&ms[r], e0, e1);
  }
  std::sort(ms.begin(), ms.end());
  const double fma = (double)blocks * threads * K * 8.0 * n;
  std::printf("{\"what\": \"fp64 fma rate, register-only\", \"compute_units\": %d, \"fma\": %.0f, "
              "\"kernel_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, "
              "\"fma_per_s\": %.4e, \"flop_per_s\": %.4e}\n",
              prop.multiProcessorCount, fma, ms[reps / 2], ms[0], ms[reps - 1],
              fma / (ms[reps / 2] * 1e-3), 2.0 * fma / (ms[reps / 2] * 1e-3));
  hipFree(out);
  return 0;
}
