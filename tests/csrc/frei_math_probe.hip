// frei_math_probe.hip — test-only: frei_math.h's primitives and formulas one value at a time,
// for tests/test_gpu_math.py (built by frei_amd/build.py build_probe() with the library's
// flags into tests/csrc/libfrei_mathprobe.so; not part of libfrei_hip.so).
//
//   int frei_mathprobe(int fn, int64_t n, const double* a, const double* b, const double* c,
//                      double* out, double* dev_ref)
// Host pointers; a, b, c hold n doubles each (b and c may be null where fn does not read them),
// out holds n doubles (3 n for shell_step: e, u, v as three consecutive blocks), dev_ref n.
// dev_ref receives the compiler's own lowering of the same operation computed in the same
// kernel (a / b, 1.0 / a, ::sqrt, ::exp) and NaN where there is none.  Returns the HIP error code.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frei_math.h"

namespace {

enum Fn {
  kDiv = 0,            // fm::div(a, b)                 dev_ref a / b
  kSqrt = 1,           // fm::sqrt(a)                   dev_ref ::sqrt(a)
  kSqrtPos = 2,        // fm::sqrt_pos(a)               dev_ref ::sqrt(a)
  kRcpNr = 3,          // fm::rcp_nr(a)                 dev_ref 1.0 / a
  kExpNeg = 4,         // fm::exp_neg(a)                dev_ref ::exp(a)
  kExpNegNf = 5,       // fm::exp_neg_nf(a)             dev_ref ::exp(a)
  kExpNegUnclamped = 6,  // fm::exp_neg_unclamped(a)    dev_ref ::exp(a)
  kPlanck = 7,         // planck(c1 = a, hcl = b, iT = c)
  kPlanckEm = 8,       // planck_em(c1 = a, hcl = b, iT = c)
  kShellStep = 9,      // shell_step at x = a with (I, Bl, Bn) the unit vectors: e, u, v
  kFnCount = 10
};

__global__ void __launch_bounds__(256)
probe(int fn, int64_t n, const double* __restrict__ a, const double* __restrict__ b,
      const double* __restrict__ c, double* __restrict__ out, double* __restrict__ ref) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = a[i];
  double got = 0.0, want = __builtin_nan("");
  switch (fn) {
    case kDiv: got = frei::fm::div(x, b[i]); want = x / b[i]; break;
    case kSqrt: got = frei::fm::sqrt(x); want = ::sqrt(x); break;
    case kSqrtPos: got = frei::fm::sqrt_pos(x); want = ::sqrt(x); break;
    case kRcpNr: got = frei::fm::rcp_nr(x); want = 1.0 / x; break;
    case kExpNeg: got = frei::fm::exp_neg(x); want = ::exp(x); break;
    case kExpNegNf: got = frei::fm::exp_neg_nf(x); want = ::exp(x); break;
    case kExpNegUnclamped: got = frei::fm::exp_neg_unclamped(x); want = ::exp(x); break;
    case kPlanck: got = frei::planck(x, b[i], c[i]); break;
    case kPlanckEm: got = frei::planck_em(x, b[i], c[i]); break;
    case kShellStep: {
      double e = 1.0, u = 0.0, v = 0.0;
      frei::shell_step(e, x, 0.0, 0.0);
      frei::shell_step(u, x, 1.0, 0.0);
      frei::shell_step(v, x, 0.0, 1.0);
      out[n + i] = u;
      out[2 * n + i] = v;
      got = e;
      break;
    }
    default: break;
  }
  out[i] = got;
  ref[i] = want;
}

}  // namespace

extern "C" int frei_mathprobe(int fn, int64_t n, const double* a, const double* b,
                              const double* c, double* out, double* dev_ref) {
  if (fn < 0 || fn >= kFnCount || n <= 0 || n > (int64_t(1) << 24) || !a || !out || !dev_ref)
    return (int)hipErrorInvalidValue;
  const bool needs_b = fn == kDiv || fn == kPlanck || fn == kPlanckEm;
  const bool needs_c = fn == kPlanck || fn == kPlanckEm;
  if ((needs_b && !b) || (needs_c && !c)) return (int)hipErrorInvalidValue;
  const size_t bytes = (size_t)n * sizeof(double);
  const size_t n_out = fn == kShellStep ? 3 : 1;
  double *d_in = nullptr, *d_out = nullptr;
  // one allocation for a, b, c and one for out (1 or 3 blocks) followed by dev_ref
  hipError_t err = hipMalloc(&d_in, 3 * bytes);
  if (err == hipSuccess) err = hipMalloc(&d_out, (n_out + 1) * bytes);
  if (err == hipSuccess) err = hipMemset(d_in, 0, 3 * bytes);
  if (err == hipSuccess) err = hipMemcpy(d_in, a, bytes, hipMemcpyHostToDevice);
  if (err == hipSuccess && needs_b) err = hipMemcpy(d_in + n, b, bytes, hipMemcpyHostToDevice);
  if (err == hipSuccess && needs_c)
    err = hipMemcpy(d_in + 2 * n, c, bytes, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(probe, dim3(blocks), dim3(256), 0, 0, fn, n, d_in, d_in + n, d_in + 2 * n,
                       d_out, d_out + n_out * n);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out, d_out, n_out * bytes, hipMemcpyDeviceToHost);
  if (err == hipSuccess)
    err = hipMemcpy(dev_ref, d_out + n_out * n, bytes, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)err;
}
