// frei_observe.hip — K10: synthetic observations.  Native-resolution spectra x[n_atm][n_lam]
// are taken to the K channels of an instrument and, on request, scored against data (chi^2).
// The reference has no counterpart; the definition is the header comment of frei_obs_apply in
// include/frei_hip.h.
//
// Data: the plan (first, count, offsets: int64) and the weights stay resident in HBM with the
// handle, uploaded once at creation.  Per call one of two kernels writes obs[n_atm][K]:
//   lane per channel (form 1): consecutive lanes take consecutive channels and walk their few
//     points in order (photometry of a coarse grid, narrow spectrograph bins);
//   group per channel (form 2): G = 4 .. 64 lanes stride one channel's points with coalesced
//     8-byte loads and combine their partial sums in the fixed xor butterfly G/2, ..., 2, 1
//     (broad bands, line-spread functions of hundreds to thousands of points).
// A block takes a tile of kTile atmospheres for its channels, so plan and weights are read once
// per tile; rows past n_atm alias the tile's first row (read, never stored).  `select` gives
// every atmosphere of a tile its own num / den library row.  Every atmosphere has its own
// accumulators and a channel's order of summation depends on the plan alone: row m of a batched
// call is bitwise the call on that row alone.  No atomics, no LDS, no barrier; products are not
// contracted.  chi^2 is a second small launch, one wave per atmosphere.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

struct frei_obs {
  Stream stream;   // first: destroyed last
  int device = 0;
  int64_t n_lam = 0, K = 0, nnz = 0;
  DevBuf<int64_t> d_plan;   // first[K], count[K], off[K]
  DevBuf<double> d_w;       // [nnz]
  ~frei_obs() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

namespace {

constexpr int kTile = 4;   // atmospheres per block
// form 0: form 2 above this many points per channel.  The value is K8's (frei_stellar.hip
// kWavePerBinFrom), inherited.  Measured for this kernel on MI355X (tools/observe_probe.py, 64
// atmospheres x 100k wavelengths, no library, the forms taking turns over 15 rounds;
// profiles/r09/observe/README.md), lane form against group form, median ms: 0.023 / 0.032 at 2
// points per channel, 0.027 / 0.026 at 3 (a tie within the spread), 0.025 / 0.023 at 4 (0.093 /
// 0.077 at 500k), 0.026 / 0.023 at 5, 0.029 / 0.023 at 6, 0.050 / 0.021 at 8.  The crossover
// lies near 3; the constant stays at 4 with channels of exactly 4 points on the lane form, which
// the feature's specification pins (tests/test_gpu_observe.py, test_both_regimes), at a measured
// cost of 9 to 17 % for such instruments at 500k.
constexpr double kGroupPerChannelFrom = 4.0;

struct ObsArgs {
  const double* x;        // row m at x + m * xs
  int64_t xs;
  const double* num;      // [n_lib][n] or null
  const double* den;      // [n_lib][n] or null
  const int32_t* select;  // [n_atm] or null (row 0)
  const double* scale;    // [n_atm] or null (1)
  const int64_t *first, *count, *off;
  const double* w;
  int64_t K, n;
  int n_atm;
  double* obs;            // [n_atm][K]
};

// The rows of this block's atmosphere tile: nr <= kTile valid ones, the others alias the first
// (read, never stored).
template <bool NUM, bool DEN>
__device__ __forceinline__ int tile_rows(const ObsArgs& a, const double* (&xr)[kTile],
                                         const double* (&nu)[kTile],
                                         const double* (&de)[kTile]) {
  const int r0 = blockIdx.y * kTile;
  const int nr = min(kTile, a.n_atm - r0);
#pragma unroll
  for (int r = 0; r < kTile; ++r) {
    const int m = r0 + (r < nr ? r : 0);
    const int64_t lib = (a.select ? (int64_t)a.select[m] : 0) * a.n;
    xr[r] = a.x + (int64_t)m * a.xs;
    nu[r] = NUM ? a.num + lib : nullptr;
    de[r] = DEN ? a.den + lib : nullptr;
  }
  return nr;
}

// One point of a channel for every row of the tile: N += (w x) num, D += w den.
template <bool NUM, bool DEN>
__device__ __forceinline__ void point(double w, int64_t i, const double* (&xr)[kTile],
                                      const double* (&nu)[kTile], const double* (&de)[kTile],
                                      double (&N)[kTile], double (&D)[kTile]) {
#pragma unroll
  for (int r = 0; r < kTile; ++r) {
    double p = w * xr[r][i];
    if (NUM) p = p * nu[r][i];
    N[r] = N[r] + p;
    if (DEN) D[r] = D[r] + w * de[r][i];
  }
}

__device__ __forceinline__ void store_tile(const ObsArgs& a, int nr, int64_t k,
                                           const double (&N)[kTile], const double (&D)[kTile]) {
  const int r0 = blockIdx.y * kTile;
  for (int r = 0; r < nr; ++r) {
    const double v = N[r] / D[r];
    a.obs[(int64_t)(r0 + r) * a.K + k] = a.scale ? a.scale[r0 + r] * v : v;
  }
}

// form 1: one lane per channel, its points in order.
template <bool NUM, bool DEN>
__global__ __launch_bounds__(256) void obs_lane_kernel(const ObsArgs a) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.K) return;
  const double *xr[kTile], *nu[kTile], *de[kTile];
  const int nr = tile_rows<NUM, DEN>(a, xr, nu, de);
  const int64_t s = a.first[k], c = a.count[k];
  const double* __restrict__ w = a.w + a.off[k];
  double N[kTile], D[kTile], sw = 0.0;
#pragma unroll
  for (int r = 0; r < kTile; ++r) N[r] = D[r] = 0.0;
  for (int64_t t = 0; t < c; ++t) {
    const double wt = w[t];
    if (!DEN) sw = sw + wt;
    point<NUM, DEN>(wt, s + t, xr, nu, de, N, D);
  }
  if (!DEN) {
#pragma unroll
    for (int r = 0; r < kTile; ++r) D[r] = sw;
  }
  store_tile(a, nr, k, N, D);
}

// form 2: one group of G lanes per channel (256 / G channels per block, consecutive groups on
// consecutive channels).  Lane l of the group sums the points l, l + G, ... in order; the G
// partial sums combine in the xor butterfly G/2, ..., 2, 1 (a + b is commutative, so every lane
// ends with the same bits); lane 0 divides and stores.  Every lane of a wave reaches the
// butterfly (no early exit).
template <int G, bool NUM, bool DEN>
__global__ __launch_bounds__(256) void obs_group_kernel(const ObsArgs a) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t k = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;   // group-uniform
  const bool valid = k < a.K;
  const double *xr[kTile], *nu[kTile], *de[kTile];
  const int nr = tile_rows<NUM, DEN>(a, xr, nu, de);
  const int64_t s = valid ? a.first[k] : 0, c = valid ? a.count[k] : 0;
  const double* __restrict__ w = a.w + (valid ? a.off[k] : 0);
  double N[kTile], D[kTile], sw = 0.0;
#pragma unroll
  for (int r = 0; r < kTile; ++r) N[r] = D[r] = 0.0;
  for (int64_t t = lane; t < c; t += G) {
    const double wt = w[t];
    if (!DEN) sw = sw + wt;
    point<NUM, DEN>(wt, s + t, xr, nu, de, N, D);
  }
#pragma unroll
  for (int o = G / 2; o >= 1; o >>= 1) {
    if (!DEN) sw = sw + __shfl_xor(sw, o);
#pragma unroll
    for (int r = 0; r < kTile; ++r) {
      N[r] = N[r] + __shfl_xor(N[r], o);
      if (DEN) D[r] = D[r] + __shfl_xor(D[r], o);
    }
  }
  if (!DEN) {
#pragma unroll
    for (int r = 0; r < kTile; ++r) D[r] = sw;
  }
  if (valid && lane == 0) store_tile(a, nr, k, N, D);
}

// chi^2: one wave per atmosphere, lane l takes the channels l, l + 64, ... in order, then the
// butterfly 32, ..., 1.  A channel of infinite sigma contributes exactly 0.
__global__ __launch_bounds__(64) void obs_chi2_kernel(const double* __restrict__ obs,
                                                      const double* __restrict__ data,
                                                      const double* __restrict__ sigma, int64_t K,
                                                      double* __restrict__ chi2) {
  const int m = blockIdx.x;
  const double* __restrict__ row = obs + (int64_t)m * K;
  double acc = 0.0;
  for (int64_t k = threadIdx.x; k < K; k += 64) {
    const double sg = sigma[k];
    const double r = (row[k] - data[k]) / sg;
    acc = acc + (isinf(sg) ? 0.0 : r * r);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = acc + __shfl_xor(acc, o);
  if (threadIdx.x == 0) chi2[m] = acc;
}

template <bool NUM, bool DEN>
void launch_form(int f, int G, const ObsArgs& a, hipStream_t st) {
  const unsigned tiles = (unsigned)((a.n_atm + kTile - 1) / kTile);
  auto grid = [&](int per) { return dim3((unsigned)((a.K + per - 1) / per), tiles); };
  if (f == 1) {
    obs_lane_kernel<NUM, DEN><<<grid(256), 256, 0, st>>>(a);
    return;
  }
  switch (G) {
    case 4: obs_group_kernel<4, NUM, DEN><<<grid(64), 256, 0, st>>>(a); break;
    case 8: obs_group_kernel<8, NUM, DEN><<<grid(32), 256, 0, st>>>(a); break;
    case 16: obs_group_kernel<16, NUM, DEN><<<grid(16), 256, 0, st>>>(a); break;
    case 32: obs_group_kernel<32, NUM, DEN><<<grid(8), 256, 0, st>>>(a); break;
    default: obs_group_kernel<64, NUM, DEN><<<grid(4), 256, 0, st>>>(a); break;
  }
}

// Lanes per channel of form 2 from the mean points per channel: K8's measured thresholds
// (frei_stellar.hip wave_group), inherited; with them the group form runs at 0.69 to 0.73 of the
// HBM peak from 4 to 3000 points per channel (same probe, 64 x 500k, no library).
int group_lanes(double mean_points) {
  return mean_points >= 300.0 ? 64 : mean_points >= 53.0 ? 32 : mean_points >= 28.0 ? 16
         : mean_points >= 12.0 ? 8 : 4;
}

}  // namespace

// ==================================================================== C ABI
extern "C" {

int frei_obs_create(frei_obs** out, int device, int64_t n_lam, int64_t n_chan,
                    const int64_t* first, const int64_t* count, const double* weights) {
  // the plan is validated on the host before any device call
  if (!out || !first || !count || !weights) return set_error("null argument");
  *out = nullptr;
  if (n_lam < 1) return set_error("frei_obs_create: n_lam must be >= 1");
  if (n_chan < 1) return set_error("frei_obs_create: n_chan must be >= 1");
  std::vector<int64_t> plan((size_t)n_chan * 3);
  int64_t nnz = 0;
  for (int64_t k = 0; k < n_chan; ++k) {
    const std::string ch = "channel " + std::to_string(k);
    if (count[k] < 1) return set_error("frei_obs_create: " + ch + " has count < 1");
    if (first[k] < 0 || first[k] > n_lam || count[k] > n_lam - first[k])
      return set_error("frei_obs_create: " + ch + " has a range outside the axis [0, " +
                       std::to_string(n_lam) + ")");
    double sum = 0.0;
    for (int64_t t = 0; t < count[k]; ++t) {
      const double w = weights[nnz + t];
      if (!std::isfinite(w) || w < 0.0)
        return set_error("frei_obs_create: " + ch + " has a negative or non-finite weight");
      sum += w;
    }
    if (!(sum > 0.0)) return set_error("frei_obs_create: " + ch + " has a zero weight sum");
    plan[k] = first[k];
    plan[n_chan + k] = count[k];
    plan[2 * n_chan + k] = nnz;
    nnz += count[k];
  }
  frei_obs* o = new frei_obs();
  o->device = device;
  o->n_lam = n_lam;
  o->K = n_chan;
  o->nnz = nnz;
  if (hipSetDevice(device) != hipSuccess || o->stream.create() || o->d_plan.alloc(plan.size()) ||
      o->d_w.alloc((size_t)nnz)) {
    delete o;
    (void)hipGetLastError();
    return set_error("frei_obs_create: device allocation failed");
  }
  if (hipMemcpy(o->d_plan, plan.data(), plan.size() * sizeof(int64_t), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(o->d_w, weights, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice) !=
          hipSuccess) {
    delete o;
    (void)hipGetLastError();
    return set_error("frei_obs_create: host-to-device copy failed");
  }
  *out = o;
  return 0;
}

int frei_obs_destroy(frei_obs* o) {
  if (o) delete o;
  return 0;
}

// The five sources of x — a host array, a context's emergent rows, a broadener's kept result
// (K13), an interpolator's (K15), a phase integrator's (K16) — feed the same x and stride below.
static int obs_apply_impl(frei_obs* o, frei_ctx* ctx, const double* x, frei_brd* brd,
                          frei_itp* itp, frei_phs* phs, int n_atm, const double* num,
                          const double* den, int n_lib, const int32_t* select,
                          const double* scale, const double* data, const double* sigma, int form,
                          double* obs, double* chi2, int* form_used, double* kernel_ms) {
  if (!o || !obs) return set_error("frei_obs_apply: null handle or null obs");
  if (!x && !ctx && !brd && !itp && !phs)
    return set_error("frei_obs_apply: x and ctx are both null");
  if (n_atm < 1) return set_error("frei_obs_apply: n_atm must be >= 1");
  if (form < 0 || form > 2)
    return set_error("frei_obs_apply: form must be 0 (automatic), 1 (lane per channel) or 2 "
                     "(group per channel)");
  const bool lib = num || den;
  if (lib && n_lib < 1) return set_error("frei_obs_apply: n_lib must be >= 1 with num or den");
  if (lib) TRY(check_select("frei_obs_apply", select, n_atm, n_lib));
  if (chi2) {
    if (!data || !sigma) return set_error("frei_obs_apply: chi2 requested without data or sigma");
    for (int64_t k = 0; k < o->K; ++k)
      if (!(sigma[k] > 0.0))
        return set_error("frei_obs_apply: sigma[" + std::to_string(k) +
                         "] must be > 0 (+inf removes the channel)");
  }
  SpectrumRows src;
  TRY(spectrum_rows(x, ctx, brd, itp, phs, n_atm, o->n_lam, o->device, o->stream, "instrument",
                    "frei_obs_apply", &src));
  const double mean_points = (double)o->nnz / (double)o->K;
  int f = form;
  if (f == 0) f = mean_points > kGroupPerChannelFrom ? 2 : 1;
  if (form_used) *form_used = f;

  HIP_TRY(hipSetDevice(o->device));
  hipStream_t st = src.stream;
  const size_t A = (size_t)n_atm, n = (size_t)o->n_lam, K = (size_t)o->K;
  DeviceCall call(st, "observation");
  ObsArgs a;
  const double* u_x = call.upload(x, A * n);
  a.x = u_x ? u_x : src.rows;
  a.xs = src.stride;
  a.num = call.upload(num, (size_t)n_lib * n);
  a.den = call.upload(den, (size_t)n_lib * n);
  a.select = call.upload(lib ? select : nullptr, A);
  a.scale = call.upload(scale, A);
  a.first = o->d_plan;
  a.count = o->d_plan + K;
  a.off = o->d_plan + 2 * K;
  a.w = o->d_w;
  a.K = o->K;
  a.n = o->n_lam;
  a.n_atm = n_atm;
  a.obs = call.alloc<double>(A * K);
  const double* d_data = call.upload(chi2 ? data : nullptr, K);
  const double* d_sigma = call.upload(chi2 ? sigma : nullptr, K);
  double* d_chi2 = chi2 ? call.alloc<double>(A) : nullptr;
  call.begin(kernel_ms);
  if (call.ok()) {
    const int G = group_lanes(mean_points);
    if (num && den) launch_form<true, true>(f, G, a, st);
    else if (num) launch_form<true, false>(f, G, a, st);
    else if (den) launch_form<false, true>(f, G, a, st);
    else launch_form<false, false>(f, G, a, st);
    if (chi2)
      obs_chi2_kernel<<<dim3((unsigned)n_atm), 64, 0, st>>>(a.obs, d_data, d_sigma, o->K, d_chi2);
  }
  call.end();
  call.download(obs, a.obs, A * K);
  call.download(chi2, d_chi2, A);
  return call.finish();
}

int frei_obs_apply(frei_obs* o, frei_ctx* ctx, const double* x, int n_atm, const double* num,
                   const double* den, int n_lib, const int32_t* select, const double* scale,
                   const double* data, const double* sigma, int form, double* obs, double* chi2,
                   int* form_used, double* kernel_ms) {
  return obs_apply_impl(o, ctx, x, nullptr, nullptr, nullptr, n_atm, num, den, n_lib, select, scale,
                        data, sigma, form, obs, chi2, form_used, kernel_ms);
}

int frei_obs_apply_brd(frei_obs* o, frei_brd* src, int n_atm, const double* num,
                       const double* den, int n_lib, const int32_t* select, const double* scale,
                       const double* data, const double* sigma, int form, double* obs,
                       double* chi2, int* form_used, double* kernel_ms) {
  if (!src) return set_error("frei_obs_apply_brd: null broadener");
  return obs_apply_impl(o, nullptr, nullptr, src, nullptr, nullptr, n_atm, num, den, n_lib, select,
                        scale, data, sigma, form, obs, chi2, form_used, kernel_ms);
}

int frei_obs_apply_itp(frei_obs* o, frei_itp* src, int n_atm, const double* num,
                       const double* den, int n_lib, const int32_t* select, const double* scale,
                       const double* data, const double* sigma, int form, double* obs,
                       double* chi2, int* form_used, double* kernel_ms) {
  if (!src) return set_error("frei_obs_apply_itp: null interpolator");
  return obs_apply_impl(o, nullptr, nullptr, nullptr, src, nullptr, n_atm, num, den, n_lib, select,
                        scale, data, sigma, form, obs, chi2, form_used, kernel_ms);
}

int frei_obs_apply_phs(frei_obs* o, frei_phs* src, int n_atm, const double* num,
                       const double* den, int n_lib, const int32_t* select, const double* scale,
                       const double* data, const double* sigma, int form, double* obs,
                       double* chi2, int* form_used, double* kernel_ms) {
  if (!src) return set_error("frei_obs_apply_phs: null phase integrator");
  return obs_apply_impl(o, nullptr, nullptr, nullptr, nullptr, src, n_atm, num, den, n_lib, select,
                        scale, data, sigma, form, obs, chi2, form_used, kernel_ms);
}

}  // extern "C"
