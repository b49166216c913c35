// frei_stellar.hip — K8: binning of high-resolution stellar model spectra onto a grid's
// wavelength bins (frei/phoenix.py:13-17, 43-52 get_binned_phoenix_spectrum: xarray
// groupby_bins + integrate / (max - min) per group).
//
// Data: a library of spectra on one shared wavelength axis stays resident in HBM as float64
// [n_spec][n_hi].  The host builds the plan once per call — pandas.cut(right=True) edge
// positions pos[k] = upper_bound(wl_hi, wl_bins[k]), so bin k holds the points [pos[k],
// pos[k+1]) (every bin right-closed, the last included: no cropping of the axis as K6 does) —
// and one of two kernels writes the aligned result out[n_spec][n_bins], NaN for bins of fewer
// than two points:
//   lane per bin (form 1): consecutive lanes take consecutive bins and walk their few points
//     in order (fine grids, 0 to a few points per bin);
//   wave per bin (form 2): the 64 lanes stride the bin's intervals with coalesced 8-byte loads
//     and combine their partial sums in a fixed xor butterfly (coarse grids, hundreds to
//     thousands of points per bin); where the bins hold fewer points than a wave has lanes the
//     wave splits into groups of 4 to 32 lanes, one group per bin.
// A block takes a tile of kTile spectra for its bins: dx is formed once per interval and the
// wavelength axis is read once per tile, not once per spectrum.  No atomics: each form is
// bitwise reproducible.  Terms (dx * 0.5) * (y[i+1] + y[i]) round as numpy's (no contraction).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

struct frei_sspec {
  Stream stream;   // first: destroyed last
  int device = 0;
  int n_spec = 0;
  int64_t nhi = 0;
  std::vector<double> wl;     // µm, strictly ascending
  DevBuf<double> d_flux;   // [n_spec][nhi]
  DevBuf<double> d_wl;     // [nhi]
  DevBuf<int64_t> d_pos;   // [n_bins + 1] plan of the last call (kept between calls, grow-only)
  DevBuf<double> d_out;    // [n_spec][n_bins] result of the last call (grow-only)
  ~frei_sspec() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

namespace {

constexpr int kTile = 4;   // spectra per block
// form 0: form 2 from this many points per non-empty bin on.  Measured on MI355X
// (tools/stellar_bin_probe.py, 64 spectra x 1.525 M points; profiles/r07/stellar_bin/README.md):
// at 3.0 points per bin the lane-per-bin form takes 0.232 ms against 0.256 ms, at 5.0 points
// 0.302 ms against 0.201 ms: the crossover lies between, at about 4.
constexpr double kWavePerBinFrom = 4.0;

__device__ __forceinline__ double quiet_nan() {
  return __longlong_as_double(0x7ff8000000000000ll);
}

// The rows of this block's spectra tile: nr <= kTile valid ones, the others alias the first
// (read, never stored).
__device__ __forceinline__ int tile_rows(const double* __restrict__ flux, int64_t nhi, int n_spec,
                                         const double* (&rows)[kTile]) {
  const int r0 = blockIdx.y * kTile;
  const int nr = min(kTile, n_spec - r0);
#pragma unroll
  for (int r = 0; r < kTile; ++r) rows[r] = flux + (int64_t)(r0 + (r < nr ? r : 0)) * nhi;
  return nr;
}

// form 1: one lane per bin, its points in order.
__global__ __launch_bounds__(256) void sspec_lane_kernel(
    const double* __restrict__ flux, const double* __restrict__ wl,
    const int64_t* __restrict__ pos, int64_t nb, int64_t nhi, int n_spec,
    double* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  const double* rows[kTile];
  const int nr = tile_rows(flux, nhi, n_spec, rows);
  const int64_t s = pos[k], e = pos[k + 1];
  double v[kTile];
  if (e - s >= 2) {
    double acc[kTile], y0[kTile];
    double x0 = wl[s];
#pragma unroll
    for (int r = 0; r < kTile; ++r) {
      acc[r] = 0.0;
      y0[r] = rows[r][s];
    }
    for (int64_t i = s + 1; i < e; ++i) {
      const double x1 = wl[i];
      const double hdx = (x1 - x0) * 0.5;
#pragma unroll
      for (int r = 0; r < kTile; ++r) {
        const double y1 = rows[r][i];
        acc[r] = acc[r] + hdx * (y1 + y0[r]);
        y0[r] = y1;
      }
      x0 = x1;
    }
    const double D = x0 - wl[s];
#pragma unroll
    for (int r = 0; r < kTile; ++r) v[r] = acc[r] / D;
  } else {
#pragma unroll
    for (int r = 0; r < kTile; ++r) v[r] = quiet_nan();
  }
  const int r0 = blockIdx.y * kTile;
  for (int r = 0; r < nr; ++r) out[(int64_t)(r0 + r) * nb + k] = v[r];
}

// form 2: one wave per bin — in general one group of G lanes per bin, G = 64 (a whole wave, 4
// bins per block) for the coarse grids it is meant for and 8, 16 or 32 where the bins hold
// fewer points than a wave has lanes (256 / G bins per block, consecutive groups on consecutive
// bins, so a wave's loads still fall on neighbouring lines).  Lane l of the group sums the
// intervals s + l, s + l + G, ... in order; the G partial sums combine in the xor butterfly
// G/2, ..., 2, 1 (a + b is commutative, so every lane ends with the same bits); lane 0 divides
// and stores.  Every lane of a wave reaches the butterfly (no early exit).
template <int G>
__global__ __launch_bounds__(256) void sspec_wave_kernel(
    const double* __restrict__ flux, const double* __restrict__ wl,
    const int64_t* __restrict__ pos, int64_t nb, int64_t nhi, int n_spec,
    double* __restrict__ out) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t k = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;   // group-uniform
  const bool valid = k < nb;
  const double* rows[kTile];
  const int nr = tile_rows(flux, nhi, n_spec, rows);
  const int64_t s = valid ? pos[k] : 0, e = valid ? pos[k + 1] : 0;
  double acc[kTile];
#pragma unroll
  for (int r = 0; r < kTile; ++r) acc[r] = 0.0;
  for (int64_t i = s + lane; i + 1 < e; i += G) {
    const double hdx = (wl[i + 1] - wl[i]) * 0.5;
#pragma unroll
    for (int r = 0; r < kTile; ++r) acc[r] = acc[r] + hdx * (rows[r][i + 1] + rows[r][i]);
  }
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1)
#pragma unroll
    for (int r = 0; r < kTile; ++r) acc[r] = acc[r] + __shfl_xor(acc[r], off);
  if (valid && lane == 0) {
    const bool two = e - s >= 2;
    const double D = two ? wl[e - 1] - wl[s] : 1.0;
    const int r0 = blockIdx.y * kTile;
    for (int r = 0; r < nr; ++r)
      out[(int64_t)(r0 + r) * nb + k] = two ? acc[r] / D : quiet_nan();
  }
}

template <int G>
void launch_wave(const frei_sspec* s, int64_t n_bins, unsigned tiles, hipStream_t st) {
  constexpr int per = 256 / G;
  dim3 grid((unsigned)((n_bins + per - 1) / per), tiles);
  sspec_wave_kernel<G><<<grid, 256, 0, st>>>(s->d_flux, s->d_wl, s->d_pos, n_bins, s->nhi,
                                             s->n_spec, s->d_out);
}

// Lanes per bin of form 2 from the mean points per non-empty bin.  Measured with one group size
// forced at a time (same probe and file; ms at 5 / 10 / 15 / 21 / 37 / 75 / 300 points per bin):
//   G = 4   0.201 0.188 0.213 0.236 0.264 0.295 0.344
//   G = 8   0.282 0.195 0.182 0.182 0.188 0.196 0.248
//   G = 16  0.534 0.284 0.223 0.186 0.163 0.158 0.167
//   G = 32  1.109 0.572 0.390 0.287 0.196 0.151 0.134
//   G = 64  2.443 1.245 0.839 0.593 0.348 0.202 0.132
// The thresholds sit between the measured points on either side of each change of the fastest.
int wave_group(double mean_points) {
#ifdef FREI_SSPEC_GROUP   // A/B builds (tools/build_variant.sh): one group size throughout
  (void)mean_points;
  return FREI_SSPEC_GROUP;
#else
  return mean_points >= 300.0 ? 64 : mean_points >= 53.0 ? 32 : mean_points >= 28.0 ? 16
         : mean_points >= 12.0 ? 8 : 4;
#endif
}

}  // namespace

// ==================================================================== C ABI
extern "C" {

int frei_sspec_create(frei_sspec** out, int device, const double* flux, int n_spec, int64_t n_hi,
                      const double* wl_hi) {
  if (!out || !flux || !wl_hi) return set_error("null argument");
  *out = nullptr;
  if (n_spec < 1) return set_error("frei_sspec_create: n_spec must be >= 1");
  if (n_hi < 2) return set_error("frei_sspec_create: n_hi must be >= 2");
  if (int rc = check_ascending(wl_hi, n_hi, "high-resolution wavelengths")) return rc;
  frei_sspec* s = new frei_sspec();
  s->device = device;
  s->n_spec = n_spec;
  s->nhi = n_hi;
  s->wl.assign(wl_hi, wl_hi + n_hi);
  const size_t nflux = (size_t)n_spec * n_hi;
  if (hipSetDevice(device) != hipSuccess || s->stream.create() || s->d_flux.alloc(nflux) ||
      s->d_wl.alloc((size_t)n_hi)) {
    delete s;
    (void)hipGetLastError();
    return set_error("frei_sspec_create: device allocation failed");
  }
  if (hipMemcpy(s->d_flux, flux, nflux * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(s->d_wl, wl_hi, (size_t)n_hi * sizeof(double), hipMemcpyHostToDevice) !=
          hipSuccess) {
    delete s;
    (void)hipGetLastError();
    return set_error("frei_sspec_create: host-to-device copy failed");
  }
  *out = s;
  return 0;
}

int frei_sspec_destroy(frei_sspec* s) {
  if (s) delete s;
  return 0;
}

int frei_sspec_bin(frei_sspec* s, const double* wl_bins, int64_t n_bins, int form, double* out,
                   int64_t* counts, int* form_used, double* kernel_ms) {
  // the arguments that need no handle first: testable without a device
  if (!wl_bins) return set_error("null argument");
  if (n_bins < 1) return set_error("frei_sspec_bin: n_bins must be >= 1");
  if (form < 0 || form > 2)
    return set_error("frei_sspec_bin: form must be 0 (automatic), 1 (lane per bin) or 2 (wave per bin)");
  if (int rc = check_ascending(wl_bins, n_bins + 1, "wl_bins")) return rc;
  if (!s) return set_error("null argument");
  // plan: pandas.cut(right=True) edge positions, bin k = points [pos[k], pos[k+1])
  const std::vector<double>& wl = s->wl;
  std::vector<int64_t> pos((size_t)n_bins + 1);
  for (int64_t k = 0; k <= n_bins; ++k)
    pos[k] = std::upper_bound(wl.begin(), wl.end(), wl_bins[k]) - wl.begin();
  int64_t filled = 0;
  for (int64_t k = 0; k < n_bins; ++k) {
    if (counts) counts[k] = pos[k + 1] - pos[k];
    filled += pos[k + 1] > pos[k];
  }
  const int64_t P = pos[n_bins] - pos[0];
  const double mean_points = filled > 0 ? (double)P / (double)filled : 0.0;
  int f = form;
  if (f == 0) f = mean_points >= kWavePerBinFrom ? 2 : 1;
  if (form_used) *form_used = f;

  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const size_t total = (size_t)s->n_spec * n_bins;
  // d_pos and d_out are the handle's, kept between calls: the call owns nothing
  DeviceCall call(st, "stellar binning");
  call.check(s->d_pos.reserve(pos.size()));
  if (call.ok()) call.check(s->d_out.reserve(total));
  call.copy_in(s->d_pos, pos.data(), pos.size());
  call.begin(kernel_ms);
  if (call.ok()) {
    const unsigned tiles = (unsigned)((s->n_spec + kTile - 1) / kTile);
    if (f == 1) {
      dim3 grid((unsigned)((n_bins + 255) / 256), tiles);
      sspec_lane_kernel<<<grid, 256, 0, st>>>(s->d_flux, s->d_wl, s->d_pos, n_bins, s->nhi,
                                              s->n_spec, s->d_out);
    } else {
      switch (wave_group(mean_points)) {
        case 4: launch_wave<4>(s, n_bins, tiles, st); break;
        case 8: launch_wave<8>(s, n_bins, tiles, st); break;
        case 16: launch_wave<16>(s, n_bins, tiles, st); break;
        case 32: launch_wave<32>(s, n_bins, tiles, st); break;
        default: launch_wave<64>(s, n_bins, tiles, st); break;
      }
    }
  }
  call.end();
  call.download(out, s->d_out, total);
  return call.finish();
}

}  // extern "C"
