// frei_transit.hip — K9: transmission (transit-depth) spectrum of a converged atmosphere from
// the final emit's vertical optical depths (frei_transit).  The reference has no counterpart;
// the definition is the header comment of frei_transit in include/frei_hip.h.
//
// Per atmosphere the host hands over the nL level radii r_1 < ... < r_nL (r[k] = r_{k+1}) and
// builds the chord weights once per call (transit_build_weights):
//   G[i][j] = 2 (r_{j+1} + r_j) / (s(i, j+1) + s(i, j)),  s(i, k) = sqrt((r_k - r_i)(r_k + r_i)),
// for shells 1 <= i <= j <= nL - 1 (shell l lies between levels l and l + 1, its vertical
// optical depth is row l of dtaus; row 0 is never read).  One lane per wavelength, grid
// (256-wavelength blocks, atmosphere):
//   tau_i = sum_{j = i}^{nL-1} G[i][j] dtaus[j]      ascending j, starting from the j = i term
//   f_i   = -expm1(-tau_i),  f_nL = 0
//   A     = r_1 r_1 + sum_{i = 1}^{nL-1} (f_i r_i + f_{i+1} r_{i+1}) (r_{i+1} - r_i)   ascending i
//   depth = A / (R_star R_star)
// The triangular product runs over tiles of kTile tangent levels: kTile accumulators per column
// live in registers while the lane walks the column from the tile's first shell upwards, so a
// column is read about ceil((nL - 1) / kTile) / 2 times, the re-reads from L2 (140 loads for the
// 59 shells of nL = 60 at kTile = 16).  The weights are wave-uniform and stored in the order the
// walk reads them (per tile, per shell, kTile values), so they arrive through scalar loads and
// cost no vector register or LDS; that also serves any nL up to kMaxLayers straight from global
// memory.  Whatever the tiling, every tau_i and A are the same operations in the same order:
// bitwise reproducible, and identical between a single and a batched context.  No atomics, no
// LDS, no barrier.
//
// Measured (MI355X, 60 layers; profiles/r08/transit/README.md): 0.139 ms for 500k wavelengths,
// 1.58 ms for 64 atmospheres x 100k; the multiply-add pairs alone run at 0.32-0.37 of the
// unfused fp64 vector rate and the algorithmic bytes at 0.22-0.24 of the HBM peak: fp64 issue
// is the nearer bound.  Tiles of 4, 8 and 32 levels and deeper column prefetch were slower; two
// columns per lane (kLams = 2: every weight loaded serves two columns) measured 6 % faster and
// is kept as an A/B switch, the kernel's contract being one lane per wavelength.
#include <cmath>
#include <vector>

#include "frei_device.h"

namespace frei {
namespace {

// Tangent levels per pass, wavelengths per lane and shells per group above a tile (a group's
// column values are loaded while the group before it is summed).  Measured on MI355X
// (tools/transit_probe.py, profiles/r08/transit/README.md).
#ifdef FREI_TRANSIT_TILE   // A/B builds (tools/build_variant.sh)
constexpr int kTile = FREI_TRANSIT_TILE;
#else
constexpr int kTile = 16;
#endif
#ifdef FREI_TRANSIT_LAMS
constexpr int kLams = FREI_TRANSIT_LAMS;
#else
constexpr int kLams = 1;
#endif
#ifdef FREI_TRANSIT_AHEAD
constexpr int kAhead = FREI_TRANSIT_AHEAD;
#else
constexpr int kAhead = 2;
#endif

// A block takes 256 * NV consecutive wavelengths, lane t the NV columns j0 + t + 256 v: every
// weight a wave loads serves NV columns.  A column past the end repeats the lane's first one
// (summed, never stored).
template <int TI, int NV, bool TAU>
__global__ __launch_bounds__(256) void transit_kernel(
    const double* __restrict__ dtaus,   // [n_atm][nL][n]
    const double* __restrict__ radii,   // [n_atm][nL]
    const double* __restrict__ w,       // [n_atm][w_stride] tiled chord weights
    int64_t w_stride, double rs2,       // R_star * R_star
    double* __restrict__ depth,         // [n_atm][n]
    double* __restrict__ tau_out,       // [n_atm][nL - 1][n] (TAU)
    int nL, int64_t n) {
  const int m = blockIdx.y;
  const int64_t j0 = (int64_t)blockIdx.x * (256 * NV);   // block-uniform
  if (j0 + threadIdx.x >= n) return;
  int off[NV];
  bool own[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    own[v] = j0 + threadIdx.x + 256 * v < n;
    off[v] = threadIdx.x + (own[v] ? 256 * v : 0);
  }
  const int nS = nL - 1;                          // shells 1 .. nS
  // block-uniform bases: row l of column v is col[l * n + off[v]]
  const double* __restrict__ col = dtaus + (int64_t)m * nL * n + j0;
  const double* __restrict__ r = radii + (int64_t)m * nL;
  const double* __restrict__ g = w + (int64_t)m * w_stride;
  double* __restrict__ tau = TAU ? tau_out + (int64_t)m * nS * n + j0 : nullptr;

  double area[NV], q_prev[NV];                    // q_prev: f_{i-1} r_{i-1} of the level before
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    area[v] = r[0] * r[0];
    q_prev[v] = 0.0;
  }
  for (int i0 = 1; i0 <= nS; i0 += TI) {          // tangent levels i0 .. i0 + TI - 1
    double acc[TI][NV];
#pragma unroll
    for (int t = 0; t < TI; ++t)
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[t][v] = 0.0;
    // the tile's triangle: shell i0 + c reaches the tangent levels t <= c (rows past the last
    // shell are clamped to it: loaded, never used)
    double dt[TI][NV];
#pragma unroll
    for (int c = 0; c < TI; ++c)
#pragma unroll
      for (int v = 0; v < NV; ++v) dt[c][v] = col[(int64_t)min(i0 + c, nS) * n + off[v]];
#pragma unroll
    for (int c = 0; c < TI; ++c) {
      if (i0 + c <= nS) {
#pragma unroll
        for (int t = 0; t <= c; ++t)
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const double term = g[c * TI + t] * dt[c][v];
            acc[t][v] = (t == c) ? term : acc[t][v] + term;
          }
      }
    }
    // the shells above the tile reach all of its levels, kAhead of them per group; two buffers
    // take turns, so a group's column values load while the group before it is summed
    auto load = [&](double (&d)[kAhead][NV], int l0) {
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
#pragma unroll
        for (int v = 0; v < NV; ++v) d[u][v] = col[(int64_t)min(l0 + u, nS) * n + off[v]];
    };
    auto shell = [&](const double (&d)[kAhead][NV], int l0, int u) {
      const double* __restrict__ gl = g + (int64_t)(l0 + u - i0) * TI;
#pragma unroll
      for (int t = 0; t < TI; ++t)
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[t][v] = acc[t][v] + gl[t] * d[u][v];
    };
    auto group = [&](const double (&d)[kAhead][NV], int l0) {   // l0 + kAhead - 1 <= nS
#pragma unroll
      for (int u = 0; u < kAhead; ++u) shell(d, l0, u);
    };
    auto rest = [&](const double (&d)[kAhead][NV], int l0) {    // fewer than kAhead shells left
#pragma unroll
      for (int u = 0; u < kAhead - 1; ++u)
        if (l0 + u <= nS) shell(d, l0, u);
    };
    int l = i0 + TI;
    double da[kAhead][NV], db[kAhead][NV];
    load(da, l);
    for (; l + 2 * kAhead - 1 <= nS; l += 2 * kAhead) {
      load(db, l + kAhead);
      group(da, l);
      load(da, l + 2 * kAhead);
      group(db, l + kAhead);
    }
    if (l + kAhead - 1 <= nS) {
      load(db, l + kAhead);
      group(da, l);
      rest(db, l + kAhead);
    } else {
      rest(da, l);
    }
    g += (int64_t)(nS - i0 + 1) * TI;
#pragma unroll
    for (int t = 0; t < TI; ++t) {
      const int i = i0 + t;
      if (i <= nS) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          if constexpr (TAU)
            if (own[v]) tau[(int64_t)(i - 1) * n + off[v]] = acc[t][v];
          const double q = -expm1(-acc[t][v]) * r[i - 1];
          if (i > 1) area[v] = area[v] + (q_prev[v] + q) * (r[i - 1] - r[i - 2]);
          q_prev[v] = q;
        }
      }
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    // i = nL - 1: f_nL = 0, so f_nL r_nL = 0
    area[v] = area[v] + (q_prev[v] + 0.0) * (r[nS] - r[nS - 1]);
    if (own[v]) depth[(int64_t)m * n + j0 + off[v]] = area[v] / rs2;
  }
}

}  // namespace

int64_t transit_weight_count(int nL) {
  const int64_t nS = nL - 1;
  int64_t cnt = 0;
  for (int64_t i0 = 1; i0 <= nS; i0 += kTile) cnt += (nS - i0 + 1) * kTile;
  return cnt;
}

void transit_build_weights(const double* r, int nL, double* w) {
  const int nS = nL - 1;
  // r[k - 1] = r_k; s(i, k) = sqrt((r_k - r_i) * (r_k + r_i))
  auto s = [&](int i, int k) { return std::sqrt((r[k - 1] - r[i - 1]) * (r[k - 1] + r[i - 1])); };
  for (int i0 = 1; i0 <= nS; i0 += kTile) {
    for (int l = i0; l <= nS; ++l) {
      for (int t = 0; t < kTile; ++t) {
        const int i = i0 + t;
        double v = 0.0;                           // never read (i > l or past the last level)
        if (i <= nS && i <= l) v = 2.0 * (r[l] + r[l - 1]) / (s(i, l + 1) + s(i, l));
        *w++ = v;
      }
    }
  }
}

void launch_transit(const double* dtaus, const double* radii, const double* w, int64_t w_stride,
                    double r_star, int nL, int64_t n, int n_atm, double* depth, double* tau,
                    hipStream_t st) {
  const double rs2 = r_star * r_star;
  constexpr int per = 256 * kLams;
  const dim3 grid((unsigned)((n + per - 1) / per), (unsigned)n_atm);
  if (tau)
    hipLaunchKernelGGL((transit_kernel<kTile, kLams, true>), grid, dim3(256), 0, st, dtaus, radii,
                       w, w_stride, rs2, depth, tau, nL, n);
  else
    hipLaunchKernelGGL((transit_kernel<kTile, kLams, false>), grid, dim3(256), 0, st, dtaus,
                       radii, w, w_stride, rs2, depth, tau, nL, n);
}

}  // namespace frei
