// frei_emergent.hip — K11: emergent specific intensities I(mu) at the top of a converged
// atmosphere and their disk quadrature, the formal solution along rays through the final emit's
// vertical optical depths (frei_emergent).  The reference has no counterpart; the definition is
// the header comment of frei_emergent in include/frei_hip.h.  The dtaus are absorption optical
// depths, so this is the pure-absorption formal solution: scattering enters neither as
// extinction nor as source.
//
// One lane per wavelength, grid (256-wavelength blocks, atmosphere), as K9.  The lane walks its
// column upwards once per tile of at most kTile = 8 angles: the tile's I_k live in registers,
// each dtaus[l][j] is loaded once per tile (coalesced, kAhead shells ahead of its use), B_{l+1}
// is formed once per shell for every angle of the tile and becomes the next shell's B_l.
// 1 / mu[k], c_k = weights[k] mu[k] and 1 / T_l are wave-uniform and arrive through scalar loads.
// More than kTile angles are further passes of the same lane (the column's re-reads come from
// L2); the flux sum stays in its register across them, so it is added in ascending k whatever
// the tiling.  No LDS, no atomics, no barrier.
//
// Per (shell, angle) one exponential polynomial gives e = exp(-x), em = 1 - e and v together
// (exp_em, frei_math.h), so the step costs one exponential and one division, not two exponentials and
// a division.  Every angle's recurrence is the same operations in the same order whichever
// instantiation runs it (the library is built with -ffp-contract=off: nothing is fused but the
// explicit fma of the polynomial and of the division core), so intensity[m][k] is bitwise
// independent of the tile position, of n_mu, of whether the flux is asked for, and of a single
// or batched context.
//
// Measured (MI355X, 60 layers, flux only; profiles/r10/emergent/README.md): 0.081 / 0.173 /
// 0.298 / 0.584 ms for 1 / 4 / 8 / 16 angles at 500k wavelengths, 0.99 / 2.35 / 4.29 / 8.35 ms
// for 64 atmospheres x 100k; 7.3e11 to 9.1e11 exponentials per second, 0.37 to 0.05 of the HBM
// peak for the algorithmic bytes: fp64 vector issue is the bound at every angle count.  A tile
// of 4 angles took 12-14 % longer at 8 and 16 angles; 2 against 4 shells ahead is inside the
// spread, 8 ahead costs a wave and is slower.
#include "frei_device.h"
#include "frei_math.h"

namespace frei {
namespace {

// Angles per pass (their I_k in registers, 8 at most) and shells a column value is loaded ahead
// of its use.  Measured on MI355X (tools/emergent_probe.py, profiles/r10/emergent/README.md).
#ifdef FREI_EMERGENT_TILE    // A/B builds (tools/build_variant.sh)
constexpr int kTile = FREI_EMERGENT_TILE;
#else
constexpr int kTile = 8;
#endif
#ifdef FREI_EMERGENT_AHEAD
constexpr int kAhead = FREI_EMERGENT_AHEAD;
#else
constexpr int kAhead = 4;
#endif
static_assert(kTile >= 1 && kTile <= 8 && kAhead >= 1, "tile of 1 .. 8 angles");
constexpr double kTwoPi = 6.283185307179586;

// exp_em, planck_em, shell_step (one exponential polynomial per shell and angle) and column_walk
// (the walk of one tile's rays up a column, shared with K16) are in frei_math.h with the
// primitives they are built on.

// The angles k0 .. k0 + TI - 1 of one column: the walk from level 1 to the top.  col: the
// column's row 0; it[l] = 1 / T_l for l = 1 .. nS + 1 (the virtual top level repeats the last).
// out: intensity[m][0] + j, or null; ck: null without the flux.
template <int TI>
__device__ __forceinline__ void emergent_pass(const double* __restrict__ col, int64_t n, int nS,
                                              double c1, double hcl,
                                              const double* __restrict__ it,
                                              const double* __restrict__ imu,
                                              const double* __restrict__ ck, int k0,
                                              double* __restrict__ out, double& F) {
  double w[TI], I[TI];
#pragma unroll
  for (int t = 0; t < TI; ++t) w[t] = imu[k0 + t];
  column_walk<TI, kAhead>(col, n, nS, c1, hcl, it, w, I);
#pragma unroll
  for (int t = 0; t < TI; ++t) {
    if (out) out[(int64_t)(k0 + t) * n] = I[t];
    if (ck) {
      const double term = ck[k0 + t] * I[t];
      F = (k0 + t == 0) ? term : F + term;        // ascending k, from the k = 0 term
    }
  }
}

__global__ __launch_bounds__(256) void emergent_kernel(
    const double* __restrict__ dtaus,   // [n_atm][nL][n]
    const double* __restrict__ c1,      // [n]
    const double* __restrict__ hcl,     // [n]
    const double* __restrict__ iT,      // [n_atm][nL + 1]: 1 / T_l, l = 1 .. nL
    const double* __restrict__ imu,     // [n_mu]: 1 / mu[k]
    const double* __restrict__ ck,      // [n_mu]: weights[k] mu[k], or null
    int n_mu, int nL, int64_t n,
    double* __restrict__ intensity,     // [n_atm][n_mu][n], or null
    double* __restrict__ flux) {        // [n_atm][n], or null
  const int m = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int nS = nL - 1;                              // shells 1 .. nS
  const double* __restrict__ col = dtaus + (int64_t)m * nL * n + j;
  const double* __restrict__ it = iT + (int64_t)m * (nL + 1);
  double* __restrict__ out = intensity ? intensity + (int64_t)m * n_mu * n + j : nullptr;
  const double a = c1[j], b = hcl[j];
  double F = 0.0;
  int k0 = 0;
  for (; k0 + kTile <= n_mu; k0 += kTile)
    emergent_pass<kTile>(col, n, nS, a, b, it, imu, ck, k0, out, F);
  switch (n_mu - k0) {                                // the partial tile, at its own width
    case 1: emergent_pass<1>(col, n, nS, a, b, it, imu, ck, k0, out, F); break;
    case 2: emergent_pass<2>(col, n, nS, a, b, it, imu, ck, k0, out, F); break;
    case 3: emergent_pass<3>(col, n, nS, a, b, it, imu, ck, k0, out, F); break;
    case 4: emergent_pass<4>(col, n, nS, a, b, it, imu, ck, k0, out, F); break;
    case 5: emergent_pass<5>(col, n, nS, a, b, it, imu, ck, k0, out, F); break;
    case 6: emergent_pass<6>(col, n, nS, a, b, it, imu, ck, k0, out, F); break;
    case 7: emergent_pass<7>(col, n, nS, a, b, it, imu, ck, k0, out, F); break;
    default: break;
  }
  if (flux) flux[(int64_t)m * n + j] = kTwoPi * F;
}

}  // namespace

void launch_emergent(const double* dtaus, const double* c1, const double* hcl, const double* iT,
                     const double* imu, const double* ck, int n_mu, int nL, int64_t n, int n_atm,
                     double* intensity, double* flux, hipStream_t st) {
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)n_atm);
  hipLaunchKernelGGL(emergent_kernel, grid, dim3(256), 0, st, dtaus, c1, hcl, iT, imu, ck, n_mu,
                     nL, n, intensity, flux);
}

}  // namespace frei
