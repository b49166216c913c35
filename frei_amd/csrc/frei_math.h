// frei_math.h — fp64 exp / sqrt / division / reciprocal for the sweep kernels, cheaper on
// gfx950's VALU than the ocml / LLVM lowering they replace, and the small formulas built on them
// (planck, exp_em, planck_em, shell_step).  What each function guarantees is checked against
// exact arithmetic on the GPU by tests/test_gpu_math.py (through tests/csrc/frei_math_probe.hip);
// the figures quoted here are that test's, measured on MI355X.
//
// Why: the sweep is fp64-VALU-bound, and three lowering choices cost ~25% of
// its instructions per flux update:
//   * ocml's exp Horner chain is emitted as `v_fmac_f64 acc(=c_k) += r * p`, so every
//     polynomial coefficient is first copied into a VGPR pair (two v_mov_b32 per term, ~18
//     VALU moves per call).  Here each term of the sweep's exp (exp_neg*) is one
//     `v_fma_f64 p, r, p, s[c_k]` with the coefficient in an SGPR pair (materialised by SALU
//     moves, off the VALU port).  Same constants, same fma order: bit-identical to the
//     compiler's ::exp for every x <= 0 (2^20 uniform points, every reduction boundary, the
//     subnormal-result window), within 0.80 ulp of exp(x).
//   * IEEE fp64 division is lowered with v_div_scale x2 / v_div_fmas / v_div_fixup around the
//     Newton-Raphson core.  Those only act when an operand is within ~2^768 of the exponent
//     range ends, denormal, zero, infinite or NaN; every quotient the sweep forms (optical
//     depths, Planck terms, albedos, 1/chi) is far from the range ends, so the bare core below
//     serves.  Of the special operands only a zero numerator is kept exact (+-0 / b has the IEEE
//     sign); a zero, infinite or NaN divisor gives NaN.
//   * sqrt's denormal-range scaling (x < 2^-767) is likewise dropped: the sweep takes square
//     roots of 1 - w0 style quantities in (2^-53, 2].
//   * division and sqrt refine the hardware estimate with one Newton-Raphson step fewer than
//     the LLVM / ocml sequences (gfx950's v_rcp_f64 and v_rsq_f64 are good to ~2^-24), after
//     which the quotient's residual correction (sqrt: the final Newton correction) still
//     rounds correctly on every operand that is not constructed to defeat it: 0 differences
//     from the correctly rounded result on 2^20 random operands per range and on the operand
//     families the kernels form ((B1 - B2) / dtau, Emw / E, pi (1 - w0) / Emw, c1 e / (1 - e),
//     power-of-two divisors).  The results are faithfully rounded, not always correctly
//     rounded: the shorter refinement leaves the reciprocal (and with it the correction term)
//     a few ulp off, so a result very close to a rounding midpoint can come out one ulp off.
//     On 25 000 constructed quotients within 2^-53 ulp of a midpoint, 2762 are the other
//     neighbour (e.g. 0x1.60cb52fd9f943p+52 / 0x1.ffca01812618bp+52 gives 0x1.60f08b52d22cbp-1,
//     correctly rounded 0x1.60f08b52d22ccp-1); on 326 constructed arguments whose root is within
//     2^-45 ulp of a midpoint, 5 are (e.g. sqrt(0x1.d539343604b1cp-1) gives
//     0x1.ea2531e60718fp-1, correctly rounded 0x1.ea2531e607190p-1); none is further off.
//     No bitwise identity between sweep forms depends on correct rounding: every form calls
//     the same div and sqrt.
//     -1.2 % sweep time at 500k, -3.9 % at 62.5k (profiles/r02_ab_short_div.txt).
// tools/mathcheck.hip is the stand-alone 2^28-operand version of the bitwise comparisons.
#pragma once
#include <hip/hip_runtime.h>

namespace frei {
namespace fm {

// d = a * b + c with c held in an SGPR pair (wave-uniform constant).
__device__ __forceinline__ double fma_sc(double a, double b, double c) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
  return d;
}

__device__ __forceinline__ double c64(unsigned long long bits) {
  return __builtin_bit_cast(double, bits);
}

// exp(x): ocml's own (the standalone two_stream form; the sweeps use exp_neg* below).  The
// SGPR-coefficient form of the whole-range exp pushed the one-lane sweep past the SGPR file (18
// spills), 2 % slower (profiles/r01_ab_fastmath.txt).
__device__ __forceinline__ double exp(double x) { return ::exp(x); }

// exp(x) for x <= 0 or NaN (a layer transmission exp(-2 sqrt(..) dtau)): ocml's sequence
// (round-to-nearest reduction by ln2 split in two, degree-11 Horner polynomial, two final fma
// with 1.0, ldexp) with the argument clamped at -1100 instead of its two range selects — below
// -1075 the final ldexp underflows to the same 0 ocml returns, so bit-identical for every
// x <= 0; NaN passes through.
// exp_neg's Horner terms as VOP3 fma with SGPR coefficients: otherwise the compiler keeps the
// coefficients in VGPRs and copies each into the accumulator of a two-address v_fmac (one
// extra move per term) — 174 vs 183 VALU instructions per flux update and -6 % sweep time
// at 500k despite a few SGPR spills (profiles/r02_ab_exp_sc.txt)
__device__ __forceinline__ double hfma(double r, double p, unsigned long long c) {
  return fma_sc(r, p, c64(c));
}
__device__ __forceinline__ double exp_neg(double x) {
  x = (x < -1100.0) ? -1100.0 : x;
  const double n = __builtin_rint(x * c64(0x3ff71547652b82feull));
  double r = __builtin_fma(c64(0xbfe62e42fefa39efull), n, x);
  r = __builtin_fma(c64(0xbc7abc9e3b39803full), n, r);
  double p = __builtin_fma(c64(0x3e5ade156a5dcb37ull), r, c64(0x3e928af3fca7ab0cull));
  p = hfma(r, p, 0x3ec71dee623fde64ull);
  p = hfma(r, p, 0x3efa01997c89e6b0ull);
  p = hfma(r, p, 0x3f2a01a014761f6eull);
  p = hfma(r, p, 0x3f56c16c1852b7b0ull);
  p = hfma(r, p, 0x3f81111111122322ull);
  p = hfma(r, p, 0x3fa55555555502a1ull);
  p = hfma(r, p, 0x3fc5555555555511ull);
  p = hfma(r, p, 0x3fe000000000000bull);
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
  return __builtin_ldexp(p, (int)n);
}

// exp_neg for an argument that cannot be NaN (the contracted-table sweeps: K3 is only built
// for NaN-free tables): the clamp is one v_max_f64 instead of a compare and two selects (maxNum
// would turn a NaN into -1100; here there is none).  Bit-identical to exp_neg otherwise.
__device__ __forceinline__ double exp_neg_nf(double x) {
  x = __builtin_fmax(x, -1100.0);
  const double n = __builtin_rint(x * c64(0x3ff71547652b82feull));
  double r = __builtin_fma(c64(0xbfe62e42fefa39efull), n, x);
  r = __builtin_fma(c64(0xbc7abc9e3b39803full), n, r);
  double p = __builtin_fma(c64(0x3e5ade156a5dcb37ull), r, c64(0x3e928af3fca7ab0cull));
  p = hfma(r, p, 0x3ec71dee623fde64ull);
  p = hfma(r, p, 0x3efa01997c89e6b0ull);
  p = hfma(r, p, 0x3f2a01a014761f6eull);
  p = hfma(r, p, 0x3f56c16c1852b7b0ull);
  p = hfma(r, p, 0x3f81111111122322ull);
  p = hfma(r, p, 0x3fa55555555502a1ull);
  p = hfma(r, p, 0x3fc5555555555511ull);
  p = hfma(r, p, 0x3fe000000000000bull);
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
  return __builtin_ldexp(p, (int)n);
}

// exp(x) for x <= 0 without the clamp (Planck factors, frei_kernels.hip planck_e): exp_neg's
// sequence, so bit-identical to it for x in [-1100, 0]; below, n stays an int32 and the final
// ldexp still underflows to 0.  NaN propagates; x = -inf gives NaN (a zero temperature).
__device__ __forceinline__ double exp_neg_unclamped(double x) {
  const double n = __builtin_rint(x * c64(0x3ff71547652b82feull));
  double r = __builtin_fma(c64(0xbfe62e42fefa39efull), n, x);
  r = __builtin_fma(c64(0xbc7abc9e3b39803full), n, r);
  double p = __builtin_fma(c64(0x3e5ade156a5dcb37ull), r, c64(0x3e928af3fca7ab0cull));
  p = hfma(r, p, 0x3ec71dee623fde64ull);
  p = hfma(r, p, 0x3efa01997c89e6b0ull);
  p = hfma(r, p, 0x3f2a01a014761f6eull);
  p = hfma(r, p, 0x3f56c16c1852b7b0ull);
  p = hfma(r, p, 0x3f81111111122322ull);
  p = hfma(r, p, 0x3fa55555555502a1ull);
  p = hfma(r, p, 0x3fc5555555555511ull);
  p = hfma(r, p, 0x3fe000000000000bull);
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
  return __builtin_ldexp(p, (int)n);
}

// 1 / b within one ulp: the reciprocal part of the division core below (rcp and two
// Newton-Raphson steps) without the quotient's final residual correction.  Used where the
// result only scales a sum (1 / chi of the flux update), so an ulp is not amplified.
// (One Newton step: within 11 ulp, two VALU fewer per update, 0..1.5 % sweep time —
// noise-level, profiles/r03/ab_rcp_steps.txt — but batched-vs-single temperatures then differ by
// 2e-11 after 3 iterations: not adopted.)
__device__ __forceinline__ double rcp_nr(double b) {
  double r = __builtin_amdgcn_rcp(b);
  double e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-b, r, 1.0);
  return __builtin_fma(r, e, r);
}

// a / b: LLVM's fp64 division core (rcp, one Newton-Raphson step where LLVM takes two,
// quotient, one residual correction) without the div_scale / div_fmas / div_fixup guards; the
// sign of the quotient estimate is copied onto the result (one v_bfi_b32: a zero numerator of
// either sign gives the IEEE zero; no change for any other operand; no measurable cost at 500k).
__device__ __forceinline__ double div(double a, double b) {
  double r = __builtin_amdgcn_rcp(b);
  const double e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  const double q = a * r;
  const double rem = __builtin_fma(-b, q, a);
  // q has the quotient's sign; for a = -0 and b > 0 the sum below is (+0) + (-0) = +0
  return __builtin_copysign(__builtin_fma(rem, r, q), q);
}

// sqrt(x): ocml's rsq + Newton-Raphson sequence (its last correction dropped) without the
// x < 2^-767 rescaling; +-0 and +inf pass through as in ocml.
__device__ __forceinline__ double sqrt(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y;
  double h = y * 0.5;
  const double e = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, e, g);
  h = __builtin_fma(h, e, h);
  double d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  return __builtin_amdgcn_class(x, 0x260) ? x : g;   // +-0, +inf
}

// sqrt(x) for the sweep's square roots — E (E - w0), (E - w0) / E and 1 - w0 with
// w0 = sigma / (2 sigma + sum of table terms) <= 1/2 and E in [1, 1.21], i.e. x in (1/2, 1.21]
// for non-negative opacities: sqrt's sequence without the +-0 / +inf pass-through (three
// instructions), which only differs at exactly those inputs; NaN propagates as before.
__device__ __forceinline__ double sqrt_pos(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y;
  double h = y * 0.5;
  const double e = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, e, g);
  h = __builtin_fma(h, e, h);
  double d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  return g;
}

}  // namespace fm

// ---------------------------------------------------------------- formulas on the primitives
// The sweeps' Planck function (frei_kernels.hip) and the emergent rays' exponential forms
// (frei_emergent.hip) live here so that tests/csrc/frei_math_probe.hip can call them one value at
// a time; the kernels' code is unchanged by where they are declared.

// twostream.py:64-67: 2hc^2/lam^5 / expm1(hc / (lam k T)).  The exponent is formed as
// (hc / (lam k)) * (1 / T) — a per-wavelength constant (host) times a per-layer one (the step
// record) — instead of one division per update: within 1.5 ulp of the reference's
// hc / ((lam k) T), which moves spectra and T by < 1e-13.
//
// The value is formed as c1 e / (1 - e) with e = exp(-x), from the transmission's exp (its
// coefficients are wave-uniform SGPR constants the sweep already holds) instead of an expm1
// whose ten coefficients occupied 20 VGPRs per lane: four VALU and 20 VGPRs fewer per update,
// no range guard (e in [0, 1]: the quotient never overflows, and e underflows to the
// reference's 0 at x > 745).  Error: a few ulp, growing as ~1 ulp / x for x < 1 (the
// cancellation in 1 - e) — 1e-15 relative at x = 0.1, far inside the 1e-10 parity bar.  A NaN
// temperature propagates.  Between x = 709.8 (where numpy's expm1 overflows, B = 0) and 745 it
// returns the subnormal c1 e instead of 0.
__device__ __forceinline__ double planck(double c1, double hcl, double iT) {
  const double e = fm::exp_neg_unclamped(-(hcl * iT));
  return fm::div(c1 * e, 1.0 - e);
}

// For y <= 0 (or NaN): e = exp(y), em = 1 - e = -expm1(y), and the short-range quantities
//   n0 = (the reduction took no power of two: |y| <= ln2 / 2), q = (e - 1 - y) / y^2 for n0,
// from fm::exp_neg's sequence (same constants, same fma order: e is bit-identical to it).  With
// n0 the reduced argument is y itself and the polynomial is 1 + y (1 + y q), so
//   em = -y (1 + y q) and (e - 1 - y) / y = y q
// come without cancellation; otherwise e <= 2^-1/2 and 1 - e loses less than two bits.  e is
// never formed as 1 - em.  y below -1100 (and -inf) is clamped: e underflows to 0 smoothly.
__device__ __forceinline__ void exp_em(double y, double& e, double& em, bool& n0, double& q) {
  y = (y < -1100.0) ? -1100.0 : y;
  const double n = __builtin_rint(y * fm::c64(0x3ff71547652b82feull));
  double r = __builtin_fma(fm::c64(0xbfe62e42fefa39efull), n, y);
  r = __builtin_fma(fm::c64(0xbc7abc9e3b39803full), n, r);
  double p = __builtin_fma(fm::c64(0x3e5ade156a5dcb37ull), r, fm::c64(0x3e928af3fca7ab0cull));
  p = fm::hfma(r, p, 0x3ec71dee623fde64ull);
  p = fm::hfma(r, p, 0x3efa01997c89e6b0ull);
  p = fm::hfma(r, p, 0x3f2a01a014761f6eull);
  p = fm::hfma(r, p, 0x3f56c16c1852b7b0ull);
  p = fm::hfma(r, p, 0x3f81111111122322ull);
  p = fm::hfma(r, p, 0x3fa55555555502a1ull);
  p = fm::hfma(r, p, 0x3fc5555555555511ull);
  q = fm::hfma(r, p, 0x3fe000000000000bull);
  const double p1 = __builtin_fma(r, q, 1.0);
  e = __builtin_ldexp(__builtin_fma(r, p1, 1.0), (int)n);
  n0 = n == 0.0;
  em = n0 ? -(r * p1) : 1.0 - e;
}

// B = c1 / expm1(hcl / T) as c1 e / (1 - e) with e = exp(-hcl / T) (the sweeps' planck above),
// the denominator from exp_em: no cancellation at long wavelengths.
__device__ __forceinline__ double planck_em(double c1, double hcl, double iT) {
  double e, em, q;
  bool n0;
  exp_em(-(hcl * iT), e, em, n0, q);
  return fm::div(c1 * e, em);
}

// One shell along one ray: I = I e + (Bl u + Bn v), x = dtau / mu.
//   v = 1 - em / x, by x q where the polynomial's q is that quotient's series (x <= ln2 / 2: no
//   cancellation, v(0) = 0), by the division above it (x >= 2^60, inf included: v = 1 exactly,
//   as the rounded 1 - em / x is); u = em - v.  e, u, v >= 0 and e + u + v = 1.
__device__ __forceinline__ void shell_step(double& I, double x, double Bl, double Bn) {
  double e, em, q;
  bool n0;
  exp_em(-x, e, em, n0, q);
  const double xd = __builtin_fmin(x, 0x1p60);
  const double v = n0 ? x * q : 1.0 - fm::div(em, xd);
  const double u = em - v;
  I = I * e + (Bl * u + Bn * v);
}

// TI rays through one column, from the opaque base at level 1 to the top: the walk K11
// (frei_emergent.hip) and K16 (frei_phase.hip) share, so that a ray's intensity is the same bits
// in both.  col: the column's row 0 (rows n apart); it[l] = 1 / T_l for l = 1 .. nS + 1 (the
// virtual top level repeats the last); w[t] = 1 / mu of ray t; I[t] receives its intensity.  Each
// dtaus[l] is loaded once, AHEAD shells ahead of its use (rows past the last shell are clamped to
// it: loaded, never used), and B_{l+1} is formed once per shell for every ray and becomes the next
// shell's B_l.
template <int TI, int AHEAD>
__device__ __forceinline__ void column_walk(const double* __restrict__ col, int64_t n, int nS,
                                            double c1, double hcl,
                                            const double* __restrict__ it, const double (&w)[TI],
                                            double (&I)[TI]) {
  double Bl = planck_em(c1, hcl, it[1]);
#pragma unroll
  for (int t = 0; t < TI; ++t) I[t] = Bl;
  double d[AHEAD];
#pragma unroll
  for (int u = 0; u < AHEAD; ++u) d[u] = col[(int64_t)min(1 + u, nS) * n];
  for (int l0 = 1; l0 <= nS; l0 += AHEAD) {
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int l = l0 + u;
      if (l <= nS) {
        const double dt = d[u];
        d[u] = col[(int64_t)min(l + AHEAD, nS) * n];
        const double Bn = planck_em(c1, hcl, it[l + 1]);
#pragma unroll
        for (int t = 0; t < TI; ++t) shell_step(I[t], dt * w[t], Bl, Bn);
        Bl = Bn;
      }
    }
  }
}

}  // namespace frei
