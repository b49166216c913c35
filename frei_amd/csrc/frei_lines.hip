// frei_lines.hip — K17: a species' cross-section computed line by line from a line list into a
// resident frei_xsec (frei_xsec_create_lines; the definition is in include/frei_hip.h), and
// frei_xsec_values, the read-back of a resident cross-section's rows.  No reference counterpart:
// the reference downloads this table (opacity.py:345-372, 493-540).
//
// Host (C++, this file): argument checks, nu_i = 1e4 / wl_hi[i], the pre-pass (per (T node,
// line): A = S / (alpha sqrt(pi)), 1 / alpha, gT / alpha — n_T n_line values, microseconds beside
// the main kernel) and the plan (per block of 256 axis points the range of lines within the cutoff
// of the block's wavenumber span, by binary search with the kernel's own comparison).
// Device: one lane per axis point, grid (256-point blocks, T nodes, tiles of pressure nodes).  A
// lane walks its block's lines in ascending index, forms |nu_i - nu0| and x once per line for its
// tile of pressure nodes, and adds A K(x, y) into one fp64 accumulator per node; one float32 store
// per (node, point).  The line parameters are wave-uniform: staged in LDS chunks of 256 lines that
// every lane reads at one address (a broadcast), one pressure node per lane.  Scalar loads and
// tiles of 2 and 4 nodes were measured against it and are kept behind FREI_LINES_FORM for the
// probe (tools/lines_probe.py): 1.8 % and 8 to 14 % slower (profiles/r17/lines).
//
// K(x, y) = Re w(x + iy), relative error <= 2^-26 on x in [0, 1e6], y in [1e-8, 1e5] (measured
// worst 2.2e-11 against scipy.special.wofz, tests/test_lines_host.py), all fp64:
//   |z| >= 8             Laplace's continued fraction, 12 levels from the bottom up, carried as a
//                        ratio P / Q of s = r / z so that it costs two divisions (voigt_far);
//   |z| < 8, y >= 1e-3   Weideman's N = 40 rational form (SIAM J. Numer. Anal. 31, 1994), its 40
//                        real coefficients computed once on the host (rational);
//   |z| < 8, y < 1e-3    Re w(x) = exp(-x^2) and Im w(x) from the same rational form on the real
//                        axis, then a third-order Taylor step in y through w' = -2 z w + 2i/sqrt(pi).
// -ffp-contract=off: an fma below is written, never inferred, so every instantiation of the
// kernel (tile width, staging form) adds the same bits (tests/test_gpu_lines.py).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

namespace {

constexpr int kNRat = 40;                       // Weideman's N
constexpr double kLRat = 5.318295896944989;     // sqrt(N / sqrt(2))
constexpr int kCfLevels = 12;
constexpr double kZFar2 = 64.0;                 // |z|^2 >= 64: continued fraction
constexpr double kYSmall = 1e-3;
constexpr double kInvSqrtPi = 0.5641895835477563;
constexpr double kAmu = 1.6605390666e-24;       // g (frei_amd/constants.py AMU)
constexpr int kChunk = 256;                     // lines per LDS chunk (the staged form)

struct VoigtCoef {
  double c[kNRat];   // p(Z) = sum_n c[n] Z^n
};

// w(x + iy) by the rational form: Z = (L + iz) / (L - iz),
// w = 2 p(Z) / (L - iz)^2 + (1 / sqrt(pi)) / (L - iz).
__device__ __forceinline__ void rational(double x, double y, const VoigtCoef& cf, double& wr,
                                         double& wi) {
  const double a = kLRat - y, b = kLRat + y;
  const double xx = x * x;
  const double inv = 1.0 / __builtin_fma(b, b, xx);
  const double Zr = __builtin_fma(a, b, -xx) * inv;
  const double Zi = ((2.0 * kLRat) * x) * inv;
  double pr = cf.c[kNRat - 1], pi = 0.0;
#pragma unroll
  for (int n = kNRat - 2; n >= 0; --n) {
    const double tr = __builtin_fma(-pi, Zi, __builtin_fma(pr, Zr, cf.c[n]));
    pi = __builtin_fma(pr, Zi, pi * Zr);
    pr = tr;
  }
  const double ur = b * inv, ui = x * inv;
  const double vr = __builtin_fma(ur, ur, -(ui * ui));
  const double vi = (2.0 * ur) * ui;
  wr = __builtin_fma(2.0, __builtin_fma(pr, vr, -(pi * vi)), kInvSqrtPi * ur);
  wi = __builtin_fma(2.0, __builtin_fma(pr, vi, pi * vr), kInvSqrtPi * ui);
}

// Re w by the continued fraction w = (i / sqrt(pi)) / (z - (1/2) / (z - 1 / (z - (3/2) / ...))):
// with s = r / z and q = 1 / z^2 a level is s <- 1 - (k / 2) q / s; s = P / Q gives
// (P, Q) <- (P - (k / 2) q Q, P) and w = (i / sqrt(pi)) Q / (z P).  Every quantity is O(1) for any
// |z| >= 8, and the imaginary parts (which carry Re w when y << x) never meet a real part.
__device__ __forceinline__ double voigt_far(double x, double y) {
  const double z2r = __builtin_fma(x, x, -(y * y));
  const double z2i = (2.0 * x) * y;
  const double m = 1.0 / __builtin_fma(z2r, z2r, z2i * z2i);
  const double qr = z2r * m, qi = -(z2i * m);
  double Pr = 1.0, Pi = 0.0, Qr = 1.0, Qi = 0.0;
#pragma unroll
  for (int k = kCfLevels; k >= 1; --k) {
    const double c = 0.5 * k;
    const double tr = __builtin_fma(qr, Qr, -(qi * Qi));
    const double ti = __builtin_fma(qr, Qi, qi * Qr);
    Qr = Pr;
    Qi = Pi;
    Pr = __builtin_fma(-c, tr, Pr);
    Pi = __builtin_fma(-c, ti, Pi);
  }
  const double Dr = __builtin_fma(x, Pr, -(y * Pi));
  const double Di = __builtin_fma(x, Pi, y * Pr);
  return kInvSqrtPi * (__builtin_fma(Qr, Di, -(Qi * Dr)) / __builtin_fma(Dr, Dr, Di * Di));
}

// K(x, y) for x >= 0, y > 0.
__device__ __forceinline__ double voigt(double x, double y, const VoigtCoef& cf) {
  if (__builtin_fma(x, x, y * y) >= kZFar2) return voigt_far(x, y);
  const bool small = y < kYSmall;
  double wr, wi;
  rational(x, small ? 0.0 : y, cf, wr, wi);
  if (!small) return wr;
  const double w0r = ::exp(-(x * x));
  const double x2 = 2.0 * x;
  const double w1r = -(x2 * w0r);
  const double w1i = __builtin_fma(-x2, wi, 2.0 * kInvSqrtPi);
  const double w2r = __builtin_fma(-x2, w1r, -(2.0 * w0r));
  const double w2i = __builtin_fma(-x2, w1i, -(2.0 * wi));
  const double w3i = __builtin_fma(-x2, w2i, -(4.0 * w1i));
  const double y2 = y * y;
  return __builtin_fma((y2 * y) * (1.0 / 6.0), w3i,
                       __builtin_fma(-(0.5 * y2), w2r, __builtin_fma(-y, w1i, w0r)));
}

// One line's share of a lane's TP accumulators (ascending line index: the caller's loop).
template <int TP>
__device__ __forceinline__ void add_line(double nui, double n0, double a, double ial, double gal,
                                         const double (&pv)[TP], double cutoff,
                                         const VoigtCoef& cf, double (&acc)[TP]) {
  const double dnu = __builtin_fabs(nui - n0);
  if (dnu <= cutoff) {   // the definition's comparison
    const double x = dnu * ial;
#pragma unroll
    for (int k = 0; k < TP; ++k) acc[k] = acc[k] + a * voigt(x, gal * pv[k], cf);
  }
}

// grid (256-point blocks, T nodes, pressure tiles of TP nodes starting at node p0).  A, ia, ga:
// [n_T][n_line]; blk_lo / blk_hi: the block's line range; out[n_T][n_p][n_hi].
template <int TP, bool STAGED>
__global__ __launch_bounds__(256) void lines_kernel(
    const double* __restrict__ nu, int64_t n_hi, const double* __restrict__ nu0,
    const double* __restrict__ A, const double* __restrict__ ia, const double* __restrict__ ga,
    int64_t n_line, const int64_t* __restrict__ blk_lo, const int64_t* __restrict__ blk_hi,
    const double* __restrict__ p, int n_p, int p0, double cutoff, double inv_m, VoigtCoef cf,
    float* __restrict__ out) {
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool act = i < n_hi;
  const double nui = nu[act ? i : n_hi - 1];
  const int t = blockIdx.y;
  const int pk = p0 + (int)blockIdx.z * TP;
  const int64_t lo = blk_lo[blockIdx.x], hi = blk_hi[blockIdx.x];   // block-uniform
  const double* __restrict__ At = A + (int64_t)t * n_line;
  const double* __restrict__ iat = ia + (int64_t)t * n_line;
  const double* __restrict__ gat = ga + (int64_t)t * n_line;
  double pv[TP], acc[TP];
#pragma unroll
  for (int k = 0; k < TP; ++k) {
    pv[k] = p[pk + k];
    acc[k] = 0.0;
  }
  if (STAGED) {
    __shared__ double sh[4][kChunk];
    for (int64_t c = lo; c < hi; c += kChunk) {
      const int nc = (int)min((int64_t)kChunk, hi - c);
      if (tid < nc) {
        sh[0][tid] = nu0[c + tid];
        sh[1][tid] = At[c + tid];
        sh[2][tid] = iat[c + tid];
        sh[3][tid] = gat[c + tid];
      }
      __syncthreads();
      for (int j = 0; j < nc; ++j)   // one address for all lanes: a broadcast read
        add_line<TP>(nui, sh[0][j], sh[1][j], sh[2][j], sh[3][j], pv, cutoff, cf, acc);
      __syncthreads();   // the next chunk overwrites these
    }
  } else {
    for (int64_t l = lo; l < hi; ++l)   // uniform index: scalar loads
      add_line<TP>(nui, nu0[l], At[l], iat[l], gat[l], pv, cutoff, cf, acc);
  }
  if (act) {
#pragma unroll
    for (int k = 0; k < TP; ++k)
      out[((int64_t)t * n_p + pk + k) * n_hi + i] = (float)(inv_m * acc[k]);
  }
}

template <int TP, bool STAGED>
void launch_tiles(dim3 grid, hipStream_t st, const double* nu, int64_t n_hi, const double* nu0,
                  const double* A, const double* ia, const double* ga, int64_t n_line,
                  const int64_t* lo, const int64_t* hi, const double* p, int n_p, int p0,
                  double cutoff, double inv_m, const VoigtCoef& cf, float* out) {
  lines_kernel<TP, STAGED><<<grid, 256, 0, st>>>(nu, n_hi, nu0, A, ia, ga, n_line, lo, hi, p, n_p,
                                                 p0, cutoff, inv_m, cf, out);
}

// The 40 coefficients: the cosine series of f(t) = exp(-t^2) (L^2 + t^2) on t = L tan(theta / 2),
// theta = k pi / M, M = 2 N (Weideman's FFT written out: c[n-1] = (f(0) + 2 sum_k f_k cos(pi n k /
// M)) / (2 M), summed in ascending k).
VoigtCoef weideman_coefficients() {
  constexpr int M = 2 * kNRat;
  double f[M];
  for (int k = 1; k < M; ++k) {
    const double t = kLRat * std::tan(k * kPi / (2 * M));
    f[k] = std::exp(-t * t) * (kLRat * kLRat + t * t);
  }
  VoigtCoef cf;
  for (int n = 1; n <= kNRat; ++n) {
    double s = 0.0;
    for (int k = 1; k < M; ++k) s = s + f[k] * std::cos(kPi * n * k / M);
    cf.c[n - 1] = (kLRat * kLRat + 2.0 * s) / (2 * M);
  }
  return cf;
}

const char* kWhat = "frei_xsec_create_lines: ";

int bad(const char* name, int64_t i, double v, const char* why) {
  char buf[64];
  snprintf(buf, sizeof buf, "%.17g", v);
  return set_error(std::string(kWhat) + name + "[" + std::to_string(i) + "] = " + buf + " " + why);
}

// The first element of a[n] that is not finite or fails `ok`.
template <typename F>
int check_each(const char* name, const double* a, int64_t n, const char* why, F ok) {
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(a[i])) return bad(name, i, a[i], "is not finite");
    if (!ok(a[i])) return bad(name, i, a[i], why);
  }
  return 0;
}

// FREI_LINES_FORM: "l" (LDS-staged chunks) or "s" (scalar loads), then the pressure-tile width
// 1, 2 or 4; default "l1", the fastest measured.  Every form adds the same bits.
int lines_form(bool* staged, int* tile) {
  const char* e = getenv("FREI_LINES_FORM");
  const std::string f = e && *e ? e : "l1";
  if (f.size() != 2 || (f[0] != 's' && f[0] != 'l') || (f[1] != '1' && f[1] != '2' && f[1] != '4'))
    return set_error(std::string(kWhat) + "FREI_LINES_FORM = '" + f +
                     "' is not s1, s2, s4, l1, l2 or l4");
  *staged = f[0] == 'l';
  *tile = f[1] - '0';
  return 0;
}

}  // namespace

namespace frei {
// The plan of K17: for every block of 256 consecutive axis points (nu descending, as wl_hi
// ascends) the lines [lo, hi) that can lie within `cutoff` of one of its points.  The two
// predicates are the kernel's comparison at the block's ends, and rounded subtraction is
// monotone, so a line outside the range fails the comparison at every point of the block.
void lines_plan(const double* nu, int64_t n_hi, const double* nu0, int64_t n_line, double cutoff,
                std::vector<int64_t>* lo, std::vector<int64_t>* hi) {
  const int64_t nblk = (n_hi + 255) / 256;
  lo->resize(nblk);
  hi->resize(nblk);
  for (int64_t b = 0; b < nblk; ++b) {
    const double nu_max = nu[b * 256], nu_min = nu[std::min(n_hi, b * 256 + 256) - 1];
    const int64_t a = std::partition_point(nu0, nu0 + n_line, [&](double v) {
                        return nu_min - v > cutoff; }) - nu0;
    const int64_t e = std::partition_point(nu0, nu0 + n_line, [&](double v) {
                        return !(v - nu_max > cutoff); }) - nu0;
    (*lo)[b] = a;
    (*hi)[b] = std::max(a, e);
  }
}
}  // namespace frei

// ==================================================================== C ABI
extern "C" {

int frei_xsec_create_lines(frei_xsec** out, int device, int64_t n_line, const double* nu0,
                           const double* S_ref, const double* E_low, const double* gamma_ref,
                           const double* n_exp, double mass_amu, double T_ref, double cutoff,
                           const double* q_ratio, int n_T, int n_p, int64_t n_hi,
                           const double* T_nodes, const double* p_nodes, const double* wl_hi,
                           double* kernel_ms) {
  // ---- every argument error, before any device call
  if (!out) return set_error(std::string(kWhat) + "null argument");
  *out = nullptr;
  if (!nu0 || !S_ref || !E_low || !gamma_ref || !n_exp || !q_ratio || !T_nodes || !p_nodes ||
      !wl_hi)
    return set_error(std::string(kWhat) + "null argument");
  if (n_line < 1) return set_error(std::string(kWhat) + "n_line < 1");
  if (n_T < 1 || n_p < 1 || n_hi < 2) return set_error(std::string(kWhat) + "empty cross-section grid");
  if (n_T > 65535) return set_error(std::string(kWhat) + "more than 65535 temperature nodes");
  if (!std::isfinite(mass_amu) || !(mass_amu > 0))
    return set_error(std::string(kWhat) + "mass_amu must be finite and > 0");
  if (!std::isfinite(T_ref) || !(T_ref > 0))
    return set_error(std::string(kWhat) + "T_ref must be finite and > 0");
  if (!std::isfinite(cutoff) || !(cutoff > 0))
    return set_error(std::string(kWhat) + "cutoff must be finite and > 0");
  TRY(check_each("nu0", nu0, n_line, "must be > 0", [](double v) { return v > 0; }));
  for (int64_t l = 1; l < n_line; ++l)
    if (nu0[l] < nu0[l - 1]) return bad("nu0", l, nu0[l], "is below its predecessor (line positions must be nondecreasing)");
  TRY(check_each("S_ref", S_ref, n_line, "must be >= 0", [](double v) { return v >= 0; }));
  TRY(check_each("E_low", E_low, n_line, "", [](double) { return true; }));
  TRY(check_each("gamma_ref", gamma_ref, n_line, "must be > 0", [](double v) { return v > 0; }));
  TRY(check_each("n_exp", n_exp, n_line, "", [](double) { return true; }));
  TRY(check_each("q_ratio", q_ratio, n_T, "must be > 0", [](double v) { return v > 0; }));
  TRY(check_each("T_nodes", T_nodes, n_T, "must be > 0", [](double v) { return v > 0; }));
  TRY(check_each("p_nodes", p_nodes, n_p, "must be > 0", [](double v) { return v > 0; }));
  TRY(check_each("wl_hi", wl_hi, n_hi, "must be > 0", [](double v) { return v > 0; }));
  for (int64_t i = 1; i < n_hi; ++i)
    if (!(wl_hi[i] > wl_hi[i - 1])) return bad("wl_hi", i, wl_hi[i], "is not above its predecessor (the axis must be strictly ascending)");
  bool staged = true;
  int tile = 1;
  TRY(lines_form(&staged, &tile));

  // ---- host: wavenumbers, pre-pass, plan
  std::vector<double> nu(n_hi);
  for (int64_t i = 0; i < n_hi; ++i) nu[i] = 1e4 / wl_hi[i];
  const double c2 = kH * kC / kKB, m = mass_amu * kAmu;
  const size_t nTL = (size_t)n_T * n_line;
  std::vector<double> A(nTL), ia(nTL), ga(nTL);
  for (int t = 0; t < n_T; ++t) {
    const double T = T_nodes[t];
    const double lnr = std::log(T_ref / T);
    const double dinv = 1.0 / T - 1.0 / T_ref;
    const double vth = std::sqrt(((2.0 * kKB) * T) / m);
    for (int64_t l = 0; l < n_line; ++l) {
      const double boltz = std::exp(-(c2 * E_low[l]) * dinv);
      const double stim = std::expm1(-(c2 * nu0[l]) / T) / std::expm1(-(c2 * nu0[l]) / T_ref);
      const double S = ((S_ref[l] * q_ratio[t]) * boltz) * stim;
      const double alpha = nu0[l] * vth / kC;
      const double gT = gamma_ref[l] * std::exp(n_exp[l] * lnr);
      const size_t k = (size_t)t * n_line + l;
      A[k] = S / (alpha * std::sqrt(kPi));
      ia[k] = 1.0 / alpha;
      ga[k] = gT / alpha;
    }
  }
  std::vector<int64_t> lo, hi;
  lines_plan(nu.data(), n_hi, nu0, n_line, cutoff, &lo, &hi);
  static const VoigtCoef cf = weideman_coefficients();

  // ---- device
  frei_xsec* x = new frei_xsec();
  x->device = device;
  x->nT = n_T;
  x->np = n_p;
  x->nhi = n_hi;
  x->T.assign(T_nodes, T_nodes + n_T);
  x->p.assign(p_nodes, p_nodes + n_p);
  x->wl.assign(wl_hi, wl_hi + n_hi);
  if (hipSetDevice(device) != hipSuccess || x->stream.create() ||
      x->d_x.alloc((size_t)n_T * n_p * n_hi)) {
    (void)hipGetLastError();
    delete x;
    return set_error(std::string(kWhat) + "device allocation failed");
  }
  int rc = 0;
  {
    DeviceCall call(x->stream, "line cross-section");
    const double* d_nu = call.upload(nu.data(), nu.size());
    const double* d_nu0 = call.upload(nu0, (size_t)n_line);
    const double* d_A = call.upload(A.data(), nTL);
    const double* d_ia = call.upload(ia.data(), nTL);
    const double* d_ga = call.upload(ga.data(), nTL);
    const double* d_p = call.upload(p_nodes, (size_t)n_p);
    const int64_t* d_lo = call.upload(lo.data(), lo.size());
    const int64_t* d_hi = call.upload(hi.data(), hi.size());
    const double inv_m = 1.0 / m;
    call.begin(kernel_ms);
    if (call.ok()) {
      // whole tiles of `tile` nodes, then the rest at its own width
      const int full = n_p / tile, rest = n_p % tile;
      auto go = [&](int width, int tiles, int p0) {
        const dim3 grid((unsigned)lo.size(), (unsigned)n_T, (unsigned)tiles);
#define FREI_LINES_GO(W, S)                                                                  \
  launch_tiles<W, S>(grid, x->stream, d_nu, n_hi, d_nu0, d_A, d_ia, d_ga, n_line, d_lo, d_hi, \
                     d_p, n_p, p0, cutoff, inv_m, cf, x->d_x)
        if (staged) {
          if (width == 4) FREI_LINES_GO(4, true);
          else if (width == 3) FREI_LINES_GO(3, true);
          else if (width == 2) FREI_LINES_GO(2, true);
          else FREI_LINES_GO(1, true);
        } else {
          if (width == 4) FREI_LINES_GO(4, false);
          else if (width == 3) FREI_LINES_GO(3, false);
          else if (width == 2) FREI_LINES_GO(2, false);
          else FREI_LINES_GO(1, false);
        }
#undef FREI_LINES_GO
      };
      for (int z0 = 0; z0 < full; z0 += 65535)   // grid z is 16 bits wide
        go(tile, std::min(65535, full - z0), z0 * tile);
      if (rest) go(rest, 1, full * tile);
    }
    call.end();
    rc = call.finish();
  }
  if (rc) {
    delete x;
    return rc;
  }
  *out = x;
  return 0;
}

int frei_xsec_values(frei_xsec* x, int t, int p, int64_t lo, int64_t n, float* out) {
  if (!x || !out) return set_error("frei_xsec_values: null argument");
  if (t < 0 || t >= x->nT || p < 0 || p >= x->np)
    return set_error("frei_xsec_values: node (" + std::to_string(t) + ", " + std::to_string(p) +
                     ") lies outside the " + std::to_string(x->nT) + " x " +
                     std::to_string(x->np) + " nodes");
  if (lo < 0 || n < 0 || lo > x->nhi || n > x->nhi - lo)
    return set_error("frei_xsec_values: points [" + std::to_string(lo) + ", " +
                     std::to_string(lo) + " + " + std::to_string(n) + ") lie outside the " +
                     std::to_string(x->nhi) + " of the axis");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->stream));
  HIP_TRY(hipMemcpy(out, x->d_x + ((int64_t)t * x->np + p) * x->nhi + lo, (size_t)n * sizeof(float),
                    hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
