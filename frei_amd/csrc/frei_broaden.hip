// frei_broaden.hip — K13: rotational and instrumental broadening of batched spectra.  A
// native-resolution spectrum x[n_atm][n_lam] is convolved with a kernel tabulated in velocity:
// out[m][i] = (sum_j w_ij x[m][j]) / norm[i], w_ij formed in registers from the resident vectors
// u = c ln(lam), tw (trapezoid weights in u) and the kernel table.  The reference has no
// counterpart; the definition is the header comment of frei_brd_apply in include/frei_hip.h.
//
// Data: u, tw, first, count, norm and the table stay resident in HBM with the handle; norm is
// formed on the host at creation with the very weight function the kernels use (brd_weight, not
// contracted).  Per call one of two kernels writes out[n_atm][n_lam]:
//   form 1 (brd_valu_kernel): one lane per output point, a register tile of 1, 4 or 8
//     atmospheres per lane (the weight is formed once per tap and used for all of them); taps in
//     ascending j, one fma per tap and atmosphere; consecutive lanes read consecutive j.
//   form 2 (brd_mfma_kernel): one wave per tile of 16 outputs x 16 atmospheres on
//     v_mfma_f64_16x16x4_f64.  The tile's span of x (and of u, tw) goes through LDS in chunks of
//     64 points, read from HBM in rows of 64 consecutive doubles a chunk ahead; each lane forms
//     its own weight straight into the A operand, 0 outside its output's window.
// Every (atmosphere, output) has its own accumulator and its order of summation depends on the
// handle alone: no atomics, results bitwise the same from call to call and for a row alone.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

struct frei_brd {
  Stream stream;   // first: destroyed last
  int device = 0;
  int64_t n_lam = 0;
  int n_tab = 0;
  double h = 0.0, inv_dv = 0.0;
  DevBuf<double> d_u, d_tw, d_norm, d_tab;
  DevBuf<int32_t> d_first, d_count;
  double mean_points = 0.0;   // per window: form 0 picks by it and by n_atm
  DevBuf<double> d_keep;      // [keep_atm][n_lam]: the last apply's result when it asked to keep
  int keep_atm = 0;
  ~frei_brd() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

namespace {

constexpr int kChunkJ = 64;  // form 2: points of x staged per turn (16 MFMA steps)
// form 0: form 2 from kMfmaFromAtmospheres atmospheres where a window holds kMfmaFromPoints points
// or more on average, and from 2 atmospheres where it holds kMfmaWidePoints or more; form 1
// otherwise.  Measured on MI355X (tools/broaden_probe.py, 500k points, the forms taking turns over
// 5 rounds; profiles/r12/broaden/README.md), VALU against MFMA form, median ms at 1 / 4 / 8 / 16 /
// 64 atmospheres: windows of 9 points 0.018 / 0.061, 0.029 / 0.066, 0.044 / 0.074, 0.081 / 0.090,
// 0.281 / 0.340; of 33 points 0.042 / 0.079, 0.070 / 0.085, 0.104 / 0.093, 0.204 / 0.109, 0.760 /
// 0.419; of 129 points 0.135 / 0.177, 0.229 / 0.183, 0.353 / 0.197, 0.709 / 0.218, 2.712 / 0.833;
// of 513 points 0.490 / 0.485, 0.837 / 0.492, 1.344 / 0.562, 2.736 / 0.611, 10.237 / 2.430
// (run-to-run spread below 4 %).  The VALU form steps up with every 8 atmospheres (one tile of 4
// for 2 to 4), the MFMA form with every 16.  At 9 points the VALU form wins at every count; from
// 33 points the MFMA form wins from 8 atmospheres on; from 129 points it wins at 4 too, and a
// single atmosphere is a tie or the VALU form's.  Not timed: 2, 3 and 5 to 7 atmospheres and
// windows between the four widths.  The thresholds are where the VALU form takes its tile of 4
// (2) and of 8 (5), and the midpoints of neighbouring widths (21 and 81).
constexpr int kMfmaFromAtmospheres = 5;
constexpr double kMfmaFromPoints = 21.0;
constexpr double kMfmaWidePoints = 81.0;

// The weight of input j in output i: exactly these operations, none contracted (the library is
// built with -ffp-contract=off).  d = u[j] - u[i].
__host__ __device__ __forceinline__ double brd_weight(double d, double twj, double inv_dv,
                                                      double h, int n_tab,
                                                      const double* __restrict__ tab) {
  const double t = d * inv_dv;
  const double q = t + h;
  const double kf = fmin(fmax(floor(q), 0.0), (double)(n_tab - 2));
  const double f = q - kf;
  const int k = (int)kf;
  const double t0 = tab[k];
  const double dt = tab[k + 1] - t0;
  const double fd = f * dt;
  const double K = t0 + fd;
  return twj * K;
}

struct BrdArgs {
  const double* x;   // row m at x + m * xs
  int64_t xs, n;
  const double *u, *tw, *norm, *tab;
  const int32_t *first, *count;
  int n_tab, n_atm;
  double h, inv_dv;
  double* out;       // [n_atm][n]
};

// form 1: one lane per output point, BT atmospheres per lane; rows past n_atm alias the tile's
// first (read, never stored).
template <int BT>
__global__ __launch_bounds__(256) void brd_valu_kernel(const BrdArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int m0 = blockIdx.y * BT;
  const int nr = min(BT, a.n_atm - m0);
  const double* xr[BT];
#pragma unroll
  for (int r = 0; r < BT; ++r) xr[r] = a.x + (int64_t)(m0 + (r < nr ? r : 0)) * a.xs;
  const int64_t j0 = a.first[i], j1 = j0 + a.count[i];
  const double ui = a.u[i];
  double acc[BT];
#pragma unroll
  for (int r = 0; r < BT; ++r) acc[r] = 0.0;
  for (int64_t j = j0; j < j1; ++j) {
    const double d = a.u[j] - ui;
    const double w = brd_weight(d, a.tw[j], a.inv_dv, a.h, a.n_tab, a.tab);
#pragma unroll
    for (int r = 0; r < BT; ++r) acc[r] = fma(w, xr[r][j], acc[r]);
  }
  const double nm = a.norm[i];
#pragma unroll
  for (int r = 0; r < BT; ++r)
    if (r < nr) a.out[(int64_t)(m0 + r) * a.n + i] = acc[r] / nm;
}

// form 2: one wave (one block) per tile of 16 outputs i0 .. i0 + 15 and 16 atmospheres m0 ..
// m0 + 15 on v_mfma_f64_16x16x4_f64 (operand maps as in K12, frei_crosscorr.hip): A = 16 outputs
// x 4 points — lane l holds the weight of output i0 + (l & 15) for the point (l >> 4) of the
// step —, B = 4 points x 16 atmospheres (lane l: point l >> 4, atmosphere l & 15), D = 16 outputs
// x 16 atmospheres (lane l: outputs (l >> 4) + 4 r, atmosphere l & 15).  The tile's span is
// [jlo, jhi) = [first[i0], first[il] + count[il]), il the tile's last output on the axis
// (windows move up with i).  Chunks of 64 points from jlo: lane l reads x[m][jc + l] for the 16
// atmospheres (rows of 64 consecutive doubles) and u, tw at jc + l into registers — a chunk
// ahead of the one being multiplied — and from there into LDS; points at or past jhi and
// atmospheres at or past n_atm enter as 0.  Then the steps s = 0 .. 15 of the chunk (those that
// begin before jhi), each the points jc + 4 s + (0 .. 3), ascending: the lane's weights of all
// steps first (independent chains of LDS read, table gather and arithmetic, in flight together),
// then the matrix steps.  The result passes through LDS once more so that 16 consecutive outputs
// of an atmosphere are stored together.  (Tried and dropped, tools/broaden_probe.py: 2 to 4
// blocks of 16 atmospheres per wave sharing one A operand — the LDS and registers they take
// leave one wave per SIMD, and 64 atmospheres x 129 points ran in 1.38 to 2.19 ms against 0.83.)
__global__ __launch_bounds__(64) void brd_mfma_kernel(const BrdArgs a) {
  typedef double dbl4 __attribute__((ext_vector_type(4)));
  constexpr int kP = 17;   // LDS row pitch in doubles: odd, so the staging stores of 64
                           // consecutive points fall into distinct banks
  constexpr int kSteps = kChunkJ / 4;
  __shared__ double sx[kChunkJ * kP];
  __shared__ double su[kChunkJ], st[kChunkJ];
  const int lane = threadIdx.x;
  const int row = lane & 15, kq = lane >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * 16;
  const int m0 = blockIdx.y * 16;
  const int64_t il = min(i0 + 15, a.n - 1);
  const int64_t jlo = a.first[i0], jhi = (int64_t)a.first[il] + a.count[il];   // uniform
  const int64_t i = i0 + row;
  const bool have = i < a.n;
  const int64_t ic = have ? i : il;
  const int64_t f0 = a.first[ic], f1 = have ? f0 + a.count[ic] : f0;   // empty past the axis
  const double ui = a.u[ic];
  dbl4 acc = dbl4{0.0, 0.0, 0.0, 0.0};
  double nx[16], nu, nt;
  // a uniform row pointer and one 32-bit lane offset for all rows; lanes past the span and rows
  // past n_atm read a valid neighbour (jhi <= n: the loads stay on the axis) and take 0
  auto fetch = [&](int64_t jc) {
    const int nin = (int)min((int64_t)kChunkJ, jhi - jc);   // uniform, >= 1
    const unsigned off = (unsigned)min(lane, nin - 1);
    const bool in = lane < nin;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool rowok = m0 + r < a.n_atm;                  // uniform
      const double* __restrict__ rp = a.x + (int64_t)(rowok ? m0 + r : m0) * a.xs + jc;
      const double v = rp[off];
      nx[r] = (in && rowok) ? v : 0.0;
    }
    const double vu = (a.u + jc)[off], vt = (a.tw + jc)[off];
    nu = in ? vu : 0.0;
    nt = in ? vt : 0.0;
  };
  fetch(jlo);
  for (int64_t jc = jlo; jc < jhi; jc += kChunkJ) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sx[lane * kP + r] = nx[r];
    su[lane] = nu;
    st[lane] = nt;
    __syncthreads();
    if (jc + kChunkJ < jhi) fetch(jc + kChunkJ);    // uniform; in flight during the steps
    const int steps = (int)min((int64_t)kSteps, (jhi - jc + 3) / 4);   // uniform
    double av[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      av[s] = 0.0;
      if (s < steps) {                              // uniform
        const int o = 4 * s + kq;
        const int64_t jj = jc + o;
        const bool mine = jj >= f0 && jj < f1;
        const double d = mine ? su[o] - ui : 0.0;
        const double w = brd_weight(d, st[o], a.inv_dv, a.h, a.n_tab, a.tab);
        av[s] = mine ? w : 0.0;
      }
    }
#pragma unroll
    for (int s = 0; s < kSteps; ++s)
      if (s < steps)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], sx[(4 * s + kq) * kP + row], acc, 0, 0,
                                                   0);
    __syncthreads();
  }
  // D to LDS as [output][atmosphere], then lane l stores the output l & 15 of the atmospheres
  // (l >> 4) + 4 r
#pragma unroll
  for (int r = 0; r < 4; ++r) sx[(kq + 4 * r) * kP + row] = acc[r];
  __syncthreads();
  if (have) {
    const double nm = a.norm[i];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + kq + 4 * r;
      if (m < a.n_atm) a.out[(int64_t)m * a.n + i] = sx[row * kP + kq + 4 * r] / nm;
    }
  }
}

std::string at1(const char* name, int64_t i) {
  return std::string(name) + "[" + std::to_string(i) + "]";
}

}  // namespace

namespace frei {
int brd_kept_rows(frei_brd* b, BrdRows* out) {
  if (!b) return set_error("null broadener");
  out->rows = b->d_keep;
  out->n_lam = b->n_lam;
  out->n_atm = b->keep_atm;
  out->device = b->device;
  return 0;
}
}  // namespace frei

// ==================================================================== C ABI
extern "C" {

int frei_brd_create(frei_brd** out, int device, int64_t n_lam, const double* u, const double* tw,
                    const int32_t* first, const int32_t* count, int n_tab, double dv,
                    double inv_dv, const double* tab) {
  // everything is validated on the host before any device call
  if (!out || !u || !tw || !first || !count || !tab) return set_error("null argument");
  *out = nullptr;
  if (n_lam < 2) return set_error("frei_brd_create: n_lam must be >= 2");
  if (n_lam > INT32_MAX) return set_error("frei_brd_create: n_lam exceeds the int32 plan");
  if (!(dv > 0.0) || !std::isfinite(dv)) return set_error("frei_brd_create: dv must be > 0");
  if (!(inv_dv > 0.0) || !std::isfinite(inv_dv))
    return set_error("frei_brd_create: inv_dv must be > 0");
  if (n_tab < 3 || n_tab % 2 == 0)
    return set_error("frei_brd_create: n_tab = " + std::to_string(n_tab) +
                     " must be odd and >= 3");
  for (int k = 0; k < n_tab; ++k)
    if (!std::isfinite(tab[k]) || tab[k] < 0.0)
      return set_error("frei_brd_create: " + at1("tab", k) + " is negative or not finite");
  for (int64_t j = 0; j < n_lam; ++j) {
    if (!std::isfinite(u[j]))
      return set_error("frei_brd_create: " + at1("u", j) + " is not finite");
    if (j > 0 && !(u[j] > u[j - 1]))
      return set_error("frei_brd_create: " + at1("u", j) + " is not above " + at1("u", j - 1) +
                       ": the axis must be strictly ascending");
    if (!std::isfinite(tw[j]) || tw[j] < 0.0)
      return set_error("frei_brd_create: " + at1("tw", j) + " is negative or not finite");
  }
  const double h = (double)((n_tab - 1) / 2);
  const double H = h * dv;
  std::vector<double> norm((size_t)n_lam);
  int64_t taps = 0;
  for (int64_t i = 0; i < n_lam; ++i) {
    const int64_t f = first[i], c = count[i];
    if (c < 1) return set_error("frei_brd_create: " + at1("count", i) + " is < 1");
    if (f < 0 || f + c > n_lam)
      return set_error("frei_brd_create: the window of output " + std::to_string(i) +
                       " leaves the axis [0, " + std::to_string(n_lam) + ")");
    if (i < f || i >= f + c)
      return set_error("frei_brd_create: the window of output " + std::to_string(i) +
                       " does not contain its own point");
    if (c > FREI_BRD_MAX_COUNT)
      return set_error("frei_brd_create: " + at1("count", i) + " = " + std::to_string(c) +
                       " exceeds the cap of " + std::to_string(FREI_BRD_MAX_COUNT) + " taps");
    // u ascends and a rounded difference is monotone, so the ends decide for the whole run
    if (!(std::fabs(u[f] - u[i]) <= H) || !(std::fabs(u[f + c - 1] - u[i]) <= H))
      return set_error("frei_brd_create: the window of output " + std::to_string(i) +
                       " holds a point farther than the table's half-width");
    if ((f > 0 && std::fabs(u[f - 1] - u[i]) <= H) ||
        (f + c < n_lam && std::fabs(u[f + c] - u[i]) <= H))
      return set_error("frei_brd_create: the window of output " + std::to_string(i) +
                       " leaves out a point within the table's half-width");
    double s = 0.0;
    for (int64_t j = f; j < f + c; ++j)
      s = s + brd_weight(u[j] - u[i], tw[j], inv_dv, h, n_tab, tab);
    if (!std::isfinite(s) || !(s > 0.0))
      return set_error("frei_brd_create: " + at1("norm", i) + " is not finite and > 0");
    norm[(size_t)i] = s;
    taps += c;
  }
  frei_brd* b = new frei_brd();
  b->device = device;
  b->n_lam = n_lam;
  b->n_tab = n_tab;
  b->h = h;
  b->inv_dv = inv_dv;
  b->mean_points = (double)taps / (double)n_lam;
  const size_t n = (size_t)n_lam;
  Stream& st = b->stream;   // (the copies complete before the sources go)
  if (hipSetDevice(device) != hipSuccess || st.create() || upload(b->d_u, u, n, st) ||
      upload(b->d_tw, tw, n, st) || upload(b->d_norm, norm.data(), n, st) ||
      upload(b->d_tab, tab, (size_t)n_tab, st) || upload(b->d_first, first, n, st) ||
      upload(b->d_count, count, n, st) || hipStreamSynchronize(st) != hipSuccess) {
    delete b;
    (void)hipGetLastError();
    return set_error("frei_brd_create: device allocation or copy failed");
  }
  *out = b;
  return 0;
}

int frei_brd_destroy(frei_brd* b) {
  if (b) delete b;
  return 0;
}

int frei_brd_norm(frei_brd* b, double* norm) {
  if (!b || !norm) return set_error("frei_brd_norm: null argument");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipMemcpy(norm, b->d_norm, (size_t)b->n_lam * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// The four sources of x — a host array, a context's emergent rows, an interpolator's kept
// result (K15), a phase integrator's (K16) — feed the same x and stride below.
static int brd_apply_impl(frei_brd* b, frei_ctx* ctx, const double* x, frei_itp* itp,
                          frei_phs* phs, int n_atm, int form, double* out, int keep,
                          int* form_used, double* kernel_ms) {
  if (!b) return set_error("frei_brd_apply: null handle");
  if (!x && !ctx && !itp && !phs) return set_error("frei_brd_apply: x and ctx are both null");
  if (!out && !keep) return set_error("frei_brd_apply: out is null and keep is not set");
  if (n_atm < 1) return set_error("frei_brd_apply: n_atm must be >= 1");
  if (form < 0 || form > 2)
    return set_error("frei_brd_apply: form must be 0 (automatic), 1 (VALU) or 2 (fp64 MFMA)");
  SpectrumRows src;
  TRY(spectrum_rows(x, ctx, nullptr, itp, phs, n_atm, b->n_lam, b->device, b->stream, "broadener",
                    "frei_brd_apply", &src));
  int f = form;
  if (f == 0)
    f = (n_atm >= kMfmaFromAtmospheres && b->mean_points >= kMfmaFromPoints) ||
                (n_atm >= 2 && b->mean_points >= kMfmaWidePoints)
            ? 2
            : 1;
  if (form_used) *form_used = f;

  HIP_TRY(hipSetDevice(b->device));
  // what an earlier call kept ends here, whether or not this call succeeds
  if (b->d_keep) {
    (void)hipStreamSynchronize(b->stream);
    b->d_keep.reset();
    b->keep_atm = 0;
  }
  hipStream_t st = src.stream;
  const size_t A = (size_t)n_atm, n = (size_t)b->n_lam;
  // form 1: 1, 4 or 8 atmospheres per lane; form 2: blocks of 16 atmospheres
  const int bt = n_atm == 1 ? 1 : n_atm <= 4 ? 4 : 8;
  const int cb = (n_atm + 15) / 16;
  if ((n_atm + bt - 1) / bt > 65535)
    return set_error("frei_brd_apply: n_atm exceeds the launch grid");
  DeviceCall call(st, "broadening");
  const double* u_x = call.upload(x, A * n);
  double* d_out = call.alloc<double>(A * n);
  call.begin(kernel_ms);
  if (call.ok()) {
    BrdArgs a;
    a.x = u_x ? u_x : src.rows;
    a.xs = src.stride;
    a.n = b->n_lam;
    a.u = b->d_u;
    a.tw = b->d_tw;
    a.norm = b->d_norm;
    a.tab = b->d_tab;
    a.first = b->d_first;
    a.count = b->d_count;
    a.n_tab = b->n_tab;
    a.n_atm = n_atm;
    a.h = b->h;
    a.inv_dv = b->inv_dv;
    a.out = d_out;
    const dim3 g1((unsigned)((n + 255) / 256), (unsigned)((n_atm + bt - 1) / bt));
    const dim3 g2((unsigned)((n + 15) / 16), (unsigned)cb);
    if (f == 1) {
      if (bt == 1) brd_valu_kernel<1><<<g1, 256, 0, st>>>(a);
      else if (bt == 4) brd_valu_kernel<4><<<g1, 256, 0, st>>>(a);
      else brd_valu_kernel<8><<<g1, 256, 0, st>>>(a);
    } else {
      brd_mfma_kernel<<<g2, 64, 0, st>>>(a);
    }
  }
  call.end();
  call.download(out, d_out, A * n);
  if (keep) call.keep(d_out);
  const int rc = call.finish();
  if (!rc && keep) {
    b->d_keep.adopt(d_out, A * n);   // complete: finish() synchronised the stream
    b->keep_atm = n_atm;
  }
  return rc;
}

int frei_brd_apply(frei_brd* b, frei_ctx* ctx, const double* x, int n_atm, int form,
                   double* out, int keep, int* form_used, double* kernel_ms) {
  return brd_apply_impl(b, ctx, x, nullptr, nullptr, n_atm, form, out, keep, form_used,
                        kernel_ms);
}

int frei_brd_apply_itp(frei_brd* b, frei_itp* src, int n_atm, int form, double* out, int keep,
                       int* form_used, double* kernel_ms) {
  if (!src) return set_error("frei_brd_apply_itp: null interpolator");
  return brd_apply_impl(b, nullptr, nullptr, src, nullptr, n_atm, form, out, keep, form_used,
                        kernel_ms);
}

int frei_brd_apply_phs(frei_brd* b, frei_phs* src, int n_atm, int form, double* out, int keep,
                       int* form_used, double* kernel_ms) {
  if (!src) return set_error("frei_brd_apply_phs: null phase integrator");
  return brd_apply_impl(b, nullptr, nullptr, nullptr, src, n_atm, form, out, keep, form_used,
                        kernel_ms);
}

}  // extern "C"
