// frei_stack.hip — K14: the detection statistic of the cross-correlation sums (CCF or the
// Brogi & Line log-likelihood) and its stack over the exposures along trial orbits, one
// K_p-V_sys map per atmosphere.  The reference has no counterpart; the definition is the header
// comment of frei_stack_apply in include/frei_hip.h.
//
// Statistic pass (stack_statistic_kernel): one lane per (m, e, v) of [n_atm][n_exp][n_vel],
//   gbar = sg / W;  C_fg = sfg - gbar * S_wf[e];  V_g = sgg - sg * gbar;  V_f[e] from the host;
//   ccf = C_fg / sqrt(V_f * V_g);  loglike = half * log(((V_f - 2 * C_fg) + V_g) / W),
//   half = -(n_eff / 2) formed on the host.  Plain IEEE operations in that order, nothing
//   contracted (-ffp-contract=off); / and sqrt are the correctly rounded ones.
// Stack pass (stack_kernel): lanes over s (256 per block), blockIdx.y = k, blockIdx.z = a tile
//   of kAT atmospheres.  Per exposure, ascending, a lane forms
//     u = (vsys[s] + dv[k][e]) + v_obs[e], clamped to [vel[0], vel[n_vel-1]],
//     j = the largest index with vel[j] <= u limited to n_vel - 2, by a binary search whose trip
//       count depends on n_vel alone (no divergence),
//     t = (u - vel[j]) / (vel[j+1] - vel[j])
//   once for the tile, and then for each atmosphere of the tile
//     val = f[j] + t * (f[j+1] - f[j]);  acc = acc + val        (f = values[m][e][:])
//   with all 2 kAT loads issued before the first use.  dv[k][e] and v_obs[e] are uniform over the
//   block (scalar loads).  The search runs on a copy of vel in LDS (form 1, n_vel <= kLdsVel) or
//   on vel in global memory (form 2); the values are read where they lie — the lanes' brackets
//   are near-consecutive for a monotone vsys and the 13 MB of the headline shape stay in L2.
//   Atmospheres past the end of a tile alias the tile's first (read, never stored).
// One accumulator per output, no atomics, the order of summation fixed by n_exp: results repeat
// bit for bit, a row alone is bitwise its row of the batch, an output does not depend on which
// other k or s the handle holds, and the two forms agree bitwise.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

struct frei_stack {
  Stream stream;   // first: destroyed last; created by the first apply, before any buffer
  int device = 0;
  int n_exp = 0, n_vel = 0, n_kp = 0, n_vsys = 0;
  // the host copies frei_stack_create checked; uploaded by the first apply
  std::vector<double> vel, dv, v_obs, vsys;
  bool resident = false;
  DevBuf<double> d_vel;    // [n_vel]
  DevBuf<double> d_dv;     // [n_kp][n_exp]
  DevBuf<double> d_vobs;   // [n_exp]
  DevBuf<double> d_vsys;   // [n_vsys]
  ~frei_stack() {
    if (!stream) return;   // no device was touched
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
  }
};

namespace {

constexpr int kAT = 8;                          // atmospheres per lane (frei_amd.stack.ATM_TILE)
constexpr int kLdsVel = FREI_STACK_LDS_VEL;     // the longest vel that form 1 copies to LDS
constexpr int kThreads = 256;

struct StackArgs {
  const double *vel, *dv, *vobs, *vsys;
  const double* f;      // values [n_atm][n_exp][n_vel]
  double* map;          // [n_atm][n_kp][n_vsys]
  int n_vel, n_exp, n_kp, n_vsys, n_atm;
};

__global__ __launch_bounds__(256) void stack_statistic_kernel(
    const double* __restrict__ sfg, const double* __restrict__ sg,
    const double* __restrict__ sgg, const double* __restrict__ swf,
    const double* __restrict__ vf, double W, double half, int statistic, int n_exp, int n_vel,
    int64_t total, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t me = i / n_vel;
  const int v = (int)(i - me * n_vel);
  const int64_t m = me / n_exp;
  const int e = (int)(me - m * n_exp);
  const double g = sg[m * n_vel + v];
  const double gbar = g / W;
  const double gs = gbar * swf[e];
  const double c_fg = sfg[i] - gs;
  const double gg = g * gbar;
  const double v_g = sgg[m * n_vel + v] - gg;
  const double v_f = vf[e];
  double r;
  if (statistic == 1) {
    const double p = v_f * v_g;
    r = c_fg / sqrt(p);
  } else {
    const double c2 = 2.0 * c_fg;
    const double d = v_f - c2;
    const double q = (d + v_g) / W;
    r = half * log(q);
  }
  out[i] = r;
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void stack_kernel(const StackArgs a) {
  __shared__ double s_vel[LDS ? kLdsVel : 1];
  if (LDS) {
    for (int i = threadIdx.x; i < a.n_vel; i += kThreads) s_vel[i] = a.vel[i];
    __syncthreads();
  }
  const double* vg = LDS ? s_vel : a.vel;
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= a.n_vsys) return;                    // after the block's only barrier
  const int k = blockIdx.y;
  const int m0 = blockIdx.z * kAT;
  const int nr = min(kAT, a.n_atm - m0);
  const int64_t row = (int64_t)a.n_exp * a.n_vel;
  const double* fr[kAT];
#pragma unroll
  for (int r = 0; r < kAT; ++r) fr[r] = a.f + (int64_t)(m0 + (r < nr ? r : 0)) * row;
  const double vs = a.vsys[s];
  const double v_lo = vg[0], v_hi = vg[a.n_vel - 1];
  const double* dvk = a.dv + (int64_t)k * a.n_exp;
  double acc[kAT];
#pragma unroll
  for (int r = 0; r < kAT; ++r) acc[r] = 0.0;
  for (int e = 0; e < a.n_exp; ++e) {
    double u = (vs + dvk[e]) + a.vobs[e];
    u = u < v_lo ? v_lo : (u > v_hi ? v_hi : u);
    int lo = 0, hi = a.n_vel - 2;               // the largest j in [0, n_vel - 2] with vel[j] <= u
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (vg[mid] <= u) lo = mid; else hi = mid - 1;
    }
    const double x0 = vg[lo], x1 = vg[lo + 1];
    const double t = (u - x0) / (x1 - x0);
    const int64_t o = (int64_t)e * a.n_vel + lo;
    double f0[kAT], f1[kAT];
#pragma unroll
    for (int r = 0; r < kAT; ++r) {
      f0[r] = fr[r][o];
      f1[r] = fr[r][o + 1];
    }
#pragma unroll
    for (int r = 0; r < kAT; ++r) {
      // three operations, not contracted
      const double d = f1[r] - f0[r];
      const double td = t * d;
      const double val = f0[r] + td;
      acc[r] = acc[r] + val;
    }
  }
#pragma unroll
  for (int r = 0; r < kAT; ++r)
    if (r < nr) a.map[((int64_t)(m0 + r) * a.n_kp + k) * a.n_vsys + s] = acc[r];
}

std::string at1(const char* name, int64_t i) {
  return std::string(name) + "[" + std::to_string(i) + "]";
}

int check_finite(const char* name, const double* x, int64_t n, int64_t cols) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i]))
      return set_error("frei_stack_create: " +
                       (cols ? at1(name, i / cols) + "[" + std::to_string(i % cols) + "]"
                             : at1(name, i)) +
                       " is not finite");
  return 0;
}

// The stacker's arrays on its device, uploaded once.
int make_resident(frei_stack* s) {
  if (s->resident) return 0;
  HIP_TRY(hipSetDevice(s->device));
  if (!s->stream) TRY(s->stream.create());
  auto up = [&](DevBuf<double>& d, const std::vector<double>& h) {
    if (!d) TRY(d.alloc(h.size()));
    HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
  };
  TRY(up(s->d_vel, s->vel));
  TRY(up(s->d_dv, s->dv));
  TRY(up(s->d_vobs, s->v_obs));
  TRY(up(s->d_vsys, s->vsys));
  s->resident = true;
  return 0;
}

}  // namespace

// ==================================================================== C ABI
extern "C" {

int frei_stack_create(frei_stack** out, int device, int n_exp, int n_vel, const double* vel,
                      int n_kp, const double* dv, const double* v_obs, int n_vsys,
                      const double* vsys) {
  // everything is validated on the host; no device is touched before the first apply
  if (!out || !vel || !dv || !v_obs || !vsys) return set_error("null argument");
  *out = nullptr;
  if (n_exp < 1) return set_error("frei_stack_create: n_exp must be >= 1");
  if (n_vel < 2) return set_error("frei_stack_create: n_vel must be >= 2");
  if (n_kp < 1) return set_error("frei_stack_create: n_kp must be >= 1");
  if (n_vsys < 1) return set_error("frei_stack_create: n_vsys must be >= 1");
  for (int j = 0; j < n_vel; ++j) {
    if (!std::isfinite(vel[j]))
      return set_error("frei_stack_create: " + at1("vel", j) + " is not finite");
    if (j > 0 && !(vel[j] > vel[j - 1]))
      return set_error("frei_stack_create: " + at1("vel", j) + " is not above " +
                       at1("vel", j - 1) + ": the velocities must be strictly ascending");
  }
  TRY(check_finite("dv", dv, (int64_t)n_kp * n_exp, n_exp));
  TRY(check_finite("v_obs", v_obs, n_exp, 0));
  TRY(check_finite("vsys", vsys, n_vsys, 0));
  frei_stack* s = new frei_stack();
  s->device = device;
  s->n_exp = n_exp;
  s->n_vel = n_vel;
  s->n_kp = n_kp;
  s->n_vsys = n_vsys;
  s->vel.assign(vel, vel + n_vel);
  s->dv.assign(dv, dv + (size_t)n_kp * (size_t)n_exp);
  s->v_obs.assign(v_obs, v_obs + n_exp);
  s->vsys.assign(vsys, vsys + n_vsys);
  *out = s;
  return 0;
}

int frei_stack_destroy(frei_stack* s) {
  if (s) delete s;
  return 0;
}

int frei_stack_apply(frei_stack* s, frei_ccf* kept, int n_atm, const double* sfg,
                     const double* sg, const double* sgg, int statistic, double W,
                     const double* S_wf, const double* S_wff, double n_eff, double* map,
                     double* values, int form, int* form_used, double* kernel_ms) {
  const std::string me = "frei_stack_apply: ";
  if (!s) return set_error(me + "null handle");
  if (!map) return set_error(me + "map is null");
  if (n_atm < 1) return set_error(me + "n_atm must be >= 1");
  if (statistic < 0 || statistic > 2)
    return set_error(me + "statistic must be 0 (values), 1 (ccf) or 2 (loglike)");
  if (form < 0 || form > 2)
    return set_error(me + "form must be 0 (automatic), 1 (velocities in LDS) or 2 (in global "
                          "memory)");
  if (form == 1 && s->n_vel > kLdsVel)
    return set_error(me + "form 1 holds at most " + std::to_string(kLdsVel) +
                     " velocities in LDS, not n_vel = " + std::to_string(s->n_vel));
  const bool stat = statistic != 0;
  const bool host = sfg || sg || sgg;
  if (!host && !kept) return set_error(me + "neither host sums nor a kept source");
  if (host && !sfg) return set_error(me + "the host sums lack sfg");
  if (host && stat && (!sg || !sgg))
    return set_error(me + "the statistic needs sfg, sg and sgg");
  if (stat && (!S_wf || !S_wff || W == 0.0))
    return set_error(me + "the statistic needs W, S_wf and S_wff");
  CcfKept ks{};
  if (!host) {
    TRY(ccf_kept_sums(kept, &ks));
    if (!ks.sfg && !ks.sg && !ks.sgg)
      return set_error(me + "the correlator holds nothing kept (frei_ccf_keep, then apply)");
    if (!ks.sfg || (stat && (!ks.sg || !ks.sgg)))
      return set_error(me + "a kept sum is missing: statistic " + std::to_string(statistic) +
                       " needs " + (stat ? "sfg, sg and sgg" : "sfg"));
    if (ks.n_atm != n_atm)
      return set_error(me + "the correlator keeps " + std::to_string(ks.n_atm) +
                       " atmospheres, not n_atm = " + std::to_string(n_atm));
    if (ks.n_exp != s->n_exp)
      return set_error(me + "the correlator's n_exp = " + std::to_string(ks.n_exp) +
                       " is not the stacker's " + std::to_string(s->n_exp));
    if (ks.n_vel != s->n_vel)
      return set_error(me + "the correlator's n_vel = " + std::to_string(ks.n_vel) +
                       " is not the stacker's " + std::to_string(s->n_vel));
    if (ks.device != s->device)
      return set_error(me + "correlator and stacker live on different devices");
  }
  const int tiles = (n_atm + kAT - 1) / kAT;
  if (s->n_kp > 65535 || tiles > 65535)
    return set_error(me + "n_kp or n_atm / 8 exceeds the launch grid");
  const int f = form ? form : (s->n_vel <= kLdsVel ? 1 : 2);
  if (form_used) *form_used = f;

  TRY(make_resident(s));
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const size_t A = (size_t)n_atm, E = (size_t)s->n_exp, V = (size_t)s->n_vel;
  std::vector<double> vf;   // V_f[e]; lives until finish()
  if (stat) {
    vf.resize(E);
    for (size_t e = 0; e < E; ++e) {
      const double sq = S_wf[e] * S_wf[e];
      vf[e] = S_wff[e] - sq / W;
    }
  }
  const double half = -(n_eff / 2.0);
  DeviceCall call(st, "orbital stack");
  const double* d_sfg = host ? call.upload(sfg, A * E * V) : ks.sfg;
  const double* d_sg = host ? call.upload(stat ? sg : nullptr, A * V) : ks.sg;
  const double* d_sgg = host ? call.upload(stat ? sgg : nullptr, A * V) : ks.sgg;
  const double* d_swf = call.upload(stat ? S_wf : nullptr, E);
  const double* d_vf = call.upload(stat ? vf.data() : nullptr, E);
  double* d_val = stat ? call.alloc<double>(A * E * V) : nullptr;
  double* d_map = call.alloc<double>(A * (size_t)s->n_kp * (size_t)s->n_vsys);
  call.begin(kernel_ms);
  if (call.ok()) {
    const int64_t total = (int64_t)(A * E * V);
    if (stat)
      stack_statistic_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(
          d_sfg, d_sg, d_sgg, d_swf, d_vf, W, half, statistic, s->n_exp, s->n_vel, total, d_val);
    StackArgs a;
    a.vel = s->d_vel;
    a.dv = s->d_dv;
    a.vobs = s->d_vobs;
    a.vsys = s->d_vsys;
    a.f = stat ? d_val : d_sfg;
    a.map = d_map;
    a.n_vel = s->n_vel;
    a.n_exp = s->n_exp;
    a.n_kp = s->n_kp;
    a.n_vsys = s->n_vsys;
    a.n_atm = n_atm;
    const dim3 grid((unsigned)((s->n_vsys + kThreads - 1) / kThreads), (unsigned)s->n_kp,
                    (unsigned)tiles);
    if (f == 1) stack_kernel<true><<<grid, kThreads, 0, st>>>(a);
    else stack_kernel<false><<<grid, kThreads, 0, st>>>(a);
  }
  call.end();
  call.download(map, d_map, A * (size_t)s->n_kp * (size_t)s->n_vsys);
  call.download(values, stat ? d_val : d_sfg, A * E * V);
  return call.finish();
}

}  // extern "C"
