// frei_phase.hip — K16: phase curves.  A batch's columns are the cells of a planet's surface;
// per orbital phase p the disk integral out[p][j] = sum_c coef[p][c] I_pc[j] runs over the cells
// visible at p (mu[p][c] > 0), I_pc being frei_emergent's intensity of atmosphere select[c] at
// the angle mu[p][c].  The reference has no counterpart; the definition is the header comment of
// frei_phs_apply in include/frei_hip.h.
//
// One lane per wavelength, grid (256-wavelength blocks, tiles of kTile = 8 consecutive phases), as
// K11.  A block owns its tile's accumulators in registers and walks the tile's visits: the cells
// visible at one phase of the tile or more, ascending, listed on the host at create.  A visit
// holds the cell's row and, compacted, the nv <= 8 phases of the tile that see the cell: 1 / mu,
// coef and the accumulator each belongs to.  The lane walks the cell's column upwards once with
// those nv rays (K11's pass at width nv: each dtaus[l][j] loaded once, kAhead shells ahead of its
// use, B_{l+1} formed once per shell for every ray), so pairs that see nothing cost nothing and a
// cell no phase of the tile sees is never visited.  A visit is wave-uniform and arrives through
// scalar loads; the pass width is chosen by a scalar branch, the accumulator by selects.  Every
// ray's recurrence is K11's own code (column_walk, shell_step and planck_em of frei_math.h;
// the library is built with -ffp-contract=off), so I_pc is bitwise frei_emergent's intensity and
// does not depend on the width of the pass, on the tile or on what else the plan holds.  The sum
// takes its terms in ascending c, the first one starting it: one multiply and one add per later
// term.  No LDS, no atomics, no barrier.
//
// Measured (MI355X, 60 layers; tools/phase_probe.py, profiles/r16/phase/README.md): 16 x 8 cells x
// 32 phases x 100k wavelengths 20.9 ms, 32 x 16 cells x 64 phases 135 ms, 16 cells x 32 phases x
// 500k wavelengths 10.0 ms; 5.8e11, 7.2e11 and 7.5e11 shell steps per second against 6.9e11 to
// 7.2e11 for K11 at 8 angles in the same process (the first shape is a launch of only 1564
// workgroups, about 1.5 rounds of what the CUs hold).  118 VGPRs, 4 waves per SIMD, no scratch.
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"
#include "frei_math.h"

using namespace frei;

namespace {

constexpr int kTile = 8;    // phases per block (their sums in registers): K11's measured tile
constexpr int kAhead = 4;   // shells a column value is loaded ahead of its use, as K11
constexpr int kFirst = 0x100;

// One cell as one tile of phases sees it.  slot[k] = the tile's accumulator (0 .. kTile - 1) of
// ray k, ascending in k, | kFirst where the cell is the first the phase sees.
struct PhsVisit {
  double imu[kTile];
  double coef[kTile];
  int32_t row, nv;
  int32_t slot[kTile];
};
static_assert(sizeof(PhsVisit) % sizeof(double) == 0, "visits lie back to back, 8-byte aligned");

struct PhsArgs {
  const double* dtaus;        // [n_atm][nL][n]
  const double* c1;           // [n]
  const double* hcl;          // [n]
  const double* iT;           // [n_atm][nL + 1]: 1 / T_l, l = 1 .. nL
  const PhsVisit* visits;     // tile t's are tile_off[t] .. tile_off[t + 1] - 1
  const int32_t* tile_off;    // [n_tile + 1]
  int n_phase, nL;
  int64_t n;
  double* out;                // [n_phase][n]
};

// One term into the accumulator s names: it starts the sum with kFirst, else one add.  The
// accumulators are indexed by constants and chosen by wave-uniform selects, never by a run-time
// index (which would move them out of the registers).
template <int... Ts>
__device__ __forceinline__ void add_term(double (&acc)[kTile], int s, double term,
                                         std::integer_sequence<int, Ts...>) {
  const int slot = s & (kFirst - 1);
  const bool first = (s & kFirst) != 0;
  ((acc[Ts] = slot == Ts ? (first ? term : acc[Ts] + term) : acc[Ts]), ...);
}

// The TI rays of one visit along one column (column_walk of frei_math.h, K11's own walk), then
// their terms into the accumulators they belong to.
template <int TI>
__device__ __forceinline__ void phase_pass(const double* __restrict__ col, int64_t n, int nS,
                                           double c1, double hcl, const double* __restrict__ it,
                                           const PhsVisit* __restrict__ v, double (&acc)[kTile]) {
  double w[TI], I[TI];
#pragma unroll
  for (int t = 0; t < TI; ++t) w[t] = v->imu[t];
  column_walk<TI, kAhead>(col, n, nS, c1, hcl, it, w, I);
  // ray k belongs to accumulator slot[k] >= k
#pragma unroll
  for (int k = 0; k < TI; ++k)
    add_term(acc, v->slot[k], v->coef[k] * I[k], std::make_integer_sequence<int, kTile>{});
}

__global__ __launch_bounds__(256) void phase_kernel(const PhsArgs a) {
  const int tile = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const int nS = a.nL - 1;                              // shells 1 .. nS
  const double c1 = a.c1[j], hcl = a.hcl[j];
  double acc[kTile];
#pragma unroll
  for (int t = 0; t < kTile; ++t) acc[t] = 0.0;         // a phase that sees no cell
  const int v1 = a.tile_off[tile + 1];
  for (int i = a.tile_off[tile]; i < v1; ++i) {
    const PhsVisit* __restrict__ v = a.visits + i;
    const int m = v->row;
    const double* __restrict__ col = a.dtaus + (int64_t)m * a.nL * a.n + j;
    const double* __restrict__ it = a.iT + (int64_t)m * (a.nL + 1);
    switch (v->nv) {                                    // the pass at the visit's own width
      case 1: phase_pass<1>(col, a.n, nS, c1, hcl, it, v, acc); break;
      case 2: phase_pass<2>(col, a.n, nS, c1, hcl, it, v, acc); break;
      case 3: phase_pass<3>(col, a.n, nS, c1, hcl, it, v, acc); break;
      case 4: phase_pass<4>(col, a.n, nS, c1, hcl, it, v, acc); break;
      case 5: phase_pass<5>(col, a.n, nS, c1, hcl, it, v, acc); break;
      case 6: phase_pass<6>(col, a.n, nS, c1, hcl, it, v, acc); break;
      case 7: phase_pass<7>(col, a.n, nS, c1, hcl, it, v, acc); break;
      case 8: phase_pass<8>(col, a.n, nS, c1, hcl, it, v, acc); break;
      default: break;
    }
  }
  const int p0 = tile * kTile;
#pragma unroll
  for (int t = 0; t < kTile; ++t)
    if (p0 + t < a.n_phase) a.out[(int64_t)(p0 + t) * a.n + j] = acc[t];
}

std::string at2(const char* name, int p, int c) {
  return std::string(name) + "[" + std::to_string(p) + "][" + std::to_string(c) + "]";
}

}  // namespace

struct frei_phs {
  int device = 0;
  int n_cell = 0, n_phase = 0, n_tile = 0;
  std::vector<int32_t> select;        // [n_cell]
  std::vector<char> visible_cell;     // [n_cell]: some phase sees the cell
  // the plan frei_phs_create built; uploaded by the first apply
  std::vector<PhsVisit> visits;
  std::vector<int32_t> tile_off;      // [n_tile + 1]
  bool resident = false;
  DevBuf<PhsVisit> d_visits;
  DevBuf<int32_t> d_tile_off;
  // The result buffer, reused from call to call and grown when a call needs more, of which the
  // first n_phase * keep_lam doubles are the last apply's result when it asked to keep
  // (keep_lam = 0: nothing kept).
  DevBuf<double> d_out;
  int64_t keep_lam = 0;
  // (no stream of its own: it works on the context's, and every apply ends synchronised)
  ~frei_phs() {
    if (d_visits || d_tile_off || d_out) (void)hipSetDevice(device);
  }
};

namespace {

// The handle's plan on its device, uploaded once.
int make_resident(frei_phs* p) {
  if (p->resident) return 0;
  const size_t nv = p->visits.size();
  if (!p->d_visits) TRY(p->d_visits.alloc(nv));
  if (!p->d_tile_off) TRY(p->d_tile_off.alloc(p->tile_off.size()));
  if (nv)
    HIP_TRY(hipMemcpy(p->d_visits, p->visits.data(), nv * sizeof(PhsVisit),
                      hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_tile_off, p->tile_off.data(), p->tile_off.size() * sizeof(int32_t),
                    hipMemcpyHostToDevice));
  p->resident = true;
  return 0;
}

}  // namespace

namespace frei {
int phs_kept_rows(frei_phs* p, PhsRows* out) {
  if (!p) return set_error("null phase integrator");
  out->rows = p->keep_lam ? p->d_out : nullptr;
  out->n_lam = p->keep_lam;
  out->n_phase = p->n_phase;
  out->device = p->device;
  return 0;
}
}  // namespace frei

// ==================================================================== C ABI
extern "C" {

int frei_phs_create(frei_phs** out, int device, int n_cell, int n_phase, const int32_t* select,
                    const double* mu, const double* coef) {
  // everything is validated on the host; no device is touched before the first apply
  const std::string me = "frei_phs_create: ";
  if (!out || !select || !mu || !coef) return set_error(me + "null argument");
  *out = nullptr;
  if (device < 0) return set_error(me + "device must be >= 0");
  if (n_cell < 1) return set_error(me + "n_cell must be >= 1");
  if (n_phase < 1) return set_error(me + "n_phase must be >= 1");
  for (int c = 0; c < n_cell; ++c)
    if (select[c] < 0)
      return set_error(me + "select[" + std::to_string(c) + "] = " + std::to_string(select[c]) +
                       " must be >= 0");
  const size_t C = (size_t)n_cell;
  for (int p = 0; p < n_phase; ++p)
    for (int c = 0; c < n_cell; ++c) {
      const double m = mu[p * C + c];
      if (!std::isfinite(m) || m > 1.0)
        return set_error(me + at2("mu", p, c) + " must be finite and <= 1");
      if (!(m > 0.0)) continue;                  // invisible: its coef is never read
      if (!std::isfinite(1.0 / m)) return set_error(me + "1 / " + at2("mu", p, c) + " overflows");
      const double k = coef[p * C + c];
      if (!std::isfinite(k) || k < 0.0)
        return set_error(me + at2("coef", p, c) + " must be finite and >= 0");
    }
  frei_phs* h = new frei_phs();
  h->device = device;
  h->n_cell = n_cell;
  h->n_phase = n_phase;
  h->n_tile = (n_phase + kTile - 1) / kTile;
  h->select.assign(select, select + n_cell);
  h->visible_cell.assign(C, 0);
  h->tile_off.reserve((size_t)h->n_tile + 1);
  for (int t = 0; t < h->n_tile; ++t) {
    h->tile_off.push_back((int32_t)h->visits.size());
    const int p0 = t * kTile, p1 = std::min(n_phase, p0 + kTile);
    bool started[kTile] = {};
    for (int c = 0; c < n_cell; ++c) {
      PhsVisit v{};
      v.row = select[c];
      for (int p = p0; p < p1; ++p) {
        const double m = mu[p * C + c];
        if (!(m > 0.0)) continue;
        v.imu[v.nv] = 1.0 / m;
        v.coef[v.nv] = coef[p * C + c];
        v.slot[v.nv] = (p - p0) | (started[p - p0] ? 0 : kFirst);
        started[p - p0] = true;
        ++v.nv;
      }
      if (!v.nv) continue;
      h->visible_cell[c] = 1;
      h->visits.push_back(v);
    }
  }
  h->tile_off.push_back((int32_t)h->visits.size());
  *out = h;
  return 0;
}

int frei_phs_destroy(frei_phs* p) {
  if (p) delete p;
  return 0;
}

int frei_phs_apply(frei_phs* p, frei_ctx* ctx, const double* dtaus, const double* T, double* out,
                   int keep, int form, int* form_used, double* kernel_ms) {
  const std::string me = "frei_phs_apply: ";
  if (!p) return set_error(me + "null handle");
  if (p->n_tile > 65535)
    return set_error(me + "n_phase / 8 exceeds the launch grid (65535 tiles)");
  if (!ctx || !T) return set_error(me + "null context or null T");
  if (!out && !keep) return set_error(me + "out is null and keep is not set");
  if (form < 0 || form > 1) return set_error(me + "form must be 0 (automatic) or 1");
  CtxColumns cc{};
  TRY(ctx_columns(ctx, false, &cc));
  if (cc.device != p->device)
    return set_error(me + "context and phase integrator live on different devices");
  const size_t A = (size_t)cc.n_atm, nL = (size_t)cc.nL, n = (size_t)cc.n_lam, per = nL * n;
  // 1 / T_l of the atmospheres some visible cell uses, formed here once per call (wave-uniform
  // in the kernel) as frei_emergent forms them; the others' rows are never read
  std::vector<char> used(A, 0);
  for (int c = 0; c < p->n_cell; ++c) {
    if ((size_t)p->select[c] >= A)
      return set_error(me + "select[" + std::to_string(c) + "] = " +
                       std::to_string(p->select[c]) + " lies outside [0, n_atm = " +
                       std::to_string(A) + ") (cell " + std::to_string(c) + ")");
    if (p->visible_cell[c]) used[p->select[c]] = 1;
  }
  std::vector<double> iT(A * (nL + 1), 0.0);
  for (size_t m = 0; m < A; ++m) {
    if (!used[m]) continue;
    for (size_t l = 1; l < nL; ++l) {
      const double t = T[m * nL + l];
      if (!(std::isfinite(t) && t > 0.0))
        return set_error(me + "T must be finite and positive (atmosphere " + std::to_string(m) +
                         ", layer " + std::to_string(l) + ")");
      iT[m * (nL + 1) + l] = 1.0 / t;
    }
    iT[m * (nL + 1) + nL] = iT[m * (nL + 1) + nL - 1];
  }
  if (!dtaus) TRY(ctx_columns(ctx, true, &cc));
  if (form_used) *form_used = 1;

  HIP_TRY(hipSetDevice(p->device));
  p->keep_lam = 0;   // what an earlier call kept ends here, whether or not this call succeeds
  TRY(make_resident(p));
  const size_t P = (size_t)p->n_phase;
  DeviceCall call(cc.stream, "phase curve");
  call.check(p->d_out.reserve(P * n));   // every earlier call has finished (synchronised)
  const double* u_dt = call.upload(dtaus, A * per);
  PhsArgs a;
  a.dtaus = u_dt ? u_dt : cc.dtaus;
  a.c1 = cc.c1;
  a.hcl = cc.hcl;
  a.iT = call.upload(iT.data(), iT.size());
  a.visits = p->d_visits;
  a.tile_off = p->d_tile_off;
  a.n_phase = p->n_phase;
  a.nL = cc.nL;
  a.n = cc.n_lam;
  a.out = p->d_out;
  call.begin(kernel_ms);
  if (call.ok()) {
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)p->n_tile);
    phase_kernel<<<grid, 256, 0, cc.stream>>>(a);
  }
  call.end();
  call.download(out, a.out, P * n);
  const int rc = call.finish();   // the host vectors are read by the uploads until here
  if (!rc && keep) p->keep_lam = cc.n_lam;   // complete: finish() synchronised the stream
  return rc;
}

}  // extern "C"
