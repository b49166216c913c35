// frei_crosscorr.hip — K12: Doppler cross-correlation of batched spectra with high-resolution
// data.  Templates y[n_atm][n_lam] are sampled at the data's pixels for every trial velocity
// (a resident plan idx / frac) and summed against every exposure: S_fg, S_g, S_gg.  The reference
// has no counterpart; the definition is the header comment of frei_ccf_apply in
// include/frei_hip.h.
//
// Data: the plan (idx int32, frac double: [n_vel][p_pad], rows pitched to 16 pixels), the
// weighted data as a[n_exp][n_pix] (form 1: a wave's pixels contiguous) and transposed to
// aT[p_pad][e_pad] (form 2: e_pad = n_exp rounded up to 16, an MFMA step's 16 exposures one
// 128-byte row) and the pixel weights stay resident in HBM with the handle; pads are zeros.  Per call a small pre-pass forms y = scale (x / den) - offset (skipped
// when all three are absent: x is read where it lies).  The pixels are cut into chunks of kChunk;
// a wave sums one chunk for its tile of (atmospheres, velocities, exposures), in one of two forms:
//   form 1 (ccf_valu_kernel): lane l forms g and accumulates a * g (fma) for the pixels l,
//     l + 64, ... of the chunk in order; the 64 lane sums combine in the xor butterfly 32, ..., 1
//     (every lane ends with the same bits).  A register tile of kAT x kVT x kET sums per lane;
//     the same kernel with w in place of a gives S_g and S_gg.
//   form 2 (ccf_mfma_kernel): S_fg on v_mfma_f64_16x16x4_f64, each lane forming its g straight
//     into the A operand; S_g and S_gg on the VALU beside it.
// With more than one chunk the waves write partial sums [n_chunks][...] and ccf_combine_kernel
// adds them in ascending chunk order; with one chunk they write the results.  Every (atmosphere,
// exposure, velocity) has its own accumulator and, for a given form, its order of summation
// depends on n_pix alone: results are bitwise the same from call to call, for a row alone, for
// any subset of the exposures or velocities and whichever outputs are asked for.  No atomics, no
// LDS, no barrier; g's three operations are not contracted (-ffp-contract=off), the
// accumulations are explicit fma.  Rows, velocities and exposures past the end of a tile alias
// the tile's first (read, never stored).
#include <cmath>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

struct frei_ccf {
  Stream stream;   // first: destroyed last
  int device = 0;
  int64_t n_lam = 0, n_pix = 0;
  int n_vel = 0, n_exp = 0, e_pad = 0;
  int64_t p_pad = 0;          // n_pix rounded up to 16: the plan's row pitch; pads are zeros
  DevBuf<int32_t> d_idx;   // [n_vel][p_pad]
  DevBuf<double> d_frac;   // [n_vel][p_pad]
  DevBuf<double> d_a;      // [n_exp][n_pix]  (form 1: coalesced along the pixels)
  DevBuf<double> d_at;     // [p_pad][e_pad]  (form 2: an MFMA step's 16 exposures contiguous)
  DevBuf<double> d_w;      // [p_pad]
  // keep mode (frei_ccf_keep): the last successful apply's sums stay here for frei_stack_apply
  bool keep = false;
  DevBuf<double> k_sfg, k_sg, k_sgg;
  int k_atm = 0;
  ~frei_ccf() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

namespace {

constexpr int kChunk = 4096;  // pixels per chunk (frei_amd.crosscorr.PIXEL_CHUNK)
constexpr int kAT = 2;        // atmospheres per wave
constexpr int kVT = 2;        // velocities per wave
constexpr int kET = 8;        // exposures per wave
constexpr int kWaves = 4;     // waves (velocity tiles) per block
constexpr int kEPad = 16;     // aT's rows are padded to whole MFMA exposure blocks (and kET)
// form 0: form 2 from this many exposures.  Measured on MI355X (tools/crosscorr_probe.py, 8
// atmospheres x 101 velocities x 40 960 pixels, the forms taking turns over 7 rounds;
// profiles/r11/crosscorr/README.md), VALU against MFMA form, median ms: 0.166 / 0.191 at 1
// exposure, 0.166 / 0.191 at 4, 0.170 / 0.191 at 8, 0.233 / 0.192 at 16, 0.289 / 0.237 at 20,
// 0.292 / 0.236 at 24, 0.353 / 0.237 at 32 (run-to-run spread below 3 %).  The VALU form steps
// up with every tile of 8 exposures, the MFMA form with every block of 16; they cross where the
// VALU form takes its second tile.
constexpr int kMfmaFromExposures = 9;

struct CcfArgs {
  const double* y;        // row m at y + m * ys
  int64_t ys;
  const int32_t* idx;
  const double* frac;
  const double* ap;       // a [n_exp][n_pix]
  const double* at;       // aT [p_pad][e_pad]
  const double* w;
  int64_t n_pix, p_pad;
  int n_vel, n_exp, e_pad, n_atm;
  int e_tiles;            // exposure tiles per chunk in blockIdx.y
  // outputs of chunk c at sfg + c * fg_size, sg / sgg + c * g_size (one chunk: the results)
  int64_t fg_size, g_size;
  double *sfg, *sg, *sgg;
};

// y = scale (x / den) - offset; an absent operand drops its operation.
__global__ __launch_bounds__(256) void ccf_template_kernel(
    const double* __restrict__ x, int64_t xs, const double* __restrict__ den,
    const int32_t* __restrict__ select, const double* __restrict__ scale,
    const double* __restrict__ offset, int64_t n, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int m = blockIdx.y;
  if (i >= n) return;
  double v = x[(int64_t)m * xs + i];
  if (den) v = v / den[(select ? (int64_t)select[m] : 0) * n + i];
  if (scale) v = scale[m] * v;
  if (offset) v = v - offset[m];
  y[(int64_t)m * n + i] = v;
}

// The wave's tile: velocities v[], template rows yr[]; false when the wave has no velocity.
__device__ __forceinline__ bool wave_tile(const CcfArgs& a, int (&v)[kVT],
                                          const double* (&yr)[kAT], int& nv, int& nr) {
  const int wv = threadIdx.x >> 6;
  const int v0 = (blockIdx.z * kWaves + wv) * kVT;
  if (v0 >= a.n_vel) return false;
  nv = min(kVT, a.n_vel - v0);
  const int r0 = blockIdx.x * kAT;
  nr = min(kAT, a.n_atm - r0);
#pragma unroll
  for (int q = 0; q < kVT; ++q) v[q] = v0 + (q < nv ? q : 0);
#pragma unroll
  for (int r = 0; r < kAT; ++r) yr[r] = a.y + (int64_t)(r0 + (r < nr ? r : 0)) * a.ys;
  return true;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = x + __shfl_xor(x, o);
  return x;
}

// form 1.  STATS false: S_fg of one (chunk, exposure tile) per wave, blockIdx.y = chunk *
// e_tiles + tile; STATS true: S_g and S_gg of one chunk, blockIdx.y = chunk.  A lane takes two
// pixels per turn (l + 128 i, then l + 128 i + 64: its pixels in ascending order) with the loads
// of both in flight together and the plan entries of the next turn fetched a turn ahead, so the
// dependent chain plan -> template gather is off the critical path.  Pixels past the chunk's end
// enter as g = 0, a = 0, w = 0.
template <bool STATS>
__global__ __launch_bounds__(64 * kWaves) void ccf_valu_kernel(const CcfArgs a) {
  int v[kVT], nv, nr;
  const double* yr[kAT];
  if (!wave_tile(a, v, yr, nv, nr)) return;   // a whole wave; the kernel has no barrier
  const int lane = threadIdx.x & 63;
  const int c = STATS ? blockIdx.y : blockIdx.y / a.e_tiles;
  const int e0 = STATS ? 0 : (blockIdx.y % a.e_tiles) * kET;   // e0 + kET <= e_pad
  const int64_t lo = (int64_t)c * kChunk, hi = min(lo + (int64_t)kChunk, a.n_pix);
  const bool want_g = a.sg != nullptr, want_gg = a.sgg != nullptr;   // uniform
  constexpr int NE = STATS ? 2 : kET;
  double acc[kAT][kVT][NE];
#pragma unroll
  for (int r = 0; r < kAT; ++r)
#pragma unroll
    for (int q = 0; q < kVT; ++q)
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[r][q][e] = 0.0;
  int jn[2][kVT];
  double tn[2][kVT];
  auto plan = [&](int64_t p) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t pu = min(p + 64 * u, hi - 1);   // loads stay inside the arrays
#pragma unroll
      for (int q = 0; q < kVT; ++q) {
        const int64_t k = (int64_t)v[q] * a.p_pad + pu;
        jn[u][q] = a.idx[k];
        tn[u][q] = a.frac[k];
      }
    }
  };
  plan(lo + lane);
  for (int64_t p = lo + lane; p < hi; p += 128) {
    int j[2][kVT];
    double t[2][kVT], y0[2][kAT][kVT], y1[2][kAT][kVT], f[2][STATS ? 1 : kET];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < kVT; ++q) {
        j[u][q] = jn[u][q];
        t[u][q] = tn[u][q];
#pragma unroll
        for (int r = 0; r < kAT; ++r) {
          y0[u][r][q] = yr[r][j[u][q]];
          y1[u][r][q] = yr[r][j[u][q] + 1];
        }
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t pu = min(p + 64 * u, hi - 1);
      if (STATS) {
        f[u][0] = a.w[pu];
      } else {
#pragma unroll
        for (int e = 0; e < (STATS ? 1 : kET); ++e)   // exposures past n_exp alias the last
          f[u][e] = a.ap[(int64_t)min(e0 + e, a.n_exp - 1) * a.n_pix + pu];
      }
    }
    plan(p + 128);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bool ok = p + 64 * u < hi;
#pragma unroll
      for (int r = 0; r < kAT; ++r)
#pragma unroll
        for (int q = 0; q < kVT; ++q) {
          // g: three operations, not contracted
          const double d = y1[u][r][q] - y0[u][r][q];
          const double td = t[u][q] * d;
          const double g = ok ? y0[u][r][q] + td : 0.0;
          if (STATS) {
            const double w = ok ? f[u][0] : 0.0;
            if (want_g) acc[r][q][0] = fma(w, g, acc[r][q][0]);
            if (want_gg) {
              const double wg = w * g;
              acc[r][q][1] = fma(wg, g, acc[r][q][1]);
            }
          } else {
#pragma unroll
            for (int e = 0; e < (STATS ? 0 : kET); ++e)
              acc[r][q][e] = fma(ok ? f[u][e] : 0.0, g, acc[r][q][e]);
          }
        }
    }
  }
#pragma unroll
  for (int r = 0; r < kAT; ++r)
#pragma unroll
    for (int q = 0; q < kVT; ++q)
#pragma unroll
      for (int e = 0; e < NE; ++e)
        if (!STATS || (e == 0 ? want_g : want_gg)) acc[r][q][e] = wave_sum(acc[r][q][e]);
  if (lane != 0) return;
  const int r0 = blockIdx.x * kAT;
  if (STATS) {
#pragma unroll
    for (int r = 0; r < kAT; ++r)
#pragma unroll
      for (int q = 0; q < kVT; ++q)
        if (r < nr && q < nv) {
          const int64_t o = (int64_t)c * a.g_size + (int64_t)(r0 + r) * a.n_vel + v[q];
          if (want_g) a.sg[o] = acc[r][q][0];
          if (want_gg) a.sgg[o] = acc[r][q][1];
        }
  } else {
    const int ne = min(kET, a.n_exp - e0);
#pragma unroll
    for (int r = 0; r < kAT; ++r)
#pragma unroll
      for (int q = 0; q < kVT; ++q)
#pragma unroll
        for (int e = 0; e < NE; ++e)
          if (r < nr && q < nv && e < ne)
            a.sfg[(int64_t)c * a.fg_size +
                  ((int64_t)(r0 + r) * a.n_exp + e0 + e) * a.n_vel + v[q]] = acc[r][q][e];
  }
}

// form 2: S_fg on the fp64 matrix cores, v_mfma_f64_16x16x4_f64 (operand maps as in K7,
// frei_kernels.hip contract_batch_kernel): A = 16 velocities x 4 pixels of one atmosphere — lane
// l forms the g of velocity l & 15 at pixel l >> 4 of the step straight into its A operand —,
// B = 4 pixels x 16 exposures from aT (lane l: pixel l >> 4, exposure l & 15), D = 16 velocities
// x 16 exposures (lane l: velocities (l >> 4) + 4 r, exposure l & 15).  One wave per (atmosphere,
// 16 velocities, chunk, NB exposure blocks of 16), blockIdx.y = chunk * e_tiles + tile, the four
// waves of a block on four consecutive atmospheres (plan and data shared in L1); A is reused for
// the NB blocks.  S_g and S_gg accumulate on the VALU beside it (the waves of exposure tile 0;
// fma, in the lane's pixel order) and combine over the four pixel lanes of a velocity as
// (k0 + k1) + (k2 + k3) (xor 16, then 32).  The pixels go in groups of 16 (four MFMA steps) whose
// loads are all issued before the first use, the plan entries a group ahead.  Lane (velocity,
// k) holds the pixels p0 + 4 k + s of the group at p0, so step s multiplies the pixels p0 + s,
// p0 + 4 + s, p0 + 8 + s, p0 + 12 + s; pixels past n_pix enter as g = 0, a = 0, w = 0.  NB = 0:
// the statistics alone.
typedef double dbl4 __attribute__((ext_vector_type(4)));
typedef int int4v __attribute__((ext_vector_type(4)));

template <int NB, bool STATS>
__global__ __launch_bounds__(256) void ccf_mfma_kernel(const CcfArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int m = blockIdx.x * 4 + wv;
  if (m >= a.n_atm) return;                    // a whole wave; the kernel has no barrier
  const int row = lane & 15, kq = lane >> 4;
  const int v0 = blockIdx.z * 16;
  const int v = v0 + row < a.n_vel ? v0 + row : v0;
  const int c = blockIdx.y / a.e_tiles, tile = blockIdx.y % a.e_tiles;
  const int64_t lo = (int64_t)c * kChunk, hi = min(lo + (int64_t)kChunk, a.n_pix);
  const int cb = a.e_pad / 16;                 // exposure blocks there are
  const bool stats = STATS && tile == 0;       // uniform
  const bool want_g = a.sg != nullptr, want_gg = a.sgg != nullptr;
  const double* __restrict__ yr = a.y + (int64_t)m * a.ys;
  const int32_t* __restrict__ ip = a.idx + (int64_t)v * a.p_pad;
  const double* __restrict__ fp = a.frac + (int64_t)v * a.p_pad;
  int boff[NB > 0 ? NB : 1];                   // this lane's column of each exposure block
#pragma unroll
  for (int q = 0; q < NB; ++q) boff[q] = min(tile * NB + q, cb - 1) * 16 + row;
  dbl4 acc[NB > 0 ? NB : 1];
#pragma unroll
  for (int q = 0; q < NB; ++q) acc[q] = dbl4{0.0, 0.0, 0.0, 0.0};
  double ag = 0.0, agg = 0.0;
  // lane (row, kq) holds the pixels p0 + 4 kq + s, s = 0 .. 3, of a group: its four plan
  // entries are one 16-byte and one 32-byte load (rows are pitched to 16 pixels, pads zero)
  const int64_t last = (hi - 1) / 16 * 16;     // the chunk's last group
  int4v jn;
  dbl4 tn;
  auto plan = [&](int64_t p0) {
    const int64_t k = min(p0, last) + 4 * kq;
    jn = *reinterpret_cast<const int4v*>(ip + k);
    tn = *reinterpret_cast<const dbl4*>(fp + k);
  };
  plan(lo);
  for (int64_t p0 = lo; p0 < hi; p0 += 16) {
    const int64_t pl = p0 + 4 * kq;
    const int4v j = jn;
    const dbl4 t = tn;
    double y0[4], y1[4], bv[4][NB > 0 ? NB : 1];
    dbl4 wp;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      y0[s] = yr[j[s]];
      y1[s] = yr[j[s] + 1];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < NB; ++q) bv[s][q] = a.at[(pl + s) * a.e_pad + boff[q]];
    if (stats) wp = *reinterpret_cast<const dbl4*>(a.w + pl);
    plan(p0 + 16);
    double g[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double d = y1[s] - y0[s];
      const double td = t[s] * d;
      g[s] = pl + s < hi ? y0[s] + td : 0.0;   // a and w are zero past n_pix
#pragma unroll
      for (int q = 0; q < NB; ++q)
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(g[s], bv[s][q], acc[q], 0, 0, 0);
    }
    if (stats) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (want_g) ag = fma(wp[s], g[s], ag);
        if (want_gg) {
          const double wg = wp[s] * g[s];
          agg = fma(wg, g[s], agg);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int e = (tile * NB + q) * 16 + row;
    if (tile * NB + q >= cb || e >= a.n_exp) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int vr = v0 + kq + 4 * r;
      if (vr < a.n_vel)
        a.sfg[(int64_t)c * a.fg_size + ((int64_t)m * a.n_exp + e) * a.n_vel + vr] = acc[q][r];
    }
  }
  if (stats) {
    if (want_g) {
      ag = ag + __shfl_xor(ag, 16);
      ag = ag + __shfl_xor(ag, 32);
    }
    if (want_gg) {
      agg = agg + __shfl_xor(agg, 16);
      agg = agg + __shfl_xor(agg, 32);
    }
    if (kq == 0 && v0 + row < a.n_vel) {
      const int64_t o = (int64_t)c * a.g_size + (int64_t)m * a.n_vel + v0 + row;
      if (want_g) a.sg[o] = ag;
      if (want_gg) a.sgg[o] = agg;
    }
  }
}

template <bool STATS>
void launch_mfma(int nb, dim3 grid, const CcfArgs& a, hipStream_t st) {
  switch (nb) {
    case 0: ccf_mfma_kernel<0, STATS><<<grid, 256, 0, st>>>(a); break;
    case 1: ccf_mfma_kernel<1, STATS><<<grid, 256, 0, st>>>(a); break;
    case 2: ccf_mfma_kernel<2, STATS><<<grid, 256, 0, st>>>(a); break;
    case 3: ccf_mfma_kernel<3, STATS><<<grid, 256, 0, st>>>(a); break;
    default: ccf_mfma_kernel<4, STATS><<<grid, 256, 0, st>>>(a); break;
  }
}

// The chunks' partial sums part[n_chunks][n] added in ascending chunk order.
__global__ __launch_bounds__(256) void ccf_combine_kernel(const double* __restrict__ part,
                                                          int n_chunks, int64_t n,
                                                          double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = part[i];
  for (int c = 1; c < n_chunks; ++c) s = s + part[(int64_t)c * n + i];
  out[i] = s;
}

std::string at2(const char* name, int64_t i, int64_t k) {
  return std::string(name) + "[" + std::to_string(i) + "][" + std::to_string(k) + "]";
}

// What keep mode left ends here (the stream is idle: every apply ends synchronised).
void drop_kept(frei_ccf* c) {
  if (c->k_sfg || c->k_sg || c->k_sgg) (void)hipSetDevice(c->device);
  c->k_sfg.reset();
  c->k_sg.reset();
  c->k_sgg.reset();
  c->k_atm = 0;
}

}  // namespace

namespace frei {
int ccf_kept_sums(frei_ccf* c, CcfKept* out) {
  if (!c) return set_error("null correlator");
  *out = CcfKept{c->k_sfg, c->k_sg, c->k_sgg, c->k_atm, c->n_exp, c->n_vel, c->device};
  return 0;
}
}  // namespace frei

// ==================================================================== C ABI
extern "C" {

int frei_ccf_create(frei_ccf** out, int device, int64_t n_lam, int64_t n_pix, int n_vel,
                    const int32_t* idx, const double* frac, int n_exp, const double* a,
                    const double* w) {
  // plan, data and weights are validated on the host before any device call
  if (!out || !idx || !frac || !a || !w) return set_error("null argument");
  *out = nullptr;
  if (n_lam < 2) return set_error("frei_ccf_create: n_lam must be >= 2");
  if (n_lam > INT32_MAX) return set_error("frei_ccf_create: n_lam exceeds the int32 plan");
  if (n_pix < 1) return set_error("frei_ccf_create: n_pix must be >= 1");
  if (n_vel < 1) return set_error("frei_ccf_create: n_vel must be >= 1");
  if (n_exp < 1) return set_error("frei_ccf_create: n_exp must be >= 1");
  for (int v = 0; v < n_vel; ++v)
    for (int64_t p = 0; p < n_pix; ++p) {
      const int64_t k = (int64_t)v * n_pix + p;
      if (idx[k] < 0 || idx[k] > n_lam - 2)
        return set_error("frei_ccf_create: " + at2("idx", v, p) + " = " +
                         std::to_string(idx[k]) + " lies outside [0, n_lam - 2 = " +
                         std::to_string(n_lam - 2) + "]");
      if (!std::isfinite(frac[k]) || frac[k] < 0.0 || frac[k] > 1.0)
        return set_error("frei_ccf_create: " + at2("frac", v, p) + " lies outside [0, 1]");
    }
  for (int e = 0; e < n_exp; ++e)
    for (int64_t p = 0; p < n_pix; ++p)
      if (!std::isfinite(a[(int64_t)e * n_pix + p]))
        return set_error("frei_ccf_create: " + at2("a", e, p) + " is not finite");
  double sum = 0.0;
  for (int64_t p = 0; p < n_pix; ++p) {
    if (!std::isfinite(w[p]) || w[p] < 0.0)
      return set_error("frei_ccf_create: w[" + std::to_string(p) +
                       "] is negative or not finite");
    sum += w[p];
  }
  if (!(sum > 0.0)) return set_error("frei_ccf_create: the weights w sum to zero");

  const int e_pad = (n_exp + kEPad - 1) / kEPad * kEPad;
  const int64_t p_pad = (n_pix + 15) / 16 * 16;
  const size_t np = (size_t)n_vel * (size_t)p_pad;
  std::vector<int32_t> idx_p(np, 0);
  std::vector<double> frac_p(np, 0.0), at((size_t)p_pad * e_pad, 0.0), w_p((size_t)p_pad, 0.0);
  for (int v = 0; v < n_vel; ++v)
    for (int64_t p = 0; p < n_pix; ++p) {
      idx_p[(size_t)v * p_pad + p] = idx[(int64_t)v * n_pix + p];
      frac_p[(size_t)v * p_pad + p] = frac[(int64_t)v * n_pix + p];
    }
  for (int e = 0; e < n_exp; ++e)
    for (int64_t p = 0; p < n_pix; ++p) at[(size_t)p * e_pad + e] = a[(int64_t)e * n_pix + p];
  for (int64_t p = 0; p < n_pix; ++p) w_p[p] = w[p];
  frei_ccf* c = new frei_ccf();
  c->device = device;
  c->n_lam = n_lam;
  c->n_pix = n_pix;
  c->p_pad = p_pad;
  c->n_vel = n_vel;
  c->n_exp = n_exp;
  c->e_pad = e_pad;
  const size_t na = (size_t)n_exp * (size_t)n_pix;
  if (hipSetDevice(device) != hipSuccess || c->stream.create() || c->d_idx.alloc(np) ||
      c->d_frac.alloc(np) || c->d_a.alloc(na) || c->d_at.alloc(at.size()) ||
      c->d_w.alloc(w_p.size())) {
    delete c;
    (void)hipGetLastError();
    return set_error("frei_ccf_create: device allocation failed");
  }
  if (hipMemcpy(c->d_idx, idx_p.data(), np * sizeof(int32_t), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(c->d_frac, frac_p.data(), np * sizeof(double), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(c->d_a, a, na * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_at, at.data(), at.size() * sizeof(double), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(c->d_w, w_p.data(), w_p.size() * sizeof(double), hipMemcpyHostToDevice) !=
          hipSuccess) {
    delete c;
    (void)hipGetLastError();
    return set_error("frei_ccf_create: host-to-device copy failed");
  }
  *out = c;
  return 0;
}

int frei_ccf_destroy(frei_ccf* c) {
  if (c) delete c;
  return 0;
}

// The five sources of x — a host array, a context's emergent rows, a broadener's kept result
// (K13), an interpolator's (K15), a phase integrator's (K16) — feed the same src and stride below.
static int ccf_apply_impl(frei_ccf* c, frei_ctx* ctx, const double* x, frei_brd* brd,
                          frei_itp* itp, frei_phs* phs, int n_atm, const double* den, int n_lib,
                          const int32_t* select, const double* scale, const double* offset, int form, double* sfg,
                          double* sg, double* sgg, int* form_used, double* kernel_ms) {
  if (!c) return set_error("frei_ccf_apply: null handle");
  if (!sfg && !sg && !sgg && !c->keep)
    return set_error("frei_ccf_apply: sfg, sg and sgg are all null");
  // the sums to compute: those asked for; in keep mode with none asked for, all three
  const bool all = !sfg && !sg && !sgg;
  const bool w_fg = sfg || all, w_g = sg || all, w_gg = sgg || all;
  if (!x && !ctx && !brd && !itp && !phs)
    return set_error("frei_ccf_apply: x and ctx are both null");
  if (n_atm < 1) return set_error("frei_ccf_apply: n_atm must be >= 1");
  if (form < 0 || form > 2)
    return set_error("frei_ccf_apply: form must be 0 (automatic), 1 (VALU) or 2 (fp64 MFMA)");
  if (den && n_lib < 1) return set_error("frei_ccf_apply: n_lib must be >= 1 with den");
  if (den) TRY(check_select("frei_ccf_apply", select, n_atm, n_lib));
  SpectrumRows rows;
  TRY(spectrum_rows(x, ctx, brd, itp, phs, n_atm, c->n_lam, c->device, c->stream, "correlator",
                    "frei_ccf_apply", &rows));
  int f = form;
  if (f == 0) f = c->n_exp >= kMfmaFromExposures ? 2 : 1;
  if (form_used) *form_used = f;

  HIP_TRY(hipSetDevice(c->device));
  drop_kept(c);   // what an earlier call kept ends here, whether or not this call succeeds
  hipStream_t st = rows.stream;
  const size_t A = (size_t)n_atm, n = (size_t)c->n_lam, V = (size_t)c->n_vel,
               E = (size_t)c->n_exp;
  const bool prepass = den || scale || offset;
  const int nc = (int)((c->n_pix + kChunk - 1) / kChunk);   // chunks: partial sums beyond one
  if ((int64_t)nc * ((c->n_exp + kET - 1) / kET) > 65535)
    return set_error("frei_ccf_apply: n_pix / 4096 * n_exp / 8 exceeds the launch grid");
  DeviceCall call(st, "cross-correlation");
  auto result = [&](bool want, size_t cnt) { return want ? call.alloc<double>(cnt) : nullptr; };
  const double* u_x = call.upload(x, A * n);
  const double* d_den = call.upload(den, (size_t)n_lib * n);
  const int32_t* d_sel = call.upload(den ? select : nullptr, A);
  const double* d_scale = call.upload(scale, A);
  const double* d_off = call.upload(offset, A);
  double* d_y = result(prepass, A * n);
  double* d_sfg = result(w_fg, A * E * V);
  double* d_sg = result(w_g, A * V);
  double* d_sgg = result(w_gg, A * V);
  double* p_sfg = result(nc > 1 && w_fg, (size_t)nc * A * E * V);
  double* p_sg = result(nc > 1 && w_g, (size_t)nc * A * V);
  double* p_sgg = result(nc > 1 && w_gg, (size_t)nc * A * V);
  call.begin(kernel_ms);
  if (call.ok()) {
    const double* src = u_x ? u_x : rows.rows;
    const int64_t xs = rows.stride;
    if (prepass)
      ccf_template_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)n_atm), 256, 0, st>>>(
          src, xs, d_den, d_sel, d_scale, d_off, c->n_lam, d_y);
    // the atmosphere tiles are blockIdx.x: blocks that run together share plan and data in L2
    CcfArgs a;
    a.y = prepass ? d_y : src;
    a.ys = prepass ? (int64_t)n : xs;
    a.idx = c->d_idx;
    a.frac = c->d_frac;
    a.ap = c->d_a;
    a.at = c->d_at;
    a.p_pad = c->p_pad;
    a.w = c->d_w;
    a.n_pix = c->n_pix;
    a.n_vel = c->n_vel;
    a.n_exp = c->n_exp;
    a.e_pad = c->e_pad;
    a.n_atm = n_atm;
    a.fg_size = (int64_t)(A * E * V);
    a.g_size = (int64_t)(A * V);
    a.sfg = nc > 1 ? p_sfg : d_sfg;
    a.sg = nc > 1 ? p_sg : d_sg;
    a.sgg = nc > 1 ? p_sgg : d_sgg;
    const unsigned bx = (unsigned)((c->n_vel + kVT * kWaves - 1) / (kVT * kWaves));
    const unsigned bz = (unsigned)((n_atm + kAT - 1) / kAT);
    if (f == 1) {
      a.e_tiles = (c->n_exp + kET - 1) / kET;
      if (w_fg)
        ccf_valu_kernel<false><<<dim3(bz, (unsigned)(nc * a.e_tiles), bx), 64 * kWaves, 0, st>>>(a);
      if (w_g || w_gg)
        ccf_valu_kernel<true><<<dim3(bz, (unsigned)nc, bx), 64 * kWaves, 0, st>>>(a);
    } else {
      // exposure blocks of 16 spread evenly over the fewest tiles of at most 4
      const int cb = w_fg ? c->e_pad / 16 : 0, ty = (cb + 3) / 4;
      const int nb = ty ? (cb + ty - 1) / ty : 0;
      a.e_tiles = ty ? ty : 1;
      const dim3 grid((unsigned)((n_atm + 3) / 4), (unsigned)(nc * a.e_tiles),
                      (unsigned)((c->n_vel + 15) / 16));
      if (w_g || w_gg) launch_mfma<true>(nb, grid, a, st);
      else launch_mfma<false>(nb, grid, a, st);
    }
    if (nc > 1) {
      auto combine = [&](const double* part, int64_t cnt, double* out) {
        if (out)
          ccf_combine_kernel<<<dim3((unsigned)((cnt + 255) / 256)), 256, 0, st>>>(part, nc, cnt,
                                                                                 out);
      };
      combine(p_sfg, a.fg_size, d_sfg);
      combine(p_sg, a.g_size, d_sg);
      combine(p_sgg, a.g_size, d_sgg);
    }
  }
  call.end();
  call.download(sfg, d_sfg, A * E * V);
  call.download(sg, d_sg, A * V);
  call.download(sgg, d_sgg, A * V);
  if (c->keep) {
    call.keep(d_sfg);
    call.keep(d_sg);
    call.keep(d_sgg);
  }
  const int rc = call.finish();
  if (!rc && c->keep) {   // complete: finish() synchronised the stream
    c->k_sfg.adopt(d_sfg, A * E * V);
    c->k_sg.adopt(d_sg, A * V);
    c->k_sgg.adopt(d_sgg, A * V);
    c->k_atm = n_atm;
  }
  return rc;
}

int frei_ccf_apply(frei_ccf* c, frei_ctx* ctx, const double* x, int n_atm, const double* den,
                   int n_lib, const int32_t* select, const double* scale, const double* offset,
                   int form, double* sfg, double* sg, double* sgg, int* form_used,
                   double* kernel_ms) {
  return ccf_apply_impl(c, ctx, x, nullptr, nullptr, nullptr, n_atm, den, n_lib, select, scale,
                        offset, form, sfg, sg, sgg, form_used, kernel_ms);
}

int frei_ccf_keep(frei_ccf* c, int on) {
  if (!c) return set_error("frei_ccf_keep: null handle");
  c->keep = on != 0;
  if (!c->keep) drop_kept(c);
  return 0;
}

int frei_ccf_apply_brd(frei_ccf* c, frei_brd* src, int n_atm, const double* den, int n_lib,
                       const int32_t* select, const double* scale, const double* offset,
                       int form, double* sfg, double* sg, double* sgg, int* form_used,
                       double* kernel_ms) {
  if (!src) return set_error("frei_ccf_apply_brd: null broadener");
  return ccf_apply_impl(c, nullptr, nullptr, src, nullptr, nullptr, n_atm, den, n_lib, select,
                        scale, offset, form, sfg, sg, sgg, form_used, kernel_ms);
}

int frei_ccf_apply_itp(frei_ccf* c, frei_itp* src, int n_atm, const double* den, int n_lib,
                       const int32_t* select, const double* scale, const double* offset,
                       int form, double* sfg, double* sg, double* sgg, int* form_used,
                       double* kernel_ms) {
  if (!src) return set_error("frei_ccf_apply_itp: null interpolator");
  return ccf_apply_impl(c, nullptr, nullptr, nullptr, src, nullptr, n_atm, den, n_lib, select,
                        scale, offset, form, sfg, sg, sgg, form_used, kernel_ms);
}

int frei_ccf_apply_phs(frei_ccf* c, frei_phs* src, int n_atm, const double* den, int n_lib,
                       const int32_t* select, const double* scale, const double* offset,
                       int form, double* sfg, double* sg, double* sgg, int* form_used,
                       double* kernel_ms) {
  if (!src) return set_error("frei_ccf_apply_phs: null phase integrator");
  return ccf_apply_impl(c, nullptr, nullptr, nullptr, nullptr, src, n_atm, den, n_lib, select,
                        scale, offset, form, sfg, sg, sgg, form_used, kernel_ms);
}

}  // extern "C"
