// frei_kdist.hip — K18: correlated-k tables.  frei_xsec_mix premixes several species' resident
// cross-sections into one (a plain stream), and frei_xsec_kdist / frei_set_table_kdist sort the
// points of every wavelength bin of a resident cross-section into a monotone k(g) and sample it at
// a few quadrature points g_q (the definitions are in include/frei_hip.h).  No reference
// counterpart: the projects this engine's physics follows give their line-by-line calculator this
// second output (HELIOS-K's k-distribution for HELIOS).
//
// Bin membership and the source node of each target node are K6's (bin_ranges, source_rows:
// frei_binning.hip).  The sampling plan (j, f per (bin size, g_q)) is built here on the host in
// fp64, so that the NumPy restatement shares it to the bit.
//
// Kernels: every float32 becomes an order-preserving uint32 key (-0 -> +0, every NaN the
// canonical quiet NaN, which sorts last as in np.sort), a (source row, bin) pair's keys are sorted
// ascending, then n_g lanes gather s_j and s_{j+1}, interpolate and store the value to every
// destination row that selected the source row.  Two forms, by bin size:
//   block: one block per (row, bin); the keys are loaded coalesced into LDS, padded to a power of
//     two P with 0xFFFFFFFF (above every key) and sorted in place by a bitonic network, whose
//     steps of stride below 64 run on cross-lane exchanges instead of LDS.  Bins are
//     launched by P class, with P * 4 bytes of dynamic LDS and min(1024, max(64, P / 2)) lanes, so
//     a launch of small bins keeps several blocks per CU; P <= 32768 (128 KiB of the 160 KiB LDS);
//   wave: bins of at most 64 points, one wave per (row, bin) and four per block; each lane holds
//     one key, the network runs on cross-lane exchanges and the gather on lane reads (no LDS).
// Sorting is exact and the sample is one fixed expression, so both forms give the same bits.
// A merge pass for bins wider than 32768 points is out of scope: such a bin is an error.
// HBM traffic: the selected source rows once (4 B per point) and the table once (8 B per value).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

namespace {

constexpr int kMaxBin = 32768;   // points of the widest bin (its keys: 128 KiB of LDS)
constexpr int kWaveBin = 64;     // points of the widest bin of the wave form

struct KdBin {
  int64_t start;   // first point of the bin on the axis
  int32_t n;       // its points
  int32_t plan;    // row of the sampling plan (one per distinct n)
  int64_t bin;     // the bin's index: its columns are [bin * n_g, (bin + 1) * n_g)
};

// float32 -> uint32 whose unsigned order is np.sort's: -0 -> +0, any NaN -> 0x7FC00000 (last).
__device__ __forceinline__ uint32_t key_of(float v) {
  uint32_t b = __float_as_uint(v);
  if (v != v) b = 0x7FC00000u;
  if (v == 0.0f) b = 0u;
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ double value_of(uint32_t k) {
  return (double)__uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// k = s_j + f (s_{j+1} - s_j), unfused (the build sets -ffp-contract=off)
__device__ __forceinline__ double sample(double a, double b, double f) { return a + f * (b - a); }

// One compare-exchange of the bitonic network across lanes: lane ^ j holds the partner.
__device__ __forceinline__ uint32_t exchange(uint32_t key, int j, bool keep_min) {
  const uint32_t other = __shfl_xor(key, j);
  return keep_min ? min(key, other) : max(key, other);
}

// Column `q` of bin `b` to every destination row of source row u, when the slice holds it.
__device__ __forceinline__ void fan_store(double v, const KdBin& b, int q, int n_g, int u,
                                          const int32_t* __restrict__ fan_off,
                                          const int64_t* __restrict__ fan_dst, int64_t col_lo,
                                          int64_t n_out, double* __restrict__ out) {
  const int64_t c = b.bin * n_g + q - col_lo;
  if (c < 0 || c >= n_out) return;
  for (int f = fan_off[u]; f < fan_off[u + 1]; ++f)
    __builtin_nontemporal_store(v, out + fan_dst[f] + c);   // streaming: written once
}

// block form: block blockIdx.x = u * nb + (bin of the launch), keys[P] in dynamic LDS.
__global__ __launch_bounds__(1024) void kdist_block_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ row_off, const KdBin* __restrict__ bins,
    int nb, int P, const int32_t* __restrict__ pj, const double* __restrict__ pf, int n_g,
    const int32_t* __restrict__ fan_off, const int64_t* __restrict__ fan_dst, int64_t col_lo,
    int64_t n_out, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t keys[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int u = blockIdx.x / nb;
  const KdBin b = bins[blockIdx.x - u * nb];
  const float* src = x + row_off[u] + b.start;
  // The network's steps of stride j < 64 stay inside an aligned run of 64 keys: a wave takes the
  // run one key per lane and does them on cross-lane exchanges, as the wave form does (no LDS
  // traffic, no barrier between them).  First every phase k <= 64 while the keys are loaded, then
  // per phase k >= 128 the strides k/2 .. 64 in LDS with a barrier each and 32 .. 1 in one pass.
  const int lane = tid & 63;
  for (int i = tid; i < P; i += nt) {   // nt and P are multiples of 64: whole waves, whole runs
    uint32_t key = i < b.n ? key_of(src[i]) : 0xFFFFFFFFu;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1)
        key = exchange(key, j, ((lane & j) == 0) == ((i & k) == 0));
    keys[i] = key;
  }
  __syncthreads();
  for (int k = 128; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= 64; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += nt) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // bit j clear
        const int l = i | j;
        const uint32_t a = keys[i], c = keys[l];
        if ((a > c) == ((i & k) == 0)) {
          keys[i] = c;
          keys[l] = a;
        }
      }
      __syncthreads();
    }
    for (int i = tid; i < P; i += nt) {
      uint32_t key = keys[i];
#pragma unroll
      for (int j = 32; j > 0; j >>= 1)
        key = exchange(key, j, ((lane & j) == 0) == ((i & k) == 0));
      keys[i] = key;
    }
    __syncthreads();
  }
  if (tid < n_g) {
    double v = __builtin_nan("");
    if (b.n == 1) {
      v = value_of(keys[0]);
    } else if (b.n > 1) {
      const int j = pj[b.plan * n_g + tid];
      v = sample(value_of(keys[j]), value_of(keys[j + 1]), pf[b.plan * n_g + tid]);
    }
    fan_store(v, b, tid, n_g, u, fan_off, fan_dst, col_lo, n_out, out);
  }
}

// wave form: wave (blockIdx.x * 4 + wave of the block) = u * nb + (bin of the launch), n <= 64.
__global__ __launch_bounds__(256) void kdist_wave_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ row_off, const KdBin* __restrict__ bins,
    int nb, int n_pairs, const int32_t* __restrict__ pj, const double* __restrict__ pf, int n_g,
    const int32_t* __restrict__ fan_off, const int64_t* __restrict__ fan_dst, int64_t col_lo,
    int64_t n_out, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  // (wave-uniform by construction: said so, the row and bin records come through scalar loads;
  // n_pairs < 2^31 is checked on the host)
  const unsigned w = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= (unsigned)n_pairs) return;   // wave-uniform; the kernel has no barrier
  const int u = (int)(w / (unsigned)nb);
  const KdBin b = bins[w - (unsigned)u * (unsigned)nb];
  uint32_t key = lane < b.n ? key_of(x[row_off[u] + b.start + lane]) : 0xFFFFFFFFu;
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1)
      key = exchange(key, j, ((lane & j) == 0) == ((lane & k) == 0));
  // every lane takes part in the lane reads; lanes >= n_g read lane 0
  const bool act = lane < n_g;
  const int j = (act && b.n > 1) ? pj[b.plan * n_g + lane] : 0;
  const uint32_t k0 = __shfl(key, j), k1 = __shfl(key, j + 1);
  if (!act) return;
  double v = __builtin_nan("");
  if (b.n == 1) v = value_of(k0);
  else if (b.n > 1) v = sample(value_of(k0), value_of(k1), pf[b.plan * n_g + lane]);
  fan_store(v, b, lane, n_g, u, fan_off, fan_dst, col_lo, n_out, out);
}

// premix: lane q takes points [4 q, 4 q + 4) of the flat [row][point] array, one 16-byte load per
// source; per point acc = acc + w[s][row] * double(src_s), s ascending from +0.0, rounded once.
__global__ __launch_bounds__(256) void xsec_mix_kernel(const float* const* __restrict__ src,
                                                       int n_src, const double* __restrict__ w,
                                                       int64_t n_rows, int64_t nhi, int64_t total,
                                                       float* __restrict__ out) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= total) return;
  const int64_t r0 = i0 / nhi;
  if (i0 + 4 <= total) {
    int64_t r[4];
    int64_t rem = i0 - r0 * nhi, row = r0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[e] = row;
      if (++rem == nhi) rem = 0, ++row;
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < n_src; ++s) {
      const float4 v = *reinterpret_cast<const float4*>(src[s] + i0);
      const double* ws = w + (int64_t)s * n_rows;
      acc[0] = acc[0] + ws[r[0]] * (double)v.x;
      acc[1] = acc[1] + ws[r[1]] * (double)v.y;
      acc[2] = acc[2] + ws[r[2]] * (double)v.z;
      acc[3] = acc[3] + ws[r[3]] * (double)v.w;
    }
    *reinterpret_cast<float4*>(out + i0) =
        make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    return;
  }
  for (int64_t i = i0; i < total; ++i) {   // the last, partial quad
    const int64_t row = i / nhi;
    double acc = 0.0;
    for (int s = 0; s < n_src; ++s) acc = acc + w[(int64_t)s * n_rows + row] * (double)src[s][i];
    out[i] = (float)acc;
  }
}

// FREI_KDIST_FORM: "auto" (by bin size, the default), "block" or "wave" (-1 on anything else).
int kdist_form() {
  const char* e = getenv("FREI_KDIST_FORM");
  const std::string f = e ? e : "auto";
  if (f == "auto" || f.empty()) return 0;
  if (f == "block") return 1;
  if (f == "wave") return 2;
  return -1;
}

const char* kWhat = "frei_xsec_kdist: ";

// Columns [col_lo, col_lo + n_out) of the k-distribution of x into d_out, rows at dest_off; a null
// d_out is x's scratch buffer, grown to scratch_n values once the arguments have passed.
int kdist_into(frei_xsec* x, const double* wl_bins, int64_t n_bins, int n_g, const double* g,
               int64_t col_lo, int64_t n_out, const double* T_t, int n_T, const double* p_t,
               int n_p, const std::vector<int64_t>& dest_off, double* d_out, size_t scratch_n,
               int64_t* counts) {
  // ---- every argument error, before any device call
  if (n_g < 1 || n_g > 64)
    return set_error(std::string(kWhat) + "n_g = " + std::to_string(n_g) + " lies outside [1, 64]");
  for (int q = 0; q < n_g; ++q)
    if (!std::isfinite(g[q]) || !(g[q] > 0.0) || !(g[q] < 1.0))
      return set_error(std::string(kWhat) + "g[" + std::to_string(q) + "] = " +
                       std::to_string(g[q]) + " must be finite and in (0, 1)");
  if (n_bins < 1) return set_error(std::string(kWhat) + "n_bins < 1");
  if (n_T < 1 || n_p < 1) return set_error(std::string(kWhat) + "need at least one target (T, p) node");
  TRY(check_ascending(wl_bins, n_bins + 1, "wl_bins"));
  if (col_lo < 0 || n_out < 1 || col_lo + n_out > n_bins * n_g)
    return set_error(std::string(kWhat) + "columns [" + std::to_string(col_lo) + ", " +
                     std::to_string(col_lo + n_out) + ") lie outside the " +
                     std::to_string(n_bins * n_g) + " of the table");
  const int form = kdist_form();
  if (form < 0)
    return set_error(std::string(kWhat) + "FREI_KDIST_FORM must be auto, block or wave");
  std::vector<int64_t> start, end;
  bin_ranges(x->wl, wl_bins, n_bins, &start, &end);
  for (int64_t k = 0; counts && k < n_bins; ++k) counts[k] = end[k] - start[k];
  for (int64_t k = 0; k < n_bins; ++k)
    if (end[k] - start[k] > kMaxBin)
      return set_error(std::string(kWhat) + "bin " + std::to_string(k) + " holds " +
                       std::to_string(end[k] - start[k]) + " points, more than " +
                       std::to_string(kMaxBin) + " (the keys of one bin are sorted in LDS)");

  // ---- host plan: the bins of the slice by launch class, the sampling plan per distinct size
  const SourceRows sr = source_rows(x, T_t, n_T, p_t, n_p, dest_off);
  const int U = (int)sr.row_off.size();
  std::map<int, std::vector<KdBin>> cls;   // P of the block form, 0: the wave form
  std::map<int, int> plan_of;              // bin size -> plan row
  std::vector<int32_t> pj;
  std::vector<double> pf;
  for (int64_t k = col_lo / n_g; k <= (col_lo + n_out - 1) / n_g; ++k) {
    const int n = (int)(end[k] - start[k]);
    if (form == 2 && n > kWaveBin)
      return set_error(std::string(kWhat) + "FREI_KDIST_FORM = wave, but bin " + std::to_string(k) +
                       " holds " + std::to_string(n) + " points, more than " +
                       std::to_string(kWaveBin));
    auto it = plan_of.find(n);
    if (it == plan_of.end()) {
      it = plan_of.emplace(n, (int)plan_of.size()).first;
      for (int q = 0; q < n_g; ++q) {
        // t = g n - 1/2, j = clamp(floor(t), 0, n - 2), f = clamp(t - j, 0, 1)
        const double t = g[q] * (double)n - 0.5;
        const double j = std::min(std::max(std::floor(t), 0.0), (double)std::max(n - 2, 0));
        pj.push_back((int32_t)j);
        pf.push_back(std::min(std::max(t - j, 0.0), 1.0));
      }
    }
    int P = 0;
    if (form == 1 || n > kWaveBin)
      for (P = 64; P < n; P <<= 1) {}
    cls[P].push_back(KdBin{start[k], n, it->second, k});
  }
  std::vector<KdBin> bins;
  for (auto& kv : cls) {
    if ((int64_t)kv.second.size() * U > 0x7FFFFFFF)
      return set_error(std::string(kWhat) + "more than 2^31 (source row, bin) pairs in a launch");
    bins.insert(bins.end(), kv.second.begin(), kv.second.end());
  }

  // ---- device
  if (!d_out) {
    TRY(x->d_scratch.reserve(scratch_n));
    d_out = x->d_scratch;
  }
  double ms = 0.0;
  DeviceCall call(x->stream, "k-distribution");
  const int64_t* d_row = call.upload(sr.row_off.data(), sr.row_off.size());
  const int32_t* d_fo = call.upload(sr.fan_off.data(), sr.fan_off.size());
  const int64_t* d_fd = call.upload(sr.fan_dst.data(), sr.fan_dst.size());
  const KdBin* d_bins = call.upload(bins.data(), bins.size());
  const int32_t* d_pj = call.upload(pj.data(), pj.size());
  const double* d_pf = call.upload(pf.data(), pf.size());
  if (call.ok() && !cls.empty() && cls.rbegin()->first * sizeof(uint32_t) > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&kdist_block_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(cls.rbegin()->first * sizeof(uint32_t))) != hipSuccess)
    call.check(set_error(std::string(kWhat) + "LDS opt-in failed"));
  call.begin(x->timing ? &ms : nullptr);
  if (call.ok()) {
    size_t at = 0;
    for (auto& kv : cls) {
      const int P = kv.first, nb = (int)kv.second.size();
      const int64_t pairs = (int64_t)nb * U;
      if (P == 0)
        kdist_wave_kernel<<<(unsigned)((pairs + 3) / 4), 256, 0, x->stream>>>(
            x->d_x, d_row, d_bins + at, nb, (int)pairs, d_pj, d_pf, n_g, d_fo, d_fd, col_lo, n_out,
            d_out);
      else
        kdist_block_kernel<<<(unsigned)pairs, std::min(1024, std::max(64, P / 2)),
                             (size_t)P * sizeof(uint32_t), x->stream>>>(
            x->d_x, d_row, d_bins + at, nb, P, d_pj, d_pf, n_g, d_fo, d_fd, col_lo, n_out, d_out);
      at += kv.second.size();
    }
  }
  call.end();
  const int rc = call.finish();
  if (!rc && x->timing) {
    x->t_ms += ms;
    x->t_n += 1;
  }
  return rc;
}

int mix_bad_axis(int s, const char* name, int64_t i, double a, double b) {
  return set_error("frei_xsec_mix: source " + std::to_string(s) + " differs from source 0 at " +
                   name + "[" + std::to_string(i) + "] (" + std::to_string(a) + " against " +
                   std::to_string(b) + ")");
}
int mix_same_axis(int s, const char* name, const std::vector<double>& a,
                  const std::vector<double>& b) {
  if (a.size() != b.size())
    return set_error("frei_xsec_mix: source " + std::to_string(s) + " has " +
                     std::to_string(a.size()) + " " + name + ", source 0 has " +
                     std::to_string(b.size()));
  for (size_t i = 0; i < a.size(); ++i)
    if (!(a[i] == b[i])) return mix_bad_axis(s, name, (int64_t)i, a[i], b[i]);
  return 0;
}

}  // namespace

namespace frei {
int kdist_into_table(frei_xsec* x, const double* wl_bins, int64_t n_bins, int n_g,
                     const double* g, int64_t col_lo, int64_t n_out, const double* T_t, int n_T,
                     const double* p_t, int n_p, const int64_t* row_off, double* d_tab,
                     int device) {
  if (!x) return set_error("null cross-section");
  if (x->device != device) return set_error("cross-section and context are on different devices");
  const std::vector<int64_t> dest(row_off, row_off + (size_t)std::max(n_p, 0) * std::max(n_T, 0));
  HIP_TRY(hipSetDevice(x->device));
  return kdist_into(x, wl_bins, n_bins, n_g, g, col_lo, n_out, T_t, n_T, p_t, n_p, dest, d_tab, 0,
                    nullptr);
}
}  // namespace frei

// ==================================================================== C ABI
extern "C" {

int frei_xsec_mix(frei_xsec** out, int n_src, frei_xsec* const* src, const double* weight,
                  double* kernel_ms) {
  // ---- every argument error, before any device call
  if (!out) return set_error("frei_xsec_mix: null argument");
  *out = nullptr;
  if (n_src < 1) return set_error("frei_xsec_mix: n_src < 1");
  if (!src || !weight) return set_error("frei_xsec_mix: null argument");
  for (int s = 0; s < n_src; ++s)
    if (!src[s]) return set_error("frei_xsec_mix: source " + std::to_string(s) + " is null");
  const frei_xsec* x0 = src[0];
  for (int s = 1; s < n_src; ++s) {
    if (src[s]->device != x0->device)
      return set_error("frei_xsec_mix: source " + std::to_string(s) + " lives on device " +
                       std::to_string(src[s]->device) + ", source 0 on device " +
                       std::to_string(x0->device));
    TRY(mix_same_axis(s, "T_nodes", src[s]->T, x0->T));
    TRY(mix_same_axis(s, "p_nodes", src[s]->p, x0->p));
    TRY(mix_same_axis(s, "wl_hi", src[s]->wl, x0->wl));
  }
  const int64_t n_rows = (int64_t)x0->nT * x0->np;
  for (int s = 0; s < n_src; ++s)
    for (int64_t r = 0; r < n_rows; ++r) {
      const double v = weight[(int64_t)s * n_rows + r];
      if (!std::isfinite(v) || v < 0.0)
        return set_error("frei_xsec_mix: weight[" + std::to_string(s) + "][" +
                         std::to_string(r / x0->np) + "][" + std::to_string(r % x0->np) + "] = " +
                         std::to_string(v) + " must be finite and >= 0");
    }
  const int64_t total = n_rows * x0->nhi;
  if ((total / 4 + 1 + 255) / 256 > 0x7FFFFFFF)
    return set_error("frei_xsec_mix: the cross-section is too large for one launch");

  // ---- device
  HIP_TRY(hipSetDevice(x0->device));
  for (int s = 0; s < n_src; ++s) HIP_TRY(hipStreamSynchronize(src[s]->stream));   // values complete
  frei_xsec* x = nullptr;
  TRY(xsec_alloc(&x, x0->device, x0->nT, x0->np, x0->nhi, x0->T.data(), x0->p.data(),
                 x0->wl.data()));
  std::vector<const float*> ptr(n_src);
  for (int s = 0; s < n_src; ++s) ptr[s] = src[s]->d_x;
  int rc = 0;
  {
    DeviceCall call(x->stream, "cross-section mix");
    const float* const* d_ptr = call.upload(ptr.data(), ptr.size());
    const double* d_w = call.upload(weight, (size_t)n_src * n_rows);
    call.begin(kernel_ms);
    if (call.ok())
      xsec_mix_kernel<<<(unsigned)(((total + 3) / 4 + 255) / 256), 256, 0, x->stream>>>(
          d_ptr, n_src, d_w, n_rows, x0->nhi, total, x->d_x);
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

int frei_xsec_kdist(frei_xsec* x, const double* wl_bins, int64_t n_bins, int n_g, const double* g,
                    const double* T_nodes, int n_T, const double* p_nodes, int n_p, double* out,
                    int64_t* counts) {
  if (!x || !wl_bins || !g || !T_nodes || !p_nodes)
    return set_error(std::string(kWhat) + "null argument");
  HIP_TRY(hipSetDevice(x->device));
  // (kdist_into refuses sizes below 1 before it reads any of this)
  const int64_t n_col = n_bins * n_g;
  std::vector<int64_t> dest((size_t)std::max(n_p, 0) * std::max(n_T, 0));
  for (size_t r = 0; r < dest.size(); ++r) dest[r] = (int64_t)r * n_col;
  const size_t total = dest.size() * (size_t)std::max<int64_t>(n_col, 0);
  TRY(kdist_into(x, wl_bins, n_bins, n_g, g, 0, n_col, T_nodes, n_T, p_nodes, n_p, dest, nullptr,
                 total, counts));
  if (out) HIP_TRY(hipMemcpy(out, x->d_scratch, total * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
