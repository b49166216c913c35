// frei_kmix.hip — K19: a gas mixture's k-table from the species' k-tables by random overlap with
// resort-and-rebin (the definition is in include/frei_hip.h).  A frei_klib keeps n_src k-tables
// K_s[n_p][n_T][n_bins][n_g] on shared nodes, bins and one quadrature resident in HBM;
// frei_klib_mix folds them, species after species, into the mixture's table for any number of
// compositions, and frei_set_table_kmix (frei_runtime.hip) writes one composition's mixture
// straight into a context.  No reference counterpart: every correlated-k code mixes this way
// (Lacis & Oinas 1991; Amundsen et al. 2017, "random overlap with resorting and rebinning").
//
// One work item per (listed row, bin), a row being one (composition, node) pair with its own
// destination (K20: a batch of atmospheres lists only the pressure rows its layers sit on); the
// running a[n_g] stays on chip over the species loop.  Per fold the n_g^2 pair values
// v_e = a[q] + b[r] become 64-bit order-preserving keys (-0 -> +0, every NaN the canonical quiet NaN, which sorts last), the pairs are sorted by
// (key, e), the fixed-point pair weights are scanned exactly in uint64, and lane q sums
// double(overlap) * log(v) over the pairs that overlap its quadrature interval, in sorted order.
// Two forms; the automatic choice is the wave form for n_g <= 2 and the block form above, as
// measured:
//   wave:  n_g <= 8, one wave per item and four per block; one pair per lane, the bitonic network,
//     the scan and the walk all on cross-lane reads (no LDS);
//   block: one block per item; the pairs are padded to a power of two P (64 .. 4096) with keys
//     above every key, key[P] (8 B), e[P] (2 B) and log v[P] (8 B) live in dynamic LDS (18 P + 2048
//     bytes: 74 KiB at P = 4096, two blocks per CU), strides below 64 of the network run on
//     cross-lane exchanges as in kdist_block_kernel, the scan is a wave scan per run of 64 plus a
//     scan of the run totals, and the first n_g lanes find their interval's first pair by
//     bisection and walk it sequentially.
// Sorting and the integer scan are exact and the walk is one fixed sequence of operations, so
// both forms give the same bits.  8-byte keys one per lane touch every LDS bank once per half
// wave (bank = (address / 4) mod 64 for 8-byte reads): the network's accesses are conflict-free.
// HBM traffic per item: n_src * n_g values read, n_g written.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

struct frei_klib {
  Stream stream;   // first: destroyed last
  int device = 0;
  int n_src = 0, n_p = 0, n_T = 0, n_g = 0;
  int64_t n_bins = 0;
  std::vector<double> wl_bins, g, w, p, T;
  std::vector<uint64_t> W;   // [n_g] fixed-point weights
  std::vector<uint64_t> E;   // [n_g + 1] interval bounds in units of Wt^2
  std::vector<char> set;     // [n_src] slot holds a table
  DevBuf<double> d_k;        // [n_src][n_p][n_T][n_bins][n_g]
  DevBuf<uint64_t> d_W;
  DevBuf<uint64_t> d_E;
  DevBuf<double> d_out;      // the result of frei_klib_mix (grow-only)
  ~frei_klib() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

namespace {

constexpr int kMaxG = 64;    // quadrature points (4096 pairs: the block form's largest P)
constexpr int kWaveG = 8;    // the wave form's (64 pairs: one per lane)
// The automatic choice (measured, tools/kmix_probe.py): the wave form is 3 to 9 % ahead at
// n_g = 2 and 1.2 to 3.0 times behind at n_g = 4 and 8; n_g = 3 was not measured.
constexpr int kAutoWaveG = 2;
enum { kAuto = 0, kWave = 1, kBlock = 2 };

struct KmixArgs {
  const double* k;       // [n_src][n_nodes][n_bins][n_g]
  const double* x;       // [n_comp][n_src][n_nodes]
  const uint64_t* W;     // [n_g]
  const uint64_t* E;     // [n_g + 1]
  const KmixRow* rows;   // [n_rows] the (composition, node) pairs to mix, each with the element
                         // offset of its destination row in out
  double* out;
  int64_t col_lo, n_out; // the columns [col_lo, col_lo + n_out) of the n_bins * n_g are stored
  int64_t slot;          // n_nodes * n_bins * n_g: values of one table
  int n_src, n_nodes, n_bins, n_g;
  int bin_lo, nbl;       // the bins [bin_lo, bin_lo + nbl) are mixed
  unsigned n_items;      // n_rows * nbl
  unsigned first;        // the launch's first item (a launch is kept below 2^31 lanes)
};

// double -> uint64 whose unsigned order is K18's: -0 -> +0, any NaN -> the canonical NaN (last).
__device__ __forceinline__ uint64_t key_of(double v) {
  uint64_t b = (uint64_t)__double_as_longlong(v);
  if (v != v) b = 0x7FF8000000000000ull;
  if (v == 0.0) b = 0ull;
  return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// One compare-exchange of the bitonic network across lanes on (key, e): lane ^ j is the partner.
__device__ __forceinline__ void exchange(uint64_t& key, int& e, int j, bool keep_min) {
  const uint64_t ok = __shfl_xor((unsigned long long)key, j);
  const int oe = __shfl_xor(e, j);
  const bool less = key < ok || (key == ok && e < oe);
  if (less != keep_min) {
    key = ok;
    e = oe;
  }
}

// Inclusive scan of one value per lane over the wave, exact in uint64.
__device__ __forceinline__ uint64_t wave_scan(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up((unsigned long long)v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// Item w = listed row * nbl + (bin - bin_lo).
struct Item {
  int bin;
  int64_t dst;        // element offset of the row's column 0 in out
  const double* k0;   // K_0 of the item's (node, bin)
  const double* x0;   // x_0 of its (composition, node)
};
__device__ __forceinline__ Item item_of(const KmixArgs& a, unsigned w) {
  Item it;
  const unsigned row = w / (unsigned)a.nbl;
  it.bin = a.bin_lo + (int)(w - row * (unsigned)a.nbl);
  const KmixRow r = a.rows[row];
  const int c = r.comp, nd = r.node;
  it.dst = r.dst;
  it.k0 = a.k + ((int64_t)nd * a.n_bins + it.bin) * a.n_g;
  it.x0 = a.x + (int64_t)c * a.n_src * a.n_nodes + nd;
  return it;
}
__device__ __forceinline__ void store(const KmixArgs& a, const Item& it, int q, double v) {
  const int64_t c = (int64_t)it.bin * a.n_g + q - a.col_lo;
  if (c >= 0 && c < a.n_out) a.out[it.dst + c] = v;
}

// wave form: wave (blockIdx.x * 4 + wave of the block) is the item; n_g <= 8.
__global__ __launch_bounds__(256) void kmix_wave_kernel(const KmixArgs a) {
  const int lane = threadIdx.x & 63;
  const unsigned w = a.first + blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= a.n_items) return;   // wave-uniform; the kernel has no barrier
  const Item it = item_of(a, w);
  const int n_g = a.n_g, n = n_g * n_g;
  const bool own = lane < n_g;    // lane q holds a[q], b[q], W_q and q's interval
  const int q = lane / n_g, r = lane - q * n_g;   // the lane's pair e = lane, when lane < n
  const uint64_t Wm = own ? a.W[lane] : 0ull;
  const uint64_t Elo = own ? a.E[lane] : 0ull, Ehi = own ? a.E[lane + 1] : 0ull;
  double av = own ? it.x0[0] * it.k0[lane] : 0.0;
  for (int s = 1; s < a.n_src; ++s) {
    const double bv = own ? it.x0[(int64_t)s * a.n_nodes] * it.k0[s * a.slot + lane] : 0.0;
    const double v = __shfl(av, q) + __shfl(bv, r);
    uint64_t key = lane < n ? key_of(v) : ~0ull;
    int e = lane;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1)
        exchange(key, e, j, ((lane & j) == 0) == ((lane & k) == 0));
    // lane i now holds the i-th pair of the order; the padding (e >= n) sits behind the n pairs
    const int eq = e / n_g, er = e - eq * n_g;
    const uint64_t wq = __shfl((unsigned long long)Wm, eq & 63);
    const uint64_t wr = __shfl((unsigned long long)Wm, er);
    const uint64_t u = e < n ? wq * wr : 0ull;
    const uint64_t C = wave_scan(u, lane) - u;
    const double lnv = log(value_of(key));
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
      const uint64_t Ci = __shfl((unsigned long long)C, i), ui = __shfl((unsigned long long)u, i);
      const double li = __shfl(lnv, i);
      const uint64_t lo = max(Ci, Elo), hi = min(Ci + ui, Ehi);
      if (own && hi > lo) acc = acc + (double)(hi - lo) * li;
    }
    av = own ? exp(acc / (double)(Ehi - Elo)) : 0.0;
  }
  if (own) store(a, it, lane, av);
}

// block form: block blockIdx.x is the item; P >= n_g^2 pairs in dynamic LDS.
__global__ __launch_bounds__(1024) void kmix_block_kernel(const KmixArgs a, int P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem);   // [P] the key, after the scan C in its run
  double* lnv = reinterpret_cast<double*>(keys + P);    // [P] log v of the sorted pairs
  double* sa = lnv + P;                                 // [64] a
  double* sb = sa + 64;                                 // [64] b
  uint64_t* sW = reinterpret_cast<uint64_t*>(sb + 64);  // [64] W
  uint64_t* runs = sW + 64;                             // [64] exclusive offsets of the runs of 64
  uint16_t* idx = reinterpret_cast<uint16_t*>(runs + 64);   // [P] e
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
  const Item it = item_of(a, a.first + blockIdx.x);
  const int n_g = a.n_g, n = n_g * n_g;
  if (tid < n_g) {
    sa[tid] = it.x0[0] * it.k0[tid];
    sW[tid] = a.W[tid];
  }
  for (int s = 1; s < a.n_src; ++s) {
    if (tid < n_g) sb[tid] = it.x0[(int64_t)s * a.n_nodes] * it.k0[s * a.slot + tid];
    __syncthreads();
    // every phase k <= 64 of the network while the pairs are formed (nt and P are multiples of
    // 64: whole waves take whole aligned runs of 64 pairs, one per lane)
    for (int i = tid; i < P; i += nt) {
      const int q = i / n_g;
      uint64_t key = i < n ? key_of(sa[q] + sb[i - q * n_g]) : ~0ull;
      int e = i;
#pragma unroll
      for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
          exchange(key, e, j, ((lane & j) == 0) == ((i & k) == 0));
      keys[i] = key;
      idx[i] = (uint16_t)e;
    }
    __syncthreads();
    for (int k = 128; k <= P; k <<= 1) {
      for (int j = k >> 1; j >= 64; j >>= 1) {
        for (int t = tid; t < (P >> 1); t += nt) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // bit j clear
          const int l = i | j;
          const uint64_t ka = keys[i], kc = keys[l];
          const uint16_t ea = idx[i], ec = idx[l];
          const bool gt = ka > kc || (ka == kc && ea > ec);
          if (gt == ((i & k) == 0)) {
            keys[i] = kc;
            keys[l] = ka;
            idx[i] = ec;
            idx[l] = ea;
          }
        }
        __syncthreads();
      }
      for (int i = tid; i < P; i += nt) {
        uint64_t key = keys[i];
        int e = idx[i];
#pragma unroll
        for (int j = 32; j > 0; j >>= 1)
          exchange(key, e, j, ((lane & j) == 0) == ((i & k) == 0));
        keys[i] = key;
        idx[i] = (uint16_t)e;
      }
      __syncthreads();
    }
    // log v and the exclusive prefix of the pair weights inside each run of 64
    for (int i = tid; i < P; i += nt) {
      const int e = idx[i];
      const int eq = e / n_g;
      const uint64_t u = e < n ? sW[eq] * sW[e - eq * n_g] : 0ull;
      lnv[i] = log(value_of(keys[i]));
      const uint64_t inc = wave_scan(u, lane);
      keys[i] = inc - u;
      if (lane == 63) runs[i >> 6] = inc;
    }
    __syncthreads();
    if (tid < 64) {
      const uint64_t t = tid < (P >> 6) ? runs[tid] : 0ull;
      runs[tid] = wave_scan(t, lane) - t;
    }
    __syncthreads();
    // lane q: the last pair that starts at or before E_q, then the pairs up to E_{q+1} in order
    double res = 0.0;
    if (tid < n_g) {
      const uint64_t Elo = a.E[tid], Ehi = a.E[tid + 1], Eall = a.E[n_g];
      int lo = 0, hi = n - 1;   // C_0 = 0 <= Elo
      while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (keys[m] + runs[m >> 6] <= Elo) lo = m; else hi = m - 1;
      }
      double acc = 0.0;
      for (int i = lo; i < n; ++i) {
        const uint64_t Ci = keys[i] + runs[i >> 6];
        if (Ci >= Ehi) break;
        const uint64_t Cn = i + 1 < n ? keys[i + 1] + runs[(i + 1) >> 6] : Eall;
        acc = acc + (double)(min(Cn, Ehi) - max(Ci, Elo)) * lnv[i];
      }
      res = exp(acc / (double)(Ehi - Elo));
    }
    __syncthreads();   // (sa was last read while the pairs were formed)
    if (tid < n_g) sa[tid] = res;
  }
  __syncthreads();
  if (tid < n_g) store(a, it, tid, sa[tid]);
}

int block_P(int n_g) {
  int P = 64;
  while (P < n_g * n_g) P <<= 1;
  return P;
}
size_t block_lds(int P) { return (size_t)P * 18 + 4 * 64 * 8; }

// FREI_KMIX_FORM: "auto" (by n_g, the default), "wave" or "block" (-1 on anything else).
int env_form() {
  const char* e = getenv("FREI_KMIX_FORM");
  const std::string f = e ? e : "auto";
  if (f == "auto" || f.empty()) return kAuto;
  if (f == "wave") return kWave;
  if (f == "block") return kBlock;
  return -1;
}

// The form to launch for the request *form (0: FREI_KMIX_FORM, then by n_g), or its error.
int choose_form(const std::string& me, const frei_klib* lib, int* form) {
  if (*form < 0 || *form > 2)
    return set_error(me + "form must be 0 (automatic), 1 (wave) or 2 (block)");
  if (*form == kAuto) *form = env_form();
  if (*form < 0) return set_error(me + "FREI_KMIX_FORM must be auto, wave or block");
  if (*form == kWave && lib->n_g > kWaveG)
    return set_error(me + "the wave form takes n_g <= " + std::to_string(kWaveG) + ", not n_g = " +
                     std::to_string(lib->n_g));
  if (*form == kAuto) *form = lib->n_g <= kAutoWaveG ? kWave : kBlock;
  return 0;
}

// Every argument error of a mix but the form's (choose_form), before any device call.
int check_mix(const std::string& me, const frei_klib* lib, int n_comp, const double* x,
              int64_t col_lo, int64_t n_out) {
  if (!lib) return set_error(me + "null library");
  if (!x) return set_error(me + "null x");
  if (n_comp < 1) return set_error(me + "n_comp < 1");
  for (int s = 0; s < lib->n_src; ++s)
    if (!lib->set[s]) return set_error(me + "slot " + std::to_string(s) + " holds no table");
  const int64_t n_col = lib->n_bins * lib->n_g;
  if (col_lo < 0 || n_out < 1 || col_lo + n_out > n_col)
    return set_error(me + "columns [" + std::to_string(col_lo) + ", " +
                     std::to_string(col_lo + n_out) + ") lie outside the " +
                     std::to_string(n_col) + " of the table");
  for (int c = 0; c < n_comp; ++c)
    for (int s = 0; s < lib->n_src; ++s)
      for (int kp = 0; kp < lib->n_p; ++kp)
        for (int kt = 0; kt < lib->n_T; ++kt) {
          const double v = x[(((size_t)c * lib->n_src + s) * lib->n_p + kp) * lib->n_T + kt];
          if (!std::isfinite(v) || v < 0.0)
            return set_error(me + "x[" + std::to_string(c) + "][" + std::to_string(s) + "][" +
                             std::to_string(kp) + "][" + std::to_string(kt) + "] = " +
                             std::to_string(v) + " must be finite and >= 0");
        }
  const int64_t nbl = (col_lo + n_out - 1) / lib->n_g - col_lo / lib->n_g + 1;
  if ((int64_t)n_comp * lib->n_p * lib->n_T * nbl > 0x7FFFFFFF)
    return set_error(me + "more than 2^31 (composition, node, bin) items in a launch");
  return 0;
}

// Every (composition, node) row, row (c, node) at dst[c * n_nodes + node]: the full list.
std::vector<KmixRow> all_rows(int n_comp, int n_nodes, const int64_t* dst) {
  std::vector<KmixRow> rows((size_t)n_comp * n_nodes);
  for (int c = 0; c < n_comp; ++c)
    for (int nd = 0; nd < n_nodes; ++nd)
      rows[(size_t)c * n_nodes + nd] = KmixRow{c, nd, dst[(size_t)c * n_nodes + nd]};
  return rows;
}

// The mixture's columns [col_lo, col_lo + n_out) of the listed rows of n_comp compositions (already
// checked) into d_out on the stream st; the call returns when the stream has finished.
int mix_into(frei_klib* lib, int n_comp, const double* x, int64_t col_lo, int64_t n_out,
             const KmixRow* rows, size_t n_rows, double* d_out, int form, double* kernel_ms,
             hipStream_t st) {
  const int n_nodes = lib->n_p * lib->n_T;
  KmixArgs a{};
  a.k = lib->d_k;
  a.W = lib->d_W;
  a.E = lib->d_E;
  a.out = d_out;
  a.col_lo = col_lo;
  a.n_out = n_out;
  a.slot = (int64_t)n_nodes * lib->n_bins * lib->n_g;
  a.n_src = lib->n_src;
  a.n_nodes = n_nodes;
  a.n_bins = (int)lib->n_bins;
  a.n_g = lib->n_g;
  a.bin_lo = (int)(col_lo / lib->n_g);
  a.nbl = (int)((col_lo + n_out - 1) / lib->n_g) - a.bin_lo + 1;
  a.n_items = (unsigned)((int64_t)n_rows * a.nbl);
  const int P = block_P(lib->n_g);
  DeviceCall call(st, "k-table mix");
  a.x = call.upload(x, (size_t)n_comp * lib->n_src * n_nodes);
  a.rows = call.upload(rows, n_rows);
  if (call.ok() && form == kBlock && block_lds(P) > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&kmix_block_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)block_lds(P)) != hipSuccess)
    call.check(set_error("frei_klib_mix: LDS opt-in failed"));
  call.begin(kernel_ms);
  if (call.ok()) {
    // a launch's lanes (blocks x lanes per block) must stay below 2^32: at most 2^31 per launch
    const unsigned nt = form == kWave ? 256u : (unsigned)std::min(1024, std::max(64, P / 2));
    const unsigned per = (0x80000000u / nt) * (form == kWave ? 4u : 1u);   // items per launch
    for (a.first = 0; a.first < a.n_items; a.first += per) {
      const unsigned n = std::min(per, a.n_items - a.first);
      if (form == kWave)
        kmix_wave_kernel<<<(n + 3u) / 4u, nt, 0, st>>>(a);
      else
        kmix_block_kernel<<<n, nt, block_lds(P), st>>>(a, P);
    }
  }
  call.end();
  return call.finish();
}

}  // namespace

namespace frei {
int klib_batch_args(const std::string& me, frei_klib* lib, int n_comp, const double* x,
                    int64_t col_lo, int64_t n_out, int device, KlibNodes* out) {
  int form = kAuto;   // (a bad FREI_KMIX_FORM is refused here too, before the context changes)
  TRY(check_mix(me, lib, n_comp, x, col_lo, n_out));
  TRY(choose_form(me, lib, &form));
  if (lib->device != device)
    return set_error(me + "the library lives on device " + std::to_string(lib->device) +
                     ", the context on device " + std::to_string(device));
  if (out) *out = KlibNodes{lib->p.data(), lib->T.data(), lib->n_p, lib->n_T, lib->n_src};
  return 0;
}

int kmix_rows_into(const std::string& me, frei_klib* lib, int n_comp, const double* x,
                   int64_t col_lo, int64_t n_out, const KmixRow* rows, size_t n_rows,
                   double* d_out, hipStream_t st) {
  int form = kAuto;
  TRY(choose_form(me, lib, &form));
  if (n_rows == 0) return 0;
  return mix_into(lib, n_comp, x, col_lo, n_out, rows, n_rows, d_out, form, nullptr, st);
}
}  // namespace frei

// ==================================================================== C ABI
extern "C" {

int frei_klib_create(frei_klib** out, int device, int n_src, int n_p, int n_T, int64_t n_bins,
                     int n_g, const double* wl_bins, const double* g, const double* w,
                     const double* p_nodes, const double* T_nodes) {
  // ---- every argument error, before any device call
  const std::string me = "frei_klib_create: ";
  if (!out) return set_error(me + "null argument");
  *out = nullptr;
  if (!wl_bins || !g || !w || !p_nodes || !T_nodes) return set_error(me + "null argument");
  if (device < 0) return set_error(me + "device must be >= 0");
  if (n_src < 1) return set_error(me + "n_src < 1");
  if (n_p < 1 || n_T < 1) return set_error(me + "need at least one (T, p) node");
  if (n_bins < 1) return set_error(me + "n_bins < 1");
  if (n_g < 1 || n_g > kMaxG)
    return set_error(me + "n_g = " + std::to_string(n_g) + " lies outside [1, 64]");
  TRY(check_ascending(wl_bins, n_bins + 1, "wl_bins"));
  for (int q = 0; q < n_g; ++q)
    if (!std::isfinite(g[q]) || !(g[q] > 0.0) || !(g[q] < 1.0) || (q > 0 && !(g[q] > g[q - 1])))
      return set_error(me + "g[" + std::to_string(q) + "] = " + std::to_string(g[q]) +
                       " must be finite, in (0, 1) and above the g before it");
  std::vector<uint64_t> W(n_g), E(n_g + 1);
  uint64_t Wt = 0;
  for (int q = 0; q < n_g; ++q) {
    if (!std::isfinite(w[q]) || !(w[q] > 0.0) || w[q] > 2.0)
      return set_error(me + "w[" + std::to_string(q) + "] = " + std::to_string(w[q]) +
                       " must be finite and positive, and the weights sum to at most 2");
    W[q] = (uint64_t)std::llrint(w[q] * 1073741824.0);
    if (W[q] < 1)
      return set_error(me + "w[" + std::to_string(q) + "] = " + std::to_string(w[q]) +
                       " is below the fixed-point step 2^-30");
    Wt += W[q];
    if (Wt > (1ull << 31))
      return set_error(me + "the weights up to w[" + std::to_string(q) + "] sum to more than 2");
  }
  uint64_t acc = 0;
  for (int q = 0; q <= n_g; ++q) {
    E[q] = Wt * acc;
    if (q < n_g) acc += W[q];
  }
  for (int k = 0; k < n_p; ++k)
    if (!std::isfinite(p_nodes[k]))
      return set_error(me + "p_nodes[" + std::to_string(k) + "] is not finite");
  for (int k = 0; k < n_T; ++k)
    if (!std::isfinite(T_nodes[k]))
      return set_error(me + "T_nodes[" + std::to_string(k) + "] is not finite");

  // ---- device
  HIP_TRY(hipSetDevice(device));
  frei_klib* h = new frei_klib();
  h->device = device;
  h->n_src = n_src;
  h->n_p = n_p;
  h->n_T = n_T;
  h->n_g = n_g;
  h->n_bins = n_bins;
  h->wl_bins.assign(wl_bins, wl_bins + n_bins + 1);
  h->g.assign(g, g + n_g);
  h->w.assign(w, w + n_g);
  h->p.assign(p_nodes, p_nodes + n_p);
  h->T.assign(T_nodes, T_nodes + n_T);
  h->W = W;
  h->E = E;
  h->set.assign(n_src, 0);
  const size_t total = (size_t)n_src * n_p * n_T * (size_t)n_bins * n_g;
  if (h->stream.create() || h->d_k.alloc(total) || h->d_W.alloc(W.size()) ||
      h->d_E.alloc(E.size()) ||
      hipMemcpy(h->d_W, W.data(), W.size() * sizeof(uint64_t), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(h->d_E, E.data(), E.size() * sizeof(uint64_t), hipMemcpyHostToDevice) !=
          hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return set_error(me + "device allocation failed");
  }
  *out = h;
  return 0;
}

int frei_klib_destroy(frei_klib* lib) {
  if (lib) delete lib;
  return 0;
}

int frei_klib_set(frei_klib* lib, int s, const double* k) {
  const std::string me = "frei_klib_set: ";
  if (!lib || !k) return set_error(me + "null argument");
  if (s < 0 || s >= lib->n_src)
    return set_error(me + "slot " + std::to_string(s) + " lies outside [0, n_src = " +
                     std::to_string(lib->n_src) + ")");
  HIP_TRY(hipSetDevice(lib->device));
  const size_t slot = (size_t)lib->n_p * lib->n_T * (size_t)lib->n_bins * lib->n_g;
  lib->set[s] = 0;
  HIP_TRY(hipMemcpy(lib->d_k + s * slot, k, slot * sizeof(double), hipMemcpyHostToDevice));
  lib->set[s] = 1;
  return 0;
}

int frei_klib_set_kdist(frei_klib* lib, int s, frei_xsec* x) {
  const std::string me = "frei_klib_set_kdist: ";
  if (!lib || !x) return set_error(me + "null argument");
  if (s < 0 || s >= lib->n_src)
    return set_error(me + "slot " + std::to_string(s) + " lies outside [0, n_src = " +
                     std::to_string(lib->n_src) + ")");
  if (x->device != lib->device)
    return set_error(me + "the cross-section lives on device " + std::to_string(x->device) +
                     ", the library on device " + std::to_string(lib->device));
  const int64_t n_col = lib->n_bins * lib->n_g;
  std::vector<int64_t> row_off((size_t)lib->n_p * lib->n_T);
  for (size_t r = 0; r < row_off.size(); ++r) row_off[r] = (int64_t)r * n_col;
  lib->set[s] = 0;
  TRY(kdist_into_table(x, lib->wl_bins.data(), lib->n_bins, lib->n_g, lib->g.data(), 0, n_col,
                       lib->T.data(), lib->n_T, lib->p.data(), lib->n_p, row_off.data(),
                       lib->d_k + (size_t)s * row_off.size() * n_col, lib->device));
  lib->set[s] = 1;
  return 0;
}

int frei_klib_mix(frei_klib* lib, int n_comp, const double* x, double* out, int form,
                  double* kernel_ms) {
  const std::string me = "frei_klib_mix: ";
  if (kernel_ms) *kernel_ms = 0.0;
  const int64_t n_col = lib ? lib->n_bins * lib->n_g : 0;
  TRY(check_mix(me, lib, n_comp, x, 0, n_col));
  TRY(choose_form(me, lib, &form));
  const size_t rows = (size_t)n_comp * lib->n_p * lib->n_T, total = rows * (size_t)n_col;
  HIP_TRY(hipSetDevice(lib->device));
  TRY(lib->d_out.reserve(total));
  std::vector<int64_t> dst(rows);
  for (size_t r = 0; r < rows; ++r) dst[r] = (int64_t)r * n_col;
  const std::vector<KmixRow> list = all_rows(n_comp, lib->n_p * lib->n_T, dst.data());
  TRY(mix_into(lib, n_comp, x, 0, n_col, list.data(), list.size(), lib->d_out, form, kernel_ms,
               lib->stream));
  if (out) HIP_TRY(hipMemcpy(out, lib->d_out, total * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
