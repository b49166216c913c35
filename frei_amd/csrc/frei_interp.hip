// frei_interp.hip — K15: spectra interpolated between the node spectra of a grid sweep.  A
// library X[n_node][n_lam] stays resident with the handle; a call takes a plan idx[n_query]
// [n_corner], w[n_query][n_corner] and writes out[q][i] = sum_c w[q][c] X[idx[q][c]][i], the
// corners in ascending c, one multiply and one add per term.  The reference has no counterpart;
// the definition is the header comment of frei_itp_apply in include/frei_hip.h.
//
// Data: the library is copied once into a buffer of the handle's own, rows at a pitch of n_lam
// rounded up to kPitchQuantum doubles and the padding zero: every row starts 16-byte aligned,
// and a tile's or a pair's read past n_lam stays inside the row (it feeds outputs that are never
// stored).  Per call one of two kernels writes out[n_query][n_lam]:
//   form 1 (itp_gather_kernel): one lane per pair of consecutive outputs of a query, its corners'
//     node values read from global memory 16 bytes at a time.  blockIdx.x runs over the queries
//     (kGatherQueries per block), blockIdx.y over the tiles of 512 wavelengths: blocks that run
//     together read the same slab X[..][tile], from L2.
//   form 2 (itp_lds_kernel): one workgroup per tile of T = 64, 128 or 256 consecutive
//     wavelengths stages X[0 .. n_node)[tile] in LDS once and runs over every query, wave v
//     taking q = v, v + kLdsWaves, ...: idx and w of the query are wave-uniform (one load per
//     lane, broadcast by v_readlane), lane l reads the LDS doubles n T + l + 64 k (consecutive
//     8-byte addresses: conflict-free) and a row of out is written in runs of a whole tile.
// Both forms run the same operations per output: the bits are the same.  No atomics.
#include <string>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

struct frei_itp {
  Stream stream;   // first: destroyed last; created by the first frei_itp_set_nodes
  int device = 0;
  int64_t n_lam = 0, pitch = 0;
  int n_node = 0;
  int tile = 0;                   // form 2's tile width, 0 where the library is too tall for it
  DevBuf<double> d_x;             // [n_node][pitch]
  bool have_nodes = false;
  // The result buffer, reused from call to call and grown when a call needs more (a sampler
  // step of thousands of queries then allocates and frees no gigabytes), of which the first
  // keep_q * n_lam doubles are the last apply's result when it asked to keep (else 0).
  DevBuf<double> d_out;
  int keep_q = 0;
  ~frei_itp() {
    if (!stream) return;   // no device was touched
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
  }
};

namespace {

constexpr int kPitchQuantum = 256;          // doubles: the widest tile of form 2
constexpr int kGatherQueries = 4;           // form 1: queries a block takes in turn
constexpr int kGatherTile = 512;            // form 1: wavelengths per block (256 lanes x 2)
constexpr int kLdsWaves = FREI_ITP_LDS_WAVES;
constexpr size_t kLdsBytes = FREI_ITP_LDS_BYTES;
// form 0: form 2 where it fits, the tiles give every CU a workgroup (kLdsFromTiles: one
// workgroup owns a tile, so fewer tiles than CUs leave CUs idle whatever the query count) and
// the call holds kLdsFromQueries queries and kLdsFromCorners corners or more; form 1 otherwise.
// Measured on MI355X (tools/interp_probe.py, 256 nodes x 100k wavelengths, the forms taking
// turns over 5 rounds; profiles/r15/interp/README.md), gather against LDS form, median ms: 8
// corners x 1 / 64 / 4096 queries 0.007 / 0.037, 0.065 / 0.064, 1.83 / 1.90; 4096 queries x 2
// corners 0.99 / 1.35, x 16 corners 3.01 / 2.74; 16 corners x 64 / 512 queries 0.116 / 0.081,
// 0.663 / 0.385 (run-to-run spread up to 7 % at these shapes, 31 % for the 7 us single-query
// call).  The LDS form wins at 16 corners from 64 queries on, ties at 8 corners within the
// spread, and loses at 2 corners and for a single query (it stages the whole library first).
// Not timed: 3 to 7 and 9 to 15 corners, 2 to 63 queries, 16 corners with fewer than 64 queries.
// The thresholds are the midpoints of the timed neighbours: 12 corners, 32 queries.
constexpr int kLdsFromTiles = 256;
constexpr int kLdsFromQueries = FREI_ITP_LDS_FROM_QUERIES;
constexpr int kLdsFromCorners = FREI_ITP_LDS_FROM_CORNERS;

// The widest tile of 256, 128 or 64 wavelengths whose slab n_node x T doubles fits the LDS
// budget; 0 where not even 64 do.
int tile_width(int n_node) {
  for (int t = 256; t >= 64; t /= 2)
    if ((size_t)n_node * (size_t)t * sizeof(double) <= kLdsBytes) return t;
  return 0;
}

struct ItpArgs {
  const double* x;     // node n at x + n * pitch
  int64_t pitch, n_lam;
  const int32_t* idx;  // [n_query][n_corner]
  const double* w;     // [n_query][n_corner]
  int n_node, n_query, n_corner;
  double* out;         // [n_query][n_lam]
};

// The term and the sum: a rounded product, then a rounded sum (the library is built with
// -ffp-contract=off; nothing here may fuse).
__device__ __forceinline__ double first_term(double w, double x) { return w * x; }
__device__ __forceinline__ double next_term(double acc, double w, double x) {
  const double p = w * x;
  return acc + p;
}

// form 1
__global__ __launch_bounds__(256) void itp_gather_kernel(const ItpArgs a) {
  const int64_t i = ((int64_t)blockIdx.y * 256 + threadIdx.x) * 2;
  if (i >= a.n_lam) return;
  const int q0 = blockIdx.x * kGatherQueries;
  const int nq = min(kGatherQueries, a.n_query - q0);
  const bool pair = (a.n_lam & 1) == 0;   // rows of out are 16-byte aligned
  for (int r = 0; r < nq; ++r) {
    const int q = q0 + r;
    const int32_t* __restrict__ iq = a.idx + (int64_t)q * a.n_corner;   // block-uniform
    const double* __restrict__ wq = a.w + (int64_t)q * a.n_corner;
    const double2 v0 = *reinterpret_cast<const double2*>(a.x + (int64_t)iq[0] * a.pitch + i);
    double ax = first_term(wq[0], v0.x), ay = first_term(wq[0], v0.y);
#pragma unroll 4
    for (int c = 1; c < a.n_corner; ++c) {
      const double2 v = *reinterpret_cast<const double2*>(a.x + (int64_t)iq[c] * a.pitch + i);
      ax = next_term(ax, wq[c], v.x);
      ay = next_term(ay, wq[c], v.y);
    }
    double* o = a.out + (int64_t)q * a.n_lam + i;
    if (pair) {
      *reinterpret_cast<double2*>(o) = double2{ax, ay};
    } else {
      o[0] = ax;
      if (i + 1 < a.n_lam) o[1] = ay;
    }
  }
}

__device__ __forceinline__ double lane_value(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// form 2: T = 64 K
template <int K>
__global__ __launch_bounds__(64 * kLdsWaves) void itp_lds_kernel(const ItpArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sx[];   // [n_node][T]
  constexpr int T = 64 * K, H = T / 2;
  const int64_t i0 = (int64_t)blockIdx.x * T;   // i0 + T <= pitch: the pitch is a multiple of T
  const int pairs = a.n_node * H;
  for (int e = threadIdx.x; e < pairs; e += 64 * kLdsWaves) {
    const int n = e / H, j = (e - n * H) * 2;
    *reinterpret_cast<double2*>(sx + n * T + j) =
        *reinterpret_cast<const double2*>(a.x + (int64_t)n * a.pitch + i0 + j);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cl = min(lane, a.n_corner - 1);   // lanes past the corners re-read the last one
  for (int q = wave; q < a.n_query; q += kLdsWaves) {
    const int my_n = a.idx[(int64_t)q * a.n_corner + cl];
    const double my_w = a.w[(int64_t)q * a.n_corner + cl];
    double acc[K];
    {
      const double wc = lane_value(my_w, 0);
      const double* row = sx + __builtin_amdgcn_readlane(my_n, 0) * T + lane;
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = first_term(wc, row[64 * k]);
    }
    for (int c = 1; c < a.n_corner; ++c) {
      const double wc = lane_value(my_w, c);
      const double* row = sx + __builtin_amdgcn_readlane(my_n, c) * T + lane;
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = next_term(acc[k], wc, row[64 * k]);
    }
    double* o = a.out + (int64_t)q * a.n_lam + i0 + lane;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (i0 + lane + 64 * k < a.n_lam) o[64 * k] = acc[k];
  }
}

template <int K>
int launch_lds(const ItpArgs& a, int tiles, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&itp_lds_kernel<K>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return set_error("frei_itp_apply: LDS opt-in failed");
  itp_lds_kernel<K><<<dim3((unsigned)tiles), 64 * kLdsWaves, lds, st>>>(a);
  return 0;
}

}  // namespace

namespace frei {
int itp_kept_rows(frei_itp* p, ItpRows* out) {
  if (!p) return set_error("null interpolator");
  out->rows = p->keep_q ? p->d_out : nullptr;
  out->n_lam = p->n_lam;
  out->n_query = p->keep_q;
  out->device = p->device;
  return 0;
}
}  // namespace frei

// ==================================================================== C ABI
extern "C" {

int frei_itp_create(frei_itp** out, int device, int64_t n_lam, int n_node) {
  // validated on the host; no device is touched before the first frei_itp_set_nodes
  if (!out) return set_error("frei_itp_create: null argument");
  *out = nullptr;
  if (device < 0) return set_error("frei_itp_create: device must be >= 0");
  if (n_lam < 1) return set_error("frei_itp_create: n_lam must be >= 1");
  if (n_node < 1) return set_error("frei_itp_create: n_node must be >= 1");
  // form 1's grid: one block row per 512 wavelengths
  if ((n_lam + kGatherTile - 1) / kGatherTile > 65535)
    return set_error("frei_itp_create: n_lam / 512 exceeds the launch grid");
  frei_itp* p = new frei_itp();
  p->device = device;
  p->n_lam = n_lam;
  p->pitch = (n_lam + kPitchQuantum - 1) / kPitchQuantum * kPitchQuantum;
  p->n_node = n_node;
  p->tile = tile_width(n_node);
  *out = p;
  return 0;
}

int frei_itp_destroy(frei_itp* p) {
  if (p) delete p;
  return 0;
}

int frei_itp_set_nodes(frei_itp* p, frei_ctx* ctx, frei_brd* brd, const double* x) {
  if (!p) return set_error("frei_itp_set_nodes: null handle");
  if (!x && !ctx && !brd) return set_error("frei_itp_set_nodes: x, ctx and brd are all null");
  SpectrumRows src;
  TRY(spectrum_rows(x, ctx, brd, nullptr, nullptr, p->n_node, p->n_lam, p->device, nullptr,
                    "interpolator", "frei_itp_set_nodes", &src));
  HIP_TRY(hipSetDevice(p->device));
  if (!p->stream) TRY(p->stream.create());
  // the library and whatever was kept end here, whether or not this call succeeds
  p->keep_q = 0;
  p->have_nodes = false;
  HIP_TRY(hipStreamSynchronize(p->stream));
  const size_t rows = (size_t)p->n_node, pitch = (size_t)p->pitch * sizeof(double);
  if (!p->d_x) TRY(p->d_x.alloc(rows * (size_t)p->pitch));
  // a context's rows are copied on its stream, behind the work that writes them
  hipStream_t st = src.stream ? src.stream : (hipStream_t)p->stream;
  HIP_TRY(hipMemsetAsync(p->d_x, 0, rows * pitch, st));
  if (x)
    HIP_TRY(hipMemcpy2DAsync(p->d_x, pitch, x, (size_t)p->n_lam * sizeof(double),
                             (size_t)p->n_lam * sizeof(double), rows, hipMemcpyHostToDevice, st));
  else
    HIP_TRY(hipMemcpy2DAsync(p->d_x, pitch, src.rows, (size_t)src.stride * sizeof(double),
                             (size_t)p->n_lam * sizeof(double), rows, hipMemcpyDeviceToDevice,
                             st));
  HIP_TRY(hipStreamSynchronize(st));
  p->have_nodes = true;
  return 0;
}

int frei_itp_apply(frei_itp* p, int n_query, int n_corner, const int32_t* idx, const double* w,
                   int form, double* out, int keep, int* form_used, double* kernel_ms) {
  const std::string me = "frei_itp_apply: ";
  if (!p) return set_error(me + "null handle");
  if (n_query < 1) return set_error(me + "n_query must be >= 1");
  if (n_corner < 1 || n_corner > FREI_ITP_MAX_CORNERS)
    return set_error(me + "n_corner = " + std::to_string(n_corner) + " lies outside [1, " +
                     std::to_string(FREI_ITP_MAX_CORNERS) + "]");
  if (!idx || !w) return set_error(me + "idx or w is null");
  if (!out && !keep) return set_error(me + "out is null and keep is not set");
  if (form < 0 || form > 2)
    return set_error(me + "form must be 0 (automatic), 1 (gather) or 2 (LDS-staged)");
  for (int q = 0; q < n_query; ++q)
    for (int c = 0; c < n_corner; ++c) {
      const int32_t n = idx[(size_t)q * n_corner + c];
      if (n < 0 || n >= p->n_node)
        return set_error(me + "idx[" + std::to_string(q) + "][" + std::to_string(c) + "] = " +
                         std::to_string(n) + " lies outside [0, n_node = " +
                         std::to_string(p->n_node) + ")");
    }
  if (form == 2 && !p->tile)
    return set_error(me + "form 2 stages at most " + std::to_string(FREI_ITP_LDS_MAX_NODES) +
                     " nodes in LDS, not n_node = " + std::to_string(p->n_node));
  if (!p->have_nodes) return set_error(me + "no nodes set (frei_itp_set_nodes)");
  const int tiles = p->tile ? (int)((p->n_lam + p->tile - 1) / p->tile) : 0;
  int f = form;
  if (f == 0)
    f = p->tile && tiles >= kLdsFromTiles && n_query >= kLdsFromQueries &&
                n_corner >= kLdsFromCorners
            ? 2
            : 1;
  if (form_used) *form_used = f;

  HIP_TRY(hipSetDevice(p->device));
  p->keep_q = 0;   // what an earlier call kept ends here, whether or not this call succeeds
  hipStream_t st = p->stream;
  const size_t Q = (size_t)n_query, n = (size_t)p->n_lam, C = (size_t)n_corner;
  DeviceCall call(st, "interpolation");
  call.check(p->d_out.reserve(Q * n));   // every earlier call has finished (synchronised)
  ItpArgs a;
  a.x = p->d_x;
  a.pitch = p->pitch;
  a.n_lam = p->n_lam;
  a.idx = call.upload(idx, Q * C);
  a.w = call.upload(w, Q * C);
  a.n_node = p->n_node;
  a.n_query = n_query;
  a.n_corner = n_corner;
  a.out = p->d_out;
  call.begin(kernel_ms);
  if (call.ok()) {
    if (f == 1) {
      const dim3 grid((unsigned)((n_query + kGatherQueries - 1) / kGatherQueries),
                      (unsigned)((n + kGatherTile - 1) / kGatherTile));
      itp_gather_kernel<<<grid, 256, 0, st>>>(a);
    } else {
      const size_t lds = (size_t)p->n_node * (size_t)p->tile * sizeof(double);
      if (p->tile == 256) call.check(launch_lds<4>(a, tiles, lds, st));
      else if (p->tile == 128) call.check(launch_lds<2>(a, tiles, lds, st));
      else call.check(launch_lds<1>(a, tiles, lds, st));
    }
  }
  call.end();
  call.download(out, a.out, Q * n);
  const int rc = call.finish();
  if (!rc && keep) p->keep_q = n_query;   // complete: finish() synchronised the stream
  return rc;
}

}  // extern "C"
