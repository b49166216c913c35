// frei_host.h — the host code every translation unit's C entry points share: the error macros,
// device allocation and copies, the scaffold of one post-processing call (DeviceCall) and the
// resolution of a spectrum's sources.  Host code only; a new post-processing call starts
// from DeviceCall and spectrum_rows ("Host scaffold").
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <string>
#include <vector>

#include "frei_device.h"

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return frei::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

#define TRY(expr)            \
  do {                       \
    int _r = (expr);         \
    if (_r != 0) return _r;  \
  } while (0)

namespace frei {

// K6's host plan (frei_binning.hip), which K18 (frei_kdist.hip) shares: the nearest source node of
// each target (scipy 'nearest' on the sorted nodes), pandas.cut's point ranges [start_k, end_k)
// of the bins on an ascending axis, and the distinct source rows the target nodes (kp, kt)
// select with the destination rows dest_off[kp * n_T + kt] that read each (CSR).
std::vector<int> nearest_index(const std::vector<double>& nodes, const double* t, int n);
void bin_ranges(const std::vector<double>& wl, const double* wl_bins, int64_t n_bins,
                std::vector<int64_t>* start, std::vector<int64_t>* end);
struct SourceRows {
  std::vector<int64_t> row_off;   // [U] element offset of each distinct source row in d_x
  std::vector<int32_t> fan_off;   // [U + 1]
  std::vector<int64_t> fan_dst;   // [n_p * n_T] destination row offsets, grouped by source row
};
SourceRows source_rows(const frei_xsec* x, const double* T_t, int n_T, const double* p_t, int n_p,
                       const std::vector<int64_t>& dest_off);
int check_ascending(const double* a, int64_t n, const char* what);
int xsec_alloc(frei_xsec** out, int device, int n_T, int n_p, int64_t n_hi,
               const double* T_nodes, const double* p_nodes, const double* wl_hi);

template <typename T>
int dalloc(T** p, size_t n) {
  if (n == 0) n = 1;
  HIP_TRY(hipMalloc((void**)p, n * sizeof(T)));
  // FREI_ALLOC_FILL (diagnostic): fill every new device buffer with a byte value, so a read of
  // memory the engine never wrote shows up as changed results
  static const int fill = [] {
    const char* e = getenv("FREI_ALLOC_FILL");
    return e ? atoi(e) : -1;
  }();
  if (fill >= 0) {   // (the null-stream memset must finish before the caller's stream uses p)
    HIP_TRY(hipMemset((void*)*p, fill, n * sizeof(T)));
    HIP_TRY(hipDeviceSynchronize());
  }
  return 0;
}

// What is alive in this process (frei_live_resources): raised by the owning types below when
// they acquire, lowered when they let go.
enum LiveKind { kLiveDevice, kLivePinned, kLiveStream, kLiveEvent };
inline std::atomic<int64_t> g_live[4];

struct DeviceMem {
  static constexpr LiveKind kind = kLiveDevice;
  template <typename T>
  static int get(T** p, size_t n) { return dalloc(p, n); }
  static void put(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
  static constexpr LiveKind kind = kLivePinned;
  template <typename T>
  static int get(T** p, size_t n) {
    HIP_TRY(hipHostMalloc((void**)p, (n ? n : 1) * sizeof(T), hipHostMallocDefault));
    return 0;
  }
  static void put(void* p) { (void)hipHostFree(p); }
};

// Owns n elements of device (DevBuf) or pinned host (PinnedBuf) memory; converts to T* wherever
// a raw pointer is read.  reserve() and reset() never synchronise: where queued work may still
// read the old buffer, the caller synchronises its stream first.
template <typename T, typename Mem>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) adopt_counted(o.p_, o.cap_), o.p_ = nullptr, o.cap_ = 0;
    return *this;
  }
  ~Buf() { reset(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }

  // Releases what it holds and allocates exactly n elements (one for n == 0).
  int alloc(size_t n) {
    reset();
    if (int rc = Mem::get(&p_, n)) {
      p_ = nullptr;
      (void)hipGetLastError();   // a failed allocation must not fail the next call's checks
      return rc;
    }
    cap_ = n;
    ++g_live[Mem::kind];
    return 0;
  }
  // Grow-only; contents are never preserved, and a failure leaves the capacity at zero.
  int reserve(size_t n) { return p_ && n <= cap_ ? 0 : alloc(n); }
  void reset() {
    if (p_) Mem::put((void*)p_), --g_live[Mem::kind];
    p_ = nullptr, cap_ = 0;
  }
  T* release() {
    T* p = p_;
    if (p) --g_live[Mem::kind];
    p_ = nullptr, cap_ = 0;
    return p;
  }
  // Takes n elements at p obtained elsewhere (freed like its own).
  void adopt(T* p, size_t n) {
    if (p) ++g_live[Mem::kind];
    adopt_counted(p, n);
  }

 private:
  void adopt_counted(T* p, size_t n) {
    reset();
    p_ = p, cap_ = p ? n : 0;
  }
  T* p_ = nullptr;
  size_t cap_ = 0;
};
template <typename T>
using DevBuf = Buf<T, DeviceMem>;
template <typename T>
using PinnedBuf = Buf<T, PinnedMem>;

class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s_) (void)hipStreamDestroy(s_), --g_live[kLiveStream];
  }
  operator hipStream_t() const { return s_; }
  int create() {   // once; non-blocking
    HIP_TRY(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
    ++g_live[kLiveStream];
    return 0;
  }

 private:
  hipStream_t s_ = nullptr;
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) reset(), e_ = o.e_, o.e_ = nullptr;
    return *this;
  }
  ~Event() { reset(); }
  operator hipEvent_t() const { return e_; }
  int create(unsigned flags = hipEventDefault) {
    reset();
    HIP_TRY(hipEventCreateWithFlags(&e_, flags));
    ++g_live[kLiveEvent];
    return 0;
  }
  void reset() {
    if (e_) (void)hipEventDestroy(e_), --g_live[kLiveEvent];
    e_ = nullptr;
  }

 private:
  hipEvent_t e_ = nullptr;
};

// A device pointer parameter whose T is deduced from the host pointer beside it, so that a
// DevBuf<T> converts where it is passed.
template <typename T>
struct NoDeduce { using type = T; };
template <typename T>
using DevPtr = typename NoDeduce<T>::type*;

// Queued on st: the source must outlive the stream's next synchronisation.
template <typename T>
int h2d(DevPtr<T> d, const T* h, size_t n, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, st));
  return 0;
}

// d becomes n elements holding h (queued on st, like h2d).
template <typename T>
int upload(DevBuf<T>& d, const T* h, size_t n, hipStream_t st) {
  TRY(d.alloc(n));
  return n ? h2d(d.get(), h, n, st) : 0;
}
template <typename T>
int upload(DevBuf<T>& d, const std::vector<T>& h, hipStream_t st) {
  return upload(d, h.data(), h.size(), st);
}

// One post-processing call on one stream: owns what the call allocates, keeps the first error
// (every later step is then a no-op), times the kernels on request, and ends in finish().
//   DeviceCall call(st, "observation");          // `what` names the call in its messages
//   const double* d_x = call.upload(x, n);       // null for a null host pointer
//   double* d_y = call.alloc<double>(n);
//   call.begin(kernel_ms);
//   if (call.ok()) { kernel<<<..., st>>>(...); }
//   call.end();
//   call.download(y, d_y, n);
//   call.keep(d_y);                              // optional: d_y outlives a successful finish()
//   return call.finish();
// Host arrays passed to upload() and download() must live until finish() returns.
class DeviceCall {
 public:
  DeviceCall(hipStream_t st, const char* what) : st_(st), what_(what) {}
  DeviceCall(const DeviceCall&) = delete;
  DeviceCall& operator=(const DeviceCall&) = delete;
  ~DeviceCall() { finish(); }

  bool ok() const { return rc_ == 0; }
  // Takes the status of a step done outside (a handle's own buffer growing, say).
  void check(int rc) {
    if (rc && !rc_) rc_ = rc;
  }

  template <typename T>
  T* alloc(size_t n) {
    if (rc_) return nullptr;
    owned_.emplace_back();
    rc_ = owned_.back().alloc(n * sizeof(T));
    return reinterpret_cast<T*>(owned_.back().get());
  }
  template <typename T>
  T* upload(const T* host, size_t n) {
    T* p = host ? alloc<T>(n) : nullptr;
    if (p) copy_in(p, host, n);
    return p;
  }
  // Into a buffer the call does not own.
  template <typename T>
  void copy_in(DevPtr<T> dev, const T* host, size_t n) {
    if (!rc_) rc_ = h2d(dev, host, n, st_);
  }
  template <typename T>
  void download(T* host, DevPtr<const T> dev, size_t n) {
    if (!rc_ && host &&
        hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st_) != hipSuccess)
      rc_ = set_error(what_ + " copy failed");
  }

  // Around the launches.  *ms receives the kernels' time in finish(), 0 after a failure; a
  // null ms times nothing.  end() also collects a failed launch.  A timed call waits for its
  // second event there: a read-back queued behind kernels still running adds 1 to 3 µs to the
  // events' interval (MI355X, profiles/r13/post_scaffold).
  void begin(double* ms) {
    if (rc_ || !ms) return;
    ms_ = ms;
    *ms_ = 0.0;
    if (ev_[0].create() || ev_[1].create() || hipEventRecord(ev_[0], st_) != hipSuccess)
      rc_ = set_error(what_ + ": timing event failed");
  }
  void end() {
    if (rc_) return;
    if (hipGetLastError() != hipSuccess)
      rc_ = set_error(what_ + " kernel launch failed");
    else if (ms_ && (hipEventRecord(ev_[1], st_) != hipSuccess ||
                     hipEventSynchronize(ev_[1]) != hipSuccess))
      rc_ = set_error(what_ + ": timing event failed");
  }

  // p (from alloc; null is ignored) outlives a successful finish() as the caller's, who adopts
  // it into a DevBuf; a failed one frees it.  Any number of buffers may be kept.
  void keep(void* p) {
    if (p) kept_.push_back(p);
  }

  // Synchronises the stream, reads the timer, destroys the events, frees what the call owns
  // and returns the status.
  int finish() {
    if (done_) return rc_;
    done_ = true;
    if (hipStreamSynchronize(st_) != hipSuccess && !rc_) rc_ = set_error(what_ + " kernel failed");
    float ms = 0.f;
    if (!rc_ && ms_ && hipEventElapsedTime(&ms, ev_[0], ev_[1]) == hipSuccess) *ms_ = ms;
    for (Event& e : ev_) e.reset();
    for (DevBuf<char>& b : owned_)
      if (!rc_ && std::find(kept_.begin(), kept_.end(), (void*)b.get()) != kept_.end())
        (void)b.release();
    owned_.clear();
    if (rc_) (void)hipGetLastError();   // a failed allocation must not fail the next call's checks
    return rc_;
  }

 private:
  hipStream_t st_;
  std::string what_;
  int rc_ = 0;
  bool done_ = false;
  double* ms_ = nullptr;
  Event ev_[2];
  std::vector<DevBuf<char>> owned_;
  std::vector<void*> kept_;
};

// Where a consumer (an instrument, a correlator, a broadener, an interpolator's library) reads
// its spectra x[n_atm][n_lam]: the caller's host array (rows stays null: the caller uploads x), a
// context's emergent rows in place, what a broadener kept (K13), what an interpolator kept
// (K15: its queries are the atmospheres) or what a phase integrator kept (K16: its phases are).
// `noun` is the consumer in the messages, `entry` its C entry point.
struct SpectrumRows {
  const double* rows;
  int64_t stride;
  hipStream_t stream;
};

inline int spectrum_rows(const double* x, frei_ctx* ctx, frei_brd* brd, frei_itp* itp,
                         frei_phs* phs, int n_atm, int64_t n_lam, int device, hipStream_t own,
                         const std::string& noun, const std::string& entry, SpectrumRows* out) {
  *out = SpectrumRows{nullptr, n_lam, own};
  const std::string N = std::to_string(n_atm);
  if (phs) {
    const std::string e = entry + "_phs: ";
    PhsRows pr{};
    TRY(phs_kept_rows(phs, &pr));
    if (!pr.rows) return set_error(e + "the phase integrator holds nothing kept (apply with keep)");
    if (pr.n_lam != n_lam)
      return set_error(e + "the phase integrator's n_lam = " + std::to_string(pr.n_lam) +
                       " is not the " + noun + "'s " + std::to_string(n_lam));
    if (pr.n_phase != n_atm)
      return set_error(e + "the phase integrator keeps " + std::to_string(pr.n_phase) +
                       " phases, not n_atm = " + N);
    if (pr.device != device)
      return set_error(e + "phase integrator and " + noun + " live on different devices");
    out->rows = pr.rows;
  } else if (itp) {
    const std::string e = entry + "_itp: ";
    ItpRows ir{};
    TRY(itp_kept_rows(itp, &ir));
    if (!ir.rows) return set_error(e + "the interpolator holds nothing kept (apply with keep)");
    if (ir.n_lam != n_lam)
      return set_error(e + "the interpolator's n_lam = " + std::to_string(ir.n_lam) +
                       " is not the " + noun + "'s " + std::to_string(n_lam));
    if (ir.n_query != n_atm)
      return set_error(e + "the interpolator keeps " + std::to_string(ir.n_query) +
                       " queries, not n_atm = " + N);
    if (ir.device != device)
      return set_error(e + "interpolator and " + noun + " live on different devices");
    out->rows = ir.rows;
  } else if (brd) {
    const std::string e = entry + "_brd: ";
    BrdRows br{};
    TRY(brd_kept_rows(brd, &br));
    if (!br.rows) return set_error(e + "the broadener holds nothing kept (apply with keep)");
    if (br.n_lam != n_lam)
      return set_error(e + "the broadener's n_lam = " + std::to_string(br.n_lam) + " is not the " +
                       noun + "'s " + std::to_string(n_lam));
    if (br.n_atm != n_atm)
      return set_error(e + "the broadener keeps " + std::to_string(br.n_atm) +
                       " atmospheres, not n_atm = " + N);
    if (br.device != device)
      return set_error(e + "broadener and " + noun + " live on different devices");
    out->rows = br.rows;
  } else if (!x) {
    CtxRows cr{};
    TRY(ctx_emergent_rows(ctx, &cr));
    if (cr.n_atm != n_atm)
      return set_error(entry + ": the context holds " + std::to_string(cr.n_atm) +
                       " atmospheres, not n_atm = " + N);
    if (cr.n_lam != n_lam)
      return set_error(entry + ": the context's n_lam = " + std::to_string(cr.n_lam) +
                       " is not the " + noun + "'s " + std::to_string(n_lam));
    if (cr.device != device)
      return set_error(entry + ": context and " + noun + " live on different devices");
    // the context's own stream where its spectra are read in place: ordered behind its work
    *out = SpectrumRows{cr.rows, cr.stride, cr.stream};
  }
  return 0;
}

inline int check_select(const std::string& name, const int32_t* select, int n_atm, int n_lib) {
  for (int m = 0; select && m < n_atm; ++m)
    if (select[m] < 0 || select[m] >= n_lib)
      return set_error(name + ": select[" + std::to_string(m) + "] = " +
                       std::to_string(select[m]) + " lies outside [0, n_lib = " +
                       std::to_string(n_lib) + ")");
  return 0;
}

}  // namespace frei

// One species' high-resolution cross-section resident in HBM (include/frei_hip.h): uploaded or
// generated by frei_binning.hip, computed from a line list by frei_lines.hip (K17), binned by K6.
struct frei_xsec {
  frei::Stream stream;           // first: destroyed after everything queued on it is freed
  int device = 0;
  int nT = 0, np = 0;
  int64_t nhi = 0;
  std::vector<double> T, p, wl;  // K, bar, µm (ascending)
  frei::DevBuf<float> d_x;          // [nT][np][nhi]
  frei::DevBuf<double> d_hdx;       // 0.5 * (wl[i+1] - wl[i]), exact mode (lazy)
  frei::DevBuf<double> d_scratch;   // output of frei_xsec_bin(out = NULL), grow-only
  bool timing = false;
  double t_ms = 0;
  int t_n = 0;
  // the per-call plan arrays, kept between calls (slot k, in bytes, grow-only): no allocation
  // per binning call
  std::vector<frei::DevBuf<char>> plan;
  // pinned host staging of the plan uploads (DMA copies; pageable hipMemcpyAsync stalled the
  // next kernel launch by milliseconds)
  frei::PinnedBuf<char> pinned;
  size_t pinned_used = 0;
  ~frei_xsec() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};
