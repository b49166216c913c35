// frei_host.h — the host code every translation unit's C entry points share: the error macros,
// device allocation and copies, the scaffold of one post-processing call (DeviceCall) and the
// resolution of a spectrum's sources.  Host code only; a new post-processing call starts
// from DeviceCall and spectrum_rows ("Host scaffold").
#pragma once
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

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}

// Queued on st: the source must outlive the stream's next synchronisation.
template <typename T>
int h2d(T* d, const T* h, size_t n, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, st));
  return 0;
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
    T* p = nullptr;
    if (rc_ || (rc_ = dalloc(&p, n))) return nullptr;
    owned_.push_back(p);
    return p;
  }
  template <typename T>
  T* upload(const T* host, size_t n) {
    T* p = host ? alloc<T>(n) : nullptr;
    if (p) copy_in(p, host, n);
    return p;
  }
  // Into a buffer the call does not own.
  template <typename T>
  void copy_in(T* dev, const T* host, size_t n) {
    if (!rc_) rc_ = h2d(dev, host, n, st_);
  }
  template <typename T>
  void download(T* host, const T* dev, size_t n) {
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
    if (hipEventCreate(&ev_[0]) != hipSuccess || hipEventCreate(&ev_[1]) != hipSuccess ||
        hipEventRecord(ev_[0], st_) != hipSuccess)
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

  // p (from alloc; null is ignored) outlives a successful finish() as the caller's; a failed
  // one frees it.  Any number of buffers may be kept.
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
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
    for (void* p : owned_)
      if (rc_ || std::find(kept_.begin(), kept_.end(), p) == kept_.end()) (void)hipFree(p);
    if (rc_) (void)hipGetLastError();   // a failed allocation must not fail the next call's checks
    return rc_;
  }

 private:
  hipStream_t st_;
  std::string what_;
  int rc_ = 0;
  bool done_ = false;
  double* ms_ = nullptr;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  std::vector<void*> owned_;
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
