// frei_runtime.hip — native runtime and C ABI (include/frei_hip.h) of the frei MI355X engine.
//
// Owns device memory, the HIP stream, the device-resident T-P loop driver (frei_run:
// core.py:233-338), and the optional RCCL exchange of per-sweep bolometric partial sums
// (one ncclAllGather of n_layers*4 doubles per sweep).
#include <dlfcn.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/frei_hip.h"
#include "frei_host.h"

using namespace frei;

namespace {

thread_local std::string g_err;

int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

}  // namespace

namespace frei {
int set_error(const std::string& msg) { return fail(msg); }
}  // namespace frei

namespace {

// ---------------------------------------------------------------- RCCL (dlopen)
struct Rccl {
  void* h = nullptr;
  typedef int (*GetId)(void*);
  typedef int (*InitRank)(void**, int, /*ncclUniqueId by value*/ struct Id128, int);
  int (*getUniqueId)(void*) = nullptr;
  int (*commInitRank)(void**, int, struct Id128, int) = nullptr;
  int (*allGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*commDestroy)(void*) = nullptr;
  const char* (*errStr)(int) = nullptr;
};
struct Id128 { char b[128]; };

Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    r.h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!r.h) r.h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (r.h) {
      r.getUniqueId = (int (*)(void*))dlsym(r.h, "ncclGetUniqueId");
      r.commInitRank = (int (*)(void**, int, Id128, int))dlsym(r.h, "ncclCommInitRank");
      r.allGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(
          r.h, "ncclAllGather");
      r.commDestroy = (int (*)(void*))dlsym(r.h, "ncclCommDestroy");
      r.errStr = (const char* (*)(int))dlsym(r.h, "ncclGetErrorString");
    }
  }
  return (r.h && r.getUniqueId && r.commInitRank && r.allGather) ? &r : nullptr;
}
constexpr int kNcclFloat64 = 8;

struct Species {
  DevBuf<double> d_tab;
  int n_p = 0, n_T = 0;
  int has_nan = 1;     // set by a device scan after upload/generation
  int64_t stride = 0;  // row pitch in elements (n_lam rounded up to 64, zero padded)
  std::vector<double> p_nodes, T_nodes;
  std::vector<int32_t> rank;   // [n_T] storage row (T ascending) of the caller's node kt
};

// Element offset in q's table of the row of the caller's node (kp, kt).
int64_t node_offset(const Species& q, int kp, int kt) {
  return ((int64_t)kp * q.n_T + q.rank[kt]) * q.stride;
}

}  // namespace

struct frei_ctx {
  Stream stream;   // first: destroyed last, after every buffer and event
  int device = 0;
  int nL = 0, S = 0;
  int64_t nlam = 0;
  int nblocks = 0;
  // grid
  DevBuf<double> d_c1, d_hcl, d_sig, d_ftoa, d_wtr, d_p, d_lnp;
  std::vector<double> p;
  double p_top2 = 0, g = 0, m_bar = 0;
  bool grid_set = false;
  // state
  DevBuf<double> d_Fu, d_Fd, d_dT, d_dtaus, d_bol;
  // the fused reduce + update writes the new temperatures into the other buffer and the two
  // swap (d_T is always the current one); d_done: its arrival counter.  The three temperature
  // buffers are owned by T_buf; d_T, d_T_alt, d_T3 and d_T_home are views that rotate over them
  DevBuf<double> T_buf[3];
  double* d_T = nullptr;
  double* d_T_alt = nullptr;
  double* d_T3 = nullptr;               // third temperature buffer (chained launches)
  double* d_T_home = nullptr;           // the buffer d_T names after a host upload
  // Chained launches (FREI_CHAIN): a sweep's fused update is deferred and runs as the leading
  // workgroups of the next sweep's launch (launch_sweep_chain)
  int chain = 1;                        // FREI_CHAIN
  bool has_pend = false;                // an update deferred to the next launch
  UpdateArgs pend{};
  DevBuf<unsigned long long> d_epoch;     // [n_layers] the chained update's per-layer granules
  unsigned long long chain_seq = 0;
  DevBuf<int> d_chain_err;              // a chained sweep block's wait gave up
  DevBuf<unsigned> d_done;
  int fused_update = 1;                 // FREI_FUSED_UPDATE=0: separate reduce and update kernels
  // T-P iterations replayed from a captured hipGraph (frei_iterate / frei_run, timing off,
  // single rank): g_key holds the hashes of one iteration's kernel arguments; any change
  // (pointers, options, loop parameters) re-captures.  Off by default (FREI_GRAPH=1 turns it
  // on): measured no faster than stream launches, whose dispatch already overlaps the
  // previous kernel (profiles/r02_ab_graph.txt).
  int use_graph = 0;
  int graph_iters = 4;                  // iterations per captured graph
  hipGraphExec_t g_exec = nullptr;
  std::vector<uint64_t> g_key;
  int g_captures = 0, g_replays = 0;     // frei_graph_info
  int64_t n_chained = 0;                // chained sweep launches so far (frei_chain_info)
  // Trailing update (FREI_TAIL, round 6): the producer/consumer sweep's launch carries its own
  // fused update as trailing workgroups that reduce each layer as soon as the sweep has
  // published its steps (launch_sweep_pipe_tail).  Two partial-sum buffers used alternately:
  // a launch publishes into one and its update workgroups put the other back to kPoisonT.
  int tail = 1;                         // FREI_TAIL: 1 when it applies, 0 off
  DevBuf<double> d_tpart;               // [2][tpart_n]
  int64_t tpart_n = 0;
  int tpart_parity = 0;
  bool tpart_fill = true;               // both buffers must be (re)filled with kPoisonT
  int64_t n_tail = 0;                   // trailing-update launches so far (frei_tail_info)
  bool shared_device = false;           // ranks share this GPU: no chained launches
  std::vector<uint64_t>* keys = nullptr;  // collecting run_sweep's argument hashes
  bool dry = false;                       // run_sweep computes hashes only (no launches)
  // tables
  std::vector<Species> sp;
  std::vector<double> mmr;
  bool meta_dirty = true;
  bool mmr_dirty = false;               // only the mixing ratios changed (per-sweep provider)
  int fast = 1;
  DevBuf<SpecMeta> d_smeta;
  DevBuf<PMeta> d_pmeta;
  DevBuf<double> d_tnodes;
  DevBuf<int32_t> d_tperm;
  DevBuf<double> d_mmr;
  std::vector<SpecMeta> smeta;
  std::vector<PMeta> pmeta;
  std::vector<double> tnodes;
  std::vector<int32_t> tperm;
  // sweep scratch
  DevBuf<StepP> d_steps;
  DevBuf<TermP> d_terms;
  DevBuf<FastStep> d_fsteps;
  DevBuf<FastStepS> d_ssteps;
  int shared = 0;   // fast path with one bracket for all species (identical nodes)
  // Species-contracted table (K3): with shared nodes, no NaN and fixed per-layer mmr the
  // sweep reads eff[p][t][:] = sum_s mmr_s(l) tab_s[p][t][:] (2 rows per layer, not 2 S).
  // FREI_PRECONTRACT=0 keeps the per-species sum inside the sweep.
  int eff = 0, eff_mode = -1;
  DevBuf<double> d_eff;   // grow-only
  // Lazy K3 (FREI_LAZY_K3, round 6): with the two-wavelength sweep, the setup contracts no row;
  // a sweep contracts the rows its records mask as missing (the lane's own wavelengths), and the
  // update after it marks them (d_kvalid).  A run touches a fraction of the table's T nodes (C3
  // to radiative equilibrium: 191 of 960 rows).  Any other sweep form first contracts the
  // whole table (eff_complete).
  int lazy_k3 = 1;
  bool lazy_on = false;
  bool eff_complete = true;
  DevBuf<int32_t> d_kvalid;
  DevBuf<SpecMeta> d_smeta_eff;
  DevBuf<double> d_ones;
  DevBuf<int32_t> d_prow;
  bool dtaus_valid = false;  // d_dtaus holds the last frei_run's final-emit dtaus
  // Batched atmospheres (frei_ctx_create_batch): n_atm atmospheres share the wavelength and
  // pressure grids and the opacity tables; every per-atmosphere buffer is n_atm blocks.
  int n_atm = 1;
  DevBuf<double> d_g;         // [n_atm] gravity (batched)
  size_t eff_stride = 0;      // elements per atmosphere of d_eff
  PinnedBuf<int> h_conv;      // pinned [2][n_atm] convergence flags (frei_run_batch)
  bool batch_api = false;     // created through frei_ctx_create_batch (n_atm may be 1)
  // d_dtaus holds every atmosphere's final-emit dtaus [n_atm][nL][nlam] of the last
  // frei_run_batch_ex(keep_dtaus) and d_T / d_Fu are still that run's (frei_post_batch)
  bool dtaus_batch_valid = false;
  double post_ms = 0.0;       // HIP-event time of the last post-processing call's kernels
  DevBuf<double> d_part, d_Fb, d_Fb_all;
  // T-P loop state
  DevBuf<int> d_conv;
  DevBuf<int> d_iter;
  DevBuf<double> d_Tb, d_Ta, d_hist;
  int hist_cap = 0;
  DevBuf<int32_t> d_flips, d_prev, d_ndiff;
  PinnedBuf<int> h_flag;  // pinned [2]
  PinnedBuf<int> h_err;   // pinned [2]: the chained-poll and P2P error flags (check_comm)
  // pinned staging of the per-sweep host round trip of a chemistry provider stepping the loop
  // (frei_get_temperatures, frei_sweep's dT / bolometric sums, frei_set_mmr's upload): one
  // stream synchronisation per read, none for the upload (pageable copies add their own)
  PinnedBuf<double> h_T;     // [n_layers * n_atm]
  PinnedBuf<double> h_dT;    // [n_layers]
  PinnedBuf<double> h_bol;   // [n_layers * 4]
  PinnedBuf<double> h_mmr;   // [n_species * n_layers * n_atm]
  Event mmr_ev;              // the last upload from h_mmr
  bool mmr_ev_set = false;
  int64_t chain_checked = 0;   // n_chained at the last check_comm
  Event flag_ev[2];
  // comm
  void* comm = nullptr;
  int nranks = 1, rank = 0;
  int prefetch_depth = 0;               // 0 = automatic (FREI_PREFETCH_DEPTH overrides)
  int k7_mfma = 1;                      // FREI_K7_MFMA: batched contraction on MFMA (1) or VALU (0)
  int prefetch_steps = 0;               // FREI_PREFETCH_STEPS: contracted one-lane sweep's load
                                        // distance in steps (0 = automatic, 8 / 16 = deeper)
  // Shared-bracket kernel (step table staged in LDS): used when every species shares its
  // nodes AND the slice is small (nblocks <= shared_max_blocks, about one resident round of
  // blocks), where each CU runs ~1 block and the per-step scalar loads would miss the K$.
  // FREI_SHARED=0/1 forces it off/on; FREI_SHARED_MAX_BLOCKS moves the threshold.
  int shared_mode = -1;
  int shared_max_blocks = 640;          // <= 164k lambda (125k: LDS 4 % faster; 164k tie; 250k: global 1 % faster)
  // Grouped-lane sweep (2 or 4 lanes per wavelength): contracted table, LDS step table and
  // at most this many 256-wavelength blocks, i.e. about one wave per SIMD or less.
  int pair_max_blocks = 420;            // FREI_PAIR_MAX_BLOCKS (<= 107k lambda per GPU)
  int quad_max_blocks = 208;            // FREI_QUAD_MAX_BLOCKS (<= 53k lambda per GPU)
  int group_q = 0;                      // FREI_GROUP_Q forces 1, 2 or 4 lanes per wavelength
  int pipe_nc = -1;                     // FREI_PIPE: producer/consumer sweep, 1/2/4 consumers per
                                        // block, 0 off, -1 by slice size (pipe_*_blocks; the
                                        // default again since its roles were balanced over the
                                        // SIMDs: -2 % per T-P iteration at 62.5k with P2P vs
                                        // the chained grouped-lane form, profiles/r03/chain/)
  int pipe_min_blocks = 208;            // FREI_PIPE_MIN_BLOCKS / _MAX_BLOCKS: 256-wavelength
  int pipe_max_blocks = -1;             // blocks per GPU where the auto choice takes NC = 4
                                        // (-1: the CU count, one 16-wave block per CU)
  int n_cu = 256;                       // hipDeviceProp multiProcessorCount
  int rec_sweep = -1;                   // FREI_REC_SWEEP: sweeps form their own step records
                                        // (1 every form, 0 never, -1 single-atmosphere contexts
                                        // without the producer/consumer sweep)
  bool rec_skipped = false;             // the last update wrote no records (the sweep did)
  int pipe_m = 2;                       // steps per producer and phase
  int pipe_pf = 1;                      // FREI_PIPE_PF: phases the producers load ahead (1, 2)
  int red_rows = 1;                     // FREI_RED_ROWS=0: full wave sums per step
  int red_stage = 1;                    // FREI_RED_STAGE=0: no staged sums (one-lane sweep)
  int lam2 = -1;                        // FREI_LAM2: two wavelengths per lane in the contracted
                                        // one-lane sweep (1 on, 0 off, -1 large slices)
  int sweep_lds_kb = 0;                 // FREI_SWEEP_LDS_KB: minimum LDS per sweep block (KiB)
  int group_waves = 4;                  // FREI_GROUP_WAVES: waves per grouped-lane sweep block
  int depth4_max_blocks = 0;            // FREI_DEPTH4_MAX_BLOCKS (4 steps in flight: off, measured no faster)
  size_t lds_per_block = 64 * 1024;     // hipDeviceProp sharedMemPerBlock
  size_t lds_optin = 64 * 1024;         // with the dynamic-LDS opt-in (gfx950: 160 KiB)
  bool ftoa_per_atm = false;            // batched: one F_TOA per atmosphere (frei_set_ftoa_batch)
  double setup_ms[5] = {0, 0, 0, 0, 0};  // last metadata build, by phase (frei_setup_timing)
  double contract_ms = 0.0;     // last K3 / K7 kernel, HIP events (frei_contract_timing)
  double contract_bytes = 0.0;  // its algorithmic HBM bytes
  // T-dependent chemistry (frei_set_chemistry): mmr tables on (T, p) nodes
  bool chem_on = false;
  int chem_nT = 0, chem_np = 0;
  std::vector<double> chem_tab, chem_T, chem_logp;   // host copies (frei_kappa)
  DevBuf<double> d_chem_tab, d_chem_T, d_chem_pz;
  DevBuf<int32_t> d_chem_pj;
  // batched contexts (frei_set_chemistry_batch): chem_ntab tables, atmosphere m reads table
  // chem_atm[m] (empty: one table for the context, frei_set_chemistry)
  int chem_ntab = 1;
  std::vector<int32_t> chem_atm;
  DevBuf<int32_t> d_chem_atm;
  // Atmosphere-tiled per-species sweep of a chemistry batch (sweep_tile_kernel): atmospheres
  // per block, FREI_ATM_TILE 1 (one block per (wavelength block, atmosphere): the one-lane
  // per-species sweep), 2, 4 or -1 = automatic; tile: the width the last metadata build chose
  // (0: not a chemistry batch)
  int atm_tile = -1;
  int tile = 0;
  // K20, a k-mix batch (frei_set_table_kmix_batch): the k(g) of several species do not add, so
  // atmosphere m's table in d_eff is the random-overlap mixture (K19) of its own composition
  // kmix_x[m], written by the K19 kernels through a row list instead of K7's species sum.  Only
  // the pressure rows some layer sits on (kmix_used) are mixed.  kmix_lib is the caller's and
  // must outlive the context's use of it.
  frei_klib* kmix_lib = nullptr;
  std::vector<double> kmix_x;        // [n_atm][n_src][n_p][n_T]
  int64_t kmix_col_lo = 0;
  int kmix_nsrc = 0;
  std::vector<char> kmix_used;       // [n_p] a layer sits on the row (the last metadata build)
  // P2P exchange over xGMI (frei_comm_p2p_*): own mailbox (uncached device memory), the
  // mapped mailboxes of every rank (own included) and the per-sweep sequence number
  DevBuf<double> d_mbox;                 // (adopted: allocated uncached)
  DevBuf<double*> d_peers;
  std::vector<void*> peer_mapped;        // IPC mappings to close (not allocations)
  uint64_t p2p_seq = 0;
  DevBuf<int> d_comm_err;                // set by a kernel when a peer never published
  DevBuf<unsigned long long> d_wait_ticks;
  double p2p_timeout_s = 30.0;           // FREI_P2P_TIMEOUT_S
  frei_allgather_fn host_ag = nullptr;  // host all-gather callback (alternative to RCCL)
  void* host_ag_user = nullptr;
  PinnedBuf<double> h_ag;               // pinned [nranks + 1][n_steps * 4]
  // timing
  bool timing = false;
  std::vector<Event> ev_pool;
  size_t ev_used = 0;
  std::vector<Event> xev_pool;          // around the rank exchange (all-gather) of each sweep
  size_t xev_used = 0;
  ~frei_ctx();
};

namespace {

int set_device(frei_ctx* c) {
  HIP_TRY(hipSetDevice(c->device));
  return 0;
}

// A setup or per-run upload (never inside the T-P loop) that waits for the copy: the sources are
// often temporaries (pageable, freed at the caller's scope exit).
template <typename T>
int h2d_wait(DevPtr<T> d, const T* h, size_t n, hipStream_t st) {
  TRY(h2d(d, h, n, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// Species contraction (K3) when every species shares its nodes (one bracket per layer), no
// table holds a NaN (the reference's nansum, Q8, is per species) and S >= 2.
// two wavelengths per lane from this many one-lane blocks per launch (all atmospheres of a
// batched launch): about 1.1 rounds of the one-lane form at five waves per SIMD
constexpr int kLam2MinBlocks = 1400;
bool lam2_blocks(const frei_ctx* c) {
  return (int64_t)c->nblocks * (c->n_atm > 1 ? c->n_atm : 1) >= kLam2MinBlocks;
}

// Staged partial sums (red_rows 2): the per-wave LDS tile plus one row per wave and the step
// table within 48 KiB (deep atmospheres, above ~160 steps, do not fit).
bool staged_sums_fit(int ns) {
  return ((size_t)(kBlock / 64) * ns * 4 + (size_t)(kBlock / 64) * 2 * 4 * 72) * sizeof(double) +
             (size_t)ns * sizeof(FastStepS) <= 48 * 1024;
}
// Prefetch depth of the one-lane sweep: below ~2 waves per SIMD (small per-GPU slices, e.g. 500k
// lambda over 8 GPUs) a second layer in flight hides HBM latency; at full occupancy one suffices.
// With one table (K3) and few blocks per CU, four steps in flight add the instruction-level
// parallelism that occupancy cannot (FREI_DEPTH4_MAX_BLOCKS).
int sweep_depth(const frei_ctx* c, int S_run) {
  return c->prefetch_depth > 0 ? c->prefetch_depth
         : (S_run == 1 && c->nblocks <= c->depth4_max_blocks) ? 4 : 2;
}
// Loads issued pf steps ahead (the contracted table only; 0: the coefficient block's depth;
// prefetch_steps 2 with depth 1: one step per coefficient block, loads two steps ahead).
int sweep_pf(const frei_ctx* c, bool eff, int S_run, int depth) {
  return (eff && S_run == 1 && (depth >= 2 || c->prefetch_steps == 2)) ? c->prefetch_steps : 0;
}
// The two-wavelength sweep's requirements besides the contracted NaN-free table, one lane per
// wavelength, global step records and no chained launch: an even slice, enough one-lane blocks
// (or FREI_LAM2=1), a depth-2 coefficient block loading at most two steps ahead, and the staged
// partial sums.  The sweep's plan (sweep_plan) and the batched step-table choice (build_meta,
// which runs before the contracted table the plan needs exists) decide by it.
bool lam2_static(const frei_ctx* c, int depth, int pf) {
  return c->lam2 != 0 && c->nlam % 2 == 0 && (c->lam2 > 0 || lam2_blocks(c)) && depth == 2 &&
         pf <= 2 && c->red_stage && staged_sums_fit(c->nL - 1);
}

// What one sweep launches, decided in one place (sweep_plan, below): run_sweep launches from it,
// frei_ctx_path reports it, build_contracted asks it whether the lazy contraction applies and
// the graph-replay key hashes it (all int: no padding bytes).
enum SweepForm : int { kGeneric = 0, kOneLane, kTiled, kLam2, kGrouped, kPipe };
struct SweepPlan {
  int form;        // SweepForm
  int chain;       // chained launches apply to this context's sweeps
  int merge;       // chained: this launch's leading workgroups run the pending update
  int defer_own;   // chained: this sweep's own update waits for the next launch
  int tail_nT;     // update workgroups trailing the producer/consumer sweep (0: none)
  int S_run, depth, pf, Q, NW, NC, pipe_pf, red_rows;
  int nan_check;   // the per-species sweep tests for NaN (never on the contracted table)
  int lds_steps;   // shared-bracket step records (one bracket for all species)
  int tile;        // atmospheres per block of the tiled form
  int rec_on;      // the sweep forms its own step records
  int fused;       // reduce + update in one launch
  int nb_run;      // partial-sum columns the sweep writes
  int whole_table; // lazy K3: every row must be contracted before this sweep
};
SweepPlan sweep_plan(const frei_ctx* c, bool pending, bool defer);

// Atmospheres per block of a chemistry batch's sweep (0: not a chemistry batch).  The tiled
// kernel is instantiated for S = 2..8 and reduces with the staged sums of the one-lane sweep it
// must equal bit for bit (two steps in flight, red_stage); its LDS (one partial-sum block per
// atmosphere) must fit 64 KiB.  Anything else takes the one-lane per-species sweep over
// (block, atmosphere).  Automatic: the widest tile that still leaves the launch one resident
// round of blocks (four per CU) — measured at 32 x 100k lambda x 8 species, 4 atmospheres per
// block run 1.54x and 2 run 1.32x the rate of 1 (profiles/r07/batch_chem/, DESIGN.md §3 "K1,
// atmosphere-tiled"); a launch that a wider tile would leave with idle CUs was not measured
// and keeps the narrower one.
int atm_tile_width(const frei_ctx* c, bool shared_nodes) {
  if (!(c->n_atm > 1 && c->chem_on)) return 0;
  int t = c->atm_tile;
  if (t < 0) {
    const int64_t round = 4 * (int64_t)c->n_cu;
    t = 1;
    for (int w = 2; w <= 4; w *= 2)
      if ((int64_t)c->nblocks * ((c->n_atm + w - 1) / w) >= round) t = w;
  }
  const int ns = c->nL - 1;
  bool ok = c->fast && shared_nodes && c->S >= 2 && c->S <= kMaxFastS &&
            sweep_depth(c, c->S) == 2 && c->red_stage && staged_sums_fit(ns);
  for (int s = 0; s < c->S && ok; ++s) ok = !c->sp[s].has_nan;
  if (!ok) return 1;
  while (t > 1 && tile_lds_bytes(t, ns) > 64 * 1024) t /= 2;
  return t;
}

// Device NaN scan of n tables of len elements, table i at base + i * stride, on the context's
// stream: flag[i] (host) becomes nonzero when table i holds a NaN.  Returns when the stream has
// finished.
int scan_tables(frei_ctx* c, const double* base, size_t stride, int64_t len, int n, int* flag) {
  DeviceCall call(c->stream, "NaN scan");
  int* d_flag = call.alloc<int>((size_t)n);
  if (call.ok() && hipMemsetAsync(d_flag, 0, (size_t)n * sizeof(int), c->stream) != hipSuccess)
    call.check(fail("NaN scan: clearing the flags failed"));
  for (int i = 0; i < n && call.ok(); ++i)
    launch_nan_scan(base + (size_t)i * stride, len, d_flag + i, c->stream);
  call.end();
  call.download(flag, d_flag, (size_t)n);
  return call.finish();
}

// K20: the tables of the atmospheres [atm_lo, atm_lo + n) of a k-mix batch mixed into d_eff on
// the context's stream, each (used pressure row, T node) a row of K19's list (`me` prefixes the
// mixer's messages); then a NaN in any of them fails the call and names the first atmosphere.
// The rest of each table (the other rows, the column padding, the tail) is zero since the
// metadata build and is not touched.
int kmix_fill(frei_ctx* c, int atm_lo, int n, const std::string& me) {
  const Species& q0 = c->sp[0];
  std::vector<KmixRow> rows;
  for (int i = 0; i < n; ++i)
    for (int kp = 0; kp < q0.n_p; ++kp)
      for (int kt = 0; kt < q0.n_T && c->kmix_used[kp]; ++kt)
        rows.push_back(KmixRow{i, kp * q0.n_T + kt,
                               (int64_t)((size_t)(atm_lo + i) * c->eff_stride) +
                                   node_offset(q0, kp, kt)});
  const size_t per_x = (size_t)c->kmix_nsrc * q0.n_p * q0.n_T;
  TRY(kmix_rows_into(me, c->kmix_lib, n, c->kmix_x.data() + (size_t)atm_lo * per_x,
                     c->kmix_col_lo, c->nlam, rows.data(), rows.size(), c->d_eff, c->stream));
  std::vector<int> flag((size_t)n, 0);
  TRY(scan_tables(c, c->d_eff + (size_t)atm_lo * c->eff_stride, c->eff_stride,
                  (int64_t)q0.n_p * q0.n_T * q0.stride, n, flag.data()));
  for (int i = 0; i < n; ++i)
    if (flag[i])
      return fail("the mixed table of atmosphere " + std::to_string(atm_lo + i) +
                  " holds a NaN in a row a layer uses (a batched context needs tables without "
                  "NaN)");
  return 0;
}

template <typename Lap>
int build_contracted(frei_ctx* c, bool shared_fast, Lap&& lap) {
  const int nL = c->nL, S = c->S;
  c->lazy_on = false;        // (decided below, with the contracted table)
  c->eff_complete = true;
  const bool batch = c->n_atm > 1;
  // a k-mix batch (K20): species 0 carries the nodes (and composition 0's mixture, which a
  // context of one atmosphere sweeps as it is); the per-atmosphere tables are mixed below
  const bool kmix = batch && c->kmix_lib != nullptr;
  // (a T-dependent chemistry changes mmr every sweep: the species sum stays in the sweep)
  bool on = shared_fast && (S >= 2 || batch) && (c->eff_mode != 0 || batch) && !c->chem_on;
  for (int s = 0; s < S && on && !kmix; ++s) on = !c->sp[s].has_nan;
  std::vector<int32_t> prow(nL, 0);
  if (on) {
    std::vector<int> owner((size_t)c->sp[0].n_p, -1);
    for (int l = 0; l < nL && on; ++l) {
      const PMeta& pm = c->pmeta[l];  // species 0 (shared nodes)
      prow[l] = (pm.wp_lo != 0.0) ? pm.p_lo : pm.p_hi;
      if (owner[prow[l]] >= 0) {  // two layers on one pressure row: mmr must agree
        for (size_t m = 0; m < (size_t)c->n_atm && on; ++m)
          for (int s = 0; s < S && on; ++s)
            on = c->mmr[(m * S + s) * nL + l] == c->mmr[(m * S + s) * nL + owner[prow[l]]];
      }
      owner[prow[l]] = l;
    }
  }
  c->eff = on ? 1 : 0;
  if (!on) {
    // a chemistry batch (frei_set_chemistry_batch) contracts nothing and allocates no table,
    // but its sweeps read the per-species tables through one bracket per step all the same
    bool chem_batch = batch && c->chem_on && shared_fast;
    for (int s = 0; s < S && chem_batch; ++s) chem_batch = !c->sp[s].has_nan;
    if (batch && !chem_batch)
      return fail("a batched context needs tables on shared on-node p/T nodes without NaN "
                  "(one contracted table per atmosphere; chemistry batches need them too: "
                  "every atmosphere reads the species' tables through one shared bracket)");
    return 0;
  }
  const Species& q0 = c->sp[0];
  const size_t per = (size_t)q0.n_p * q0.n_T * (size_t)q0.stride + 64;
  const size_t need = per * c->n_atm;
  if (c->d_eff.capacity() < need) {
    HIP_TRY(hipStreamSynchronize(c->stream));   // no queued sweep still reads the old table
    TRY(c->d_eff.reserve(need));
  }
  lap(2);
  c->eff_stride = per;
  // the contraction writes every column (padding included) of the pressure rows the layers
  // use; only the other rows and each atmosphere's 64-element tail are zero-filled here (a
  // fill of the whole table would double the setup's HBM writes: 24.6 GB at C5)
  {
    const size_t rowblk = (size_t)q0.n_T * q0.stride;
    std::vector<char> used((size_t)q0.n_p, 0);
    for (int l = 0; l < nL; ++l) used[prow[l]] = 1;
    for (size_t m = 0; m < (size_t)c->n_atm; ++m) {
      double* base = c->d_eff + m * per;
      for (int p = 0; p < q0.n_p;) {
        if (used[p]) {
          ++p;
          continue;
        }
        int e = p;
        while (e < q0.n_p && !used[e]) ++e;
        HIP_TRY(hipMemsetAsync(base + (size_t)p * rowblk, 0,
                               (size_t)(e - p) * rowblk * sizeof(double), c->stream));
        p = e;
      }
      HIP_TRY(hipMemsetAsync(base + (size_t)q0.n_p * rowblk, 0, 64 * sizeof(double),
                             c->stream));
      // (K19 writes the n_lam columns of a row: the padding up to the pitch is cleared here)
      if (kmix && q0.stride > c->nlam)
        HIP_TRY(hipMemset2DAsync(base + c->nlam, (size_t)q0.stride * sizeof(double), 0,
                                 (size_t)(q0.stride - c->nlam) * sizeof(double),
                                 (size_t)q0.n_p * q0.n_T, c->stream));
    }
    if (kmix) c->kmix_used = used;
  }
  lap(3);
  if (!c->d_ones) {
    std::vector<double> ones(nL, 1.0);
    TRY(c->d_ones.alloc(nL));
    TRY(h2d_wait(c->d_ones, ones.data(), nL, c->stream));
  }
  TRY(c->d_prow.reserve(nL));
  TRY(h2d_wait(c->d_prow, prow.data(), nL, c->stream));
  const double* tabs[kMaxFastS];
  for (int s = 0; s < S; ++s) tabs[s] = c->sp[s].d_tab;
  // lazy K3: the sweeps that read this table take two wavelengths per lane (the form run_sweep
  // launches for a loop's sweeps), one atmosphere
  c->lazy_on = c->lazy_k3 && !batch && sweep_plan(c, false, false).form == kLam2;
  c->eff_complete = !c->lazy_on;
  if (c->lazy_on) {
    TRY(c->d_kvalid.reserve((size_t)q0.n_p * q0.n_T));
    HIP_TRY(hipMemsetAsync(c->d_kvalid, 0, (size_t)q0.n_p * q0.n_T * sizeof(int32_t),
                           c->stream));
    // a layer outside the hull reads rows 0 and 1 with zero weights: finite (zero) until then
    HIP_TRY(hipMemsetAsync(c->d_eff, 0, 2 * (size_t)q0.stride * sizeof(double), c->stream));
    c->contract_ms = 0.0;
    c->contract_bytes = 0.0;
    lap(4);
    SpecMeta m = c->smeta[0];
    m.tab = c->d_eff;
    if (!c->d_smeta_eff) TRY(c->d_smeta_eff.alloc(1));
    TRY(h2d_wait(c->d_smeta_eff, &m, 1, c->stream));
    return 0;
  }
  Event k0, k1;   // the contraction kernel alone (frei_contract_timing)
  if (k0.create() || k1.create()) return fail("hipEventCreate failed");
  HIP_TRY(hipEventRecord(k0, c->stream));
  if (kmix) {               // K20: K19's random-overlap mixture per atmosphere, not a species sum
    const int rc = kmix_fill(c, 0, c->n_atm, "k-mix batch tables: ");
    if (rc) return rc;
  } else if (batch && c->k7_mfma)  // K7: [n_atm x S] . [S x n_T*pitch] per layer on fp64 MFMA
    launch_contract_batch(tabs, S, c->d_mmr, c->d_prow, nL, q0.n_T, q0.stride, c->n_atm,
                          (int64_t)per, c->d_eff, c->stream);
  else if (batch)           // K7 on the VALU, K3's species order
    launch_contract_batch_valu(tabs, S, c->d_mmr, c->d_prow, nL, q0.n_T, q0.stride,
                               c->n_atm, (int64_t)per, c->d_eff, c->stream);
  else
    launch_contract(tabs, S, c->d_mmr, c->d_prow, nL, q0.n_T, q0.stride, c->d_eff, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(k1, c->stream));
  lap(4);
  {
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(k1));
    HIP_TRY(hipEventElapsedTime(&ms, k0, k1));
    c->contract_ms = ms;
    // bytes the launch must move: the S tables' used rows read once, n_atm tables written
    // (every column of the used rows, padding included)
    std::vector<char> used((size_t)q0.n_p, 0);
    for (int l = 0; l < nL; ++l) used[prow[l]] = 1;
    size_t rows = 0;
    for (char u : used) rows += u;
    const double rowbytes = (double)q0.n_T * q0.stride * sizeof(double);
    c->contract_bytes = rows * rowbytes * (S + c->n_atm);
  }
  SpecMeta m = c->smeta[0];
  m.tab = c->d_eff;
  if (!c->d_smeta_eff) TRY(c->d_smeta_eff.alloc(1));
  TRY(h2d_wait(c->d_smeta_eff, &m, 1, c->stream));
  return 0;
}

// Build the per-(species, layer) pressure brackets and upload all table metadata.
double now_ms() {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}

int build_meta(frei_ctx* c) {
  if (!c->meta_dirty) {
    if (c->mmr_dirty) {   // new mixing ratios only: up on the stream, ahead of the next sweep
      // (through pinned staging, no synchronisation: the previous upload from it has finished
      // once its event has)
      if (c->mmr_ev_set) HIP_TRY(hipEventSynchronize(c->mmr_ev));
      std::memcpy(c->h_mmr, c->mmr.data(), c->mmr.size() * sizeof(double));
      HIP_TRY(hipMemcpyAsync(c->d_mmr, c->h_mmr, c->mmr.size() * sizeof(double),
                             hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipEventRecord(c->mmr_ev, c->stream));
      c->mmr_ev_set = true;
      c->mmr_dirty = false;
    }
    return 0;
  }
  if (!c->grid_set) return fail("frei_set_grid must be called before using tables");
  double t_prev = now_ms();
  auto lap = [&](int k) {   // frei_setup_timing phases (host wall clock, stream synced)
    (void)hipStreamSynchronize(c->stream);
    const double t = now_ms();
    c->setup_ms[k] += t - t_prev;
    t_prev = t;
  };
  for (double& x : c->setup_ms) x = 0.0;
  const int nL = c->nL, S = c->S;
  c->smeta.assign(S, SpecMeta{});
  c->pmeta.assign((size_t)S * nL, PMeta{});
  c->tnodes.clear();
  c->tperm.clear();
  int fast = 1;
  for (int s = 0; s < S; ++s) {
    const Species& q = c->sp[s];
    if (!q.d_tab) return fail("opacity table of species " + std::to_string(s) + " not set");
    SpecMeta m{};
    m.tab = q.d_tab;
    m.n_lam = q.stride;
    m.n_p = q.n_p;
    m.n_T = q.n_T;
    m.t_off = (int32_t)c->tnodes.size();
    // sorted temperature nodes (xarray sortby) + permutation to memory rows
    std::vector<int32_t> perm(q.n_T);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(),
                     [&](int a, int b) { return q.T_nodes[a] < q.T_nodes[b]; });
    int n_unique = q.n_T > 0 ? 1 : 0;
    for (int k = 1; k < q.n_T; ++k)
      if (q.T_nodes[perm[k]] != q.T_nodes[perm[k - 1]]) ++n_unique;
    m.one_T = (n_unique <= 1) ? 1 : 0;
    if (!m.one_T && n_unique != q.n_T)
      return fail("duplicate temperature nodes (drop_duplicates first, opacity.py:339)");
    for (int k = 0; k < q.n_T; ++k) {
      c->tnodes.push_back(q.T_nodes[perm[k]]);
      c->tperm.push_back(perm[k]);
    }
    if (m.one_T) fast = 0;
    if (S > kMaxFastS) fast = 0;
    c->smeta[s] = m;
    // sorted pressure nodes + bracket of every layer pressure
    std::vector<int32_t> pp(q.n_p);
    std::iota(pp.begin(), pp.end(), 0);
    std::stable_sort(pp.begin(), pp.end(),
                     [&](int a, int b) { return q.p_nodes[a] < q.p_nodes[b]; });
    std::vector<double> ps(q.n_p);
    for (int k = 0; k < q.n_p; ++k) ps[k] = q.p_nodes[pp[k]];
    for (int l = 0; l < nL; ++l) {
      PMeta pm{};
      const double x = c->p[l];
      if (m.one_T) {
        // scipy interp1d: searchsorted(left) clipped to [1, n-1]
        int jx = (int)(std::lower_bound(ps.begin(), ps.end(), x) - ps.begin());
        jx = std::max(1, std::min(jx, q.n_p - 1));
        pm.p_lo = pp[jx - 1];
        pm.p_hi = pp[jx];
        pm.x1 = x - ps[jx - 1];
        pm.dx = ps[jx] - ps[jx - 1];
        pm.oob = (x < ps[0] || x > ps[q.n_p - 1]) ? 1 : 0;
      } else {
        int i, oob;
        double y;
        bracket(ps.data(), q.n_p, x, i, y, oob);
        pm.p_lo = pp[i];
        pm.p_hi = pp[i + 1];
        pm.wp_lo = 1.0 - y;
        pm.wp_hi = y;
        pm.oob = oob;
        if (!oob && pm.wp_lo != 0.0 && pm.wp_hi != 0.0) fast = 0;  // off-node pressure
      }
      c->pmeta[(size_t)s * nL + l] = pm;
    }
  }
  c->fast = fast;
  lap(0);
  // One bracket serves every species when their nodes, shapes and row pitch coincide.
  int shared = 1;
  for (int s = 1; s < S; ++s) {
    const Species &q0 = c->sp[0], &q = c->sp[s];
    shared = shared && q.n_p == q0.n_p && q.n_T == q0.n_T && q.stride == q0.stride &&
             q.p_nodes == q0.p_nodes && q.T_nodes == q0.T_nodes;
  }
  // batched launches with many blocks in all take the two-wavelength sweep, which reads the
  // step records from global memory (C5, 32 x 100k lambda: -9 % per step, profiles/r04/c5/)
  // (a batched context always has the contracted table without NaN, or fails in build_contracted)
  const int bdepth = sweep_depth(c, 1);
  // (a chemistry batch has no contracted table: the per-species one-lane or tiled sweep)
  const bool lam2_batch = c->n_atm > 1 && !c->chem_on &&
                          lam2_static(c, bdepth, sweep_pf(c, true, 1, bdepth));
  const bool small = c->nblocks <= c->shared_max_blocks && !lam2_batch;
  c->tile = atm_tile_width(c, shared != 0);
  // the LDS-staged step table plus one partial-sum row per wave must leave room for several
  // blocks per CU (deep atmospheres: > ~260 layers read the step table from global memory)
  const size_t ns_l = (size_t)nL - 1;
  const bool lds_fits =
      (size_t)(kBlock / 64) * ns_l * 4 * sizeof(double) + ns_l * sizeof(FastStepS) <= 64 * 1024;
  c->shared = (c->shared_mode == 1 || (c->shared_mode < 0 && small)) && lds_fits ? shared : 0;
  if (c->tile > 1) c->shared = shared;   // the tiled sweep reads the shared-bracket records
  HIP_TRY(hipStreamSynchronize(c->stream));   // queued kernels may still read the metadata
  TRY(c->d_smeta.reserve(S));
  TRY(c->d_pmeta.reserve((size_t)S * nL));
  TRY(c->d_tnodes.reserve(c->tnodes.size()));
  TRY(c->d_tperm.reserve(c->tperm.size()));
  TRY(h2d_wait(c->d_smeta, c->smeta.data(), S, c->stream));
  TRY(h2d_wait(c->d_pmeta, c->pmeta.data(), (size_t)S * nL, c->stream));
  TRY(h2d_wait(c->d_tnodes, c->tnodes.data(), c->tnodes.size(), c->stream));
  TRY(h2d_wait(c->d_tperm, c->tperm.data(), c->tperm.size(), c->stream));
  if (c->mmr.size() != (size_t)S * nL * c->n_atm) return fail("frei_set_mmr must be called");
  TRY(h2d_wait(c->d_mmr, c->mmr.data(), (size_t)S * nL * c->n_atm, c->stream));
  lap(1);
  TRY(build_contracted(c, fast && shared, lap));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->meta_dirty = false;
  c->mmr_dirty = false;
  return 0;
}

AtmStride atm_stride(const frei_ctx* c);

// The steps of sweep_plan, which calls each once.
// Lanes per wavelength of the sweep: the grouped-lane kernel (2 or 4 lanes) when the slice
// leaves about one wave per SIMD or less (contracted table, LDS step table), else 1.
int group_lanes(const frei_ctx* c) {
  if (!(c->fast && c->eff && c->shared)) return 1;
  if (c->group_q > 0) return c->group_q;
  const int64_t blocks = (int64_t)c->nblocks * c->n_atm;   // 256-wavelength blocks
  if (blocks <= c->quad_max_blocks) return 4;
  if (blocks <= c->pair_max_blocks) return 2;
  return 1;
}

// Consumers per block of the producer/consumer sweep (0: not used).  Contracted table and the
// FastStepS records (the LDS-step-table path); the block's LDS must fit the device.
int pipe_consumers(const frei_ctx* c) {
  if (!(c->fast && c->eff && c->shared) || c->pipe_nc == 0) return 0;
  int nc = c->pipe_nc;
  if (nc < 0) {   // by slice size: one 256-wavelength block per CU or fewer
    const int64_t blocks = (int64_t)c->nblocks * c->n_atm;
    const int64_t mx = c->pipe_max_blocks < 0 ? c->n_cu : c->pipe_max_blocks;
    if (blocks <= c->pipe_min_blocks || blocks > mx) return 0;
    nc = 4;
  }
  if (pipe_lds_bytes(nc, c->pipe_m, c->nL - 1) > c->lds_optin) return 0;
  return nc;
}

// Sweeps form their own step records in their prologue (and the update kernels skip writing
// them) when the sweep reads the shared-bracket records from LDS — every form on the contracted
// table with shared brackets — and the mixing ratios are fixed (no T-dependent chemistry).
// NC: pipe_consumers.
bool records_in_sweep(const frei_ctx* c, int NC) {
  if (!(c->rec_sweep && c->fast && c->eff && c->shared && !c->chem_on)) return false;
  // auto: not for batched contexts (every (block, atmosphere) would form the records: C5 -2 %,
  // profiles/r02_ab_rec_sweep.txt), nor for the producer/consumer sweep unless its launches
  // are chained (neutral to slower on their own; a chained sweep must form its records)
  return c->rec_sweep > 0 || (c->n_atm == 1 && (NC == 0 || c->chain == 2));
}

SetupArgs setup_args(const frei_ctx* c) {
  SetupArgs u{};
  u.n_layers = c->nL;
  u.n_species = c->eff ? 1 : c->S;
  u.fast = c->fast;
  u.T = c->d_T;
  u.p = c->d_p;
  u.p_top2 = c->p_top2;
  u.g = c->g;
  u.spec = c->eff ? c->d_smeta_eff : c->d_smeta;
  u.pmeta = c->d_pmeta;
  u.tnodes = c->d_tnodes;
  u.n_tnodes = (int)c->tnodes.size();
  u.tperm = c->d_tperm;
  u.mmr = c->eff ? c->d_ones : c->d_mmr;
  u.steps = c->d_steps;
  u.terms = c->d_terms;
  u.fsteps = c->d_fsteps;
  u.ssteps = c->d_ssteps;
  u.shared = c->shared;
  u.bs = atm_stride(c);
  u.kvalid = c->lazy_on ? c->d_kvalid : nullptr;
  u.kpitch = c->sp.empty() ? 0 : c->sp[0].stride;
  if (c->chem_on) {
    u.chem.tab = c->d_chem_tab;
    u.chem.T = c->d_chem_T;
    u.chem.pj = c->d_chem_pj;
    u.chem.pz = c->d_chem_pz;
    u.chem.n_T = c->chem_nT;
    u.chem.n_p = c->chem_np;
    const int64_t per = (int64_t)c->S * c->chem_nT * c->chem_np;
    if (c->n_atm > 1 && !c->chem_atm.empty()) {   // atm_view picks each atmosphere's table
      u.chem.atm_tab = c->d_chem_atm;
      u.chem.tab_stride = per;
    } else if (!c->chem_atm.empty()) {            // a batched context of one atmosphere
      u.chem.tab += c->chem_atm[0] * per;
    }
  }
  return u;
}

hipEvent_t next_event_in(std::vector<Event>& pool, size_t& used) {
  if (used == pool.size()) {
    Event e;
    if (e.create()) return nullptr;
    pool.push_back(std::move(e));
  }
  return pool[used++];
}
hipEvent_t next_event(frei_ctx* c) { return next_event_in(c->ev_pool, c->ev_used); }

struct SweepOpts {
  int dir = kEmit;
  int next_dir = -1;   // setup for the next sweep inside update
  int force = 0;       // ignore the convergence flag
  int track = 0;       // T-P history / convergence bookkeeping
  int stop_on_conv = 0;
  int n_zero_crossings = 2;
  double convergence_dT = 3.0;
  double alpha = 1.0;
  double* dtaus = nullptr;    // device
  double* dT_out = nullptr;   // device
  double* bol_out = nullptr;  // device
  int live_only = 0;          // T-P loop: skip stores no later sweep reads
};

// Temperature buffers: d_T is the current one; an update writes a buffer that is neither d_T
// (its input) nor `busy` (the input of an update still running in the same launch), which
// then becomes d_T.
void rotate_T(frei_ctx* c, double* out) {
  double* b[3] = {c->d_T, c->d_T_alt, c->d_T3};
  double* rest[2];
  int n = 0;
  for (double* x : b)
    if (x != out && n < 2) rest[n++] = x;
  c->d_T = out;
  c->d_T_alt = rest[0];
  c->d_T3 = rest[1];
}
double* free_T(frei_ctx* c, const double* busy) { return c->d_T_alt != busy ? c->d_T_alt : c->d_T3; }

// Drop a deferred update that will never run (an error part-way through a run).  The sweep that
// deferred it already made its output buffer the current temperatures, filled with kPoisonT
// ("not published"), so the current temperatures go back to that update's input: a later sweep
// or read that skips frei_state_init sees the last published temperatures, not poison.
void drop_pending(frei_ctx* c) {
  if (!c->has_pend) return;
  c->has_pend = false;
  rotate_T(c, c->pend.su.T);
}

// reduce + update fused into one launch: one atmosphere, exchange local or P2P (RCCL and the
// host hook need the rank's sums in memory between the two kernels)
bool fused_ok(const frei_ctx* c) {
  return c->fused_update && c->n_atm == 1 && !c->comm && !(c->nranks > 1 && c->host_ag) &&
         (2 * (size_t)c->nL + c->tnodes.size()) * sizeof(double) <= 32 * 1024;
}

// Sweep and update share launches (chained launches, the trailing update) only as stream
// launches (no graph capture) and not while per-sweep HIP events are on (frei_timing): events
// around such a launch would also cover the update it runs, including its wait for the peers'
// sums, so a timed run launches sweep and update separately and the events time the sweep
// alone.  Nor when ranks share this device (frei_comm_shared_device): the launch's sweep or
// update blocks spin on workgroups that wait for every rank's sums, and could hold the CUs
// another rank's kernels need.
bool shared_launch_ok(const frei_ctx* c) {
  return c->fast && c->eff && c->shared && !c->use_graph && !c->keys && !c->timing &&
         !c->shared_device;
}

// This context's sweeps run chained: a grouped-lane or one-lane (two or more steps in flight)
// sweep of the contracted table forming its own step records (p.rec_on), fused update (p.fused).
bool chain_ready(const frei_ctx* c, const SweepPlan& p) {
  if (!(c->chain && shared_launch_ok(c) && p.rec_on && p.fused)) return false;
  // producer/consumer, four consumers per block; the chained kernel adds the update body's
  // static LDS (4.3 KiB) to the sweep's, which must still fit the CU (deep atmospheres do not)
  // — only on request (FREI_CHAIN=2): chained, its 1024-thread update blocks take 6 µs where
  // the separate update kernel takes 3 (profiles/r03/chain/ab_pipe.txt)
  if (p.NC > 0)
    return c->chain == 2 && p.NC == 4 &&
           pipe_lds_bytes(4, c->pipe_m, c->nL - 1) + 6 * 1024 <= c->lds_optin;
  if (p.Q > 1) return true;      // grouped-lane
  // one-lane (two or more steps in flight): measured neutral to slower at 125k-500k
  // (profiles/r03/chain/ab_onelane.txt), so only on request (FREI_CHAIN=2)
  return c->chain == 2 && c->prefetch_depth != 1;
}

// Update workgroups of a trailing-update launch (0: not used): the producer/consumer sweep with
// four consumers and the update's records (not p.rec_on), the fused update, one atmosphere, fixed
// mixing ratios, and — so that they are resident beside the sweep, never waiting behind it — at
// least two CUs left free by the sweep's one block per CU (eight update blocks at most).
int tail_blocks(const frei_ctx* c, const SweepPlan& p) {
  if (!(c->tail && shared_launch_ok(c) && c->n_atm == 1 && !c->chem_on && p.fused)) return 0;
  if (p.NC != 4 || p.rec_on) return 0;
  if (pipe_tail_lds_bytes(c->nL - 1, (int)c->tnodes.size()) + 6 * 1024 > c->lds_optin) return 0;
  const int free_cu = c->n_cu - p.nb_run;
  return free_cu >= 2 ? std::min(free_cu, 8) : 0;
}

// The plan of one sweep.  pending: an update deferred by the sweep before waits for a launch;
// defer: this sweep may defer its own (both only matter when chained launches apply).
SweepPlan sweep_plan(const frei_ctx* c, bool pending, bool defer) {
  SweepPlan p{};
  const int ns = c->nL - 1;
  p.S_run = c->eff ? 1 : c->S;
  p.lds_steps = c->shared;
  p.pipe_pf = c->pipe_pf;
  // per-row partials while the one-lane sweep's LDS stays within 48 KiB (3+ blocks per CU)
  p.red_rows = c->red_rows &&
               (size_t)16 * ns * 4 * sizeof(double) + (size_t)ns * sizeof(FastStepS) <= 48 * 1024;
  p.depth = sweep_depth(c, p.S_run);
  p.pf = sweep_pf(c, c->eff != 0, p.S_run, p.depth);
  bool any_nan = false;
  for (int q = 0; q < c->S; ++q) any_nan = any_nan || c->sp[q].has_nan;
  p.nan_check = any_nan && !c->eff;
  p.Q = group_lanes(c);
  // staged partial sums (mode 2): the one-lane sweep with two steps in flight, and the
  // grouped-lane sweep (two groups in flight)
  if ((p.Q > 1 || p.depth == 2 || (p.depth == 1 && p.pf == 2)) && c->red_stage &&
      staged_sums_fit(ns))
    p.red_rows = 2;
  p.NW = c->group_waves;
  p.NC = pipe_consumers(c);
  p.rec_on = records_in_sweep(c, p.NC);
  p.fused = fused_ok(c);
  // (a dry pass only hashes the launches a graph capture would issue: never chained)
  p.chain = !c->dry && chain_ready(c, p);
  p.merge = p.chain && pending;
  p.defer_own = p.chain && defer;
  p.nb_run = c->nblocks;
  if (!c->fast) {
    p.form = kGeneric;
  } else if (p.NC > 0) {
    p.form = kPipe;
    p.nb_run = (int)((c->nlam + 64 * p.NC - 1) / (64 * p.NC));
    if (!p.merge) p.tail_nT = tail_blocks(c, p);
  } else if (p.Q > 1) {
    p.form = kGrouped;
    p.nb_run = (int)((c->nlam + 64 * p.NW / p.Q - 1) / (64 * p.NW / p.Q));
  } else if (p.merge) {   // the one-lane contracted sweep, records formed in the block
    p.form = kOneLane;
  } else if (c->eff && p.S_run == 1 && !c->shared && !any_nan && p.red_rows == 2 &&
             lam2_static(c, p.depth, p.pf)) {
    // two wavelengths per lane: the one-lane contracted sweep on slices that need more than
    // about one round of one-lane blocks (1280 resident at five waves per SIMD on 256 CUs)
    p.form = kLam2;
    p.nb_run = (int)((c->nlam + 2 * kBlock - 1) / (2 * kBlock));
  } else if (c->tile > 1 && !c->eff && c->chem_on && c->shared && p.red_rows == 2) {
    p.form = kTiled;   // a chemistry batch, c->tile atmospheres per block
    p.tile = c->tile;
  } else {
    p.form = kOneLane;
  }
  // lazy K3: only the two-wavelength sweep with the fused update (which marks the rows it
  // used) contracts on the way; any other form gets the whole table first
  p.whole_table = c->fast && !(p.form == kLam2 && p.fused);
  return p;
}

// Launch a deferred update on its own (the next sweep cannot take it, or the caller needs its
// results now).  Its output buffer holds kPoisonT until the update writes it.
int flush_update(frei_ctx* c) {
  if (!c->has_pend) return 0;
  c->has_pend = false;
  launch_update_fused(c->pend, c->stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

// FNV-1a over an argument block (zero-initialised structs: padding bytes are zero)
template <typename T>
uint64_t arg_hash(uint64_t h, const T& x) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(&x);
  for (size_t i = 0; i < sizeof(T); ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

// Lazy K3: contract every row not contracted yet (any sweep form other than the two-wavelength
// one, which contracts its masked rows itself, or an update that does not mark them).
int complete_contraction(frei_ctx* c) {
  if (c->eff_complete) return 0;
  const Species& q0 = c->sp[0];
  const double* tabs[kMaxFastS];
  for (int s = 0; s < c->S; ++s) tabs[s] = c->sp[s].d_tab;
  std::vector<int32_t> prow(c->nL);
  for (int l = 0; l < c->nL; ++l) {
    const PMeta& pm = c->pmeta[l];
    prow[l] = (pm.wp_lo != 0.0) ? pm.p_lo : pm.p_hi;
  }
  launch_contract(tabs, c->S, c->d_mmr, c->d_prow, c->nL, q0.n_T, q0.stride, c->d_eff, c->stream);
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> ones((size_t)q0.n_p * q0.n_T, 0);
  for (int l = 0; l < c->nL; ++l)
    for (int t = 0; t < q0.n_T; ++t) ones[(size_t)prow[l] * q0.n_T + t] = 1;
  TRY(h2d_wait(c->d_kvalid, ones.data(), ones.size(), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // (the host vector)
  c->eff_complete = true;
  return 0;
}

// p2p_timeout_s in wall_clock64 ticks (100 MHz): the bound of every device-side wait
long long timeout_ticks(const frei_ctx* c) { return (long long)(c->p2p_timeout_s * 1e8); }

SweepArgs generic_args(const frei_ctx* c, const SweepOpts& o) {
  SweepArgs a{};
  a.n_lam = c->nlam;
  a.n_steps = c->nL - 1;
  a.n_species = c->S;
  a.force = o.force;
  a.live_only = o.live_only;
  a.c1 = c->d_c1;
  a.hcl = c->d_hcl;
  a.sig = c->d_sig;
  a.wtr = c->d_wtr;
  a.ftoa = c->d_ftoa;
  a.steps = c->d_steps;
  a.terms = c->d_terms;
  a.F_up = c->d_Fu;
  a.F_down = c->d_Fd;
  a.dtaus = o.dtaus;
  a.part = c->d_part;
  a.conv = c->d_conv;
  return a;
}

// Arguments of every sweep form on the contracted / per-species tables (c->fast).  T_next: the
// buffer this sweep's update writes (a deferred update's output starts as kPoisonT).
FastArgs fast_args(const frei_ctx* c, const SweepOpts& o, const SweepPlan& p, double* T_next) {
  FastArgs f{};
  f.n_lam = c->nlam;
  f.pitch = c->sp[0].stride;
  f.n_steps = c->nL - 1;
  f.force = o.force;
  f.live_only = o.live_only;
  f.c1 = c->d_c1;
  f.hcl = c->d_hcl;
  f.sig = c->d_sig;
  f.wtr = c->d_wtr;
  f.ftoa = c->d_ftoa;
  for (int q = 0; q < kMaxFastS; ++q) f.tab[q] = q < c->S ? c->sp[q].d_tab : nullptr;
  if (c->eff) f.tab[0] = c->d_eff;
  if (c->lazy_on && !c->eff_complete) {   // the two-wavelength sweep contracts masked rows
    for (int q = 0; q < kMaxFastS; ++q) f.ktab[q] = q < c->S ? c->sp[q].d_tab : nullptr;
    f.kmmr = c->d_mmr;
    f.kS = c->S;
    f.kNL = c->nL;
  }
  f.steps = c->d_fsteps;
  f.ssteps = c->d_ssteps;
  f.F_up = c->d_Fu;
  f.F_down = c->d_Fd;
  f.dtaus = o.dtaus;
  f.part = c->d_part;
  f.conv = c->d_conv;
  f.bs = atm_stride(c);
  f.n_atm = c->n_atm;
  f.unit_mmr = c->eff ? 1 : 0;
  f.rec_on = p.rec_on;
  f.min_lds = c->sweep_lds_kb * 1024;
  if (p.merge) {   // this launch's leading workgroups run the deferred update
    f.ch_epoch = c->d_epoch;
    f.ch_val = c->chain_seq;
    f.ch_can_conv = c->pend.track && c->pend.dir == kAbsorb && c->pend.stop_on_conv;
    f.ch_timeout = timeout_ticks(c);
    f.ch_err = c->d_chain_err;
  }
  if (p.defer_own) f.poison = T_next;
  if (f.rec_on) f.rec = setup_args(c);   // T of this sweep: c->d_T now
  f.red_rows = p.red_rows;
  return f;
}

// The one place a sweep is launched: by the plan's form and modifiers.  A merged launch takes
// the pending update with it; a trailing-update launch waits for its update (launch_tail).
void launch_planned(frei_ctx* c, int dir, const SweepPlan& p, const SweepArgs& a,
                    const FastArgs& f) {
  UpdateArgs pend{};
  if (p.merge) {
    pend = c->pend;
    pend.epoch = c->d_epoch;
    pend.epoch_val = c->chain_seq;
    c->has_pend = false;
    ++c->n_chained;
  }
  switch (p.form) {
    case kGeneric:
      launch_sweep(dir, a, p.nb_run, c->stream);
      break;
    case kPipe:
      if (p.merge) launch_sweep_pipe_chain(dir, p.pipe_pf, f, pend, p.nb_run, c->stream);
      else if (p.tail_nT == 0) launch_sweep_pipe(dir, p.NC, p.pipe_pf, f, p.nb_run, c->stream);
      break;
    case kGrouped:
      if (p.merge) launch_sweep_chain(dir, p.Q, p.NW, f, pend, p.nb_run, c->stream);
      else launch_sweep_group(dir, p.Q, p.NW, f, p.nb_run, c->stream);
      break;
    case kOneLane:
      if (p.merge) launch_sweep_fast_chain(dir, p.depth, p.pf, f, pend, p.nb_run, c->stream);
      else launch_sweep_fast(dir, p.S_run, p.depth, p.pf, p.nan_check != 0, p.lds_steps != 0, f,
                             p.nb_run, c->stream);
      break;
    case kLam2:
      launch_sweep_pair(dir, f, p.nb_run, c->stream);
      break;
    case kTiled:
      launch_sweep_tile(dir, p.S_run, p.tile, f, p.nb_run, c->stream);
      break;
  }
}

// P2P: each rank's sums are pushed and waited for on the device
void p2p_args(frei_ctx* c, P2PPush& push, P2PWait& wait) {
  const uint64_t seq = ++c->p2p_seq;
  push.peers = c->d_peers;
  push.nranks = c->nranks;
  push.rank = c->rank;
  push.n = (int64_t)(c->nL - 1) * 4;
  push.seq = seq;
  wait.mbox = c->d_mbox;
  wait.nranks = c->nranks;
  wait.n = push.n;
  wait.seq = seq;
  wait.timeout_ticks = timeout_ticks(c);
  wait.err = c->d_comm_err;
  wait.wait_ticks = c->timing ? c->d_wait_ticks : nullptr;
}

// The rank exchange of the reduced sums through the host hook or RCCL (P2P runs inside the
// kernels), between HIP events when timing is on.  *Fb: where the update reads the sums.
int exchange(frei_ctx* c, const double** Fb) {
  const size_t n = (size_t)(c->nL - 1) * 4;
  const bool host = c->nranks > 1 && c->host_ag;
  *Fb = c->d_Fb;
  if (!host && !c->comm) return 0;
  hipEvent_t x1 = nullptr;
  if (c->timing) {
    hipEvent_t x0 = next_event_in(c->xev_pool, c->xev_used);
    x1 = next_event_in(c->xev_pool, c->xev_used);
    if (!x0 || !x1) return fail("hipEventCreate failed");
    HIP_TRY(hipEventRecord(x0, c->stream));
  }
  if (host) {
    HIP_TRY(hipMemcpyAsync(c->h_ag, c->d_Fb, n * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->host_ag(c->h_ag, c->h_ag + n, (int64_t)n, c->host_ag_user) != 0)
      return fail("host all-gather callback failed");
    HIP_TRY(hipMemcpyAsync(c->d_Fb_all, c->h_ag + n, c->nranks * n * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
  } else {  // RCCL (also a forced 1-rank communicator, FREI_FORCE_RCCL=1)
    Rccl* r = rccl();
    if (!r) return fail("RCCL communicator not initialised");
    int rc = r->allGather(c->d_Fb, c->d_Fb_all, n, kNcclFloat64, c->comm, c->stream);
    if (rc != 0)
      return fail(std::string("ncclAllGather: ") + (r->errStr ? r->errStr(rc) : "error"));
  }
  *Fb = c->d_Fb_all;
  if (x1) HIP_TRY(hipEventRecord(x1, c->stream));
  return 0;
}

// The update of this sweep (K4/K5, or the fused reduce + update writing T_next).  With the
// records formed in the sweeps the update writes none for the next one (c->rec_skipped).
UpdateArgs update_args(frei_ctx* c, const SweepOpts& o, const SweepPlan& p, const P2PPush& push,
                       const P2PWait& wait, const double* Fb, double* T_next) {
  UpdateArgs u{};
  u.su = setup_args(c);
  u.p2p = wait;
  u.dir = o.dir;
  u.next_dir = o.next_dir;
  if (p.rec_on && o.next_dir >= 0) {   // the next sweep forms its own
    u.next_dir = -1;
    c->rec_skipped = true;
  }
  u.nranks = c->nranks;
  u.force = o.force;
  u.track = o.track;
  u.stop_on_conv = o.stop_on_conv;
  u.n_zero_crossings = o.n_zero_crossings;
  u.hist_cap = c->hist_cap;
  u.m_bar = c->m_bar;
  u.alpha = o.alpha;
  u.convergence_dT = o.convergence_dT;
  u.Fb = Fb;
  u.lnp = c->d_lnp;
  u.dT_out = o.dT_out;
  u.bol_out = o.bol_out;
  u.Tb = c->d_Tb;
  u.Ta = c->d_Ta;
  u.hist = c->d_hist;
  u.flips = c->d_flips;
  u.prev_sign = c->d_prev;
  u.ndiff = c->d_ndiff;
  u.iter = c->d_iter;
  u.conv = c->d_conv;
  // metadata in LDS when the update's whole allocation (the launch's own formula) fits the
  // 64 KiB a workgroup may request
  u.meta_in_lds = update_lds_bytes(c->nL, (int)c->tnodes.size(), p.S_run, true) <=
                  std::min<size_t>(c->lds_per_block, 64 * 1024);
  if (p.fused) {
    u.part = c->d_part;
    u.nblocks = p.nb_run;
    u.push = push;
    u.T_out = T_next;
    u.done = c->d_done;
  }
  return u;
}

// The trailing-update launch: the producer/consumer sweep f and its update u in one launch.
// The sweep publishes into one of two partial-sum buffers, which the update polls; the update
// workgroups put the other (the launch before) back to kPoisonT.
int launch_tail(frei_ctx* c, int dir, const SweepPlan& p, FastArgs f, UpdateArgs u) {
  const int64_t need = (int64_t)p.nb_run * (c->nL - 1) * 4;
  if (c->tpart_n < need) {
    c->tpart_n = 0;
    TRY(c->d_tpart.reserve(2 * (size_t)need));
    c->tpart_n = need;
    c->tpart_fill = true;
  }
  if (c->tpart_fill) {
    launch_poison(c->d_tpart, 2 * c->tpart_n, c->stream);
    c->tpart_fill = false;
    c->tpart_parity = 0;
  }
  double* cur = c->d_tpart + c->tpart_parity * c->tpart_n;
  double* other = c->d_tpart + (1 - c->tpart_parity) * c->tpart_n;
  c->tpart_parity ^= 1;
  f.tail_part = cur;
  u.part = cur;
  u.poll = 1;
  u.poll_timeout = timeout_ticks(c);
  u.poll_err = c->d_chain_err;
  launch_sweep_pipe_tail(dir, p.pipe_pf, f, u, p.nb_run, p.tail_nT, other, c->stream);
  ++c->n_tail;
  return 0;
}

// One sweep: K1 -> fused reduce + update (+ next setup; P2P exchange inside), or K1 ->
// reduce -> [RCCL / host all-gather] -> K4/K5 (batched contexts, RCCL, host hook,
// fused_update 0).  Asynchronous.
//   plan -> setup / contraction the plan asks for -> sweep launch -> exchange ->
//   update launched, deferred (chained) or trailing the sweep -> rotate_T
// With c->dry it only appends the hash of every launch's arguments to c->keys and applies
// the host-side state changes (temperature buffer swap), launching nothing.
int run_sweep(frei_ctx* c, const SweepOpts& o, bool defer = false) {
  const SweepPlan p = sweep_plan(c, c->has_pend, defer);
  if (c->has_pend && !p.merge) TRY(flush_update(c));   // (not chained: the next cannot take it)
  // the output buffer of this sweep's update: not d_T, and not the merged update's input
  double* T_next = p.chain ? free_T(c, p.merge ? c->pend.su.T : nullptr) : c->d_T_alt;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c->timing) {
    e0 = next_event(c);
    e1 = next_event(c);
    if (!e0 || !e1) return fail("hipEventCreate failed");
    HIP_TRY(hipEventRecord(e0, c->stream));
  }
  // a sweep that reads the update's records after one whose update skipped them (an option or
  // the tables changed mid-run): write this sweep's records first
  if (!p.rec_on && c->rec_skipped && !c->dry) {
    launch_setup(setup_args(c), o.dir, c->stream, c->n_atm);
    HIP_TRY(hipGetLastError());
  }
  c->rec_skipped = false;
  if (p.whole_table && c->lazy_on && !c->eff_complete && !c->dry) TRY(complete_contraction(c));
  if (p.merge) ++c->chain_seq;
  const SweepArgs a = generic_args(c, o);
  const FastArgs f = c->fast ? fast_args(c, o, p, T_next) : FastArgs{};
  if (c->keys) {   // any change of the plan or of the arguments re-captures
    const uint64_t seed = 1469598103934665603ull;
    const uint64_t h = c->fast ? arg_hash(seed, f) : arg_hash(seed, a);
    c->keys->push_back(arg_hash(arg_hash(h, p), o.dir));
  }
  if (!c->dry) launch_planned(c, o.dir, p, a, f);
  HIP_TRY(hipGetLastError());
  if (c->timing) HIP_TRY(hipEventRecord(e1, c->stream));
  P2PPush push{};
  P2PWait wait{};
  if (c->d_mbox && !c->dry) p2p_args(c, push, wait);
  if (!p.fused && c->dry) {   // not graph-replayable (the check in iterate() sees the marker)
    if (c->keys) c->keys->push_back(0);
    return 0;
  }
  if (!p.fused) {
    const AtmStride bs = atm_stride(c);
    launch_reduce(c->d_part, p.nb_run, c->d_Fb, (c->nL - 1) * 4, c->d_conv, o.force, c->stream,
                  c->n_atm, bs.part, bs.fb, c->d_mbox ? &push : nullptr);
  }
  HIP_TRY(hipGetLastError());
  const double* Fb = nullptr;
  TRY(exchange(c, &Fb));
  const UpdateArgs u = update_args(c, o, p, push, wait, Fb, T_next);
  if (!p.fused) {
    launch_update(u, c->stream, c->n_atm);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  if (c->keys) c->keys->push_back(arg_hash(1469598103934665603ull, u));
  if (p.defer_own) {   // runs at the head of the next sweep's launch, or flush_update
    c->pend = u;
    c->has_pend = true;
  } else if (p.tail_nT > 0) {
    TRY(launch_tail(c, o.dir, p, f, u));
  } else if (!c->dry) {
    launch_update_fused(u, c->stream);
  }
  HIP_TRY(hipGetLastError());
  rotate_T(c, T_next);
  return 0;
}

// A host upload overwrites the current temperatures, so the fused update's ping-pong can
// restart from the same buffer (every run then issues identical launch arguments).
void home_temperatures(frei_ctx* c) {
  if (c->d_T != c->d_T_home) rotate_T(c, c->d_T_home);
}

int reset_loop_state(frei_ctx* c) {
  const size_t A = c->n_atm;
  HIP_TRY(hipMemsetAsync(c->d_conv, 0, sizeof(int) * A, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_iter, 0, sizeof(int) * A, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_flips, 0, sizeof(int32_t) * c->nL * A, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_prev, 0, sizeof(int32_t) * c->nL * A, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_ndiff, 0, sizeof(int32_t) * c->nL * A, c->stream));
  return 0;
}

int ensure_hist(frei_ctx* c, int cap) {
  if (cap <= c->hist_cap) return 0;
  HIP_TRY(hipStreamSynchronize(c->stream));   // queued update kernels may still write it
  c->hist_cap = 0;
  TRY(c->d_hist.reserve((size_t)cap * 2 * c->nL * c->n_atm));
  c->hist_cap = cap;
  return 0;
}

// Per-atmosphere strides of a batched context (all zero for one atmosphere).
AtmStride atm_stride(const frei_ctx* c) {
  AtmStride b{};
  if (c->n_atm <= 1) return b;
  const int64_t nL = c->nL, ns = nL - 1;
  b.layers = nL;
  b.steps = ns;
  b.fb = ns * 4;
  b.hist = (int64_t)c->hist_cap * 2 * nL;
  b.flux = nL * c->nlam;
  b.tab = c->eff ? (int64_t)c->eff_stride : 0;   // (a chemistry batch: the shared tables)
  b.part = ns * 4 * (int64_t)(4 * c->nblocks);
  b.ftoa = c->ftoa_per_atm ? c->nlam : 0;
  b.g = c->d_g;
  return b;
}

int ensure_dtaus(frei_ctx* c) {
  if (!c->d_dtaus) TRY(c->d_dtaus.alloc((size_t)c->nL * c->nlam));
  launch_fill(c->d_dtaus, c->nlam, 1.0, c->stream);  // row 0 placeholder (Q12)
  HIP_TRY(hipGetLastError());
  return 0;
}

// Every atmosphere's dtaus [n_atm][nL][nlam] of a batched context, allocated on the first
// request only (n_atm = 1: ensure_dtaus' buffer); row 0 of every atmosphere is the ones
// placeholder (Q12).  A failed allocation names its size and leaves the context as it was.
int ensure_dtaus_batch(frei_ctx* c) {
  if (c->n_atm == 1) return ensure_dtaus(c);
  const size_t per = (size_t)c->nL * c->nlam, n = per * c->n_atm;
  if (!c->d_dtaus && c->d_dtaus.alloc(n))   // (no sticky error: alloc cleared it)
    return fail("cannot allocate " + std::to_string(n * sizeof(double)) + " bytes for " +
                std::to_string(c->n_atm) + " atmospheres' dtaus (keep_dtaus)");
  launch_fill_rows(c->d_dtaus, c->nlam, (int64_t)per, c->n_atm, 1.0, c->stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

bool ready(frei_ctx* c) { return c && c->grid_set; }

// Tuning knobs (frei_set_option and FREI_<NAME> environment variables); each takes effect at
// the next metadata build (the tables' sweep path is re-derived).
const char* const kOptionNames[] = {"prefetch_depth", "shared", "shared_max_blocks",
                                    "precontract", "depth4_max_blocks", "pair_max_blocks",
                                    "quad_max_blocks", "red_rows", "red_stage", "group_q",
                                    "fused_update", "graph", "pipe", "pipe_pf", "pipe_min_blocks", "rec_sweep",
                                    "pipe_max_blocks", "prefetch_steps", "k7_mfma", "sweep_lds_kb", "group_waves", "chain",
                                    "lam2", "tail", "lazy_k3", "atm_tile", nullptr};
int set_option(frei_ctx* c, const std::string& k, int v) {
  if (k == "prefetch_depth") c->prefetch_depth = v;
  else if (k == "shared") c->shared_mode = v < 0 ? -1 : (v ? 1 : 0);
  else if (k == "shared_max_blocks") c->shared_max_blocks = v;
  else if (k == "precontract") c->eff_mode = v < 0 ? -1 : (v ? 1 : 0);
  else if (k == "depth4_max_blocks") c->depth4_max_blocks = v;
  else if (k == "pair_max_blocks") c->pair_max_blocks = v;
  else if (k == "quad_max_blocks") c->quad_max_blocks = v;
  else if (k == "red_rows") c->red_rows = v != 0;
  else if (k == "red_stage") c->red_stage = v != 0;
  else if (k == "group_q") c->group_q = (v == 1 || v == 2 || v == 4) ? v : 0;
  else if (k == "fused_update") c->fused_update = v != 0;
  else if (k == "graph") c->use_graph = v != 0;
  else if (k == "pipe") c->pipe_nc = (v == 1 || v == 2 || v == 4 || v == -1) ? v : 0;
  else if (k == "pipe_min_blocks") c->pipe_min_blocks = v;
  else if (k == "rec_sweep") c->rec_sweep = v < 0 ? -1 : (v ? 1 : 0);
  else if (k == "pipe_max_blocks") c->pipe_max_blocks = v;
  else if (k == "pipe_pf") c->pipe_pf = v == 1 ? 1 : 2;
  else if (k == "k7_mfma") c->k7_mfma = v != 0;
  else if (k == "group_waves") c->group_waves = v == 8 ? 8 : 4;
  else if (k == "chain") c->chain = v < 0 ? 0 : (v > 2 ? 2 : v);
  else if (k == "lam2") c->lam2 = v < 0 ? -1 : (v ? 1 : 0);
  else if (k == "tail") c->tail = v != 0;
  else if (k == "lazy_k3") c->lazy_k3 = v != 0;
  else if (k == "atm_tile") c->atm_tile = (v == 1 || v == 2 || v == 4) ? v : -1;
  else if (k == "sweep_lds_kb") c->sweep_lds_kb = v < 0 ? 0 : (v > 160 ? 160 : v);
  else if (k == "prefetch_steps") c->prefetch_steps = v >= 16 ? 16 : v >= 8 ? 8 : v == 2 ? 2 : 0;
  else return fail("unknown option '" + k + "'");
  c->meta_dirty = true;
  return 0;
}

// After a stream synchronize: did a chained sweep's poll or a P2P wait time out (a rank never
// published its sums)?  The flags are read only when they can have been set — a chained launch
// since the last check, a P2P communicator — and into pinned memory on the context's stream: a
// pageable hipMemcpy here cost ~20 ms the first time (its staging buffer), which left the GPU
// idle right before a timed loop (bench.py's warm-up synchronize) and changed how the power
// management clocked the loop that followed (profiles/r04/bisect/README.md).
int check_comm(frei_ctx* c) {
  const bool chain = c->d_chain_err && c->n_chained + c->n_tail != c->chain_checked;
  const bool comm = c->d_comm_err != nullptr;
  if (!chain && !comm) return 0;
  if (chain)
    HIP_TRY(hipMemcpyAsync(&c->h_err[0], c->d_chain_err, sizeof(int), hipMemcpyDeviceToHost,
                           c->stream));
  if (comm)
    HIP_TRY(hipMemcpyAsync(&c->h_err[1], c->d_comm_err, sizeof(int), hipMemcpyDeviceToHost,
                           c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->chain_checked = c->n_chained + c->n_tail;
  if (chain && c->h_err[0]) {   // reported once: rearm it so later runs are not failed by it
    drop_pending(c);
    c->tpart_fill = true;       // a trailing update gave up: its buffers are in no known state
    const int code = c->h_err[0];
    c->h_err[0] = 0;
    HIP_TRY(hipMemsetAsync(c->d_chain_err, 0, sizeof(int), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // (the first wait to give up: 1 a chained sweep block's temperatures, 3 a trailing update
    // slot's partial sums)
    return fail("chained sweep / trailing update: a wait for values another workgroup "
                "publishes gave up (FREI_P2P_TIMEOUT_S; wait " + std::to_string(code) + ")");
  }
  if (comm && c->h_err[1])
    return fail("P2P exchange timed out: a peer rank did not publish its partial sums "
                "(FREI_P2P_TIMEOUT_S)");
  return 0;
}

// The dtaus a post-processing call reads when the caller passes none: the last run's, kept on
// the device (a batched run's with keep_dtaus).
int need_device_dtaus(frei_ctx* c, bool batch) {
  if (c->d_dtaus && (batch ? c->dtaus_batch_valid : c->dtaus_valid)) return 0;
  return fail(batch ? "no device dtaus: run frei_run_batch_ex with keep_dtaus first, or pass dtaus"
                    : "no device dtaus: run frei_run first or pass dtaus");
}

}  // namespace

namespace frei {
int ctx_emergent_rows(frei_ctx* c, CtxRows* out) {
  if (!ready(c) || !c->d_Fu) return fail("context not ready");
  out->rows = c->d_Fu + (size_t)(c->nL - 1) * c->nlam;
  out->stride = (int64_t)c->nL * c->nlam;
  out->n_atm = c->n_atm;
  out->n_lam = c->nlam;
  out->device = c->device;
  out->stream = c->stream;
  return 0;
}
int ctx_columns(frei_ctx* c, bool need_dtaus, CtxColumns* out) {
  if (!ready(c)) return fail("context not ready");
  if (need_dtaus) TRY(need_device_dtaus(c, c->batch_api));
  out->dtaus = need_dtaus ? c->d_dtaus : nullptr;
  out->c1 = c->d_c1;
  out->hcl = c->d_hcl;
  out->n_lam = c->nlam;
  out->nL = c->nL;
  out->n_atm = c->n_atm;
  out->device = c->device;
  out->stream = c->stream;
  return 0;
}
}  // namespace frei

frei_ctx::~frei_ctx() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  if (comm) {
    Rccl* r = rccl();
    if (r && r->commDestroy) r->commDestroy(comm);
  }
  if (g_exec) (void)hipGraphExecDestroy(g_exec);
  for (void* p : peer_mapped) (void)hipIpcCloseMemHandle(p);
}

// One row of ctx_create's allocation table: a buffer of either kind and its element count
// (kNone: not for this context).
constexpr size_t kNone = ~size_t(0);
struct Want {
  int (*alloc)(void*, size_t);
  void* buf;
  size_t n;
};
template <typename T, typename Mem>
Want want(Buf<T, Mem>& b, size_t n) {
  return {[](void* p, size_t k) { return static_cast<Buf<T, Mem>*>(p)->alloc(k); }, &b, n};
}

// ==================================================================== C ABI
extern "C" {

int frei_version(void) { return 20000; }

const char* frei_last_error(void) { return g_err.c_str(); }

int frei_device_count(int* n) {
  if (!n) return fail("null argument");
  HIP_TRY(hipGetDeviceCount(n));
  return 0;
}

int frei_live_resources(int64_t* device_buffers, int64_t* pinned_buffers, int64_t* streams,
                        int64_t* events) {
  int64_t* const out[4] = {device_buffers, pinned_buffers, streams, events};
  for (int k = 0; k < 4; ++k)
    if (out[k]) *out[k] = g_live[k].load();
  return 0;
}

static int ctx_create(frei_ctx** out, int device, int n_layers, int64_t n_lam, int n_species,
                      int n_atm) {
  if (!out) return fail("null argument");
  *out = nullptr;
  if (n_atm < 1 || n_atm > 65535) return fail("n_atm must be in [1, 65535]");
  if (n_layers < 4 || n_layers > kMaxLayers)
    return fail("n_layers must be in [4, 1024] (the emit top layer uses p[-3])");
  if (n_lam < 2) return fail("n_lam must be >= 2");
  if (n_species < 1 || n_species > 64) return fail("n_species must be in [1, 64]");
  frei_ctx* c = new frei_ctx();
  c->device = device;
  c->nL = n_layers;
  c->nlam = n_lam;
  c->S = n_species;
  c->n_atm = n_atm;
  c->sp.resize(n_species);
  c->nblocks = (int)((n_lam + kBlock - 1) / kBlock);
  // tuning knobs: FREI_<NAME> in the environment, or frei_set_option(ctx, "<name>", v)
  for (const char* const* k = kOptionNames; *k; ++k) {
    std::string env = "FREI_";
    for (const char* q = *k; *q; ++q) env += (char)std::toupper((unsigned char)*q);
    if (const char* e = getenv(env.c_str())) (void)set_option(c, *k, atoi(e));
  }
  auto bail = [&](int rc) {
    delete c;
    return rc;
  };
  int rc;
  if ((rc = set_device(c))) return bail(rc);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.sharedMemPerBlock > 0) {
      c->lds_per_block = prop.sharedMemPerBlock;
      c->lds_optin = std::max(c->lds_per_block, (size_t)prop.sharedMemPerBlockOptin);
      if (prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    }
  }
  if (c->stream.create()) return bail(fail("hipStreamCreate failed"));
  const size_t NL = n_layers, NS = n_species, ns = n_layers - 1, A = n_atm;
  const size_t F = NL * (size_t)n_lam * A;   // per-atmosphere buffers are n_atm blocks
  // every buffer a context starts with and its element count (the others grow on demand)
  const Want device_bufs[] = {
      want(c->d_c1, n_lam), want(c->d_hcl, n_lam), want(c->d_sig, n_lam), want(c->d_ftoa, n_lam),
      want(c->d_wtr, n_lam), want(c->d_p, NL), want(c->d_lnp, NL), want(c->d_Fu, F),
      want(c->d_Fd, F), want(c->T_buf[0], NL * A), want(c->T_buf[1], NL * A),
      want(c->T_buf[2], NL * A), want(c->d_epoch, NL), want(c->d_chain_err, 1),
      want(c->d_done, 1), want(c->d_dT, NL * A), want(c->d_bol, NL * 4 * A),
      want(c->d_mmr, NS * NL * A), want(c->d_steps, ns * A), want(c->d_terms, ns * NS * A),
      want(c->d_fsteps, ns * A), want(c->d_ssteps, ns * A),
      want(c->d_part, ns * 4 * (size_t)(4 * c->nblocks) * A), want(c->d_Fb, ns * 4 * A),
      want(c->d_Fb_all, ns * 4), want(c->d_conv, A), want(c->d_iter, A), want(c->d_Tb, NL * A),
      want(c->d_Ta, NL * A), want(c->d_flips, NL * A), want(c->d_prev, NL * A),
      want(c->d_ndiff, NL * A), want(c->d_g, A > 1 ? A : kNone)};
  const Want pinned_bufs[] = {
      want(c->h_flag, 2), want(c->h_err, 2), want(c->h_conv, A > 1 ? 2 * A : kNone),
      want(c->h_T, NL * A), want(c->h_dT, NL), want(c->h_bol, NL * 4), want(c->h_mmr, NS * NL * A)};
  for (const Want& w : device_bufs)
    if (w.n != kNone && (rc = w.alloc(w.buf, w.n))) return bail(rc);
  for (const Want& w : pinned_bufs)
    if (w.n != kNone && w.alloc(w.buf, w.n)) return bail(fail("hipHostMalloc failed"));
  c->d_T = c->d_T_home = c->T_buf[0];
  c->d_T_alt = c->T_buf[1];
  c->d_T3 = c->T_buf[2];
  c->h_err[0] = c->h_err[1] = 0;
  if (c->flag_ev[0].create(hipEventDisableTiming) || c->flag_ev[1].create(hipEventDisableTiming) ||
      c->mmr_ev.create(hipEventDisableTiming))
    return bail(fail("hipEventCreate failed"));
  // stream-ordered (the context's stream does not synchronise with the null stream)
  if (hipMemsetAsync(c->d_Fu, 0, F * sizeof(double), c->stream) != hipSuccess ||
      hipMemsetAsync(c->d_Fd, 0, F * sizeof(double), c->stream) != hipSuccess ||
      hipMemsetAsync(c->d_conv, 0, sizeof(int) * A, c->stream) != hipSuccess ||
      hipMemsetAsync(c->d_done, 0, sizeof(unsigned), c->stream) != hipSuccess ||
      hipMemsetAsync(c->d_epoch, 0, sizeof(unsigned long long) * NL, c->stream) != hipSuccess ||
      hipMemsetAsync(c->d_chain_err, 0, sizeof(int), c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return bail(fail("hipMemsetAsync failed"));
  *out = c;
  return 0;
}

int frei_ctx_create(frei_ctx** out, int device, int n_layers, int64_t n_lam, int n_species) {
  return ctx_create(out, device, n_layers, n_lam, n_species, 1);
}

int frei_ctx_create_batch(frei_ctx** out, int device, int n_layers, int64_t n_lam,
                          int n_species, int n_atm) {
  TRY(ctx_create(out, device, n_layers, n_lam, n_species, n_atm));
  (*out)->batch_api = true;
  return 0;
}

int frei_ctx_destroy(frei_ctx* c) {
  if (c) delete c;
  return 0;
}

int frei_set_grid(frei_ctx* c, const double* c1, const double* lk, const double* sigma,
                  const double* f_toa, const double* trapz_w, const double* p, double g,
                  double m_bar) {
  if (!c || !c1 || !lk || !sigma || !f_toa || !trapz_w || !p) return fail("null argument");
  if (!(g > 0) || !(m_bar > 0)) return fail("g and m_bar must be positive");
  TRY(set_device(c));
  const int64_t n = c->nlam;
  c->p.assign(p, p + c->nL);
  for (int l = 1; l < c->nL; ++l)
    if (!(c->p[l] < c->p[l - 1])) return fail("pressures must be strictly descending (BOA first)");
  // emit's top layer: p_2 = p[-1] * p[-2] / p[-3] (twostream.py:359)
  c->p_top2 = c->p[c->nL - 1] * c->p[c->nL - 2] / c->p[c->nL - 3];
  c->g = g;
  c->m_bar = m_bar;
  if (c->n_atm > 1) {  // default gravity of every atmosphere (frei_set_gravity overrides)
    std::vector<double> gv(c->n_atm, g);
    TRY(h2d_wait(c->d_g, gv.data(), gv.size(), c->stream));
  }
  TRY(h2d_wait(c->d_c1, c1, n, c->stream));
  {   // the Planck exponent's per-wavelength factor hc / (lam k_B) (kernels: times 1 / T)
    std::vector<double> hcl(n);
    for (int64_t j = 0; j < n; ++j) hcl[j] = kHC / lk[j];
    TRY(h2d_wait(c->d_hcl, hcl.data(), n, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // hcl is a temporary
  }
  TRY(h2d_wait(c->d_sig, sigma, n, c->stream));
  TRY(h2d_wait(c->d_ftoa, f_toa, n, c->stream));
  c->ftoa_per_atm = false;   // one F_TOA for every atmosphere again
  TRY(h2d_wait(c->d_wtr, trapz_w, n, c->stream));
  TRY(h2d_wait(c->d_p, c->p.data(), c->nL, c->stream));
  launch_log_ratio(c->d_p, c->p_top2, c->nL, c->d_lnp, c->stream);
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->grid_set = true;
  c->meta_dirty = true;
  return 0;
}

// Ascending order of the temperature nodes: tables are stored with the T axis sorted so
// that the upper bracket row is always the next row (row_hi = row_lo + n_lam).
static std::vector<int32_t> t_order(const double* T_nodes, int n_T) {
  std::vector<int32_t> perm(n_T);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(),
                   [&](int a, int b) { return T_nodes[a] < T_nodes[b]; });
  return perm;
}

// Begins species s's table on the nodes (dyn cm^-2, K; T in any order): sized, zeroed, the nodes
// recorded with T ascending and the row order in q.rank.  Every setter starts here (the table
// path: DESIGN.md, "Table path of the opacity setters"), writes the rows at node_offset() and
// ends in scan_nan().
static int set_table_common(frei_ctx* c, int s, const double* p_nodes, int n_p,
                            const double* T_nodes, int n_T) {
  if (s < 0 || s >= c->S) return fail("species index out of range");
  if (n_p < 2) return fail("a table needs at least 2 pressure nodes");
  if (n_T < 1) return fail("a table needs at least 1 temperature node");
  Species& q = c->sp[s];
  const int64_t stride = (c->nlam + 63) / 64 * 64;
  const size_t need = (size_t)n_p * n_T * (size_t)stride + 64;
  // queued sweeps of the old tables must finish before they are overwritten or freed
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!q.d_tab || (size_t)q.n_p * q.n_T != (size_t)n_p * n_T) {
    TRY(q.d_tab.alloc(need));
  }
  // finite padding; on the context's stream, ordered before the table upload / generation.
  // (A null-stream hipMemset is not ordered with the non-blocking stream: it could still be
  // zeroing the table while gen_table_kernel writes it — the intermittent C5 results of round 2.)
  HIP_TRY(hipMemsetAsync(q.d_tab, 0, need * sizeof(double), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // before frei_set_table's blocking host copies
  q.stride = stride;
  q.n_p = n_p;
  q.n_T = n_T;
  q.p_nodes.assign(p_nodes, p_nodes + n_p);
  const std::vector<int32_t> perm = t_order(T_nodes, n_T);
  q.T_nodes.resize(n_T);
  q.rank.resize(n_T);
  for (int t = 0; t < n_T; ++t) {
    q.T_nodes[t] = T_nodes[perm[t]];  // stored ascending
    q.rank[perm[t]] = t;
  }
  c->kmix_lib = nullptr;   // a new table ends a k-mix batch (frei_set_table_kmix_batch sets it after)
  c->meta_dirty = true;
  return 0;
}

// Device NaN scan of species s's table: the sweep drops the per-species NaN skip of the
// reference's nansum (Q8) when no table can produce a NaN.
static int scan_nan(frei_ctx* c, int s) {
  Species& q = c->sp[s];
  int h = 1;
  TRY(scan_tables(c, q.d_tab, 0, (int64_t)q.n_p * q.n_T * q.stride, 1, &h));
  q.has_nan = h;
  return 0;
}

int frei_set_table(frei_ctx* c, int s, const double* values, const double* p_nodes, int n_p,
                   const double* T_nodes, int n_T) {
  if (!c || !values || !p_nodes || !T_nodes) return fail("null argument");
  TRY(set_device(c));
  TRY(set_table_common(c, s, p_nodes, n_p, T_nodes, n_T));
  const Species& q = c->sp[s];
  bool ident = true;
  for (int t = 0; t < n_T; ++t) ident = ident && q.rank[t] == t;
  const size_t row = (size_t)c->nlam;
  if (ident) {
    HIP_TRY(hipMemcpy2D(q.d_tab, (size_t)q.stride * sizeof(double), values, row * sizeof(double),
                        row * sizeof(double), (size_t)n_p * n_T, hipMemcpyHostToDevice));
  } else {
    for (int kp = 0; kp < n_p; ++kp)
      for (int kt = 0; kt < n_T; ++kt)
        HIP_TRY(hipMemcpy(q.d_tab + node_offset(q, kp, kt), values + ((size_t)kp * n_T + kt) * row,
                          row * sizeof(double), hipMemcpyHostToDevice));
  }
  return scan_nan(c, s);
}

int frei_set_table_separable(frei_ctx* c, int s, const double* base, const double* fp,
                             const double* fT, double lo, double hi, const double* p_nodes,
                             int n_p, const double* T_nodes, int n_T) {
  if (!c || !base || !fp || !fT || !p_nodes || !T_nodes) return fail("null argument");
  TRY(set_device(c));
  TRY(set_table_common(c, s, p_nodes, n_p, T_nodes, n_T));
  const Species& q = c->sp[s];
  std::vector<double> fT_sorted(n_T);   // (outlives finish(): the uploads are queued)
  for (int t = 0; t < n_T; ++t) fT_sorted[q.rank[t]] = fT[t];
  DeviceCall call(c->stream, "separable table");
  const double* d_base = call.upload(base, (size_t)c->nlam);
  const double* d_fp = call.upload(fp, (size_t)n_p);
  const double* d_fT = call.upload(fT_sorted.data(), (size_t)n_T);
  if (call.ok())
    launch_gen_table(q.d_tab, d_base, d_fp, d_fT, n_p, n_T, c->nlam, q.stride, lo, hi, c->stream);
  call.end();
  TRY(call.finish());
  return scan_nan(c, s);
}

// Element offset in q's table of the row of every node (kp, kt) of the caller, [n_p * n_T].
static std::vector<int64_t> node_row_offsets(const Species& q) {
  std::vector<int64_t> row_off((size_t)q.n_p * q.n_T);
  for (int kp = 0; kp < q.n_p; ++kp)
    for (int kt = 0; kt < q.n_T; ++kt) row_off[(size_t)kp * q.n_T + kt] = node_offset(q, kp, kt);
  return row_off;
}

// The one body of the setters whose table the device writes (K6, K18, K19): species s's table on
// the nodes p_bar (bar) and T_nodes (K, any order) is begun, fill(row_off, d_tab) writes the row
// of node (kp, kt) at d_tab + row_off[kp * n_T + kt] and returns when it is complete, and the
// table is scanned for NaN.
using TableFill = std::function<int(const int64_t* row_off, double* d_tab)>;
static int set_table_filled(frei_ctx* c, int s, const double* p_bar, int n_p,
                            const double* T_nodes, int n_T, const TableFill& fill) {
  TRY(set_device(c));
  std::vector<double> p_cgs(n_p > 0 ? n_p : 0);
  for (int k = 0; k < n_p; ++k) p_cgs[k] = p_bar[k] * 1e6;  // bar -> dyn cm^-2
  TRY(set_table_common(c, s, p_cgs.data(), n_p, T_nodes, n_T));
  TRY(fill(node_row_offsets(c->sp[s]).data(), c->sp[s].d_tab));
  return scan_nan(c, s);
}

int frei_set_table_binned(frei_ctx* c, int s, frei_xsec* x, int mode, const double* wl_bins,
                          const double* lam, int64_t n_bins, int64_t lam_lo,
                          const double* T_nodes, int n_T, const double* p_nodes, int n_p) {
  if (!c || !x || !wl_bins || !lam || !T_nodes || !p_nodes) return fail("null argument");
  return set_table_filled(c, s, p_nodes, n_p, T_nodes, n_T,
                          [&](const int64_t* row_off, double* d_tab) {
    return bin_into_table(x, mode, wl_bins, lam, n_bins, lam_lo, c->nlam, T_nodes, n_T, p_nodes,
                          n_p, row_off, d_tab, c->device);
  });
}

int frei_set_table_kdist(frei_ctx* c, int s, frei_xsec* x, const double* wl_bins, int64_t n_bins,
                         int n_g, const double* g, const double* T_nodes, int n_T,
                         const double* p_nodes, int n_p, int64_t col_lo) {
  if (!c || !x || !wl_bins || !g || !T_nodes || !p_nodes) return fail("null argument");
  return set_table_filled(c, s, p_nodes, n_p, T_nodes, n_T,
                          [&](const int64_t* row_off, double* d_tab) {
    return kdist_into_table(x, wl_bins, n_bins, n_g, g, col_lo, c->nlam, T_nodes, n_T, p_nodes,
                            n_p, row_off, d_tab, c->device);
  });
}

// K19's fill of a whole table: every node of the one composition x (already checked), on the
// context's stream (the library's tables are complete when frei_klib_set* return).
static TableFill kmix_table_fill(frei_ctx* c, const std::string& me, frei_klib* lib,
                                 const double* x, int64_t col_lo, int n_nodes) {
  return [=](const int64_t* row_off, double* d_tab) {
    std::vector<KmixRow> rows((size_t)n_nodes);
    for (int nd = 0; nd < n_nodes; ++nd) rows[nd] = KmixRow{0, nd, row_off[nd]};
    return kmix_rows_into(me, lib, 1, x, col_lo, c->nlam, rows.data(), rows.size(), d_tab,
                          c->stream);
  };
}

int frei_set_table_kmix(frei_ctx* c, int s, frei_klib* lib, const double* x, int64_t col_lo) {
  const std::string me = "frei_set_table_kmix: ";
  if (!c || !lib || !x) return fail("null argument");
  KlibNodes nd{};
  TRY(klib_batch_args(me, lib, 1, x, col_lo, c->nlam, c->device, &nd));
  return set_table_filled(c, s, nd.p, nd.n_p, nd.T, nd.n_T,
                          kmix_table_fill(c, me, lib, x, col_lo, nd.n_p * nd.n_T));
}

int frei_set_table_kmix_batch(frei_ctx* c, frei_klib* lib, const double* x, int64_t col_lo) {
  const std::string me = "frei_set_table_kmix_batch: ";
  if (!c || !lib || !x) return fail(me + "null argument");
  if (!c->batch_api) return fail(me + "needs a context from frei_ctx_create_batch");
  if (c->S != 1)
    return fail(me + "needs n_species = 1 (the mixture is the one species), not n_species = " +
                std::to_string(c->S));
  if (!c->grid_set) return fail(me + "frei_set_grid must be called first");
  if (c->chem_on)
    return fail(me + "the context holds chemistry tables (frei_set_chemistry_batch); a k-mix "
                     "batch's compositions hold the mixing ratios");
  KlibNodes nd{};
  TRY(klib_batch_args(me, lib, c->n_atm, x, col_lo, c->nlam, c->device, &nd));
  // species 0: the nodes and composition 0's mixture
  TRY(set_table_filled(c, 0, nd.p, nd.n_p, nd.T, nd.n_T,
                       kmix_table_fill(c, me, lib, x, col_lo, nd.n_p * nd.n_T)));
  c->kmix_x.assign(x, x + (size_t)c->n_atm * nd.n_src * nd.n_p * nd.n_T);
  c->kmix_col_lo = col_lo;
  c->kmix_nsrc = nd.n_src;
  c->kmix_lib = lib;
  c->mmr.assign((size_t)c->nL * c->n_atm, 1.0);
  c->meta_dirty = true;
  return build_meta(c);   // the per-atmosphere tables are mixed here
}

int frei_kmix_batch_update(frei_ctx* c, int atm_lo, int n, const double* x) {
  const std::string me = "frei_kmix_batch_update: ";
  if (!c || !x) return fail(me + "null argument");
  if (!c->kmix_lib)
    return fail(me + "the context holds no k-mix batch (frei_set_table_kmix_batch)");
  if (atm_lo < 0 || n < 1 || (int64_t)atm_lo + n > c->n_atm)
    return fail(me + "atmospheres [" + std::to_string(atm_lo) + ", " +
                std::to_string((int64_t)atm_lo + n) + ") lie outside [0, n_atm = " +
                std::to_string(c->n_atm) + ")");
  TRY(klib_batch_args(me, c->kmix_lib, n, x, c->kmix_col_lo, c->nlam, c->device, nullptr));
  TRY(set_device(c));
  const Species& q0 = c->sp[0];
  const size_t per_x = (size_t)c->kmix_nsrc * q0.n_p * q0.n_T;
  std::copy(x, x + (size_t)n * per_x, c->kmix_x.begin() + (size_t)atm_lo * per_x);
  if (c->n_atm == 1) {   // the one atmosphere sweeps species 0's table: re-mixed in place, on the
                         // context's stream behind the sweeps that still read it
    const TableFill remix = kmix_table_fill(c, me, c->kmix_lib, x, c->kmix_col_lo, q0.n_p * q0.n_T);
    TRY(remix(node_row_offsets(q0).data(), q0.d_tab));
    const int had = q0.has_nan;
    TRY(scan_nan(c, 0));
    if (c->sp[0].has_nan != had) c->meta_dirty = true;   // the sweep's NaN skip changes
    return 0;
  }
  if (c->meta_dirty) return 0;   // the next metadata build mixes every atmosphere
  const int rc = kmix_fill(c, atm_lo, n, me);
  if (rc) c->meta_dirty = true;   // no run on a table that holds a NaN
  return rc;
}

int frei_get_table_batch(frei_ctx* c, int atm, double* out) {
  const std::string me = "frei_get_table_batch: ";
  if (!c || !out) return fail(me + "null argument");
  if (!c->batch_api) return fail(me + "needs a context from frei_ctx_create_batch");
  if (atm < 0 || atm >= c->n_atm)
    return fail(me + "atmosphere " + std::to_string(atm) + " lies outside [0, n_atm = " +
                std::to_string(c->n_atm) + ")");
  TRY(set_device(c));
  TRY(build_meta(c));
  if (!c->eff && c->S != 1)
    return fail(me + "the sweeps of this context sum the species themselves: it has no "
                     "per-atmosphere table");
  const Species& q0 = c->sp[0];
  const double* src = c->eff ? c->d_eff + (size_t)atm * c->eff_stride : q0.d_tab;
  const size_t rows = (size_t)q0.n_p * q0.n_T, n = (size_t)c->nlam;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!c->kmix_lib) {   // as stored: T ascending
    HIP_TRY(hipMemcpy2D(out, n * sizeof(double), src, (size_t)q0.stride * sizeof(double),
                        n * sizeof(double), rows, hipMemcpyDeviceToHost));
    return 0;
  }
  // a k-mix batch: the rows in the library's node order
  std::vector<double> tmp(rows * (size_t)q0.stride);
  HIP_TRY(hipMemcpy(tmp.data(), src, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int kp = 0; kp < q0.n_p; ++kp)
    for (int kt = 0; kt < q0.n_T; ++kt)
      std::memcpy(out + ((size_t)kp * q0.n_T + kt) * n, tmp.data() + node_offset(q0, kp, kt),
                  n * sizeof(double));
  return 0;
}

int frei_set_mmr(frei_ctx* c, const double* mmr) {
  if (!c || !mmr) return fail("null argument");
  if (c->kmix_lib) {   // K20: every mixing ratio of a k-mix batch is 1 and stays 1
    for (size_t i = 0; i < (size_t)c->nL * c->n_atm; ++i)
      if (mmr[i] != 1.0)
        return fail("frei_set_mmr: mmr[" + std::to_string(i) + "] = " + std::to_string(mmr[i]) +
                    " on a k-mix batch: the compositions hold the mixing ratios");
    return 0;
  }
  const size_t n = (size_t)c->S * c->nL * c->n_atm;
  // A chemistry provider evaluated between sweeps (T-dependent, frei_amd Engine) sets new mixing
  // ratios before every sweep.  When the metadata is built and the sweep sums the species itself
  // (no contraction K3 formed from the old ratios), nothing else depends on them: they only go up
  // to the device before the next sweep forms its step records — not a metadata rebuild (bracket
  // searches, uploads and stream synchronizations) per sweep.
  const bool light = !c->meta_dirty && !c->eff && c->mmr.size() == n && c->d_mmr != nullptr;
  c->mmr.assign(mmr, mmr + n);
  if (light) c->mmr_dirty = true;
  else c->meta_dirty = true;
  return 0;
}

int frei_set_ftoa_batch(frei_ctx* c, const double* f_toa) {
  if (!c || !f_toa) return fail("null argument");
  if (c->n_atm < 2) return fail("frei_set_ftoa_batch needs a batched context (frei_set_grid sets F_TOA)");
  if (!c->grid_set) return fail("frei_set_grid must be called first");
  TRY(set_device(c));
  const size_t n = (size_t)c->nlam * c->n_atm;
  DeviceCall call(c->stream, "F_TOA upload");
  double* d = call.upload(f_toa, n);
  call.keep(d);
  TRY(call.finish());   // (queued sweeps have finished with the old F_TOA too)
  c->d_ftoa.adopt(d, n);
  c->ftoa_per_atm = true;
  return 0;
}

// The chemistry tables of a context: n_tab tables values[n_tab][S][n_T][n_p] on shared nodes;
// atm_tab[n_atm] names each atmosphere's table (nullptr: one table, frei_set_chemistry).
static int set_chem_tables(frei_ctx* c, const double* values, int n_tab, const int32_t* atm_tab,
                           const double* T_nodes, int n_T, const double* p_nodes, int n_p) {
  if (!T_nodes || !p_nodes || n_T < 1 || n_p < 1) return fail("chemistry table needs nodes");
  for (int k = 1; k < n_T; ++k)
    if (!(T_nodes[k] > T_nodes[k - 1])) return fail("chemistry T nodes must ascend");
  for (int k = 0; k < n_p; ++k)
    if (!(p_nodes[k] > 0) || (k > 0 && !(p_nodes[k] > p_nodes[k - 1])))
      return fail("chemistry p nodes must be positive and ascend");
  const int nL = c->nL;
  const size_t nv = (size_t)n_tab * c->S * n_T * n_p;
  HIP_TRY(hipStreamSynchronize(c->stream));   // no queued update still reads the old tables
  c->chem_tab.assign(values, values + nv);
  c->chem_T.assign(T_nodes, T_nodes + n_T);
  c->chem_logp.resize(n_p);
  for (int k = 0; k < n_p; ++k) c->chem_logp[k] = std::log10(p_nodes[k]);
  std::vector<int32_t> pj(nL);
  std::vector<double> pz(nL);
  for (int l = 0; l < nL; ++l)   // layer pressures are fixed: their log10 p brackets once
    chem_bracket(c->chem_logp.data(), n_p, std::log10(c->p[l]), pj[l], pz[l]);
  c->d_chem_atm.reset();
  c->chem_on = false;
  TRY(c->d_chem_tab.alloc(nv));
  TRY(c->d_chem_T.alloc(n_T));
  TRY(c->d_chem_pj.alloc(nL));
  TRY(c->d_chem_pz.alloc(nL));
  TRY(h2d_wait(c->d_chem_tab, c->chem_tab.data(), nv, c->stream));
  TRY(h2d_wait(c->d_chem_T, c->chem_T.data(), n_T, c->stream));
  TRY(h2d_wait(c->d_chem_pj, pj.data(), nL, c->stream));
  TRY(h2d_wait(c->d_chem_pz, pz.data(), nL, c->stream));
  c->chem_atm.clear();
  if (atm_tab) {
    c->chem_atm.assign(atm_tab, atm_tab + c->n_atm);
    TRY(c->d_chem_atm.alloc(c->n_atm));
    TRY(h2d_wait(c->d_chem_atm, c->chem_atm.data(), c->n_atm, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->chem_ntab = n_tab;
  c->chem_nT = n_T;
  c->chem_np = n_p;
  c->chem_on = true;
  c->meta_dirty = true;   // the species contraction (K3 / K7) no longer applies
  return 0;
}

int frei_set_chemistry(frei_ctx* c, const double* values, const double* T_nodes, int n_T,
                       const double* p_nodes, int n_p) {
  if (!c) return fail("null argument");
  if (!c->grid_set) return fail("frei_set_grid must be called first");
  TRY(set_device(c));
  if (!values) {   // back to the fixed per-layer mmr arrays
    c->chem_on = false;
    c->meta_dirty = true;
    return 0;
  }
  if (c->n_atm > 1) return fail("a chemistry table is per atmosphere: not for batched contexts");
  return set_chem_tables(c, values, 1, nullptr, T_nodes, n_T, p_nodes, n_p);
}

int frei_set_chemistry_batch(frei_ctx* c, const double* values, int n_tab,
                             const int32_t* atm_tab, const double* T_nodes, int n_T,
                             const double* p_nodes, int n_p) {
  if (!c) return fail("null argument");
  if (!c->batch_api)
    return fail("frei_set_chemistry_batch needs a context from frei_ctx_create_batch "
                "(a single context takes frei_set_chemistry)");
  if (!c->grid_set) return fail("frei_set_grid must be called first");
  TRY(set_device(c));
  if (!values) {   // back to frei_set_mmr's fixed arrays and the contracted path
    c->chem_on = false;
    c->meta_dirty = true;
    return 0;
  }
  if (c->kmix_lib)
    return fail("frei_set_chemistry_batch: the context holds a k-mix batch "
                "(frei_set_table_kmix_batch); its compositions hold the mixing ratios");
  if (n_tab < 1) return fail("n_tab must be >= 1");
  if (!atm_tab) return fail("null atm_tab");
  for (int m = 0; m < c->n_atm; ++m)
    if (atm_tab[m] < 0 || atm_tab[m] >= n_tab)
      return fail("atm_tab[" + std::to_string(m) + "] = " + std::to_string(atm_tab[m]) +
                  " is outside [0, n_tab)");
  return set_chem_tables(c, values, n_tab, atm_tab, T_nodes, n_T, p_nodes, n_p);
}

int frei_set_gravity(frei_ctx* c, const double* g) {
  if (!c || !g) return fail("null argument");
  if (c->n_atm < 2) return fail("frei_set_gravity needs a batched context (frei_set_grid sets g)");
  for (int m = 0; m < c->n_atm; ++m)
    if (!(g[m] > 0)) return fail("g must be positive");
  TRY(set_device(c));
  TRY(h2d_wait(c->d_g, g, c->n_atm, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int frei_set_fluxes(frei_ctx* c, const double* up, const double* down) {
  if (!c) return fail("null argument");
  TRY(set_device(c));
  const size_t F = (size_t)c->nL * c->nlam * c->n_atm;
  if (up) TRY(h2d_wait(c->d_Fu, up, F, c->stream));
  if (down) TRY(h2d_wait(c->d_Fd, down, F, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int frei_get_fluxes(frei_ctx* c, double* up, double* down) {
  if (!c) return fail("null argument");
  TRY(set_device(c));
  const size_t F = (size_t)c->nL * c->nlam * c->n_atm;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (up) HIP_TRY(hipMemcpy(up, c->d_Fu, F * sizeof(double), hipMemcpyDeviceToHost));
  if (down) HIP_TRY(hipMemcpy(down, c->d_Fd, F * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int frei_get_spectrum(frei_ctx* c, double* spec) {
  if (!c || !spec) return fail("null argument");
  if (c->n_atm > 1) return fail("frei_get_spectrum is per atmosphere: use frei_run_batch");
  TRY(set_device(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(spec, c->d_Fu + (size_t)(c->nL - 1) * c->nlam, c->nlam * sizeof(double),
                    hipMemcpyDeviceToHost));
  return 0;
}

int frei_set_temperatures(frei_ctx* c, const double* T) {
  if (!c || !T) return fail("null argument");
  const size_t n = (size_t)c->nL * c->n_atm;
  for (size_t l = 0; l < n; ++l)
    if (!(T[l] > 0)) return fail("temperatures must be positive");
  TRY(set_device(c));
  home_temperatures(c);
  TRY(h2d_wait(c->d_T, T, n, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int frei_get_temperatures(frei_ctx* c, double* T) {
  if (!c || !T) return fail("null argument");
  TRY(set_device(c));
  const size_t n = (size_t)c->nL * c->n_atm;
  HIP_TRY(hipMemcpyAsync(c->h_T, c->d_T, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::memcpy(T, c->h_T, n * sizeof(double));
  return 0;
}

int frei_sweep(frei_ctx* c, int direction, double alpha, double* dT, double* bol,
               double* dtaus) {
  if (c && c->n_atm > 1) return fail("frei_sweep is per atmosphere: use frei_iterate / frei_run_batch");
  if (!ready(c)) return fail("context not ready (frei_set_grid)");
  if (direction != FREI_EMIT && direction != FREI_ABSORB) return fail("bad direction");
  TRY(set_device(c));
  TRY(build_meta(c));
  SweepOpts o;
  o.dir = direction;
  o.force = 1;
  o.alpha = alpha;
  o.dT_out = c->d_dT;
  o.bol_out = c->d_bol;
  if (dtaus) {
    TRY(ensure_dtaus(c));
    o.dtaus = c->d_dtaus;
  }
  c->dtaus_valid = false;
  c->dtaus_batch_valid = false;
  launch_setup(setup_args(c), direction, c->stream);
  HIP_TRY(hipGetLastError());
  TRY(run_sweep(c, o));
  // the small results through pinned staging, ordered on the stream: one synchronisation
  if (dT) HIP_TRY(hipMemcpyAsync(c->h_dT, c->d_dT, c->nL * sizeof(double), hipMemcpyDeviceToHost,
                                 c->stream));
  if (bol) HIP_TRY(hipMemcpyAsync(c->h_bol, c->d_bol, c->nL * 4 * sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  TRY(check_comm(c));
  if (dT) std::memcpy(dT, c->h_dT, c->nL * sizeof(double));
  if (bol) {
    std::memcpy(bol, c->h_bol, c->nL * 4 * sizeof(double));
    // rows of layers a sweep does not visit are undefined on the device: zero them
    const int skip = (direction == FREI_EMIT) ? 0 : c->nL - 1;
    for (int q = 0; q < 4; ++q) bol[skip * 4 + q] = 0.0;
  }
  if (dtaus)
    HIP_TRY(hipMemcpy(dtaus, c->d_dtaus, (size_t)c->nL * c->nlam * sizeof(double),
                      hipMemcpyDeviceToHost));
  return 0;
}

int frei_state_init(frei_ctx* c, const double* T_init) {
  if (!ready(c) || !T_init) return fail("context not ready or null T_init");
  TRY(set_device(c));
  c->dtaus_batch_valid = false;   // the kept dtaus belong to the state this call replaces
  TRY(build_meta(c));
  c->has_pend = false;   // an update deferred by an interrupted run must not land on the new T
  home_temperatures(c);
  TRY(h2d_wait(c->d_T, T_init, (size_t)c->nL * c->n_atm, c->stream));
  const size_t F = (size_t)c->nL * c->nlam * c->n_atm;
  HIP_TRY(hipMemsetAsync(c->d_Fu, 0, F * sizeof(double), c->stream));  // core.py:265-266
  HIP_TRY(hipMemsetAsync(c->d_Fd, 0, F * sizeof(double), c->stream));
  TRY(reset_loop_state(c));
  launch_setup(setup_args(c), kEmit, c->stream, c->n_atm);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int iterate_steps(frei_ctx* c, int n, int nzc, double thr, double alpha, bool stop);

// An error part-way leaves no update deferred (drop_pending): a later frei_state_init + sweep
// must not flush a stale one over the freshly uploaded temperatures, and a read without
// frei_state_init sees the deferred update's input temperatures, not its poisoned output.
static int iterate_direct(frei_ctx* c, int n, int nzc, double thr, double alpha, bool stop) {
  const int rc = iterate_steps(c, n, nzc, thr, alpha, stop);
  if (rc != 0) drop_pending(c);
  return rc;
}

static int iterate_steps(frei_ctx* c, int n, int nzc, double thr, double alpha, bool stop) {
  for (int it = 0; it < n; ++it) {
    SweepOpts e;
    e.dir = kEmit;
    e.next_dir = kAbsorb;
    e.track = 1;
    e.alpha = alpha;
    e.live_only = 1;
    TRY(run_sweep(c, e, true));
    SweepOpts a = e;
    a.dir = kAbsorb;
    a.next_dir = kEmit;
    a.stop_on_conv = stop ? 1 : 0;
    a.n_zero_crossings = nzc;
    a.convergence_dT = thr;
    TRY(run_sweep(c, a, true));
  }
  return flush_update(c);   // no call returns with an update still deferred
}

// Graph replay applies when one iteration is two fused launches pairs on one rank with no
// per-launch host work (no events, no exchange), i.e. when its kernel arguments repeat.
static bool graph_ok(frei_ctx* c) {
  return c->use_graph && c->graph_iters > 0 && !c->timing && c->fused_update && c->n_atm == 1 &&
         c->nranks == 1 && !c->comm && !c->d_mbox;
}

static int iterate(frei_ctx* c, int n, int nzc, double thr, double alpha, bool stop) {
  const int G = c->graph_iters;
  if (!graph_ok(c) || n < G) return iterate_direct(c, n, nzc, thr, alpha, stop);
  // the hashes of one iteration's launches as they would be issued now
  std::vector<uint64_t> key;
  c->keys = &key;
  c->dry = true;
  // the dry pass launches nothing, so it must leave no state behind that a real sweep reads:
  // run_sweep clears / sets rec_skipped as it would for real launches
  const bool rec_skipped = c->rec_skipped;
  const int rc = iterate_direct(c, 1, nzc, thr, alpha, stop);
  c->rec_skipped = rec_skipped;
  c->dry = false;
  c->keys = nullptr;
  TRY(rc);
  // sweep, fused update, sweep, fused update (0: a launch that is not replayable)
  const bool fused_only = key.size() == 4 && std::find(key.begin(), key.end(), 0ull) == key.end();
  if (!fused_only) return iterate_direct(c, n, nzc, thr, alpha, stop);
  if (!c->g_exec || key != c->g_key) {
    if (c->g_exec) (void)hipGraphExecDestroy(c->g_exec);
    c->g_exec = nullptr;
    c->g_key.clear();
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    const int rc2 = iterate_direct(c, G, nzc, thr, alpha, stop);
    const hipError_t e = hipStreamEndCapture(c->stream, &g);
    TRY(rc2);
    if (e != hipSuccess) return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(&c->g_exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
      c->g_exec = nullptr;
      return fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
    }
    c->g_key = key;
    ++c->g_captures;
    // the capture swapped the temperature buffers 2 G times: an even count, back in place
  }
  int done = 0;
  for (; done + G <= n; done += G) {
    HIP_TRY(hipGraphLaunch(c->g_exec, c->stream));
    ++c->g_replays;
  }
  return iterate_direct(c, n - done, nzc, thr, alpha, stop);
}

int frei_iterate(frei_ctx* c, int n, int n_zero_crossings, double convergence_dT,
                 double alpha) {
  if (!ready(c)) return fail("context not ready");
  TRY(set_device(c));
  c->dtaus_batch_valid = false;
  TRY(ensure_hist(c, 1));
  const bool stop = n_zero_crossings >= 0;
  return iterate(c, n, stop ? n_zero_crossings : 0x7fffffff, convergence_dT, alpha, stop);
}

int frei_graph_info(frei_ctx* c, int* captures, int* replays) {
  if (!c) return fail("null argument");
  if (captures) *captures = c->g_captures;
  if (replays) *replays = c->g_replays;
  return 0;
}

int frei_comm_shared_device(frei_ctx* c, int shared) {
  if (!c) return fail("null argument");
  c->shared_device = shared != 0;
  return 0;
}

int frei_device_pci_bus_id(int device, char* buf, int len) {
  if (!buf || len < 16) return fail("null argument or buffer under 16 bytes");
  HIP_TRY(hipDeviceGetPCIBusId(buf, len, device));
  return 0;
}

int frei_tail_info(frei_ctx* c, int64_t* launches) {
  if (!c || !launches) return fail("null argument");
  *launches = c->n_tail;
  return 0;
}

int frei_chain_info(frei_ctx* c, int64_t* chained) {
  if (!c || !chained) return fail("null argument");
  *chained = c->n_chained;
  return 0;
}

int frei_synchronize(frei_ctx* c) {
  if (!c) return fail("null argument");
  TRY(set_device(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return check_comm(c);
}

int frei_run(frei_ctx* c, const double* T_init, int n_timesteps, int n_zero_crossings,
             double convergence_dT, double alpha, int* n_iter, double* T_final,
             double* temp_hist, double* dtaus, double* spectrum) {
  if (!ready(c) || !T_init || !n_iter) return fail("context not ready or null argument");
  if (c->n_atm > 1) return fail("batched context: use frei_run_batch");
  if (n_timesteps < 1) return fail("n_timesteps must be >= 1");
  TRY(set_device(c));
  TRY(ensure_hist(c, n_timesteps));
  TRY(frei_state_init(c, T_init));
  // device-resident loop; poll the convergence flag one chunk behind
  const int chunk = 4;
  int launched = 0, k = 0;
  while (launched < n_timesteps) {
    const int n = std::min(chunk, n_timesteps - launched);
    TRY(iterate(c, n, n_zero_crossings, convergence_dT, alpha, true));
    launched += n;
    HIP_TRY(hipMemcpyAsync(&c->h_flag[k & 1], c->d_conv, sizeof(int), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipEventRecord(c->flag_ev[k & 1], c->stream));
    if (k > 0) {
      HIP_TRY(hipEventSynchronize(c->flag_ev[(k - 1) & 1]));
      if (c->h_flag[(k - 1) & 1]) break;
    }
    ++k;
  }
  // final emit without alpha (alpha = 1, core.py:323-333), writes dtaus
  TRY(ensure_dtaus(c));
  c->dtaus_valid = true;
  SweepOpts f;
  f.dir = kEmit;
  f.force = 1;
  f.alpha = 1.0;
  f.dtaus = c->d_dtaus;
  TRY(run_sweep(c, f));
  HIP_TRY(hipStreamSynchronize(c->stream));
  TRY(check_comm(c));
  int it = 0;
  HIP_TRY(hipMemcpy(&it, c->d_iter, sizeof(int), hipMemcpyDeviceToHost));
  *n_iter = it;
  const int nL = c->nL;
  if (T_final) HIP_TRY(hipMemcpy(T_final, c->d_T, nL * sizeof(double), hipMemcpyDeviceToHost));
  if (temp_hist && it > 0) {
    std::vector<double> h((size_t)it * 2 * nL);
    HIP_TRY(hipMemcpy(h.data(), c->d_hist, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int l = 0; l < nL; ++l)
      for (int col = 0; col < 2 * it; ++col) temp_hist[(size_t)l * 2 * it + col] = h[(size_t)col * nL + l];
  }
  if (dtaus)
    HIP_TRY(hipMemcpy(dtaus, c->d_dtaus, (size_t)nL * c->nlam * sizeof(double),
                      hipMemcpyDeviceToHost));
  if (spectrum)
    HIP_TRY(hipMemcpy(spectrum, c->d_Fu + (size_t)(nL - 1) * c->nlam, c->nlam * sizeof(double),
                      hipMemcpyDeviceToHost));
  return 0;
}

int frei_run_batch(frei_ctx* c, const double* T_init, int n_timesteps, int n_zero_crossings,
                   double convergence_dT, double alpha, int* n_iter, double* T_final,
                   double* spectra) {
  return frei_run_batch_ex(c, T_init, n_timesteps, n_zero_crossings, convergence_dT, alpha,
                           n_iter, T_final, spectra, nullptr, 0);
}

int frei_run_batch_ex(frei_ctx* c, const double* T_init, int n_timesteps, int n_zero_crossings,
                      double convergence_dT, double alpha, int* n_iter, double* T_final,
                      double* spectra, double* temp_hist, int keep_dtaus) {
  if (!ready(c) || !T_init || !n_iter) return fail("context not ready or null argument");
  if (n_timesteps < 1) return fail("n_timesteps must be >= 1");
  TRY(set_device(c));
  TRY(ensure_hist(c, n_timesteps));
  c->dtaus_batch_valid = false;
  if (keep_dtaus) {   // before the state changes: a failed allocation leaves the context as it was
    TRY(ensure_dtaus_batch(c));
    c->dtaus_valid = false;   // the buffer no longer holds a frei_run's dtaus
  }
  TRY(frei_state_init(c, T_init));
  const int A = c->n_atm;
  int* flags = c->h_conv ? c->h_conv : c->h_flag;   // pinned [2][A]
  // every atmosphere iterates until its own convergence test holds (its kernels then
  // return at once); the host polls all flags one chunk behind
  const int chunk = 4;
  int launched = 0, k = 0;
  while (launched < n_timesteps) {
    const int n = std::min(chunk, n_timesteps - launched);
    TRY(iterate(c, n, n_zero_crossings, convergence_dT, alpha, true));
    launched += n;
    HIP_TRY(hipMemcpyAsync(flags + (k & 1) * A, c->d_conv, A * sizeof(int),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->flag_ev[k & 1], c->stream));
    if (k > 0) {
      HIP_TRY(hipEventSynchronize(c->flag_ev[(k - 1) & 1]));
      bool all = true;
      for (int m = 0; m < A; ++m) all = all && flags[((k - 1) & 1) * A + m] != 0;
      if (all) break;
    }
    ++k;
  }
  // final emit of every atmosphere without alpha (alpha = 1, core.py:323-333)
  SweepOpts f;
  f.dir = kEmit;
  f.force = 1;
  f.alpha = 1.0;
  if (keep_dtaus) f.dtaus = c->d_dtaus;   // every sweep form offsets it by the atmosphere
  TRY(run_sweep(c, f));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->dtaus_batch_valid = keep_dtaus != 0;
  HIP_TRY(hipMemcpy(n_iter, c->d_iter, A * sizeof(int), hipMemcpyDeviceToHost));
  const size_t nL = c->nL;
  if (temp_hist) {   // [n_atm][n_layers][2 * n_timesteps], zero past 2 * n_iter[m] columns
    const size_t cols = 2 * (size_t)n_timesteps;
    std::fill(temp_hist, temp_hist + (size_t)A * nL * cols, 0.0);
    std::vector<double> h;
    for (int m = 0; m < A; ++m) {
      const size_t it = (size_t)std::min(std::max(n_iter[m], 0), n_timesteps);
      if (it == 0) continue;
      h.resize(it * 2 * nL);
      HIP_TRY(hipMemcpy(h.data(), c->d_hist + (size_t)m * c->hist_cap * 2 * nL,
                        h.size() * sizeof(double), hipMemcpyDeviceToHost));
      double* out = temp_hist + (size_t)m * nL * cols;
      for (size_t l = 0; l < nL; ++l)
        for (size_t col = 0; col < 2 * it; ++col) out[l * cols + col] = h[col * nL + l];
    }
  }
  if (T_final)
    HIP_TRY(hipMemcpy(T_final, c->d_T, nL * A * sizeof(double), hipMemcpyDeviceToHost));
  if (spectra)  // F_up[n_layers - 1] of every atmosphere
    HIP_TRY(hipMemcpy2D(spectra, c->nlam * sizeof(double),
                        c->d_Fu + (nL - 1) * c->nlam, nL * c->nlam * sizeof(double),
                        c->nlam * sizeof(double), A, hipMemcpyDeviceToHost));
  return 0;
}

int frei_kappa(frei_ctx* c, double T, double p, double* k, double* sigma) {
  if (!ready(c) || !k) return fail("context not ready or null argument");
  if (c->n_atm > 1) return fail("frei_kappa is per atmosphere: use a single-atmosphere context");
  TRY(set_device(c));
  TRY(build_meta(c));
  std::vector<TermP> terms(c->S);
  for (int s = 0; s < c->S; ++s) {
    const Species& q = c->sp[s];
    const SpecMeta& sm = c->smeta[s];
    // pressure bracket of the query point (same rules as build_meta)
    std::vector<int32_t> pp(q.n_p);
    std::iota(pp.begin(), pp.end(), 0);
    std::stable_sort(pp.begin(), pp.end(),
                     [&](int a, int b) { return q.p_nodes[a] < q.p_nodes[b]; });
    std::vector<double> ps(q.n_p);
    for (int i = 0; i < q.n_p; ++i) ps[i] = q.p_nodes[pp[i]];
    PMeta pm{};
    if (sm.one_T) {
      int jx = (int)(std::lower_bound(ps.begin(), ps.end(), p) - ps.begin());
      jx = std::max(1, std::min(jx, q.n_p - 1));
      pm.p_lo = pp[jx - 1];
      pm.p_hi = pp[jx];
      pm.x1 = p - ps[jx - 1];
      pm.dx = ps[jx] - ps[jx - 1];
      pm.oob = (p < ps[0] || p > ps[q.n_p - 1]) ? 1 : 0;
    } else {
      int i, oob;
      double y;
      bracket(ps.data(), q.n_p, p, i, y, oob);
      pm.p_lo = pp[i];
      pm.p_hi = pp[i + 1];
      pm.wp_lo = 1.0 - y;
      pm.wp_hi = y;
      pm.oob = oob;
    }
    // mmr: the chemistry table at (T, p) when set (opacity.py:246-248), else the layer whose
    // pressure equals p, else the first layer's value
    double m = c->mmr[(size_t)s * c->nL];
    for (int l = 0; l < c->nL; ++l)
      if (c->p[l] == p) m = c->mmr[(size_t)s * c->nL + l];
    if (c->chem_on) {
      int j;
      double z;
      chem_bracket(c->chem_logp.data(), c->chem_np, std::log10(p), j, z);
      // (a batched context of one atmosphere: its own table of the n_tab)
      const size_t t0 = c->chem_atm.empty()
                            ? 0 : (size_t)c->chem_atm[0] * c->S * c->chem_nT * c->chem_np;
      ChemArgs h{c->chem_tab.data() + t0, c->chem_T.data(), nullptr, nullptr, c->chem_nT,
                 c->chem_np};
      m = chem_mmr_at(h, s, j, z, T);
    }
    terms[s] = make_term(sm, pm, c->tnodes.data(), c->tperm.data(), m, T, 0);
  }
  DevBuf<TermP> d_terms;
  DevBuf<double> d_k;
  TRY(d_terms.alloc(c->S));
  TRY(d_k.alloc(c->nlam));
  TRY(h2d_wait(d_terms, terms.data(), c->S, c->stream));
  launch_kappa(c->nlam, d_terms, c->S, c->d_sig, d_k, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(k, d_k, c->nlam * sizeof(double), hipMemcpyDeviceToHost));
  if (sigma) HIP_TRY(hipMemcpy(sigma, c->d_sig, c->nlam * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int frei_propagate_fluxes(int device, int64_t n, const double* c1, const double* lk,
                          const double* F_1_up, const double* F_2_down, double T_1,
                          double T_2, const double* delta_tau, const double* omega_0,
                          const double* g_0, double* F_2_up, double* F_1_down) {
  if (n <= 0) return 0;
  if (!c1 || !lk || !F_1_up || !F_2_down || !delta_tau || !omega_0 || !F_2_up || !F_1_down)
    return fail("null argument");
  HIP_TRY(hipSetDevice(device));
  // inputs c1, lk, F_1_up, F_2_down, delta_tau, omega_0 [, g_0]; outputs F_2_up, F_1_down
  const double* in[7] = {c1, lk, F_1_up, F_2_down, delta_tau, omega_0, g_0};
  const int n_in = g_0 ? 7 : 6;
  Stream st;   // (before the buffers: destroyed after them)
  DevBuf<double> d[9];
  int rc = 0;
  if (st.create()) return fail("hipStreamCreate failed");
  for (int i = 0; i < n_in + 2 && !rc; ++i) rc = d[i].alloc(n);
  for (int i = 0; i < n_in && !rc; ++i) rc = h2d_wait(d[i], in[i], n, st);
  if (!rc) {
    launch_propagate(n, d[0], d[1], d[2], d[3], T_1, T_2, d[4], d[5], g_0 ? d[6].get() : nullptr,
                     d[n_in], d[n_in + 1], st);
    if (hipGetLastError() != hipSuccess) rc = fail("propagate kernel launch failed");
  }
  if (!rc && (hipMemcpyAsync(F_2_up, d[n_in], n * sizeof(double), hipMemcpyDeviceToHost, st) !=
                  hipSuccess ||
              hipMemcpyAsync(F_1_down, d[n_in + 1], n * sizeof(double), hipMemcpyDeviceToHost,
                             st) != hipSuccess))
    rc = fail("propagate copy failed");
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail("propagate kernel failed");
  return rc;
}

int frei_comm_unique_id(void* id128) {
  if (!id128) return fail("null argument");
  Rccl* r = rccl();
  if (!r) return fail("librccl.so.1 not loadable");
  int rc = r->getUniqueId(id128);
  if (rc != 0) return fail("ncclGetUniqueId failed");
  return 0;
}

int frei_comm_init(frei_ctx* c, int nranks, int rank, const void* id128) {
  if (c && c->n_atm > 1)
    return fail("batched contexts shard atmospheres across ranks: no exchange");
  if (!c || !id128) return fail("null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail("bad rank/nranks");
  TRY(set_device(c));
  const char* force = getenv("FREI_FORCE_RCCL");
  if (nranks == 1 && !(force && force[0] == '1')) {
    c->nranks = 1;
    c->rank = 0;
    return 0;
  }
  Rccl* r = rccl();
  if (!r) return fail("librccl.so.1 not loadable");
  Id128 id;
  std::memcpy(id.b, id128, 128);
  void* comm = nullptr;
  int rc = r->commInitRank(&comm, nranks, id, rank);
  if (rc != 0)
    return fail(std::string("ncclCommInitRank: ") + (r->errStr ? r->errStr(rc) : "error"));
  c->comm = comm;
  c->nranks = nranks;
  c->rank = rank;
  TRY(c->d_Fb_all.alloc((size_t)nranks * (c->nL - 1) * 4));
  return 0;
}

int frei_comm_init_host(frei_ctx* c, int nranks, int rank, frei_allgather_fn fn, void* user) {
  if (c && c->n_atm > 1)
    return fail("batched contexts shard atmospheres across ranks: no exchange");
  if (!c || !fn) return fail("null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail("bad rank/nranks");
  TRY(set_device(c));
  const size_t n = (size_t)(c->nL - 1) * 4;
  if (c->h_ag.alloc((nranks + 1) * n)) return fail("hipHostMalloc failed");
  TRY(c->d_Fb_all.alloc((size_t)nranks * n));
  c->host_ag = fn;
  c->host_ag_user = user;
  c->nranks = nranks;
  c->rank = rank;
  return 0;
}

// ---- P2P exchange: mailbox + IPC handle, then map every rank's mailbox.
int frei_comm_p2p_handle(frei_ctx* c, int nranks, int rank, void* handle64) {
  if (c && c->n_atm > 1)
    return fail("batched contexts shard atmospheres across ranks: no exchange");
  if (!c || !handle64) return fail("null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail("bad rank/nranks");
  if (c->comm || c->host_ag || c->d_mbox) return fail("communicator already initialised");
  TRY(set_device(c));
  const int64_t n = (int64_t)(c->nL - 1) * 4;
  void* mb = nullptr;
  HIP_TRY(hipExtMallocWithFlags(&mb, mbox_bytes(nranks, n), hipDeviceMallocUncached));
  c->d_mbox.adopt(static_cast<double*>(mb), mbox_bytes(nranks, n) / sizeof(double));
  // flags 0: nothing published; complete before the handle goes to the peers
  HIP_TRY(hipMemsetAsync(c->d_mbox, 0, mbox_bytes(nranks, n), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  hipIpcMemHandle_t h;
  HIP_TRY(hipIpcGetMemHandle(&h, c->d_mbox));
  std::memcpy(handle64, &h, sizeof(h));
  c->nranks = nranks;
  c->rank = rank;
  if (const char* e = getenv("FREI_P2P_TIMEOUT_S")) c->p2p_timeout_s = atof(e);
  return 0;
}

int frei_comm_p2p_open(frei_ctx* c, const void* handles) {
  if (!c || !handles) return fail("null argument");
  if (!c->d_mbox) return fail("frei_comm_p2p_handle first");
  if (c->d_peers) return fail("P2P mailboxes already mapped");
  TRY(set_device(c));
  const int R = c->nranks;
  std::vector<double*> ptr(R, nullptr);
  for (int r = 0; r < R; ++r) {
    if (r == c->rank) {
      ptr[r] = c->d_mbox;
      continue;
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, static_cast<const char*>(handles) + (size_t)r * sizeof(h), sizeof(h));
    void* p = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    c->peer_mapped.push_back(p);
    ptr[r] = static_cast<double*>(p);
  }
  TRY(c->d_peers.alloc(R));
  TRY(h2d_wait(c->d_peers, ptr.data(), R, c->stream));
  TRY(c->d_comm_err.alloc(1));
  TRY(c->d_wait_ticks.alloc(1));
  HIP_TRY(hipMemsetAsync(c->d_comm_err, 0, sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(c->d_wait_ticks, 0, sizeof(unsigned long long), c->stream));
  TRY(c->d_Fb_all.alloc((size_t)R * (c->nL - 1) * 4));
  // handshake: every rank publishes flag 1 in every mailbox and waits for all (bounded)
  P2PPush push{};
  push.peers = c->d_peers;
  push.nranks = R;
  push.rank = c->rank;
  push.n = (int64_t)(c->nL - 1) * 4;
  push.seq = ++c->p2p_seq;
  P2PWait wait{};
  wait.mbox = c->d_mbox;
  wait.nranks = R;
  wait.n = push.n;
  wait.seq = push.seq;
  wait.timeout_ticks = (int64_t)(std::min(c->p2p_timeout_s, 20.0) * 1e8);
  wait.err = c->d_comm_err;
  launch_p2p_handshake(push, wait, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return check_comm(c);
}

// dtaus for a single context's post-processing: the caller's host array or frei_run's.
static int post_dtaus(frei_ctx* c, const double* h) {
  if (c->n_atm > 1) return fail("post-processing is per atmosphere: use a single context");
  return h ? 0 : need_device_dtaus(c, false);
}

// The post-processing calls below time their kernels into c->post_ms (frei_post_timing).
int frei_milne_pressure(frei_ctx* c, const double* dtaus, const double* p_bar,
                        double* p_milne) {
  if (!ready(c) || !p_bar || !p_milne) return fail("context not ready or null argument");
  TRY(set_device(c));
  TRY(post_dtaus(c, dtaus));
  DeviceCall call(c->stream, "milne");
  const double* u_dt = call.upload(dtaus, (size_t)c->nL * c->nlam);
  const double* d_fp = call.upload(p_bar, c->nL);
  double* d_out = call.alloc<double>(c->nlam);
  call.begin(&c->post_ms);
  if (call.ok()) launch_milne(u_dt ? u_dt : c->d_dtaus, c->nL, c->nlam, d_fp, d_out, c->stream);
  call.end();
  call.download(p_milne, d_out, c->nlam);
  return call.finish();
}

int frei_contribution(frei_ctx* c, const double* dtaus, const double* nu, const double* ratio,
                      const double* T, double hcperk, double* cf) {
  if (!ready(c) || !nu || !ratio || !T || !cf) return fail("context not ready or null argument");
  TRY(set_device(c));
  TRY(post_dtaus(c, dtaus));
  const size_t n = (size_t)c->nL * c->nlam;
  DeviceCall call(c->stream, "contribution");
  const double* u_dt = call.upload(dtaus, n);
  const double* d_nu = call.upload(nu, c->nlam);
  const double* d_ratio = call.upload(ratio, c->nL);
  const double* d_T = call.upload(T, c->nL);
  double* d_cf = call.alloc<double>(n);
  call.begin(&c->post_ms);
  if (call.ok())
    launch_contribution(u_dt ? u_dt : c->d_dtaus, c->nL, c->nlam, d_nu, d_ratio, d_T, hcperk, d_cf,
                        c->stream);
  call.end();
  call.download(cf, d_cf, n);
  return call.finish();
}

int frei_get_dtaus_batch(frei_ctx* c, int atm_lo, int n, double* out) {
  if (!ready(c) || !out) return fail("context not ready or null argument");
  if (!c->batch_api) return fail("not a batched context: frei_run returns a single context's dtaus");
  if (atm_lo < 0 || n < 0 || (int64_t)atm_lo + n > c->n_atm)
    return fail("atmosphere range outside [0, n_atm)");
  if (!c->dtaus_batch_valid || !c->d_dtaus)
    return fail("no device dtaus: run frei_run_batch_ex with keep_dtaus first");
  TRY(set_device(c));
  const size_t per = (size_t)c->nL * c->nlam;
  if (n > 0)
    HIP_TRY(hipMemcpy(out, c->d_dtaus + (size_t)atm_lo * per, (size_t)n * per * sizeof(double),
                      hipMemcpyDeviceToHost));
  return 0;
}

int frei_post_batch(frei_ctx* c, const double* dtaus, const double* spectra, const double* T,
                    const double* p_bar, const double* lam_cm, const double* nu,
                    const double* ratio, double hcperk, double* sums, double* p_milne,
                    double* cf) {
  if (!ready(c) || !p_bar || !lam_cm || !sums) return fail("context not ready or null argument");
  if (cf && (!nu || !ratio)) return fail("null nu or ratio with cf requested");
  if (!c->batch_api)
    return fail("frei_post_batch needs a context from frei_ctx_create_batch: on a single "
                "context use frei_milne_pressure / frei_contribution");
  if ((!dtaus || !spectra || (cf && !T)) && (!c->dtaus_batch_valid || !c->d_dtaus))
    return fail("no device dtaus: run frei_run_batch_ex with keep_dtaus first, or pass dtaus, "
                "spectra and T");
  TRY(set_device(c));
  const size_t A = c->n_atm, nL = c->nL, n = c->nlam, per = nL * n;
  const int nb = post_batch_blocks(c->nlam);
  DeviceCall call(c->stream, "post-processing");
  const double* u_dt = call.upload(dtaus, A * per);
  const double* u_sp = call.upload(spectra, A * n);
  const double* u_T = call.upload(cf ? T : nullptr, A * nL);
  const double* d_nu = call.upload(cf ? nu : nullptr, n);
  const double* d_ratio = call.upload(cf ? ratio : nullptr, nL);
  const double* d_fp = call.upload(p_bar, nL);
  const double* d_lam = call.upload(lam_cm, n);
  double* d_part = call.alloc<double>(A * 3 * (size_t)nb);
  double* d_sums = call.alloc<double>(A * 3);
  double* d_pm = p_milne ? call.alloc<double>(A * n) : nullptr;
  double* d_cf = cf ? call.alloc<double>(A * per) : nullptr;
  call.begin(&c->post_ms);
  if (call.ok()) {
    // the emergent row F_up[n_layers - 1] of every atmosphere, in place in the flux state
    const double* F_top = u_sp ? u_sp : c->d_Fu + (nL - 1) * n;
    const int64_t f_stride = u_sp ? (int64_t)n : (int64_t)per;
    launch_post_batch(u_dt ? u_dt : c->d_dtaus, F_top, f_stride, u_T ? u_T : c->d_T, d_fp, d_lam,
                      c->d_wtr, d_nu, d_ratio, hcperk, c->nL, c->nlam, c->n_atm, d_pm, d_cf,
                      d_part, d_sums, c->stream);
  }
  call.end();
  call.download(sums, d_sums, A * 3);
  call.download(p_milne, d_pm, A * n);
  call.download(cf, d_cf, A * per);
  return call.finish();
}

int frei_transit(frei_ctx* c, const double* dtaus, const double* radii, double r_star,
                 double* depth, double* tau_slant) {
  if (!ready(c) || !radii || !depth) return fail("context not ready or null argument");
  if (!(r_star > 0.0)) return fail("frei_transit: r_star must be > 0");
  const size_t A = c->n_atm, nL = c->nL, n = c->nlam, per = nL * n;
  for (size_t m = 0; m < A; ++m)
    for (size_t k = 0; k + 1 < nL; ++k)
      if (!(radii[m * nL + k + 1] > radii[m * nL + k]))
        return fail("frei_transit: radii must be strictly ascending (atmosphere " +
                    std::to_string(m) + ", level " + std::to_string(k + 1) + ")");
  if (!dtaus) TRY(need_device_dtaus(c, c->batch_api));
  TRY(set_device(c));
  // chord weights, once per call and atmosphere (wave-uniform in the kernel)
  const size_t nw = (size_t)transit_weight_count(c->nL);
  std::vector<double> w(A * nw);
  for (size_t m = 0; m < A; ++m) transit_build_weights(radii + m * nL, c->nL, w.data() + m * nw);
  DeviceCall call(c->stream, "transit");
  const double* u_dt = call.upload(dtaus, A * per);
  const double* d_r = call.upload(radii, A * nL);
  const double* d_w = call.upload(w.data(), A * nw);
  double* d_depth = call.alloc<double>(A * n);
  double* d_tau = tau_slant ? call.alloc<double>(A * (nL - 1) * n) : nullptr;
  call.begin(&c->post_ms);
  if (call.ok())
    launch_transit(u_dt ? u_dt : c->d_dtaus, d_r, d_w, (int64_t)nw, r_star, c->nL, c->nlam,
                   c->n_atm, d_depth, d_tau, c->stream);
  call.end();
  call.download(depth, d_depth, A * n);
  call.download(tau_slant, d_tau, A * (nL - 1) * n);
  return call.finish();
}

int frei_emergent(frei_ctx* c, const double* dtaus, const double* T, const double* mu,
                  const double* weights, int n_mu, double* intensity, double* flux) {
  if (!ready(c) || !T || !mu) return fail("context not ready or null argument");
  if (!intensity && !flux) return fail("frei_emergent: intensity and flux are both null");
  if ((weights != nullptr) != (flux != nullptr))
    return fail("frei_emergent: weights and flux must be both given or both null");
  if (n_mu < 1 || n_mu > 64) return fail("frei_emergent: n_mu must be in [1, 64]");
  const size_t A = c->n_atm, nL = c->nL, n = c->nlam, per = nL * n, K = (size_t)n_mu;
  // 1 / mu[k], c_k = weights[k] mu[k] and 1 / T_l, formed here once per call (wave-uniform in
  // the kernel); iT[m][nL] is the virtual top level's, iT[m][0] is never read
  std::vector<double> imu(K), ck(K), iT(A * (nL + 1), 0.0);
  for (size_t k = 0; k < K; ++k) {
    if (!(mu[k] > 0.0 && mu[k] <= 1.0))
      return fail("frei_emergent: mu must lie in (0, 1] (angle " + std::to_string(k) + ")");
    imu[k] = 1.0 / mu[k];
    if (weights) {
      if (!std::isfinite(weights[k]))
        return fail("frei_emergent: weights must be finite (angle " + std::to_string(k) + ")");
      ck[k] = weights[k] * mu[k];
    }
  }
  for (size_t m = 0; m < A; ++m) {
    for (size_t l = 1; l < nL; ++l) {
      const double t = T[m * nL + l];
      if (!(std::isfinite(t) && t > 0.0))
        return fail("frei_emergent: T must be finite and positive (atmosphere " +
                    std::to_string(m) + ", layer " + std::to_string(l) + ")");
      iT[m * (nL + 1) + l] = 1.0 / t;
    }
    iT[m * (nL + 1) + nL] = iT[m * (nL + 1) + nL - 1];
  }
  if (!dtaus) TRY(need_device_dtaus(c, c->batch_api));
  TRY(set_device(c));
  DeviceCall call(c->stream, "emergent");
  const double* u_dt = call.upload(dtaus, A * per);
  const double* d_iT = call.upload(iT.data(), iT.size());
  const double* d_imu = call.upload(imu.data(), K);
  const double* d_ck = call.upload(flux ? ck.data() : nullptr, K);
  double* d_int = intensity ? call.alloc<double>(A * K * n) : nullptr;
  double* d_flux = flux ? call.alloc<double>(A * n) : nullptr;
  call.begin(&c->post_ms);
  if (call.ok())
    launch_emergent(u_dt ? u_dt : c->d_dtaus, c->d_c1, c->d_hcl, d_iT, d_imu, d_ck, n_mu, c->nL,
                    c->nlam, c->n_atm, d_int, d_flux, c->stream);
  call.end();
  call.download(intensity, d_int, A * K * n);
  call.download(flux, d_flux, A * n);
  return call.finish();   // the host vectors are read by the uploads until here
}

int frei_post_timing(frei_ctx* c, double* ms) {
  if (!c || !ms) return fail("null argument");
  *ms = c->post_ms;
  return 0;
}

int frei_ctx_path(frei_ctx* c, int* flags) {
  if (!ready(c) || !flags) return fail("context not ready or null argument");
  TRY(set_device(c));
  TRY(build_meta(c));
  int nan = 0;
  for (const auto& q : c->sp) nan = nan || q.has_nan;
  // the plan run_sweep launches from, for a loop's sweeps after the first: they merge a deferred
  // update when chained launches apply
  const SweepPlan p = sweep_plan(c, true, false);
  const int tile = (c->fast && !c->eff) ? c->tile : 0;   // a chemistry batch's sweep
  *flags = (tile << 12) |
           (c->fast ? 1 : 0) | (c->fast && c->shared && tile <= 1 ? 2 : 0) | (c->eff ? 4 : 0) |
           (nan ? 8 : 0) | (p.form == kGrouped && p.Q == 2 ? 16 : 0) |
           (p.form == kGrouped && p.Q == 4 ? 32 : 0) | (p.NC << 6) |
           (p.form == kLam2 ? 512 : 0) | (p.tail_nT > 0 ? 1024 : 0) | (c->lazy_on ? 2048 : 0);
  return 0;
}

int frei_set_option(frei_ctx* c, const char* name, int value) {
  if (!c || !name) return fail("null argument");
  return set_option(c, name, value);
}

int frei_setup_timing(frei_ctx* c, double* ms) {
  if (!c || !ms) return fail("null argument");
  for (int k = 0; k < 5; ++k) ms[k] = c->setup_ms[k];
  return 0;
}

int frei_contract_timing(frei_ctx* c, double* ms, double* bytes) {
  if (!c || !ms || !bytes) return fail("null argument");
  *ms = c->contract_ms;
  *bytes = c->contract_bytes;
  return 0;
}

int frei_timing_enable(frei_ctx* c, int on) {
  if (!c) return fail("null argument");
  TRY(set_device(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->timing = on != 0;
  c->ev_used = 0;
  c->xev_used = 0;
  if (c->d_wait_ticks)
    HIP_TRY(hipMemsetAsync(c->d_wait_ticks, 0, sizeof(unsigned long long), c->stream));
  return 0;
}

int frei_timing_read(frei_ctx* c, double* total_ms, int* n_launches) {
  if (!c || !total_ms || !n_launches) return fail("null argument");
  TRY(set_device(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  double tot = 0;
  for (size_t k = 0; k + 1 < c->ev_used; k += 2) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_pool[k], c->ev_pool[k + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *n_launches = (int)(c->ev_used / 2);
  return 0;
}

int frei_timing_read_exchange(frei_ctx* c, double* total_ms, int* n_calls) {
  if (!c || !total_ms || !n_calls) return fail("null argument");
  TRY(set_device(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->d_mbox && c->d_wait_ticks) {   // P2P: time the update kernels spent waiting
    unsigned long long t = 0;
    HIP_TRY(hipMemcpy(&t, c->d_wait_ticks, sizeof(t), hipMemcpyDeviceToHost));
    *total_ms = (double)t * 1e-5;       // 100 MHz ticks
    *n_calls = (int)(c->ev_used / 2);   // one wait per timed sweep
    return 0;
  }
  double tot = 0;
  for (size_t k = 0; k + 1 < c->xev_used; k += 2) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->xev_pool[k], c->xev_pool[k + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *n_calls = (int)(c->xev_used / 2);
  return 0;
}

}  // extern "C"
