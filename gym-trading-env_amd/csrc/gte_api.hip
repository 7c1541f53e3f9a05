// gte_api.hip — host side of libgte: the C ABI declared in include/gte.h.
//
// Owns the HBM-resident datasets, per-env state and outputs, validates the
// arguments the way the reference constructor / reset do
// (environments.py:79-125,163-199) and launches the kernels of
// the other units (gte_launch.h).  No CPU path exists: without a gfx950 device every entry
// point that needs one fails with GTE_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "gte_launch.h"
#include "gte_ledger.h"
#include "gte_plan.h"

using gte::DatasetDesc;
using gte::EnvRec;
using gte::Params;
using gte_plan::LaunchPlan;
using gte_plan::SLIDE_AB_ORDER;
using gte_ledger::FLAGS;
using gte_ledger::WINDOW;
using gte_ledger::ledger;

static thread_local std::string g_err = "";

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                              \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess)                                                         \
      return fail(e_ == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP,          \
                  "%s failed: %s", #expr, hipGetErrorString(e_));                 \
  } while (0)

// a library-owned device block that only grows: grow(), below, with the leaderboard analyses' checks
struct Scratch { void* base = nullptr; size_t bytes = 0; };

struct gte_env {
  gte_config cfg;
  Params p;
  int n_cu = 0;  // compute units of cfg.device (require_device)
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<void*> allocs;       // everything freed in gte_destroy
  std::vector<DatasetDesc> h_ds;   // host copy of the descriptor table
  std::vector<void*> ds_allocs[4]; // per dataset: feat, close, high, low
  DatasetDesc* d_ds = nullptr;
  gte_outputs owned;
  // staging buffers for host-side arguments
  int32_t* d_actions = nullptr;
  uint8_t* d_mask = nullptr;
  int32_t *d_inj_idx = nullptr, *d_inj_pos = nullptr, *d_inj_ds = nullptr;
  int32_t *d_q_idx = nullptr, *d_q_pos = nullptr, *d_q_ds = nullptr;
  double* d_lo_limit_in = nullptr;  // staging for gte_add_limit_orders
  uint8_t* d_lo_persist_in = nullptr;
  bool finalized = false;
  bool was_reset = false;
  LaunchPlan plan;  // every launch choice, decided by the rules of gte_plan.h (plan_launches, finalize, rollout)
  int32_t* term_base = nullptr;  // the two-slot terminal counter in use (owned or bound)
  int term_slot = 0;       // slot the last launch added to
  // L2-affinity processing order (plan.affinity_period)
  int steps_since_rebuild = 0;
  int32_t* d_perm = nullptr;
  int32_t* d_slot_of_rank = nullptr;
  int32_t* d_bins = nullptr;
  gte::StateSoA soa = {};  // host-facing struct-of-arrays mirrors (gte_get_state)
  gte::StateSoA fsoa = {}; // the same for the terminal records (gte_get_final_state)
  gte::LogArrays log = {}; // device trajectory log (cfg.log_steps rows per env)
  // Log cursor: the row count on the device, i64 [2] (log_cursor_other, gte_device.h).  A launch
  // that appends a row when the terminal counter's slot is s reads log_cursor[s ^ 1] and writes
  // log_cursor[s]; so whenever the stream is idle log_cursor[term_slot] == log_rows, the host's
  // mirror of it (gte_get_log().rows, the host-side reads), which every host-side change of
  // term_slot keeps true (park_cursor).  Nothing enqueued depends on a row index computed here.
  int64_t* log_cursor = nullptr;
  int64_t log_rows = 0;
  int32_t* d_group_counter = nullptr; // the resident kernel's work queue (next group of envs)
  // gte_backtest: the statistics records and, in same-step mode without final_obs, terminal records
  // of its own (the terminal valuation is read from them); allocated by the first call
  gte_backtest_stats* bt_stats = nullptr;
  EnvRec* bt_final_rec = nullptr;
  // gte_backtest_curves: the window of every env that is open between the fused launch and the fold (gte_curves.hip)
  gte::CurveCarry* cv_carry = nullptr;
  // gte_track_trades: the trade records (allocated by the first call that turns tracking on), whether the
  // backtest calls maintain them, and whether that changed since the last backtest call (which then clears)
  gte_trade_stats* tr_stats = nullptr;
  bool tr_on = false, tr_changed = false;
  // gte_track_trade_list: the [N][tl_cap] list (tl_cap == 0: off; tl_alloc_cap: the capacity it was allocated
  // for) and the open_row of every env; a change sets tr_changed.  gte_read_trade_list: its device block (ids,
  // first, closed, trades) and the host copy `out` points into
  gte_trade* tl_list = nullptr;
  int32_t* tl_open_row = nullptr;
  int32_t tl_cap = 0, tl_alloc_cap = 0;
  void* tl_dev = nullptr;
  size_t tl_dev_bytes = 0;
  void* tl_host = nullptr;
  size_t tl_host_bytes = 0;
  // gte_track_periods / gte_bind_periods: the [N][pd_B] period records (pd_B == 0: tracking off; pd_alloc_B: the B
  // they were allocated for), whether tracking, B or a row changed since the last backtest call (which then
  // clears), and the period row of every dataset (base null = none bound; the base IS the library's allocation)
  // on the host and on the device
  gte_period_stats* pd_stats = nullptr;
  int32_t pd_B = 0, pd_alloc_B = 0;
  bool pd_changed = false;
  std::vector<gte::PeriodRow> h_prow;
  gte::PeriodRow* d_prow = nullptr;
  // signal tables (gte_bind_signals): one descriptor per dataset (base null = none bound), the host
  // copy and the device array the kernels read; the lookup's output for gte_backtest_signals
  std::vector<gte::SignalTable> h_sig;
  gte::SignalTable* d_sig = nullptr;
  int32_t sig_S = 0;  // strategies of every bound table (0 = none bound)
  int32_t* d_sig_actions = nullptr;
  // exit rules (gte_bind_exit_rules): the caller's rules and map (rules null = none bound) and the per-env
  // state, allocated by the first bind
  gte::ExitRules exits = {nullptr, nullptr, nullptr, 0};
  // gte_rank_strategies: the two candidate lists (gte_strategy.hip), allocated by the first call and
  // again when S outgrows them (the old ones stay until gte_destroy: launches in flight may read them)
  double* rank_score[2] = {nullptr, nullptr};
  int32_t* rank_index[2] = {nullptr, nullptr};
  int64_t rank_entries[2] = {0, 0};
  // gte_reality_check, gte_cscv, gte_diversify, gte_trade_monte_carlo: the scratch of each (gte_bootstrap.hip,
  // gte_cscv.hip, gte_diversify.hip, gte_montecarlo.hip), a block of its own that grow() keeps the same way
  Scratch boot_scratch, cscv_scratch, div_scratch, mc_scratch;
  bool timer_marked = false;  // gte_timer_stop(NULL) recorded the end event already
  // multi-GPU return exchange (gte_comm.hip): one RCCL communicator per env
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 0;
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ready = nullptr;
  hipEvent_t comm_done[4] = {nullptr, nullptr, nullptr, nullptr};  // ring: one per overlapped gather
  int64_t comm_seq = 0;                                              // overlapped gathers so far
  uint8_t* gathered_returns = nullptr;  // u8 [world, 6N], library-owned destination
  void* h_snap = nullptr;  // pinned host memory for gte_read_envs: snapshots, then observations
  size_t h_snap_bytes = 0;
  bool view_reads = false; // gte_read_envs_view has been used: the buffer is kept at full size
  void* h_logpack = nullptr;  // pinned host memory for gte_read_log_envs
  size_t h_logpack_bytes = 0;
  // sliding observation buffer (gte_bind_sliding_obs).  p.obs is its base, p.obs_rows = W + M and p.obs_head
  // the head the last launch wrote at.  Whether the next step may slide, or store its flags sparsely, is
  // for the ledger to say (gte_ledger.h)
  bool sliding = false;
};

// bytes of E's own observation buffer, whichever layout it has
static size_t own_obs_bytes(const gte_env* E) {
  return sizeof(float) * (size_t)E->p.N * (size_t)obs_env_stride(E->p);
}

// what the ledger is told (gte_ledger.h): E's own observation buffer, a buffer of N flag bytes
static gte_ledger::Span obs_span(const gte_env* E) { return {E->p.obs, own_obs_bytes(E)}; }
static gte_ledger::Span flag_span(const gte_env* E, const uint8_t* flags) { return {flags, (size_t)E->p.N}; }

template <typename T>
static int dev_alloc(gte_env* E, T** out, size_t count, bool zero = true) {
  void* ptr = nullptr;
  size_t bytes = sizeof(T) * (count ? count : 1);
  HIPCHK(hipMalloc(&ptr, bytes));
  if (getenv("GTE_DEBUG_ALLOC")) fprintf(stderr, "[gte] alloc %p %zu bytes\n", ptr, bytes);
  E->allocs.push_back(ptr);
  if (zero) HIPCHK(hipMemset(ptr, 0, bytes));
  *out = (T*)ptr;
  return GTE_OK;
}

#define TRY(expr)            \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != GTE_OK) return rc_; \
  } while (0)

// dev_alloc after create, for a buffer the env's stream uses next: the zero-fill ran on the null
// stream and the env's stream is non-blocking, so wait for it here
template <typename T>
static int dev_alloc_late(gte_env* E, T** out, size_t count) {
  TRY(dev_alloc(E, out, count));
  HIPCHK(hipDeviceSynchronize());
  return GTE_OK;
}

static int validate(const gte_config* c) {
  if (!c) return fail(GTE_ERR_INVALID, "config is NULL");
  if (c->abi_version != GTE_ABI_VERSION || c->struct_bytes != (int32_t)sizeof(gte_config))
    return fail(GTE_ERR_INVALID, "ABI mismatch: header version %d / %d bytes, library %d / %zu",
                c->abi_version, c->struct_bytes, GTE_ABI_VERSION, sizeof(gte_config));
  if (c->n_envs <= 0) return fail(GTE_ERR_INVALID, "n_envs must be > 0");
  if (c->n_datasets <= 0) return fail(GTE_ERR_INVALID, "n_datasets must be > 0");
  if (c->n_static < 0 || c->n_dyn < 0 || c->n_dyn > GTE_MAX_DYN)
    return fail(GTE_ERR_INVALID, "n_static >= 0 and 0 <= n_dyn <= %d required", GTE_MAX_DYN);
  if (c->n_static + c->n_dyn <= 0) return fail(GTE_ERR_INVALID, "observation has no columns");
  if (c->n_static + c->n_dyn > 2048) return fail(GTE_ERR_INVALID, "F_obs > 2048 unsupported");
  for (int i = 0; i < c->n_dyn; ++i)
    if (c->dyn_kind[i] != GTE_DYN_LAST_POSITION && c->dyn_kind[i] != GTE_DYN_REAL_POSITION)
      return fail(GTE_ERR_INVALID, "dyn_kind[%d] = %d unknown", i, c->dyn_kind[i]);
  if (c->window < 0) return fail(GTE_ERR_INVALID, "window must be >= 0");
  if (c->window >= 32768)  // JobRec.meta keeps the zero-row count of a window in 15 bits
    return fail(GTE_ERR_INVALID, "window must be < 32768");
  const int64_t W = c->window > 0 ? c->window : 1;
  if (W * (c->n_static + c->n_dyn) > (1 << 18))
    return fail(GTE_ERR_INVALID, "window * F_obs > 2^18 floats unsupported");
  if (c->n_positions <= 0 || c->n_positions > GTE_MAX_POSITIONS)
    return fail(GTE_ERR_INVALID, "1..%d positions required", GTE_MAX_POSITIONS);
  if (c->initial_position_index < -1 || c->initial_position_index >= c->n_positions)
    return fail(GTE_ERR_INVALID,
                "The 'initial_position' parameter must be 'random' or a position mentionned "
                "in the 'position' parameter.");  // environments.py:106
  if (c->max_episode_duration < 0 || c->max_episode_duration == 1)
    return fail(GTE_ERR_INVALID, "max_episode_duration must be 0 ('max') or >= 2");
  if (!(c->portfolio_initial_value > 0.0))
    return fail(GTE_ERR_INVALID, "portfolio_initial_value must be > 0");
  if (c->reward_kind < 0 || c->reward_kind > GTE_REWARD_CLIPPED_LOG_RETURN)
    return fail(GTE_ERR_INVALID, "reward_kind %d unknown", c->reward_kind);
  if (c->autoreset < 0 || c->autoreset > GTE_AUTORESET_SAME_STEP)
    return fail(GTE_ERR_INVALID, "autoreset %d unknown", c->autoreset);
  if (c->episodes_between_dataset_switch < 1)
    return fail(GTE_ERR_INVALID, "episodes_between_dataset_switch must be >= 1");
  if (c->nontemporal_obs < 0 || c->nontemporal_obs > 3)
    return fail(GTE_ERR_INVALID, "nontemporal_obs must be 0 (plain), 1 (nt), 2 (sc1) or 3 (automatic)");
  if (c->log_steps < 0) return fail(GTE_ERR_INVALID, "log_steps must be >= 0");
  if (c->final_obs && c->autoreset != GTE_AUTORESET_SAME_STEP)
    return fail(GTE_ERR_INVALID, "final_obs needs autoreset = same-step");
  if (c->envs_per_wave < 0 || c->envs_per_wave > 64)
    return fail(GTE_ERR_INVALID, "envs_per_wave must be 0 (automatic) or 1..64");
  if (c->obs_slack_rows < -1 || c->obs_slack_rows > 32768)
    return fail(GTE_ERR_INVALID, "obs_slack_rows must be -1 (off), 0 (automatic) or 1..32768");
  return GTE_OK;
}

// *n_cu: the device's compute units, which the launch planner sizes by
static int require_device(int device, int* n_cu) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(GTE_ERR_NO_DEVICE,
                "no HIP device available (%s): libgte has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "0 devices");
  if (device < 0 || device >= n)
    return fail(GTE_ERR_NO_DEVICE, "device %d out of range (have %d)", device, n);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(GTE_ERR_NO_DEVICE, "device %d is %s; libgte is built for gfx950 (MI355X) only",
                device, prop.gcnArchName);
  if (prop.multiProcessorCount <= 0)
    return fail(GTE_ERR_NO_DEVICE, "device %d reports no compute units", device);
  *n_cu = prop.multiProcessorCount;
  return GTE_OK;
}

static int alloc_soa(gte_env* E, gte::StateSoA* o, size_t N) {
  for (int32_t** a : {&o->idx, &o->step, &o->pos, &o->dsi, &o->start, &o->episode, &o->needs_reset})
    TRY(dev_alloc(E, a, N));
  for (double** a : {&o->asset, &o->fiat, &o->ia, &o->ifi, &o->pv, &o->realpos}) TRY(dev_alloc(E, a, N));
  return GTE_OK;
}

// gte_create's way out once the env exists: free it, keep the message of the failure
static int create_failed(gte_env* E, int rc) {
  const std::string keep = g_err;
  gte_destroy(E);
  g_err = keep;
  return rc;
}

// --- launch planning: the rules are in gte_plan.h; here are what they are given and what is done with the result

static gte_plan::Shape plan_shape(const gte_env* E) {
  const Params& p = E->p;
  const gte_config& c = E->cfg;
  gte_plan::Shape s;
  s.N = p.N; s.D = p.D; s.W = p.W; s.has_window = p.has_window != 0; s.Fobs = p.Fobs; s.nd = p.nd;
  s.persist = p.persist != 0; s.max_dur = p.max_dur; s.final_obs = c.final_obs != 0; s.log_steps = c.log_steps;
  s.envs_per_wave = c.envs_per_wave; s.nontemporal_obs = c.nontemporal_obs; s.obs_slack_rows = c.obs_slack_rows;
  s.affinity_period = c.affinity_period; s.kernel_variant = c.kernel_variant; s.debug_flags = c.debug_flags;
  return s;
}

static bool debug_geometry() { return getenv("GTE_DEBUG_GEOMETRY") != nullptr; }

// The environment switches, read at the moments include/gte.h promises (tests set them between two gte_create
// calls of one process): the slide switches and the bins at gte_create, GTE_RESIDENT_EPB at the first rollout
// that chooses a resident geometry for a store policy, GTE_DEBUG_GEOMETRY whenever a line would be printed.
enum KnobsMoment { KNOBS_CREATE, KNOBS_ROLLOUT };
static gte_plan::Knobs read_knobs(KnobsMoment when) {
  gte_plan::Knobs k;
  k.debug_geometry = debug_geometry();
  if (when == KNOBS_CREATE) {
    k.slide_full_windows = getenv("GTE_SLIDE_FULL_WINDOWS") != nullptr;
    if (const char* o = getenv("GTE_SLIDE_AB")) k.slide_ab = atoi(o);
    if (const char* o = getenv("GTE_SLIDE_STORE"))
      if (o[0] >= '0' && o[0] <= '2' && o[1] == '\0') k.slide_store = o[0] - '0';
    if (const char* o = getenv("GTE_AFFINITY_BINS")) { k.has_affinity_bins = true; k.affinity_bins = atoi(o); }
  } else if (const char* o = getenv("GTE_RESIDENT_EPB")) {
    k.has_resident_epb = true;
    k.resident_epb = atoi(o);
  }
  return k;
}

// The chip as the planner sees it: the kernels' LDS images and what the HIP runtime says of their residency.
// Every answer is asked afresh (the resident query opts its kernel into large LDS as a side effect).
// GTE_DEBUG_GEOMETRY: each question prints its arguments and its answer.
struct DeviceChip final : gte_plan::Chip {
  const gte_env* E;
  explicit DeviceChip(const gte_env* env) : E(env) { n_cu = said(env->n_cu, "n_cu device=%d", env->cfg.device); }
  template <typename T>
  static T said(T answer, const char* fmt, ...) {
    if (debug_geometry()) {
      char q[128];
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(q, sizeof q, fmt, ap);
      va_end(ap);
      fprintf(stderr, "[gte] chip: %s -> %lld\n", q, (long long)answer);
    }
    return answer;
  }
  size_t step_lds_bytes(int epw, int stage) override {
    // (no trajectory row: planning has always run before a launch sets p.log)
    return said(gte::lds_image_bytes(epw, E->p.W, E->p.nd, E->cfg.final_obs != 0, false, stage),
                "step_lds_bytes epw=%d stage=%d", epw, stage);
  }
  int hot_per_cu(int store, size_t smem) override {
    return said(store == 1 ? gte::hot_blocks_per_cu_nt(smem) : gte::hot_blocks_per_cu(smem),
                "hot_per_cu store=%d smem=%zu", store, smem);
  }
  size_t resident_lds_bytes(int epb) override {
    return said(gte::resident_lds_bytes(E->p, epb), "resident_lds_bytes epb=%d", epb);
  }
  int resident_per_cu(int epb, int store) override {
    return said(gte::resident_blocks_per_cu(E->p, epb, store), "resident_per_cu epb=%d store=%d", epb, store);
  }
  int gather_per_cu(int epw, int store) override {
    Params q = E->p;
    q.epw = epw;
    return said(gte::rollout_blocks_per_cu(q, store), "gather_per_cu epw=%d store=%d", epw, store);
  }
};

// GTE_DEBUG_GEOMETRY: the whole plan on one line, after every moment that decides some of it
static void report_plan(const gte_env* E, const char* when) {
  if (debug_geometry()) gte_plan::print_plan(stderr, when, E->plan);
}

// gte_create: plan every launch, copy what the plan decides of Params, allocate what it asks for
static int plan_launches(gte_env* E) {
  LaunchPlan& L = E->plan;
  Params& p = E->p;
  const gte_plan::Shape shape = plan_shape(E);
  DeviceChip chip(E);
  L = gte_plan::plan_create(shape, read_knobs(KNOBS_CREATE), chip);
  p.epw = L.epw; p.lean_rows = L.lean_rows; p.hot_lds = L.hot_lds; p.debug = L.debug;
  if (L.affinity_period > 0) {
    const size_t N = (size_t)p.N;
    std::vector<int32_t> slot_of_rank(N);
    gte_plan::fill_slot_of_rank(shape, L.epw, slot_of_rank.data());
    TRY(dev_alloc(E, &E->d_perm, N, false));
    TRY(dev_alloc(E, &E->d_slot_of_rank, N, false));
    TRY(dev_alloc(E, &E->d_bins, (size_t)2 * p.D * L.n_bins_per_ds));  // histogram (zero-filled) + cursors
    if (hipMemcpy(E->d_slot_of_rank, slot_of_rank.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice) !=
        hipSuccess)
      return fail(GTE_ERR_HIP, "copying slot_of_rank failed");
  }
  return GTE_OK;
}

extern "C" {

int gte_abi_version(void) { return GTE_ABI_VERSION; }

const char* gte_last_error(void) { return g_err.c_str(); }

int gte_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gte_create(const gte_config* cfg, gte_env** out) {
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  *out = nullptr;
  TRY(validate(cfg));
  int n_cu = 0;
  TRY(require_device(cfg->device, &n_cu));
  HIPCHK(hipSetDevice(cfg->device));
  gte_env* E = new (std::nothrow) gte_env();
  if (!E) return fail(GTE_ERR_OOM, "host allocation failed");
  E->cfg = *cfg;
  E->n_cu = n_cu;
  memset(&E->p, 0, sizeof(Params));
  memset(&E->owned, 0, sizeof(gte_outputs));
  Params& p = E->p;
  p.N = cfg->n_envs;
  p.D = cfg->n_datasets;
  p.Fs = cfg->n_static;
  p.nd = cfg->n_dyn;
  p.Fobs = p.Fs + p.nd;
  p.has_window = cfg->window > 0;
  p.W = p.has_window ? cfg->window : 1;
  p.P = cfg->n_positions;
  for (int i = 0; i < GTE_MAX_DYN; ++i) p.dyn_kind[i] = cfg->dyn_kind[i];
  p.init_pos_index = cfg->initial_position_index;
  p.max_dur = cfg->max_episode_duration;
  p.reward_kind = cfg->reward_kind;
  p.autoreset = cfg->autoreset;
  p.switch_every = cfg->episodes_between_dataset_switch;
  p.persist = cfg->dyn_persist ? 1 : 0;
  p.fees = cfg->trading_fees;
  p.rate = cfg->borrow_interest_rate;
  p.V0 = cfg->portfolio_initial_value;
  p.rp0 = cfg->reward_param0;
  p.rp1 = cfg->reward_param1;
  p.rp2 = cfg->reward_param2;
  p.seed = cfg->seed;
  p.env_id_base = cfg->env_id_base;

  int rc = GTE_OK;
  auto chk = [&](int r) { if (rc == GTE_OK) rc = r; };
  const size_t N = (size_t)p.N;
  chk(hipStreamCreateWithFlags(&E->own_stream, hipStreamNonBlocking) == hipSuccess
          ? GTE_OK : fail(GTE_ERR_HIP, "hipStreamCreate failed"));
  E->stream = E->own_stream;
  chk(hipEventCreate(&E->ev0) == hipSuccess && hipEventCreate(&E->ev1) == hipSuccess
          ? GTE_OK : fail(GTE_ERR_HIP, "hipEventCreate failed"));
  chk(dev_alloc(E, &p.rec, N));  // zero-filled: every counter starts at 0
  // the datasets each env has picked in its current round of D (gte_device.h, pick_dataset)
  if (p.D > 1) {
    const size_t words = N * (size_t)((p.D + 31) / 32);
    chk(words <= 0xFFFFFFFFull ? GTE_OK : fail(GTE_ERR_INVALID, "n_envs x ceil(n_datasets / 32) must be < 2^32"));
    chk(dev_alloc(E, &p.ds_used, words));
  }
  chk(alloc_soa(E, &E->soa, N));
  // (the library's own observation buffers are allocated on first use, ensure_owned_obs: a caller
  // that binds its own — the torch path — never pays for a second copy of [N, W, F_obs])
  if (cfg->final_obs) {
    chk(dev_alloc(E, &p.final_rec, N));
    chk(alloc_soa(E, &E->fsoa, N));
  }
  {  // reward f32 [N] | terminated u8 [N] | truncated u8 [N] in ONE buffer of 6N bytes: the
     // layout a sharded run all-gathers as it is (gte_allgather_returns), no packing kernel
    uint8_t* packed = nullptr;
    chk(dev_alloc(E, &packed, 6 * N + 16));
    E->owned.reward = (float*)packed;
    E->owned.terminated = packed ? packed + 4 * N : nullptr;
    E->owned.truncated = packed ? packed + 5 * N : nullptr;
  }
  chk(dev_alloc(E, &E->owned.reward64, N));
  chk(dev_alloc(E, &E->owned.term_count, 2)); chk(dev_alloc(E, &E->owned.term_ids, N));
  chk(dev_alloc(E, &E->d_actions, N)); chk(dev_alloc(E, &E->d_mask, N));
  chk(dev_alloc(E, &E->d_inj_idx, N)); chk(dev_alloc(E, &E->d_inj_pos, N));
  chk(dev_alloc(E, &E->d_inj_ds, N));
  if (cfg->log_steps > 0) {
    const size_t LN = (size_t)cfg->log_steps * N;
    chk(dev_alloc(E, &E->log.rows, LN));  // 80 B per (row, env)
    chk(dev_alloc(E, &E->log_cursor, 2));  // (hipMalloc: 256-byte aligned, as the slot pair needs)
    p.log_L = cfg->log_steps;
  }
  double* d_pos = nullptr;
  chk(dev_alloc(E, &d_pos, GTE_MAX_POSITIONS));
  chk(dev_alloc(E, &E->d_ds, (size_t)p.D));
  if (rc == GTE_OK &&
      hipMemcpy(d_pos, cfg->positions, sizeof(double) * p.P, hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(GTE_ERR_HIP, "copying positions failed");
  if (rc != GTE_OK) return create_failed(E, rc);
  p.positions = d_pos;
  p.ds = E->d_ds;
  E->owned.obs_elems_per_env = (int64_t)p.W * p.Fobs;
  // the observation buffers come later (ensure_owned_obs / gte_bind_outputs)
  p.final_obs = nullptr;
  p.obs = nullptr; p.reward = E->owned.reward; p.reward64 = E->owned.reward64;
  p.obs_rows = p.W; p.obs_head = 0; p.slide = 0;  // classic layout until gte_bind_sliding_obs
  p.terminated = E->owned.terminated; p.truncated = E->owned.truncated;
  E->term_base = E->owned.term_count; p.term_ids = E->owned.term_ids;
  E->h_ds.assign((size_t)p.D, DatasetDesc{nullptr, nullptr, nullptr, nullptr, 0});
  for (auto& v : E->ds_allocs) v.assign((size_t)p.D, nullptr);

  rc = plan_launches(E);
  if (rc != GTE_OK) return create_failed(E, rc);
  // the zero-fills above ran on the null stream; the env's stream is non-blocking
  if (hipDeviceSynchronize() != hipSuccess)
    return create_failed(E, fail(GTE_ERR_HIP, "hipDeviceSynchronize failed after allocation"));
  report_plan(E, "create");
  *out = E;
  return GTE_OK;
}

// Dataset d's signal table becomes t (base null = unbound), on the host and on the device; the
// caller has waited for the stream.  Nothing changes if the copy fails.
static int publish_signal_table(gte_env* E, int32_t d, const gte::SignalTable& t) {
  const gte::SignalTable before = E->h_sig[d];
  E->h_sig[d] = t;
  const hipError_t e = hipMemcpy(E->d_sig, E->h_sig.data(), sizeof(gte::SignalTable) * E->h_sig.size(),
                                 hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    E->h_sig[d] = before;
    return fail(GTE_ERR_HIP, "publishing the signal table of dataset %d: %s", d, hipGetErrorString(e));
  }
  bool any = false;
  for (const gte::SignalTable& x : E->h_sig) any = any || x.base != nullptr;
  if (!any) E->sig_S = 0;
  return GTE_OK;
}

// Dataset d's period row becomes r (base null = unbound), on the host and on the device, and the row it had is
// freed; the caller has waited for the stream.  Nothing changes if the copy fails.
static int publish_period_row(gte_env* E, int32_t d, const gte::PeriodRow& r) {
  const gte::PeriodRow before = E->h_prow[d];
  E->h_prow[d] = r;
  const hipError_t e = hipMemcpy(E->d_prow, E->h_prow.data(), sizeof(gte::PeriodRow) * E->h_prow.size(),
                                 hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    E->h_prow[d] = before;
    return fail(GTE_ERR_HIP, "publishing the period row of dataset %d: %s", d, hipGetErrorString(e));
  }
  if (before.base) (void)hipFree(const_cast<int8_t*>(before.base));
  // while tracking is on the next backtest call clears: its records would mix two period maps (off, nothing is
  // kept, and switching on marks the change itself: an untracked backtest keeps honouring its `clear`)
  if (E->pd_B > 0) E->pd_changed = true;
  return GTE_OK;
}

int gte_upload_dataset(gte_env* E, int32_t d, const float* feat, const double* close,
                       const double* high, const double* low, int64_t T) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  const Params& p = E->p;
  if (d < 0 || d >= p.D) return fail(GTE_ERR_INVALID, "dataset index %d out of range", d);
  if (!feat || !close) return fail(GTE_ERR_INVALID, "feat and close are required");
  if (T <= 0 || T > 0x7FFFFFF0ll) return fail(GTE_ERR_INVALID, "T out of range");
  // the conditions under which the reference's reset/step are defined (:171-177)
  const int64_t idx0 = p.has_window ? p.W - 1 : 0;
  if (T < idx0 + 2) return fail(GTE_ERR_INVALID, "dataset of %lld rows is too short for windows=%d",
                                (long long)T, p.W);
  if (p.max_dur > 0 && T - p.max_dur - idx0 <= idx0)
    return fail(GTE_ERR_INVALID, "low >= high: %lld rows cannot host episodes of %d steps",
                (long long)T, p.max_dur);
  if (E->finalized && p.persist && T > p.depth)
    return fail(GTE_ERR_STATE, "dyn_persist: cannot upload a longer dataset after the first reset");
  // After a reset envs may sit anywhere in the old table: a shorter replacement would leave
  // their next step reading rows past the new allocation.  (The reference's own _set_df is only
  // ever followed by reset(); MultiDatasetTradingEnv's drop-in builds a fresh batch per dataset.)
  if (E->was_reset && T < E->h_ds[d].T)
    return fail(GTE_ERR_STATE, "dataset %d: cannot replace %lld rows by %lld after gte_reset "
                "(running environments may be past the new end); create a new env instead",
                d, (long long)E->h_ds[d].T, (long long)T);
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));
  const void* srcs[4] = {feat, close, high, low};
  const size_t bytes[4] = {sizeof(float) * (size_t)T * p.Fobs, sizeof(double) * (size_t)T,
                           sizeof(double) * (size_t)T, sizeof(double) * (size_t)T};
  // new buffers first; the old ones stay in the descriptor table (and valid) until the new
  // table has been published, so a failure on the way leaves the env exactly as it was
  void* dev[4] = {nullptr, nullptr, nullptr, nullptr};
  auto undo = [&]() { for (void* q : dev) if (q) (void)hipFree(q); };
  for (int k = 0; k < 4; ++k) {
    if (!srcs[k]) continue;
    hipError_t e = hipMalloc(&dev[k], bytes[k]);
    if (e == hipSuccess && getenv("GTE_DEBUG_ALLOC"))
      fprintf(stderr, "[gte] dataset %d column %d at %p, %zu bytes\n", d, k, dev[k], bytes[k]);
    if (e == hipSuccess) e = hipMemcpy(dev[k], srcs[k], bytes[k], hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      undo();
      return fail(e == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP, "uploading dataset %d: %s", d,
                  hipGetErrorString(e));
    }
  }
  const DatasetDesc before = E->h_ds[d];
  E->h_ds[d] = DatasetDesc{(const float*)dev[0], (const double*)dev[1], (const double*)dev[2],
                           (const double*)dev[3], T};
  const hipError_t e = hipMemcpy(E->d_ds, E->h_ds.data(), sizeof(DatasetDesc) * p.D, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    E->h_ds[d] = before;
    undo();
    return fail(GTE_ERR_HIP, "publishing the descriptor of dataset %d: %s", d, hipGetErrorString(e));
  }
  for (int k = 0; k < 4; ++k) {
    if (E->ds_allocs[k][d]) (void)hipFree(E->ds_allocs[k][d]);
    E->ds_allocs[k][d] = dev[k];
  }
  // T may have changed: the dataset's signal table was checked against the old one
  if (E->d_sig && E->h_sig[d].base) TRY(publish_signal_table(E, d, gte::SignalTable{nullptr, 0}));
  if (E->d_prow && E->h_prow[d].base) TRY(publish_period_row(E, d, gte::PeriodRow{nullptr, 0}));  // and its period row
  return GTE_OK;
}

static int finalize(gte_env* E) {
  if (E->finalized) return GTE_OK;
  Params& p = E->p;
  int64_t maxT = 0;
  for (int d = 0; d < p.D; ++d) {
    if (E->h_ds[d].T <= 0) return fail(GTE_ERR_STATE, "dataset %d was never uploaded", d);
    if (E->h_ds[d].T > maxT) maxT = E->h_ds[d].T;
  }
  p.depth = p.persist ? maxT : p.W;
  size_t table_bytes = 0;
  for (int d = 0; d < p.D; ++d) table_bytes += (size_t)E->h_ds[d].T * p.Fobs * sizeof(float);
  gte_plan::affinity_after_upload(E->plan, plan_shape(E), table_bytes);
  TRY(dev_alloc(E, &p.ring, (size_t)p.N * p.depth * (p.nd ? p.nd : 1)));
  HIPCHK(hipDeviceSynchronize());
  report_plan(E, "finalize");
  E->finalized = true;
  return GTE_OK;
}

// injected draws come from the caller: refuse values the kernel would use as
// out-of-range row / position / dataset indices
static int check_injection(const gte_env* E, size_t count, const int32_t* idx, const int32_t* pos,
                           const int32_t* ds) {
  const Params& p = E->p;
  int64_t maxT = 0, minT = INT64_MAX;
  for (int d = 0; d < p.D; ++d) {
    if (E->h_ds[d].T > maxT) maxT = E->h_ds[d].T;
    if (E->h_ds[d].T > 0 && E->h_ds[d].T < minT) minT = E->h_ds[d].T;
  }
  const int64_t idx0 = p.has_window ? p.W - 1 : 0;
  for (size_t i = 0; i < count; ++i) {
    if (pos && pos[i] >= p.P) return fail(GTE_ERR_INVALID, "injected position index %d >= %d", pos[i], p.P);
    if (ds && ds[i] >= p.D) return fail(GTE_ERR_INVALID, "injected dataset %d >= %d", ds[i], p.D);
    if (idx && idx[i] >= 0) {
      // an env needs at least one row after its start row; its dataset is known only when
      // it is injected too, otherwise the shortest dataset bounds it
      const int64_t T = (ds && ds[i] >= 0) ? E->h_ds[ds[i]].T : minT;
      if (idx[i] < idx0 || idx[i] > T - 2)
        return fail(GTE_ERR_INVALID, "injected start row %d outside [%lld, %lld]", idx[i],
                    (long long)idx0, (long long)(T - 2));
    }
  }
  return GTE_OK;
}

// append one trajectory row per env (after a reset or a step, whose Params p were; term_slot is
// the launch's slot).  mask (a masked reset once the log has a row): no row is appended, the masked
// envs' slot of the newest row is rewritten with their reset row, and the count stays.
static int append_log(gte_env* E, const Params& p, const uint8_t* mask = nullptr) {
  if (E->cfg.log_steps <= 0) return GTE_OK;
  if (E->log_rows == 0) mask = nullptr;
  HIPCHK(gte::launch_log(p.rec, p.reward64, p.terminated, p.truncated, p.N, E->log_cursor + (E->term_slot ^ 1),
                         E->cfg.log_steps, E->log, mask, E->stream));
  if (!mask) E->log_rows += 1;
  return GTE_OK;
}

// Before the host resets term_slot: log_cursor[slot] is the slot the next appending launch will
// read, so copy the count there from the slot the last launch wrote (stream-ordered, device to
// device: the count never passes through the host).
static int park_cursor(gte_env* E, int slot) {
  if (!E->log_cursor || E->term_slot == slot) return GTE_OK;
  HIPCHK(hipMemcpyAsync(E->log_cursor + slot, E->log_cursor + E->term_slot, sizeof(int64_t),
                        hipMemcpyDeviceToDevice, E->stream));
  return GTE_OK;
}

static int stage(gte_env* E, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, E->stream));
  return GTE_OK;
}

// The library's own observation buffers, on first need: nobody bound one (gte_bind_outputs) by
// the first gte_reset / gte_get_outputs, or a binding was withdrawn.
static int ensure_owned_obs(gte_env* E) {
  Params& p = E->p;
  const size_t elems = (size_t)p.N * (size_t)p.W * (size_t)p.Fobs;
  bool fresh = false;
  if (!p.obs) {
    if (!E->owned.obs) { TRY(dev_alloc(E, &E->owned.obs, elems)); fresh = true; }
    p.obs = E->owned.obs;
  }
  if (E->cfg.final_obs && !p.final_obs) {
    if (!E->owned.final_obs) { TRY(dev_alloc(E, &E->owned.final_obs, elems)); fresh = true; }
    p.final_obs = E->owned.final_obs;
  }
  if (fresh) HIPCHK(hipDeviceSynchronize());  // zero-filled on the null stream; E->stream is non-blocking
  return GTE_OK;
}

// Re-sort the processing order (gte_kernels.hip, "L2-affinity permutation").  The histogram is
// zero between re-sorts only because the scan kernel clears it: if a launch fails part-way it may be
// left counting, and a later scatter would hand out ranks past N.  So a failure turns the re-sort off
// for good and the env goes on in identity order (results do not depend on the order).
static int resort(gte_env* E) {
  E->steps_since_rebuild = 0;
  const hipError_t e = gte::launch_affinity_rebuild(E->p, E->d_bins, E->plan.n_bins_per_ds,
                                                    E->d_slot_of_rank, E->d_perm, E->stream);
  if (e != hipSuccess) {
    E->plan.affinity_period = 0;
    E->p.perm = nullptr;
    return fail(GTE_ERR_HIP, "re-sort of the processing order: %s", hipGetErrorString(e));
  }
  E->p.perm = E->d_perm;
  return GTE_OK;
}

int gte_reset(gte_env* E, const uint8_t* mask, const int32_t* inj_idx,
              const int32_t* inj_pos_index, const int32_t* inj_dataset) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(ensure_owned_obs(E));
  TRY(finalize(E));
  TRY(check_injection(E, (size_t)E->p.N, inj_idx, inj_pos_index, inj_dataset));
  Params p = E->p;  // (a masked reset writes the masked envs' windows at the current head)
  const bool fresh_run = E->sliding && !mask;  // every window is written: a fresh run of slides from head 0
  if (fresh_run) p.obs_head = 0;
  // masked envs get zero flags, flags_out untouched: the next step stores densely.  The window claim stands
  // through a masked reset; a fresh run gives it up until the launch below has gone out (a failed reset
  // proves nothing)
  ledger().wrote(E, {obs_span(E), flag_span(E, p.terminated), flag_span(E, p.truncated)}, false,
                 fresh_run ? FLAGS | WINDOW : FLAGS);
  const size_t N = (size_t)p.N;
  p.mask = nullptr; p.inj_idx = p.inj_pos = p.inj_ds = nullptr;
  if (mask) { TRY(stage(E, E->d_mask, mask, N)); p.mask = E->d_mask; }
  if (inj_idx) { TRY(stage(E, E->d_inj_idx, inj_idx, 4 * N)); p.inj_idx = E->d_inj_idx; }
  if (inj_pos_index) { TRY(stage(E, E->d_inj_pos, inj_pos_index, 4 * N)); p.inj_pos = E->d_inj_pos; }
  if (inj_dataset) { TRY(stage(E, E->d_inj_ds, inj_dataset, 4 * N)); p.inj_ds = E->d_inj_ds; }
  HIPCHK(hipMemsetAsync(E->term_base, 0, 2 * sizeof(int32_t), E->stream));
  TRY(park_cursor(E, 1));  // the reset's log row (slot 0) reads the count from slot 1
  E->term_slot = 0;
  p.term_count = E->term_base;
  p.term_count_next = E->term_base + 1;
  const LaunchPlan& L = E->plan;
  HIPCHK(gte::launch_reset(p, L.vec, L.store, L.coop, L.stage, L.blocks, L.threads, E->stream));
  if (fresh_run) {  // the buffer holds every env's window at head 0 now
    E->p.obs_head = 0;
    ledger().establish(E, WINDOW, {obs_span(E)}, false);
  }
  TRY(append_log(E, p, p.mask));
  if (L.affinity_period > 0) TRY(resort(E));  // new start rows: re-sort the processing order
  // host staging buffers may be reused by the caller right away: pageable copies above
  // are complete on return, but keep the contract simple and explicit
  HIPCHK(hipStreamSynchronize(E->stream));
  E->was_reset = true;
  return GTE_OK;
}

int gte_set_autoreset_injection(gte_env* E, int32_t n, const int32_t* inj_idx,
                                const int32_t* inj_pos_index, const int32_t* inj_dataset) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (n < 0) return fail(GTE_ERR_INVALID, "n_episodes must be >= 0");
  for (int d = 0; d < E->p.D; ++d)
    if (E->h_ds[d].T <= 0) return fail(GTE_ERR_STATE, "upload every dataset before queueing draws");
  TRY(check_injection(E, (size_t)E->p.N * (size_t)n, inj_idx, inj_pos_index, inj_dataset));
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));
  Params& p = E->p;
  const size_t count = (size_t)p.N * (size_t)n;
  // the queues of an earlier call are released here (the stream is idle: nothing reads them)
  auto put = [&](int32_t** slot, const int32_t* src, const int32_t** param) -> int {
    *param = nullptr;
    if (*slot) { (void)hipFree(*slot); *slot = nullptr; }
    if (!src || n == 0) return GTE_OK;
    void* dev = nullptr;
    HIPCHK(hipMalloc(&dev, sizeof(int32_t) * count));
    *slot = (int32_t*)dev;  // owned by the env from here on (freed above or in gte_destroy)
    HIPCHK(hipMemcpy(dev, src, sizeof(int32_t) * count, hipMemcpyHostToDevice));
    *param = *slot;
    return GTE_OK;
  };
  TRY(put(&E->d_q_idx, inj_idx, &p.q_idx));
  TRY(put(&E->d_q_pos, inj_pos_index, &p.q_pos));
  TRY(put(&E->d_q_ds, inj_dataset, &p.q_ds));
  p.q_n = n;
  HIPCHK(gte::launch_rewind_queue(p.rec, p.N, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));
  HIPCHK(hipDeviceSynchronize());
  return GTE_OK;
}

// Stream capture (hipStreamBeginCapture by whoever owns the stream — e.g. torch.cuda.graph around
// policy + step): everything a step enqueues is capturable — the step kernel and the re-sort's
// three kernels, no memset — provided nothing comes from pageable host memory, and the host-side bookkeeping a
// replay cannot repeat stays consistent: the two-slot terminal counter alternates per launch, so
// a graph must hold an EVEN number of steps and be replayed from the slot it was captured at
// (gte_get_outputs().term_slot; StepGraph in step_graph.py checks both).  The trajectory log's
// row index comes from the device cursor (log_cursor above), so logged envs are capturable too;
// the host's mirror of it (log_rows) advances during a capture as if the steps ran: the owner of
// the capture restores it and advances it per replay (gte_get_schedule / gte_set_schedule /
// gte_advance_log).
static bool stream_capturing(gte_env* E) {
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(E->stream, &capture) != hipSuccess) { (void)hipGetLastError(); capture = hipStreamCaptureStatusNone; }
  return capture == hipStreamCaptureStatusActive;
}

// two-slot terminal counter: this launch adds to one slot (cleared by the previous
// launch or by gte_reset) and clears the other, so no memset sits between steps
static void advance_term_slot(gte_env* E, Params& p) {
  E->term_slot ^= 1;
  p.term_count = E->term_base + E->term_slot;
  p.term_count_next = E->term_base + (E->term_slot ^ 1);
}

// What one step launch reads and writes: the env's own buffers (gte_step) or one row of a
// rollout's per-step buffers.  The actions are on the device.
struct StepTargets {
  const int32_t* actions;
  float *obs, *reward;
  double* reward64;
  uint8_t *terminated, *truncated;
  bool own_obs;  // obs is the env's own buffer (its layout and its window claim apply), not a rollout's row
};

static StepTargets own_targets(const gte_env* E, const int32_t* actions) {
  return {actions, E->p.obs, E->p.reward, E->p.reward64, E->p.terminated, E->p.truncated, true};
}

// The processing order ages with every step, fused or not: re-sort once it is due
static int age_order(gte_env* E, int32_t steps) {
  if (E->plan.affinity_period > 0 && (E->steps_since_rebuild += steps) >= E->plan.affinity_period) {
    // envs drift one row per step and ~1/duration of them jump at a reset: re-sort now and
    // then (3 tiny launches, stream-ordered between two steps)
    TRY(resort(E));
  }
  return GTE_OK;
}

// The one place a step is launched (gte_step; gte_rollout and gte_backtest one launch per step), with
// store policy `store`, or the plan's slide_store where the launch stores one row per env.  terminal_rec: terminal records for this launch where the env keeps none
// (gte_backtest in same-step mode).
static int enqueue_step(gte_env* E, const StepTargets& t, int store, bool capturing,
                        EnvRec* terminal_rec = nullptr) {
  const LaunchPlan& L = E->plan;
  const bool slides_own = t.own_obs && E->sliding;
  gte_ledger::Span obs = obs_span(E);
  // slide while the buffer provably holds this env's windows (its window claim) at a head below M;
  // otherwise (and at head M: the wrap) every window in full at head 0, which makes it so again
  const bool slide = slides_own && !capturing && ledger().holds(E, WINDOW, {obs}) && E->p.obs_head < L.slide_rows;
  // A launch that stores one row per env runs in env order: the L2-affinity order exists so that the
  // full-window gathers of one XCD hit its L2, and a slide reads one 128-byte table row per env; what the
  // order costs it is the hop perm[slot] -> rec[env] at the head of phase A and 64 scattered addresses per
  // wave instruction for every per-env store (reward, ring, flags).  Results do not depend on the order
  // (resort()); term_ids has no order contract (its users sort or scatter by id: terminal_ids() sorts).
  // A re-sort that falls due in a run of such launches waits for the next launch that writes full
  // windows — the wrap, or a full step after a withdrawn claim; steps_since_rebuild keeps counting.
  const bool env_order = slide && !L.full_windows && !(L.slide_ab & SLIDE_AB_ORDER);
  if (env_order) { if (L.affinity_period > 0) E->steps_since_rebuild += 1; }
  else TRY(age_order(E, 1));
  Params p = E->p;  // (after the re-sort: it sets p.perm)
  if (env_order) p.perm = nullptr;
  if (terminal_rec) p.final_rec = terminal_rec;
  p.actions = t.actions; p.obs = t.obs; p.reward = t.reward; p.reward64 = t.reward64;
  p.terminated = t.terminated; p.truncated = t.truncated;
  if (!t.own_obs) {  // a rollout's per-step row: a classic [N, W, F_obs] block
    p.obs_rows = p.W; p.obs_head = 0;
    obs = {t.obs, sizeof(float) * (size_t)p.N * p.W * p.Fobs};
  } else if (E->sliding) {
    if (slide) {
      E->p.obs_head += 1;
      // JOB_SLIDES shares bit 1 of the job record with dyn_persist's "zero the store" (gte_device.h):
      // plan_create (gte_plan.h) never grants slide_rows with dyn_persist, and only this launch ever sets p.slide
      if (p.persist || p.final_obs)
        return fail(GTE_ERR_STATE, "internal: a sliding step with dyn_persist or final_obs (the planner grants neither)");
      p.slide = L.full_windows ? 0 : 1;
    } else {
      E->p.obs_head = 0;
    }
    p.obs_head = E->p.obs_head;
  }
  advance_term_slot(E, p);
  if (L.fused_log) {
    p.log = E->log;
    p.log_cursor = E->log_cursor + (E->term_slot ^ 1);
  }
  // terminated / truncated: only the changed ones, where the env's flag claim proves the buffers hold the
  // previous step's flags (dense inside a capture: a replay cannot rely on what ran before it)
  const gte_ledger::Span term = flag_span(E, p.terminated), trunc = flag_span(E, p.truncated);
  p.flags_sparse = !capturing && !L.always_dense && ledger().holds(E, FLAGS, {term, trunc}) ? 1 : 0;
  // what this launch writes; its own claims hold again once it has gone out
  ledger().wrote(E, {obs, term, trunc}, capturing, FLAGS | WINDOW);
  // (hot_tu_covers: the isolated instantiations have no terminal records and no trajectory row)
  const bool hot = L.hot_tu && gte::hot_tu_covers(p);
  if (p.slide) store = L.slide_store;  // one row per env: the policy of its own (gte_plan.h)
  if (hot && store == 2)
    HIPCHK(gte::launch_step_hot(p, L.blocks, L.threads, gte::lds_bytes(p, L.stage), E->stream));
  else if (hot && store == 1)
    HIPCHK(gte::launch_step_hot_nt(p, L.blocks, L.threads, gte::lds_bytes(p, L.stage), E->stream));
  else
    HIPCHK(gte::launch_step(p, L.vec, store, L.coop, L.stage, L.blocks, L.threads, E->stream));
  ledger().establish(E, FLAGS, {term, trunc}, capturing);
  if (slides_own) ledger().establish(E, WINDOW, {obs}, capturing);
  if (L.fused_log) E->log_rows += 1;
  else TRY(append_log(E, p));
  return GTE_OK;
}

int gte_step(gte_env* E, const int32_t* actions, int32_t actions_on_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_step before gte_reset");
  if (!actions) return fail(GTE_ERR_INVALID, "actions is NULL");
  const bool capturing = stream_capturing(E);
  if (capturing && !actions_on_device)
    return fail(GTE_ERR_STATE, "gte_step on a capturing stream needs device-resident actions "
                               "(a copy from pageable host memory cannot be captured)");
  if (!actions_on_device) {
    TRY(stage(E, E->d_actions, actions, sizeof(int32_t) * (size_t)E->p.N));
    actions = E->d_actions;
  }
  return enqueue_step(E, own_targets(E, actions), E->plan.store, capturing);
}

// The host schedule a stream capture advances without running anything (term_slot, log_rows,
// steps_since_rebuild): saved before a capture and put back after it, whether it succeeded or not.
int gte_get_schedule(gte_env* E, gte_schedule* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  out->log_rows = E->log_rows;
  out->term_slot = E->term_slot;
  out->steps_since_rebuild = E->steps_since_rebuild;
  return GTE_OK;
}

int gte_set_schedule(gte_env* E, const gte_schedule* s) {
  if (!E || !s) return fail(GTE_ERR_INVALID, "NULL argument");
  if ((s->term_slot != 0 && s->term_slot != 1) || s->log_rows < 0 || s->steps_since_rebuild < 0)
    return fail(GTE_ERR_INVALID, "not a schedule gte_get_schedule returned");
  E->log_rows = s->log_rows;
  E->term_slot = s->term_slot;
  E->steps_since_rebuild = s->steps_since_rebuild;
  // captured steps may have been recorded as run: the next step stores densely, full windows at head 0
  ledger().withdraw(E, FLAGS | WINDOW);
  return GTE_OK;
}

int gte_advance_log(gte_env* E, int64_t rows) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  if (rows < 0) return fail(GTE_ERR_INVALID, "rows must be >= 0");
  E->log_rows += rows;
  return GTE_OK;
}

// GTE_DEBUG_GEOMETRY: name the path each gte_rollout call takes (the tests assert it)
static void report_rollout_path(const char* path, int32_t n_steps) {
  if (debug_geometry()) fprintf(stderr, "[gte] rollout path: %s, %d steps\n", path, n_steps);
}

// gte_rollout's launches, after its checks
static int rollout(gte_env* E, const int32_t* actions, int32_t n_steps, const gte_rollout_bufs* b) {
  const size_t N = (size_t)E->p.N;
  const size_t V = (size_t)E->p.W * (size_t)E->p.Fobs;
  const LaunchPlan& L = E->plan;
  // per-step observation rows are written once and not read back by the kernels: a stream
  // (non-temporal stores where the caller left the policy automatic)
  const int nt = (b->obs && E->cfg.nontemporal_obs == 3) ? 1 : L.store;
  const bool capturing = stream_capturing(E);
  // The fused kernels write the per-step rows and advance the envs without writing the env's own observation
  // buffer: the window claim goes (a step that goes out as an ordinary launch into the own buffer below
  // establishes it again).  They store the env's own flags densely, flags_out with them, so the flag claim
  // stands for the ordinary step launches below; gte_rollout withdraws it after the copies that follow them.
  const size_t rows = (size_t)n_steps * N;
  ledger().wrote(E, {{b->obs, sizeof(float) * rows * V}, {b->terminated, rows}, {b->truncated, rows},
                     flag_span(E, E->p.terminated), flag_span(E, E->p.truncated)}, capturing, WINDOW);
  // one step as its own launch, writing row k of every per-step buffer (what the unfused path
  // does for every step, and the backtest path for its last one)
  auto step_row = [&](int32_t k) -> int {
    StepTargets t = own_targets(E, actions + (size_t)k * N);
    if (b->obs) { t.obs = b->obs + (size_t)k * N * V; t.own_obs = false; }
    if (b->reward) t.reward = b->reward + (size_t)k * N;
    if (b->reward64) t.reward64 = b->reward64 + (size_t)k * N;
    if (b->terminated) t.terminated = b->terminated + (size_t)k * N;
    if (b->truncated) t.truncated = b->truncated + (size_t)k * N;
    TRY(enqueue_step(E, t, nt, capturing));
    if (b->valuation) {
      hipError_t e = gte::launch_extract_state(E->p.rec, E->p.N, E->soa, E->stream);
      if (e == hipSuccess)
        e = hipMemcpyAsync(b->valuation + (size_t)k * N, E->soa.pv, 8 * N, hipMemcpyDeviceToDevice,
                           E->stream);
      if (e != hipSuccess) return fail(GTE_ERR_HIP, "rollout: %s", hipGetErrorString(e));
    }
    return GTE_OK;
  };
  if (!L.fused_rollout) {
    // same results, one launch per step
    report_rollout_path("per-step", n_steps);
    for (int32_t k = 0; k < n_steps; ++k) TRY(step_row(k));
  } else if (!b->obs) {
    // Backtest: no observation is kept but the last one.  n_steps - 1 steps of pure state machine
    // from registers (gte_rollout_state_kernel), then the last step as an ordinary launch, which
    // also produces the observation and the terminal list.
    report_rollout_path(n_steps > 1 ? "state-only" : "per-step", n_steps);
    if (n_steps > 1) {
      TRY(age_order(E, n_steps - 1));
      gte::RolloutArgs r = {actions, n_steps - 1, nullptr, b->reward, b->reward64, b->terminated,
                            b->truncated, b->valuation, 0, 0, nullptr};
      // identity order: with no window to gather, the L2-affinity order would only scatter the
      // per-env loads and stores (actions, rewards, flags) that are coalesced in env order
      Params ps = E->p;
      ps.perm = nullptr;
      const hipError_t le = gte::launch_rollout_state(ps, r, n_steps - 1, L.state_epw, E->stream);
      if (le != hipSuccess) return fail(GTE_ERR_HIP, "rollout launch: %s", hipGetErrorString(le));
    }
    TRY(step_row(n_steps - 1));
  } else {
    TRY(age_order(E, n_steps));
    Params p = E->p;
    if (L.resident_epb[nt] == 0) {
      DeviceChip chip(E);
      gte_plan::choose_resident_epb(E->plan, plan_shape(E), read_knobs(KNOBS_ROLLOUT), chip, nt);
      report_plan(E, "resident");
    }
    advance_term_slot(E, p);
    report_rollout_path(L.resident_epb[nt] > 0 ? "resident" : "gather", n_steps);
    if (L.resident_epb[nt] > 0) {
      // identity processing order: the L2-affinity order exists for the table reads of the
      // per-step gather; here one row per env and step is read, and consecutive envs make each
      // workgroup's observation stores one contiguous run
      p.perm = nullptr;
      if (!E->d_group_counter) TRY(dev_alloc_late(E, &E->d_group_counter, 4));
      HIPCHK(hipMemsetAsync(E->d_group_counter, 0, sizeof(int32_t), E->stream));
      const int epb = L.resident_epb[nt];
      const int n_groups = (p.N + epb - 1) / epb;
      gte::RolloutArgs r = {actions, n_steps, b->obs, b->reward, b->reward64, b->terminated,
                            b->truncated, b->valuation, epb, n_groups, E->d_group_counter};
      const int blocks = n_groups < L.resident_slots[nt] ? n_groups : L.resident_slots[nt];
      const hipError_t le = gte::launch_rollout_resident(p, r, nt, blocks, E->stream);
      if (le != hipSuccess) return fail(GTE_ERR_HIP, "rollout launch: %s", hipGetErrorString(le));
    } else {
      if (L.rollout_epw == 0) {
        DeviceChip chip(E);
        gte_plan::choose_rollout_epw(E->plan, plan_shape(E), chip, nt);
        report_plan(E, "gather");
      }
      p.epw = L.rollout_epw;
      const int r_blocks = gte::rollout_blocks(p.N, p.epw);
      gte::RolloutArgs r = {actions, n_steps, b->obs, b->reward, b->reward64, b->terminated,
                            b->truncated, b->valuation, 0, 0, nullptr};
      const hipError_t le = gte::launch_rollout(p, r, nt, r_blocks, E->stream);
      if (le != hipSuccess) return fail(GTE_ERR_HIP, "rollout launch: %s", hipGetErrorString(le));
    }
  }
  // the env's own return buffers describe the last step
  const size_t last = (size_t)(n_steps - 1) * N;
  if (b->reward) HIPCHK(hipMemcpyAsync(E->p.reward, b->reward + last, 4 * N, hipMemcpyDeviceToDevice, E->stream));
  if (b->reward64) HIPCHK(hipMemcpyAsync(E->p.reward64, b->reward64 + last, 8 * N, hipMemcpyDeviceToDevice, E->stream));
  if (b->terminated) HIPCHK(hipMemcpyAsync(E->p.terminated, b->terminated + last, N, hipMemcpyDeviceToDevice, E->stream));
  if (b->truncated) HIPCHK(hipMemcpyAsync(E->p.truncated, b->truncated + last, N, hipMemcpyDeviceToDevice, E->stream));
  return GTE_OK;
}

int gte_rollout(gte_env* E, const int32_t* actions, int32_t n_steps, const gte_rollout_bufs* b) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_rollout before gte_reset");
  if (!actions) return fail(GTE_ERR_INVALID, "actions is NULL");
  if (n_steps < 1) return fail(GTE_ERR_INVALID, "n_steps must be >= 1");
  static const gte_rollout_bufs none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (!b) b = &none;
  if (b->obs && ((uintptr_t)b->obs & 15)) return fail(GTE_ERR_INVALID, "obs must be 16-byte aligned");
  HIPCHK(hipSetDevice(E->cfg.device));
  const int rc = rollout(E, actions, n_steps, b);
  ledger().withdraw(E, FLAGS);  // (the copies into the env's own flags follow the last step's launch)
  return rc;
}

// gte_backtest's launches, after its checks: the steps of gte_rollout(actions, n_steps, NULL), each
// folded into the statistics records
// With actions == NULL (gte_backtest_signals) each step's actions are looked up in the bound signal tables
// for `strategy` instead.
// the lookup of gte_signal_actions, with the exits decided as well while rules are bound
static hipError_t launch_lookup(gte_env* E, const int32_t* strategy, int32_t* actions) {
  if (E->exits.rules)
    return gte::launch_exit_actions(E->p, E->d_sig, E->sig_S, strategy, E->exits, actions, E->stream);
  return gte::launch_signal_actions(E->p, E->d_sig, E->sig_S, strategy, actions, E->stream);
}

// With `cv` (gte_backtest_curves) the launches are those of gte_curves.hip, which write the rows as well.
static int backtest(gte_env* E, const int32_t* actions, const int32_t* strategy, int32_t n_steps, int32_t clear,
                    gte::Curves* cv = nullptr) {
  const size_t N = (size_t)E->p.N;
  const LaunchPlan& L = E->plan;
  const bool signals = actions == nullptr;
  // the summary kernels advance the envs without writing observations: the window claim goes (the ordinary
  // step launches below establish it again).  They store the env's own flags densely, so the flag claim
  // stands for those launches; backtest_entry withdraws it afterwards
  ledger().wrote(E, {flag_span(E, E->p.terminated), flag_span(E, E->p.truncated)}, false, WINDOW);
  if (signals && !E->d_sig_actions) TRY(dev_alloc_late(E, &E->d_sig_actions, N));
  if (cv) {  // the window that is open between two launches of a call (gte_curves.hip), allocated by the first such call
    if (!E->cv_carry) TRY(dev_alloc_late(E, &E->cv_carry, N));
    cv->carry = E->cv_carry;
  }
  if (!E->bt_stats) {
    if (E->p.autoreset == GTE_AUTORESET_SAME_STEP && !E->p.final_rec) TRY(dev_alloc(E, &E->bt_final_rec, N));
    TRY(dev_alloc_late(E, &E->bt_stats, N));  // (its wait covers the fill before it too)
    clear = 1;
  }
  // tracking was switched since the last call: both records start afresh, so that they cover the same transitions
  if (E->tr_changed) clear = 1;
  E->tr_changed = false;
  gte_trade_stats* const trades = E->tr_on ? E->tr_stats : nullptr;
  // ... with the trade list on, through the unit that writes it as well (gte_trade_list.hip)
  const bool listed = trades && E->tl_cap > 0;
  const gte::TradeList tl = {E->tl_list, E->tl_open_row, E->tl_cap};
  // the same for period tracking (never on together with trades: gte_track_periods, gte_track_trades)
  if (E->pd_changed) clear = 1;
  E->pd_changed = false;
  const bool periods = E->pd_B > 0;
  const gte::Periods per = {E->d_prow, E->pd_stats, E->pd_B};
  // same-step mode: the terminal valuation comes from the terminal records, the env's or our own
  EnvRec* const terminal = E->p.final_rec ? E->p.final_rec : E->bt_final_rec;
  Params ps = E->p;
  ps.perm = nullptr;  // identity order, as in the state-only rollout: per-env loads and stores coalesce
  ps.final_rec = terminal;
  hipError_t le = listed   ? gte::launch_trade_list_begin(ps, E->bt_stats, trades, tl, clear, E->stream)
                  : trades ? gte::launch_trade_begin(ps, E->bt_stats, trades, clear, E->stream)
                           : gte::launch_backtest_begin(ps, E->bt_stats, clear, E->stream);
  if (le != hipSuccess) return fail(GTE_ERR_HIP, "backtest launch: %s", hipGetErrorString(le));
  if (periods && clear)  // a cleared period record is all zero, and a reset row changes none
    HIPCHK(hipMemsetAsync(E->pd_stats, 0, sizeof(gte_period_stats) * N * (size_t)E->pd_B, E->stream));
  // one step as an ordinary launch (it also produces the observation and the terminal list), then
  // its results into the records
  auto step_and_fold = [&](int32_t k) -> int {
    if (signals) {
      const hipError_t se = launch_lookup(E, strategy, E->d_sig_actions);
      if (se != hipSuccess) return fail(GTE_ERR_HIP, "backtest launch: %s", hipGetErrorString(se));
    }
    const int32_t* const row = signals ? E->d_sig_actions : actions + (size_t)k * N;
    TRY(enqueue_step(E, own_targets(E, row), L.store, false, E->bt_final_rec));
    const hipError_t fe = cv        ? gte::launch_curve_fold(ps, E->bt_stats, *cv, k, n_steps, E->stream)
                          : listed  ? gte::launch_trade_list_fold(ps, E->bt_stats, trades, tl, E->stream)
                          : trades  ? gte::launch_trade_fold(ps, E->bt_stats, trades, E->stream)
                          : periods ? gte::launch_period_fold(ps, E->bt_stats, per, E->stream)
                                    : gte::launch_backtest_fold(ps, E->bt_stats, E->stream);
    if (fe != hipSuccess) return fail(GTE_ERR_HIP, "backtest launch: %s", hipGetErrorString(fe));
    return GTE_OK;
  };
  if (!L.fused_rollout) {
    report_rollout_path(cv ? "backtest curves per-step" : signals ? "backtest signals per-step" : "backtest per-step",
                        n_steps);
    for (int32_t k = 0; k < n_steps; ++k) TRY(step_and_fold(k));
    return GTE_OK;
  }
  if (cv) report_rollout_path(n_steps > 1 ? "backtest curves summary" : "backtest curves per-step", n_steps);
  else if (signals) report_rollout_path(n_steps > 1 ? "backtest signals summary" : "backtest signals per-step", n_steps);
  else report_rollout_path(n_steps > 1 ? "backtest summary" : "backtest per-step", n_steps);
  if (n_steps > 1) {
    TRY(age_order(E, n_steps - 1));
    // one launch, its actions from `src`; with a tracker on, the unit that keeps that record in registers as well
    const gte::SummarySource src = {actions, E->d_sig, E->sig_S, strategy, E->exits.rules ? &E->exits : nullptr};
    const int32_t k = n_steps - 1, epw = L.state_epw;
    le = cv        ? gte::launch_curve_summary(ps, src, E->bt_stats, *cv, k, epw, E->stream)
         : listed  ? gte::launch_trade_list_summary(ps, src, E->bt_stats, trades, tl, k, epw, E->stream)
         : trades  ? gte::launch_trade_summary(ps, src, E->bt_stats, trades, k, epw, E->stream)
         : periods ? gte::launch_period_summary(ps, src, E->bt_stats, per, k, epw, E->stream)
         : signals ? gte::launch_signal_summary(ps, src, E->bt_stats, k, epw, E->stream)
                   : gte::launch_backtest_summary(ps, src, E->bt_stats, k, epw, E->stream);
    if (le != hipSuccess) return fail(GTE_ERR_HIP, "backtest launch: %s", hipGetErrorString(le));
  }
  return step_and_fold(n_steps - 1);
}

// what gte_backtest and gte_backtest_signals (`who`) share once their own arguments are checked
static int backtest_entry(gte_env* E, const char* who, const int32_t* actions, const int32_t* strategy,
                          int32_t n_steps, int32_t clear, gte_backtest_stats** stats_device,
                          gte::Curves* cv = nullptr) {
  if (n_steps < 1) return fail(GTE_ERR_INVALID, "n_steps must be >= 1");
  if (stream_capturing(E))
    return fail(GTE_ERR_STATE, "%s inside a stream capture: a backtest is one launch already, run it eagerly", who);
  if (E->pd_B > 0)
    for (int d = 0; d < E->p.D; ++d)
      if (!E->d_prow || !E->h_prow[d].base)
        return fail(GTE_ERR_STATE, "%s: period tracking is on and dataset %d has no period row (gte_bind_periods)", who, d);
  HIPCHK(hipSetDevice(E->cfg.device));
  const int rc = backtest(E, actions, strategy, n_steps, clear, cv);
  ledger().withdraw(E, FLAGS);  // (as after a rollout: the next step stores densely)
  if (stats_device) *stats_device = E->bt_stats;
  return rc;
}

int gte_backtest(gte_env* E, const int32_t* actions, int32_t n_steps, int32_t clear,
                 gte_backtest_stats** stats_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_backtest before gte_reset");
  if (!actions) return fail(GTE_ERR_INVALID, "actions is NULL");
  return backtest_entry(E, "gte_backtest", actions, nullptr, n_steps, clear, stats_device);
}

// ---- a per-dataset table of rows on the device: the checks gte_bind_signals and the builders share ----
// A row holds T elements and is padded: the stride is a whole number of 16-byte pieces and at least T
// rounded up to 16 elements, so that an aligned 16-byte access anywhere in a row stays inside it.
static int64_t round_up_16(int64_t T) { return (T + 15) / 16 * 16; }

// dataset d of a builder call -> its T: a builder runs outside a capture, on a dataset that was uploaded
static int builder_dataset(gte_env* E, const char* who, int32_t d, int64_t* T) {
  if (d < 0 || d >= E->p.D) return fail(GTE_ERR_INVALID, "dataset index %d out of range", d);
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "%s inside a stream capture", who);
  *T = E->h_ds[d].T;
  if (*T <= 0) return fail(GTE_ERR_STATE, "%s: dataset %d was never uploaded", who, d);
  return GTE_OK;
}

// `stride`, in elements of `elem` bytes, of a table over the T rows of dataset d
static int check_stride(const char* name, int64_t stride, size_t elem, int64_t T, int32_t d) {
  const int64_t k = 16 / (int64_t)elem;
  if (stride % k == 0 && stride >= round_up_16(T)) return GTE_OK;
  return fail(GTE_ERR_INVALID, "%s %lld%s: a multiple of %lld and >= %lld (the %lld rows of dataset %d rounded up "
              "to 16) required", name, (long long)stride, elem == sizeof(float) ? " floats" : "", (long long)k,
              (long long)round_up_16(T), (long long)T, d);
}

// what a kernel touches of a table: T16 elements of each of its rows
struct RowSpan { const void* base; int64_t rows, stride; size_t elem; };
static bool spans_overlap(const RowSpan& r, const RowSpan& w, int64_t T16) {
  const uintptr_t r0 = (uintptr_t)r.base, w0 = (uintptr_t)w.base;
  const uintptr_t r1 = r0 + r.elem * (size_t)((r.rows - 1) * r.stride + T16);
  const uintptr_t w1 = w0 + w.elem * (size_t)((w.rows - 1) * w.stride + T16);
  return r0 < w1 && w0 < r1;
}

// ---- what the reductions, rankings and reads of the per-env record families share: each family's entry
// points run these in the order they always refused in, `who` being the entry point for the message.  The
// leaderboard analyses of the [S, B] period records (gte_reality_check, gte_cscv, gte_diversify) take from here
// as well what they share: the stats and resample checks, the walk over a period mask, the test of a list of
// output pointers, the scratch each of them keeps and the tail after their launches ----
// the head of every gte_reduce_* / gte_rank_* call and of the three analyses
static int check_strategies(const gte_env* E, int32_t n_strategies) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (n_strategies < 1) return fail(GTE_ERR_INVALID, "n_strategies must be >= 1");
  return GTE_OK;
}

static int check_n_periods(int32_t n_periods, int lo) {
  if (n_periods >= lo && n_periods <= GTE_MAX_PERIODS) return GTE_OK;
  return fail(GTE_ERR_INVALID, "n_periods %d outside [%d, %d]", n_periods, lo, GTE_MAX_PERIODS);
}

static int check_period_mask(const uint64_t* period_mask) {
  return period_mask ? GTE_OK : fail(GTE_ERR_INVALID, "period_mask is NULL");
}

// n = the periods the two words select; a bit at or above n_periods is refused (how few are too few, and the
// words for it, is the caller's)
static int count_periods(const uint64_t* period_mask, int32_t n_periods, int* n) {
  *n = 0;
  for (int b = 0; b < 128; ++b) {
    if (!((period_mask[b >> 6] >> (b & 63)) & 1)) continue;
    if (b >= n_periods) return fail(GTE_ERR_INVALID, "period_mask selects period %d, at or above n_periods %d", b, n_periods);
    ++*n;
  }
  return GTE_OK;
}

static int check_stats(const void* stats) {
  if (stats && !((uintptr_t)stats & 15)) return GTE_OK;
  return fail(GTE_ERR_INVALID, "stats_device must be a 16-byte aligned device array");
}

static int check_n_resamples(int32_t n_resamples) {
  if (n_resamples >= 1 && n_resamples <= GTE_BOOT_MAX_RESAMPLES) return GTE_OK;
  return fail(GTE_ERR_INVALID, "n_resamples %d outside [1, %d]", n_resamples, GTE_BOOT_MAX_RESAMPLES);
}

// the pools of gte_pool_trades and gte_trade_monte_carlo
static int check_n_pools(int32_t n_pools) {
  if (n_pools >= 1 && n_pools <= GTE_MC_MAX_POOLS) return GTE_OK;
  return fail(GTE_ERR_INVALID, "n_pools %d outside [1, %d]", n_pools, GTE_MC_MAX_POOLS);
}

// every pointer of the list set, and none with a bit of `low_bits` (alignment less one) in its address
static bool all_aligned(std::initializer_list<const void*> ptrs, uintptr_t low_bits) {
  uintptr_t address_bits = 0;
  for (const void* p : ptrs) {
    if (!p) return false;
    address_bits |= (uintptr_t)p;
  }
  return !(address_bits & low_bits);
}

// at least `need` bytes behind s->base: too small a block gives way to one of max(need, 2 * have) bytes (the old
// one stays until gte_destroy: launches in flight may use it)
static int grow(gte_env* E, Scratch* s, size_t need) {
  if (s->bytes >= need) return GTE_OK;
  const size_t bytes = need > 2 * s->bytes ? need : 2 * s->bytes;
  uint8_t* fresh = nullptr;
  TRY(dev_alloc(E, &fresh, bytes, false));
  s->base = fresh;
  s->bytes = bytes;
  return GTE_OK;
}

// what an analysis returns once its launches are enqueued, `what` naming it
static int launched(hipError_t e, const char* what) {
  return e == hipSuccess ? GTE_OK : fail(GTE_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
}

static int check_reduce_args(gte_env* E, const char* who, const void* records, const int32_t* group_offsets,
                             const int32_t* group_envs, const void* out) {
  if (!out || ((uintptr_t)out & 15)) return fail(GTE_ERR_INVALID, "out_device must be a 16-byte aligned device array");
  if ((uintptr_t)records & 15) return fail(GTE_ERR_INVALID, "records must be 16-byte aligned");
  if ((group_offsets == nullptr) != (group_envs == nullptr))
    return fail(GTE_ERR_INVALID, "group_offsets and group_envs: both or neither");
  if (((uintptr_t)group_offsets & 3) || ((uintptr_t)group_envs & 3))
    return fail(GTE_ERR_INVALID, "the group lists must be 4-byte aligned");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "%s inside a stream capture", who);
  return GTE_OK;
}

// metric in [lo, hi], the family's first and last
static int check_rank_args(gte_env* E, const char* who, int32_t k, int32_t metric, int lo, int hi, const void* stats,
                           const int32_t* top_index, const double* top_score, const double* scores) {
  if (k < 1 || k > GTE_RANK_MAX) return fail(GTE_ERR_INVALID, "k must lie in [1, %d]", GTE_RANK_MAX);
  if (metric < lo || metric > hi) return fail(GTE_ERR_INVALID, "metric %d unknown", metric);
  TRY(check_stats(stats));
  if (!top_index || ((uintptr_t)top_index & 3) || !top_score || ((uintptr_t)top_score & 7))
    return fail(GTE_ERR_INVALID, "top_index_device (int32 [k]) and top_score_device (f64 [k]) must be aligned device arrays");
  if ((uintptr_t)scores & 7) return fail(GTE_ERR_INVALID, "scores_device must be 8-byte aligned");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "%s inside a stream capture", who);
  return GTE_OK;
}

// rows first .. first + count - 1 of a per-env record array (`base`: row_bytes per env, or NULL before the call
// `before` made it) to the host, after everything enqueued on the env's stream
static int read_records(gte_env* E, const char* who, const char* before, const void* base, size_t row_bytes,
                        int32_t first, int32_t count, void* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!base) return fail(GTE_ERR_STATE, "%s before %s", who, before);
  if (first < 0 || count < 0 || (int64_t)first + count > E->p.N)
    return fail(GTE_ERR_INVALID, "env range [%d, %d) outside [0, %d)", first, first + count, E->p.N);
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));
  if (count > 0)
    HIPCHK(hipMemcpy(out, (const char*)base + (size_t)first * row_bytes, (size_t)count * row_bytes, hipMemcpyDeviceToHost));
  return GTE_OK;
}

int gte_bind_signals(gte_env* E, int32_t d, const int8_t* signals_device, int32_t n_strategies,
                     int64_t row_stride) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  const Params& p = E->p;
  if (d < 0 || d >= p.D) return fail(GTE_ERR_INVALID, "dataset index %d out of range", d);
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bind_signals inside a stream capture");
  if (signals_device) {
    const int64_t T = E->h_ds[d].T;
    if (T <= 0) return fail(GTE_ERR_STATE, "gte_bind_signals: dataset %d was never uploaded", d);
    if ((uintptr_t)signals_device & 15) return fail(GTE_ERR_INVALID, "signals must be 16-byte aligned");
    TRY(check_stride("row_stride", row_stride, sizeof(int8_t), T, d));
    if (n_strategies < 1) return fail(GTE_ERR_INVALID, "n_strategies must be >= 1");
    for (int o = 0; o < (int)E->h_sig.size(); ++o)
      if (o != d && E->h_sig[o].base && E->sig_S != n_strategies)
        return fail(GTE_ERR_INVALID, "n_strategies %d: the table of dataset %d has %d", n_strategies, o, E->sig_S);
  } else if (!E->d_sig) {
    return GTE_OK;  // nothing was ever bound
  }
  HIPCHK(hipSetDevice(E->cfg.device));
  if (!E->d_sig) {
    E->h_sig.assign((size_t)p.D, gte::SignalTable{nullptr, 0});
    TRY(dev_alloc(E, &E->d_sig, (size_t)p.D));
  }
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight read the descriptors
  TRY(publish_signal_table(E, d, signals_device ? gte::SignalTable{signals_device, row_stride}
                                                : gte::SignalTable{nullptr, 0}));
  if (signals_device) E->sig_S = n_strategies;
  return GTE_OK;
}

// every resident dataset has a table: the lookups may run
static int signals_ready(const gte_env* E, const char* who) {
  if (!E->was_reset) return fail(GTE_ERR_STATE, "%s before gte_reset", who);
  for (int d = 0; d < E->p.D; ++d)
    if (!E->d_sig || !E->h_sig[d].base)
      return fail(GTE_ERR_STATE, "%s: dataset %d has no signal table (gte_bind_signals)", who, d);
  return GTE_OK;
}

int gte_signal_actions(gte_env* E, const int32_t* strategy_device, int32_t* actions_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!actions_device) return fail(GTE_ERR_INVALID, "actions is NULL");
  TRY(signals_ready(E, "gte_signal_actions"));
  if (!stream_capturing(E)) HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = launch_lookup(E, strategy_device, actions_device);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "signal lookup launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_backtest_signals(gte_env* E, const int32_t* strategy_device, int32_t n_steps, int32_t clear,
                         gte_backtest_stats** stats_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  TRY(signals_ready(E, "gte_backtest_signals"));
  return backtest_entry(E, "gte_backtest_signals", nullptr, strategy_device, n_steps, clear, stats_device);
}

int gte_backtest_curves(gte_env* E, const int32_t* actions, const int32_t* strategy_device, int32_t n_steps,
                        int32_t stride, int32_t clear, const gte_curve_bufs* bufs, gte_backtest_stats** stats_device) {
  const char* const who = "gte_backtest_curves";
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "%s before gte_reset", who);
  if (!bufs) return fail(GTE_ERR_INVALID, "%s: bufs is NULL", who);
  if (n_steps < 1) return fail(GTE_ERR_INVALID, "n_steps must be >= 1");
  if (stride < 1) return fail(GTE_ERR_INVALID, "%s: stride %d must be >= 1", who, stride);
  if (!bufs->valuation && !bufs->drawdown && !bufs->reward && !bufs->position && !bufs->row && !bufs->flags)
    return fail(GTE_ERR_INVALID, "%s: all six columns are NULL, nothing to keep", who);
  if (((uintptr_t)bufs->valuation | (uintptr_t)bufs->drawdown | (uintptr_t)bufs->reward) & 7)
    return fail(GTE_ERR_INVALID, "%s: valuation, drawdown and reward must be 8-byte aligned", who);
  if (((uintptr_t)bufs->position | (uintptr_t)bufs->row) & 3)
    return fail(GTE_ERR_INVALID, "%s: position and row must be 4-byte aligned", who);
  if (E->tr_on || E->pd_B > 0)
    return fail(GTE_ERR_STATE, "%s: %s tracking is on, and a launch keeps one tracker (gte_track_%s(env, 0, ...) first)",
                who, E->tr_on ? "trade" : "period", E->tr_on ? "trades" : "periods");
  if (!actions) TRY(signals_ready(E, who));
  // (the carry is the library's: backtest() allocates it, on the env's device, and fills it in)
  gte::Curves cv = {nullptr, stride, *bufs};
  return backtest_entry(E, who, actions, actions ? nullptr : strategy_device, n_steps, clear, stats_device, &cv);
}

int gte_bind_exit_rules(gte_env* E, const gte_exit_rule* rules_device, int32_t n_rules,
                        const int32_t* rule_of_env_device, gte_exit_state** state_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bind_exit_rules inside a stream capture");
  if (rules_device) {
    if ((uintptr_t)rules_device & 3) return fail(GTE_ERR_INVALID, "exit rules must be 4-byte aligned");
    if ((uintptr_t)rule_of_env_device & 3) return fail(GTE_ERR_INVALID, "rule_of_env must be 4-byte aligned");
    if (n_rules < 1) return fail(GTE_ERR_INVALID, "n_rules must be >= 1");
  }
  HIPCHK(hipSetDevice(E->cfg.device));
  if (rules_device && !E->exits.state) TRY(dev_alloc_late(E, &E->exits.state, (size_t)E->p.N));
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight read the rules and the state
  if (E->exits.state) {
    const hipError_t e = gte::launch_exit_init(E->exits.state, E->p.N, E->stream);
    if (e != hipSuccess) return fail(GTE_ERR_HIP, "exit state launch: %s", hipGetErrorString(e));
  }
  E->exits.rules = rules_device;
  E->exits.rule_of_env = rules_device ? rule_of_env_device : nullptr;
  E->exits.n_rules = rules_device ? n_rules : 0;
  if (state_device) *state_device = E->exits.state;
  return GTE_OK;
}

int gte_read_exit_state(gte_env* E, int32_t first, int32_t count, gte_exit_state* out) {
  return read_records(E, "gte_read_exit_state", "gte_bind_exit_rules", E ? E->exits.state : nullptr,
                      sizeof(gte_exit_state), first, count, out);
}

int gte_build_signals(gte_env* E, int32_t d, const float* indicators_device, int32_t n_indicators,
                      int64_t ind_stride, const gte_signal_rule* rules_device, int32_t n_rules,
                      int8_t* table_device, int64_t row_stride) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  int64_t T;
  TRY(builder_dataset(E, "gte_build_signals", d, &T));
  if (!indicators_device || !rules_device || !table_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (((uintptr_t)indicators_device & 15) || ((uintptr_t)table_device & 15))
    return fail(GTE_ERR_INVALID, "the indicator bank and the table must be 16-byte aligned");
  if ((uintptr_t)rules_device & 3) return fail(GTE_ERR_INVALID, "rules must be 4-byte aligned");
  TRY(check_stride("row_stride", row_stride, sizeof(int8_t), T, d));
  TRY(check_stride("ind_stride", ind_stride, sizeof(float), T, d));
  if (n_indicators < 1) return fail(GTE_ERR_INVALID, "n_indicators must be >= 1");
  if (n_rules < 1) return fail(GTE_ERR_INVALID, "n_rules must be >= 1");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_build_signals(indicators_device, n_indicators, ind_stride, rules_device, n_rules,
                                                 T, table_device, row_stride, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "signal build launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_compose_signals(gte_env* E, int32_t d, const int8_t* clauses_device, int32_t n_clause_rows,
                        int64_t clause_stride, const gte_signal_compose* specs_device, int32_t n_specs,
                        int8_t* table_device, int64_t row_stride) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  int64_t T;
  TRY(builder_dataset(E, "gte_compose_signals", d, &T));
  if (!clauses_device || !specs_device || !table_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (((uintptr_t)clauses_device & 15) || ((uintptr_t)table_device & 15))
    return fail(GTE_ERR_INVALID, "the clause table and the table must be 16-byte aligned");
  if ((uintptr_t)specs_device & 3) return fail(GTE_ERR_INVALID, "specs must be 4-byte aligned");
  TRY(check_stride("row_stride", row_stride, sizeof(int8_t), T, d));
  TRY(check_stride("clause_stride", clause_stride, sizeof(int8_t), T, d));
  if (n_clause_rows < 1) return fail(GTE_ERR_INVALID, "n_clause_rows must be >= 1");
  if (n_specs < 1) return fail(GTE_ERR_INVALID, "n_specs must be >= 1");
  // what the kernel may read of the clause table and what it writes of the table: disjoint
  if (spans_overlap({clauses_device, n_clause_rows, clause_stride, sizeof(int8_t)},
                    {table_device, n_specs, row_stride, sizeof(int8_t)}, round_up_16(T)))
    return fail(GTE_ERR_INVALID, "the clause table and the table overlap");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_compose_signals(clauses_device, n_clause_rows, clause_stride, specs_device, n_specs,
                                                   T, table_device, row_stride, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "signal compose launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_build_indicators(gte_env* E, int32_t d, const gte_indicator_spec* specs_device, int32_t n_specs,
                         const float* input_device, int32_t n_inputs, int64_t input_stride, float* bank_device,
                         int64_t ind_stride) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  int64_t T;
  TRY(builder_dataset(E, "gte_build_indicators", d, &T));
  if (T > INT32_MAX - 2 * GTE_IND_MAX_WINDOW)  // (the kernel indexes rows with 32 bits, like EnvRec.idx)
    return fail(GTE_ERR_INVALID, "gte_build_indicators: dataset %d has too many rows", d);
  if (!specs_device || !bank_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (n_inputs < 0) return fail(GTE_ERR_INVALID, "n_inputs must be >= 0");
  if ((input_device != nullptr) != (n_inputs > 0))
    return fail(GTE_ERR_INVALID, "input_device must be non-NULL exactly when n_inputs > 0");
  if (((uintptr_t)bank_device & 15) || ((uintptr_t)input_device & 15))
    return fail(GTE_ERR_INVALID, "the indicator bank and the input bank must be 16-byte aligned");
  if ((uintptr_t)specs_device & 3) return fail(GTE_ERR_INVALID, "specs must be 4-byte aligned");
  TRY(check_stride("ind_stride", ind_stride, sizeof(float), T, d));
  if (n_inputs > 0) TRY(check_stride("input_stride", input_stride, sizeof(float), T, d));
  if (n_specs < 1) return fail(GTE_ERR_INVALID, "n_specs must be >= 1");
  // what the kernel reads of the input and what it writes of the bank: disjoint
  if (n_inputs > 0 && spans_overlap({input_device, n_inputs, input_stride, sizeof(float)},
                                    {bank_device, n_specs, ind_stride, sizeof(float)}, round_up_16(T)))
    return fail(GTE_ERR_INVALID, "the input bank and the indicator bank overlap");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_build_indicators(E->h_ds[d], E->p.Fobs, E->p.Fobs - E->p.nd, specs_device, n_specs,
                                                    input_device, n_inputs, input_stride, bank_device, ind_stride,
                                                    E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "indicator build launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_reduce_backtest_stats(gte_env* E, const gte_backtest_stats* records_device, int32_t n_strategies,
                              const int32_t* group_offsets_device, const int32_t* group_envs_device,
                              gte_strategy_stats* out_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_reduce_args(E, "gte_reduce_backtest_stats", records_device, group_offsets_device, group_envs_device,
                        out_device));
  const gte_backtest_stats* const records = records_device ? records_device : E->bt_stats;
  if (!records) return fail(GTE_ERR_STATE, "gte_reduce_backtest_stats before gte_backtest: the env has no records yet");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_reduce_strategies(records, E->p.N, n_strategies, E->cfg.env_id_base,
                                                     group_offsets_device, group_envs_device, out_device, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "strategy reduction launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

// the two candidate lists of the selection launches, grown to what S strategies need (gte_strategy.hip)
static int rank_scratch(gte_env* E, int32_t n_strategies) {
  for (int w = 0; w < 2; ++w) {
    const int64_t need = gte::rank_scratch_entries(n_strategies, w);
    if (E->rank_entries[w] >= need) continue;
    const int64_t entries = need > 2 * E->rank_entries[w] ? need : 2 * E->rank_entries[w];
    TRY(dev_alloc(E, &E->rank_score[w], (size_t)entries, false));
    TRY(dev_alloc(E, &E->rank_index[w], (size_t)entries, false));
    E->rank_entries[w] = entries;
  }
  return GTE_OK;
}

// how gte_rank_trade_stats and gte_rank_period_stats end: their score kernel (e: its launch) has filled
// candidate list 0, the selection launches of gte_strategy.hip follow
static int rank_select(gte_env* E, hipError_t e, const char* what, int32_t n_strategies, int32_t k, int32_t* top_index,
                       double* top_score) {
  if (e == hipSuccess)
    e = gte::launch_rank_select(n_strategies, k, top_index, top_score, E->rank_score, E->rank_index, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "%s ranking launch: %s", what, hipGetErrorString(e));
  return GTE_OK;
}

int gte_rank_strategies(gte_env* E, const gte_strategy_stats* stats_device, int32_t n_strategies, int32_t metric,
                        int64_t min_episodes, int32_t k, int32_t* top_index_device, double* top_score_device,
                        double* scores_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_rank_args(E, "gte_rank_strategies", k, metric, GTE_METRIC_MEAN_REWARD, GTE_METRIC_WORST_REWARD_SUM,
                      stats_device, top_index_device, top_score_device, scores_device));
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(rank_scratch(E, n_strategies));
  const hipError_t e = gte::launch_rank_strategies(stats_device, n_strategies, metric, min_episodes, k,
                                                   top_index_device, top_score_device, scores_device, E->rank_score,
                                                   E->rank_index, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "strategy ranking launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_reduce_trade_stats(gte_env* E, const gte_trade_stats* records_device, int32_t n_strategies,
                           const int32_t* group_offsets_device, const int32_t* group_envs_device,
                           gte_strategy_trade_stats* out_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_reduce_args(E, "gte_reduce_trade_stats", records_device, group_offsets_device, group_envs_device,
                        out_device));
  const gte_trade_stats* const records = records_device ? records_device : E->tr_stats;
  if (!records) return fail(GTE_ERR_STATE, "gte_reduce_trade_stats before gte_track_trades: the env has no trade records yet");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_reduce_trade_stats(records, E->p.N, n_strategies, E->cfg.env_id_base,
                                                      group_offsets_device, group_envs_device, out_device, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "trade reduction launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_rank_trade_stats(gte_env* E, const gte_strategy_trade_stats* stats_device, int32_t n_strategies, int32_t metric,
                         int64_t min_trades, int32_t k, int32_t* top_index_device, double* top_score_device,
                         double* scores_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_rank_args(E, "gte_rank_trade_stats", k, metric, GTE_TRADE_METRIC_WIN_RATE,
                      GTE_TRADE_METRIC_NEG_MAX_LOSS_STREAK, stats_device, top_index_device, top_score_device,
                      scores_device));
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(rank_scratch(E, n_strategies));
  const hipError_t e = gte::launch_trade_scores(stats_device, n_strategies, metric, min_trades, scores_device,
                                                E->rank_score[0], E->rank_index[0], E->stream);
  return rank_select(E, e, "trade", n_strategies, k, top_index_device, top_score_device);
}

int gte_read_backtest_stats(gte_env* E, int32_t first, int32_t count, gte_backtest_stats* out) {
  return read_records(E, "gte_read_backtest_stats", "gte_backtest", E ? E->bt_stats : nullptr,
                      sizeof(gte_backtest_stats), first, count, out);
}

// the list turned off: its memory goes back (N * capacity * 48 bytes; the env's stream is idle), open_row stays
static void drop_trade_list(gte_env* E) {
  if (E->tl_list) (void)hipFree(E->tl_list);
  E->tl_list = nullptr;
  E->tl_cap = E->tl_alloc_cap = 0;
}

int gte_track_trades(gte_env* E, int32_t on, gte_trade_stats** records_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_track_trades before gte_reset");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_track_trades inside a stream capture");
  if (on && E->pd_B > 0)
    return fail(GTE_ERR_STATE, "gte_track_trades: period tracking is on, and trade and period records together are "
                "not implemented (gte_track_periods(env, 0, ...) first)");
  HIPCHK(hipSetDevice(E->cfg.device));
  if (on && !E->tr_stats) TRY(dev_alloc_late(E, &E->tr_stats, (size_t)E->p.N));
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight write the records
  if ((on != 0) != E->tr_on) E->tr_changed = true;
  E->tr_on = on != 0;
  if (!on && E->tl_cap > 0) {  // the list goes with the tracking
    drop_trade_list(E);
    E->tr_changed = true;
  }
  if (records_device) *records_device = E->tr_stats;
  return GTE_OK;
}

int gte_track_trade_list(gte_env* E, int32_t capacity, gte_trade** list_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (capacity < 0 || capacity > GTE_MAX_TRADE_LIST)
    return fail(GTE_ERR_INVALID, "gte_track_trade_list: capacity %d outside [0, %d]", capacity, GTE_MAX_TRADE_LIST);
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_track_trade_list before gte_reset");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_track_trade_list inside a stream capture");
  if (capacity > 0 && !E->tr_on)
    return fail(GTE_ERR_STATE, "gte_track_trade_list: trade tracking is off (gte_track_trades(env, 1, ...) first)");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight write the list
  if (capacity > 0 && capacity != E->tl_alloc_cap) {
    void *fresh = nullptr, *rows = E->tl_open_row;
    hipError_t e = hipMalloc(&fresh, sizeof(gte_trade) * (size_t)E->p.N * (size_t)capacity);
    if (e == hipSuccess && !rows) {
      e = hipMalloc(&rows, sizeof(int32_t) * (size_t)E->p.N);
      if (e != hipSuccess) (void)hipFree(fresh);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(e == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP, "trade list (%d envs x %d trades): %s", E->p.N,
                  capacity, hipGetErrorString(e));
    }
    if (E->tl_list) (void)hipFree(E->tl_list);
    E->tl_list = (gte_trade*)fresh;  // (never zeroed: `closed` says what of it is valid)
    E->tl_open_row = (int32_t*)rows;  // (written by the next backtest call's clearing: tr_changed)
    E->tl_alloc_cap = capacity;
  }
  if (capacity != E->tl_cap) E->tr_changed = true;
  E->tl_cap = capacity;
  if (capacity == 0) drop_trade_list(E);
  if (list_device) *list_device = E->tl_list;
  return GTE_OK;
}

// what both gathers check first
static int trade_list_on(gte_env* E, const char* who) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (E->tl_cap < 1 || !E->tl_list || !E->tr_stats)
    return fail(GTE_ERR_STATE, "%s: the trade list is off (gte_track_trade_list)", who);
  // a switch of tracking, of the list or of its capacity since the last backtest call: `closed` still counts the
  // trades of before, and the list (fresh memory, never zeroed) holds none of them
  if (E->tr_changed)
    return fail(GTE_ERR_STATE, "%s: the trade list was switched and no backtest call has cleared the records since: "
                "it holds nothing yet", who);
  return GTE_OK;
}

static size_t round_up_16z(size_t n) { return (n + 15) & ~(size_t)15; }

int gte_read_trade_list(gte_env* E, const int32_t* env_ids, int32_t n_ids, gte_trade_batch* out) {
  TRY(trade_list_on(E, "gte_read_trade_list"));
  if (!out) return fail(GTE_ERR_INVALID, "NULL argument");
  const int N = E->p.N;
  if (!env_ids) n_ids = N;
  if (n_ids < 0) return fail(GTE_ERR_INVALID, "n_ids must be >= 0");
  for (int32_t i = 0; env_ids && i < n_ids; ++i)
    if (env_ids[i] < 0 || env_ids[i] >= N) return fail(GTE_ERR_INVALID, "env_ids[%d] = %d out of range", i, env_ids[i]);
  HIPCHK(hipSetDevice(E->cfg.device));
  // the device block: [ids i32 n -> 16] [first i64 n+1 | closed i32 n -> 16] [trades]; the host copy: from `first` on
  const size_t n = (size_t)n_ids;
  const size_t ids_bytes = round_up_16z(4 * n), head = round_up_16z(8 * (n + 1) + 4 * n);
  const gte::TradeList tl = {E->tl_list, E->tl_open_row, E->tl_cap};
  int64_t total = 0;
  char* b = nullptr;
  int64_t* first = nullptr;
  // count and scan; one read of the total; if the block cannot hold that many records it grows and is counted
  // into again; then the pack
  for (int pass = 0; pass < 2; ++pass) {
    const size_t need = ids_bytes + head + sizeof(gte_trade) * (size_t)total;
    if (pass == 1 && need <= E->tl_dev_bytes) break;
    if (need > E->tl_dev_bytes) {
      void* fresh = nullptr;
      const size_t bytes = need + need / 2;
      const hipError_t e = hipMalloc(&fresh, bytes);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP, "trade list block (%zu bytes): %s", bytes,
                    hipGetErrorString(e));
      }
      HIPCHK(hipStreamSynchronize(E->stream));  // (a gather in flight writes the old block)
      if (E->tl_dev) (void)hipFree(E->tl_dev);
      E->tl_dev = fresh;
      E->tl_dev_bytes = bytes;
    }
    b = (char*)E->tl_dev;
    first = (int64_t*)(b + ids_bytes);
    if (env_ids && n) HIPCHK(hipMemcpyAsync(b, env_ids, 4 * n, hipMemcpyHostToDevice, E->stream));
    const hipError_t le = gte::launch_trade_list_scan(E->tr_stats, tl, N, env_ids ? (const int32_t*)b : nullptr, n_ids,
                                                      first, (int32_t*)(first + n + 1), E->stream);
    if (le != hipSuccess) return fail(GTE_ERR_HIP, "trade list scan launch: %s", hipGetErrorString(le));
    if (pass == 0) {
      HIPCHK(hipMemcpyAsync(&total, first + n, 8, hipMemcpyDeviceToHost, E->stream));
      HIPCHK(hipStreamSynchronize(E->stream));
    }
  }
  if (total > 0) {
    const hipError_t le = gte::launch_trade_list_pack(tl, N, env_ids ? (const int32_t*)b : nullptr, n_ids, first,
                                                      (gte_trade*)(b + ids_bytes + head), total, E->stream);
    if (le != hipSuccess) return fail(GTE_ERR_HIP, "trade list pack launch: %s", hipGetErrorString(le));
  }
  const size_t bytes = head + sizeof(gte_trade) * (size_t)total;
  if (bytes > E->tl_host_bytes) {
    if (E->tl_host) HIPCHK(hipHostFree(E->tl_host));
    E->tl_host = nullptr; E->tl_host_bytes = 0;
    HIPCHK(hipHostMalloc(&E->tl_host, bytes + bytes / 2, hipHostMallocDefault));
    E->tl_host_bytes = bytes + bytes / 2;
  }
  HIPCHK(hipMemcpyAsync(E->tl_host, (char*)E->tl_dev + ids_bytes, bytes, hipMemcpyDeviceToHost, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));
  out->n_ids = n_ids;
  out->capacity = E->tl_cap;
  out->n_trades = total;
  out->first = (const int64_t*)E->tl_host;
  out->closed = (const int32_t*)(out->first + n + 1);
  out->trades = (const gte_trade*)((const char*)E->tl_host + head);
  return GTE_OK;
}

int gte_pack_trade_list(gte_env* E, const int32_t* env_ids_device, int32_t n_ids, int64_t* first_device,
                        int32_t* closed_device, gte_trade* trades_device, int64_t max_trades) {
  TRY(trade_list_on(E, "gte_pack_trade_list"));
  if (!env_ids_device) n_ids = E->p.N;
  if (n_ids < 0) return fail(GTE_ERR_INVALID, "n_ids must be >= 0");
  if (max_trades < 0 || (max_trades > 0 && !trades_device))
    return fail(GTE_ERR_INVALID, "trades_device (gte_trade [max_trades]) is NULL or max_trades < 0");
  if (!first_device || ((uintptr_t)first_device & 7) || (n_ids > 0 && !closed_device) ||
      ((uintptr_t)closed_device & 3) || ((uintptr_t)env_ids_device & 3))
    return fail(GTE_ERR_INVALID, "first_device (int64 [n_ids + 1]), closed_device and env_ids_device (int32 [n_ids]) "
                "must be aligned device pointers");
  if ((uintptr_t)trades_device & 15) return fail(GTE_ERR_INVALID, "trades_device must be 16-byte aligned");
  HIPCHK(hipSetDevice(E->cfg.device));
  const gte::TradeList tl = {E->tl_list, E->tl_open_row, E->tl_cap};
  hipError_t le = gte::launch_trade_list_scan(E->tr_stats, tl, E->p.N, env_ids_device, n_ids, first_device,
                                              closed_device, E->stream);
  if (le == hipSuccess && max_trades > 0 && n_ids > 0)
    le = gte::launch_trade_list_pack(tl, E->p.N, env_ids_device, n_ids, first_device, trades_device, max_trades,
                                     E->stream);
  if (le != hipSuccess) return fail(GTE_ERR_HIP, "trade list gather launch: %s", hipGetErrorString(le));
  return GTE_OK;
}

int gte_read_trade_stats(gte_env* E, int32_t first, int32_t count, gte_trade_stats* out) {
  return read_records(E, "gte_read_trade_stats", "gte_track_trades", E ? E->tr_stats : nullptr,
                      sizeof(gte_trade_stats), first, count, out);
}

int gte_bind_periods(gte_env* E, int32_t d, const int8_t* period_of_row) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  const Params& p = E->p;
  if (d < 0 || d >= p.D) return fail(GTE_ERR_INVALID, "dataset index %d out of range", d);
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bind_periods inside a stream capture");
  const int64_t T = E->h_ds[d].T;
  if (period_of_row && T <= 0) return fail(GTE_ERR_STATE, "gte_bind_periods: dataset %d was never uploaded", d);
  if (!period_of_row && !E->d_prow) return GTE_OK;  // nothing was ever bound
  HIPCHK(hipSetDevice(E->cfg.device));
  if (!E->d_prow) {
    E->h_prow.assign((size_t)p.D, gte::PeriodRow{nullptr, 0});
    TRY(dev_alloc(E, &E->d_prow, (size_t)p.D));
  }
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight read the rows
  if (!period_of_row) {
    if (E->h_prow[d].base) TRY(publish_period_row(E, d, gte::PeriodRow{nullptr, 0}));
    return GTE_OK;
  }
  const size_t T16 = (size_t)round_up_16(T);
  void* row = nullptr;
  hipError_t e = hipMalloc(&row, T16);
  if (e == hipSuccess) e = hipMemset(row, 0xFF, T16);  // the padding: -1, a row of no period
  if (e == hipSuccess) e = hipMemcpy(row, period_of_row, (size_t)T, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    if (row) (void)hipFree(row);
    return fail(e == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP, "period row of dataset %d: %s", d,
                hipGetErrorString(e));
  }
  const int rc = publish_period_row(E, d, gte::PeriodRow{(const int8_t*)row, (int32_t)T16});
  if (rc != GTE_OK) (void)hipFree(row);
  return rc;
}

int gte_track_periods(gte_env* E, int32_t n_periods, gte_period_stats** records_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  TRY(check_n_periods(n_periods, 0));
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_track_periods before gte_reset");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_track_periods inside a stream capture");
  if (n_periods > 0 && E->tr_on)
    return fail(GTE_ERR_STATE, "gte_track_periods: trade tracking is on, and trade and period records together are "
                "not implemented (gte_track_trades(env, 0, ...) first)");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight write the records
  if (n_periods > 0 && n_periods != E->pd_alloc_B) {
    void* fresh = nullptr;
    const hipError_t e = hipMalloc(&fresh, sizeof(gte_period_stats) * (size_t)E->p.N * (size_t)n_periods);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(e == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP, "period records (%d envs x %d periods): %s",
                  E->p.N, n_periods, hipGetErrorString(e));
    }
    if (E->pd_stats) (void)hipFree(E->pd_stats);
    E->pd_stats = (gte_period_stats*)fresh;  // (cleared by the next backtest call: pd_changed)
    E->pd_alloc_B = n_periods;
  }
  if (n_periods != E->pd_B) E->pd_changed = true;
  E->pd_B = n_periods;
  if (records_device) *records_device = E->pd_stats;
  return GTE_OK;
}

int gte_read_period_stats(gte_env* E, int32_t first, int32_t count, gte_period_stats* out) {
  return read_records(E, "gte_read_period_stats", "gte_track_periods", E ? E->pd_stats : nullptr,
                      E ? sizeof(gte_period_stats) * (size_t)E->pd_alloc_B : 0, first, count, out);
}

int gte_reduce_period_stats(gte_env* E, const gte_period_stats* records_device, int32_t n_periods, int32_t n_strategies,
                            const int32_t* group_offsets_device, const int32_t* group_envs_device,
                            gte_strategy_period_stats* out_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  TRY(check_reduce_args(E, "gte_reduce_period_stats", records_device, group_offsets_device, group_envs_device,
                        out_device));
  if (!records_device && !E->pd_stats)
    return fail(GTE_ERR_STATE, "gte_reduce_period_stats before gte_track_periods: the env has no period records yet");
  if (!records_device && n_periods != E->pd_alloc_B)
    return fail(GTE_ERR_INVALID, "n_periods %d: the env's records have %d", n_periods, E->pd_alloc_B);
  const gte_period_stats* const records = records_device ? records_device : E->pd_stats;
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_reduce_period_stats(records, E->p.N, n_periods, n_strategies, E->cfg.env_id_base,
                                                       group_offsets_device, group_envs_device, out_device, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "period reduction launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_rank_period_stats(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                          int32_t n_periods, const uint64_t period_mask[2], int32_t metric, int64_t min_steps, int32_t k,
                          int32_t* top_index_device, double* top_score_device, double* scores_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  TRY(check_period_mask(period_mask));
  TRY(check_rank_args(E, "gte_rank_period_stats", k, metric, GTE_PERIOD_METRIC_MEAN_REWARD,
                      GTE_PERIOD_METRIC_POSITIVE_SHARE, stats_device, top_index_device, top_score_device,
                      scores_device));
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(rank_scratch(E, n_strategies));
  const hipError_t e = gte::launch_period_scores(stats_device, n_strategies, n_periods, period_mask, metric, min_steps,
                                                 scores_device, E->rank_score[0], E->rank_index[0], E->stream);
  return rank_select(E, e, "period", n_strategies, k, top_index_device, top_score_device);
}

int gte_bootstrap_weights(gte_env* E, int32_t n, int32_t n_resamples, double block, uint64_t seed,
                          double* weights_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (n < 2 || n > GTE_MAX_PERIODS) return fail(GTE_ERR_INVALID, "n %d outside [2, %d]", n, GTE_MAX_PERIODS);
  TRY(check_n_resamples(n_resamples));
  if (!(block >= 1.0)) return fail(GTE_ERR_INVALID, "block must be >= 1.0");
  if (!weights_device || ((uintptr_t)weights_device & 7))
    return fail(GTE_ERR_INVALID, "weights_device must be an 8-byte aligned device array");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bootstrap_weights inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  double t = floor(4294967296.0 / block);
  if (t > 4294967295.0) t = 4294967295.0;
  return launched(gte::launch_bootstrap_weights(n, n_resamples, (uint32_t)t, block == 1.0 ? 1 : 0, seed,
                                                weights_device, E->stream),
                  "bootstrap weights");
}

int gte_reality_check(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                      int32_t n_periods, const uint64_t period_mask[2], const double* benchmark_device,
                      const double* weights_device, int32_t n_resamples, const gte_reality_check_out* out) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  TRY(check_n_resamples(n_resamples));
  TRY(check_period_mask(period_mask));
  int n;
  TRY(count_periods(period_mask, n_periods, &n));
  if (n < 2) return fail(GTE_ERR_INVALID, "period_mask selects %d periods: at least two are needed", n);
  TRY(check_stats(stats_device));
  if (!weights_device || ((uintptr_t)weights_device & 7) || ((uintptr_t)benchmark_device & 7))
    return fail(GTE_ERR_INVALID, "weights_device (required) and benchmark_device must be 8-byte aligned device arrays");
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  if (!all_aligned({out->mean, out->boot_sum, out->boot_sq_sum, out->max_stat, out->summary}, 7))
    return fail(GTE_ERR_INVALID, "out: mean, boot_sum, boot_sq_sum, max_stat and summary must be 8-byte aligned device pointers");
  if (!all_aligned({out->count_ge, out->count_adj, out->max_index}, 3))
    return fail(GTE_ERR_INVALID, "out: count_ge, count_adj and max_index must be 4-byte aligned device pointers");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_reality_check inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->boot_scratch, gte::reality_check_scratch_bytes(n_strategies, n, n_resamples)));
  return launched(gte::launch_reality_check(stats_device, n_strategies, n_periods, period_mask, n, benchmark_device,
                                            weights_device, n_resamples, *out, E->boot_scratch.base, E->stream),
                  "reality check");
}

int gte_cscv(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies, int32_t n_periods,
             const uint64_t* group_masks, int32_t n_groups, const uint32_t* is_groups, const uint32_t* oos_groups,
             int32_t n_splits, int32_t metric, const gte_cscv_out* out) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  if (n_groups < 2 || n_groups > GTE_CSCV_MAX_GROUPS)
    return fail(GTE_ERR_INVALID, "n_groups %d outside [2, %d]", n_groups, GTE_CSCV_MAX_GROUPS);
  if (n_splits < 1 || n_splits > GTE_CSCV_MAX_SPLITS)
    return fail(GTE_ERR_INVALID, "n_splits %d outside [1, %d]", n_splits, GTE_CSCV_MAX_SPLITS);
  if (metric != GTE_PERIOD_METRIC_MEAN_REWARD && metric != GTE_PERIOD_METRIC_SHARPE &&
      metric != GTE_PERIOD_METRIC_REWARD_SUM)
    return fail(GTE_ERR_INVALID, "metric %d: gte_cscv scores by MEAN_REWARD, SHARPE or REWARD_SUM", metric);
  TRY(check_stats(stats_device));
  if (!all_aligned({group_masks}, 7)) return fail(GTE_ERR_INVALID, "group_masks must be an 8-byte aligned host array");
  if (!all_aligned({is_groups, oos_groups}, 3))
    return fail(GTE_ERR_INVALID, "is_groups and oos_groups must be 4-byte aligned host arrays");
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  if (!all_aligned({out->is_score, out->oos_score}, 7) || !all_aligned({out->summary}, 3))
    return fail(GTE_ERR_INVALID, "out: is_score and oos_score must be 8-byte, summary 4-byte aligned device pointers");
  if (!all_aligned({out->best, out->below, out->equal, out->ranked}, 3))
    return fail(GTE_ERR_INVALID, "out: best, below, equal and ranked must be 4-byte aligned device pointers");
  uint64_t seen[2] = {0, 0};
  for (int g = 0; g < n_groups; ++g) {
    const uint64_t w0 = group_masks[2 * g], w1 = group_masks[2 * g + 1];
    if (!(w0 | w1)) return fail(GTE_ERR_INVALID, "group %d is empty", g);
    for (int b = n_periods; b < 128; ++b)
      if (((b < 64 ? w0 : w1) >> (b & 63)) & 1)
        return fail(GTE_ERR_INVALID, "group %d selects period %d, at or above n_periods %d", g, b, n_periods);
    if ((w0 & seen[0]) | (w1 & seen[1])) return fail(GTE_ERR_INVALID, "group %d shares a period with an earlier group", g);
    seen[0] |= w0;
    seen[1] |= w1;
  }
  const uint32_t all = n_groups == 32 ? 0xFFFFFFFFu : (1u << n_groups) - 1u;
  for (int c = 0; c < n_splits; ++c) {
    const uint32_t a = is_groups[c], b = oos_groups[c];
    if (!a || !b) return fail(GTE_ERR_INVALID, "split %d has an empty %s side", c, !a ? "in-sample" : "out-of-sample");
    if ((a | b) & ~all) return fail(GTE_ERR_INVALID, "split %d uses a group at or above n_groups %d", c, n_groups);
    if (a & b) return fail(GTE_ERR_INVALID, "split %d has a group on both sides", c);
  }
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_cscv inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->cscv_scratch, gte::cscv_scratch_bytes(n_strategies, n_groups, n_splits)));
  // the three tables packed as gte_launch.h lays them out, so that one copy stages them
  std::vector<uint8_t> tables(gte::cscv_table_bytes(n_groups, n_splits));
  memcpy(tables.data(), group_masks, 16 * (size_t)n_groups);
  memcpy(tables.data() + 16 * (size_t)n_groups, is_groups, 4 * (size_t)n_splits);
  memcpy(tables.data() + 16 * (size_t)n_groups + 4 * (size_t)n_splits, oos_groups, 4 * (size_t)n_splits);
  return launched(gte::launch_cscv(stats_device, n_strategies, n_periods, tables.data(), n_groups, n_splits, metric,
                                   *out, E->cscv_scratch.base, E->stream),
                  "cscv");
}

int gte_diversify(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies, int32_t n_periods,
                  const uint64_t period_mask[2], const double* scores_device, double max_corr, int32_t k,
                  const gte_diversify_out* out) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  if (k < 1 || k > GTE_RANK_MAX) return fail(GTE_ERR_INVALID, "k must lie in [1, %d]", GTE_RANK_MAX);
  TRY(check_period_mask(period_mask));
  int n;
  TRY(count_periods(period_mask, n_periods, &n));
  if (n < 3) return fail(GTE_ERR_INVALID, "period_mask selects %d periods: a correlation needs at least three", n);
  if (max_corr != max_corr) return fail(GTE_ERR_INVALID, "max_corr is NaN");
  TRY(check_stats(stats_device));
  if (!all_aligned({scores_device}, 7)) return fail(GTE_ERR_INVALID, "scores_device must be an 8-byte aligned device array");
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  if (!all_aligned({out->pick_score, out->owner_corr, out->pick_corr}, 7))
    return fail(GTE_ERR_INVALID, "out: pick_score, owner_corr and pick_corr must be 8-byte aligned device pointers");
  if (!all_aligned({out->pick, out->cluster_size, out->owner, out->summary}, 3))
    return fail(GTE_ERR_INVALID, "out: pick, cluster_size, owner and summary must be 4-byte aligned device pointers");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_diversify inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->div_scratch, gte::diversify_scratch_bytes(n_strategies, n, k)));
  return launched(gte::launch_diversify(stats_device, n_strategies, n_periods, period_mask, n, scores_device, max_corr,
                                        k, *out, E->div_scratch.base, E->stream),
                  "diversify");
}

int gte_pool_trades(gte_env* E, int32_t n_strategies, const int32_t* group_offsets_device,
                    const int32_t* group_envs_device, const int32_t* strategies_device, int32_t n_pools,
                    int64_t* first_device, int32_t* truncated_device, double* factors_device, int64_t max_factors) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_pools(n_pools));
  if ((group_offsets_device == nullptr) != (group_envs_device == nullptr))
    return fail(GTE_ERR_INVALID, "group_offsets and group_envs: both or neither");
  if (((uintptr_t)group_offsets_device & 3) || ((uintptr_t)group_envs_device & 3))
    return fail(GTE_ERR_INVALID, "the group lists must be 4-byte aligned");
  if (!all_aligned({strategies_device, truncated_device}, 3))
    return fail(GTE_ERR_INVALID, "strategies_device and truncated_device (int32 [n_pools]) must be 4-byte aligned device pointers");
  if (!all_aligned({first_device}, 7))
    return fail(GTE_ERR_INVALID, "first_device (int64 [n_pools + 1]) must be an 8-byte aligned device pointer");
  if (max_factors < 0 || (max_factors > 0 && !factors_device) || ((uintptr_t)factors_device & 7))
    return fail(GTE_ERR_INVALID, "factors_device (f64 [max_factors]) is NULL or not 8-byte aligned, or max_factors < 0");
  TRY(trade_list_on(E, "gte_pool_trades"));
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_pool_trades inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  const gte::TradeList tl = {E->tl_list, E->tl_open_row, E->tl_cap};
  hipError_t le = gte::launch_pool_count(E->tr_stats, tl, E->p.N, n_strategies, E->cfg.env_id_base,
                                         group_offsets_device, group_envs_device, strategies_device, n_pools,
                                         first_device, truncated_device, E->stream);
  if (le == hipSuccess && max_factors > 0)
    le = gte::launch_pool_pack(E->tr_stats, tl, E->p.N, n_strategies, E->cfg.env_id_base, group_offsets_device,
                               group_envs_device, strategies_device, n_pools, first_device, factors_device,
                               max_factors, E->stream);
  return launched(le, "trade pool");
}

int gte_trade_monte_carlo(gte_env* E, const double* factors_device, const int64_t* first_device,
                          const uint32_t* stream_device, int32_t n_pools, int32_t n_resamples, int32_t path_len,
                          uint64_t seed, double ruin_level, const double* dd_levels, int32_t n_levels,
                          const gte_mc_out* out) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  TRY(check_n_pools(n_pools));
  if (n_resamples < 1 || n_resamples > GTE_MC_MAX_RESAMPLES)
    return fail(GTE_ERR_INVALID, "n_resamples %d outside [1, %d]", n_resamples, GTE_MC_MAX_RESAMPLES);
  if (path_len < 0 || path_len > GTE_MC_MAX_PATH)
    return fail(GTE_ERR_INVALID, "path_len %d outside [0, %d]", path_len, GTE_MC_MAX_PATH);
  if (n_levels < 0 || n_levels > GTE_MC_MAX_LEVELS)
    return fail(GTE_ERR_INVALID, "n_levels %d outside [0, %d]", n_levels, GTE_MC_MAX_LEVELS);
  if (ruin_level != ruin_level) return fail(GTE_ERR_INVALID, "ruin_level is NaN");
  if (!all_aligned({factors_device, first_device}, 7))
    return fail(GTE_ERR_INVALID, "factors_device (f64) and first_device (int64 [n_pools + 1]) must be 8-byte aligned device pointers");
  if ((uintptr_t)stream_device & 3) return fail(GTE_ERR_INVALID, "stream_device must be 4-byte aligned");
  if (n_levels > 0 && !all_aligned({dd_levels}, 7))
    return fail(GTE_ERR_INVALID, "dd_levels must be an 8-byte aligned host array of n_levels doubles");
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  if (!all_aligned({out->pool}, 15)) return fail(GTE_ERR_INVALID, "out: pool must be a 16-byte aligned device pointer");
  if (((uintptr_t)out->final & 7) || ((uintptr_t)out->max_drawdown & 7) || ((uintptr_t)out->low & 7) ||
      ((uintptr_t)out->max_loss_streak & 3))
    return fail(GTE_ERR_INVALID, "out: final, max_drawdown and low must be 8-byte, max_loss_streak 4-byte aligned device pointers");
  if (((uintptr_t)out->dd_count & 3) || (n_levels > 0 && !out->dd_count))
    return fail(GTE_ERR_INVALID, "out: dd_count (int32 [n_pools * n_levels]) must be a 4-byte aligned device pointer");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_trade_monte_carlo inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->mc_scratch, gte::monte_carlo_scratch_bytes(n_pools, n_resamples, n_levels)));
  return launched(gte::launch_trade_monte_carlo(factors_device, first_device, stream_device, n_pools, n_resamples,
                                                path_len, seed, ruin_level, dd_levels, n_levels, *out,
                                                E->mc_scratch.base, E->stream),
                  "trade Monte Carlo");
}

int gte_add_limit_orders(gte_env* E, const int32_t* pos_index, const double* limit,
                         const uint8_t* persistent) {
  if (!E || !pos_index || !limit) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_add_limit_orders before gte_reset");
  Params& p = E->p;
  for (int d = 0; d < p.D; ++d)
    if (!E->h_ds[d].high || !E->h_ds[d].low)
      return fail(GTE_ERR_STATE, "limit orders need high/low columns in dataset %d", d);
  const size_t N = (size_t)p.N;
  for (size_t i = 0; i < N; ++i)
    if (pos_index[i] >= p.P) return fail(GTE_ERR_INVALID, "pos_index[%zu] out of range", i);
  HIPCHK(hipSetDevice(E->cfg.device));
  if (!p.lo_pos) {  // first use: allocate the order tables (the counts live in EnvRec)
    int32_t* lo_pos = nullptr;
    TRY(dev_alloc(E, &lo_pos, N * p.P));
    TRY(dev_alloc(E, &p.lo_limit, N * p.P));
    TRY(dev_alloc(E, &p.lo_persist, N * p.P));
    TRY(dev_alloc(E, &E->d_lo_limit_in, N));
    TRY(dev_alloc(E, &E->d_lo_persist_in, N));
    HIPCHK(hipDeviceSynchronize());
    p.lo_pos = lo_pos;
  }
  TRY(stage(E, E->d_inj_pos, pos_index, 4 * N));
  TRY(stage(E, E->d_lo_limit_in, limit, 8 * N));
  if (persistent) TRY(stage(E, E->d_lo_persist_in, persistent, N));
  HIPCHK(gte::launch_add_orders(p, E->d_inj_pos, E->d_lo_limit_in,
                                persistent ? E->d_lo_persist_in : nullptr, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));  // host arrays and staging buffers are free again
  return GTE_OK;
}

int gte_get_log(gte_env* E, gte_log_view* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  gte::LogRow* r = E->log.rows;  // the columns as strided views of the [L, N] rows
  out->idx = &r->idx; out->step = &r->step; out->position_index = &r->pos;
  out->dataset_index = &r->dsi; out->portfolio_valuation = &r->pv;
  out->real_position = &r->realpos; out->reward = &r->reward; out->flags = &r->flags;
  out->rows = E->log_rows; out->L = E->cfg.log_steps; out->N = E->p.N;
  out->asset = &r->asset; out->fiat = &r->fiat;
  out->interest_asset = &r->ia; out->interest_fiat = &r->ifi;
  out->env_stride = (int64_t)sizeof(gte::LogRow);
  out->row_stride = (int64_t)sizeof(gte::LogRow) * E->p.N;
  out->cursor = E->log_cursor; out->cursor_slot = E->term_slot; out->reserved0 = 0;
  return GTE_OK;
}

// rows first .. first+n-1 (mod L) of ONE env, oldest first: at most two strided 2-D copies per array
static int pull_log_column(gte_env* E, int32_t env_id, int64_t first, int32_t n, void* host,
                           size_t offset, size_t elem) {
  if (!host) return GTE_OK;
  const int N = E->p.N, L = E->cfg.log_steps;
  const size_t pitch = sizeof(gte::LogRow) * (size_t)N;  // the same env, one row later
  const char* col = (const char*)E->log.rows + offset + sizeof(gte::LogRow) * (size_t)env_id;
  const int64_t run1 = (first + n <= L) ? n : (L - first);
  HIPCHK(hipMemcpy2D(host, elem, col + (size_t)first * pitch, pitch, elem, (size_t)run1,
                     hipMemcpyDeviceToHost));
  if (run1 < n)
    HIPCHK(hipMemcpy2D((char*)host + run1 * elem, elem, col, pitch, elem, (size_t)(n - run1),
                       hipMemcpyDeviceToHost));
  return GTE_OK;
}

static int log_window(gte_env* E, int32_t env_id, int32_t* n, int32_t* n_out, int64_t* first) {
  if (!E || !n_out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  const int N = E->p.N, L = E->cfg.log_steps;
  if (env_id < 0 || env_id >= N) return fail(GTE_ERR_INVALID, "env_id out of range");
  const int64_t have = E->log_rows < L ? E->log_rows : L;
  if (*n > have) *n = (int32_t)have;
  if (*n < 0) *n = 0;
  *n_out = *n;
  *first = *n ? (E->log_rows - *n) % L : 0;
  if (*n) {
    HIPCHK(hipSetDevice(E->cfg.device));
    HIPCHK(hipStreamSynchronize(E->stream));
  }
  return GTE_OK;
}

int gte_read_log(gte_env* E, int32_t env_id, int32_t n, int32_t* idx, int32_t* step,
                 int32_t* position_index, int32_t* dataset_index, double* portfolio_valuation,
                 double* real_position, double* reward, uint8_t* flags, int32_t* n_out) {
  int64_t first = 0;
  TRY(log_window(E, env_id, &n, n_out, &first));
  if (n == 0) return GTE_OK;
  TRY(pull_log_column(E, env_id, first, n, idx, offsetof(gte::LogRow, idx), 4));
  TRY(pull_log_column(E, env_id, first, n, step, offsetof(gte::LogRow, step), 4));
  TRY(pull_log_column(E, env_id, first, n, position_index, offsetof(gte::LogRow, pos), 4));
  TRY(pull_log_column(E, env_id, first, n, dataset_index, offsetof(gte::LogRow, dsi), 4));
  TRY(pull_log_column(E, env_id, first, n, portfolio_valuation, offsetof(gte::LogRow, pv), 8));
  TRY(pull_log_column(E, env_id, first, n, real_position, offsetof(gte::LogRow, realpos), 8));
  TRY(pull_log_column(E, env_id, first, n, reward, offsetof(gte::LogRow, reward), 8));
  TRY(pull_log_column(E, env_id, first, n, flags, offsetof(gte::LogRow, flags), 1));
  return GTE_OK;
}

int gte_read_log_portfolio(gte_env* E, int32_t env_id, int32_t n, double* asset, double* fiat,
                           double* interest_asset, double* interest_fiat, int32_t* n_out) {
  int64_t first = 0;
  TRY(log_window(E, env_id, &n, n_out, &first));
  if (n == 0) return GTE_OK;
  TRY(pull_log_column(E, env_id, first, n, asset, offsetof(gte::LogRow, asset), 8));
  TRY(pull_log_column(E, env_id, first, n, fiat, offsetof(gte::LogRow, fiat), 8));
  TRY(pull_log_column(E, env_id, first, n, interest_asset, offsetof(gte::LogRow, ia), 8));
  TRY(pull_log_column(E, env_id, first, n, interest_fiat, offsetof(gte::LogRow, ifi), 8));
  return GTE_OK;
}

int gte_read_log_envs(gte_env* E, const int32_t* env_ids, int32_t n_ids, int32_t max_rows,
                      int32_t finished, gte_log_batch* out) {
  if (!E || !env_ids || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  if (n_ids < 0) return fail(GTE_ERR_INVALID, "n_ids must be >= 0");
  if (finished && !E->p.final_rec)
    return fail(GTE_ERR_STATE, "finished episodes need autoreset = same-step with final_obs");
  const int N = E->p.N, L = E->cfg.log_steps;
  if (max_rows <= 0 || max_rows > L) max_rows = L;
  for (int32_t i = 0; i < n_ids; ++i)
    if (env_ids[i] < 0 || env_ids[i] >= N) return fail(GTE_ERR_INVALID, "env_ids[%d] = %d out of range", i, env_ids[i]);
  memset(out, 0, sizeof *out);
  out->n_ids = n_ids; out->max_rows = max_rows;
  if (n_ids == 0) return GTE_OK;
  HIPCHK(hipSetDevice(E->cfg.device));
  // [ids i32 n | n_rows i32 n | pad -> 16] [7 f64 columns] [4 i32 columns] [u8 column]
  const size_t cells = (size_t)n_ids * (size_t)max_rows;
  const size_t head = (((size_t)n_ids * 8) + 15) & ~(size_t)15;
  const size_t need = head + cells * (7 * 8 + 4 * 4 + 1);
  if (need > E->h_logpack_bytes) {  // pinned and mapped: the kernel writes host memory directly
    if (E->h_logpack) HIPCHK(hipHostFree(E->h_logpack));
    E->h_logpack = nullptr; E->h_logpack_bytes = 0;
    HIPCHK(hipHostMalloc(&E->h_logpack, need + need / 2, hipHostMallocMapped));
    E->h_logpack_bytes = need + need / 2;
  }
  char* b = (char*)E->h_logpack;
  int32_t* ids = (int32_t*)b;
  memcpy(ids, env_ids, sizeof(int32_t) * (size_t)n_ids);
  gte::LogPack o;
  o.n_rows = ids + n_ids;
  double* f = (double*)(b + head);
  o.pv = f; o.realpos = f + cells; o.reward = f + 2 * cells; o.asset = f + 3 * cells;
  o.fiat = f + 4 * cells; o.ia = f + 5 * cells; o.ifi = f + 6 * cells;
  int32_t* w = (int32_t*)(f + 7 * cells);
  o.idx = w; o.step = w + cells; o.pos = w + 2 * cells; o.dsi = w + 3 * cells;
  o.flags = (uint8_t*)(w + 4 * cells);
  HIPCHK(gte::launch_pack_log(E->log, N, L, (long long)E->log_rows, ids, n_ids, max_rows, finished ? 1 : 0,
                              E->cfg.autoreset == GTE_AUTORESET_DISABLED ? 1 : 0,
                              E->p.final_rec, E->p.reward64, o, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));
  out->n_rows = o.n_rows;
  out->idx = o.idx; out->step = o.step; out->position_index = o.pos; out->dataset_index = o.dsi;
  out->portfolio_valuation = o.pv; out->real_position = o.realpos; out->reward = o.reward;
  out->asset = o.asset; out->fiat = o.fiat; out->interest_asset = o.ia; out->interest_fiat = o.ifi;
  out->flags = o.flags;
  return GTE_OK;
}

int gte_set_log_reward(gte_env* E, const double* reward_device) {
  if (!E || !reward_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  if (E->log_rows <= 0) return fail(GTE_ERR_STATE, "the log is empty");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_set_log_reward(E->log.rows, E->log_cursor + E->term_slot, E->cfg.log_steps, E->p.N,
                                    reward_device, E->stream));
  return GTE_OK;
}

int gte_apply_reward(gte_env* E, const double* reward_device, int32_t terminal_view) {
  if (!E || !reward_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  if (E->log_rows <= 0) return fail(GTE_ERR_STATE, "the log is empty");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_apply_reward(E->p, reward_device, E->log.rows, E->log_cursor + E->term_slot,
                                  terminal_view ? 1 : 0, E->stream));
  return GTE_OK;
}

int gte_get_outputs(gte_env* E, gte_outputs* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(ensure_owned_obs(E));
  const Params& p = E->p;
  out->obs = p.obs;  // (the BASE of a sliding buffer: gte_obs_view says where the window is)
  out->reward = p.reward; out->reward64 = p.reward64;
  out->terminated = p.terminated; out->truncated = p.truncated;
  out->term_count = E->term_base; out->term_ids = p.term_ids;
  out->obs_elems_per_env = (int64_t)p.W * p.Fobs;
  out->term_slot = E->term_slot;
  out->reserved0 = 0;
  out->final_obs = p.final_obs;
  return GTE_OK;
}

int gte_bind_outputs(gte_env* E, const gte_outputs* b) {
  if (!E || !b) return fail(GTE_ERR_INVALID, "NULL argument");
  HIPCHK(hipStreamSynchronize(E->stream));
  Params& p = E->p;
  if (b->obs && ((uintptr_t)b->obs & 15)) return fail(GTE_ERR_INVALID, "obs must be 16-byte aligned");
  E->sliding = false;  // back to the classic layout, whatever was bound
  p.obs_rows = p.W; p.obs_head = 0;
  p.obs = b->obs;  // NULL: back to the library's own buffers (allocated on first need)
  ledger().wrote(E, {obs_span(E)}, false, FLAGS | WINDOW);  // (other envs that slide in that buffer stop)
  if (E->cfg.final_obs) p.final_obs = b->final_obs;
  if (E->was_reset) TRY(ensure_owned_obs(E));
  p.reward = b->reward ? b->reward : E->owned.reward;
  p.reward64 = b->reward64 ? b->reward64 : E->owned.reward64;
  p.terminated = b->terminated ? b->terminated : E->owned.terminated;
  p.truncated = b->truncated ? b->truncated : E->owned.truncated;
  E->term_base = b->term_count ? b->term_count : E->owned.term_count;  // i32 [2]
  HIPCHK(hipMemset(E->term_base, 0, 2 * sizeof(int32_t)));
  TRY(park_cursor(E, 0));  // the next step (slot 1) reads the log's count from slot 0
  HIPCHK(hipDeviceSynchronize());
  E->term_slot = 0;
  p.term_ids = b->term_ids ? b->term_ids : E->owned.term_ids;
  return GTE_OK;
}

int gte_obs_view(gte_env* E, gte_obs_view_t* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  out->base = E->p.obs;
  out->rows_per_env = E->p.obs_rows;
  out->head = E->p.obs_head;
  out->sliding = E->sliding ? 1 : 0;
  out->slack_rows = E->plan.slide_rows;
  return GTE_OK;
}

int gte_bind_sliding_obs(gte_env* E, float* base, int32_t rows_per_env) {
  if (!E || !base) return fail(GTE_ERR_INVALID, "NULL argument");
  const LaunchPlan& L = E->plan;
  if (L.slide_rows <= 0)
    return fail(GTE_ERR_STATE, "this env does not slide (gte_obs_view().slack_rows is 0): bind a classic buffer");
  Params& p = E->p;
  if (rows_per_env != p.W + L.slide_rows)
    return fail(GTE_ERR_INVALID, "rows_per_env must be window + slack_rows = %d", p.W + L.slide_rows);
  if ((uintptr_t)base & 15) return fail(GTE_ERR_INVALID, "obs must be 16-byte aligned");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bind_sliding_obs inside a stream capture");
  HIPCHK(hipStreamSynchronize(E->stream));
  p.obs = base;
  p.obs_rows = rows_per_env;
  p.obs_head = 0;
  E->sliding = true;
  // the next step writes every window in full at head 0 (and other envs that slide in that buffer stop)
  ledger().wrote(E, {obs_span(E)}, false, WINDOW);
  return GTE_OK;
}

static_assert(sizeof(gte_env_snapshot) == 96, "gte_env_snapshot layout");

static int read_envs_impl(gte_env* E, int32_t first, int32_t count, int32_t want_obs,
                          const gte_env_snapshot** out, const float** obs, bool hands_out_views) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_read_envs before gte_reset");
  if (first < 0 || count < 1 || (int64_t)first + count > E->p.N)
    return fail(GTE_ERR_INVALID, "envs %d..%lld out of range", first, (long long)first + count - 1);
  if (want_obs && !obs) return fail(GTE_ERR_INVALID, "obs is NULL");
  HIPCHK(hipSetDevice(E->cfg.device));
  const size_t elems = (size_t)E->p.W * (size_t)E->p.Fobs;
  const size_t head = sizeof(gte_env_snapshot) * (size_t)count;  // 96 B each: 16-byte aligned
  const size_t need = head + (want_obs ? sizeof(float) * elems * (size_t)count : 0);
  // Callers may hold views into the staging buffer: once it exists at full size it is never
  // reallocated, so size it for the whole batch the first time a buffer is made.
  const size_t full = (sizeof(gte_env_snapshot) + sizeof(float) * elems) * (size_t)E->p.N;
  if (hands_out_views) E->view_reads = true;
  const size_t want = E->view_reads ? full : need;
  if (want > E->h_snap_bytes) {  // pinned and mapped: the kernel writes host memory directly
    if (E->h_snap) HIPCHK(hipHostFree(E->h_snap));
    E->h_snap = nullptr; E->h_snap_bytes = 0;
    HIPCHK(hipHostMalloc(&E->h_snap, want, hipHostMallocMapped));
    E->h_snap_bytes = want;
  }
  float* h_obs = (float*)((char*)E->h_snap + head);
  HIPCHK(gte::launch_snapshot(E->p.rec, E->p.reward64, E->p.terminated, E->p.truncated, obs_window0(E->p),
                              (int64_t)elems, obs_env_stride(E->p), first, count, E->h_snap,
                              want_obs ? h_obs : nullptr, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));
  *out = (const gte_env_snapshot*)E->h_snap;
  if (obs) *obs = want_obs ? h_obs : nullptr;
  return GTE_OK;
}

int gte_read_envs_view(gte_env* E, int32_t first, int32_t count, int32_t want_obs,
                       const gte_env_snapshot** out, const float** obs) {
  return read_envs_impl(E, first, count, want_obs, out, obs, true);
}

int gte_read_envs(gte_env* E, int32_t first, int32_t count, gte_env_snapshot* out, float* obs) {
  if (!out) return fail(GTE_ERR_INVALID, "NULL argument");
  const gte_env_snapshot* snaps = nullptr;
  const float* h_obs = nullptr;
  TRY(read_envs_impl(E, first, count, obs ? 1 : 0, &snaps, &h_obs, false));
  memcpy(out, snaps, sizeof(gte_env_snapshot) * (size_t)count);
  if (obs) memcpy(obs, h_obs, sizeof(float) * (size_t)E->p.W * (size_t)E->p.Fobs * (size_t)count);
  return GTE_OK;
}

int gte_read_env(gte_env* E, int32_t e, gte_env_snapshot* out, float* obs) {
  return gte_read_envs(E, e, 1, out, obs);
}

int gte_bind_returns(gte_env* E, float* reward, uint8_t* terminated, uint8_t* truncated) {
  if (!E || !reward || !terminated || !truncated) return fail(GTE_ERR_INVALID, "NULL argument");
  // Params travel by value with every launch: later launches see the new pointers,
  // launches already enqueued keep the old ones.
  ledger().withdraw(E, FLAGS);  // (rotated buffers hold an older step's flags: the next step stores densely)
  E->p.reward = reward;
  E->p.terminated = terminated;
  E->p.truncated = truncated;
  return GTE_OK;
}

// the state lives in 128-byte records; snapshot it into struct-of-arrays mirrors
// (stream-ordered: the views reflect every launch enqueued before this call)
static int state_view(gte_env* E, const EnvRec* rec, const gte::StateSoA& o, gte_state_view* out) {
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_extract_state(rec, E->p.N, o, E->stream));
  out->idx = o.idx; out->step = o.step; out->position_index = o.pos;
  out->dataset_index = o.dsi; out->start_idx = o.start; out->episode = o.episode;
  out->needs_reset = o.needs_reset; out->asset = o.asset; out->fiat = o.fiat;
  out->interest_asset = o.ia; out->interest_fiat = o.ifi;
  out->portfolio_valuation = o.pv; out->real_position = o.realpos;
  return GTE_OK;
}

int gte_get_state(gte_env* E, gte_state_view* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  return state_view(E, E->p.rec, E->soa, out);
}

int gte_set_dynamic_features(gte_env* E, const float* values_device, uint32_t mask) {
  if (!E || !values_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_set_dynamic_features before gte_reset");
  if (E->p.nd <= 0 || (mask >> E->p.nd) != 0u)
    return fail(GTE_ERR_INVALID, "mask 0x%x names features beyond n_dyn = %d", mask, E->p.nd);
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_set_dynamic(E->p, values_device, mask, E->stream));
  return GTE_OK;
}

int gte_set_dynamic_columns(gte_env* E, const void* const* columns_device, const int32_t* is_f64) {
  if (!E || !columns_device || !is_f64) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_set_dynamic_columns before gte_reset");
  if (E->p.nd <= 0) return fail(GTE_ERR_INVALID, "the env has no dynamic features");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_set_dynamic_columns(E->p, columns_device, is_f64, E->stream));
  return GTE_OK;
}

int gte_get_final_state(gte_env* E, gte_state_view* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->p.final_rec) return fail(GTE_ERR_STATE, "created without final_obs");
  return state_view(E, E->p.final_rec, E->fsoa, out);
}

// ---------------------------------------------------------------------------
// multi-GPU: the return all-gather over RCCL (gte_comm.hip)

int gte_comm_unique_id(uint8_t* id_out) {
  if (!id_out) return fail(GTE_ERR_INVALID, "id_out is NULL");
  if (const char* why = gte::rccl_load()) return fail(GTE_ERR_STATE, "RCCL unavailable: %s", why);
  const int r = gte::rccl_unique_id(id_out);
  if (r != 0) return fail(GTE_ERR_HIP, "ncclGetUniqueId: %s", gte::rccl_error(r));
  return GTE_OK;
}

int gte_comm_init(gte_env* E, const uint8_t* id, int32_t rank, int32_t world) {
  if (!E || !id) return fail(GTE_ERR_INVALID, "NULL argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(GTE_ERR_INVALID, "rank %d of %d", rank, world);
  if (E->comm) return fail(GTE_ERR_STATE, "the env already has a communicator");
  if (const char* why = gte::rccl_load()) return fail(GTE_ERR_STATE, "RCCL unavailable: %s", why);
  HIPCHK(hipSetDevice(E->cfg.device));
  const int r = gte::rccl_comm_init(&E->comm, id, rank, world);
  if (r != 0) { E->comm = nullptr; return fail(GTE_ERR_HIP, "ncclCommInitRank: %s", gte::rccl_error(r)); }
  E->comm_rank = rank;
  E->comm_world = world;
  // anything failing from here on must not leave a half-made communicator behind (a retry would
  // be refused with "already has a communicator"): undo everything, keep the error message
  auto finish = [&]() -> int {
    HIPCHK(hipStreamCreateWithFlags(&E->comm_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&E->comm_ready, hipEventDisableTiming));
    for (auto& ev : E->comm_done) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (E->gathered_returns) {  // a communicator of another size was here before
      for (void*& q : E->allocs) if (q == (void*)E->gathered_returns) q = nullptr;
      (void)hipFree(E->gathered_returns);
      E->gathered_returns = nullptr;
    }
    TRY(dev_alloc(E, &E->gathered_returns, (size_t)world * 6 * (size_t)E->p.N));
    HIPCHK(hipDeviceSynchronize());
    return GTE_OK;
  };
  const int rc = finish();
  if (rc != GTE_OK) {
    const std::string keep = g_err;
    (void)gte_comm_destroy(E);
    g_err = keep;
  }
  return rc;
}

int gte_allgather(gte_env* E, const void* src_device, void* dst_device, uint64_t bytes_per_rank,
                  int32_t mode) {
  if (!E || !src_device || !dst_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->comm) return fail(GTE_ERR_STATE, "gte_allgather before gte_comm_init");
  if (mode != 0 && mode != 1) return fail(GTE_ERR_INVALID, "mode must be 0 (env stream) or 1 (overlapped)");
  hipStream_t s = E->stream;
  if (mode == 1) {  // behind everything enqueued so far, beside everything enqueued later
    HIPCHK(hipEventRecord(E->comm_ready, E->stream));
    HIPCHK(hipStreamWaitEvent(E->comm_stream, E->comm_ready, 0));
    s = E->comm_stream;
  }
  const int r = gte::rccl_allgather_bytes(E->comm, src_device, dst_device, (size_t)bytes_per_rank, s);
  if (r != 0) return fail(GTE_ERR_HIP, "ncclAllGather: %s", gte::rccl_error(r));
  if (mode == 1) {
    HIPCHK(hipEventRecord(E->comm_done[E->comm_seq & 3], E->comm_stream));
    E->comm_seq += 1;
  }
  return GTE_OK;
}

int gte_allgather_returns(gte_env* E, void* dst_device, int32_t mode, const void** gathered) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->comm) return fail(GTE_ERR_STATE, "gte_allgather_returns before gte_comm_init");
  const Params& p = E->p;
  const size_t N = (size_t)p.N;
  if ((const uint8_t*)p.terminated != (const uint8_t*)p.reward + 4 * N || p.truncated != p.terminated + N)
    return fail(GTE_ERR_STATE, "the bound return buffers are not one packed [reward f32 | terminated u8 "
                               "| truncated u8] block of 6N bytes");
  void* dst = dst_device ? dst_device : (void*)E->gathered_returns;
  TRY(gte_allgather(E, p.reward, dst, 6 * N, mode));
  if (gathered) *gathered = dst;
  return GTE_OK;
}

int gte_allgather_obs(gte_env* E, float* dst_device, int32_t mode) {
  if (!E || !dst_device) return fail(GTE_ERR_INVALID, "NULL argument");
  const Params& p = E->p;
  if (!p.obs) return fail(GTE_ERR_STATE, "gte_allgather_obs before gte_reset (no observation exists yet)");
  if (E->sliding)
    return fail(GTE_ERR_STATE, "gte_allgather_obs on a sliding observation buffer: the windows are not contiguous "
                               "(bind a classic buffer with gte_bind_outputs first)");
  return gte_allgather(E, p.obs, dst_device, sizeof(float) * (size_t)p.N * p.W * p.Fobs, mode);
}

int gte_comm_wait(gte_env* E, int32_t back) {
  if (!E || !E->comm) return fail(GTE_ERR_STATE, "no communicator");
  if (back < 0 || back > 3) return fail(GTE_ERR_INVALID, "back must be 0..3");
  const int64_t k = E->comm_seq - 1 - back;  // the overlapped gather to wait for
  if (k < 0) return GTE_OK;                  // not issued yet: nothing to wait for
  HIPCHK(hipStreamWaitEvent(E->stream, E->comm_done[k & 3], 0));
  return GTE_OK;
}

int gte_comm_synchronize(gte_env* E) {
  if (!E || !E->comm) return fail(GTE_ERR_STATE, "no communicator");
  HIPCHK(hipStreamSynchronize(E->comm_stream));
  return GTE_OK;
}

int gte_comm_destroy(gte_env* E) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->comm) return GTE_OK;
  (void)hipStreamSynchronize(E->stream);
  if (E->comm_stream) (void)hipStreamSynchronize(E->comm_stream);
  const int r = gte::rccl_comm_destroy(E->comm);
  E->comm = nullptr;
  if (E->comm_ready) (void)hipEventDestroy(E->comm_ready);
  for (auto& ev : E->comm_done) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
  if (E->comm_stream) (void)hipStreamDestroy(E->comm_stream);
  E->comm_ready = nullptr;
  E->comm_seq = 0;
  E->comm_stream = nullptr;
  if (r != 0) return fail(GTE_ERR_HIP, "ncclCommDestroy: %s", gte::rccl_error(r));
  return GTE_OK;
}

int gte_set_stream(gte_env* E, void* hip_stream) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipStreamSynchronize(E->stream));
  E->stream = (hipStream_t)hip_stream;  // NULL = the null stream, used as such
  return GTE_OK;
}

int gte_use_own_stream(gte_env* E) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipStreamSynchronize(E->stream));
  E->stream = E->own_stream;
  return GTE_OK;
}

int gte_synchronize(gte_env* E) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipStreamSynchronize(E->stream));
  return GTE_OK;
}

int gte_timer_start(gte_env* E) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipEventRecord(E->ev0, E->stream));
  return GTE_OK;
}

int gte_timer_stop(gte_env* E, float* elapsed_ms) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!elapsed_ms) {  // mark only: record the end now (asynchronous), read it with a later call
    HIPCHK(hipEventRecord(E->ev1, E->stream));
    E->timer_marked = true;
    return GTE_OK;
  }
  if (!E->timer_marked) HIPCHK(hipEventRecord(E->ev1, E->stream));
  E->timer_marked = false;
  HIPCHK(hipEventSynchronize(E->ev1));
  HIPCHK(hipEventElapsedTime(elapsed_ms, E->ev0, E->ev1));
  return GTE_OK;
}

int gte_read_obs(gte_env* E, int32_t first_env, int32_t n, float* host_dst) {
  if (!E || !host_dst) return fail(GTE_ERR_INVALID, "NULL argument");
  const Params& p = E->p;
  if (first_env < 0 || n < 0 || (int64_t)first_env + n > p.N)
    return fail(GTE_ERR_INVALID, "env range [%d, %d) out of [0, %d)", first_env, first_env + n, p.N);
  const size_t per = (size_t)p.W * p.Fobs;
  if (!p.obs) return fail(GTE_ERR_STATE, "gte_read_obs before gte_reset (no observation exists yet)");
  HIPCHK(hipStreamSynchronize(E->stream));
  const size_t stride = (size_t)obs_env_stride(p);
  const float* src = obs_window0(p) + stride * first_env;
  if (stride == per || n == 0)  // classic buffer: one contiguous copy
    HIPCHK(hipMemcpy(host_dst, src, sizeof(float) * per * n, hipMemcpyDeviceToHost));
  else
    HIPCHK(hipMemcpy2D(host_dst, sizeof(float) * per, src, sizeof(float) * stride, sizeof(float) * per, (size_t)n,
                       hipMemcpyDeviceToHost));
  return GTE_OK;
}

int gte_copy_to_host(gte_env* E, const void* device_src, void* host_dst, uint64_t bytes) {
  if (!E || !device_src || !host_dst) return fail(GTE_ERR_INVALID, "NULL argument");
  HIPCHK(hipStreamSynchronize(E->stream));
  HIPCHK(hipMemcpy(host_dst, device_src, (size_t)bytes, hipMemcpyDeviceToHost));
  return GTE_OK;
}

int gte_get_launch_info(gte_env* E, int32_t* envs_per_wave, int32_t* threads_per_block,
                        int32_t* n_blocks, int32_t* vector_bytes) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (envs_per_wave) *envs_per_wave = E->p.epw;
  const LaunchPlan& L = E->plan;
  if (threads_per_block) *threads_per_block = L.threads;
  if (n_blocks) *n_blocks = L.blocks;
  if (vector_bytes)
    *vector_bytes = L.vec * 4 + 1000 * ((L.coop ? 1 : 0) + 2 * L.stage + 16 * L.store + 64 * (L.hot_per_cu & 15) +
                                        1024 * (E->sliding ? L.slide_store : L.store));
  return GTE_OK;
}

#ifdef GTE_STAMPS
// diagnostic build only: device buffer of u64 [n_blocks, 8] for the kernel's time stamps
int gte_debug_set_stamps(gte_env* E, void* device_buf) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  E->p.inj_ds = (const int32_t*)device_buf;
  return GTE_OK;
}
#endif

void gte_destroy(gte_env* E) {
  if (!E) return;
  (void)hipSetDevice(E->cfg.device);
  (void)gte_comm_destroy(E);
  (void)hipStreamSynchronize(E->stream);
  if (E->own_stream) (void)hipStreamSynchronize(E->own_stream);
  for (void* ptr : E->allocs) if (ptr) (void)hipFree(ptr);
  for (auto& v : E->ds_allocs)
    for (void* ptr : v)
      if (ptr) (void)hipFree(ptr);
  for (int32_t* q : {E->d_q_idx, E->d_q_pos, E->d_q_ds})
    if (q) (void)hipFree(q);
  if (E->pd_stats) (void)hipFree(E->pd_stats);
  for (void* q : {(void*)E->tl_list, (void*)E->tl_open_row, E->tl_dev})
    if (q) (void)hipFree(q);
  if (E->tl_host) (void)hipHostFree(E->tl_host);
  for (const gte::PeriodRow& r : E->h_prow)
    if (r.base) (void)hipFree(const_cast<int8_t*>(r.base));
  if (E->h_snap) (void)hipHostFree(E->h_snap);
  if (E->h_logpack) (void)hipHostFree(E->h_logpack);
  if (E->ev0) (void)hipEventDestroy(E->ev0);
  if (E->ev1) (void)hipEventDestroy(E->ev1);
  if (E->own_stream) (void)hipStreamDestroy(E->own_stream);
  ledger().forget(E);
  delete E;
}

}  // extern "C"
