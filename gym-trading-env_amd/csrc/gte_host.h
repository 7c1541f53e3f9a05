// gte_host.h — what the host units of libgte share (gte_api*.hip, the entry points of gte_comm.hip): struct gte_env,
// the error channel, the allocation helpers (the only host-side callers of hipMalloc, hipFree, hipHostMalloc and
// hipHostFree), the shared argument checks and, in namespace gte_host, the functions one unit defines and another calls.
#pragma once

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
#include "gte_own.h"
#include "gte_plan.h"

using gte::DatasetDesc;
using gte::EnvRec;
using gte::Params;
using gte_plan::LaunchPlan;
using gte_plan::SLIDE_AB_ORDER;
using gte_ledger::FLAGS;
using gte_ledger::WINDOW;
using gte_ledger::ledger;

struct gte_env;

#define HIPCHK(expr)                                                              \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess)                                                         \
      return fail(e_ == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP,          \
                  "%s failed: %s", #expr, hipGetErrorString(e_));                 \
  } while (0)

#define TRY(expr)            \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != GTE_OK) return rc_; \
  } while (0)

namespace gte_host {

// the error channel: ONE thread-local string for every unit, defined with fail() and gte_last_error() in gte_api.hip
extern thread_local std::string g_err;
int fail(int code, const char* fmt, ...);
// gte_api.hip: backtest() stays in the unit of enqueue_step; its entry points and gte_signal_actions call these
hipError_t launch_lookup(gte_env* E, const int32_t* strategy, int32_t* actions);
int backtest_entry(gte_env* E, const char* who, const int32_t* actions, const int32_t* strategy, int32_t n_steps,
                   int32_t clear, gte_backtest_stats** stats_device, gte::Curves* cv);

// the owner type (gte_own.h) bound to HIP: a device block, a pinned host block
inline void device_free(void* p) { (void)hipFree(p); }
inline void pinned_free(void* p) { (void)hipHostFree(p); }
using DeviceBlock = gte_own::Block<device_free>;
using PinnedBlock = gte_own::Block<pinned_free>;
// gte_api_backtest.hip: an upload unbinds what was checked against the old T; the trade pools read the list
int publish_signal_table(gte_env* E, int32_t d, const gte::SignalTable& t);
int publish_period_row(gte_env* E, int32_t d, DeviceBlock&& row);
int trade_list_on(gte_env* E, const char* who);
// a library-owned device block that only grows: grow(), below, with the leaderboard analyses' checks
struct Scratch { void* base = nullptr; size_t bytes = 0; };

// ---- what gte_env keeps per feature.  A buffer that is allocated once is in gte_env::allocs; one that may be
// replaced is an owner (DeviceBlock, PinnedBlock) here, released by `delete E`: gte_destroy names none of them ----
struct BacktestState {
  // gte_backtest: the statistics records and, in same-step mode without final_obs, terminal records
  // of its own (the terminal valuation is read from them); allocated by the first call
  gte_backtest_stats* stats = nullptr;
  EnvRec* final_rec = nullptr;
  int32_t* sig_actions = nullptr;  // the lookup's output for gte_backtest_signals
  // gte_backtest_curves: the window of every env that is open between the fused launch and the fold (gte_curves.hip)
  gte::CurveCarry* carry = nullptr;
};

struct TradeState {
  // gte_track_trades: the trade records (allocated by the first call that turns tracking on), whether the
  // backtest calls maintain them, and whether that changed since the last backtest call (which then clears)
  gte_trade_stats* stats = nullptr;
  bool on = false, changed = false;
  // gte_track_trade_list: the [N][cap] list (cap == 0: off; alloc_cap: the capacity it was allocated
  // for) and the open_row of every env; a change sets `changed`.  gte_read_trade_list: its device block (ids,
  // first, closed, trades) and the host copy `out` points into
  DeviceBlock list, open_row;
  int32_t cap = 0, alloc_cap = 0;
  DeviceBlock dev;
  PinnedBlock host;
};

struct PeriodState {
  // gte_track_periods / gte_bind_periods: the [N][B] period records (B == 0: tracking off; alloc_B: the B
  // they were allocated for), whether tracking, B or a row changed since the last backtest call (which then
  // clears), and the period row of every dataset (base null = none bound; the base IS the library's allocation,
  // held by row_block) on the host and on the device
  DeviceBlock stats;
  int32_t B = 0, alloc_B = 0;
  bool changed = false;
  std::vector<gte::PeriodRow> h_row;
  std::vector<DeviceBlock> row_block;
  gte::PeriodRow* d_row = nullptr;
};

struct SignalState {
  // signal tables (gte_bind_signals): one descriptor per dataset (base null = none bound), the host
  // copy and the device array the kernels read
  std::vector<gte::SignalTable> h_tab;
  gte::SignalTable* d_tab = nullptr;
  int32_t S = 0;  // strategies of every bound table (0 = none bound)
  // exit rules (gte_bind_exit_rules): the caller's rules and map (rules null = none bound) and the per-env
  // state, allocated by the first bind
  gte::ExitRules exits = {nullptr, nullptr, nullptr, 0};
};

struct RankState {
  // gte_rank_strategies: the two candidate lists (gte_strategy.hip), allocated by the first call and
  // again when S outgrows them (the old ones stay until gte_destroy: launches in flight may read them)
  double* score[2] = {nullptr, nullptr};
  int32_t* index[2] = {nullptr, nullptr};
  int64_t entries[2] = {0, 0};
  // gte_reality_check, gte_cscv, gte_diversify, gte_trade_monte_carlo, gte_spa_test: the scratch of each
  // (gte_bootstrap.hip, gte_cscv.hip, gte_diversify.hip, gte_montecarlo.hip, gte_spa.hip), a block of its own that
  // grow() keeps the same way (gte_spa_test also runs a reality check: in boot_scratch, as gte_reality_check does)
  Scratch boot_scratch, cscv_scratch, div_scratch, mc_scratch, spa_scratch;
};

struct CommState {
  // multi-GPU return exchange (gte_comm.hip): one RCCL communicator per env
  void* handle = nullptr;
  int rank = 0, world = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ready = nullptr;
  hipEvent_t done[4] = {nullptr, nullptr, nullptr, nullptr};  // ring: one per overlapped gather
  int64_t seq = 0;                                             // overlapped gathers so far
  DeviceBlock gathered_returns;  // u8 [world, 6N], library-owned destination
};

struct ReadbackState {
  PinnedBlock snap;         // pinned host memory for gte_read_envs: snapshots, then observations
  bool view_reads = false;  // gte_read_envs_view has been used: the buffer is kept at full size
  PinnedBlock logpack;      // pinned host memory for gte_read_log_envs
};

}  // namespace gte_host
using namespace gte_host;

struct gte_env {
  gte_config cfg;
  Params p;
  int n_cu = 0;  // compute units of cfg.device (require_device)
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<void*> allocs;       // everything freed in gte_destroy
  std::vector<DatasetDesc> h_ds;   // host copy of the descriptor table
  std::vector<DeviceBlock> ds_allocs[4]; // per dataset: feat, close, high, low
  DatasetDesc* d_ds = nullptr;
  gte_outputs owned;
  // staging buffers for host-side arguments
  int32_t* d_actions = nullptr;
  uint8_t* d_mask = nullptr;
  int32_t *d_inj_idx = nullptr, *d_inj_pos = nullptr, *d_inj_ds = nullptr;
  DeviceBlock d_q_idx, d_q_pos, d_q_ds;  // the queued draws of gte_set_autoreset_injection
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
  BacktestState backtest;
  TradeState trades;
  PeriodState periods;
  SignalState signals;
  RankState rank;
  CommState comm;
  ReadbackState readback;
  bool timer_marked = false;  // gte_timer_stop(NULL) recorded the end event already
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

// dev_alloc after create, for a buffer the env's stream uses next: the zero-fill ran on the null
// stream and the env's stream is non-blocking, so wait for it here
template <typename T>
static int dev_alloc_late(gte_env* E, T** out, size_t count) {
  TRY(dev_alloc(E, out, count));
  HIPCHK(hipDeviceSynchronize());
  return GTE_OK;
}

// Allocate-and-report for a replaceable device block: `bytes` fresh bytes into *out (what it held is released
// after the allocation succeeded), or the caller's message, whose last %s is HIP's word for the failure
template <typename... Args>
static int device_alloc(DeviceBlock* out, size_t bytes, const char* fmt, Args... args) {
  void* fresh = nullptr;
  const hipError_t e = hipMalloc(&fresh, bytes);
  if (e == hipSuccess) return out->replace(fresh, bytes), GTE_OK;
  (void)hipGetLastError();
  return fail(e == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP, fmt, args..., hipGetErrorString(e));
}

// The pinned host blocks: what *out held is freed first, then `bytes` fresh bytes with hipHostMalloc's `flags`
static int pinned_alloc(PinnedBlock* out, size_t bytes, unsigned flags) {
  out->reset();
  void* fresh = nullptr;
  HIPCHK(hipHostMalloc(&fresh, bytes, flags));
  out->replace(fresh, bytes);
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

// ---- a per-dataset table of rows on the device: the checks gte_bind_signals and the builders share ----
// A row holds T elements and is padded: the stride is a whole number of 16-byte pieces and at least T
// rounded up to 16 elements, so that an aligned 16-byte access anywhere in a row stays inside it.
static int64_t round_up_16(int64_t T) { return (T + 15) / 16 * 16; }

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
  const size_t bytes = gte_own::grow_doubling(s->bytes, need);
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
