// gte_trade_list.hip — the trade list (gte_track_trade_list, include/gte.h): the kernels of gte_trades.hip that
// also write one 48-byte gte_trade per closed trade into list[e][closed], and the gather that reads lists back.
// Own translation unit: nothing here can perturb the code generated for the kernels of gte_backtest.hip,
// gte_exits.hip, gte_trades.hip and gte_periods.hip, which run whenever the list is off.
//
//   gte_trade_list_backtest_kernel   [K][N] actions
//   gte_trade_list_signal_kernel     signal table
//   gte_trade_list_exit_kernel       signal table + exit rules: summary_body (gte_summary_body.h) with that source and
//                                    TradeListTracker — TradeTracker plus the list base, the capacity and the env's
//                                    open_row.  The tracker is the sink of trade_step() (gte_trade_regs.h): the
//                                    record is written inside a close only, as three plain 16-byte stores, so a
//                                    step that closes nothing issues no request its gte_trades.hip twin does not.
//   gte_trade_list_fold_kernel       gte_trade_fold_kernel: ONE ordinary step into both records and the list.
//   gte_trade_list_begin_kernel      gte_trade_begin_kernel, and open_row where a record is cleared or reset.
//   gte_trade_list_scan_kernel       the gather: closed[j] and first[j], the running sum of min(closed, capacity),
//                                    one workgroup that loops over the requests with a carry
//   gte_trade_list_pack_kernel       ... and the valid records of request j to out[first[j] ..), one wavefront
//                                    per request, 16-byte pieces, consecutive lanes consecutive pieces on both sides
//
// The fold and begin kernels find row_t the way gte_period_fold_kernel does: one before the row of the env record,
// or of the terminal record after a same-step reset.  What is written: list[e][c] for e < N and c < capacity only
// (TradeListTracker::write checks c); out[i] for i < max_out only.  Compiled WITHOUT GTE_HOT_ONLY like
// gte_backtest.hip.
#include "gte_summary_body.h"

namespace gte {

static_assert(sizeof(gte_trade) == 48 && offsetof(gte_trade, position) == 16 && offsetof(gte_trade, entry_row) == 24 &&
              offsetof(gte_trade, hold) == 32 && offsetof(gte_trade, flags) == 44,
              "gte_trade: three doubles, six 32-bit words, three 16-byte pieces");

// TradeTracker and the list.  row / dsi: where the env stood before the step (before()); next: where it stands
// after it (landed()); open_row is loaded once and stored once per launch like the record.
struct TradeListTracker {
  static constexpr bool pieces = false;
  gte_trade_stats* trades;
  const TradeList tl;
  gte_trade_stats t = {};
  gte_trade* mine = nullptr;
  int32_t open_row = 0, row = 0, dsi = 0, next = 0;
  __device__ __forceinline__ TradeListTracker(gte_trade_stats* trades_, const TradeList& tl_)
      : trades(trades_), tl(tl_) {}
  __device__ __forceinline__ void init(bool active, int e) {
    mine = tl.list + (int64_t)e * tl.capacity;
    if (!active) return;
    load_trades(trades + e, t);
    open_row = tl.open_row[e];
  }
  __device__ __forceinline__ void dataset(int32_t) {}
  __device__ __forceinline__ void piece(int32_t) {}
  __device__ __forceinline__ int32_t limit() const { return 0; }
  __device__ __forceinline__ void before(int32_t idx, int32_t dsi_) { row = idx; dsi = dsi_; }
  __device__ __forceinline__ void landed(int32_t idx) { next = idx; }
  // the sink of trade_step(): rec is the record directly before trade_close()
  __device__ __forceinline__ void write(const gte_trade_stats& rec, double vc, int32_t kind, int32_t flags) const {
    if ((uint32_t)rec.closed >= (uint32_t)tl.capacity) return;
    const int32_t exit_row = kind == 2 ? row + 1 : row;
    const double2_t d0 = {rec.open_value, vc};
    const int4_t c1 = {__double2loint(rec.open_position), __double2hiint(rec.open_position), open_row, exit_row};
    const int4_t c2 = {rec.open_len, dsi, kind, flags};
    gte_trade* const dst = mine + rec.closed;
    reinterpret_cast<double2_t*>(dst)[0] = d0;
    reinterpret_cast<int4_t*>(dst)[1] = c1;
    reinterpret_cast<int4_t*>(dst)[2] = c2;
  }
  __device__ __forceinline__ void close(const gte_trade_stats& rec, double v, bool flat, int32_t flags) const {
    write(rec, flat ? v : rec.last_valuation, flat ? 0 : 1, flags);
  }
  __device__ __forceinline__ void forced(const gte_trade_stats& rec, double v, int32_t flags) const {
    write(rec, v, 2, flags);
  }
  __device__ __forceinline__ void open() { open_row = row; }
  __device__ __forceinline__ void reset_row() { open_row = next; }
  __device__ __forceinline__ void step(const gte_backtest_stats& a, const Params& p, int e, int32_t step_after,
                                       double pv, int32_t pos_after, double reward, int32_t flags) {
    trade_step(t, a, p, e, step_after, pv, pos_after, reward, flags, *this);
  }
  __device__ __forceinline__ void store(int e) {
    store_trades(trades + e, t);
    tl.open_row[e] = open_row;
  }
};

__global__ __launch_bounds__(256) void gte_trade_list_backtest_kernel(const Params p, const int32_t* actions,
                                                                      gte_backtest_stats* stats,
                                                                      gte_trade_stats* trades, const TradeList tl,
                                                                      const int n_steps, const int epw) {
  summary_body(p, stats, ActionSource(actions), TradeListTracker(trades, tl), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_trade_list_signal_kernel(const Params p, const SignalTable* tables,
                                                                    const int S, const int32_t* strategy,
                                                                    gte_backtest_stats* stats, gte_trade_stats* trades,
                                                                    const TradeList tl, const int n_steps,
                                                                    const int epw) {
  summary_body(p, stats, SignalSource(tables, S, strategy), TradeListTracker(trades, tl), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_trade_list_exit_kernel(const Params p, const SignalTable* tables, const int S,
                                                                  const int32_t* strategy, const ExitRules rules,
                                                                  gte_backtest_stats* stats, gte_trade_stats* trades,
                                                                  const TradeList tl, const int n_steps,
                                                                  const int epw) {
  summary_body(p, stats, ExitSource(tables, S, strategy, rules), TradeListTracker(trades, tl), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_trade_list_fold_kernel(const Params p, gte_backtest_stats* stats,
                                                                  gte_trade_stats* trades, const TradeList tl) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  gte_backtest_stats a;
  load_stats(stats + e, a);
  TradeListTracker trk(trades, tl);
  trk.init(true, e);
  const EnvRec* r = &p.rec[e];
  const int32_t flags = (p.terminated[e] ? 1 : 0) | (p.truncated[e] ? 2 : 0);
  // the row the env stood on before the step: one before the row it stands on now, or before the row of its
  // terminal record when the step reset it (same-step mode)
  const EnvRec* w = flags != 0 && p.autoreset == GTE_AUTORESET_SAME_STEP ? &p.final_rec[e] : r;
  const int4 at = reinterpret_cast<const int4*>(w)[0];  // idx, step, pos, dsi
  trk.before(at.x - 1, at.w);
  trk.landed(r->idx);
  trk.step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  backtest_step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
  trk.store(e);
}

__global__ __launch_bounds__(256) void gte_trade_list_begin_kernel(const Params p, gte_backtest_stats* stats,
                                                                   gte_trade_stats* trades, const TradeList tl,
                                                                   const int clear) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  gte_backtest_stats a = {};
  gte_trade_stats t = {};
  const EnvRec* r = &p.rec[e];
  if (!clear) {
    load_stats(stats + e, a);
    load_trades(trades + e, t);
  }
  if (clear) {
    backtest_reset(a, r->pv, p.positions[r->pos]);
    a.valuation_last = r->pv;
    trade_clear(t, r->pv, p.positions[r->pos]);
    tl.open_row[e] = r->idx;  // the row the env stands on
  } else if (r->episode != a.episode_seen) {
    backtest_reset(a, r->pv, p.positions[r->pos]);  // reset between two calls: the sums go on
    trade_reset_row(t, r->pv, p.positions[r->pos]);
    tl.open_row[e] = r->idx;  // row_0
  }
  a.ended = r->needs_reset;
  a.step_seen = r->step;
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
  store_trades(trades + e, t);
}

// --- the gather

constexpr int SCAN_THREADS = 256, SCAN_PER_THREAD = 4, SCAN_SPAN = SCAN_THREADS * SCAN_PER_THREAD;

// the env of request j, or -1 for an id outside [0, n_envs)
__device__ __forceinline__ int32_t requested_env(const int32_t* ids, int j, int n_envs) {
  const int32_t e = ids ? ids[j] : j;
  return (uint32_t)e < (uint32_t)n_envs ? e : -1;
}

// ONE workgroup: per pass SCAN_SPAN requests, thread i the SCAN_PER_THREAD consecutive ones from i * SCAN_PER_THREAD;
// an exclusive scan of the threads' sums through LDS, the passes chained by a carry
__global__ __launch_bounds__(SCAN_THREADS) void gte_trade_list_scan_kernel(const gte_trade_stats* trades,
                                                                           const int capacity, const int n_envs,
                                                                           const int32_t* ids, const int n_ids,
                                                                           int64_t* first, int32_t* closed) {
  __shared__ int64_t part[SCAN_THREADS];
  __shared__ int64_t carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n_ids; base += SCAN_SPAN) {
    int32_t n[SCAN_PER_THREAD];
    int64_t mine = 0;
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
      const int j = base + tid * SCAN_PER_THREAD + i;
      n[i] = 0;
      if (j < n_ids) {
        const int32_t e = requested_env(ids, j, n_envs);
        const int32_t c = e >= 0 ? trades[e].closed : -1;
        closed[j] = c;
        n[i] = c < 0 ? 0 : c < capacity ? c : capacity;
      }
      mine += n[i];
    }
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {  // inclusive scan of part[]
      const int64_t add = tid >= d ? part[tid - d] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    int64_t at = carry + part[tid] - mine;
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
      const int j = base + tid * SCAN_PER_THREAD + i;
      if (j < n_ids) first[j] = at;
      at += n[i];
    }
    __syncthreads();
    if (tid == SCAN_THREADS - 1) carry += part[tid];
    __syncthreads();
  }
  if (tid == 0) first[n_ids] = carry;
}

__global__ __launch_bounds__(256) void gte_trade_list_pack_kernel(const gte_trade* list, const int capacity,
                                                                  const int n_envs, const int32_t* ids, const int n_ids,
                                                                  const int64_t* first, gte_trade* out,
                                                                  const int64_t max_out) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= n_ids) return;
  const int32_t e = requested_env(ids, j, n_envs);
  if (e < 0) return;
  const int64_t lo = first[j], hi = first[j + 1] < max_out ? first[j + 1] : max_out;
  int64_t n = hi - lo;  // (first[j + 1] - first[j] <= capacity: the scan wrote both)
  if (n > capacity) n = capacity;
  const int4_t* src = reinterpret_cast<const int4_t*>(list + (int64_t)e * capacity);
  int4_t* dst = reinterpret_cast<int4_t*>(out + lo);
  for (int64_t i = lane; i < 3 * n; i += 64) dst[i] = src[i];
}

static bool list_unusable(const gte_backtest_stats* stats, const gte_trade_stats* trades, const TradeList& tl) {
  return !stats || !trades || !tl.list || !tl.open_row || tl.capacity < 1 || tl.capacity > GTE_MAX_TRADE_LIST;
}

hipError_t launch_trade_list_begin(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades,
                                   const TradeList& tl, int clear, hipStream_t stream) {
  if (list_unusable(stats, trades, tl)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_list_begin_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, trades, tl,
                     clear);
  return hipGetLastError();
}

hipError_t launch_trade_list_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats,
                                     gte_trade_stats* trades, const TradeList& tl, int n_steps, int epw,
                                     hipStream_t stream) {
  if (summary_refused(p, src, epw) || list_unusable(stats, trades, tl)) return hipErrorInvalidValue;
  const dim3 grid(rollout_blocks(p.N, epw)), block(64 * ROLLOUT_WAVES);
  if (src.actions)
    hipLaunchKernelGGL(gte_trade_list_backtest_kernel, grid, block, 0, stream, p, src.actions, stats, trades, tl,
                       n_steps, epw);
  else if (!src.rules)
    hipLaunchKernelGGL(gte_trade_list_signal_kernel, grid, block, 0, stream, p, src.tables, src.S, src.strategy, stats,
                       trades, tl, n_steps, epw);
  else
    hipLaunchKernelGGL(gte_trade_list_exit_kernel, grid, block, 0, stream, p, src.tables, src.S, src.strategy,
                       *src.rules, stats, trades, tl, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_trade_list_fold(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades,
                                  const TradeList& tl, hipStream_t stream) {
  if (fold_refused(p) || list_unusable(stats, trades, tl)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_list_fold_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, trades, tl);
  return hipGetLastError();
}

hipError_t launch_trade_list_scan(const gte_trade_stats* trades, const TradeList& tl, int n_envs, const int32_t* ids,
                                  int n_ids, int64_t* first, int32_t* closed, hipStream_t stream) {
  if (!trades || tl.capacity < 1 || n_envs < 1 || n_ids < 0 || !first || (n_ids > 0 && !closed))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_list_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, trades, tl.capacity, n_envs,
                     ids, n_ids, first, closed);
  return hipGetLastError();
}

hipError_t launch_trade_list_pack(const TradeList& tl, int n_envs, const int32_t* ids, int n_ids, const int64_t* first,
                                  gte_trade* out, int64_t max_out, hipStream_t stream) {
  if (!tl.list || tl.capacity < 1 || n_envs < 1 || n_ids < 1 || !first || !out || max_out < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_list_pack_kernel, dim3((n_ids + 3) / 4), dim3(256), 0, stream, tl.list, tl.capacity,
                     n_envs, ids, n_ids, first, out, max_out);
  return hipGetLastError();
}

}  // namespace gte
