// gte_trades.hip — trade statistics (gte_track_trades, include/gte.h): the backtest kernels with a second
// 128-byte record per env, the round-trip trade statistics, reduced while they step.  Own translation unit:
// nothing here can perturb the code generated for the kernels of gte_backtest.hip and gte_exits.hip, which
// run whenever tracking is off.
//
//   gte_trade_backtest_kernel   [K][N] actions
//   gte_trade_signal_kernel     signal table
//   gte_trade_exit_kernel       signal table + exit rules: summary_body (gte_summary_body.h) with that source and
//                               TradeTracker, the env's trade record in registers as well — the middle column of
//                               the table in gte_backtest.hip.  The trade record is loaded once and stored once
//                               per launch, as 16-byte pieces; a step issues no memory request its untracked
//                               twin does not issue.
//   gte_trade_fold_kernel       gte_backtest_fold_kernel: ONE ordinary step into BOTH records.
//   gte_trade_begin_kernel      gte_backtest_begin_kernel: clears both records, or applies the reset row of a
//                               gte_reset between two calls to both.
//
// Every path runs trade_step() directly before backtest_step() on the same values, so all of them give the
// same two records bit for bit (tests/test_gpu_trades.py), and the statistics record, the env state and the
// exit state are those of the kernels without the trade record.  Compiled WITHOUT GTE_HOT_ONLY like
// gte_backtest.hip.
#include "gte_summary_body.h"

namespace gte {

__global__ __launch_bounds__(256) void gte_trade_backtest_kernel(const Params p, const int32_t* actions,
                                                                 gte_backtest_stats* stats, gte_trade_stats* trades,
                                                                 const int n_steps, const int epw) {
  summary_body(p, stats, ActionSource(actions), TradeTracker(trades), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_trade_fold_kernel(const Params p, gte_backtest_stats* stats,
                                                             gte_trade_stats* trades) {
  fold_body(p, stats, TradeTracker(trades));
}

__global__ __launch_bounds__(256) void gte_trade_begin_kernel(const Params p, gte_backtest_stats* stats,
                                                              gte_trade_stats* trades, const int clear) {
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
  } else if (r->episode != a.episode_seen) {
    backtest_reset(a, r->pv, p.positions[r->pos]);  // reset between two calls: the sums go on
    trade_reset_row(t, r->pv, p.positions[r->pos]);
  }
  a.ended = r->needs_reset;
  a.step_seen = r->step;
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
  store_trades(trades + e, t);
}

__global__ __launch_bounds__(256) void gte_trade_signal_kernel(const Params p, const SignalTable* tables, const int S,
                                                               const int32_t* strategy, gte_backtest_stats* stats,
                                                               gte_trade_stats* trades, const int n_steps,
                                                               const int epw) {
  summary_body(p, stats, SignalSource(tables, S, strategy), TradeTracker(trades), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_trade_exit_kernel(const Params p, const SignalTable* tables, const int S,
                                                             const int32_t* strategy, const ExitRules rules,
                                                             gte_backtest_stats* stats, gte_trade_stats* trades,
                                                             const int n_steps, const int epw) {
  summary_body(p, stats, ExitSource(tables, S, strategy, rules), TradeTracker(trades), n_steps, epw);
}

hipError_t launch_trade_begin(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades, int clear,
                              hipStream_t stream) {
  if (!stats || !trades) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_begin_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, trades, clear);
  return hipGetLastError();
}

// what launch_backtest_summary refuses (gte_launch.h), and a launch without both records
hipError_t launch_trade_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats,
                                gte_trade_stats* trades, int n_steps, int epw, hipStream_t stream) {
  if (summary_refused(p, src, epw) || !stats || !trades) return hipErrorInvalidValue;
  const dim3 grid(rollout_blocks(p.N, epw)), block(64 * ROLLOUT_WAVES);
  if (src.actions)
    hipLaunchKernelGGL(gte_trade_backtest_kernel, grid, block, 0, stream, p, src.actions, stats, trades, n_steps, epw);
  else if (!src.rules)
    hipLaunchKernelGGL(gte_trade_signal_kernel, grid, block, 0, stream, p, src.tables, src.S, src.strategy, stats,
                       trades, n_steps, epw);
  else
    hipLaunchKernelGGL(gte_trade_exit_kernel, grid, block, 0, stream, p, src.tables, src.S, src.strategy, *src.rules,
                       stats, trades, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_trade_fold(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades,
                             hipStream_t stream) {
  if (fold_refused(p) || !stats || !trades) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_fold_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, trades);
  return hipGetLastError();
}

}  // namespace gte
