// gte_backtest.hip — backtest summaries: K consecutive TradingEnv.step calls (environments.py:233-272)
// that leave, per env, a record of running statistics (gte_backtest_stats, include/gte.h: return
// sums, drawdown, trades, episode ends) instead of [K, N] rows of per-step results.  Own translation
// unit: nothing here can perturb the code generated for the step and rollout kernels.
//
//   gte_backtest_kernel        summary_body (gte_summary_body.h: the one loop of the from-registers kernels,
//                              explained there) with the [K][N] actions as its source and no tracker.
//   gte_backtest_signal_kernel ... with the lookup in the env's signal table, at its own row, as the source.
//
//       source \ tracker     none                          trade record               period records
//       [K][N] actions       gte_backtest_kernel           gte_trade_backtest_kernel  gte_period_backtest_kernel
//       signal table         gte_backtest_signal_kernel    gte_trade_signal_kernel    gte_period_signal_kernel
//       ... + exit rules     gte_backtest_exit_kernel      gte_trade_exit_kernel      gte_period_exit_kernel
//                            (this file; gte_exits.hip)    (gte_trades.hip)           (gte_periods.hip)
//
//   gte_backtest_fold_kernel   ONE step into the records from what an ordinary step launch left behind
//                              (reward64, flags, the record, the terminal record): the last step of a
//                              call, and every step where gte_rollout itself goes step by step.
//   gte_backtest_begin_kernel  clears the records, or brings them up to date with a gte_reset.
//   gte_signal_actions_kernel  the action a signal table (gte_bind_signals) gives every env for its next
//                              step: one lane per env, the record's idx / dsi -> one byte -> int32.
//
// Both paths run the same backtest_step() on the same values, so they give the same records bit for bit
// (tests/test_gpu_backtest.py).  This unit is compiled WITHOUT GTE_HOT_ONLY (gte_summary_body.h says why).
#include "gte_summary_body.h"

namespace gte {

__global__ __launch_bounds__(256) void gte_backtest_kernel(const Params p, const int32_t* actions,
                                                           gte_backtest_stats* stats, const int n_steps,
                                                           const int epw) {
  summary_body(p, stats, ActionSource(actions), NoTracker(), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_backtest_fold_kernel(const Params p, gte_backtest_stats* stats) {
  fold_body(p, stats, NoTracker());
}

__global__ __launch_bounds__(256) void gte_backtest_begin_kernel(const Params p, gte_backtest_stats* stats,
                                                                 const int clear) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  gte_backtest_stats a = {};
  const EnvRec* r = &p.rec[e];
  if (!clear) load_stats(stats + e, a);
  if (clear) {
    backtest_reset(a, r->pv, p.positions[r->pos]);
    a.valuation_last = r->pv;
  } else if (r->episode != a.episode_seen) {
    backtest_reset(a, r->pv, p.positions[r->pos]);  // reset between two calls: the sums go on
  }
  a.ended = r->needs_reset;
  a.step_seen = r->step;
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
}

// --- signal tables: the action looked up by the row the env stands on (include/gte.h, gte_bind_signals)

__global__ __launch_bounds__(256) void gte_signal_actions_kernel(const Params p, const SignalTable* tables,
                                                                 const int S, const int32_t* strategy,
                                                                 int32_t* actions) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  const int4_t a = reinterpret_cast<const int4_t*>(&p.rec[e])[0];  // idx, step, pos, dsi
  const SignalTable t = tables[a[3]];
  actions[e] = signal_action(t.base[signal_strategy(p, strategy, S, e) * t.stride + a[0]], p.P);
}

__global__ __launch_bounds__(256) void gte_backtest_signal_kernel(const Params p, const SignalTable* tables,
                                                                  const int S, const int32_t* strategy,
                                                                  gte_backtest_stats* stats, const int n_steps,
                                                                  const int epw) {
  summary_body(p, stats, SignalSource(tables, S, strategy), NoTracker(), n_steps, epw);
}

hipError_t launch_backtest_begin(const Params& p, gte_backtest_stats* stats, int clear, hipStream_t stream) {
  hipLaunchKernelGGL(gte_backtest_begin_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, clear);
  return hipGetLastError();
}

hipError_t launch_backtest_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats, int n_steps,
                                   int epw, hipStream_t stream) {
  if (summary_refused(p, src, epw) || !src.actions) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_backtest_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream, p,
                     src.actions, stats, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_signal_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats, int n_steps,
                                 int epw, hipStream_t stream) {
  if (summary_refused(p, src, epw) || src.actions) return hipErrorInvalidValue;
  if (src.rules) return launch_exit_summary(p, src, stats, n_steps, epw, stream);  // (gte_exits.hip)
  hipLaunchKernelGGL(gte_backtest_signal_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream,
                     p, src.tables, src.S, src.strategy, stats, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_signal_actions(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                                 int32_t* actions, hipStream_t stream) {
  if (!tables_usable(tables, S) || !actions) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_signal_actions_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, tables, S,
                     strategy, actions);
  return hipGetLastError();
}

hipError_t launch_backtest_fold(const Params& p, gte_backtest_stats* stats, hipStream_t stream) {
  if (fold_refused(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_backtest_fold_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats);
  return hipGetLastError();
}

}  // namespace gte
