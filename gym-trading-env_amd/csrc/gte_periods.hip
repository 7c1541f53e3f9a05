// gte_periods.hip — period statistics (gte_track_periods, include/gte.h): the backtest kernels with one 32-byte
// record per (env, market period), reduced while they step.  Own translation unit: nothing here can perturb the
// code generated for the kernels of gte_backtest.hip, gte_exits.hip and gte_trades.hip, which run whenever
// period tracking is off.
//
//   gte_period_backtest_kernel   [K][N] actions
//   gte_period_signal_kernel     signal table
//   gte_period_exit_kernel       signal table + exit rules: summary_body (gte_summary_body.h) with that source and
//                                PeriodTracker, the record of the period the env is in held in registers
//                                (PeriodRegs, gte_period_regs.h) — the right column of the table in
//                                gte_backtest.hip.  The period bytes are read as the aligned 16-byte piece around
//                                _idx, kept in registers and fetched again every 16 rows, at a reset and at a
//                                dataset switch — in the signal kernels on the cadence of the signal piece.
//   gte_period_fold_kernel       gte_backtest_fold_kernel: ONE ordinary step into the statistics record and, as
//                                a read-modify-write, into records[e][b].
//   Clearing the period records is a hipMemsetAsync beside launch_backtest_begin (gte_api.hip): a reset row
//   changes no period record.
//
// Every path runs period_step() directly before backtest_step() on the same values, so all of them give the same
// records bit for bit (tests/test_gpu_periods.py), and the statistics record, the env state and the exit state
// are those of the kernels without period records.  What may be read of a period row: bytes [0, len) of the row
// of a dataset index the env record holds, len a multiple of 16 (period_piece checks the row index).  What is
// written: records[e][b] for e < N and 0 <= b < B only (period_step checks the byte).  Compiled WITHOUT
// GTE_HOT_ONLY like gte_backtest.hip.
#include "gte_summary_body.h"

namespace gte {

__global__ __launch_bounds__(256) void gte_period_backtest_kernel(const Params p, const int32_t* actions,
                                                                  gte_backtest_stats* stats, const Periods per,
                                                                  const int n_steps, const int epw) {
  summary_body(p, stats, ActionSource(actions), PeriodTracker(per), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_period_fold_kernel(const Params p, gte_backtest_stats* stats,
                                                              const Periods per) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  gte_backtest_stats a;
  load_stats(stats + e, a);
  const EnvRec* r = &p.rec[e];
  const int32_t flags = (p.terminated[e] ? 1 : 0) | (p.truncated[e] ? 2 : 0);
  // the row the env stood on before the step: one before the row it stands on now, or before the row of its
  // terminal record when the step reset it (same-step mode)
  const EnvRec* w = flags != 0 && p.autoreset == GTE_AUTORESET_SAME_STEP ? &p.final_rec[e] : r;
  const int4 at = reinterpret_cast<const int4*>(w)[0];  // idx, step, pos, dsi
  int32_t b = -1;
  if ((uint32_t)at.w < (uint32_t)p.D) {
    const PeriodRow prow = per.rows[at.w];
    const int32_t i = at.x - 1;
    if ((uint32_t)i < (uint32_t)prow.len) b = prow.base[i];
  }
  gte_period_stats* const mine = per.records + (int64_t)e * per.B;
  PeriodRegs o = {0.0, 0.0, 0, 0, 0, -1};
  period_step(o, mine, per.B, b, a, p, e, r->step, r->pos, p.reward64[e], flags);
  period_close(mine, o);
  backtest_step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
}

__global__ __launch_bounds__(256) void gte_period_signal_kernel(const Params p, const SignalTable* tables, const int S,
                                                                const int32_t* strategy, gte_backtest_stats* stats,
                                                                const Periods per, const int n_steps, const int epw) {
  summary_body(p, stats, SignalSource(tables, S, strategy), PeriodTracker(per), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_period_exit_kernel(const Params p, const SignalTable* tables, const int S,
                                                              const int32_t* strategy, const ExitRules rules,
                                                              gte_backtest_stats* stats, const Periods per,
                                                              const int n_steps, const int epw) {
  summary_body(p, stats, ExitSource(tables, S, strategy, rules), PeriodTracker(per), n_steps, epw);
}

// a launch without the statistics records, the period records, the rows or a B
static bool periods_unusable(const gte_backtest_stats* stats, const Periods& per) {
  return !stats || !per.records || !per.rows || per.B < 1 || per.B > GTE_MAX_PERIODS;
}

hipError_t launch_period_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats,
                                 const Periods& per, int n_steps, int epw, hipStream_t stream) {
  if (summary_refused(p, src, epw) || periods_unusable(stats, per)) return hipErrorInvalidValue;
  const dim3 grid(rollout_blocks(p.N, epw)), block(64 * ROLLOUT_WAVES);
  if (src.actions)
    hipLaunchKernelGGL(gte_period_backtest_kernel, grid, block, 0, stream, p, src.actions, stats, per, n_steps, epw);
  else if (!src.rules)
    hipLaunchKernelGGL(gte_period_signal_kernel, grid, block, 0, stream, p, src.tables, src.S, src.strategy, stats, per,
                       n_steps, epw);
  else
    hipLaunchKernelGGL(gte_period_exit_kernel, grid, block, 0, stream, p, src.tables, src.S, src.strategy, *src.rules,
                       stats, per, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_period_fold(const Params& p, gte_backtest_stats* stats, const Periods& per, hipStream_t stream) {
  if (fold_refused(p) || periods_unusable(stats, per)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_period_fold_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, per);
  return hipGetLastError();
}

}  // namespace gte
