// gte_periods.hip — period statistics (gte_track_periods, include/gte.h): the backtest kernels with one 32-byte
// record per (env, market period), reduced while they step.  Own translation unit: nothing here can perturb the
// code generated for the kernels of gte_backtest.hip, gte_exits.hip and gte_trades.hip, which run whenever
// period tracking is off.
//
//   gte_period_backtest_kernel   gte_backtest_kernel         (gte_backtest.hip) ...
//   gte_period_signal_kernel     gte_backtest_signal_kernel  (gte_backtest.hip) ...
//   gte_period_exit_kernel       gte_backtest_exit_kernel    (gte_exits.hip)    ... with the record of the period
//                                the env is in held in registers (PeriodRegs, gte_period_regs.h) — same geometry,
//                                same lambda structure, same steps, same handling of the statistics record and
//                                the exit state (see there).  The period bytes are read as the aligned 16-byte
//                                piece around _idx, kept in registers and fetched again every 16 rows, at a reset
//                                and at a dataset switch — in the signal kernels on the cadence of the signal
//                                piece.  A lane stores its open record (two 16-byte pieces) and loads the next
//                                when its env's row enters another period, and stores it at the launch's end.
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
#include "gte_exit_regs.h"
#include "gte_period_regs.h"

namespace gte {

__global__ __launch_bounds__(256) void gte_period_backtest_kernel(const Params p, const int32_t* actions,
                                                                  gte_backtest_stats* stats, const Periods per,
                                                                  const int n_steps, const int epw) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  if (active) load_stats(stats + e, a);
  gte_period_stats* const mine = per.records + (int64_t)e * per.B;
  PeriodRegs o = {0.0, 0.0, 0, 0, 0, -1};
  int32_t act = active ? actions[e] : -1;
  int32_t qdsi = -1, qbase = 0;  // the period piece in registers: of dataset qdsi, rows qbase .. qbase + 15
  PeriodRow prow = {nullptr, 0};
  int4_t pw = {-1, -1, -1, -1};
  auto fetch = [&](int32_t idx) {
    if (s.dsi != qdsi) {
      prow = per.rows[s.dsi];
      qdsi = s.dsi;
    }
    qbase = idx & ~15;
    pw = period_piece(prow.base, prow.len, idx);
  };
  if (active) fetch(s.idx);
  PriceCarry pc = {0.0, 0.0, -1, 0};
  ObsJob job;
  // (a lambda like gte_backtest_kernel's step, for the same reason)
  auto run_a = [&](int k) {
    const int32_t now = act;
    const int32_t b = signal_byte(pw, s.idx);  // the period of the row the env stands on before the step
    if (active && k + 1 < n_steps) act = actions[(int64_t)(k + 1) * p.N + e];
    if (active && k + 1 < n_steps && (s.idx & 15) == 15 && s.idx + 1 < prow.len) fetch(s.idx + 1);
    double pv = 0.0;
    StepOut so = {};
    phase_a<MODE_STEP>(p, e, active, lane, job, nullptr, /*compact=*/false, &pv, &s, &now,
                       /*write_record=*/k == n_steps - 1, &pc, &so);
    if (active) {
      period_step(o, mine, per.B, b, a, p, e, s.step, s.pos, so.reward, so.flags);
      backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
    }
    if (active && k + 1 < n_steps && (s.dsi != qdsi || (s.idx & ~15) != qbase)) fetch(s.idx);
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    a.episode_seen = p.rec[e].episode;  // (this lane's own resets wrote it)
    store_stats(stats + e, a);
    period_close(mine, o);
  }
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

// gte_backtest_signal_kernel (gte_backtest.hip: geometry, piece fetch and its bounds, record handling — see
// there) with the period records; the period piece moves with the signal piece
__global__ __launch_bounds__(256) void gte_period_signal_kernel(const Params p, const SignalTable* tables, const int S,
                                                                const int32_t* strategy, gte_backtest_stats* stats,
                                                                const Periods per, const int n_steps, const int epw) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  if (active) load_stats(stats + e, a);
  gte_period_stats* const mine = per.records + (int64_t)e * per.B;
  PeriodRegs o = {0.0, 0.0, 0, 0, 0, -1};
  const int64_t strat = active ? signal_strategy(p, strategy, S, e) : 0;
  const int8_t* row = nullptr;  // this env's row of the table of dataset pdsi
  int32_t pdsi = -1;
  int32_t lim = 0, pbase = 0;
  int4_t w = {0, 0, 0, 0};
  PeriodRow prow = {nullptr, 0};
  int4_t pw = {-1, -1, -1, -1};
  auto fetch = [&](int32_t idx) {
    if (s.dsi != pdsi) {
      const SignalTable tb = tables[s.dsi];
      row = tb.base + strat * tb.stride;
      prow = per.rows[s.dsi];
      pdsi = s.dsi;
      lim = tb.stride > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)tb.stride;
    }
    pbase = idx & ~15;
    w = *reinterpret_cast<const int4_t*>(row + pbase);
    pw = period_piece(prow.base, prow.len, idx);
  };
  if (active) fetch(s.idx);
  PriceCarry pc = {0.0, 0.0, -1, 0};
  ObsJob job;
  // (a lambda like gte_backtest_kernel's step, for the same reason)
  auto run_a = [&](int k) {
    const int32_t now = signal_action(signal_byte(w, s.idx), p.P);
    const int32_t b = signal_byte(pw, s.idx);  // the period of the same row
    if (active && k + 1 < n_steps && (s.idx & 15) == 15 && s.idx + 1 < lim) fetch(s.idx + 1);
    double pv = 0.0;
    StepOut so = {};
    phase_a<MODE_STEP>(p, e, active, lane, job, nullptr, /*compact=*/false, &pv, &s, &now,
                       /*write_record=*/k == n_steps - 1, &pc, &so);
    if (active) {
      period_step(o, mine, per.B, b, a, p, e, s.step, s.pos, so.reward, so.flags);
      backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
    }
    if (active && k + 1 < n_steps && (s.dsi != pdsi || (s.idx & ~15) != pbase)) fetch(s.idx);
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    a.episode_seen = p.rec[e].episode;  // (this lane's own resets wrote it)
    store_stats(stats + e, a);
    period_close(mine, o);
  }
}

// gte_backtest_exit_kernel (gte_exits.hip: the exit state x and the rule R in registers, the memo of a decision
// already made, the update after every step — see there) with the period records
__global__ __launch_bounds__(256) void gte_period_exit_kernel(const Params p, const SignalTable* tables, const int S,
                                                              const int32_t* strategy, const ExitRules rules,
                                                              gte_backtest_stats* stats, const Periods per,
                                                              const int n_steps, const int epw) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  if (active) load_stats(stats + e, a);
  gte_period_stats* const mine = per.records + (int64_t)e * per.B;
  PeriodRegs o = {0.0, 0.0, 0, 0, 0, -1};
  const int64_t strat = active ? signal_strategy(p, strategy, S, e) : 0;
  gte_exit_state x = {};
  gte_exit_rule R = {};
  R.exit_position = -1;
  constexpr int32_t NO_MEMO = -2;
  int32_t memo = NO_MEMO;
  if (active) {
    load_exit_state(rules.state + e, x);
    R = load_exit_rule(rules.rules, rules.n_rules, rules.rule_of_env, strat, e, p.P);
    const int32_t episode = p.rec[e].episode;
    if (x.decided && episode == x.episode_seen && s.step == x.step_seen) memo = x.decided_action;
    else exit_sync(x, episode, s.step, s.pv, s.pos);  // steps and resets since the last decision
  }
  const int8_t* row = nullptr;  // this env's row of the table of dataset pdsi
  int32_t pdsi = -1;
  int32_t lim = 0, pbase = 0;
  int4_t w = {0, 0, 0, 0};
  PeriodRow prow = {nullptr, 0};
  int4_t pw = {-1, -1, -1, -1};
  auto fetch = [&](int32_t idx) {
    if (s.dsi != pdsi) {
      const SignalTable tb = tables[s.dsi];
      row = tb.base + strat * tb.stride;
      prow = per.rows[s.dsi];
      pdsi = s.dsi;
      lim = tb.stride > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)tb.stride;
    }
    pbase = idx & ~15;
    w = *reinterpret_cast<const int4_t*>(row + pbase);
    pw = period_piece(prow.base, prow.len, idx);
  };
  if (active) fetch(s.idx);
  PriceCarry pc = {0.0, 0.0, -1, 0};
  ObsJob job;
  // (a lambda like gte_backtest_kernel's step, for the same reason)
  auto run_a = [&](int k) {
    const double v_before = s.pv;
    const int32_t i_before = s.pos, step_before = s.step;
    const bool nr = s.needs_reset != 0;
    int32_t now = memo;
    if (k != 0 || memo == NO_MEMO) now = exit_decide(x, R, signal_byte(w, s.idx), v_before, i_before, nr, p.P);
    const int32_t b = signal_byte(pw, s.idx);  // the period of the same row
    if (active && k + 1 < n_steps && (s.idx & 15) == 15 && s.idx + 1 < lim) fetch(s.idx + 1);
    double pv = 0.0;
    StepOut so = {};
    phase_a<MODE_STEP>(p, e, active, lane, job, nullptr, /*compact=*/false, &pv, &s, &now,
                       /*write_record=*/k == n_steps - 1, &pc, &so);
    if (active) {
      const bool stepped = !(nr && (p.autoreset == GTE_AUTORESET_NEXT_STEP || s.step == step_before));
      if (stepped) {
        // (a transition into a same-step reset is overwritten by the reset row: only that is written)
        if (so.flags != 0 && p.autoreset == GTE_AUTORESET_SAME_STEP) exit_reset_row(x, pv);
        else exit_transition(x, v_before, i_before, pv, s.pos, 1);
      } else if (p.autoreset == GTE_AUTORESET_NEXT_STEP) {
        exit_reset_row(x, pv);
      }
      period_step(o, mine, per.B, b, a, p, e, s.step, s.pos, so.reward, so.flags);
      backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
    }
    if (active && k + 1 < n_steps && (s.dsi != pdsi || (s.idx & ~15) != pbase)) fetch(s.idx);
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    const int32_t episode = p.rec[e].episode;  // (this lane's own resets wrote it)
    a.episode_seen = episode;
    store_stats(stats + e, a);
    period_close(mine, o);
    x.v_seen = s.pv;
    x.i_seen = s.pos;
    x.episode_seen = episode;
    x.step_seen = s.step;
    x.decided = 0;  // the row the env stands on now has no decision yet
    store_exit_state(rules.state + e, x);
  }
}

// what launch_backtest_summary refuses (gte_backtest.hip), and a launch without the records, the rows or a B
static bool period_summary_refused(const Params& p, const gte_backtest_stats* stats, const Periods& per, int epw) {
  return p.log.rows != nullptr || (p.autoreset == GTE_AUTORESET_SAME_STEP && p.final_rec == nullptr) || epw < 1 ||
         epw > 64 || !stats || !per.records || !per.rows || per.B < 1 || per.B > GTE_MAX_PERIODS;
}

hipError_t launch_period_summary(const Params& p, const int32_t* actions, gte_backtest_stats* stats, const Periods& per,
                                 int n_steps, int epw, hipStream_t stream) {
  if (period_summary_refused(p, stats, per, epw) || !actions) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_period_backtest_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream,
                     p, actions, stats, per, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_period_signal_summary(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                                        gte_backtest_stats* stats, const Periods& per, int n_steps, int epw,
                                        hipStream_t stream) {
  if (period_summary_refused(p, stats, per, epw) || !tables || S < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_period_signal_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream, p,
                     tables, S, strategy, stats, per, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_period_exit_summary(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                                      const ExitRules& rules, gte_backtest_stats* stats, const Periods& per,
                                      int n_steps, int epw, hipStream_t stream) {
  if (period_summary_refused(p, stats, per, epw) || !tables || S < 1 || !rules.rules || rules.n_rules < 1 ||
      !rules.state)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_period_exit_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream, p,
                     tables, S, strategy, rules, stats, per, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_period_fold(const Params& p, gte_backtest_stats* stats, const Periods& per, hipStream_t stream) {
  if ((p.autoreset == GTE_AUTORESET_SAME_STEP && p.final_rec == nullptr) || !stats || !per.records || !per.rows ||
      per.B < 1 || per.B > GTE_MAX_PERIODS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_period_fold_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, per);
  return hipGetLastError();
}

}  // namespace gte
