// gte_trades.hip — trade statistics (gte_track_trades, include/gte.h): the backtest kernels with a second
// 128-byte record per env, the round-trip trade statistics, reduced while they step.  Own translation unit:
// nothing here can perturb the code generated for the kernels of gte_backtest.hip and gte_exits.hip, which
// run whenever tracking is off.
//
//   gte_trade_backtest_kernel   gte_backtest_kernel         (gte_backtest.hip) ...
//   gte_trade_signal_kernel     gte_backtest_signal_kernel  (gte_backtest.hip) ...
//   gte_trade_exit_kernel       gte_backtest_exit_kernel    (gte_exits.hip)    ... with the env's trade record in
//                               registers as well — same geometry, same lambda structure, same steps, same
//                               handling of the statistics record and the exit state (see there).  The trade
//                               record is loaded once and stored once per launch, as 16-byte pieces; a step
//                               issues no memory request its model does not issue.
//   gte_trade_fold_kernel       gte_backtest_fold_kernel: ONE ordinary step into BOTH records.
//   gte_trade_begin_kernel      gte_backtest_begin_kernel: clears both records, or applies the reset row of a
//                               gte_reset between two calls to both.
//
// Every path runs trade_step() directly before backtest_step() on the same values, so all of them give the
// same two records bit for bit (tests/test_gpu_trades.py), and the statistics record, the env state and the
// exit state are those of the kernels without the trade record.  Compiled WITHOUT GTE_HOT_ONLY like
// gte_backtest.hip.
#include "gte_exit_regs.h"
#include "gte_trade_regs.h"

namespace gte {

__global__ __launch_bounds__(256) void gte_trade_backtest_kernel(const Params p, const int32_t* actions,
                                                                 gte_backtest_stats* stats, gte_trade_stats* trades,
                                                                 const int n_steps, const int epw) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  gte_trade_stats t = {};
  if (active) {
    load_stats(stats + e, a);
    load_trades(trades + e, t);
  }
  int32_t act = active ? actions[e] : -1;
  PriceCarry pc = {0.0, 0.0, -1, 0};
  ObsJob job;
  // (a lambda like gte_backtest_kernel's step, for the same reason)
  auto run_a = [&](int k) {
    const int32_t now = act;
    if (active && k + 1 < n_steps) act = actions[(int64_t)(k + 1) * p.N + e];
    double pv = 0.0;
    StepOut so = {};
    phase_a<MODE_STEP>(p, e, active, lane, job, nullptr, /*compact=*/false, &pv, &s, &now,
                       /*write_record=*/k == n_steps - 1, &pc, &so);
    if (active) {
      trade_step(t, a, p, e, s.step, pv, s.pos, so.reward, so.flags);
      backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
    }
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    a.episode_seen = p.rec[e].episode;  // (this lane's own resets wrote it)
    store_stats(stats + e, a);
    store_trades(trades + e, t);
  }
}

__global__ __launch_bounds__(256) void gte_trade_fold_kernel(const Params p, gte_backtest_stats* stats,
                                                             gte_trade_stats* trades) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  gte_backtest_stats a;
  gte_trade_stats t;
  load_stats(stats + e, a);
  load_trades(trades + e, t);
  const EnvRec* r = &p.rec[e];
  const int32_t flags = (p.terminated[e] ? 1 : 0) | (p.truncated[e] ? 2 : 0);
  trade_step(t, a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  backtest_step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
  store_trades(trades + e, t);
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

// gte_backtest_signal_kernel (gte_backtest.hip: geometry, piece fetch and its bounds, record handling — see
// there) with the trade record
__global__ __launch_bounds__(256) void gte_trade_signal_kernel(const Params p, const SignalTable* tables, const int S,
                                                               const int32_t* strategy, gte_backtest_stats* stats,
                                                               gte_trade_stats* trades, const int n_steps,
                                                               const int epw) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  gte_trade_stats t = {};
  if (active) {
    load_stats(stats + e, a);
    load_trades(trades + e, t);
  }
  const int64_t strat = active ? signal_strategy(p, strategy, S, e) : 0;
  const int8_t* row = nullptr;  // this env's row of the table of dataset pdsi
  int32_t pdsi = -1;
  int32_t lim = 0, pbase = 0;
  int4_t w = {0, 0, 0, 0};
  auto fetch = [&](int32_t idx) {
    if (s.dsi != pdsi) {
      const SignalTable tb = tables[s.dsi];
      row = tb.base + strat * tb.stride;
      pdsi = s.dsi;
      lim = tb.stride > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)tb.stride;
    }
    pbase = idx & ~15;
    w = *reinterpret_cast<const int4_t*>(row + pbase);
  };
  if (active) fetch(s.idx);
  PriceCarry pc = {0.0, 0.0, -1, 0};
  ObsJob job;
  // (a lambda like gte_backtest_kernel's step, for the same reason)
  auto run_a = [&](int k) {
    const int32_t now = signal_action(signal_byte(w, s.idx), p.P);
    if (active && k + 1 < n_steps && (s.idx & 15) == 15 && s.idx + 1 < lim) fetch(s.idx + 1);
    double pv = 0.0;
    StepOut so = {};
    phase_a<MODE_STEP>(p, e, active, lane, job, nullptr, /*compact=*/false, &pv, &s, &now,
                       /*write_record=*/k == n_steps - 1, &pc, &so);
    if (active) {
      trade_step(t, a, p, e, s.step, pv, s.pos, so.reward, so.flags);
      backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
    }
    if (active && k + 1 < n_steps && (s.dsi != pdsi || (s.idx & ~15) != pbase)) fetch(s.idx);
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    a.episode_seen = p.rec[e].episode;  // (this lane's own resets wrote it)
    store_stats(stats + e, a);
    store_trades(trades + e, t);
  }
}

// gte_backtest_exit_kernel (gte_exits.hip: the exit state x and the rule R in registers, the memo of a decision
// already made, the update after every step — see there) with the trade record
__global__ __launch_bounds__(256) void gte_trade_exit_kernel(const Params p, const SignalTable* tables, const int S,
                                                             const int32_t* strategy, const ExitRules rules,
                                                             gte_backtest_stats* stats, gte_trade_stats* trades,
                                                             const int n_steps, const int epw) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  gte_trade_stats t = {};
  if (active) {
    load_stats(stats + e, a);
    load_trades(trades + e, t);
  }
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
  auto fetch = [&](int32_t idx) {
    if (s.dsi != pdsi) {
      const SignalTable tb = tables[s.dsi];
      row = tb.base + strat * tb.stride;
      pdsi = s.dsi;
      lim = tb.stride > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)tb.stride;
    }
    pbase = idx & ~15;
    w = *reinterpret_cast<const int4_t*>(row + pbase);
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
      trade_step(t, a, p, e, s.step, pv, s.pos, so.reward, so.flags);
      backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
    }
    if (active && k + 1 < n_steps && (s.dsi != pdsi || (s.idx & ~15) != pbase)) fetch(s.idx);
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    const int32_t episode = p.rec[e].episode;  // (this lane's own resets wrote it)
    a.episode_seen = episode;
    store_stats(stats + e, a);
    store_trades(trades + e, t);
    x.v_seen = s.pv;
    x.i_seen = s.pos;
    x.episode_seen = episode;
    x.step_seen = s.step;
    x.decided = 0;  // the row the env stands on now has no decision yet
    store_exit_state(rules.state + e, x);
  }
}

hipError_t launch_trade_begin(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades, int clear,
                              hipStream_t stream) {
  if (!stats || !trades) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_begin_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, trades, clear);
  return hipGetLastError();
}

// what launch_backtest_summary refuses (gte_backtest.hip), and a launch without both records
static bool trade_summary_refused(const Params& p, const gte_backtest_stats* stats, const gte_trade_stats* trades,
                                  int epw) {
  return p.log.rows != nullptr || (p.autoreset == GTE_AUTORESET_SAME_STEP && p.final_rec == nullptr) || epw < 1 ||
         epw > 64 || !stats || !trades;
}

hipError_t launch_trade_summary(const Params& p, const int32_t* actions, gte_backtest_stats* stats,
                                gte_trade_stats* trades, int n_steps, int epw, hipStream_t stream) {
  if (trade_summary_refused(p, stats, trades, epw) || !actions) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_backtest_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream,
                     p, actions, stats, trades, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_trade_signal_summary(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                                       gte_backtest_stats* stats, gte_trade_stats* trades, int n_steps, int epw,
                                       hipStream_t stream) {
  if (trade_summary_refused(p, stats, trades, epw) || !tables || S < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_signal_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream, p,
                     tables, S, strategy, stats, trades, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_trade_exit_summary(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                                     const ExitRules& rules, gte_backtest_stats* stats, gte_trade_stats* trades,
                                     int n_steps, int epw, hipStream_t stream) {
  if (trade_summary_refused(p, stats, trades, epw) || !tables || S < 1 || !rules.rules || rules.n_rules < 1 ||
      !rules.state)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_exit_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream, p,
                     tables, S, strategy, rules, stats, trades, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_trade_fold(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades,
                             hipStream_t stream) {
  if ((p.autoreset == GTE_AUTORESET_SAME_STEP && p.final_rec == nullptr) || !stats || !trades)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_fold_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, trades);
  return hipGetLastError();
}

}  // namespace gte
