// gte_exits.hip — exit rules (gte_bind_exit_rules, include/gte.h): stop-loss, trailing stop, take-profit
// and time exits decided from the env's own path, next to the signal-table lookup.  Own translation
// unit: nothing here can perturb the code generated for the kernels of gte_backtest.hip.
//
//   gte_backtest_exit_kernel    the third row of the table in gte_backtest.hip without a tracker: what
//                               summary_body (gte_summary_body.h) does with ExitSource — the signal lookup with
//                               the env's exit state and rule in registers — kept HAND-WRITTEN here, the one
//                               exception to that header (the comment at the kernel says why).
//   gte_exit_actions_kernel     gte_signal_actions_kernel with rules bound: brings the state up to date
//                               from the env record, decides, and keeps the decision as a memo so that a
//                               second call before the env has stepped changes nothing.
//   gte_exit_init_kernel        the state a bind leaves: the next decision sees a reset row.
//
// Both paths run exit_sync() / exit_decide() on the same values, so they give the same exit state and
// actions bit for bit (tests/test_gpu_exits.py).  Compiled WITHOUT GTE_HOT_ONLY like gte_backtest.hip.
#include "gte_summary_body.h"

namespace gte {

__global__ __launch_bounds__(256) void gte_exit_init_kernel(gte_exit_state* state, const int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  gte_exit_state x = {};
  x.episode_seen = -1;  // no env has this reset count: the first decision sees a reset row
  store_exit_state(state + e, x);
}

__global__ __launch_bounds__(256) void gte_exit_actions_kernel(const Params p, const SignalTable* tables,
                                                               const int S, const int32_t* strategy,
                                                               const ExitRules rules, int32_t* actions) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  const EnvRec* r = &p.rec[e];
  const int4_t a = reinterpret_cast<const int4_t*>(r)[0];  // idx, step, pos, dsi
  const int4_t b = reinterpret_cast<const int4_t*>(r)[4];  // start, episode, needs_reset, eps_on_ds
  const double pv = r->pv;
  gte_exit_state x;
  load_exit_state(rules.state + e, x);
  if (x.decided && b[1] == x.episode_seen && a[1] == x.step_seen) {
    actions[e] = x.decided_action;  // decided already for this row: nothing changes
    return;
  }
  const int64_t strat = signal_strategy(p, strategy, S, e);
  const SignalTable t = tables[a[3]];
  const int32_t raw = t.base[strat * t.stride + a[0]];
  const gte_exit_rule R = load_exit_rule(rules.rules, rules.n_rules, rules.rule_of_env, strat, e, p.P);
  exit_sync(x, b[1], a[1], pv, a[2]);
  const int32_t act = exit_decide(x, R, raw, pv, a[2], b[2] != 0, p.P);
  x.decided = 1;
  x.decided_action = act;
  store_exit_state(rules.state + e, x);
  actions[e] = act;
}

// THE EXCEPTION to gte_summary_body.h: summary_body(p, stats, ExitSource(tables, S, strategy, rules), NoTracker(),
// n_steps, epw) written out by hand, as it was before that header.  Through the shared body this one kernel
// measured about 1 % slower than this text ("One body for the nine fused backtest kernels";
// profiles/summary_body_bench.log) and the cause was not found in its listing, so the text stays until it is.
// It must be kept in step with summary_body() and ExitSource by hand: geometry, piece fetch and its bounds, the
// memo, the order inside a step and how resets are recognised are explained there.
__global__ __launch_bounds__(256) void gte_backtest_exit_kernel(const Params p, const SignalTable* tables,
                                                                const int S, const int32_t* strategy,
                                                                const ExitRules rules, gte_backtest_stats* stats,
                                                                const int n_steps, const int epw) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  if (active) load_stats(stats + e, a);
  const int64_t strat = active ? signal_strategy(p, strategy, S, e) : 0;
  gte_exit_state x = {};
  gte_exit_rule R = {};
  R.exit_position = -1;
  // the row the env stands on may have its decision already (a gte_signal_actions call before this one): the
  // first step then takes that memo and decides nothing, as a second lookup would
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
      const SignalTable t = tables[s.dsi];
      row = t.base + strat * t.stride;
      pdsi = s.dsi;
      lim = t.stride > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)t.stride;
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
      backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
    }
    if (active && k + 1 < n_steps && (s.dsi != pdsi || (s.idx & ~15) != pbase)) fetch(s.idx);
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    const int32_t episode = p.rec[e].episode;  // (this lane's own resets wrote it)
    a.episode_seen = episode;
    store_stats(stats + e, a);
    x.v_seen = s.pv;
    x.i_seen = s.pos;
    x.episode_seen = episode;
    x.step_seen = s.step;
    x.decided = 0;  // the row the env stands on now has no decision yet
    store_exit_state(rules.state + e, x);
  }
}

hipError_t launch_exit_init(gte_exit_state* state, int n, hipStream_t stream) {
  if (!state || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_exit_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, state, n);
  return hipGetLastError();
}

hipError_t launch_exit_actions(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                               const ExitRules& rules, int32_t* actions, hipStream_t stream) {
  if (!tables_usable(tables, S) || !actions || !exit_rules_usable(rules)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_exit_actions_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, tables, S,
                     strategy, rules, actions);
  return hipGetLastError();
}

hipError_t launch_exit_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats, int n_steps,
                               int epw, hipStream_t stream) {
  if (summary_refused(p, src, epw) || src.actions || !src.rules) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_backtest_exit_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream,
                     p, src.tables, src.S, src.strategy, *src.rules, stats, n_steps, epw);
  return hipGetLastError();
}

}  // namespace gte
