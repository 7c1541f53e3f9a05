// gte_exit_regs.h — the device helpers of the exit rules (gte_bind_exit_rules, include/gte.h) that the exit
// kernels share across translation units (gte_exits.hip, gte_trades.hip): the exit state as 16-byte pieces,
// the rule of an env, and the state's update and decision.  Bodies only; every kernel stays in its own .hip.
#pragma once
#include "gte_backtest_regs.h"

namespace gte {

static_assert(sizeof(gte_exit_state) == 80 && offsetof(gte_exit_state, v_seen) == 16 &&
              offsetof(gte_exit_state, latched_raw) == 32 && offsetof(gte_exit_state, decided) == 48 &&
              offsetof(gte_exit_state, exits) == 64,
              "gte_exit_state: five 16-byte pieces");
static_assert(sizeof(gte_exit_rule) == 32 && offsetof(gte_exit_rule, max_hold) == 12 &&
              offsetof(gte_exit_rule, exit_position) == 16, "gte_exit_rule: 32 bytes");

__device__ __forceinline__ void load_exit_state(const gte_exit_state* src, gte_exit_state& x) {
  const double2_t d0 = reinterpret_cast<const double2_t*>(src)[0];
  const int4_t c1 = reinterpret_cast<const int4_t*>(src)[1], c2 = reinterpret_cast<const int4_t*>(src)[2],
               c3 = reinterpret_cast<const int4_t*>(src)[3], c4 = reinterpret_cast<const int4_t*>(src)[4];
  x.entry = d0[0]; x.peak = d0[1];
  x.v_seen = __longlong_as_double(((int64_t)c1[1] << 32) | (uint32_t)c1[0]);
  x.held = c1[2]; x.latched = c1[3];
  x.latched_raw = c2[0]; x.i_seen = c2[1]; x.episode_seen = c2[2]; x.step_seen = c2[3];
  x.decided = c3[0]; x.decided_action = c3[1];
  x.exits[0] = c4[0]; x.exits[1] = c4[1]; x.exits[2] = c4[2]; x.exits[3] = c4[3];
}

__device__ __forceinline__ void store_exit_state(gte_exit_state* dst, const gte_exit_state& x) {
  const double2_t d0 = {x.entry, x.peak};
  const int64_t vb = __double_as_longlong(x.v_seen);
  const int4_t c1 = {(int32_t)(uint32_t)vb, (int32_t)(vb >> 32), x.held, x.latched};
  const int4_t c2 = {x.latched_raw, x.i_seen, x.episode_seen, x.step_seen};
  const int4_t c3 = {x.decided, x.decided_action, 0, 0};
  const int4_t c4 = {x.exits[0], x.exits[1], x.exits[2], x.exits[3]};
  reinterpret_cast<double2_t*>(dst)[0] = d0;
  reinterpret_cast<int4_t*>(dst)[1] = c1;
  reinterpret_cast<int4_t*>(dst)[2] = c2;
  reinterpret_cast<int4_t*>(dst)[3] = c3;
  reinterpret_cast<int4_t*>(dst)[4] = c4;
}

// rule of env e (include/gte.h): the caller's map, or the env's strategy modulo the number of rules.
// The rules are caller-owned memory of which the ABI asks 4-byte alignment only: five 4-byte loads, no vector
__device__ __forceinline__ gte_exit_rule load_exit_rule(const gte_exit_rule* rules, int n_rules,
                                                        const int32_t* rule_of_env, int64_t strat, int e, int P) {
  const int64_t r = rule_of_env ? (int64_t)rule_of_env[e] : strat % n_rules;
  const int32_t* q = reinterpret_cast<const int32_t*>(rules + r);
  const int32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], b = q[4];
  gte_exit_rule R = {};
  R.stop_loss = __int_as_float(a0); R.take_profit = __int_as_float(a1); R.trailing = __int_as_float(a2);
  R.max_hold = a3;
  const int32_t xp = (int32_t)(int8_t)(b & 0xFF);
  R.exit_position = (uint32_t)xp < (uint32_t)P ? (int8_t)xp : (int8_t)-1;  // outside [0, P): the rule is off
  return R;
}

// a reset row of any kind (valuation v0)
__device__ __forceinline__ void exit_reset_row(gte_exit_state& x, double v0) {
  x.entry = v0;
  x.peak = v0;
  x.held = 0;
  x.latched = 0;
}

// d >= 1 steps seen as one transition from (v_prev, i_prev) to (v, i)
__device__ __forceinline__ void exit_transition(gte_exit_state& x, double v_prev, int32_t i_prev, double v,
                                                int32_t i, int32_t d) {
  if (i != i_prev) {
    x.entry = v_prev;
    x.peak = v_prev;
    x.held = d;
  } else {
    x.held = x.held > 0x7FFFFFFF - d ? 0x7FFFFFFF : x.held + d;
  }
  if (v > x.peak) x.peak = v;
}

// the state brought up to date with the row the env stands on: its reset count, _step, valuation, position
__device__ __forceinline__ void exit_sync(gte_exit_state& x, int32_t episode, int32_t step, double pv, int32_t pos) {
  if (episode != x.episode_seen) {
    exit_reset_row(x, pv);
  } else if (step != x.step_seen) {
    const int32_t d = step - x.step_seen;
    exit_transition(x, x.v_seen, x.i_seen, pv, pos, d < 1 ? 1 : d);
  }
  x.v_seen = pv;
  x.i_seen = pos;
  x.episode_seen = episode;
  x.step_seen = step;
}

// the action of the next step for an env on valuation v, position index i, with table byte raw
__device__ __forceinline__ int32_t exit_decide(gte_exit_state& x, const gte_exit_rule& R, int32_t raw, double v,
                                               int32_t i, bool needs_reset, int32_t P) {
  if (needs_reset) return -1;
  if (x.latched && raw != x.latched_raw) x.latched = 0;
  if (x.latched) return -1;
  const int32_t xp = R.exit_position;
  if (xp >= 0 && i != xp) {
    int k = -1;
    if (R.stop_loss > 0.0f && v <= x.entry * (1.0 - (double)R.stop_loss)) k = GTE_EXIT_STOP;
    else if (R.trailing > 0.0f && v <= x.peak * (1.0 - (double)R.trailing)) k = GTE_EXIT_TRAIL;
    else if (R.take_profit > 0.0f && v >= x.entry * (1.0 + (double)R.take_profit)) k = GTE_EXIT_TARGET;
    else if (R.max_hold > 0 && x.held >= R.max_hold) k = GTE_EXIT_TIME;
    if (k >= 0) {
      x.latched = 1;
      x.latched_raw = raw;
      x.exits[0] += k == GTE_EXIT_STOP;  // (no indexing by k: the counters stay in registers)
      x.exits[1] += k == GTE_EXIT_TRAIL;
      x.exits[2] += k == GTE_EXIT_TARGET;
      x.exits[3] += k == GTE_EXIT_TIME;
      return xp;
    }
  }
  return signal_action(raw, P);
}

}  // namespace gte
