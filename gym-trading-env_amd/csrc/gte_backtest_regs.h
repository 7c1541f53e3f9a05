// gte_backtest_regs.h — the device helpers the from-registers backtest kernels share across translation
// units (gte_backtest.hip, gte_exits.hip): the statistics record as 16-byte pieces, one step folded into
// it, and the signal-table lookup.  Bodies only; every kernel stays in its own .hip.
#pragma once
#include "gte_phase_a.h"

namespace gte {

// The 128-byte record as 16-byte pieces (the layout of gte_backtest_stats, include/gte.h): five of
// doubles (`steps` travels as the bits of one), one of the four counters, one of the bookkeeping
// pair; the last piece is reserved and stays as the allocation zeroed it.
static_assert(sizeof(gte_backtest_stats) == 128 && offsetof(gte_backtest_stats, trades) == 80 &&
              offsetof(gte_backtest_stats, episode_seen) == 96 && offsetof(gte_backtest_stats, reserved) == 104,
              "gte_backtest_stats: ten 8-byte fields, six counters, padding to one 128-byte line");

__device__ __forceinline__ void load_stats(const gte_backtest_stats* src, gte_backtest_stats& a) {
  const double2_t* q = reinterpret_cast<const double2_t*>(src);
  const double2_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
  const int4_t c = reinterpret_cast<const int4_t*>(src)[5];
  const int4_t b = reinterpret_cast<const int4_t*>(src)[6];
  a.steps = __double_as_longlong(d0[0]); a.reward_sum = d0[1];
  a.reward_sq_sum = d1[0]; a.peak = d1[1];
  a.max_drawdown = d2[0]; a.cur_return = d2[1];
  a.ep_return_sum = d3[0]; a.ep_return_sq_sum = d3[1];
  a.valuation_last = d4[0]; a.prev_position = d4[1];
  a.trades = c[0]; a.episodes = c[1]; a.terminations = c[2]; a.ended = c[3];
  a.episode_seen = b[0]; a.step_seen = b[1];
}

__device__ __forceinline__ void store_stats(gte_backtest_stats* dst, const gte_backtest_stats& a) {
  double2_t* q = reinterpret_cast<double2_t*>(dst);
  const double2_t d0 = {__longlong_as_double(a.steps), a.reward_sum}, d1 = {a.reward_sq_sum, a.peak},
                  d2 = {a.max_drawdown, a.cur_return}, d3 = {a.ep_return_sum, a.ep_return_sq_sum},
                  d4 = {a.valuation_last, a.prev_position};
  const int4_t c = {a.trades, a.episodes, a.terminations, a.ended};
  const int4_t b = {a.episode_seen, a.step_seen, 0, 0};
  q[0] = d0; q[1] = d1; q[2] = d2; q[3] = d3; q[4] = d4;
  reinterpret_cast<int4_t*>(dst)[5] = c;
  reinterpret_cast<int4_t*>(dst)[6] = b;
}

// A reset of any kind: the new episode's reset row (valuation v0, position value p0)
__device__ __forceinline__ void backtest_reset(gte_backtest_stats& a, double v0, double p0) {
  a.peak = v0;
  a.prev_position = p0;
  a.ended = 0;
}

// One transition (include/gte.h states the order)
__device__ __forceinline__ void backtest_transition(gte_backtest_stats& a, double v, double pos, double r, int32_t flags) {
  a.steps += 1;
  a.reward_sum += r;
  a.reward_sq_sum += r * r;
  if (pos != a.prev_position) a.trades += 1;
  a.prev_position = pos;
  if (v > a.peak) a.peak = v;
  const double d = 1.0 - v / a.peak;
  if (d > a.max_drawdown) a.max_drawdown = d;
  a.cur_return += r;
  if (flags != 0 && !a.ended) {
    a.episodes += 1;
    a.terminations += flags & 1;
    a.ep_return_sum += a.cur_return;
    a.ep_return_sq_sum += a.cur_return * a.cur_return;
    a.cur_return = 0.0;
  }
  if (flags != 0) a.ended = 1;
  a.valuation_last = v;
}

// One gte_step of env e into its statistics, from what the step left: the env's _step, valuation and
// position index after it, the step's f64 reward and flags (bit0 terminated, bit1 truncated) and, in
// same-step mode, the terminal record.  a.ended is the env's needs_reset before the step and
// a.step_seen its _step before it (backtest_begin, then this function keep them so).
__device__ __forceinline__ void backtest_step(gte_backtest_stats& a, const Params& p, int e, int32_t step_after,
                                     double pv_after, int32_t pos_after, double reward, int32_t flags) {
  const bool nr = a.ended != 0;
  // not a transition: the next-step auto-reset step; the frozen step of a finished env without
  // auto-reset (a step that advances the env increments _step, and nothing resets it in that mode)
  const bool stepped = !(nr && (p.autoreset == GTE_AUTORESET_NEXT_STEP || step_after == a.step_seen));
  if (stepped) {
    double v = pv_after;
    int32_t pos = pos_after;
    const bool reset_after = flags != 0 && p.autoreset == GTE_AUTORESET_SAME_STEP;
    if (reset_after) {
      // the env is already reset: its terminal valuation and position are in the terminal record,
      // read with the types store_state_at wrote them with
      const EnvRec* t = &p.final_rec[e];
      pos = reinterpret_cast<const int4*>(t)[0].z;
      v = reinterpret_cast<const double2*>(&t->asset)[2].x;
    }
    backtest_transition(a, v, p.positions[pos], reward, flags);
    if (reset_after) backtest_reset(a, pv_after, p.positions[pos_after]);
  } else if (p.autoreset == GTE_AUTORESET_NEXT_STEP) {
    backtest_reset(a, pv_after, p.positions[pos_after]);
  }
  a.step_seen = step_after;
}

// --- signal tables: the action looked up by the row the env stands on (include/gte.h, gte_bind_signals)

// strategy of env e: the caller's array, or (env_id_base + e) % S — what the unsharded run gives that env
__device__ __forceinline__ int64_t signal_strategy(const Params& p, const int32_t* strategy, int S, int e) {
  return strategy ? (int64_t)strategy[e] : (p.env_id_base + e) % S;
}

// a table value as the action of a step: outside [0, P) it means hold (None, environments.py:234)
__device__ __forceinline__ int32_t signal_action(int32_t v, int32_t P) {
  return (uint32_t)v < (uint32_t)P ? v : -1;
}

// byte idx & 15 of an aligned 16-byte piece, sign-extended: three selects and one bit-field extract
__device__ __forceinline__ int32_t signal_byte(const int4_t& w, int32_t idx) {
  const int j = idx & 15;
  const int32_t word = j < 8 ? (j < 4 ? w[0] : w[1]) : (j < 12 ? w[2] : w[3]);
  return (int32_t)(int8_t)(word >> ((j & 3) * 8));
}

}  // namespace gte
