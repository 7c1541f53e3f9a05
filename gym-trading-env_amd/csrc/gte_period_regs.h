// gte_period_regs.h — the device helpers of the period statistics (gte_track_periods, include/gte.h): the
// 32-byte record of ONE (env, period) as two 16-byte pieces, the open period's record in registers, and one step
// folded into it, next to backtest_step() of gte_backtest_regs.h.  Bodies only; the kernels are in
// gte_periods.hip.
#pragma once
#include "gte_backtest_regs.h"

namespace gte {

static_assert(sizeof(gte_period_stats) == 32 && offsetof(gte_period_stats, steps) == 16 &&
              offsetof(gte_period_stats, trades) == 24 && offsetof(gte_period_stats, episodes) == 28,
              "gte_period_stats: two doubles, one 64-bit and two 32-bit counters");

// The record a lane has open: the fields of gte_period_stats and which period of its env they belong to
// (-1: none yet).  Eleven 32-bit registers.
struct PeriodRegs {
  double reward_sum, reward_sq_sum;
  long long steps;
  int32_t trades, episodes, open;
};

// (the counters travel as the bits of doubles: `steps`, and the pair trades | episodes << 32)
__device__ __forceinline__ void load_period(const gte_period_stats* src, PeriodRegs& o) {
  const double2_t* q = reinterpret_cast<const double2_t*>(src);
  const double2_t d0 = q[0], d1 = q[1];
  o.reward_sum = d0[0]; o.reward_sq_sum = d0[1];
  o.steps = __double_as_longlong(d1[0]);
  const long long te = __double_as_longlong(d1[1]);
  o.trades = (int32_t)te; o.episodes = (int32_t)(te >> 32);
}

__device__ __forceinline__ void store_period(gte_period_stats* dst, const PeriodRegs& o) {
  double2_t* q = reinterpret_cast<double2_t*>(dst);
  const long long te = (long long)(uint32_t)o.trades | ((long long)o.episodes << 32);
  const double2_t d0 = {o.reward_sum, o.reward_sq_sum}, d1 = {__longlong_as_double(o.steps), __longlong_as_double(te)};
  q[0] = d0; q[1] = d1;
}

// the open record back to memory (a launch's end)
__device__ __forceinline__ void period_close(gte_period_stats* mine, const PeriodRegs& o) {
  if (o.open >= 0) store_period(mine + o.open, o);
}

// the aligned 16-byte piece around row idx of a period row of `len` bytes (a multiple of 16); outside it: all -1
__device__ __forceinline__ int4_t period_piece(const int8_t* row, int32_t len, int32_t idx) {
  const int4_t none = {-1, -1, -1, -1};
  return (uint32_t)idx < (uint32_t)len ? *reinterpret_cast<const int4_t*>(row + (idx & ~15)) : none;
}

// One gte_step of env e into its period records (`mine`: the B records of env e): the arguments of
// backtest_step() and b, the period byte of the row the env stood on BEFORE the step; called directly BEFORE
// backtest_step(), so that a.ended is the env's needs_reset before the step, a.step_seen its _step before it and
// a.prev_position the position value before it.  What is a transition is recognised exactly as backtest_step()
// does.  A byte outside [0, B) counts nowhere, so no byte indexes outside the records.  On entering a period
// the lane stores the record it had open and LOADS the new one: its sums go on from the stored values.
__device__ __forceinline__ void period_step(PeriodRegs& o, gte_period_stats* mine, int32_t B, int32_t b,
                                            const gte_backtest_stats& a, const Params& p, int e, int32_t step_after,
                                            int32_t pos_after, double reward, int32_t flags) {
  const bool nr = a.ended != 0;
  const bool stepped = !(nr && (p.autoreset == GTE_AUTORESET_NEXT_STEP || step_after == a.step_seen));
  if (!stepped || (uint32_t)b >= (uint32_t)B) return;
  if (b != o.open) {
    if (o.open >= 0) store_period(mine + o.open, o);
    load_period(mine + b, o);
    o.open = b;
  }
  int32_t pos = pos_after;
  if (flags != 0 && p.autoreset == GTE_AUTORESET_SAME_STEP)  // the env is already reset: its terminal position
    pos = reinterpret_cast<const int4*>(&p.final_rec[e])[0].z;
  o.steps += 1;
  o.reward_sum += reward;
  o.reward_sq_sum += reward * reward;
  if (p.positions[pos] != a.prev_position) o.trades += 1;
  if (flags != 0 && !nr) o.episodes += 1;
}

}  // namespace gte
