// gte_trade_regs.h — the device helpers of the trade statistics (gte_track_trades, include/gte.h): the
// 128-byte trade record as 16-byte pieces and one step folded into it, next to backtest_step() of
// gte_backtest_regs.h.  Bodies only; the kernels are in gte_trades.hip.
#pragma once
#include "gte_backtest_regs.h"

namespace gte {

// The record as 16-byte pieces (the layout of gte_trade_stats, include/gte.h): four of doubles, one of the
// two 64-bit counters (each travels as the bits of a double), three of 32-bit counters; the last two words
// are reserved and written as zero.
static_assert(sizeof(gte_trade_stats) == 128 && offsetof(gte_trade_stats, last_valuation) == 16 &&
              offsetof(gte_trade_stats, best_trade) == 48 && offsetof(gte_trade_stats, exposure) == 64 &&
              offsetof(gte_trade_stats, closed) == 80 && offsetof(gte_trade_stats, reversals) == 96 &&
              offsetof(gte_trade_stats, loss_streak) == 112 && offsetof(gte_trade_stats, reserved) == 120,
              "gte_trade_stats: eight doubles, two 64-bit and ten 32-bit counters, padding to one 128-byte line");

__device__ __forceinline__ void load_trades(const gte_trade_stats* src, gte_trade_stats& t) {
  const double2_t* q = reinterpret_cast<const double2_t*>(src);
  const double2_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
  const int4_t c5 = reinterpret_cast<const int4_t*>(src)[5], c6 = reinterpret_cast<const int4_t*>(src)[6],
               c7 = reinterpret_cast<const int4_t*>(src)[7];
  t.open_value = d0[0]; t.open_position = d0[1];
  t.last_valuation = d1[0]; t.gross_profit = d1[1];
  t.gross_loss = d2[0]; t.ret_sq_sum = d2[1];
  t.best_trade = d3[0]; t.worst_trade = d3[1];
  t.exposure = __double_as_longlong(d4[0]); t.hold_sum = __double_as_longlong(d4[1]);
  t.closed = c5[0]; t.wins = c5[1]; t.losses = c5[2]; t.forced = c5[3];
  t.reversals = c6[0]; t.dropped = c6[1]; t.open_len = c6[2]; t.max_len = c6[3];
  t.loss_streak = c7[0]; t.max_loss_streak = c7[1];
}

__device__ __forceinline__ void store_trades(gte_trade_stats* dst, const gte_trade_stats& t) {
  double2_t* q = reinterpret_cast<double2_t*>(dst);
  const double2_t d0 = {t.open_value, t.open_position}, d1 = {t.last_valuation, t.gross_profit},
                  d2 = {t.gross_loss, t.ret_sq_sum}, d3 = {t.best_trade, t.worst_trade},
                  d4 = {__longlong_as_double(t.exposure), __longlong_as_double(t.hold_sum)};
  const int4_t c5 = {t.closed, t.wins, t.losses, t.forced};
  const int4_t c6 = {t.reversals, t.dropped, t.open_len, t.max_len};
  const int4_t c7 = {t.loss_streak, t.max_loss_streak, 0, 0};
  q[0] = d0; q[1] = d1; q[2] = d2; q[3] = d3; q[4] = d4;
  reinterpret_cast<int4_t*>(dst)[5] = c5;
  reinterpret_cast<int4_t*>(dst)[6] = c6;
  reinterpret_cast<int4_t*>(dst)[7] = c7;
}

// a cleared record of an env on valuation v with position value pos
__device__ __forceinline__ void trade_clear(gte_trade_stats& t, double v, double pos) {
  t = {};
  t.best_trade = -__builtin_inf();
  t.worst_trade = __builtin_inf();
  t.open_position = pos;
  t.open_value = v;
  t.last_valuation = v;
}

// A reset row of any kind (valuation v0, position value p0): a trade still open was cut off by a gte_reset
__device__ __forceinline__ void trade_reset_row(gte_trade_stats& t, double v0, double p0) {
  if (t.open_position != 0.0) t.dropped += 1;
  t.open_position = p0;
  t.open_value = v0;
  t.last_valuation = v0;
  t.open_len = 0;
}

// What trade_transition() and trade_step() tell a kernel that keeps more than the sums (the trade list,
// gte_trade_list.hip), each with the record as it stands directly BEFORE trade_close(): close(t, v, flat, flags)
// for a trade left to flat (closed at v) or reversed / resized (closed at t.last_valuation), forced(t, v, flags)
// for the close at an episode's end; open() where open_value is set by a position change; reset_row() at a reset
// row.  The kernels of gte_trades.hip pass none: every member is empty.
struct NoTradeSink {
  __device__ __forceinline__ void close(const gte_trade_stats&, double, bool, int32_t) const {}
  __device__ __forceinline__ void forced(const gte_trade_stats&, double, int32_t) const {}
  __device__ __forceinline__ void open() const {}
  __device__ __forceinline__ void reset_row() const {}
};

// the open trade closed at valuation vc (include/gte.h states the order): the one f64 division of a trade
__device__ __forceinline__ void trade_close(gte_trade_stats& t, double vc) {
  const double ret = vc / t.open_value - 1.0;
  t.closed += 1;
  t.hold_sum += t.open_len;
  if (t.open_len > t.max_len) t.max_len = t.open_len;
  if (ret > 0.0) {
    t.wins += 1;
    t.gross_profit += ret;
    t.ret_sq_sum += ret * ret;
    t.loss_streak = 0;
  } else if (ret < 0.0) {
    t.losses += 1;
    t.gross_loss += ret;
    t.ret_sq_sum += ret * ret;
    t.loss_streak += 1;
    if (t.loss_streak > t.max_loss_streak) t.max_loss_streak = t.loss_streak;
  }
  if (ret > t.best_trade) t.best_trade = ret;
  if (ret < t.worst_trade) t.worst_trade = ret;
}

// One transition of an episode that has not ended (include/gte.h states the order)
template <class Sink>
__device__ __forceinline__ void trade_transition(gte_trade_stats& t, double v, double pos, int32_t flags, Sink& sink) {
  if (pos != t.open_position) {
    if (t.open_position != 0.0) {
      // left to flat: at v, which is the valuation before less the fees of leaving; a reversal or a resize:
      // at the valuation before, the flip's fees count against the new trade
      const bool flat = pos == 0.0;
      sink.close(t, v, flat, flags);
      trade_close(t, flat ? v : t.last_valuation);
      t.reversals += flat ? 0 : 1;
    }
    t.open_position = pos;
    t.open_value = t.last_valuation;
    t.open_len = 0;
    sink.open();
  }
  if (t.open_position != 0.0) {
    t.open_len += 1;
    t.exposure += 1;
  }
  if (flags != 0 && t.open_position != 0.0) {
    sink.forced(t, v, flags);
    trade_close(t, v);
    t.forced += 1;
    t.open_position = 0.0;
  }
  t.last_valuation = v;
}

// One gte_step of env e into its trade record: the arguments of backtest_step() (the reward is not read: a
// trade is defined by valuations), called directly BEFORE it, so that a.ended is the env's needs_reset before
// the step and a.step_seen its _step before it.  Next-step resets, same-step resets (terminal valuation and
// position from the terminal record) and frozen steps are recognised exactly as backtest_step() does.
template <class Sink>
__device__ __forceinline__ void trade_step(gte_trade_stats& t, const gte_backtest_stats& a, const Params& p, int e,
                                           int32_t step_after, double pv_after, int32_t pos_after, double reward,
                                           int32_t flags, Sink& sink) {
  (void)reward;
  const bool nr = a.ended != 0;
  const bool stepped = !(nr && (p.autoreset == GTE_AUTORESET_NEXT_STEP || step_after == a.step_seen));
  if (stepped) {
    double v = pv_after;
    int32_t pos = pos_after;
    const bool reset_after = flags != 0 && p.autoreset == GTE_AUTORESET_SAME_STEP;
    if (reset_after) {
      const EnvRec* r = &p.final_rec[e];
      pos = reinterpret_cast<const int4*>(r)[0].z;
      v = reinterpret_cast<const double2*>(&r->asset)[2].x;
    }
    if (!nr) trade_transition(t, v, p.positions[pos], flags, sink);  // (after the episode's end: changes nothing)
    if (reset_after) {
      trade_reset_row(t, pv_after, p.positions[pos_after]);
      sink.reset_row();
    }
  } else if (p.autoreset == GTE_AUTORESET_NEXT_STEP) {
    trade_reset_row(t, pv_after, p.positions[pos_after]);
    sink.reset_row();
  }
}

}  // namespace gte
