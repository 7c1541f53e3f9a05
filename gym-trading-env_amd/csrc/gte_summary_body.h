// gte_summary_body.h — the ONE loop of the nine from-registers backtest kernels: an action source times a
// tracker.  A kernel is one call of summary_body() with its two policies, in the file it always had
// (gte_backtest.hip, gte_exits.hip, gte_trades.hip, gte_periods.hip hold the table of which is which;
// gte_trade_list.hip adds the three of gte_trades.hip once more, with TradeListTracker, its own tracker), so a
// unit still compiles alone and holds the code of its own tracker only.  ONE kernel is not:
// gte_backtest_exit_kernel (gte_exits.hip) is this body with ExitSource and NoTracker written out by hand,
// because it measured about 1 % slower as a call — a change to the step here is made there too.  fold_body(), at the end, is the ONE
// step of gte_backtest_fold_kernel and gte_trade_fold_kernel with the same trackers.  Bodies only, like the
// *_regs.h headers this one gathers.
//
// The body.  One lane per env, epw envs per wavefront, env = slot: the geometry of gte_rollout_state_kernel
// (gte_rollout.hip).  EnvRegs, PriceCarry and the statistics record stay in registers through all fused
// steps; the record is loaded once and stored once per launch; dynamic ring and the env's own return buffers
// are written through as gte_step would; no LDS, no barrier.  The units are compiled WITHOUT GTE_HOT_ONLY:
// in same-step mode phase A has already reset the env when it returns, and the terminal valuation is what
// it stored in the terminal record (p.final_rec) just before — the lane that wrote it reads it back in
// program order.  No terminal list: the step launch that follows builds it.
//
// Why a lambda.  The step is a lambda called from the loop, like gte_rollout_state_kernel's: written as a
// plain loop body the compiler kept the env's registers in scratch memory (tests: test_kernel_register_budget).
//
// The order inside a step: the source decides the action; the tracker takes what it needs from before the
// step; the speculative piece fetch; phase A; the source's update; the tracker's landed() and step;
// backtest_step(); the corrective piece fetch.  The tracker runs directly BEFORE backtest_step(), so that
// a.ended is the env's needs_reset before the step, a.step_seen its _step before it and a.prev_position its
// position before it.
//
// The piece cursor.  A source or tracker that reads a byte per market row (`pieces`) keeps the aligned
// 16-byte piece of its row that holds idx in registers and shifts the wanted byte out (signal_byte).  The
// row a step lands on is known only after the step, so the load is amortised and speculated: a plain step
// moves to idx + 1, so on the last row of a piece the next piece is asked for BEFORE phase A and arrives
// under it; only after a reset, a dataset switch or a step that did not advance (frozen env) is the piece
// wrong when the step returns, and then it is loaded again, waited for.  One 16-byte request per 16 steps
// and env where the actions source issues a 4-byte one per step.  pbase is the piece's first row, pdsi its
// dataset; a dataset switch also reloads the row descriptors (dataset()).  Reads stay inside the row: the
// piece at idx & ~15 ends before round_up(T, 16) <= stride, and the speculative one is only asked for while
// idx + 1 < limit() — the signal row's stride where the source has pieces (the period piece then moves on
// the cadence of the signal piece), else the period row's length.
//
// How resets are recognised, by the exit source as by backtest_step(): a same-step reset by the step's
// flags, a next-step one by needs_reset before the step, a frozen step by a _step that did not move.
//
// A source has: pieces, init(p, active, e, s), dataset(dsi), piece(idx), limit(), decide(p, s, active, e,
// k, n_steps) -> action, after(p, s, pv, so), store(e, s, episode).  A tracker has: pieces, init(active, e),
// dataset(dsi), piece(idx), limit(), before(idx, dsi) — the row and the dataset the env stands on before the
// step —, landed(idx) — the row it stands on after it —, step(a, p, e, step_after, pv, pos_after, reward, flags),
// store(e).  Both hold their own registers and have __forceinline__ members only.
#pragma once
#include "gte_exit_regs.h"
#include "gte_period_regs.h"
#include "gte_trade_regs.h"

namespace gte {

// --- sources

// the [K][N] actions: the next step's action is loaded a step ahead, so its latency is under phase A
struct ActionSource {
  static constexpr bool pieces = false;
  const int32_t* actions;
  int32_t act = -1;
  __device__ __forceinline__ explicit ActionSource(const int32_t* actions_) : actions(actions_) {}
  __device__ __forceinline__ void init(const Params&, bool active, int e, const EnvRegs&) {
    if (active) act = actions[e];
  }
  __device__ __forceinline__ void dataset(int32_t) {}
  __device__ __forceinline__ void piece(int32_t) {}
  __device__ __forceinline__ int32_t limit() const { return 0; }
  __device__ __forceinline__ int32_t decide(const Params& p, const EnvRegs&, bool active, int e, int k, int n_steps) {
    const int32_t now = act;
    if (active && k + 1 < n_steps) act = actions[(int64_t)(k + 1) * p.N + e];
    return now;
  }
  __device__ __forceinline__ void after(const Params&, const EnvRegs&, double, const StepOut&) {}
  __device__ __forceinline__ void store(int, const EnvRegs&, int32_t) {}
};

// the env's signal table (gte_bind_signals) at the row it stands on: w is the piece of row `row`, the
// strategy's row of the table of the cursor's dataset
struct SignalSource {
  static constexpr bool pieces = true;
  const SignalTable* tables;
  const int32_t* strategy;
  int S;
  int64_t strat = 0;
  const int8_t* row = nullptr;
  int32_t lim = 0;
  int4_t w = {0, 0, 0, 0};
  __device__ __forceinline__ SignalSource(const SignalTable* tables_, int S_, const int32_t* strategy_)
      : tables(tables_), strategy(strategy_), S(S_) {}
  __device__ __forceinline__ void init(const Params& p, bool active, int e, const EnvRegs&) {
    strat = active ? signal_strategy(p, strategy, S, e) : 0;
  }
  __device__ __forceinline__ void dataset(int32_t dsi) {
    const SignalTable t = tables[dsi];
    row = t.base + strat * t.stride;
    lim = t.stride > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)t.stride;
  }
  __device__ __forceinline__ void piece(int32_t idx) { w = *reinterpret_cast<const int4_t*>(row + (idx & ~15)); }
  __device__ __forceinline__ int32_t limit() const { return lim; }
  __device__ __forceinline__ int32_t decide(const Params& p, const EnvRegs& s, bool, int, int, int) {
    return signal_action(signal_byte(w, s.idx), p.P);
  }
  __device__ __forceinline__ void after(const Params&, const EnvRegs&, double, const StepOut&) {}
  __device__ __forceinline__ void store(int, const EnvRegs&, int32_t) {}
};

// ... with exit rules bound (gte_bind_exit_rules): the exit state x and the rule R of the lane's env in
// registers, loaded once and stored once per launch; a step issues no memory request SignalSource does not
// issue.  Before a step the lane decides from x, the table byte and the env's registers; after it, it
// updates x from what the step left in them.  v_seen / i_seen / step_seen are the env's own registers
// during the launch and are written out with the state at the end.
struct ExitSource : SignalSource {
  static constexpr int32_t NO_MEMO = -2;
  const ExitRules rules;
  gte_exit_state x = {};
  gte_exit_rule R = {};
  int32_t memo = NO_MEMO;
  double v_before = 0.0;  // the env before the step
  int32_t i_before = 0, step_before = 0;
  bool nr = false;
  __device__ __forceinline__ ExitSource(const SignalTable* tables_, int S_, const int32_t* strategy_,
                                        const ExitRules& rules_)
      : SignalSource(tables_, S_, strategy_), rules(rules_) {}
  __device__ __forceinline__ void init(const Params& p, bool active, int e, const EnvRegs& s) {
    SignalSource::init(p, active, e, s);
    R.exit_position = -1;
    if (!active) return;
    load_exit_state(rules.state + e, x);
    R = load_exit_rule(rules.rules, rules.n_rules, rules.rule_of_env, strat, e, p.P);
    const int32_t episode = p.rec[e].episode;
    // the row the env stands on may have its decision already (a gte_signal_actions call before this one):
    // the first step then takes that memo and decides nothing, as a second lookup would
    if (x.decided && episode == x.episode_seen && s.step == x.step_seen) memo = x.decided_action;
    else exit_sync(x, episode, s.step, s.pv, s.pos);  // steps and resets since the last decision
  }
  __device__ __forceinline__ int32_t decide(const Params& p, const EnvRegs& s, bool, int, int k, int) {
    v_before = s.pv;
    i_before = s.pos;
    step_before = s.step;
    nr = s.needs_reset != 0;
    if (k == 0 && memo != NO_MEMO) return memo;
    return exit_decide(x, R, signal_byte(w, s.idx), v_before, i_before, nr, p.P);
  }
  __device__ __forceinline__ void after(const Params& p, const EnvRegs& s, double pv, const StepOut& so) {
    const bool stepped = !(nr && (p.autoreset == GTE_AUTORESET_NEXT_STEP || s.step == step_before));
    if (stepped) {
      // (a transition into a same-step reset is overwritten by the reset row: only that is written)
      if (so.flags != 0 && p.autoreset == GTE_AUTORESET_SAME_STEP) exit_reset_row(x, pv);
      else exit_transition(x, v_before, i_before, pv, s.pos, 1);
    } else if (p.autoreset == GTE_AUTORESET_NEXT_STEP) {
      exit_reset_row(x, pv);
    }
  }
  __device__ __forceinline__ void store(int e, const EnvRegs& s, int32_t episode) {
    x.v_seen = s.pv;
    x.i_seen = s.pos;
    x.episode_seen = episode;
    x.step_seen = s.step;
    x.decided = 0;  // the row the env stands on now has no decision yet
    store_exit_state(rules.state + e, x);
  }
};

// --- trackers

struct NoTracker {
  static constexpr bool pieces = false;
  __device__ __forceinline__ void init(bool, int) {}
  __device__ __forceinline__ void dataset(int32_t) {}
  __device__ __forceinline__ void piece(int32_t) {}
  __device__ __forceinline__ int32_t limit() const { return 0; }
  __device__ __forceinline__ void before(int32_t, int32_t) {}
  __device__ __forceinline__ void landed(int32_t) {}
  __device__ __forceinline__ void step(const gte_backtest_stats&, const Params&, int, int32_t, double, int32_t, double,
                                       int32_t) {}
  __device__ __forceinline__ void store(int) {}
};

// the env's trade record (gte_track_trades) in registers as well: loaded once and stored once per launch, as
// 16-byte pieces; a step issues no memory request the untracked kernel does not issue
struct TradeTracker {
  static constexpr bool pieces = false;
  gte_trade_stats* trades;
  gte_trade_stats t = {};
  __device__ __forceinline__ explicit TradeTracker(gte_trade_stats* trades_) : trades(trades_) {}
  __device__ __forceinline__ void init(bool active, int e) {
    if (active) load_trades(trades + e, t);
  }
  __device__ __forceinline__ void dataset(int32_t) {}
  __device__ __forceinline__ void piece(int32_t) {}
  __device__ __forceinline__ int32_t limit() const { return 0; }
  __device__ __forceinline__ void before(int32_t, int32_t) {}
  __device__ __forceinline__ void landed(int32_t) {}
  __device__ __forceinline__ void step(const gte_backtest_stats& a, const Params& p, int e, int32_t step_after,
                                       double pv, int32_t pos_after, double reward, int32_t flags) {
    NoTradeSink none;
    trade_step(t, a, p, e, step_after, pv, pos_after, reward, flags, none);
  }
  __device__ __forceinline__ void store(int e) { store_trades(trades + e, t); }
};

// the record of the period the env is in (gte_track_periods) in registers (PeriodRegs): a lane stores its open
// record (two 16-byte pieces) and loads the next when its env's row enters another period, and stores it at
// the launch's end.  pw is the piece of the dataset's period row; b the period of the row the env stands on
// before the step.
struct PeriodTracker {
  static constexpr bool pieces = true;
  const Periods per;
  gte_period_stats* mine = nullptr;
  PeriodRegs o = {0.0, 0.0, 0, 0, 0, -1};
  PeriodRow prow = {nullptr, 0};
  int4_t pw = {-1, -1, -1, -1};
  int32_t b = -1;
  __device__ __forceinline__ explicit PeriodTracker(const Periods& per_) : per(per_) {}
  __device__ __forceinline__ void init(bool, int e) { mine = per.records + (int64_t)e * per.B; }
  __device__ __forceinline__ void dataset(int32_t dsi) { prow = per.rows[dsi]; }
  __device__ __forceinline__ void piece(int32_t idx) { pw = period_piece(prow.base, prow.len, idx); }
  __device__ __forceinline__ int32_t limit() const { return prow.len; }
  __device__ __forceinline__ void before(int32_t idx, int32_t) { b = signal_byte(pw, idx); }
  __device__ __forceinline__ void landed(int32_t) {}
  __device__ __forceinline__ void step(const gte_backtest_stats& a, const Params& p, int e, int32_t step_after, double,
                                       int32_t pos_after, double reward, int32_t flags) {
    period_step(o, mine, per.B, b, a, p, e, step_after, pos_after, reward, flags);
  }
  __device__ __forceinline__ void store(int) { period_close(mine, o); }
};

// --- the body

template <class Src, class Trk>
__device__ __forceinline__ void summary_body(const Params& p, gte_backtest_stats* stats, Src src, Trk trk,
                                             const int n_steps, const int epw) {
  constexpr bool pieces = Src::pieces || Trk::pieces;
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  if (active) load_stats(stats + e, a);
  trk.init(active, e);
  src.init(p, active, e, s);
  int32_t pdsi = -1, pbase = 0;
  auto fetch = [&](int32_t idx) {
    if (s.dsi != pdsi) {
      src.dataset(s.dsi);
      trk.dataset(s.dsi);
      pdsi = s.dsi;
    }
    pbase = idx & ~15;
    src.piece(idx);
    trk.piece(idx);
  };
  if constexpr (pieces) {
    if (active) fetch(s.idx);
  }
  PriceCarry pc = {0.0, 0.0, -1, 0};
  ObsJob job;
  auto run_a = [&](int k) {
    const int32_t now = src.decide(p, s, active, e, k, n_steps);
    trk.before(s.idx, s.dsi);
    if constexpr (pieces) {
      const int32_t lim = Src::pieces ? src.limit() : trk.limit();
      if (active && k + 1 < n_steps && (s.idx & 15) == 15 && s.idx + 1 < lim) fetch(s.idx + 1);
    }
    double pv = 0.0;
    StepOut so = {};
    phase_a<MODE_STEP>(p, e, active, lane, job, nullptr, /*compact=*/false, &pv, &s, &now,
                       /*write_record=*/k == n_steps - 1, &pc, &so);
    if (active) {
      src.after(p, s, pv, so);
      trk.landed(s.idx);
      trk.step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
      backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
    }
    if constexpr (pieces) {
      if (active && k + 1 < n_steps && (s.dsi != pdsi || (s.idx & ~15) != pbase)) fetch(s.idx);
    }
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    const int32_t episode = p.rec[e].episode;  // (this lane's own resets wrote it)
    a.episode_seen = episode;
    store_stats(stats + e, a);
    trk.store(e);
    src.store(e, s, episode);
  }
}

// --- the one-step kernel beside it, one lane per env, with the same trackers

// ONE step into the records from what an ordinary step launch left behind (reward64, flags, the env record, the
// terminal record): the last step of a call, and every step where gte_rollout itself goes step by step
template <class Trk>
__device__ __forceinline__ void fold_body(const Params& p, gte_backtest_stats* stats, Trk trk) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  gte_backtest_stats a;
  load_stats(stats + e, a);
  trk.init(true, e);
  const EnvRec* r = &p.rec[e];
  const int32_t flags = (p.terminated[e] ? 1 : 0) | (p.truncated[e] ? 2 : 0);
  trk.step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  backtest_step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
  trk.store(e);
}

}  // namespace gte
