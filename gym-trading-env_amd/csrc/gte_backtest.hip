// gte_backtest.hip — backtest summaries: K consecutive TradingEnv.step calls (environments.py:233-272)
// that leave, per env, a record of running statistics (gte_backtest_stats, include/gte.h: return
// sums, drawdown, trades, episode ends) instead of [K, N] rows of per-step results.  Own translation
// unit: nothing here can perturb the code generated for the step and rollout kernels.
//
//   gte_backtest_kernel        the state-only rollout (gte_rollout_state_kernel) with the record in
//                              registers as well: one lane per env, EnvRegs and PriceCarry carried
//                              through all fused steps, the next action loaded a step ahead, no LDS, no
//                              barrier.  The record is loaded once and stored once per launch; dynamic
//                              ring and the env's own return buffers are written through as gte_step
//                              would.
//   gte_backtest_fold_kernel   ONE step into the records from what an ordinary step launch left behind
//                              (reward64, flags, the record, the terminal record): the last step of a
//                              call, and every step where gte_rollout itself goes step by step.
//   gte_backtest_begin_kernel  clears the records, or brings them up to date with a gte_reset.
//   gte_signal_actions_kernel  the action a signal table (gte_bind_signals) gives every env for its next
//                              step: one lane per env, the record's idx / dsi -> one byte -> int32.
//   gte_backtest_signal_kernel gte_backtest_kernel with that lookup, at the env's own row, in place of
//                              the [K][N] actions: the aligned 16-byte piece of the strategy's row that
//                              holds idx is carried in registers and the wanted byte shifted out.
//
// Both paths run the same backtest_step() on the same values, so they give the same records bit for bit
// (tests/test_gpu_backtest.py).  This unit is compiled WITHOUT GTE_HOT_ONLY: in same-step mode phase A
// has already reset the env when it returns, and the terminal valuation is what it stored in the
// terminal record (p.final_rec) just before — the lane that wrote it reads it back in program order.
#include "gte_backtest_regs.h"

namespace gte {

__global__ __launch_bounds__(256) void gte_backtest_kernel(const Params p, const int32_t* actions,
                                                           gte_backtest_stats* stats, const int n_steps,
                                                           const int epw) {
  const int lane = threadIdx.x & 63;
  // epw envs per wavefront, env = slot: the geometry of gte_rollout_state_kernel (gte_rollout.hip)
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  if (active) load_stats(stats + e, a);
  int32_t act = active ? actions[e] : -1;
  PriceCarry pc = {0.0, 0.0, -1, 0};
  ObsJob job;
  // (written like gte_rollout_state_kernel's step on purpose: as a plain loop body the compiler kept
  // the env's registers in scratch memory)
  auto run_a = [&](int k) {
    const int32_t now = act;
    if (active && k + 1 < n_steps) act = actions[(int64_t)(k + 1) * p.N + e];
    double pv = 0.0;
    StepOut so = {};
    // the record is stored once, after the last step; no terminal list: the step launch that follows
    // this one builds it
    phase_a<MODE_STEP>(p, e, active, lane, job, nullptr, /*compact=*/false, &pv, &s, &now,
                       /*write_record=*/k == n_steps - 1, &pc, &so);
    if (active) backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    a.episode_seen = p.rec[e].episode;  // (this lane's own resets wrote it)
    store_stats(stats + e, a);
  }
}

__global__ __launch_bounds__(256) void gte_backtest_fold_kernel(const Params p, gte_backtest_stats* stats) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  gte_backtest_stats a;
  load_stats(stats + e, a);
  const EnvRec* r = &p.rec[e];
  const int32_t flags = (p.terminated[e] ? 1 : 0) | (p.truncated[e] ? 2 : 0);
  backtest_step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
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

// gte_backtest_kernel (same geometry, same steps, same record handling) with each step's action taken
// from the env's signal table at s.idx / s.dsi before phase A.  gte_backtest_kernel hides its action
// load by asking for the next step's a step ahead; here the next row is known only after the step.  So
// the load is amortised and speculated instead: the lane keeps the aligned 16-byte piece of its
// strategy's row that holds idx (w; pbase = its first row, pdsi = its dataset) and shifts the wanted
// byte out.  A plain step moves to idx + 1, so on the last row of a piece the next piece is asked for
// BEFORE phase A and arrives under it; only after a reset, a dataset switch or a step that did not
// advance (frozen env) is the piece wrong when the step returns, and then it is loaded again, waited
// for.  One 16-byte request per 16 steps and env where gte_backtest_kernel issues a 4-byte one per
// step.  GTE_SIGNAL_BYTE_LOAD builds the plain variant instead (one byte per step, loaded after the
// step it follows) for the A/B run of tools/signal_bench.py.
// Reads stay inside the row: the piece at idx & ~15 ends before round_up(T, 16) <= stride, and the
// speculative one is only asked for while idx + 1 < stride (`lim`).
__global__ __launch_bounds__(256) void gte_backtest_signal_kernel(const Params p, const SignalTable* tables,
                                                                  const int S, const int32_t* strategy,
                                                                  gte_backtest_stats* stats, const int n_steps,
                                                                  const int epw) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * 4 + (threadIdx.x >> 6)) * epw + lane;
  const bool active = lane < epw && slot < p.N;
  const int e = active ? slot : 0;
  EnvRegs s = {};
  if (active) load_state(p, e, s);
  gte_backtest_stats a = {};
  if (active) load_stats(stats + e, a);
  const int64_t strat = active ? signal_strategy(p, strategy, S, e) : 0;
  const int8_t* row = nullptr;  // this env's row of the table of dataset pdsi
  int32_t pdsi = -1;
#ifndef GTE_SIGNAL_BYTE_LOAD
  int32_t lim = 0, pbase = 0;
  int4_t w = {0, 0, 0, 0};
#else
  int32_t act = -1;
#endif
  auto fetch = [&](int32_t idx) {
    if (s.dsi != pdsi) {
      const SignalTable t = tables[s.dsi];
      row = t.base + strat * t.stride;
      pdsi = s.dsi;
#ifndef GTE_SIGNAL_BYTE_LOAD
      lim = t.stride > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)t.stride;
#endif
    }
#ifndef GTE_SIGNAL_BYTE_LOAD
    pbase = idx & ~15;
    w = *reinterpret_cast<const int4_t*>(row + pbase);
#else
    act = row[idx];
#endif
  };
  if (active) fetch(s.idx);
  PriceCarry pc = {0.0, 0.0, -1, 0};
  ObsJob job;
  // (a lambda like gte_backtest_kernel's step, for the same reason)
  auto run_a = [&](int k) {
#ifndef GTE_SIGNAL_BYTE_LOAD
    const int32_t now = signal_action(signal_byte(w, s.idx), p.P);
    if (active && k + 1 < n_steps && (s.idx & 15) == 15 && s.idx + 1 < lim) fetch(s.idx + 1);
#else
    const int32_t now = signal_action(act, p.P);
#endif
    double pv = 0.0;
    StepOut so = {};
    phase_a<MODE_STEP>(p, e, active, lane, job, nullptr, /*compact=*/false, &pv, &s, &now,
                       /*write_record=*/k == n_steps - 1, &pc, &so);
    if (active) backtest_step(a, p, e, s.step, pv, s.pos, so.reward, so.flags);
#ifndef GTE_SIGNAL_BYTE_LOAD
    if (active && k + 1 < n_steps && (s.dsi != pdsi || (s.idx & ~15) != pbase)) fetch(s.idx);
#else
    if (active && k + 1 < n_steps) fetch(s.idx);
#endif
  };
  for (int k = 0; k < n_steps; ++k) run_a(k);
  if (active) {
    a.episode_seen = p.rec[e].episode;  // (this lane's own resets wrote it)
    store_stats(stats + e, a);
  }
}

hipError_t launch_backtest_begin(const Params& p, gte_backtest_stats* stats, int clear, hipStream_t stream) {
  hipLaunchKernelGGL(gte_backtest_begin_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, clear);
  return hipGetLastError();
}

// what the from-registers kernels do not do: trajectory rows (the step kernel writes them, gte_kernel);
// and in same-step mode they need somewhere for the terminal records
static bool summary_refused(const Params& p, int epw) {
  return p.log.rows != nullptr || (p.autoreset == GTE_AUTORESET_SAME_STEP && p.final_rec == nullptr) ||
         epw < 1 || epw > 64;
}

hipError_t launch_backtest_summary(const Params& p, const int32_t* actions, gte_backtest_stats* stats, int n_steps,
                                   int epw, hipStream_t stream) {
  if (summary_refused(p, epw)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_backtest_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream, p,
                     actions, stats, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_signal_actions(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                                 int32_t* actions, hipStream_t stream) {
  if (!tables || S < 1 || !actions) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_signal_actions_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, tables, S,
                     strategy, actions);
  return hipGetLastError();
}

hipError_t launch_signal_summary(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                                 gte_backtest_stats* stats, int n_steps, int epw, hipStream_t stream) {
  if (summary_refused(p, epw) || !tables || S < 1) return hipErrorInvalidValue;  // ... and a table to read
  hipLaunchKernelGGL(gte_backtest_signal_kernel, dim3(rollout_blocks(p.N, epw)), dim3(64 * ROLLOUT_WAVES), 0, stream,
                     p, tables, S, strategy, stats, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_backtest_fold(const Params& p, gte_backtest_stats* stats, hipStream_t stream) {
  if (p.autoreset == GTE_AUTORESET_SAME_STEP && p.final_rec == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_backtest_fold_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats);
  return hipGetLastError();
}

}  // namespace gte
