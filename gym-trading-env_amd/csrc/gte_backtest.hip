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

// strategy of env e: the caller's array, or (env_id_base + e) % S — what the unsharded run gives that env
__device__ __forceinline__ int64_t signal_strategy(const Params& p, const int32_t* strategy, int S, int e) {
  return strategy ? (int64_t)strategy[e] : (p.env_id_base + e) % S;
}

// a table value as the action of a step: outside [0, P) it means hold (None, environments.py:234)
__device__ __forceinline__ int32_t signal_action(int32_t v, int32_t P) {
  return (uint32_t)v < (uint32_t)P ? v : -1;
}

__global__ __launch_bounds__(256) void gte_signal_actions_kernel(const Params p, const SignalTable* tables,
                                                                 const int S, const int32_t* strategy,
                                                                 int32_t* actions) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  const int4_t a = reinterpret_cast<const int4_t*>(&p.rec[e])[0];  // idx, step, pos, dsi
  const SignalTable t = tables[a[3]];
  actions[e] = signal_action(t.base[signal_strategy(p, strategy, S, e) * t.stride + a[0]], p.P);
}

// byte idx & 15 of an aligned 16-byte piece, sign-extended: three selects and one bit-field extract
__device__ __forceinline__ int32_t signal_byte(const int4_t& w, int32_t idx) {
  const int j = idx & 15;
  const int32_t word = j < 8 ? (j < 4 ? w[0] : w[1]) : (j < 12 ? w[2] : w[3]);
  return (int32_t)(int8_t)(word >> ((j & 3) * 8));
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
