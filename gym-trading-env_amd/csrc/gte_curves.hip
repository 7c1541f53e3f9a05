// gte_curves.hip — per-step rows next to the statistics records (gte_backtest_curves, include/gte.h): the
// from-registers backtest kernels once more, with a tracker that writes what a step leaves in registers — the
// valuation, the position, the market row, the reward, the drawdown against the record's running peak, the flags
// — into caller-owned [R][N] columns, one row per `stride` steps.  Own translation unit: nothing here can perturb
// the code generated for the kernels of gte_backtest.hip, gte_exits.hip, gte_trades.hip, gte_trade_list.hip and
// gte_periods.hip, which run whenever no curve is asked for.
//
//   gte_curve_backtest_kernel   [K][N] actions
//   gte_curve_signal_kernel     signal table
//   gte_curve_exit_kernel       signal table + exit rules: summary_body (gte_summary_body.h) with that source and
//                               CurveTracker.
//   gte_curve_fold_kernel       ONE ordinary step into the record and the rows, from what the step launch left.
//
// The window.  Window j of a call covers its steps j * stride .. min((j + 1) * stride, K) - 1.  A lane keeps the
// window's running reward sum, drawdown maximum and flag bits in registers and counts the steps left in it down,
// so a step divides nothing; when the count reaches zero (or the fold is told that its step is the call's last)
// the lane stores the row — one plain store per kept column — and starts the next window.  The fused launch runs
// steps 0 .. K-2 of a call and the fold step K-1, so a window may be open where the two meet: the lane then leaves
// the three partial values in carry[e] (CurveCarry, library-owned) and the fold picks them up.  On the per-step
// path every fold but a closing one leaves them there for the next.
//
// The layout.  Column c of row j of env e is at c[j * N + e]: a wavefront's epw active lanes store epw * 8
// contiguous bytes per f64 column and closed window.  A NULL column is a uniform branch and issues nothing.
//
// What is written: column[j * N + e] for e < N and j < ceil(K / stride) only — the fused launch closes window j
// at step (j + 1) * stride - 1 <= K - 2, the fold writes row k / stride for k <= K - 1; carry[e] for e < N.
// Compiled WITHOUT GTE_HOT_ONLY like gte_backtest.hip.
#include "gte_summary_body.h"

namespace gte {

static_assert(sizeof(CurveCarry) == 32, "CurveCarry: two doubles, the flags, padding to two 16-byte pieces");

// next: where the env stands after the step (landed()); left: the steps the open window still takes, counted down
// in before(); j: the open window.  Both are set again inside step(), which only active lanes run, so they are
// per-lane values (an inactive lane counts on below zero and stores nothing); force: this step is the call's last
// (the fold's)
struct CurveTracker {
  static constexpr bool pieces = false;
  const Curves c;
  const int32_t first;  // the step of the call this launch begins with
  const bool force;
  double w_reward = 0.0, w_drawdown = 0.0;
  int32_t w_flags = 0, left = 0, next = 0, j = 0;
  __device__ __forceinline__ CurveTracker(const Curves& c_, int32_t first_, bool force_)
      : c(c_), first(first_), force(force_) {}
  __device__ __forceinline__ void init(bool active, int e) {
    const int32_t done = first % c.stride;  // steps the open window has taken already
    left = c.stride - done;
    j = first / c.stride;
    if (active && done != 0) {
      const double2_t d = *reinterpret_cast<const double2_t*>(c.carry + e);
      w_reward = d[0];
      w_drawdown = d[1];
      w_flags = c.carry[e].flags;
    }
  }
  __device__ __forceinline__ void dataset(int32_t) {}
  __device__ __forceinline__ void piece(int32_t) {}
  __device__ __forceinline__ int32_t limit() const { return 0; }
  __device__ __forceinline__ void before(int32_t, int32_t) { --left; }
  __device__ __forceinline__ void landed(int32_t idx) { next = idx; }
  // the classification of backtest_step() (gte_backtest_regs.h), which runs directly after this: `a` is the record
  // before the step
  __device__ __forceinline__ void step(const gte_backtest_stats& a, const Params& p, int e, int32_t step_after,
                                       double pv, int32_t pos_after, double reward, int32_t flags) {
    const bool nr = a.ended != 0;
    const bool stepped = !(nr && (p.autoreset == GTE_AUTORESET_NEXT_STEP || step_after == a.step_seen));
    double v = pv;
    int32_t pos = pos_after, where = next;
    if (stepped) {
      if (flags != 0 && p.autoreset == GTE_AUTORESET_SAME_STEP) {
        // the env is already reset: the row holds the terminal valuation and position (backtest_step reads them so)
        // ... and the row they were taken at; every other transition lands on the row before it + 1
        const EnvRec* t = &p.final_rec[e];
        const int4 w = reinterpret_cast<const int4*>(t)[0];  // idx, step, pos, dsi
        where = w.x;
        pos = w.z;
        v = reinterpret_cast<const double2*>(&t->asset)[2].x;
        w_flags |= GTE_CURVE_RESET;
      }
      // (computed whether or not the columns are kept: d is the d of backtest_transition(), which follows, and the
      // compiler shares the division; behind `if (c.bufs.drawdown)` it does not — DESIGN.md, "Curves")
      const double peak = v > a.peak ? v : a.peak;  // the record's peak after this transition
      const double d = 1.0 - v / peak;
      if (d > w_drawdown) w_drawdown = d;
      w_reward = w_reward + reward;
      w_flags |= flags & (GTE_CURVE_TERMINATED | GTE_CURVE_TRUNCATED);
    } else {
      w_flags |= p.autoreset == GTE_AUTORESET_NEXT_STEP ? GTE_CURVE_RESET : GTE_CURVE_FROZEN;
    }
    if (left != 0 && !force) return;
    const int64_t at = (int64_t)j * p.N + e;
    if (c.bufs.valuation) c.bufs.valuation[at] = v;
    if (c.bufs.drawdown) c.bufs.drawdown[at] = w_drawdown;
    if (c.bufs.reward) c.bufs.reward[at] = w_reward;
    if (c.bufs.position) c.bufs.position[at] = pos;
    if (c.bufs.row) c.bufs.row[at] = where;
    if (c.bufs.flags) c.bufs.flags[at] = (uint8_t)w_flags;
    w_reward = 0.0;
    w_drawdown = 0.0;
    w_flags = 0;
    left = c.stride;
    j += 1;
  }
  // a window that is open where the launch ends goes on in the next one
  __device__ __forceinline__ void store(int e) {
    if (left == c.stride) return;
    const double2_t d = {w_reward, w_drawdown};
    const int4_t f = {w_flags, 0, 0, 0};
    *reinterpret_cast<double2_t*>(c.carry + e) = d;
    reinterpret_cast<int4_t*>(c.carry + e)[1] = f;
  }
};

__global__ __launch_bounds__(256) void gte_curve_backtest_kernel(const Params p, const int32_t* actions,
                                                                 gte_backtest_stats* stats, const Curves c,
                                                                 const int n_steps, const int epw) {
  summary_body(p, stats, ActionSource(actions), CurveTracker(c, 0, false), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_curve_signal_kernel(const Params p, const SignalTable* tables, const int S,
                                                               const int32_t* strategy, gte_backtest_stats* stats,
                                                               const Curves c, const int n_steps, const int epw) {
  summary_body(p, stats, SignalSource(tables, S, strategy), CurveTracker(c, 0, false), n_steps, epw);
}

__global__ __launch_bounds__(256) void gte_curve_exit_kernel(const Params p, const SignalTable* tables, const int S,
                                                             const int32_t* strategy, const ExitRules rules,
                                                             gte_backtest_stats* stats, const Curves c,
                                                             const int n_steps, const int epw) {
  summary_body(p, stats, ExitSource(tables, S, strategy, rules), CurveTracker(c, 0, false), n_steps, epw);
}

// step `k` of a call of n_call steps
__global__ __launch_bounds__(256) void gte_curve_fold_kernel(const Params p, gte_backtest_stats* stats, const Curves c,
                                                             const int k, const int n_call) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  gte_backtest_stats a;
  load_stats(stats + e, a);
  CurveTracker trk(c, k, k == n_call - 1);
  trk.init(true, e);
  const EnvRec* r = &p.rec[e];
  const int32_t flags = (p.terminated[e] ? 1 : 0) | (p.truncated[e] ? 2 : 0);
  trk.before(0, 0);
  trk.landed(r->idx);
  trk.step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  backtest_step(a, p, e, r->step, r->pv, r->pos, p.reward64[e], flags);
  a.episode_seen = r->episode;
  store_stats(stats + e, a);
  trk.store(e);
}

static bool curves_unusable(const gte_backtest_stats* stats, const Curves& c) {
  return !stats || !c.carry || c.stride < 1;
}

hipError_t launch_curve_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats, const Curves& c,
                                int n_steps, int epw, hipStream_t stream) {
  if (summary_refused(p, src, epw) || curves_unusable(stats, c)) return hipErrorInvalidValue;
  const dim3 grid(rollout_blocks(p.N, epw)), block(64 * ROLLOUT_WAVES);
  if (src.actions)
    hipLaunchKernelGGL(gte_curve_backtest_kernel, grid, block, 0, stream, p, src.actions, stats, c, n_steps, epw);
  else if (!src.rules)
    hipLaunchKernelGGL(gte_curve_signal_kernel, grid, block, 0, stream, p, src.tables, src.S, src.strategy, stats, c,
                       n_steps, epw);
  else
    hipLaunchKernelGGL(gte_curve_exit_kernel, grid, block, 0, stream, p, src.tables, src.S, src.strategy, *src.rules,
                       stats, c, n_steps, epw);
  return hipGetLastError();
}

hipError_t launch_curve_fold(const Params& p, gte_backtest_stats* stats, const Curves& c, int k, int n_call,
                             hipStream_t stream) {
  if (fold_refused(p) || curves_unusable(stats, c) || k < 0 || k >= n_call) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_curve_fold_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p, stats, c, k, n_call);
  return hipGetLastError();
}

}  // namespace gte
