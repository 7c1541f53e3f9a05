// gte_period_strategy.hip — period statistics per strategy and their ranking over a set of periods
// (gte_reduce_period_stats, gte_rank_period_stats, include/gte.h): N * B period records folded into S * B strategy
// records, then a score per strategy that feeds the selection kernels of gte_strategy.hip (launch_rank_select).
// Own translation unit, beside gte_strategy.hip and gte_trade_strategy.hip: nothing here can perturb their code.
//
//   gte_period_reduce_kernel   ONE kernel, ONE summation order per (strategy, period) — the one of
//             gte_reduce_backtest_stats: eight interleaved accumulators, member j goes to accumulator j % 8,
//             closed as ((((((a0 + a1) + a2) + a3) + a4) + a5) + a6) + a7.  This pass reads N * B * 32 bytes
//             (134 MB at 65 536 x 64), so it is shaped for bandwidth: a thread owns one (strategy, period), the
//             threads of a strategy are neighbours and lie across its periods, and they walk the member list
//             together, one member after the other — a member's B records are one contiguous read of B * 32
//             bytes, eight members in flight per thread.  A workgroup holds 256 / B strategies
//             (B <= GTE_MAX_PERIODS = 128: at least two).  Every thread adds its own chain
//             in member order: the bits do not depend on the geometry.  No atomics, no LDS, no scratch.
//             A place past a list's end and an entry that names no env in [0, N) add nothing.
//   gte_period_score_kernel    one lane per strategy: its score over the periods of the mask, and its entry of
//             candidate list 0.
//
// What may be read: records [e * B, e * B + B) only for e checked against [0, N); group_envs only at offsets
// clamped into [0, N]; group_offsets at s and s + 1 for s < S.  What is written: the 48 bytes of out[s * B + b]
// for s < S, b < B; scores[s], cand_score[s], cand_index[s] for s < S.
#include "gte_launch.h"
#include "gte_members.h"

namespace gte {

static_assert(sizeof(gte_strategy_period_stats) == 48 && offsetof(gte_strategy_period_stats, steps) == 16 &&
              offsetof(gte_strategy_period_stats, episodes) == 32 && offsetof(gte_strategy_period_stats, envs_stepped) == 40,
              "gte_strategy_period_stats: 48 bytes (include/gte.h)");

constexpr int PS_THREADS = 256;

typedef double __attribute__((ext_vector_type(2))) ps_double2;

__global__ __launch_bounds__(PS_THREADS) void gte_period_reduce_kernel(const gte_period_stats* __restrict__ rec, int N,
                                                                       int B, int S, unsigned first_shift,
                                                                       const int32_t* __restrict__ offsets,
                                                                       const int32_t* __restrict__ envs,
                                                                       gte_strategy_period_stats* __restrict__ out) {
  const int per_block = PS_THREADS / B;  // strategies of a workgroup (B <= 128: at least two)
  const int local = threadIdx.x / B;
  const int b = threadIdx.x - local * B;
  const long long s64 = (long long)blockIdx.x * per_block + local;
  if (local >= per_block || s64 >= S) return;
  const int s = (int)s64;
  const Members g = members_of(s, N, S, first_shift, offsets);
  double r1[8], r2[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) r1[a] = r2[a] = 0.0;
  long long steps = 0, trades = 0, episodes = 0;
  int stepped = 0;
  for (int base = 0; base < g.n; base += 8) {
    ps_double2 d0[8], d1[8];
    bool have[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {  // eight members' loads in flight (a is a constant after unrolling)
      const int m = base + a;
      const long long e = m < g.n ? member_env(g, envs, N, S, m) : -1;
      have[a] = e >= 0;
      if (have[a]) {
        const ps_double2* q = reinterpret_cast<const ps_double2*>(rec + e * B + b);
        d0[a] = q[0];
        d1[a] = q[1];
      }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      if (have[a]) {
        r1[a] += d0[a][0];
        r2[a] += d0[a][1];
        const long long n = __double_as_longlong(d1[a][0]);
        const long long te = __double_as_longlong(d1[a][1]);
        steps += n;
        trades += (int32_t)te;
        episodes += (int32_t)(te >> 32);
        stepped += n > 0 ? 1 : 0;
      }
    }
  }
  double R1 = r1[0], R2 = r2[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) { R1 = R1 + r1[i]; R2 = R2 + r2[i]; }
  ps_double2* q = reinterpret_cast<ps_double2*>(out + (long long)s * B + b);
  const ps_double2 o0 = {R1, R2}, o1 = {__longlong_as_double(steps), __longlong_as_double(trades)},
                   o2 = {__longlong_as_double(episodes), __longlong_as_double((long long)(uint32_t)stepped)};
  q[0] = o0; q[1] = o1; q[2] = o2;
}

hipError_t launch_reduce_period_stats(const gte_period_stats* records, int n_envs, int n_periods, int n_strategies,
                                      int64_t env_id_base, const int32_t* group_offsets, const int32_t* group_envs,
                                      gte_strategy_period_stats* out, hipStream_t stream) {
  if (!records || !out || n_envs < 1 || n_strategies < 1 || n_periods < 1 || n_periods > GTE_MAX_PERIODS ||
      (group_offsets == nullptr) != (group_envs == nullptr))
    return hipErrorInvalidValue;
  const int64_t S = n_strategies;
  const unsigned first_shift = members_first_shift(env_id_base, S);
  const int64_t per_block = PS_THREADS / n_periods;
  hipLaunchKernelGGL(gte_period_reduce_kernel, dim3((unsigned)((S + per_block - 1) / per_block)), dim3(PS_THREADS), 0,
                     stream, records, n_envs, n_periods, n_strategies, first_shift, group_offsets, group_envs, out);
  return hipGetLastError();
}

// ---- ranking

__global__ __launch_bounds__(256) void gte_period_score_kernel(const gte_strategy_period_stats* __restrict__ stats, int S,
                                                               int B, const PeriodMask mask, int metric,
                                                               long long min_steps, double* __restrict__ scores,
                                                               double* __restrict__ cand_score,
                                                               int32_t* __restrict__ cand_index) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const gte_strategy_period_stats* t = stats + s * B;
  long long n = 0, c = 0, up = 0;
  double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, lo = __builtin_inf();
  for (int b = 0; b < B; ++b) {
    if (!mask.has(b)) continue;
    const double x = t[b].reward_sum;
    n += t[b].steps;
    s1 = s1 + x;
    s2 = s2 + t[b].reward_sq_sum;
    if (t[b].steps > 0) {
      c += 1;
      t1 = t1 + x;
      t2 = t2 + x * x;
      if (x < lo) lo = x;
      up += x > 0.0 ? 1 : 0;
    }
  }
  double score;
  if (metric == GTE_PERIOD_METRIC_REWARD_SUM) {
    score = s1;
  } else if (metric == GTE_PERIOD_METRIC_WORST_PERIOD) {
    score = c > 0 ? lo : __builtin_nan("");
  } else if (metric == GTE_PERIOD_METRIC_POSITIVE_SHARE) {
    score = (double)up / (double)c;
  } else {
    const bool by_period = metric == GTE_PERIOD_METRIC_PERIOD_SHARPE;
    const double total = by_period ? t1 : s1, sq = by_period ? t2 : s2, count = (double)(by_period ? c : n);
    const double m = total / count;
    score = m;
    if (metric != GTE_PERIOD_METRIC_MEAN_REWARD) {
      const double q = sq / count;
      double v = q - m * m;
      if (!(v > 0.0)) v = 0.0;
      score = m / sqrt(v);
    }
  }
  if (scores) scores[s] = score;
  const bool ranked = n >= (min_steps > 1 ? min_steps : 1) && score == score;
  cand_score[s] = ranked ? score : __builtin_nan("");
  cand_index[s] = ranked ? (int32_t)s : -1;
}

hipError_t launch_period_scores(const gte_strategy_period_stats* stats, int n_strategies, int n_periods,
                                const uint64_t period_mask[2], int metric, int64_t min_steps, double* scores,
                                double* cand_score, int32_t* cand_index, hipStream_t stream) {
  if (!stats || n_strategies < 1 || n_periods < 1 || n_periods > GTE_MAX_PERIODS || !period_mask || !cand_score ||
      !cand_index)
    return hipErrorInvalidValue;
  const PeriodMask mask = {{period_mask[0], period_mask[1]}};
  hipLaunchKernelGGL(gte_period_score_kernel, dim3((unsigned)(((int64_t)n_strategies + 255) / 256)), dim3(256), 0, stream,
                     stats, n_strategies, n_periods, mask, metric, (long long)min_steps, scores, cand_score, cand_index);
  return hipGetLastError();
}

}  // namespace gte
