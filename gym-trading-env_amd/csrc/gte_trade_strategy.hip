// gte_trade_strategy.hip — trade statistics per strategy and their ranking (gte_reduce_trade_stats,
// gte_rank_trade_stats, include/gte.h): N trade records folded into S strategy records, then a score per
// strategy that feeds the selection kernels of gte_strategy.hip (launch_rank_select).  Own translation unit,
// beside gte_strategy.hip: nothing here can perturb the code generated for its kernels.
//
//   Two kernels, ONE summation order (the one of gte_reduce_backtest_stats: eight interleaved accumulators,
//   member j goes to accumulator j % 8, closed as ((((((a0 + a1) + a2) + a3) + a4) + a5) + a6) + a7):
//   gte_trade_reduce_kernel        (many strategies, few members)  one lane per strategy walks its members in
//             order, all eight accumulators of the three sums in its own registers.
//   gte_trade_reduce_block_kernel  (few strategies, many members)  a workgroup of eight wavefronts per strategy.
//             Wavefront w IS accumulator w: its lanes load 64 of the places w, w + 8, w + 16, ... at once, then
//             the values are added one after the other, read across lanes in place order; the eight
//             accumulators and the order-free parts meet in LDS, where one lane closes them.
//   The host picks by N / S (the threshold of launch_reduce_strategies); the records are the same bit for bit.
//   A place past a list's end and an entry that names no env in [0, N) add nothing (0.0 to a sum, which leaves
//   every sum as it is).  No atomics, no scratch memory.
//   gte_trade_score_kernel         one lane per strategy: its score, and its entry of candidate list 0.
//
// What may be read: a record only at an index checked against [0, N); group_envs only at offsets clamped into
// [0, N]; group_offsets at s and s + 1 for s < S.  What is written: the 128 bytes of out[s] for s < S;
// scores[s], cand_score[s], cand_index[s] for s < S.
#include "gte_launch.h"
#include "gte_members.h"

namespace gte {

static_assert(sizeof(gte_strategy_trade_stats) == 128 && offsetof(gte_strategy_trade_stats, hold_sum) == 48 &&
              offsetof(gte_strategy_trade_stats, gross_profit) == 56 && offsetof(gte_strategy_trade_stats, best_trade) == 80 &&
              offsetof(gte_strategy_trade_stats, max_len) == 96 && offsetof(gte_strategy_trade_stats, reserved) == 112,
              "gte_strategy_trade_stats: 128 bytes (include/gte.h)");

constexpr int TS_BLK_WAVES = 8;  // wavefronts of the block kernel = accumulators of the stated order

// what a strategy gathers besides the three f64 sums: order-free, but for which of two equal extremes stays —
// the one met first in MEMBER order, so the place travels with the value
struct TsFold {
  long long closed = 0, wins = 0, losses = 0, forced = 0, reversals = 0, exposure = 0, hold_sum = 0;
  int max_len = 0, max_streak = 0, envs = 0, traded = 0;
  double best = -__builtin_inf(), worst = __builtin_inf();
  int best_at = INT32_MAX, worst_at = INT32_MAX;
  // member r at place m (a caller meets its members by increasing place)
  __device__ __forceinline__ void add(const gte_trade_stats& r, int m) {
    closed += r.closed; wins += r.wins; losses += r.losses; forced += r.forced; reversals += r.reversals;
    exposure += r.exposure; hold_sum += r.hold_sum;
    if (r.max_len > max_len) max_len = r.max_len;
    if (r.max_loss_streak > max_streak) max_streak = r.max_loss_streak;
    envs += 1;
    traded += r.closed > 0 ? 1 : 0;
    if (r.best_trade > best) { best = r.best_trade; best_at = m; }
    if (r.worst_trade < worst) { worst = r.worst_trade; worst_at = m; }
  }
  __device__ __forceinline__ void join(const TsFold& o) {
    closed += o.closed; wins += o.wins; losses += o.losses; forced += o.forced; reversals += o.reversals;
    exposure += o.exposure; hold_sum += o.hold_sum;
    if (o.max_len > max_len) max_len = o.max_len;
    if (o.max_streak > max_streak) max_streak = o.max_streak;
    envs += o.envs;
    traded += o.traded;
    if (o.best > best || (o.best == best && o.best_at < best_at)) { best = o.best; best_at = o.best_at; }
    if (o.worst < worst || (o.worst == worst && o.worst_at < worst_at)) { worst = o.worst; worst_at = o.worst_at; }
  }
  __device__ __forceinline__ TsFold of_lane(int from) const {
    TsFold o;
    o.closed = __shfl(closed, from, 64); o.wins = __shfl(wins, from, 64); o.losses = __shfl(losses, from, 64);
    o.forced = __shfl(forced, from, 64); o.reversals = __shfl(reversals, from, 64);
    o.exposure = __shfl(exposure, from, 64); o.hold_sum = __shfl(hold_sum, from, 64);
    o.max_len = __shfl(max_len, from, 64); o.max_streak = __shfl(max_streak, from, 64);
    o.envs = __shfl(envs, from, 64); o.traded = __shfl(traded, from, 64);
    o.best = __shfl(best, from, 64); o.worst = __shfl(worst, from, 64);
    o.best_at = __shfl(best_at, from, 64); o.worst_at = __shfl(worst_at, from, 64);
    return o;
  }
};

__device__ __forceinline__ void ts_store(gte_strategy_trade_stats* dst, const TsFold& f, double gp, double gl, double sq) {
  gte_strategy_trade_stats o = {};
  o.closed = f.closed; o.wins = f.wins; o.losses = f.losses; o.forced = f.forced; o.reversals = f.reversals;
  o.exposure = f.exposure; o.hold_sum = f.hold_sum;
  o.gross_profit = gp; o.gross_loss = gl; o.ret_sq_sum = sq;
  o.best_trade = f.best; o.worst_trade = f.worst;
  o.max_len = f.max_len; o.max_loss_streak = f.max_streak; o.envs = f.envs; o.envs_traded = f.traded;
  *dst = o;
}

__global__ __launch_bounds__(256) void gte_trade_reduce_kernel(const gte_trade_stats* __restrict__ rec, int N, int S,
                                                               unsigned first_shift,
                                                               const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ envs,
                                                               gte_strategy_trade_stats* __restrict__ out) {
  const long long s64 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s64 >= S) return;
  const int s = (int)s64;
  const Members g = members_of(s, N, S, first_shift, offsets);
  double gp[8], gl[8], sq[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) gp[a] = gl[a] = sq[a] = 0.0;
  TsFold f;
  for (int base = 0; base < g.n; base += 8) {
#pragma unroll
    for (int a = 0; a < 8; ++a) {  // (a is a constant after unrolling: the accumulators stay in registers)
      const int m = base + a;
      const long long e = m < g.n ? member_env(g, envs, N, S, m) : -1;
      if (e >= 0) {
        const gte_trade_stats r = rec[e];
        gp[a] += r.gross_profit;
        gl[a] += r.gross_loss;
        sq[a] += r.ret_sq_sum;
        f.add(r, m);
      }
    }
  }
  double GP = gp[0], GL = gl[0], SQ = sq[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) { GP = GP + gp[i]; GL = GL + gl[i]; SQ = SQ + sq[i]; }
  ts_store(out + s, f, GP, GL, SQ);
}

__global__ __launch_bounds__(64 * TS_BLK_WAVES) void gte_trade_reduce_block_kernel(
    const gte_trade_stats* __restrict__ rec, int N, int S, unsigned first_shift, const int32_t* __restrict__ offsets,
    const int32_t* __restrict__ envs, gte_strategy_trade_stats* __restrict__ out) {
  __shared__ double sh_f[TS_BLK_WAVES][5];     // the three sums, best, worst
  __shared__ long long sh_k[TS_BLK_WAVES][7];  // the 64-bit counters
  __shared__ int sh_i[TS_BLK_WAVES][6];        // max_len, max_streak, envs, traded, best_at, worst_at
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int s = blockIdx.x;  // (the grid is S workgroups)
  const Members g = members_of(s, N, S, first_shift, offsets);
  const int mine = g.n > w ? (g.n - w + 7) / 8 : 0;  // places of this accumulator: w + 8 t, t < mine

  double a_gp = 0.0, a_gl = 0.0, a_sq = 0.0;
  TsFold f;
  for (int tb = 0; tb < mine; tb += 64) {
    const int t = tb + lane;
    const int m = w + 8 * t;
    const long long e = t < mine ? member_env(g, envs, N, S, m) : -1;
    double x_gp = 0.0, x_gl = 0.0, x_sq = 0.0;
    if (e >= 0) {
      const gte_trade_stats r = rec[e];
      x_gp = r.gross_profit; x_gl = r.gross_loss; x_sq = r.ret_sq_sum;
      f.add(r, m);
    }
    const int live = mine - tb < 64 ? mine - tb : 64;  // (the same in every lane of the wavefront)
    for (int l = 0; l < live; ++l) {                   // the chain, in place order
      a_gp = a_gp + __shfl(x_gp, l, 64);
      a_gl = a_gl + __shfl(x_gl, l, 64);
      a_sq = a_sq + __shfl(x_sq, l, 64);
    }
  }
  // the wave's order-free parts over its lanes, then everything into LDS
  // (a butterfly: join is commutative and associative, the places of two lanes' extremes never being equal)
  TsFold fw = f;
  for (int off = 32; off > 0; off >>= 1) fw.join(fw.of_lane(lane ^ off));
  if (lane == 0) {
    sh_f[w][0] = a_gp; sh_f[w][1] = a_gl; sh_f[w][2] = a_sq; sh_f[w][3] = fw.best; sh_f[w][4] = fw.worst;
    sh_k[w][0] = fw.closed; sh_k[w][1] = fw.wins; sh_k[w][2] = fw.losses; sh_k[w][3] = fw.forced;
    sh_k[w][4] = fw.reversals; sh_k[w][5] = fw.exposure; sh_k[w][6] = fw.hold_sum;
    sh_i[w][0] = fw.max_len; sh_i[w][1] = fw.max_streak; sh_i[w][2] = fw.envs; sh_i[w][3] = fw.traded;
    sh_i[w][4] = fw.best_at; sh_i[w][5] = fw.worst_at;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double GP = sh_f[0][0], GL = sh_f[0][1], SQ = sh_f[0][2];
  TsFold all;
  for (int i = 0; i < TS_BLK_WAVES; ++i) {
    if (i > 0) { GP = GP + sh_f[i][0]; GL = GL + sh_f[i][1]; SQ = SQ + sh_f[i][2]; }
    TsFold o;
    o.best = sh_f[i][3]; o.worst = sh_f[i][4];
    o.closed = sh_k[i][0]; o.wins = sh_k[i][1]; o.losses = sh_k[i][2]; o.forced = sh_k[i][3];
    o.reversals = sh_k[i][4]; o.exposure = sh_k[i][5]; o.hold_sum = sh_k[i][6];
    o.max_len = sh_i[i][0]; o.max_streak = sh_i[i][1]; o.envs = sh_i[i][2]; o.traded = sh_i[i][3];
    o.best_at = sh_i[i][4]; o.worst_at = sh_i[i][5];
    all.join(o);
  }
  ts_store(out + s, all, GP, GL, SQ);
}

hipError_t launch_reduce_trade_stats(const gte_trade_stats* records, int n_envs, int n_strategies, int64_t env_id_base,
                                     const int32_t* group_offsets, const int32_t* group_envs,
                                     gte_strategy_trade_stats* out, hipStream_t stream) {
  if (!records || !out || n_envs < 1 || n_strategies < 1 || (group_offsets == nullptr) != (group_envs == nullptr))
    return hipErrorInvalidValue;
  const int64_t S = n_strategies;
  const unsigned first_shift = members_first_shift(env_id_base, S);
  // a workgroup per strategy once the average list has 32 members; speed only: the records do not depend on it
  if ((int64_t)n_envs >= 32 * S)
    hipLaunchKernelGGL(gte_trade_reduce_block_kernel, dim3((unsigned)S), dim3(64 * TS_BLK_WAVES), 0, stream, records,
                       n_envs, n_strategies, first_shift, group_offsets, group_envs, out);
  else
    hipLaunchKernelGGL(gte_trade_reduce_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, records, n_envs,
                       n_strategies, first_shift, group_offsets, group_envs, out);
  return hipGetLastError();
}

// ---- ranking

__global__ __launch_bounds__(256) void gte_trade_score_kernel(const gte_strategy_trade_stats* __restrict__ stats, int S,
                                                              int metric, long long min_trades,
                                                              double* __restrict__ scores, double* __restrict__ cand_score,
                                                              int32_t* __restrict__ cand_index) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const gte_strategy_trade_stats& t = stats[s];
  const long long closed = t.closed;
  const double count = (double)closed;
  double score;
  if (metric == GTE_TRADE_METRIC_WIN_RATE) {
    score = (double)t.wins / count;
  } else if (metric == GTE_TRADE_METRIC_PROFIT_FACTOR) {
    score = t.gross_profit / (0.0 - t.gross_loss);
  } else if (metric == GTE_TRADE_METRIC_WORST_TRADE) {
    score = t.worst_trade;
  } else if (metric == GTE_TRADE_METRIC_NEG_MAX_LOSS_STREAK) {
    score = -(double)t.max_loss_streak;
  } else {
    const double m = (t.gross_profit + t.gross_loss) / count;
    score = m;
    if (metric == GTE_TRADE_METRIC_TRADE_SHARPE) {
      const double q = t.ret_sq_sum / count;
      double v = q - m * m;
      if (!(v > 0.0)) v = 0.0;
      score = m / sqrt(v);
    }
  }
  if (scores) scores[s] = score;
  const bool ranked = closed >= (min_trades > 1 ? min_trades : 1) && score == score;
  cand_score[s] = ranked ? score : __builtin_nan("");
  cand_index[s] = ranked ? (int32_t)s : -1;
}

hipError_t launch_trade_scores(const gte_strategy_trade_stats* stats, int n_strategies, int metric, int64_t min_trades,
                               double* scores, double* cand_score, int32_t* cand_index, hipStream_t stream) {
  if (!stats || n_strategies < 1 || !cand_score || !cand_index) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_trade_score_kernel, dim3((unsigned)(((int64_t)n_strategies + 255) / 256)), dim3(256), 0, stream,
                     stats, n_strategies, metric, (long long)min_trades, scores, cand_score, cand_index);
  return hipGetLastError();
}

}  // namespace gte
