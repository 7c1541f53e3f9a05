// gte_strategy.hip — per-strategy statistics and ranking (gte_reduce_backtest_stats, gte_rank_strategies,
// include/gte.h): N env records folded into S strategy records, then the k best by a score.  Own
// translation unit: a kernel added to an existing unit perturbs its neighbours' register allocation
// (DESIGN.md §4 "Auxiliary kernels").
//
//   A record is eight 16-byte pieces; every lane folds ONE piece of its members, 16 bytes per load, so one wave
//   instruction requests whole 128-byte records.  Two kernels, ONE summation order:
//   gte_strategy_reduce_kernel        (many strategies, few members)  a wavefront folds 8 neighbouring
//             strategies, 8 lanes each.  Every lane keeps the eight interleaved accumulators of its piece
//             itself; member j goes to accumulator j % 8, eight members (loads) in flight per pass.  With the
//             default map the 8 strategies' j-th members are neighbouring records: one load instruction =
//             1 KiB contiguous, and one store instruction writes eight whole output records.
//   gte_strategy_reduce_block_kernel  (few strategies, many members)  a workgroup of eight wavefronts folds one
//             strategy.  Wavefront w IS accumulator w: it adds members w, w + 8, w + 16, ... one after the
//             other — eight of them per load instruction, four instructions in flight, the values read across
//             lanes in member order — and the eight accumulators meet in LDS.
//          In both, the sums close as ((((((a0 + a1) + a2) + a3) + a4) + a5) + a6) + a7 — the order stated in
//          include/gte.h, which depends on the member list alone; the host picks the kernel by N / S and the
//          records are the same bit for bit either way (tests/test_gpu_strategy_stats.py runs both).
//          No atomics (a float atomic sum depends on arrival order), no scratch memory.
//   gte_strategy_score_kernel       one lane per strategy: its score, and its entry of the candidate list
//                                   (score, index), or (NaN, -1) when it is not ranked.
//   gte_strategy_select_kernel      a workgroup sorts 1 024 candidates in LDS (bitonic; LDS earns its place
//                                   here: 55 compare-exchange rounds over 12 KiB) and keeps the first
//                                   `keep`; launched over shrinking lists until one workgroup holds them all.
//
// What may be read: a record is loaded only at an index checked against [0, N) (an index that fails the
// check, and a place past a list's end, load record 0 instead — N >= 1 — and count as zeros);
// group_envs only at offsets clamped into [0, N] (gte.h: offsets[S] <= N entries exist); group_offsets
// at s and s + 1 for s < S.  What is written: the 128 bytes of out[s] for s < S; scores[s]; the
// candidate lists up to the sizes launch_rank_strategies states; top_index / top_score [k].
#include "gte_launch.h"
#include "gte_members.h"

namespace gte {

typedef unsigned long long st_u2 __attribute__((ext_vector_type(2)));

static_assert(sizeof(gte_backtest_stats) == 128 && offsetof(gte_backtest_stats, steps) == 0 &&
              offsetof(gte_backtest_stats, reward_sum) == 8 && offsetof(gte_backtest_stats, reward_sq_sum) == 16 &&
              offsetof(gte_backtest_stats, max_drawdown) == 32 && offsetof(gte_backtest_stats, ep_return_sum) == 48 &&
              offsetof(gte_backtest_stats, ep_return_sq_sum) == 56 && offsetof(gte_backtest_stats, trades) == 80 &&
              offsetof(gte_backtest_stats, episodes) == 84 && offsetof(gte_backtest_stats, terminations) == 88,
              "gte_backtest_stats: the pieces the reduction reads (include/gte.h)");
static_assert(sizeof(gte_strategy_stats) == 128 && offsetof(gte_strategy_stats, reward_sum) == 8 &&
              offsetof(gte_strategy_stats, reward_sq_sum) == 16 && offsetof(gte_strategy_stats, ep_return_sum) == 24 &&
              offsetof(gte_strategy_stats, ep_return_sq_sum) == 32 && offsetof(gte_strategy_stats, max_drawdown) == 40 &&
              offsetof(gte_strategy_stats, best_reward_sum) == 48 && offsetof(gte_strategy_stats, worst_reward_sum) == 56 &&
              offsetof(gte_strategy_stats, trades) == 64 && offsetof(gte_strategy_stats, episodes) == 72 &&
              offsetof(gte_strategy_stats, terminations) == 80 && offsetof(gte_strategy_stats, envs) == 88 &&
              offsetof(gte_strategy_stats, envs_stepped) == 92 && offsetof(gte_strategy_stats, reserved) == 96,
              "gte_strategy_stats: 128 bytes (include/gte.h)");

constexpr int ST_WAVES = 4;          // wavefronts per workgroup of the reduction
constexpr int SEL_TILE = 1024;       // candidates a workgroup sorts
constexpr int SEL_THREADS = 256;
constexpr int SEL_KEEP = 256;        // ... and keeps (>= GTE_RANK_MAX)
static_assert(SEL_KEEP >= GTE_RANK_MAX && SEL_TILE >= 2 * SEL_KEEP, "a tile keeps at least k and shrinks the list");

__device__ __forceinline__ double st_f64(unsigned long long u) { return __longlong_as_double((long long)u); }
__device__ __forceinline__ unsigned long long st_u64(double d) { return (unsigned long long)__double_as_longlong(d); }

// Input pieces (gte_backtest_stats): 0 = steps | reward_sum, 1 = reward_sq_sum | peak, 2 = max_drawdown |
// cur_return, 3 = ep_return_sum | ep_return_sq_sum, 5 = trades, episodes | terminations, ended.  Every lane
// runs the same few operations on its piece (both halves summed as f64, the integer readings summed as
// i64, the maximum and the extremes followed); what a piece's lane computed on halves that are not of
// that type is never read.

// piece c of the member at place m, or zeros (which add nothing anywhere) when the place is past the list's
// end or names no env in [0, N); *ok says which.  The load itself always happens, at record 0 if need be
__device__ __forceinline__ st_u2 st_load(const gte_backtest_stats* rec, int N, int S, const Members& g,
                                         const int32_t* envs, int m, int c, bool* ok) {
  const bool in = m < g.n;
  long long e;
  if (envs) {
    const int id = envs[g.lo + (in ? m : 0)];  // (only called with g.n > 0: place 0 exists)
    *ok = in && (unsigned)id < (unsigned)N;
    e = id;
  } else {
    *ok = in;
    e = g.first + (long long)m * S;
  }
  const st_u2 v = reinterpret_cast<const st_u2*>(rec + (*ok ? e : 0))[c];
  st_u2 z;
  z.x = *ok ? v.x : 0ull;
  z.y = *ok ? v.y : 0ull;
  return z;
}

// what a lane follows of its piece besides the two f64 sums: order-free, but for which of two equal extremes
// stays — the one met first in MEMBER order, so the place travels with the value
struct StFold {
  long long k0 = 0, k1 = 0, k2 = 0;
  int cnt = 0, stepped = 0;
  double mx = 0.0, best = -__builtin_inf(), worst = __builtin_inf();
  int best_at = INT32_MAX, worst_at = INT32_MAX;
  // one member of the lane's own, at place m (a lane meets its members by increasing place)
  __device__ __forceinline__ void add(int c, bool ok, const st_u2& v, int m) {
    const double fx = st_f64(v.x), fy = st_f64(v.y);
    k0 += c == 0 ? (long long)v.x : (long long)(int32_t)(uint32_t)v.x;  // steps | trades
    k1 += (int32_t)(uint32_t)(v.x >> 32);                               // episodes
    k2 += (int32_t)(uint32_t)v.y;                                       // terminations
    cnt += ok ? 1 : 0;
    const bool st = (long long)v.x > 0;                                 // piece 0: steps > 0
    stepped += st ? 1 : 0;
    if (fx > mx) mx = fx;                                               // piece 2: max_drawdown
    if (st && fy > best) { best = fy; best_at = m; }                    // piece 0: reward_sum
    if (st && fy < worst) { worst = fy; worst_at = m; }
  }
  __device__ __forceinline__ void join(const StFold& o) {
    k0 += o.k0; k1 += o.k1; k2 += o.k2; cnt += o.cnt; stepped += o.stepped;
    if (o.mx > mx) mx = o.mx;
    if (o.best > best || (o.best == best && o.best_at < best_at)) { best = o.best; best_at = o.best_at; }
    if (o.worst < worst || (o.worst == worst && o.worst_at < worst_at)) { worst = o.worst; worst_at = o.worst_at; }
  }
  __device__ __forceinline__ StFold of_lane(int from) const {
    StFold o;
    o.k0 = __shfl(k0, from, 64); o.k1 = __shfl(k1, from, 64); o.k2 = __shfl(k2, from, 64);
    o.cnt = __shfl(cnt, from, 64); o.stepped = __shfl(stepped, from, 64);
    o.mx = __shfl(mx, from, 64); o.best = __shfl(best, from, 64); o.worst = __shfl(worst, from, 64);
    o.best_at = __shfl(best_at, from, 64); o.worst_at = __shfl(worst_at, from, 64);
    return o;
  }
};

// The output record's pieces, gathered from the lanes gbase + c of the input pieces that hold them (D0 / D1:
// the closed sums of the piece's halves), and stored by the lanes for which `store` holds: 16 bytes each
__device__ __forceinline__ void st_store(gte_strategy_stats* dst, bool store, int gbase, int c, double D0, double D1,
                                         const StFold& f) {
  const unsigned long long steps = (unsigned long long)__shfl(f.k0, gbase + 0, 64);
  const unsigned long long reward_sum = st_u64(__shfl(D1, gbase + 0, 64));
  const unsigned long long reward_sq = st_u64(__shfl(D0, gbase + 1, 64));
  const unsigned long long ep_sum = st_u64(__shfl(D0, gbase + 3, 64));
  const unsigned long long ep_sq = st_u64(__shfl(D1, gbase + 3, 64));
  const unsigned long long max_dd = st_u64(__shfl(f.mx, gbase + 2, 64));
  const unsigned long long best_u = st_u64(__shfl(f.best, gbase + 0, 64));
  const unsigned long long worst_u = st_u64(__shfl(f.worst, gbase + 0, 64));
  const unsigned long long trades = (unsigned long long)__shfl(f.k0, gbase + 5, 64);
  const unsigned long long episodes = (unsigned long long)__shfl(f.k1, gbase + 5, 64);
  const unsigned long long terms = (unsigned long long)__shfl(f.k2, gbase + 5, 64);
  const unsigned long long counts = (unsigned long long)(uint32_t)f.cnt |
                                    ((unsigned long long)(uint32_t)__shfl(f.stepped, gbase + 0, 64) << 32);
  st_u2 o;
  o.x = c == 0 ? steps : c == 1 ? reward_sq : c == 2 ? ep_sq : c == 3 ? best_u : c == 4 ? trades : c == 5 ? terms : 0ull;
  o.y = c == 0 ? reward_sum : c == 1 ? ep_sum : c == 2 ? max_dd : c == 3 ? worst_u : c == 4 ? episodes : c == 5 ? counts : 0ull;
  if (store) reinterpret_cast<st_u2*>(dst)[c] = o;
}

// Eight strategies per wavefront: lane (g, c) folds piece c of strategy 8 * wave + g, all eight accumulators
// in its own registers; a pass is eight places, eight loads in flight.
__global__ __launch_bounds__(64 * ST_WAVES) void gte_strategy_reduce_kernel(
    const gte_backtest_stats* __restrict__ rec, int N, int S, unsigned first_shift,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ envs, gte_strategy_stats* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int c = lane & 7;
  const long long s64 = ((long long)blockIdx.x * ST_WAVES + (threadIdx.x >> 6)) * 8 + (lane >> 3);
  const bool live = s64 < S;
  const int s = live ? (int)s64 : 0;
  Members g = members_of(s, N, S, first_shift, offsets);
  if (!live) g.n = 0;

  double d0[8], d1[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) d0[a] = d1[a] = 0.0;
  StFold f;
  for (int base = 0; base < g.n; base += 8) {
    st_u2 v[8];
    bool ok[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) v[a] = st_load(rec, N, S, g, envs, base + a, c, &ok[a]);
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      d0[a] += st_f64(v[a].x);
      d1[a] += st_f64(v[a].y);
      f.add(c, ok[a], v[a], base + a);
    }
  }
  double D0 = d0[0], D1 = d1[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) { D0 = D0 + d0[i]; D1 = D1 + d1[i]; }
  st_store(out + s, live, lane & ~7, c, D0, D1, f);
}

// One strategy per workgroup of EIGHT wavefronts: wavefront w is accumulator w and owns the places
// w, w + 8, w + 16, ...; lane (q, c) loads piece c of the wave's q-th, (q + 8)-th, ... place of a pass, so one
// load instruction fetches eight members and BLK_FLIGHT of them are in flight (a pass of the workgroup is
// 64 * BLK_FLIGHT places).  The accumulator stays ONE chain: after the loads every lane adds the eight
// slots' values of its piece one after the other, read across lanes in place order (the eight lanes of a
// piece run the same chain).  The eight accumulators and the order-free parts meet through LDS (5 KiB),
// where wavefront 0 closes them in the stated order — the one place of the reduction with a barrier: the
// alternative, one wavefront per strategy, leaves most of the chip idle when the strategies are few.
constexpr int BLK_WAVES = 8;
constexpr int BLK_FLIGHT = 4;
__global__ __launch_bounds__(64 * BLK_WAVES) void gte_strategy_reduce_block_kernel(
    const gte_backtest_stats* __restrict__ rec, int N, int S, unsigned first_shift,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ envs, gte_strategy_stats* __restrict__ out) {
  __shared__ double sh_f[BLK_WAVES][8][5];       // D0, D1, mx, best, worst
  __shared__ long long sh_k[BLK_WAVES][8][3];    // k0, k1, k2
  __shared__ int sh_i[BLK_WAVES][8][4];          // cnt, stepped, best_at, worst_at
  const int lane = threadIdx.x & 63;
  const int c = lane & 7, q = lane >> 3;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int s = blockIdx.x;  // (the grid is S workgroups)
  const Members g = members_of(s, N, S, first_shift, offsets);
  const int mine = g.n > w ? (g.n - w + 7) / 8 : 0;  // places of this accumulator: w + 8 t, t < mine

  double a0 = 0.0, a1 = 0.0;
  StFold f;
  for (int tb = 0; tb < mine; tb += 8 * BLK_FLIGHT) {
    st_u2 v[BLK_FLIGHT];
    bool ok[BLK_FLIGHT];
#pragma unroll
    for (int u = 0; u < BLK_FLIGHT; ++u) {
      const int t = tb + 8 * u + q;
      // (a slot past the accumulator's last place asks for a place past the list's end: zeros)
      v[u] = st_load(rec, N, S, g, envs, t < mine ? w + 8 * t : g.n, c, &ok[u]);
    }
#pragma unroll
    for (int u = 0; u < BLK_FLIGHT; ++u) {
      f.add(c, ok[u], v[u], w + 8 * (tb + 8 * u + q));
      const double fx = st_f64(v[u].x), fy = st_f64(v[u].y);
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) {  // the chain, in place order
        a0 = a0 + __shfl(fx, 8 * qq + c, 64);
        a1 = a1 + __shfl(fy, 8 * qq + c, 64);
      }
    }
  }
  // the wave's order-free parts over its eight slots, then everything of piece c into LDS
  StFold fw = f.of_lane(c);
#pragma unroll
  for (int i = 1; i < 8; ++i) fw.join(f.of_lane(8 * i + c));
  if (q == 0) {
    sh_f[w][c][0] = a0; sh_f[w][c][1] = a1; sh_f[w][c][2] = fw.mx; sh_f[w][c][3] = fw.best; sh_f[w][c][4] = fw.worst;
    sh_k[w][c][0] = fw.k0; sh_k[w][c][1] = fw.k1; sh_k[w][c][2] = fw.k2;
    sh_i[w][c][0] = fw.cnt; sh_i[w][c][1] = fw.stepped; sh_i[w][c][2] = fw.best_at; sh_i[w][c][3] = fw.worst_at;
  }
  __syncthreads();
  if (w != 0) return;
  double D0 = sh_f[0][c][0], D1 = sh_f[0][c][1];
  StFold all;
#pragma unroll
  for (int i = 0; i < BLK_WAVES; ++i) {
    if (i > 0) { D0 = D0 + sh_f[i][c][0]; D1 = D1 + sh_f[i][c][1]; }
    StFold o;
    o.mx = sh_f[i][c][2]; o.best = sh_f[i][c][3]; o.worst = sh_f[i][c][4];
    o.k0 = sh_k[i][c][0]; o.k1 = sh_k[i][c][1]; o.k2 = sh_k[i][c][2];
    o.cnt = sh_i[i][c][0]; o.stepped = sh_i[i][c][1]; o.best_at = sh_i[i][c][2]; o.worst_at = sh_i[i][c][3];
    all.join(o);
  }
  st_store(out + s, q == 0, 0, c, D0, D1, all);
}

hipError_t launch_reduce_strategies(const gte_backtest_stats* records, int n_envs, int n_strategies,
                                    int64_t env_id_base, const int32_t* group_offsets, const int32_t* group_envs,
                                    gte_strategy_stats* out, hipStream_t stream) {
  if (!records || !out || n_envs < 1 || n_strategies < 1 || (group_offsets == nullptr) != (group_envs == nullptr))
    return hipErrorInvalidValue;
  const int64_t S = n_strategies;
  const unsigned first_shift = members_first_shift(env_id_base, S);
  // a workgroup per strategy once the average list has 32 members (half of what one load instruction of its
  // eight wavefronts fetches); speed only: the records do not depend on it
  if ((int64_t)n_envs >= 32 * S)
    hipLaunchKernelGGL(gte_strategy_reduce_block_kernel, dim3((unsigned)S), dim3(64 * BLK_WAVES), 0, stream, records,
                       n_envs, n_strategies, first_shift, group_offsets, group_envs, out);
  else
    hipLaunchKernelGGL(gte_strategy_reduce_kernel, dim3((unsigned)(((S + 7) / 8 + ST_WAVES - 1) / ST_WAVES)),
                       dim3(64 * ST_WAVES), 0, stream, records, n_envs, n_strategies, first_shift, group_offsets,
                       group_envs, out);
  return hipGetLastError();
}

// ---- ranking

__global__ __launch_bounds__(256) void gte_strategy_score_kernel(const gte_strategy_stats* __restrict__ stats, int S,
                                                                 int metric, long long min_episodes,
                                                                 double* __restrict__ scores,
                                                                 double* __restrict__ cand_score,
                                                                 int32_t* __restrict__ cand_index) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const gte_strategy_stats& t = stats[s];
  const long long steps = t.steps, episodes = t.episodes;
  double score;
  if (metric == GTE_METRIC_NEG_MAX_DRAWDOWN) {
    score = -t.max_drawdown;
  } else if (metric == GTE_METRIC_WORST_REWARD_SUM) {
    score = t.worst_reward_sum;
  } else {
    const bool per_step = metric == GTE_METRIC_MEAN_REWARD || metric == GTE_METRIC_SHARPE;
    const double count = (double)(per_step ? steps : episodes);
    const double m = (per_step ? t.reward_sum : t.ep_return_sum) / count;
    score = m;
    if (metric == GTE_METRIC_SHARPE || metric == GTE_METRIC_EPISODE_SHARPE) {
      const double q = (per_step ? t.reward_sq_sum : t.ep_return_sq_sum) / count;
      double v = q - m * m;
      if (!(v > 0.0)) v = 0.0;
      score = m / sqrt(v);
    }
  }
  if (scores) scores[s] = score;
  const bool ranked = steps >= 1 && episodes >= min_episodes && score == score;
  cand_score[s] = ranked ? score : __builtin_nan("");
  cand_index[s] = ranked ? (int32_t)s : -1;
}

// candidate a stands before candidate b (an unranked one, index -1, stands behind every ranked one)
__device__ __forceinline__ bool sel_before(double as, int32_t ai, double bs, int32_t bi) {
  return ai >= 0 && (bi < 0 || as > bs || (as == bs && ai < bi));
}

__global__ __launch_bounds__(SEL_THREADS) void gte_strategy_select_kernel(const double* __restrict__ in_score,
                                                                          const int32_t* __restrict__ in_index,
                                                                          long long n, double* __restrict__ out_score,
                                                                          int32_t* __restrict__ out_index, int keep) {
  __shared__ double ls[SEL_TILE];
  __shared__ int32_t li[SEL_TILE];
  const long long base = (long long)blockIdx.x * SEL_TILE;
  for (int j = threadIdx.x; j < SEL_TILE; j += SEL_THREADS) {
    const bool in = base + j < n;
    ls[j] = in ? in_score[base + j] : __builtin_nan("");
    li[j] = in ? in_index[base + j] : -1;
  }
  for (int k = 2; k <= SEL_TILE; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int p = threadIdx.x; p < SEL_TILE / 2; p += SEL_THREADS) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
        const double as = ls[i], bs = ls[l];
        const int32_t ai = li[i], bi = li[l];
        const bool forward = (i & k) == 0;
        if (forward ? sel_before(bs, bi, as, ai) : sel_before(as, ai, bs, bi)) {
          ls[i] = bs; ls[l] = as;
          li[i] = bi; li[l] = ai;
        }
      }
    }
  __syncthreads();
  for (int j = threadIdx.x; j < keep; j += SEL_THREADS) {
    const int32_t idx = li[j];
    out_score[(long long)blockIdx.x * keep + j] = idx >= 0 ? ls[j] : __builtin_nan("");
    out_index[(long long)blockIdx.x * keep + j] = idx;
  }
}

int64_t rank_scratch_entries(int n_strategies, int which) {
  const int64_t S = n_strategies;
  return which == 0 ? S : (S + SEL_TILE - 1) / SEL_TILE * SEL_KEEP;
}

hipError_t launch_rank_strategies(const gte_strategy_stats* stats, int n_strategies, int metric, int64_t min_episodes,
                                  int k, int32_t* top_index, double* top_score, double* scores, double* const* cand_score,
                                  int32_t* const* cand_index, hipStream_t stream) {
  if (!stats || !top_index || !top_score || n_strategies < 1 || k < 1 || k > GTE_RANK_MAX || k > SEL_TILE ||
      !cand_score[0] || !cand_score[1] || !cand_index[0] || !cand_index[1])
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_strategy_score_kernel, dim3((unsigned)(((int64_t)n_strategies + 255) / 256)), dim3(256), 0, stream,
                     stats, n_strategies, metric, (long long)min_episodes, scores, cand_score[0], cand_index[0]);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : launch_rank_select(n_strategies, k, top_index, top_score, cand_score, cand_index, stream);
}

// the k best of the S candidates a score kernel left in list 0 (a score and an index each; NaN, -1: not ranked)
hipError_t launch_rank_select(int n_strategies, int k, int32_t* top_index, double* top_score, double* const* cand_score,
                              int32_t* const* cand_index, hipStream_t stream) {
  if (!top_index || !top_score || n_strategies < 1 || k < 1 || k > GTE_RANK_MAX || k > SEL_TILE || !cand_score[0] ||
      !cand_score[1] || !cand_index[0] || !cand_index[1])
    return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  // list 0 holds S candidates and list 1 what a pass over S leaves (rank_scratch_entries); every pass
  // keeps SEL_KEEP of each SEL_TILE, so a later pass fits whichever list it writes
  int64_t n = n_strategies;
  int cur = 0;
  while (e == hipSuccess && n > SEL_TILE) {
    const int64_t tiles = (n + SEL_TILE - 1) / SEL_TILE;
    hipLaunchKernelGGL(gte_strategy_select_kernel, dim3((unsigned)tiles), dim3(SEL_THREADS), 0, stream, cand_score[cur],
                       cand_index[cur], (long long)n, cand_score[cur ^ 1], cand_index[cur ^ 1], SEL_KEEP);
    e = hipGetLastError();
    n = tiles * SEL_KEEP;
    cur ^= 1;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gte_strategy_select_kernel, dim3(1), dim3(SEL_THREADS), 0, stream, cand_score[cur], cand_index[cur],
                     (long long)n, top_score, top_index, k);
  return hipGetLastError();
}

}  // namespace gte
