// gte_diversify.hip — a decorrelated leaderboard picked greedily on the device (gte_diversify, include/gte.h): the best
// strategy by the caller's scores, everything that correlates with it above a threshold dropped, the best of what is
// left, and so on for k rounds, from the S * B strategy period records.  Own translation unit, beside
// gte_bootstrap.hip and gte_cscv.hip: nothing here can perturb the code of another.
//
//   gte_div_prepare_kernel  one lane per strategy: eligibility, its standardised row into the dense transposed staging
//             array U[n][S] (a lane's u_i then lie S apart, a wavefront's side by side), its live byte, owner and
//             owner_corr as they stand before any round; per workgroup the best live (score, index) into partial
//             list 0 and the counts of eligible and candidate strategies.
//   gte_div_round_kernel    THE HOT PATH, one launch per round.  Every workgroup closes the previous launch's partial
//             list to the same pick (the comparator is a total order: any order of reduction gives the same entry),
//             puts U[:, pick] into LDS, and a lane whose strategy is live walks i ascending, c = c + u_i[s] * u_i[pick]
//             in one lane: the bits do not depend on the geometry.  A wavefront without a live lane issues no load of
//             U; a workgroup without one does not even look for the pick.  The lane updates live, owner, owner_corr;
//             the workgroup writes its best remaining candidate to the OTHER partial list and its counts of leavers
//             and of live lanes.  Workgroup 0 writes pick[r] and pick_score[r].
//   gte_div_close_kernel    workgroup a: row a of pick_corr, U[:, pick[a]] in LDS, thread b against pick[b];
//             workgroup 0 also cluster_size (the workgroups' counts added as integers) and the summary.
//
// The launch boundary is the only device-wide ordering: no atomics, no grid barrier, no scratch memory.
// What may be read: stats[s * B + b] for s < S and b a selected period < B (steps and reward_sum alone);
// scores[s] for s < S; the scratch and the outputs as written by the kernels before.  What is written: the outputs
// gte.h lists, and the library's scratch (DivScratch).
#include "gte_launch.h"
#include "gte_members.h"

namespace gte {

constexpr int DIV_TILE = 256;         // strategies of a workgroup, one per lane
constexpr int DIV_BATCH = 8;          // loads a lane of the prepare kernel issues before it uses the first
constexpr int DIV_ROUND_BATCH = 16;   // the same in a round
static_assert(sizeof(gte_diversify_summary) == 20, "gte_diversify_summary: 20 bytes (include/gte.h)");
static_assert(GTE_RANK_MAX <= DIV_TILE && GTE_MAX_PERIODS <= DIV_TILE, "the close: a thread per pick, per period");

// entry (s2, i2) takes the place of (s1, i1): an index below 0 is no entry; a higher score, or the same score at a
// lower index (-0.0 == 0.0, by comparison; no score here is NaN).  A total order on the entries.
__device__ __forceinline__ bool div_better(double s2, int i2, double s1, int i1) {
  return i2 >= 0 && (i1 < 0 || s2 > s1 || (s2 == s1 && i2 < i1));
}

// what a workgroup reduces: its best entry and two integer sums
struct DivShared {
  double score[DIV_TILE];
  int32_t index[DIV_TILE], a[DIV_TILE], b[DIV_TILE];
};

// the workgroup's best entry and sums into sh.*[0]; every thread calls, every thread may read [0] afterwards
__device__ __forceinline__ void div_reduce(DivShared& sh, int tid, double score, int index, int a, int b) {
  sh.score[tid] = score;
  sh.index[tid] = index;
  sh.a[tid] = a;
  sh.b[tid] = b;
  __syncthreads();
  for (int half = DIV_TILE / 2; half > 0; half >>= 1) {
    if (tid < half) {
      if (div_better(sh.score[tid + half], sh.index[tid + half], sh.score[tid], sh.index[tid])) {
        sh.score[tid] = sh.score[tid + half];
        sh.index[tid] = sh.index[tid + half];
      }
      sh.a[tid] += sh.a[tid + half];
      sh.b[tid] += sh.b[tid + half];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(DIV_TILE) void gte_div_prepare_kernel(
    const gte_strategy_period_stats* __restrict__ stats, int S, int B, const PeriodMask mask, int n,
    const double* __restrict__ scores, double* U, uint8_t* __restrict__ live, int32_t* __restrict__ owner,
    double* __restrict__ owner_corr, double* __restrict__ pscore, int32_t* __restrict__ pindex,
    int32_t* __restrict__ wg_eligible, int32_t* __restrict__ wg_candidates, int32_t* __restrict__ wg_live) {
  __shared__ DivShared sh;
  const int tid = threadIdx.x;
  const long long s = (long long)blockIdx.x * DIV_TILE + tid;
  bool elig = false, cand = false;
  double sc = 0.0;
  if (s < S) {
    const gte_strategy_period_stats* t = stats + s * B;
    double* col = U + s;  // (this lane's own column: what it reads back below it has written itself)
    bool ok = true;
    double sum = 0.0;
    // DIV_BATCH loads are issued before the first of them is used, in all three passes: a lane's records lie B * 48
    // bytes from its neighbour's, and one load at a time would be one memory latency per period.  The chains stay i
    // ascending; what is left after the last whole batch goes one at a time.  The selected periods are taken off the
    // mask's words lowest first (uniform: scalar registers).
    uint64_t w0 = mask.w[0], w1 = mask.w[1];
    auto next_period = [&]() {  // (called n times in all: a bit is left whenever it is called)
      int b;
      if (w0) {
        b = __builtin_ctzll(w0);
        w0 &= w0 - 1;
      } else {
        b = 64 + __builtin_ctzll(w1);
        w1 &= w1 - 1;
      }
      return b;
    };
    int i = 0;
    for (; i + DIV_BATCH <= n; i += DIV_BATCH) {
      double x[DIV_BATCH];
      long long steps[DIV_BATCH];
#pragma unroll
      for (int j = 0; j < DIV_BATCH; ++j) {
        const int b = next_period();
        x[j] = t[b].reward_sum;
        steps[j] = t[b].steps;
      }
#pragma unroll
      for (int j = 0; j < DIV_BATCH; ++j) {
        ok = ok && steps[j] > 0 && __builtin_isfinite(x[j]);
        col[(long long)(i + j) * S] = x[j];
        sum = sum + x[j];
      }
    }
    for (; i < n; ++i) {
      const int b = next_period();
      const double x = t[b].reward_sum;
      ok = ok && t[b].steps > 0 && __builtin_isfinite(x);
      col[(long long)i * S] = x;
      sum = sum + x;
    }
    const double m = sum / (double)n;
    double q = 0.0;
    for (i = 0; i + DIV_BATCH <= n; i += DIV_BATCH) {
      double x[DIV_BATCH];
#pragma unroll
      for (int j = 0; j < DIV_BATCH; ++j) x[j] = col[(long long)(i + j) * S];
#pragma unroll
      for (int j = 0; j < DIV_BATCH; ++j) {
        const double e = x[j] - m;
        q = q + e * e;
      }
    }
    for (; i < n; ++i) {
      const double e = col[(long long)i * S] - m;
      q = q + e * e;
    }
    const double norm = sqrt(q);
    for (i = 0; i + DIV_BATCH <= n; i += DIV_BATCH) {
      double x[DIV_BATCH];
#pragma unroll
      for (int j = 0; j < DIV_BATCH; ++j) x[j] = col[(long long)(i + j) * S];
#pragma unroll
      for (int j = 0; j < DIV_BATCH; ++j) {
        const double e = x[j] - m;
        col[(long long)(i + j) * S] = e / norm;
      }
    }
    for (; i < n; ++i) {
      const double e = col[(long long)i * S] - m;
      col[(long long)i * S] = e / norm;
    }
    elig = ok && __builtin_isfinite(q) && q > 0.0;
    sc = scores[s];
    cand = elig && sc == sc;
    live[s] = cand ? 1 : 0;
    owner[s] = cand ? -1 : -2;
    owner_corr[s] = __builtin_nan("");
  }
  div_reduce(sh, tid, sc, cand ? (int)s : -1, elig ? 1 : 0, cand ? 1 : 0);
  if (tid == 0) {
    pscore[blockIdx.x] = sh.score[0];
    pindex[blockIdx.x] = sh.index[0];
    wg_eligible[blockIdx.x] = sh.a[0];
    wg_candidates[blockIdx.x] = sh.b[0];
    wg_live[blockIdx.x] = sh.b[0];
  }
}

__global__ __launch_bounds__(DIV_TILE) void gte_div_round_kernel(
    const double* __restrict__ U, const double* __restrict__ scores, int S, int n, int round, double max_corr,
    int tiles, const double* __restrict__ pscore_in, const int32_t* __restrict__ pindex_in,
    double* __restrict__ pscore_out, int32_t* __restrict__ pindex_out, uint8_t* __restrict__ live,
    int32_t* __restrict__ owner, double* __restrict__ owner_corr, int32_t* __restrict__ wg_left,
    int32_t* __restrict__ wg_live, int32_t* __restrict__ pick, double* __restrict__ pick_score) {
  __shared__ DivShared sh;
  __shared__ double pcol[GTE_MAX_PERIODS];
  __shared__ int wave_live[DIV_TILE / 64];  // whether a wavefront has a live lane
  const int tid = threadIdx.x, tile = blockIdx.x;
  const long long s = (long long)tile * DIV_TILE + tid;
  bool alive = s < S && live[s] != 0;
  // What does not wait for the pick is loaded first, all of it in flight at once, because a round is a chain of
  // memory latencies (live, the list, the pick's column, the lane's column) and little else: this thread's entries
  // of the previous launch's partial list, the lane's score, and the head of its column.
  double bs = 0.0;
  int bi = -1;
  for (int t = tid; t < tiles; t += DIV_TILE) {
    const double ps = pscore_in[t];
    const int pi = pindex_in[t];
    if (div_better(ps, pi, bs, bi)) {
      bs = ps;
      bi = pi;
    }
  }
  const double* col = U + (alive ? s : 0);
  const bool headed = alive && n >= DIV_ROUND_BATCH;  // (a wavefront without a live lane issues no load of U)
  double own = 0.0, head[DIV_ROUND_BATCH];
#pragma unroll
  for (int j = 0; j < DIV_ROUND_BATCH; ++j) head[j] = 0.0;
  if (alive) own = scores[s];
  if (headed) {
#pragma unroll
    for (int j = 0; j < DIV_ROUND_BATCH; ++j) head[j] = col[(long long)j * S];
  }
  const unsigned long long live_lanes = __ballot(alive);  // (by the whole wavefront, before its lane 0 alone stores)
  if ((tid & 63) == 0) wave_live[tid >> 6] = live_lanes != 0 ? 1 : 0;
  __syncthreads();
  int any = 0;
#pragma unroll
  for (int w = 0; w < DIV_TILE / 64; ++w) any |= wave_live[w];
  if (!any && tile != 0) {  // nothing of this workgroup's is live: the pick is not its business
    if (tid == 0) {
      pscore_out[tile] = 0.0;
      pindex_out[tile] = -1;
      wg_left[tile] = 0;
      wg_live[tile] = 0;
    }
    return;
  }
  // the partial list, closed to the same entry by every workgroup
  div_reduce(sh, tid, bs, bi, 0, 0);
  const double p_score = sh.score[0];
  const int p = sh.index[0];
  __syncthreads();  // (sh is written again below)
  if (tile == 0 && tid == 0) {
    pick[round] = p;
    pick_score[round] = p >= 0 ? p_score : __builtin_nan("");
  }
  int left = 0;
  if (p >= 0) {  // (p < 0: no candidate is live anywhere, so none is here)
    if (tid < n) pcol[tid] = U[(long long)tid * S + p];
    __syncthreads();
    if (alive) {  // a wavefront without a live lane branches over the loads
      double c = 0.0;
      // DIV_ROUND_BATCH loads in flight per lane: a round runs at a wavefront per SIMD or less, so the loads of ONE
      // wavefront have to cover the latency of the staged matrix (the chain itself stays i ascending; what is left
      // after the last whole batch goes one at a time)
      int i = 0;
      if (headed) {
#pragma unroll
        for (int j = 0; j < DIV_ROUND_BATCH; ++j) c = c + head[j] * pcol[j];
        i = DIV_ROUND_BATCH;
      }
      for (; i + DIV_ROUND_BATCH <= n; i += DIV_ROUND_BATCH) {
        double u[DIV_ROUND_BATCH];
#pragma unroll
        for (int j = 0; j < DIV_ROUND_BATCH; ++j) u[j] = col[(long long)(i + j) * S];
#pragma unroll
        for (int j = 0; j < DIV_ROUND_BATCH; ++j) c = c + u[j] * pcol[i + j];
      }
      for (; i < n; ++i) c = c + col[(long long)i * S] * pcol[i];
      if (s == p || c > max_corr) {
        live[s] = 0;
        owner[s] = round;
        owner_corr[s] = c;
        alive = false;
        left = 1;
      }
    }
  }
  div_reduce(sh, tid, alive ? own : 0.0, alive ? (int)s : -1, left, alive ? 1 : 0);
  if (tid == 0) {
    pscore_out[tile] = sh.score[0];
    pindex_out[tile] = sh.index[0];
    wg_left[tile] = sh.a[0];
    wg_live[tile] = sh.b[0];
  }
}

__global__ __launch_bounds__(DIV_TILE) void gte_div_close_kernel(
    const double* __restrict__ U, int S, int n, int k, int tiles, const int32_t* __restrict__ pick,
    const int32_t* __restrict__ wg_left, const int32_t* __restrict__ wg_eligible,
    const int32_t* __restrict__ wg_candidates, const int32_t* __restrict__ wg_live, double* __restrict__ pick_corr,
    int32_t* __restrict__ cluster_size, gte_diversify_summary* __restrict__ summary) {
  __shared__ DivShared sh;
  __shared__ double pcol[GTE_MAX_PERIODS];
  const int tid = threadIdx.x, a = blockIdx.x;
  const int pa = pick[a];
  if (pa >= 0 && tid < n) pcol[tid] = U[(long long)tid * S + pa];
  __syncthreads();
  const int pb = tid < k ? pick[tid] : -1;
  if (tid < k) {
    double c = __builtin_nan("");
    if (pa >= 0 && pb >= 0) {
      const double* col = U + pb;
      c = 0.0;
      int i = 0;
      for (; i + DIV_ROUND_BATCH <= n; i += DIV_ROUND_BATCH) {  // (batched as in a round)
        double u[DIV_ROUND_BATCH];
#pragma unroll
        for (int j = 0; j < DIV_ROUND_BATCH; ++j) u[j] = col[(long long)(i + j) * S];
#pragma unroll
        for (int j = 0; j < DIV_ROUND_BATCH; ++j) c = c + pcol[i + j] * u[j];
      }
      for (; i < n; ++i) c = c + pcol[i] * col[(long long)i * S];
    }
    pick_corr[(long long)a * k + tid] = c;
  }
  if (a != 0) return;
  // round `tid`: the workgroups' counts of leavers, tile ascending (integers: any order gives the same)
  if (tid < k) {
    int size = 0;
    const int32_t* row = wg_left + (long long)tid * tiles;
    for (int t = 0; t < tiles; ++t) size += row[t];
    cluster_size[tid] = size;
  }
  int elig = 0, cands = 0, remaining = 0;
  for (int t = tid; t < tiles; t += DIV_TILE) {
    elig += wg_eligible[t];
    cands += wg_candidates[t];
    remaining += wg_live[t];
  }
  div_reduce(sh, tid, 0.0, -1, elig, cands);
  const int elig_all = sh.a[0], cands_all = sh.b[0];
  __syncthreads();
  div_reduce(sh, tid, 0.0, -1, remaining, pb >= 0 ? 1 : 0);
  if (tid == 0) {
    summary->picked = sh.b[0];
    summary->candidates = cands_all;
    summary->eligible = elig_all;
    summary->remaining = sh.a[0];
    summary->reserved = 0;
  }
}

// the library's scratch of one gte_diversify, carved out of one allocation (ScratchCarver, gte_launch.h)
struct DivScratch {
  double *U, *pscore[2];
  int32_t *pindex[2], *wg_left, *wg_eligible, *wg_candidates, *wg_live;
  uint8_t* live;
  size_t bytes;
};
static DivScratch div_carve(void* base, int64_t S, int n, int k) {
  const size_t tiles = (size_t)((S + DIV_TILE - 1) / DIV_TILE);
  ScratchCarver c = {(char*)base, 0};
  DivScratch d;
  d.U = c.take<double>((size_t)n * (size_t)S);
  for (int j = 0; j < 2; ++j) d.pscore[j] = c.take<double>(tiles);
  for (int j = 0; j < 2; ++j) d.pindex[j] = c.take<int32_t>(tiles);
  d.wg_left = c.take<int32_t>((size_t)k * tiles);
  d.wg_eligible = c.take<int32_t>(tiles);
  d.wg_candidates = c.take<int32_t>(tiles);
  d.wg_live = c.take<int32_t>(tiles);
  d.live = c.take<uint8_t>((size_t)S);
  d.bytes = c.at;
  return d;
}

size_t diversify_scratch_bytes(int n_strategies, int n, int k) { return div_carve(nullptr, n_strategies, n, k).bytes; }

hipError_t launch_diversify(const gte_strategy_period_stats* stats, int n_strategies, int n_periods,
                            const uint64_t period_mask[2], int n, const double* scores, double max_corr, int k,
                            const gte_diversify_out& out, void* scratch, hipStream_t stream) {
  if (!stats || !period_mask || !scores || !scratch || n_strategies < 1 || n_periods < 1 ||
      n_periods > GTE_MAX_PERIODS || n < 3 || n > n_periods || k < 1 || k > GTE_RANK_MAX || max_corr != max_corr ||
      !out.pick || !out.pick_score || !out.cluster_size || !out.owner || !out.owner_corr || !out.pick_corr ||
      !out.summary)
    return hipErrorInvalidValue;
  const int S = n_strategies;
  const int tiles = (int)(((int64_t)S + DIV_TILE - 1) / DIV_TILE);
  const DivScratch d = div_carve(scratch, S, n, k);
  const PeriodMask mask = {{period_mask[0], period_mask[1]}};
  hipLaunchKernelGGL(gte_div_prepare_kernel, dim3((unsigned)tiles), dim3(DIV_TILE), 0, stream, stats, S, n_periods, mask,
                     n, scores, d.U, d.live, out.owner, out.owner_corr, d.pscore[0], d.pindex[0], d.wg_eligible,
                     d.wg_candidates, d.wg_live);
  for (int r = 0; r < k; ++r)  // round r reads partial list r % 2 and writes the other
    hipLaunchKernelGGL(gte_div_round_kernel, dim3((unsigned)tiles), dim3(DIV_TILE), 0, stream, d.U, scores, S, n, r,
                       max_corr, tiles, d.pscore[r & 1], d.pindex[r & 1], d.pscore[(r + 1) & 1], d.pindex[(r + 1) & 1],
                       d.live, out.owner, out.owner_corr, d.wg_left + (size_t)r * (size_t)tiles, d.wg_live, out.pick,
                       out.pick_score);
  hipLaunchKernelGGL(gte_div_close_kernel, dim3((unsigned)k), dim3(DIV_TILE), 0, stream, d.U, S, n, k, tiles, out.pick,
                     d.wg_left, d.wg_eligible, d.wg_candidates, d.wg_live, out.pick_corr, out.cluster_size,
                     out.summary);
  return hipGetLastError();
}

}  // namespace gte
