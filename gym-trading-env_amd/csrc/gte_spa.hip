// gte_spa.hip — Hansen's test for Superior Predictive Ability and its step-down (gte_spa_test, include/gte.h): the
// studentised, recentred maxima over all strategies of their resampled means, resample by resample, and the rounds of
// the step-down, from the S * B strategy period records and what gte_reality_check left of them.  Own translation
// unit, beside gte_bootstrap.hip: nothing here can perturb the code of another.
//
//   gte_spa_prep_kernel     one lane per strategy: d_i into the dense transposed staging array D[n][S] (as
//             gte_boot_gather_kernel makes it), se_s, 1 / se_s, t_s, the three recentrings, the live byte.
//   gte_spa_begin_kernel    one workgroup: the statistic, its lowest index, the studentised strategies; crit and
//             round_rejected cleared; the done flag set at once when nothing is studentised.
//   gte_spa_pass_kernel     THE HOT PATH, 2 * R * S * n f64 operations per round, the structure of
//             gte_boot_resample_kernel.  A lane owns a strategy, a workgroup a tile of SPA_TILE strategies and a slab
//             of GTE_BOOT_SLAB resamples, taken SPA_RC at a time: SPA_RC accumulators per lane, d_i loaded once per
//             chunk, w[r][i] the same for every lane (uniform loads).  Every chain a = a + w * d runs over i
//             ascending in one lane.  It closes NJ recentrings (three in round 0, one later): the chunk's
//             z = (q - g_j) * rse cross the workgroup through LDS, one [SPA_RC][SPA_TILE] plane a recentring at a
//             time (SPA_PLANES == 1) or all at once (SPA_PLANES == 3), for the tile's maximum and its lowest index per
//             resample.  A strategy whose live byte is 0 writes -inf.  The [R, S] matrix is never written.
//   gte_spa_max_kernel      one thread per (recentring, resample): the tiles' maxima in ascending tile order, then
//             the clamp at 0.0.
//   gte_spa_count_kernel    one lane per strategy: the resamples whose consistent maximum reaches t_s.
//   gte_spa_close_kernel    one workgroup, a round's end: (round 0: the three counts against the statistic,) the
//             element of rank crit_rank of the round's maxima by a radix select on their bit patterns (every maximum
//             is >= +0.0 and no NaN: as uint64 they order like the values) a bit at a time, the rejections, the
//             summary's running fields and the done flag.
// Rounds 1 .. max_rounds-1 are enqueued unconditionally; once the done flag is set every workgroup of theirs returns
// before its first load of anything else.  No atomics, no scratch memory, vector stores only.
//
// What may be read: stats[s * B + b] for s < S and b a selected period < B (steps and reward_sum alone);
// benchmark[b] for the same b; w[r * n + i] for r < R, i < n; mean, boot_sum and boot_sq_sum of the reality check
// that ran before; the scratch and the outputs as written by the kernels before.  What is written: the outputs
// gte.h lists, and the library's scratch (SpaScratch).
#include "gte_launch.h"
#include "gte_members.h"

#ifndef GTE_SPA_PLANES
#define GTE_SPA_PLANES 1  // LDS planes of the pass kernel in round 0: 1 (32 KB, reused) or 3 (96 KB); DESIGN.md
#endif

namespace gte {

constexpr int SPA_TILE = 256;  // strategies of a workgroup, one per lane
constexpr int SPA_RC = 16;     // resamples a lane accumulates at a time
constexpr int SPA_PLANES = GTE_SPA_PLANES;
static_assert(GTE_BOOT_SLAB % SPA_RC == 0 && SPA_TILE == 16 * SPA_RC, "the chunk's maxima: 16 lanes per resample");
static_assert(SPA_PLANES == 1 || SPA_PLANES == 3, "one plane reused, or one per recentring");
static_assert(sizeof(gte_spa_summary) == 40, "gte_spa_summary: 40 bytes (include/gte.h)");

// what the rounds hand on, in scratch: written by one thread of a one-workgroup kernel, read by the launches after it
struct SpaState {
  int32_t done;  // the step-down has stopped: every later launch of a round returns at once
  int32_t live;  // strategies still live
  int32_t reserved[2];
};

__global__ __launch_bounds__(256) void gte_spa_prep_kernel(
    const gte_strategy_period_stats* __restrict__ stats, int S, int B, const PeriodMask mask,
    const double* __restrict__ benchmark, const double* __restrict__ mean, const double* __restrict__ boot_sum,
    const double* __restrict__ boot_sq_sum, int R, double threshold, double* __restrict__ D,
    double* __restrict__ rse_out, double* __restrict__ g, uint8_t* __restrict__ live, double* __restrict__ t_stat,
    double* __restrict__ std_error, uint8_t* __restrict__ recentred, int32_t* __restrict__ rejected_round) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const gte_strategy_period_stats* t = stats + s * B;
  bool ok = true;
  int i = 0;
  for (int b = 0; b < B; ++b) {
    if (!mask.has(b)) continue;
    const double x = t[b].reward_sum;
    ok = ok && t[b].steps > 0 && __builtin_isfinite(x);
    D[(long long)i * S + s] = benchmark ? x - benchmark[b] : x;
    ++i;
  }
  const double m = mean[s], dR = (double)R;
  const double m1 = boot_sum[s] / dR;
  const double v = boot_sq_sum[s] / dR - m1 * m1;
  const double se = __builtin_sqrt(v > 0 ? v : 0.0);
  const double rse = 1.0 / se;
  const bool stud = ok && __builtin_isfinite(m) && __builtin_isfinite(se) && se > 0;
  const double ts = m * rse;
  const bool keep = stud && ts >= -threshold;
  const double nan = __builtin_nan("");
  t_stat[s] = stud ? ts : nan;
  std_error[s] = ok ? se : nan;
  recentred[s] = keep ? 1 : 0;
  rejected_round[s] = -1;
  live[s] = stud ? 1 : 0;
  rse_out[s] = stud ? rse : 0.0;
  g[s] = stud && m > 0 ? m : 0.0;
  g[(long long)S + s] = keep ? m : 0.0;
  g[2 * (long long)S + s] = stud ? m : 0.0;
}

// (m2, i2) takes the place of (m1, i1): a larger value, or the same value at a lower index (an index is -1 exactly
// where the value is -inf: nothing compared greater than the start)
__device__ __forceinline__ bool spa_better(double m2, int i2, double m1, int i1) {
  return m2 > m1 || (m2 == m1 && i2 < i1);
}

// the sum of v over the 1024 threads of the workgroup, in every thread (integers: any order gives the same sum)
__device__ __forceinline__ int spa_block_sum(int v, int* part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) total += part[j];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(1024) void gte_spa_begin_kernel(const uint8_t* __restrict__ live,
                                                             const double* __restrict__ t_stat, int S, int max_rounds,
                                                             double* __restrict__ crit,
                                                             int32_t* __restrict__ round_rejected,
                                                             gte_spa_summary* __restrict__ out,
                                                             SpaState* __restrict__ state) {
  __shared__ double sm[1024];
  __shared__ int si[1024], sn[1024];
  const int tid = threadIdx.x;
  double bm = -__builtin_inf();
  int bi = -1, cnt = 0;
  for (long long s = tid; s < S; s += 1024) {  // ascending within the thread: a plain > keeps its lowest index
    if (!live[s]) continue;
    cnt += 1;
    const double v = t_stat[s];
    if (v > bm) {
      bm = v;
      bi = (int)s;
    }
  }
  sm[tid] = bm;
  si[tid] = bi;
  sn[tid] = cnt;
  __syncthreads();
  for (int half = 512; half > 0; half >>= 1) {
    if (tid < half) {
      if (spa_better(sm[tid + half], si[tid + half], sm[tid], si[tid])) {
        sm[tid] = sm[tid + half];
        si[tid] = si[tid + half];
      }
      sn[tid] += sn[tid + half];
    }
    __syncthreads();
  }
  if (tid < max_rounds) {
    crit[tid] = __builtin_nan("");
    round_rejected[tid] = 0;
  }
  if (tid == 0) {
    out->statistic = sm[0] > 0.0 ? sm[0] : 0.0;
    out->best = si[0];
    out->count_lower = 0;
    out->count_consistent = 0;
    out->count_upper = 0;
    out->rounds_run = 0;
    out->num_rejected = 0;
    out->studentised = sn[0];
    out->reserved = 0;
    state->done = sn[0] == 0 ? 1 : 0;
    state->live = sn[0];
    state->reserved[0] = 0;
    state->reserved[1] = 0;
  }
}

// the tile's maximum of resample r0 + k over the plane's row k, and its lowest index: 16 lanes per resample, lane
// `seg` over strategies seg, seg + 16, ... ascending, then the 16
__device__ __forceinline__ void spa_tile_max(const double (*plane)[SPA_TILE], int tid, int tile, int r0, int r_hi,
                                             long long at, double* __restrict__ pmax, int32_t* __restrict__ pidx) {
  const int k = tid >> 4, seg = tid & 15;
  double bm = -__builtin_inf();
  int bi = -1;
#pragma unroll
  for (int j = 0; j < SPA_TILE / 16; ++j) {
    const double v = plane[k][j * 16 + seg];
    if (v > bm) {
      bm = v;
      bi = j * 16 + seg;
    }
  }
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
    const double om = __shfl_xor(bm, off);
    const int oi = __shfl_xor(bi, off);
    if (spa_better(om, oi, bm, bi)) {
      bm = om;
      bi = oi;
    }
  }
  if (seg == 0 && r0 + k < r_hi) {
    pmax[at + r0 + k] = bm;
    pidx[at + r0 + k] = bi >= 0 ? tile * SPA_TILE + bi : -1;
  }
}

// POW2: n is a power of two and `scale` its reciprocal, a * scale IS a / n (both the correctly rounded quotient);
// otherwise `scale` is n and the division is made.  NJ recentrings, g[j][S] from j = J0 on: (3, 0) in round 0,
// (1, 1) later.  PLANES: 1, or NJ.  pmax, pidx: [NJ][tiles][R]
template <bool POW2, int NJ, int J0, int PLANES>
__global__ __launch_bounds__(SPA_TILE) void gte_spa_pass_kernel(
    const SpaState* __restrict__ state, const double* __restrict__ D, const uint8_t* __restrict__ live,
    const double* __restrict__ rse, const double* __restrict__ g, const double* __restrict__ w, int S, int n, int R,
    double scale, double* __restrict__ pmax, int32_t* __restrict__ pidx) {
  __shared__ double sc[PLANES][SPA_RC][SPA_TILE];
  if (J0 != 0 && state->done) return;  // (the same for every lane of the launch)
  const int tid = threadIdx.x, tile = blockIdx.x, slab = blockIdx.y, tiles = gridDim.x;
  const long long s = (long long)tile * SPA_TILE + tid;
  const long long sl = s < S ? s : S - 1;  // a lane past the end reads the last strategy and counts nowhere
  const bool ok = s < S && live[sl] != 0;
  const double rs = rse[sl];
  double gj[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) gj[j] = g[(long long)(J0 + j) * S + sl];
  const int r_lo = slab * GTE_BOOT_SLAB;
  const int r_hi = r_lo + GTE_BOOT_SLAB < R ? r_lo + GTE_BOOT_SLAB : R;
  const double* dcol = D + sl;
  for (int r0 = r_lo; r0 < r_hi; r0 += SPA_RC) {
    double acc[SPA_RC];
    long long row[SPA_RC];  // a chunk past the end reads the last resample's row again; its values are dropped
#pragma unroll
    for (int k = 0; k < SPA_RC; ++k) {
      acc[k] = 0.0;
      row[k] = (long long)(r0 + k < R ? r0 + k : R - 1) * n;
    }
#pragma unroll 2
    for (int i = 0; i < n; ++i) {
      const double d = dcol[(long long)i * S];
#pragma unroll
      for (int k = 0; k < SPA_RC; ++k) acc[k] = acc[k] + w[row[k] + i] * d;
    }
#pragma unroll
    for (int k = 0; k < SPA_RC; ++k) acc[k] = POW2 ? acc[k] * scale : acc[k] / scale;  // q_rs
    if (PLANES == NJ) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < SPA_RC; ++k) sc[j][k][tid] = ok ? (acc[k] - gj[j]) * rs : -__builtin_inf();
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        spa_tile_max(sc[j], tid, tile, r0, r_hi, ((long long)j * tiles + tile) * R, pmax, pidx);
      __syncthreads();
    } else {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int k = 0; k < SPA_RC; ++k) sc[0][k][tid] = ok ? (acc[k] - gj[j]) * rs : -__builtin_inf();
        __syncthreads();
        spa_tile_max(sc[0], tid, tile, r0, r_hi, ((long long)j * tiles + tile) * R, pmax, pidx);
        __syncthreads();
      }
    }
  }
}

// M, I: [NJ][R] (I may be null: the rounds after the first keep no index)
template <bool FIRST>
__global__ __launch_bounds__(256) void gte_spa_max_kernel(const SpaState* __restrict__ state,
                                                          const double* __restrict__ pmax,
                                                          const int32_t* __restrict__ pidx, int tiles, int R, int NJ,
                                                          double* __restrict__ M, int32_t* __restrict__ I) {
  if (!FIRST && state->done) return;
  const int r = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (r >= R || j >= NJ) return;
  double bm = -__builtin_inf();
  int bi = -1;
  for (int t = 0; t < tiles; ++t) {  // ascending tiles are ascending strategies: a plain > keeps the lowest index
    const long long at = ((long long)j * tiles + t) * R + r;
    const double v = pmax[at];
    if (v > bm) {
      bm = v;
      bi = pidx[at];
    }
  }
  M[(long long)j * R + r] = bm > 0.0 ? bm : 0.0;
  if (I) I[(long long)j * R + r] = bi;
}

__global__ __launch_bounds__(256) void gte_spa_count_kernel(const double* __restrict__ t_stat, int S, int R,
                                                            const double* __restrict__ M1,
                                                            int32_t* __restrict__ count_adj) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const double t = t_stat[s];  // NaN unless studentised: no maximum compares >= it
  int adj = 0;
  for (int r = 0; r < R; ++r) adj += M1[r] >= t ? 1 : 0;
  count_adj[s] = adj;
}

// round k's end.  M1: the round's consistent maxima [R]; FIRST: they are row 1 of M3 [3][R], counted against the
// statistic as well
template <bool FIRST>
__global__ __launch_bounds__(1024) void gte_spa_close_kernel(SpaState* __restrict__ state,
                                                             const double* __restrict__ M3,
                                                             const double* __restrict__ M1, int R, int crit_rank,
                                                             int k, int max_rounds, int S,
                                                             const double* __restrict__ t_stat,
                                                             uint8_t* __restrict__ live,
                                                             int32_t* __restrict__ rejected_round,
                                                             double* __restrict__ crit,
                                                             int32_t* __restrict__ round_rejected,
                                                             gte_spa_summary* __restrict__ out) {
  __shared__ int part[16];
  const int done = state->done;
  __syncthreads();  // every thread has read the flag before thread 0 may write it
  if (done) return;
  const int tid = threadIdx.x;
  int counts[3] = {0, 0, 0};
  if (FIRST) {
    const double T = out->statistic;
    for (int r = tid; r < R; r += 1024) {
#pragma unroll
      for (int j = 0; j < 3; ++j) counts[j] += M3[(long long)j * R + r] >= T ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) counts[j] = spa_block_sum(counts[j], part);
  }
  // the element of rank crit_rank: from the top bit down, how many of the values that share the bits decided so far
  // have a 0 in this one
  const unsigned long long* bits = (const unsigned long long*)M1;
  unsigned long long prefix = 0;
  int rank = crit_rank;
  for (int bit = 63; bit >= 0; --bit) {
    const unsigned long long above = bit == 63 ? 0ull : ~0ull << (bit + 1);
    int c = 0;
    for (int r = tid; r < R; r += 1024) {
      const unsigned long long x = bits[r];
      c += (x & above) == prefix && !((x >> bit) & 1) ? 1 : 0;
    }
    c = spa_block_sum(c, part);
    if (rank >= c) {
      rank -= c;
      prefix |= 1ull << bit;
    }
  }
  const double cv = __longlong_as_double((long long)prefix);
  int rej = 0;
  for (long long s = tid; s < S; s += 1024) {
    if (live[s] && t_stat[s] > cv) {
      rejected_round[s] = k;
      live[s] = 0;
      rej += 1;
    }
  }
  rej = spa_block_sum(rej, part);
  if (tid == 0) {
    crit[k] = cv;
    round_rejected[k] = rej;
    if (FIRST) {
      out->count_lower = counts[0];
      out->count_consistent = counts[1];
      out->count_upper = counts[2];
    }
    out->rounds_run = k + 1;
    out->num_rejected = out->num_rejected + rej;
    const int left = state->live - rej;
    state->live = left;
    state->done = rej == 0 || left == 0 || k == max_rounds - 1 ? 1 : 0;
  }
}

// the library's scratch of one gte_spa_test, carved out of one allocation (ScratchCarver, gte_launch.h)
struct SpaScratch {
  double *D, *rse, *g, *pmax, *M1;
  int32_t* pidx;
  uint8_t* live;
  SpaState* state;
  size_t bytes;
};
static SpaScratch spa_carve(void* base, int64_t S, int n, int R) {
  const size_t tiles = (size_t)((S + SPA_TILE - 1) / SPA_TILE);
  ScratchCarver c = {(char*)base, 0};
  SpaScratch b;
  b.D = c.take<double>((size_t)n * (size_t)S);
  b.rse = c.take<double>((size_t)S);
  b.g = c.take<double>(3 * (size_t)S);
  b.pmax = c.take<double>(3 * tiles * (size_t)R);
  b.M1 = c.take<double>((size_t)R);
  b.pidx = c.take<int32_t>(3 * tiles * (size_t)R);
  b.live = c.take<uint8_t>((size_t)S);
  b.state = c.take<SpaState>(1);
  b.bytes = c.at;
  return b;
}

size_t spa_scratch_bytes(int n_strategies, int n, int n_resamples) {
  return spa_carve(nullptr, n_strategies, n, n_resamples).bytes;
}

template <int NJ, int J0>
static void spa_launch_pass(bool pow2, dim3 grid, hipStream_t stream, const SpaScratch& b, const double* weights, int S,
                            int n, int R) {
  constexpr int PLANES = SPA_PLANES == 1 ? 1 : NJ;
  if (pow2)
    hipLaunchKernelGGL((gte_spa_pass_kernel<true, NJ, J0, PLANES>), grid, dim3(SPA_TILE), 0, stream, b.state, b.D,
                       b.live, b.rse, b.g, weights, S, n, R, 1.0 / (double)n, b.pmax, b.pidx);
  else
    hipLaunchKernelGGL((gte_spa_pass_kernel<false, NJ, J0, PLANES>), grid, dim3(SPA_TILE), 0, stream, b.state, b.D,
                       b.live, b.rse, b.g, weights, S, n, R, (double)n, b.pmax, b.pidx);
}

hipError_t launch_spa(const gte_strategy_period_stats* stats, int n_strategies, int n_periods,
                      const uint64_t period_mask[2], int n, const double* benchmark, const double* weights,
                      int n_resamples, double threshold, int crit_rank, int max_rounds,
                      const gte_reality_check_out& rc, const gte_spa_out& out, void* scratch, hipStream_t stream) {
  if (!stats || !period_mask || !weights || !scratch || n_strategies < 1 || n_periods < 1 ||
      n_periods > GTE_MAX_PERIODS || n < 2 || n > n_periods || n_resamples < 1 ||
      n_resamples > GTE_BOOT_MAX_RESAMPLES || !(threshold >= 0.0) || crit_rank < 0 || crit_rank >= n_resamples ||
      max_rounds < 1 || max_rounds > GTE_SPA_MAX_ROUNDS || !rc.mean || !rc.boot_sum || !rc.boot_sq_sum ||
      !out.t_stat || !out.std_error || !out.recentred || !out.count_adj || !out.rejected_round || !out.max_stat ||
      !out.max_index || !out.crit || !out.round_rejected || !out.summary)
    return hipErrorInvalidValue;
  const int S = n_strategies, R = n_resamples;
  const int slabs = (R + GTE_BOOT_SLAB - 1) / GTE_BOOT_SLAB, tiles = (int)(((int64_t)S + SPA_TILE - 1) / SPA_TILE);
  const SpaScratch b = spa_carve(scratch, S, n, R);
  const PeriodMask mask = {{period_mask[0], period_mask[1]}};
  const unsigned per_strategy = (unsigned)(((int64_t)S + 255) / 256), per_resample = (unsigned)((R + 255) / 256);
  hipLaunchKernelGGL(gte_spa_prep_kernel, dim3(per_strategy), dim3(256), 0, stream, stats, S, n_periods, mask,
                     benchmark, rc.mean, rc.boot_sum, rc.boot_sq_sum, R, threshold, b.D, b.rse, b.g, b.live, out.t_stat,
                     out.std_error, out.recentred, out.rejected_round);
  hipLaunchKernelGGL(gte_spa_begin_kernel, dim3(1), dim3(1024), 0, stream, b.live, out.t_stat, S, max_rounds, out.crit,
                     out.round_rejected, out.summary, b.state);
  const bool pow2 = (n & (n - 1)) == 0;
  const dim3 grid((unsigned)tiles, (unsigned)slabs);
  const double* M1 = out.max_stat + R;  // round 0: the consistent row of the three
  spa_launch_pass<3, 0>(pow2, grid, stream, b, weights, S, n, R);
  hipLaunchKernelGGL(gte_spa_max_kernel<true>, dim3(per_resample, 3), dim3(256), 0, stream, b.state, b.pmax, b.pidx,
                     tiles, R, 3, out.max_stat, out.max_index);
  hipLaunchKernelGGL(gte_spa_count_kernel, dim3(per_strategy), dim3(256), 0, stream, out.t_stat, S, R, M1,
                     out.count_adj);
  hipLaunchKernelGGL(gte_spa_close_kernel<true>, dim3(1), dim3(1024), 0, stream, b.state, out.max_stat, M1, R,
                     crit_rank, 0, max_rounds, S, out.t_stat, b.live, out.rejected_round, out.crit, out.round_rejected,
                     out.summary);
  for (int k = 1; k < max_rounds; ++k) {
    spa_launch_pass<1, 1>(pow2, grid, stream, b, weights, S, n, R);
    hipLaunchKernelGGL(gte_spa_max_kernel<false>, dim3(per_resample, 1), dim3(256), 0, stream, b.state, b.pmax,
                       b.pidx, tiles, R, 1, b.M1, (int32_t*)nullptr);
    hipLaunchKernelGGL(gte_spa_close_kernel<false>, dim3(1), dim3(1024), 0, stream, b.state, (const double*)nullptr,
                       b.M1, R, crit_rank, k, max_rounds, S, out.t_stat, b.live, out.rejected_round, out.crit,
                       out.round_rejected, out.summary);
  }
  return hipGetLastError();
}

}  // namespace gte
