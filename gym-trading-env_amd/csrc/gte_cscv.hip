// gte_cscv.hip — the probability of backtest overfitting by combinatorially symmetric cross-validation (gte_cscv,
// include/gte.h): for every split of the period groups into an in-sample and an out-of-sample side, the strategy
// that scores best in sample and where it ranks out of sample among all strategies, from the S * B strategy
// period records.  Own translation unit, beside gte_bootstrap.hip: nothing here can perturb the code of another.
//
//   gte_cscv_fold_kernel     one lane per strategy: the group sums a1, a2, n_g into the dense transposed staging
//             arrays A1[G][S], A2[G][S], N[G][S] (a lane's groups then lie S apart, a wavefront's side by side),
//             and eligibility.
//   gte_cscv_pass1_kernel    HOT.  A lane owns a strategy, a workgroup a tile of CSCV_TILE strategies and a chunk of
//             GTE_CSCV_CHUNK splits.  The lane's group triplets are loaded once and stay in registers (GCAP = 8, 16
//             or 32 of them, the smallest that holds G); the two words of a split are the same for every lane
//             (scalar loads: the address depends on the workgroup and the loop counter alone), so the branch on a
//             group's bit is uniform.  Every chain s1 = s1 + a1_g runs over g ascending in one lane: the bits do not
//             depend on the geometry.  CSCV_RC splits at a time cross the workgroup through LDS for the tile's
//             in-sample maximum, its lowest index and that strategy's out-of-sample score: [tiles][C] partials.
//   gte_cscv_winner_kernel   one thread per split: the tiles' partials in ascending tile order.
//   gte_cscv_pass2_kernel    HOT.  The same tiling; the out-of-sample scores again, counted below / equal / ranked
//             against the winner's (ballot + popcount per wavefront, the four wavefronts added through LDS) into
//             integer partials [tiles][C].
//   gte_cscv_close_kernel    one thread per split: the tiles' counts added, the rule for an invalid split.
//   gte_cscv_summary_kernel  one workgroup: valid / overfit / loss over the splits, the eligible strategies.
// The [C, S] score matrices are never written.  No atomics, no scratch memory.
//
// What may be read: stats[s * B + b] for s < S and b a period of some group (steps, reward_sum, reward_sq_sum);
// the three tables as staged in the scratch; the scratch and the outputs as written by the kernels before.  What
// is written: the outputs gte.h lists, and the library's scratch (CscvScratch).
#include "gte_launch.h"
#include "gte_members.h"

namespace gte {

constexpr int CSCV_TILE = 256;  // strategies of a workgroup, one per lane
constexpr int CSCV_RC = 8;      // splits whose scores cross the workgroup at a time in pass 1
constexpr int CSCV_RC2 = 64;    // splits whose counts cross the workgroup at a time in pass 2
static_assert(GTE_CSCV_CHUNK % CSCV_RC == 0 && GTE_CSCV_CHUNK % CSCV_RC2 == 0 && CSCV_TILE == 32 * CSCV_RC,
              "the chunk's maxima: 32 lanes per split");
static_assert(sizeof(gte_cscv_summary) == 24, "gte_cscv_summary: 24 bytes (include/gte.h)");
static_assert(GTE_CSCV_MAX_GROUPS == 32, "a split side is one 32-bit word");

__global__ __launch_bounds__(256) void gte_cscv_fold_kernel(const gte_strategy_period_stats* __restrict__ stats, int S,
                                                            int B, const PeriodMask* __restrict__ groups, int G,
                                                            double* __restrict__ A1, double* __restrict__ A2,
                                                            long long* __restrict__ NG, uint8_t* __restrict__ elig) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const gte_strategy_period_stats* t = stats + s * B;
  bool ok = true;
  for (int g = 0; g < G; ++g) {
    const PeriodMask mask = groups[g];
    double a1 = 0.0, a2 = 0.0;
    long long n = 0;
    for (int b = 0; b < B; ++b) {
      if (!mask.has(b)) continue;
      a1 = a1 + t[b].reward_sum;
      a2 = a2 + t[b].reward_sq_sum;
      n += t[b].steps;
    }
    ok = ok && n > 0 && __builtin_isfinite(a1) && __builtin_isfinite(a2);
    A1[(long long)g * S + s] = a1;
    A2[(long long)g * S + s] = a2;
    NG[(long long)g * S + s] = n;
  }
  elig[s] = ok ? 1 : 0;
}

// the MEAN_REWARD, SHARPE and REWARD_SUM formulas of gte_rank_period_stats (gte_period_strategy.hip) on (s1, s2, n)
__device__ __forceinline__ double cscv_score(int metric, double s1, double s2, long long n) {
  if (metric == GTE_PERIOD_METRIC_REWARD_SUM) return s1;
  const double count = (double)n;
  const double m = s1 / count;
  if (metric == GTE_PERIOD_METRIC_MEAN_REWARD) return m;
  const double q = s2 / count;
  double v = q - m * m;
  if (!(v > 0.0)) v = 0.0;
  return m / sqrt(v);
}

// a lane's group triplets, in registers: every index below is a constant once the loops are unrolled
template <int GCAP>
struct CscvGroups {
  double a1[GCAP], a2[GCAP];
  long long n[GCAP];
  __device__ __forceinline__ void load(const double* __restrict__ A1, const double* __restrict__ A2,
                                       const long long* __restrict__ NG, long long s, int S, int G) {
#pragma unroll
    for (int g = 0; g < GCAP; ++g) {
      const long long at = (long long)(g < G ? g : G - 1) * S + s;  // (a group past G is in no split word)
      a1[g] = A1[at];
      a2[g] = A2[at];
      n[g] = NG[at];
    }
  }
  // the score over the groups of `word` (the same for every lane), g ascending
  __device__ __forceinline__ double score(uint32_t word, int metric) const {
    double s1 = 0.0, s2 = 0.0;
    long long c = 0;
#pragma unroll
    for (int g = 0; g < GCAP; ++g) {
      if ((word >> g) & 1u) {
        // (an empty statement the compiler may not move: it keeps this a BRANCH on the scalar unit, which skips
        // the groups of the other side, where it would otherwise compute all of them and select: six selects
        // per group and side next to four additions)
        asm volatile("" ::: "memory");
        s1 = s1 + a1[g];
        s2 = s2 + a2[g];
        c += n[g];
      }
    }
    return cscv_score(metric, s1, s2, c);
  }
};

// (m2, i2) takes the place of (m1, i1): a larger value, or the same value at a lower index (an index is -1 exactly
// where the value is -inf: nothing compared greater than the start)
__device__ __forceinline__ bool cscv_better(double m2, int i2, double m1, int i1) {
  return m2 > m1 || (m2 == m1 && i2 < i1);
}

template <int GCAP>
__global__ __launch_bounds__(CSCV_TILE) void gte_cscv_pass1_kernel(
    const double* __restrict__ A1, const double* __restrict__ A2, const long long* __restrict__ NG,
    const uint8_t* __restrict__ elig, const uint32_t* __restrict__ isw, const uint32_t* __restrict__ osw, int S, int G,
    int C, int metric, double* __restrict__ pmax, double* __restrict__ poos, int32_t* __restrict__ pidx) {
  __shared__ double sc_is[CSCV_RC][CSCV_TILE], sc_oos[CSCV_RC][CSCV_TILE];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const long long s = (long long)tile * CSCV_TILE + tid;
  const bool live = s < S;
  const long long sl = live ? s : S - 1;  // a lane past the end reads the last strategy and competes nowhere
  const bool ok = live && elig[sl] != 0;
  CscvGroups<GCAP> grp;
  grp.load(A1, A2, NG, sl, S, G);
  const int c_lo = blockIdx.y * GTE_CSCV_CHUNK;
  const int c_hi = c_lo + GTE_CSCV_CHUNK < C ? c_lo + GTE_CSCV_CHUNK : C;
  for (int c0 = c_lo; c0 < c_hi; c0 += CSCV_RC) {
    for (int k = 0; k < CSCV_RC; ++k) {
      const int c = c0 + k < C ? c0 + k : C - 1;  // a split past the end: the last one again, its values dropped
      const double is = grp.score(isw[c], metric), oos = grp.score(osw[c], metric);
      sc_is[k][tid] = ok ? is : -__builtin_inf();
      sc_oos[k][tid] = oos;
    }
    __syncthreads();
    {  // split k of the sub-chunk: 32 lanes, lane `seg` over strategies seg, seg + 32, ... ascending, then the 32
      const int k = tid >> 5, seg = tid & 31;
      double bm = -__builtin_inf();
      int bi = -1;
#pragma unroll
      for (int j = 0; j < CSCV_TILE / 32; ++j) {
        const double v = sc_is[k][j * 32 + seg];
        if (v > bm) {
          bm = v;
          bi = j * 32 + seg;
        }
      }
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) {
        const double om = __shfl_xor(bm, off);
        const int oi = __shfl_xor(bi, off);
        if (cscv_better(om, oi, bm, bi)) {
          bm = om;
          bi = oi;
        }
      }
      if (seg == 0 && c0 + k < c_hi) {
        const long long at = (long long)tile * C + c0 + k;
        pmax[at] = bm;
        poos[at] = bi >= 0 ? sc_oos[k][bi] : __builtin_nan("");
        pidx[at] = bi >= 0 ? tile * CSCV_TILE + bi : -1;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void gte_cscv_winner_kernel(const double* __restrict__ pmax,
                                                              const double* __restrict__ poos,
                                                              const int32_t* __restrict__ pidx, int tiles, int C,
                                                              int32_t* __restrict__ best, double* __restrict__ is_score,
                                                              double* __restrict__ oos_score) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double bm = -__builtin_inf(), bo = __builtin_nan("");
  int bi = -1;
  for (int t = 0; t < tiles; ++t) {  // ascending tiles are ascending strategies: a plain > keeps the lowest index
    const double v = pmax[(long long)t * C + c];
    if (v > bm) {
      bm = v;
      bi = pidx[(long long)t * C + c];
      bo = poos[(long long)t * C + c];
    }
  }
  best[c] = bi;
  is_score[c] = bi >= 0 ? bm : __builtin_nan("");
  oos_score[c] = bo;
}

template <int GCAP>
__global__ __launch_bounds__(CSCV_TILE) void gte_cscv_pass2_kernel(
    const double* __restrict__ A1, const double* __restrict__ A2, const long long* __restrict__ NG,
    const uint8_t* __restrict__ elig, const uint32_t* __restrict__ osw, const double* __restrict__ oos_score, int S,
    int G, int C, int metric, int32_t* __restrict__ pbelow, int32_t* __restrict__ pequal,
    int32_t* __restrict__ pranked) {
  __shared__ int32_t wc[3][CSCV_RC2][CSCV_TILE / 64];
  const int tid = threadIdx.x, tile = blockIdx.x, wave = tid >> 6;
  const long long s = (long long)tile * CSCV_TILE + tid;
  const bool live = s < S;
  const long long sl = live ? s : S - 1;  // a lane past the end reads the last strategy and counts nowhere
  const bool ok = live && elig[sl] != 0;
  CscvGroups<GCAP> grp;
  grp.load(A1, A2, NG, sl, S, G);
  const int c_lo = blockIdx.y * GTE_CSCV_CHUNK;
  const int c_hi = c_lo + GTE_CSCV_CHUNK < C ? c_lo + GTE_CSCV_CHUNK : C;
  for (int c0 = c_lo; c0 < c_hi; c0 += CSCV_RC2) {
    for (int k = 0; k < CSCV_RC2; ++k) {
      const int c = c0 + k < C ? c0 + k : C - 1;  // a split past the end: the last one again, its counts dropped
      const double oos = grp.score(osw[c], metric);
      const double w = oos_score[c];  // NaN for an invalid split: nothing is below it or equal to it
      const int below = __popcll(__ballot(ok && oos < w));
      const int equal = __popcll(__ballot(ok && oos == w));
      const int ranked = __popcll(__ballot(ok && oos == oos));
      if ((tid & 63) == 0) {
        wc[0][k][wave] = below;
        wc[1][k][wave] = equal;
        wc[2][k][wave] = ranked;
      }
    }
    __syncthreads();
    if (tid < CSCV_RC2 && c0 + tid < c_hi) {
      const long long at = (long long)tile * C + c0 + tid;
      int t0 = 0, t1 = 0, t2 = 0;
#pragma unroll
      for (int w = 0; w < CSCV_TILE / 64; ++w) {
        t0 += wc[0][tid][w];
        t1 += wc[1][tid][w];
        t2 += wc[2][tid][w];
      }
      pbelow[at] = t0;
      pequal[at] = t1;
      pranked[at] = t2;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void gte_cscv_close_kernel(const int32_t* __restrict__ pbelow,
                                                             const int32_t* __restrict__ pequal,
                                                             const int32_t* __restrict__ pranked, int tiles, int C,
                                                             const int32_t* __restrict__ best,
                                                             const double* __restrict__ oos_score,
                                                             int32_t* __restrict__ below, int32_t* __restrict__ equal,
                                                             int32_t* __restrict__ ranked) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  int t0 = 0, t1 = 0, t2 = 0;
  for (int t = 0; t < tiles; ++t) {
    t0 += pbelow[(long long)t * C + c];
    t1 += pequal[(long long)t * C + c];
    t2 += pranked[(long long)t * C + c];
  }
  const double w = oos_score[c];
  const bool valid = best[c] >= 0 && w == w;
  below[c] = valid ? t0 : 0;
  equal[c] = valid ? t1 : 0;
  ranked[c] = t2;
}

__global__ __launch_bounds__(1024) void gte_cscv_summary_kernel(const uint8_t* __restrict__ elig, int S,
                                                                const int32_t* __restrict__ best,
                                                                const double* __restrict__ oos_score,
                                                                const int32_t* __restrict__ below,
                                                                const int32_t* __restrict__ equal,
                                                                const int32_t* __restrict__ ranked, int C,
                                                                gte_cscv_summary* __restrict__ out) {
  __shared__ int sv[1024], so[1024], sl[1024], se[1024];
  const int tid = threadIdx.x;
  int valid = 0, overfit = 0, loss = 0, eligible = 0;
  for (int c = tid; c < C; c += 1024) {
    const double w = oos_score[c];
    if (!(best[c] >= 0 && w == w)) continue;
    valid += 1;
    overfit += 2 * (long long)below[c] + equal[c] <= ranked[c] ? 1 : 0;
    loss += w < 0.0 ? 1 : 0;
  }
  for (long long s = tid; s < S; s += 1024) eligible += elig[s] ? 1 : 0;
  sv[tid] = valid;
  so[tid] = overfit;
  sl[tid] = loss;
  se[tid] = eligible;
  __syncthreads();
  for (int half = 512; half > 0; half >>= 1) {
    if (tid < half) {
      sv[tid] += sv[tid + half];
      so[tid] += so[tid + half];
      sl[tid] += sl[tid + half];
      se[tid] += se[tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out->splits = C;
    out->valid = sv[0];
    out->overfit = so[0];
    out->loss = sl[0];
    out->eligible = se[0];
    out->reserved = 0;
  }
}

// the library's scratch of one gte_cscv, carved out of one allocation (ScratchCarver, gte_launch.h).  The three
// host tables come first, packed as the host side packs them (CscvTables): one copy stages them.  The integer
// partials of pass 2 take the bytes of pass 1's: the winner kernel has read those before pass 2 runs.
struct CscvScratch {
  PeriodMask* groups;
  uint32_t *isw, *osw;
  double *A1, *A2, *pmax, *poos;
  long long* NG;
  int32_t *pidx, *pbelow, *pequal, *pranked;
  uint8_t* elig;
  size_t table_bytes, bytes;
};
static CscvScratch cscv_carve(void* base, int64_t S, int G, int C) {
  const size_t tiles = (size_t)((S + CSCV_TILE - 1) / CSCV_TILE), tc = tiles * (size_t)C;
  ScratchCarver c = {(char*)base, 0};
  CscvScratch b;
  b.table_bytes = sizeof(PeriodMask) * (size_t)G + 8 * (size_t)C;
  char* tables = c.take<char>(b.table_bytes);  // groups, then the two split tables, back to back
  b.groups = (PeriodMask*)tables;
  b.isw = (uint32_t*)(tables + sizeof(PeriodMask) * (size_t)G);
  b.osw = b.isw + C;
  b.A1 = c.take<double>((size_t)G * (size_t)S);
  b.A2 = c.take<double>((size_t)G * (size_t)S);
  b.NG = c.take<long long>((size_t)G * (size_t)S);
  b.pmax = c.take<double>(tc);
  b.poos = c.take<double>(tc);
  b.pidx = c.take<int32_t>(tc);
  b.elig = c.take<uint8_t>((size_t)S);
  b.pbelow = (int32_t*)b.pmax;
  b.pequal = b.pbelow + tc;
  b.pranked = (int32_t*)b.poos;
  b.bytes = c.at;
  return b;
}

size_t cscv_scratch_bytes(int n_strategies, int n_groups, int n_splits) {
  return cscv_carve(nullptr, n_strategies, n_groups, n_splits).bytes;
}

size_t cscv_table_bytes(int n_groups, int n_splits) { return cscv_carve(nullptr, 1, n_groups, n_splits).table_bytes; }

template <int GCAP>
static void cscv_passes(const CscvScratch& b, int S, int G, int C, int metric, int tiles, const gte_cscv_out& out,
                        hipStream_t stream) {
  const dim3 grid((unsigned)tiles, (unsigned)((C + GTE_CSCV_CHUNK - 1) / GTE_CSCV_CHUNK));
  hipLaunchKernelGGL(gte_cscv_pass1_kernel<GCAP>, grid, dim3(CSCV_TILE), 0, stream, b.A1, b.A2, b.NG, b.elig, b.isw,
                     b.osw, S, G, C, metric, b.pmax, b.poos, b.pidx);
  hipLaunchKernelGGL(gte_cscv_winner_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, b.pmax, b.poos,
                     b.pidx, tiles, C, out.best, out.is_score, out.oos_score);
  hipLaunchKernelGGL(gte_cscv_pass2_kernel<GCAP>, grid, dim3(CSCV_TILE), 0, stream, b.A1, b.A2, b.NG, b.elig, b.osw,
                     out.oos_score, S, G, C, metric, b.pbelow, b.pequal, b.pranked);
}

hipError_t launch_cscv(const gte_strategy_period_stats* stats, int n_strategies, int n_periods, const void* tables,
                       int n_groups, int n_splits, int metric, const gte_cscv_out& out, void* scratch,
                       hipStream_t stream) {
  if (!stats || !tables || !scratch || n_strategies < 1 || n_periods < 1 || n_periods > GTE_MAX_PERIODS ||
      n_groups < 2 || n_groups > GTE_CSCV_MAX_GROUPS || n_splits < 1 || n_splits > GTE_CSCV_MAX_SPLITS ||
      (metric != GTE_PERIOD_METRIC_MEAN_REWARD && metric != GTE_PERIOD_METRIC_SHARPE &&
       metric != GTE_PERIOD_METRIC_REWARD_SUM) ||
      !out.best || !out.is_score || !out.oos_score || !out.below || !out.equal || !out.ranked || !out.summary)
    return hipErrorInvalidValue;
  const int S = n_strategies, G = n_groups, C = n_splits;
  const int tiles = (int)(((int64_t)S + CSCV_TILE - 1) / CSCV_TILE);
  const CscvScratch b = cscv_carve(scratch, S, G, C);
  // (pageable host memory: the copy has taken the bytes out of `tables` when this returns)
  const hipError_t e = hipMemcpyAsync(b.groups, tables, b.table_bytes, hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gte_cscv_fold_kernel, dim3((unsigned)(((int64_t)S + 255) / 256)), dim3(256), 0, stream, stats, S,
                     n_periods, b.groups, G, b.A1, b.A2, b.NG, b.elig);
  if (G <= 8)
    cscv_passes<8>(b, S, G, C, metric, tiles, out, stream);
  else if (G <= 16)
    cscv_passes<16>(b, S, G, C, metric, tiles, out, stream);
  else
    cscv_passes<32>(b, S, G, C, metric, tiles, out, stream);
  hipLaunchKernelGGL(gte_cscv_close_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, b.pbelow, b.pequal,
                     b.pranked, tiles, C, out.best, out.oos_score, out.below, out.equal, out.ranked);
  hipLaunchKernelGGL(gte_cscv_summary_kernel, dim3(1), dim3(1024), 0, stream, b.elig, S, out.best, out.oos_score,
                     out.below, out.equal, out.ranked, C, out.summary);
  return hipGetLastError();
}

}  // namespace gte
