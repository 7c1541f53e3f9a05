// gte_bootstrap.hip — the bootstrap reality check of a strategy leaderboard (gte_bootstrap_weights,
// gte_reality_check, include/gte.h): resampling weights over the selected periods, and the maximum over all
// strategies of their centred resampled means, resample by resample, from the S * B strategy period records.
// Own translation unit, beside gte_period_strategy.hip: nothing here can perturb the code of another.
//
//   gte_boot_weights_kernel   one thread per resample: its row of w[R][n], n draws of the stationary bootstrap.
//   gte_boot_gather_kernel    one lane per strategy: eligibility, d_i = reward_sum[s][p_i] - benchmark[p_i] into the
//             dense transposed staging array D[n][S] (a lane's d_i then lie S apart, a wavefront's side by side),
//             and mean_s.
//   gte_boot_resample_kernel  THE HOT PATH, 2 * R * S * n f64 operations.  A lane owns a strategy, a workgroup a
//             tile of BOOT_TILE strategies and a slab of GTE_BOOT_SLAB resamples, taken BOOT_RC at a time: BOOT_RC
//             accumulators per lane, d_i loaded once per chunk, w[r][i] the same for every lane (scalar loads,
//             the address depends on the workgroup and the loop counters alone).  Every chain a = a + w * d runs
//             over i ascending in one lane: the bits do not depend on the geometry.  The moments of a lane's
//             c_rs over the slab, r ascending, go to the slab partials; the chunk's c_rs cross the workgroup through
//             LDS once, for the tile's maximum and its lowest index per resample.  The [R, S] matrix is never
//             written.  No atomics, no scratch.
//   gte_boot_max_kernel       one thread per resample: the tiles' maxima in ascending tile order.
//   gte_boot_close_kernel     one lane per strategy: the slab partials in ascending slab order, and the count of
//             resample maxima at or above mean_s.
//   gte_boot_summary_kernel   one workgroup: the best mean, its lowest index, its count, the eligible strategies.
//
// What may be read: stats[s * B + b] for s < S and b a selected period < B (steps and reward_sum alone);
// benchmark[b] for the same b; w[r * n + i] for r < R, i < n; the scratch and the outputs as written by the
// kernels before.  What is written: the outputs gte.h lists, and the library's scratch (BootScratch).
#include "gte_launch.h"
#include "gte_members.h"

namespace gte {

constexpr int BOOT_TILE = 256;  // strategies of a workgroup, one per lane
constexpr int BOOT_RC = 16;     // resamples a lane accumulates at a time
static_assert(GTE_BOOT_SLAB % BOOT_RC == 0 && BOOT_TILE == 16 * BOOT_RC, "the chunk's maxima: 16 lanes per resample");
static_assert(sizeof(gte_reality_check_summary) == 24, "gte_reality_check_summary: 24 bytes (include/gte.h)");

__global__ __launch_bounds__(64) void gte_boot_weights_kernel(int n, int R, uint32_t thr, int always, uint32_t k0,
                                                              uint32_t k1, double* __restrict__ w) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  double* row = w + (long long)r * n;
  for (int i = 0; i < n; ++i) row[i] = 0.0;
  int pos = 0;
  for (int j = 0; j < n; ++j) {
    uint32_t o[4];
    philox4x32_10((uint32_t)r, (uint32_t)j, 0u, 0x424F4F54u, k0, k1, o);
    if (j == 0 || always || o[0] < thr)
      pos = bounded(o[1], n);
    else
      pos = pos + 1 == n ? 0 : pos + 1;
    row[pos] = row[pos] + 1.0;  // (this thread's own stores: program order)
  }
}

hipError_t launch_bootstrap_weights(int n, int n_resamples, uint32_t thr, int always, uint64_t seed, double* weights,
                                    hipStream_t stream) {
  if (!weights || n < 2 || n > GTE_MAX_PERIODS || n_resamples < 1 || n_resamples > GTE_BOOT_MAX_RESAMPLES)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_boot_weights_kernel, dim3((unsigned)((n_resamples + 63) / 64)), dim3(64), 0, stream, n,
                     n_resamples, thr, always, (uint32_t)seed, (uint32_t)(seed >> 32), weights);
  return hipGetLastError();
}

// ---- the reality check

// PeriodMask (gte_members.h) under the name the gather kernel's symbol carries: a kernel's name spells out its
// parameter types, and this kernel's code is to stay what it was byte for byte
struct BootMask : PeriodMask {};

__global__ __launch_bounds__(256) void gte_boot_gather_kernel(const gte_strategy_period_stats* __restrict__ stats, int S,
                                                              int B, const BootMask mask, int n,
                                                              const double* __restrict__ benchmark,
                                                              double* __restrict__ D, uint8_t* __restrict__ elig,
                                                              double* __restrict__ mean) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const gte_strategy_period_stats* t = stats + s * B;
  bool ok = true;
  double sum = 0.0;
  int i = 0;
  for (int b = 0; b < B; ++b) {
    if (!mask.has(b)) continue;
    const double x = t[b].reward_sum;
    ok = ok && t[b].steps > 0 && __builtin_isfinite(x);
    const double d = benchmark ? x - benchmark[b] : x;
    D[(long long)i * S + s] = d;
    sum = sum + d;
    ++i;
  }
  const double m = sum / (double)n;
  elig[s] = ok ? 1 : 0;
  mean[s] = ok ? m : __builtin_nan("");
}

// (m2, i2) takes the place of (m1, i1): a larger value, or the same value at a lower index (an index is -1 exactly
// where the value is -inf: nothing compared greater than the start)
__device__ __forceinline__ bool boot_better(double m2, int i2, double m1, int i1) {
  return m2 > m1 || (m2 == m1 && i2 < i1);
}

// POW2: n is a power of two and `scale` its reciprocal, a * scale IS a / n (both the correctly rounded quotient);
// otherwise `scale` is n and the division is made
template <bool POW2>
__global__ __launch_bounds__(BOOT_TILE) void gte_boot_resample_kernel(
    const double* __restrict__ D, const uint8_t* __restrict__ elig, const double* __restrict__ mean,
    const double* __restrict__ w, int S, int n, int R, double scale, double* __restrict__ pq1, double* __restrict__ pq2,
    int32_t* __restrict__ pge, double* __restrict__ pmax, int32_t* __restrict__ pidx) {
  __shared__ double sc[BOOT_RC][BOOT_TILE];
  const int tid = threadIdx.x, tile = blockIdx.x, slab = blockIdx.y;
  const long long s = (long long)tile * BOOT_TILE + tid;
  const bool live = s < S;
  const long long sl = live ? s : S - 1;  // a lane past the end reads the last strategy and counts nowhere
  const bool ok = live && elig[sl] != 0;
  const double m = mean[sl];
  const int r_lo = slab * GTE_BOOT_SLAB;
  const int r_hi = r_lo + GTE_BOOT_SLAB < R ? r_lo + GTE_BOOT_SLAB : R;
  const double* dcol = D + sl;
  double q1 = 0.0, q2 = 0.0;
  int ge = 0;
  for (int r0 = r_lo; r0 < r_hi; r0 += BOOT_RC) {
    double acc[BOOT_RC];
    long long row[BOOT_RC];  // a chunk past the end reads the last resample's row again; its values are dropped
#pragma unroll
    for (int k = 0; k < BOOT_RC; ++k) {
      acc[k] = 0.0;
      row[k] = (long long)(r0 + k < R ? r0 + k : R - 1) * n;
    }
#pragma unroll 2
    for (int i = 0; i < n; ++i) {
      const double d = dcol[(long long)i * S];
#pragma unroll
      for (int k = 0; k < BOOT_RC; ++k) acc[k] = acc[k] + w[row[k] + i] * d;
    }
#pragma unroll
    for (int k = 0; k < BOOT_RC; ++k) {
      const double q = POW2 ? acc[k] * scale : acc[k] / scale;
      const double c = q - m;
      if (ok && r0 + k < r_hi) {
        q1 = q1 + c;
        q2 = q2 + c * c;
        ge += c >= m ? 1 : 0;
      }
      sc[k][tid] = ok ? c : -__builtin_inf();
    }
    __syncthreads();
    {  // resample k of the chunk: 16 lanes, lane `seg` over strategies seg, seg + 16, ... ascending, then the 16
      const int k = tid >> 4, seg = tid & 15;
      double bm = -__builtin_inf();
      int bi = -1;
#pragma unroll
      for (int j = 0; j < BOOT_TILE / 16; ++j) {
        const double v = sc[k][j * 16 + seg];
        if (v > bm) {
          bm = v;
          bi = j * 16 + seg;
        }
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const double om = __shfl_xor(bm, off);
        const int oi = __shfl_xor(bi, off);
        if (boot_better(om, oi, bm, bi)) {
          bm = om;
          bi = oi;
        }
      }
      if (seg == 0 && r0 + k < r_hi) {
        pmax[(long long)tile * R + r0 + k] = bm;
        pidx[(long long)tile * R + r0 + k] = bi >= 0 ? tile * BOOT_TILE + bi : -1;
      }
    }
    __syncthreads();
  }
  if (live) {
    pq1[(long long)slab * S + s] = q1;
    pq2[(long long)slab * S + s] = q2;
    pge[(long long)slab * S + s] = ge;
  }
}

__global__ __launch_bounds__(256) void gte_boot_max_kernel(const double* __restrict__ pmax,
                                                           const int32_t* __restrict__ pidx, int tiles, int R,
                                                           double* __restrict__ max_stat,
                                                           int32_t* __restrict__ max_index) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  double bm = -__builtin_inf();
  int bi = -1;
  for (int t = 0; t < tiles; ++t) {  // ascending tiles are ascending strategies: a plain > keeps the lowest index
    const double v = pmax[(long long)t * R + r];
    if (v > bm) {
      bm = v;
      bi = pidx[(long long)t * R + r];
    }
  }
  max_stat[r] = bm;
  max_index[r] = bi;
}

__global__ __launch_bounds__(256) void gte_boot_close_kernel(const uint8_t* __restrict__ elig,
                                                             const double* __restrict__ mean,
                                                             const double* __restrict__ pq1,
                                                             const double* __restrict__ pq2,
                                                             const int32_t* __restrict__ pge, int S, int slabs, int R,
                                                             const double* __restrict__ max_stat,
                                                             double* __restrict__ boot_sum,
                                                             double* __restrict__ boot_sq_sum,
                                                             int32_t* __restrict__ count_ge,
                                                             int32_t* __restrict__ count_adj) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  if (!elig[s]) {
    boot_sum[s] = __builtin_nan("");
    boot_sq_sum[s] = __builtin_nan("");
    count_ge[s] = 0;
    count_adj[s] = 0;
    return;
  }
  double q1 = 0.0, q2 = 0.0;
  int ge = 0;
  for (int j = 0; j < slabs; ++j) {
    q1 = q1 + pq1[(long long)j * S + s];
    q2 = q2 + pq2[(long long)j * S + s];
    ge += pge[(long long)j * S + s];
  }
  const double m = mean[s];
  int adj = 0;
  for (int r = 0; r < R; ++r) adj += max_stat[r] >= m ? 1 : 0;
  boot_sum[s] = q1;
  boot_sq_sum[s] = q2;
  count_ge[s] = ge;
  count_adj[s] = adj;
}

__global__ __launch_bounds__(1024) void gte_boot_summary_kernel(const uint8_t* __restrict__ elig,
                                                                const double* __restrict__ mean,
                                                                const int32_t* __restrict__ count_adj, int S,
                                                                gte_reality_check_summary* __restrict__ out) {
  __shared__ double sm[1024];
  __shared__ int si[1024], sn[1024];
  const int tid = threadIdx.x;
  double bm = -__builtin_inf();
  int bi = -1, cnt = 0;
  for (long long s = tid; s < S; s += 1024) {  // ascending within the thread: a plain > keeps its lowest index
    if (!elig[s]) continue;
    cnt += 1;
    const double v = mean[s];
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
      if (boot_better(sm[tid + half], si[tid + half], sm[tid], si[tid])) {
        sm[tid] = sm[tid + half];
        si[tid] = si[tid + half];
      }
      sn[tid] += sn[tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int best = si[0];
    out->best_mean = best >= 0 ? sm[0] : __builtin_nan("");
    out->best = best;
    out->count_rc = best >= 0 ? count_adj[best] : 0;
    out->eligible = sn[0];
    out->reserved = 0;
  }
}

// the library's scratch of one gte_reality_check, carved out of one allocation (ScratchCarver, gte_launch.h)
struct BootScratch {
  double *D, *pq1, *pq2, *pmax;
  int32_t *pge, *pidx;
  uint8_t* elig;
  size_t bytes;
};
static BootScratch boot_carve(void* base, int64_t S, int n, int R) {
  const size_t slabs = (size_t)((R + GTE_BOOT_SLAB - 1) / GTE_BOOT_SLAB), tiles = (size_t)((S + BOOT_TILE - 1) / BOOT_TILE);
  ScratchCarver c = {(char*)base, 0};
  BootScratch b;
  b.D = c.take<double>((size_t)n * (size_t)S);
  b.pq1 = c.take<double>(slabs * (size_t)S);
  b.pq2 = c.take<double>(slabs * (size_t)S);
  b.pmax = c.take<double>(tiles * (size_t)R);
  b.pge = c.take<int32_t>(slabs * (size_t)S);
  b.pidx = c.take<int32_t>(tiles * (size_t)R);
  b.elig = c.take<uint8_t>((size_t)S);
  b.bytes = c.at;
  return b;
}

size_t reality_check_scratch_bytes(int n_strategies, int n, int n_resamples) {
  return boot_carve(nullptr, n_strategies, n, n_resamples).bytes;
}

hipError_t launch_reality_check(const gte_strategy_period_stats* stats, int n_strategies, int n_periods,
                                const uint64_t period_mask[2], int n, const double* benchmark, const double* weights,
                                int n_resamples, const gte_reality_check_out& out, void* scratch,
                                hipStream_t stream) {
  if (!stats || !period_mask || !weights || !scratch || n_strategies < 1 || n_periods < 1 ||
      n_periods > GTE_MAX_PERIODS || n < 2 || n > n_periods || n_resamples < 1 ||
      n_resamples > GTE_BOOT_MAX_RESAMPLES || !out.mean || !out.boot_sum || !out.boot_sq_sum || !out.count_ge ||
      !out.count_adj || !out.max_stat || !out.max_index || !out.summary)
    return hipErrorInvalidValue;
  const int S = n_strategies, R = n_resamples;
  const int slabs = (R + GTE_BOOT_SLAB - 1) / GTE_BOOT_SLAB, tiles = (int)(((int64_t)S + BOOT_TILE - 1) / BOOT_TILE);
  const BootScratch b = boot_carve(scratch, S, n, R);
  const BootMask mask = {{{period_mask[0], period_mask[1]}}};
  const unsigned per_strategy = (unsigned)(((int64_t)S + 255) / 256);
  hipLaunchKernelGGL(gte_boot_gather_kernel, dim3(per_strategy), dim3(256), 0, stream, stats, S, n_periods, mask, n,
                     benchmark, b.D, b.elig, out.mean);
  const bool pow2 = (n & (n - 1)) == 0;
  const dim3 grid((unsigned)tiles, (unsigned)slabs);
  if (pow2)
    hipLaunchKernelGGL(gte_boot_resample_kernel<true>, grid, dim3(BOOT_TILE), 0, stream, b.D, b.elig, out.mean, weights,
                       S, n, R, 1.0 / (double)n, b.pq1, b.pq2, b.pge, b.pmax, b.pidx);
  else
    hipLaunchKernelGGL(gte_boot_resample_kernel<false>, grid, dim3(BOOT_TILE), 0, stream, b.D, b.elig, out.mean,
                       weights, S, n, R, (double)n, b.pq1, b.pq2, b.pge, b.pmax, b.pidx);
  hipLaunchKernelGGL(gte_boot_max_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, stream, b.pmax, b.pidx, tiles,
                     R, out.max_stat, out.max_index);
  hipLaunchKernelGGL(gte_boot_close_kernel, dim3(per_strategy), dim3(256), 0, stream, b.elig, out.mean, b.pq1, b.pq2,
                     b.pge, S, slabs, R, out.max_stat, out.boot_sum, out.boot_sq_sum, out.count_ge, out.count_adj);
  hipLaunchKernelGGL(gte_boot_summary_kernel, dim3(1), dim3(1024), 0, stream, b.elig, out.mean, out.count_adj, S,
                     out.summary);
  return hipGetLastError();
}

}  // namespace gte
