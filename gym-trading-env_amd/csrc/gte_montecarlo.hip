// gte_montecarlo.hip — the trade Monte Carlo (gte_pool_trades, gte_trade_monte_carlo, include/gte.h): the pools of
// trade factors of the requested strategies out of the env's trade list, and the resampling of pools — trades drawn
// with replacement and compounded, resample by resample.  Own translation unit, beside gte_bootstrap.hip: nothing
// here can perturb the code of another.  The walk step, the index mapping, the pool and path sizes and the slab
// tree's level are those of include/gte_mc.h, which a host program replays (tests/mc_check.cpp).
//
//   gte_mc_count_kernel  ONE workgroup: `lpp` lanes per request walk the members of its strategy (gte_members.h) and
//             add min(closed, capacity) and closed > capacity — integers, any order is exact —, then an inclusive
//             scan of the requests' sizes through LDS, the passes chained by a carry: first[] and truncated[].
//   gte_mc_pack_kernel   one workgroup per request, 256 members at a time: their sizes scanned through LDS in member
//             order, then one wavefront per member: a lane loads the first 16 bytes of a list record (open_value,
//             close_value), divides once and stores the factor; consecutive lanes consecutive places of the pool.
//   gte_mc_walk_kernel   THE HOT PATH, R * L walk steps per pool (a multiply, a divide, four compares; a Philox
//             block per four).  One workgroup of 256 lanes is one slab of one pool, a lane a resample.  A pool of
//             at most GTE_MC_LDS_POOL factors (64 KiB of the CU's 160 KiB LDS: two workgroups per CU) is staged
//             into LDS once, 16 bytes per lane and load, and the walk reads LDS; a larger pool is read in place,
//             through L2 — ONE kernel for both: a second instantiation without the 64 KiB, launched beside this
//             one for the larger pools at four times the wavefronts per CU, was measured and is SLOWER (66.7 against
//             50.7 ms at 4 096 pools of 32 768: profiles/trade_mc_bench.log); a random 8-byte load moves a whole
//             cache line out of L2, and more wavefronts leave fewer hits in L1.  The per-path columns are stored a
//             lane a resample (coalesced); the slab's four tree sums (in the LDS of the pool, taken again for the
//             4 * 256 places) and its counts go to the library's scratch.
//   gte_mc_close_kernel  one lane per pool: the slabs' partial results in ascending slab order -> pool[], dd_count[].
//
// What may be read: first[0 .. n_pools]; stream[q]; factors[first[q] + j] for j < P where P is mc_pool_size's, 0 for
// every pool not inside [first[0], first[n_pools]); a trade record only at an env checked against [0, N) and a list
// record only below min(closed, capacity); group lists as gte_trade_strategy.hip reads them.  What is written: the
// outputs gte.h lists, each at q < n_pools and r < R, factors below min(first[q + 1], max_factors) only, and the
// library's scratch (McScratch).  No atomics, no inline assembly.
#include "gte_launch.h"
#include "gte_members.h"
#include "../../include/gte_mc.h"

namespace gte {

static_assert(sizeof(gte_mc_pool) == 48 && offsetof(gte_mc_pool, mdd_sum) == 16 && offsetof(gte_mc_pool, count_loss) == 32,
              "gte_mc_pool: four doubles, four 32-bit words, three 16-byte pieces");
static_assert(MC_SLAB == GTE_MC_SLAB && MC_MAX_PATH == GTE_MC_MAX_PATH, "include/gte_mc.h states include/gte.h's limits");
static_assert(GTE_MC_LDS_POOL >= 4 * GTE_MC_SLAB, "the four trees of a slab take the pool's LDS");

constexpr int MC_COUNTS = 2 + GTE_MC_MAX_LEVELS;  // count_loss, count_ruin, dd_count[k]

// ---- the pools

constexpr int MCP_THREADS = 1024;

__global__ __launch_bounds__(MCP_THREADS) void gte_mc_count_kernel(const gte_trade_stats* __restrict__ trades,
                                                                   int capacity, int N, int S, unsigned first_shift,
                                                                   const int32_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ envs,
                                                                   const int32_t* __restrict__ strategies, int n_pools,
                                                                   int lpp, int64_t* __restrict__ first,
                                                                   int32_t* __restrict__ truncated) {
  __shared__ int64_t part[MCP_THREADS];
  __shared__ int64_t carry;
  const int tid = threadIdx.x, sub = tid % lpp, per_pass = MCP_THREADS / lpp;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n_pools; base += per_pass) {
    const int q = base + tid / lpp;
    long long n = 0;
    int tr = 0;
    if (q < n_pools) {
      const int32_t s = strategies[q];
      if ((uint32_t)s < (uint32_t)S) {
        const Members g = members_of(s, N, S, first_shift, offsets);
        for (int m = sub; m < g.n; m += lpp) {
          const long long e = member_env(g, envs, N, S, m);
          if (e < 0) continue;
          const int32_t c = trades[e].closed;
          n += c < 0 ? 0 : c < capacity ? c : capacity;
          tr += c > capacity ? 1 : 0;
        }
      }
    }
    for (int off = 1; off < lpp; off <<= 1) {  // (lpp is a power of two <= 64: a request's lanes share a wavefront)
      n += __shfl_xor(n, off, 64);
      tr += __shfl_xor(tr, off, 64);
    }
    const int64_t mine = sub == 0 && q < n_pools ? (int64_t)n : 0;
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < MCP_THREADS; d <<= 1) {  // inclusive scan of part[]
      const int64_t add = tid >= d ? part[tid - d] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    if (sub == 0 && q < n_pools) {
      first[q] = carry + part[tid] - mine;
      truncated[q] = tr;
    }
    __syncthreads();
    if (tid == MCP_THREADS - 1) carry += part[tid];
    __syncthreads();
  }
  if (tid == 0) first[n_pools] = carry;
}

__global__ __launch_bounds__(256) void gte_mc_pack_kernel(const gte_trade_stats* __restrict__ trades,
                                                          const gte_trade* __restrict__ list, int capacity, int N,
                                                          int S, unsigned first_shift,
                                                          const int32_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ envs,
                                                          const int32_t* __restrict__ strategies,
                                                          const int64_t* __restrict__ first,
                                                          double* __restrict__ factors, int64_t max_factors) {
  __shared__ int64_t at[256];
  __shared__ int32_t cnt[256], env[256];
  __shared__ int64_t carry;
  const int q = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int32_t s = strategies[q];
  if ((uint32_t)s >= (uint32_t)S) return;  // (the whole workgroup)
  const Members g = members_of(s, N, S, first_shift, offsets);
  const int64_t lo = first[q], hi = first[q + 1] < max_factors ? first[q + 1] : max_factors;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < g.n; base += 256) {
    const int m = base + tid;
    int32_t n = 0, e32 = -1;
    if (m < g.n) {
      const long long e = member_env(g, envs, N, S, m);
      if (e >= 0) {
        const int32_t c = trades[e].closed;
        n = c < 0 ? 0 : c < capacity ? c : capacity;
        e32 = (int32_t)e;
      }
    }
    cnt[tid] = n;
    env[tid] = e32;
    at[tid] = n;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan of the members' sizes
      const int64_t add = tid >= d ? at[tid - d] : 0;
      __syncthreads();
      at[tid] += add;
      __syncthreads();
    }
    const int64_t before = carry + at[tid] - n;
    __syncthreads();
    at[tid] = before;
    if (tid == 255) carry = before + n;
    __syncthreads();
    for (int k = wave; k < 256; k += 4) {  // one wavefront per member
      const int32_t nk = cnt[k];
      if (nk == 0) continue;
      const gte_trade* src = list + (int64_t)env[k] * capacity;
      const int64_t dst = lo + at[k];
      for (int i = lane; i < nk; i += 64) {
        if (dst + i >= hi) break;
        const double2 v = *reinterpret_cast<const double2*>(src + i);  // open_value, close_value
        factors[dst + i] = v.y / v.x;
      }
    }
    __syncthreads();
  }
}

static int lanes_per_pool(int n_envs, int n_strategies, int n_pools) {
  const int64_t members = ((int64_t)n_envs + n_strategies - 1) / n_strategies;  // (of the default map; else the mean)
  int lpp = 1;
  while (lpp < 64 && lpp < members && (int64_t)n_pools * lpp * 2 <= MCP_THREADS) lpp <<= 1;
  return lpp;
}

hipError_t launch_pool_count(const gte_trade_stats* trades, const TradeList& tl, int n_envs, int n_strategies,
                             int64_t env_id_base, const int32_t* group_offsets, const int32_t* group_envs,
                             const int32_t* strategies, int n_pools, int64_t* first, int32_t* truncated,
                             hipStream_t stream) {
  if (!trades || tl.capacity < 1 || n_envs < 1 || n_strategies < 1 || !strategies || n_pools < 1 ||
      n_pools > GTE_MC_MAX_POOLS || !first || !truncated || (group_offsets == nullptr) != (group_envs == nullptr))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_mc_count_kernel, dim3(1), dim3(MCP_THREADS), 0, stream, trades, tl.capacity, n_envs,
                     n_strategies, members_first_shift(env_id_base, n_strategies), group_offsets, group_envs,
                     strategies, n_pools, lanes_per_pool(n_envs, n_strategies, n_pools), first, truncated);
  return hipGetLastError();
}

hipError_t launch_pool_pack(const gte_trade_stats* trades, const TradeList& tl, int n_envs, int n_strategies,
                            int64_t env_id_base, const int32_t* group_offsets, const int32_t* group_envs,
                            const int32_t* strategies, int n_pools, const int64_t* first, double* factors,
                            int64_t max_factors, hipStream_t stream) {
  if (!trades || !tl.list || tl.capacity < 1 || n_envs < 1 || n_strategies < 1 || !strategies || n_pools < 1 ||
      n_pools > GTE_MC_MAX_POOLS || !first || !factors || max_factors < 1 ||
      (group_offsets == nullptr) != (group_envs == nullptr))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_mc_pack_kernel, dim3((unsigned)n_pools), dim3(256), 0, stream, trades, tl.list, tl.capacity,
                     n_envs, n_strategies, members_first_shift(env_id_base, n_strategies), group_offsets, group_envs,
                     strategies, first, factors, max_factors);
  return hipGetLastError();
}

// ---- the resampling

struct McPhilox {
  __device__ __forceinline__ void operator()(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                             uint32_t k1, uint32_t o[4]) const {
    philox4x32_10(c0, c1, c2, c3, k0, k1, o);
  }
};
struct McFactors {  // factor j of a pool, in LDS or in place
  const double* base;
  __device__ __forceinline__ double operator()(int32_t j) const { return base[j]; }
};
struct McLevels {  // by value into the walk kernel
  double v[GTE_MC_MAX_LEVELS];
  int32_t n;
};
struct McColumns {  // the per-path outputs, any of them null
  double *final, *mdd, *low;
  int32_t* streak;
};
struct McPartials {  // the slabs' results, entry slab * n_pools + q of each array
  double* sum[4];    // final, final^2, mdd, mdd^2: x[0] of the slab's tree
  int32_t* cnt;      // MC_COUNTS arrays one after the other
};

__global__ __launch_bounds__(GTE_MC_SLAB) void gte_mc_walk_kernel(const double* __restrict__ factors,
                                                                  const int64_t* __restrict__ first,
                                                                  const uint32_t* __restrict__ streams, int n_pools,
                                                                  int R, int slabs, int path_len, uint32_t k0,
                                                                  uint32_t k1, double ruin, const McLevels lv,
                                                                  const McColumns col, const McPartials part) {
  __shared__ double lds[GTE_MC_LDS_POOL];  // the pool; after the walk the four trees, 256 places each
  __shared__ int32_t wcnt[GTE_MC_SLAB / 64][MC_COUNTS];
  const int tid = threadIdx.x, q = blockIdx.x / slabs, slab = blockIdx.x % slabs;
  const int64_t lo = first[q];
  const int32_t P = mc_pool_size(lo, first[q + 1], first[0], first[n_pools]);
  const int32_t L = mc_path_len(P, path_len);
  const int r = slab * GTE_MC_SLAB + tid;
  const bool live = r < R;
  const uint32_t st = streams ? streams[q] : (uint32_t)q;
  const double* pool = factors + (P > 0 ? lo : 0);
  McPath s;
  if (P <= GTE_MC_LDS_POOL) {  // (the whole workgroup: P is the pool's)
    // 16-byte loads from the first 16-byte aligned factor on; the one before it and an odd last one alone
    const int head = P > 0 && ((uintptr_t)pool & 8) ? 1 : 0, pairs = (P - head) >> 1;
    const double2* src = reinterpret_cast<const double2*>(pool + head);
    for (int k = tid; k < pairs; k += GTE_MC_SLAB) {
      const double2 v = src[k];
      lds[head + 2 * k] = v.x;
      lds[head + 2 * k + 1] = v.y;
    }
    if (tid == 0 && head) lds[0] = pool[0];
    if (tid == 1 && ((P - head) & 1)) lds[P - 1] = pool[P - 1];
    __syncthreads();
    s = mc_walk(McPhilox(), McFactors{lds}, P, live ? L : 0, (uint32_t)r, st, k0, k1);
    __syncthreads();  // (the trees take the pool's place)
  } else {
    s = mc_walk(McPhilox(), McFactors{pool}, P, live ? L : 0, (uint32_t)r, st, k0, k1);
  }
  const int64_t row = (int64_t)q * R + r;
  if (live) {
    if (col.final) col.final[row] = s.e;
    if (col.mdd) col.mdd[row] = s.mdd;
    if (col.low) col.low[row] = s.low;
    if (col.streak) col.streak[row] = s.max_streak;
  }
  double* const t0 = lds;
  double* const t1 = lds + GTE_MC_SLAB;
  double* const t2 = lds + 2 * GTE_MC_SLAB;
  double* const t3 = lds + 3 * GTE_MC_SLAB;
  t0[tid] = live ? s.e : 0.0;
  t1[tid] = live ? s.e * s.e : 0.0;
  t2[tid] = live ? s.mdd : 0.0;
  t3[tid] = live ? s.mdd * s.mdd : 0.0;
  const int wave = tid >> 6;
  {  // the counts: a ballot per wavefront, its first lane into LDS
    const int loss = __popcll(__ballot(live && s.e < 1.0)), ruined = __popcll(__ballot(live && s.low <= ruin));
    if ((tid & 63) == 0) {
      wcnt[wave][0] = loss;
      wcnt[wave][1] = ruined;
    }
    for (int k = 0; k < lv.n; ++k) {
      const int ge = __popcll(__ballot(live && s.mdd >= lv.v[k]));
      if ((tid & 63) == 0) wcnt[wave][2 + k] = ge;
    }
  }
  __syncthreads();
  for (int h = GTE_MC_SLAB / 2; h > 0; h >>= 1) {
    mc_tree_level(t0, tid, h);
    mc_tree_level(t1, tid, h);
    mc_tree_level(t2, tid, h);
    mc_tree_level(t3, tid, h);
    __syncthreads();
  }
  const size_t cell = (size_t)slab * (size_t)n_pools + (size_t)q, cells = (size_t)slabs * (size_t)n_pools;
  if (tid < 4) part.sum[tid][cell] = lds[tid * GTE_MC_SLAB];
  if (tid < 2 + lv.n) {
    int total = 0;
    for (int w = 0; w < GTE_MC_SLAB / 64; ++w) total += wcnt[w][tid];
    part.cnt[(size_t)tid * cells + cell] = total;
  }
}

__global__ __launch_bounds__(256) void gte_mc_close_kernel(const int64_t* __restrict__ first, int n_pools, int slabs,
                                                           int path_len, int n_levels, const McPartials part,
                                                           gte_mc_pool* __restrict__ out,
                                                           int32_t* __restrict__ dd_count) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n_pools) return;
  const size_t cells = (size_t)slabs * (size_t)n_pools;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  int cnt[MC_COUNTS];
#pragma unroll
  for (int c = 0; c < MC_COUNTS; ++c) cnt[c] = 0;
  for (int j = 0; j < slabs; ++j) {
    const size_t cell = (size_t)j * (size_t)n_pools + (size_t)q;
#pragma unroll
    for (int c = 0; c < 4; ++c) sum[c] = sum[c] + part.sum[c][cell];
#pragma unroll
    for (int c = 0; c < MC_COUNTS; ++c)
      if (c < 2 + n_levels) cnt[c] += part.cnt[(size_t)c * cells + cell];
  }
  const int32_t P = mc_pool_size(first[q], first[q + 1], first[0], first[n_pools]);
  const double2 d0 = {sum[0], sum[1]}, d1 = {sum[2], sum[3]};
  const int4 c2 = {cnt[0], cnt[1], P, mc_path_len(P, path_len)};
  gte_mc_pool* dst = out + q;
  reinterpret_cast<double2*>(dst)[0] = d0;
  reinterpret_cast<double2*>(dst)[1] = d1;
  reinterpret_cast<int4*>(dst)[2] = c2;
#pragma unroll
  for (int k = 0; k < GTE_MC_MAX_LEVELS; ++k)
    if (k < n_levels) dd_count[(size_t)q * n_levels + k] = cnt[2 + k];
}

// the library's scratch of one gte_trade_monte_carlo, carved out of one allocation (ScratchCarver, gte_launch.h)
struct McScratch {
  McPartials part;
  size_t bytes;
};
static McScratch mc_carve(void* base, int n_pools, int R, int n_levels) {
  const size_t cells = (size_t)((R + GTE_MC_SLAB - 1) / GTE_MC_SLAB) * (size_t)n_pools;
  ScratchCarver c = {(char*)base, 0};
  McScratch m;
  for (int k = 0; k < 4; ++k) m.part.sum[k] = c.take<double>(cells);
  m.part.cnt = c.take<int32_t>(cells * (size_t)(2 + n_levels));
  m.bytes = c.at;
  return m;
}

size_t monte_carlo_scratch_bytes(int n_pools, int n_resamples, int n_levels) {
  return mc_carve(nullptr, n_pools, n_resamples, n_levels).bytes;
}

hipError_t launch_trade_monte_carlo(const double* factors, const int64_t* first, const uint32_t* streams, int n_pools,
                                    int n_resamples, int path_len, uint64_t seed, double ruin_level,
                                    const double* dd_levels, int n_levels, const gte_mc_out& out, void* scratch,
                                    hipStream_t stream) {
  if (!factors || !first || !scratch || n_pools < 1 || n_pools > GTE_MC_MAX_POOLS || n_resamples < 1 ||
      n_resamples > GTE_MC_MAX_RESAMPLES || path_len < 0 || path_len > GTE_MC_MAX_PATH || n_levels < 0 ||
      n_levels > GTE_MC_MAX_LEVELS || (n_levels > 0 && (!dd_levels || !out.dd_count)) || !out.pool ||
      ruin_level != ruin_level)
    return hipErrorInvalidValue;
  const int R = n_resamples, slabs = (R + GTE_MC_SLAB - 1) / GTE_MC_SLAB;
  const McScratch m = mc_carve(scratch, n_pools, R, n_levels);
  McLevels lv = {};
  lv.n = n_levels;
  for (int k = 0; k < n_levels; ++k) lv.v[k] = dd_levels[k];
  const McColumns col = {out.final, out.max_drawdown, out.low, out.max_loss_streak};
  hipLaunchKernelGGL(gte_mc_walk_kernel, dim3((unsigned)((int64_t)n_pools * slabs)), dim3(GTE_MC_SLAB), 0, stream,
                     factors, first, streams, n_pools, R, slabs, path_len, (uint32_t)seed, (uint32_t)(seed >> 32),
                     ruin_level, lv, col, m.part);
  hipLaunchKernelGGL(gte_mc_close_kernel, dim3((unsigned)((n_pools + 255) / 256)), dim3(256), 0, stream, first,
                     n_pools, slabs, path_len, n_levels, m.part, out.pool, out.dd_count);
  return hipGetLastError();
}

}  // namespace gte
