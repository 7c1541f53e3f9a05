/* gte_mc.h — the trade Monte Carlo of include/gte.h (gte_trade_monte_carlo) as code: which factors a pool holds, how
 * long a path is, which factor a draw takes, one step of the walk and one level of the slab tree.  Plain C++ behind
 * __device__ / __forceinline__, nothing of HIP: csrc/gte_montecarlo.hip compiles it for the device, and a host
 * program defines the two qualifiers away and replays the device's bits (tests/mc_check.cpp holds it to
 * tests/monte_carlo_model.py).  The Philox is the caller's: anything with
 *     void operator()(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o[4])
 * that computes philox4x32_10. */
#ifndef GTE_MC_H_
#define GTE_MC_H_
#include <stdint.h>

namespace gte {

constexpr int MC_SLAB = 256;                 /* GTE_MC_SLAB */
constexpr int32_t MC_MAX_PATH = 1 << 20;     /* GTE_MC_MAX_PATH */
constexpr uint32_t MC_TAG = 0x54524D43u;     /* 'TRMC': word 3 of the counter */

/* the size of the pool [lo, hi) of a table whose whole span is [span_lo, span_hi): 0 for a reversed pool, one of 2^31
 * factors or more, and one that reaches outside the span */
__device__ __forceinline__ int32_t mc_pool_size(int64_t lo, int64_t hi, int64_t span_lo, int64_t span_hi) {
  if (hi < lo || lo < span_lo || hi > span_hi) return 0;
  const uint64_t n = (uint64_t)hi - (uint64_t)lo;
  return n >= ((uint64_t)1 << 31) ? 0 : (int32_t)n;
}

/* L of a pool of P factors */
__device__ __forceinline__ int32_t mc_path_len(int32_t P, int32_t path_len) {
  if (P == 0) return 0;
  if (path_len > 0) return path_len;
  return P < MC_MAX_PATH ? P : MC_MAX_PATH;
}

/* mulhi32(word, P): the place in the pool a draw takes */
__device__ __forceinline__ int32_t mc_index(uint32_t word, int32_t P) {
  return (int32_t)(((uint64_t)word * (uint64_t)(uint32_t)P) >> 32);
}

struct McPath {
  double e, peak, mdd, low;
  int32_t streak, max_streak;
};

__device__ __forceinline__ McPath mc_start() {
  McPath s = {1.0, 1.0, 0.0, 1.0, 0, 0};
  return s;
}

/* one trade of factor f */
__device__ __forceinline__ void mc_step(McPath& s, double f) {
  s.e = s.e * f;
  if (s.e > s.peak) s.peak = s.e;
  const double d = 1.0 - s.e / s.peak;
  if (d > s.mdd) s.mdd = d;
  if (s.e < s.low) s.low = s.e;
  if (f < 1.0) {
    s.streak += 1;
    if (s.streak > s.max_streak) s.max_streak = s.streak;
  } else {
    s.streak = 0;
  }
}

/* the walk of resample r over a pool of P factors, L trades long; at(j) is factor j of the pool */
template <typename Philox, typename Pool>
__device__ __forceinline__ McPath mc_walk(Philox philox, const Pool& at, int32_t P, int32_t L, uint32_t r,
                                          uint32_t stream, uint32_t k0, uint32_t k1) {
  McPath s = mc_start();
  uint32_t o[4] = {0, 0, 0, 0};
  for (int32_t i0 = 0; i0 < L; i0 += 4) {  /* one Philox block per four draws: draw i takes word i & 3 of block i >> 2 */
    philox((uint32_t)(i0 >> 2), r, stream, MC_TAG, k0, k1, o);
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k)
      if (i0 + k < L) mc_step(s, at(mc_index(o[k], P)));
  }
  return s;
}

/* level h (128, 64, ..., 1) of the slab tree for place i: every place of a level before any of the next */
__device__ __forceinline__ void mc_tree_level(double* x, int i, int h) {
  if (i < h) x[i] = x[i] + x[i + h];
}

}  /* namespace gte */
#endif /* GTE_MC_H_ */
