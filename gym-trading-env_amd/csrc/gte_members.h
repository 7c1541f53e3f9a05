// gte_members.h — which envs belong to a strategy, and which periods a mask selects: the two rules
// include/gte.h promises for every reduction and ranking of per-strategy records, stated once for
// gte_strategy.hip, gte_trade_strategy.hip, gte_period_strategy.hip and the three leaderboard analyses, which
// all take their periods as a PeriodMask: gte_bootstrap.hip (as BootMask), gte_cscv.hip (one per group) and
// gte_diversify.hip.  Plain C++ behind __device__ / __forceinline__ (tests/test_strategy_records_cpu.py
// compiles it for the host with both defined away and holds it to tests/strategy_model.py).
#pragma once
#include <stdint.h>

namespace gte {

// the member list of strategy s: n places; place m holds env first + m * S (default map) or envs[lo + m]
struct Members {
  int n, lo;
  long long first;
};
__device__ __forceinline__ Members members_of(int s, int N, int S, unsigned first_shift, const int32_t* offsets) {
  Members g = {0, 0, 0};
  if (offsets) {
    const int o0 = offsets[s], o1 = offsets[s + 1];
    g.lo = o0 < 0 ? 0 : o0 > N ? N : o0;
    const int hi = o1 < g.lo ? g.lo : o1 > N ? N : o1;
    g.n = hi - g.lo;
  } else {
    g.first = ((unsigned)s + first_shift) % (unsigned)S;
    g.n = g.first < N ? (int)(((long long)N - g.first + S - 1) / S) : 0;
  }
  return g;
}

// env of place m < g.n, or -1 where the entry names no env in [0, N)
__device__ __forceinline__ long long member_env(const Members& g, const int32_t* envs, int N, int S, int m) {
  if (!envs) return g.first + (long long)m * S;
  const int id = envs[g.lo + m];
  return (unsigned)id < (unsigned)N ? (long long)id : -1;
}

// the default map's first_shift (host): (s + shift) % S = (s - env_id_base) mod S, the first env of strategy s
inline unsigned members_first_shift(int64_t env_id_base, int64_t S) {
  return (unsigned)((S - ((env_id_base % S) + S) % S) % S);
}

// a set of periods, bit b of the two words = period b (GTE_MAX_PERIODS = 128); crosses into kernels by value
struct PeriodMask {
  uint64_t w[2];
  __device__ __forceinline__ bool has(int b) const { return (w[b >> 6] >> (b & 63)) & 1; }
};

}  // namespace gte
