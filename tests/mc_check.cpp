// tests/mc_check.cpp — include/gte_mc.h on the host (tests/test_monte_carlo_model_cpu.py): the pool and path sizes, the
// index mapping, the walk and the slab tree of gte_trade_monte_carlo, compiled with g++ with the device qualifiers
// defined away and a Philox of its own passed in, printed for Python to hold against tests/monte_carlo_model.py.
//   mc_check <file>    the file holds unsigned integers separated by white space, doubles as their 64 bits:
//       R path_len seed ruin n_levels level[n_levels] n_pools stream[n_pools] first[n_pools + 1] n_factors factor[..]
//   prints per pool   "pool P L final_sum final_sq_sum mdd_sum mdd_sq_sum count_loss count_ruin dd_count[n_levels]"
//   and per resample  "row final max_drawdown low max_loss_streak"          (doubles as their 64 bits again)
#define __device__
#define __forceinline__ inline
#include "gte_mc.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// philox4x32_10 (Salmon et al. 2011), the generator include/gte.h names
struct HostPhilox {
  void operator()(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o[4]) const {
    for (int r = 0; r < 10; ++r) {
      const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
      const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
      c1 = (uint32_t)p1;
      c3 = (uint32_t)p0;
      c0 = n0;
      c2 = n2;
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
  }
};

struct HostFactors {
  const double* base;
  double operator()(int32_t j) const { return base[j]; }
};

static double as_double(uint64_t bits) {
  double d;
  memcpy(&d, &bits, 8);
  return d;
}
static unsigned long long as_bits(double d) {
  uint64_t bits;
  memcpy(&bits, &d, 8);
  return bits;
}

static double slab_sum(const std::vector<double>& x) {
  double total = 0.0;
  for (size_t lo = 0; lo < x.size(); lo += gte::MC_SLAB) {
    double place[gte::MC_SLAB];
    for (int i = 0; i < gte::MC_SLAB; ++i) place[i] = lo + i < x.size() ? x[lo + i] : 0.0;
    for (int h = gte::MC_SLAB / 2; h > 0; h >>= 1)
      for (int i = 0; i < gte::MC_SLAB; ++i) gte::mc_tree_level(place, i, h);
    total = total + place[0];
  }
  return total;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 2;
  std::vector<uint64_t> t;
  unsigned long long v;
  while (fscanf(in, "%llu", &v) == 1) t.push_back(v);
  fclose(in);
  size_t at = 0;
  auto next = [&]() -> uint64_t {
    if (at >= t.size()) exit(3);
    return t[at++];
  };
  const int R = (int)next(), path_len = (int)next();
  const uint64_t seed = next();
  const double ruin = as_double(next());
  const int n_levels = (int)next();
  std::vector<double> levels;
  for (int k = 0; k < n_levels; ++k) levels.push_back(as_double(next()));
  const int n_pools = (int)next();
  std::vector<uint32_t> stream;
  for (int q = 0; q < n_pools; ++q) stream.push_back((uint32_t)next());
  std::vector<int64_t> first;
  for (int q = 0; q <= n_pools; ++q) first.push_back((int64_t)next());
  const size_t n_factors = (size_t)next();
  std::vector<double> factors;
  for (size_t i = 0; i < n_factors; ++i) factors.push_back(as_double(next()));
  for (int q = 0; q < n_pools; ++q) {
    const int32_t P = gte::mc_pool_size(first[q], first[q + 1], first[0], first[n_pools]);
    const int32_t L = gte::mc_path_len(P, path_len);
    if (P > 0 && (first[q] < 0 || (size_t)(first[q] + P) > n_factors)) return 4;  // (the caller's obligation)
    const HostFactors pool = {factors.data() + (P > 0 ? first[q] : 0)};
    std::vector<gte::McPath> rows;
    std::vector<double> x[4];
    int loss = 0, ruined = 0;
    std::vector<int> ge(n_levels, 0);
    for (int r = 0; r < R; ++r) {
      const gte::McPath s = gte::mc_walk(HostPhilox(), pool, P, L, (uint32_t)r, stream[q], (uint32_t)seed,
                                         (uint32_t)(seed >> 32));
      rows.push_back(s);
      x[0].push_back(s.e);
      x[1].push_back(s.e * s.e);
      x[2].push_back(s.mdd);
      x[3].push_back(s.mdd * s.mdd);
      loss += s.e < 1.0 ? 1 : 0;
      ruined += s.low <= ruin ? 1 : 0;
      for (int k = 0; k < n_levels; ++k) ge[k] += s.mdd >= levels[k] ? 1 : 0;
    }
    printf("pool %d %d %llu %llu %llu %llu %d %d", P, L, as_bits(slab_sum(x[0])), as_bits(slab_sum(x[1])),
           as_bits(slab_sum(x[2])), as_bits(slab_sum(x[3])), loss, ruined);
    for (int k = 0; k < n_levels; ++k) printf(" %d", ge[k]);
    printf("\n");
    for (const gte::McPath& s : rows)
      printf("row %llu %llu %llu %d\n", as_bits(s.e), as_bits(s.mdd), as_bits(s.low), s.max_streak);
  }
  return 0;
}
