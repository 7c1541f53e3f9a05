// tests/members_check.cpp — csrc/gte_members.h on the host (tests/test_strategy_records_cpu.py): the member rule
// and the period mask's bit test, compiled with g++ with the device qualifiers defined away, printed for Python
// to hold against tests/strategy_model.py.
//   members_check members N S env_id_base [offsets[0..S] envs...]   one line per strategy: the env of every place
//                                                                   (-1: an entry that names no env)
//   members_check mask w0 w1                                        the periods the two words select
#define __device__
#define __forceinline__ inline
#include "gte_members.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "mask")) {
    const gte::PeriodMask mask = {{strtoull(argv[2], nullptr, 0), strtoull(argv[3], nullptr, 0)}};
    for (int b = 0; b < 128; ++b)
      if (mask.has(b)) printf("%d\n", b);
    return 0;
  }
  if (argc < 5 || strcmp(argv[1], "members")) return 2;
  const int N = atoi(argv[2]), S = atoi(argv[3]);
  const long long base = atoll(argv[4]);
  std::vector<int32_t> lists;
  for (int i = 5; i < argc; ++i) lists.push_back((int32_t)atoi(argv[i]));
  if (!lists.empty() && (int)lists.size() < S + 1) return 2;
  const int32_t* offsets = lists.empty() ? nullptr : lists.data();
  const int32_t* envs = lists.empty() ? nullptr : lists.data() + S + 1;
  const unsigned shift = gte::members_first_shift(base, S);
  for (int s = 0; s < S; ++s) {
    const gte::Members g = gte::members_of(s, N, S, shift, offsets);
    // (a list may not reach past the entries that exist: the kernels read envs[lo + m] for m < n)
    if (offsets && (g.lo < 0 || g.n < 0 || g.lo + g.n > (int)lists.size() - (S + 1))) return 3;
    printf("%d:", s);
    for (int m = 0; m < g.n; ++m) printf(" %lld", gte::member_env(g, envs, N, S, m));
    printf("\n");
  }
  return 0;
}
