// own_check.cpp — csrc/gte_own.h on the CPU (tests/test_own_cpu.py builds this with g++ under ASan + UBSan and runs
// it as a program of its own).  The owner is bound to malloc / free plus a counter of releases, so that every
// rule of the header is checked by count: a block is released exactly once, by replace, reset, the destructor or
// never by a moved-from owner.  `own_check leak` lets a block go on purpose: LeakSanitizer must report it.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "gte_own.h"

static int released = 0;
static void* last_released = nullptr;
static void counted_free(void* p) {
  released += 1;
  last_released = p;
  free(p);
}
using Block = gte_own::Block<counted_free>;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

static void owner() {
  {
    Block b;
    CHECK(b.get() == nullptr && b.bytes() == 0);
    b.reset();  // an empty owner: nothing happens
    CHECK(released == 0);
    void* first = malloc(16);
    b.replace(first, 16);  // adopts, releases nothing
    CHECK(released == 0 && b.get() == first && b.bytes() == 16 && b.as<char>() == (char*)first);
    void* second = malloc(32);
    b.replace(second, 32);  // the old block exactly once, the new one adopted
    CHECK(released == 1 && last_released == first && b.get() == second && b.bytes() == 32);
    b.reset();
    CHECK(released == 2 && last_released == second && !b.get() && b.bytes() == 0);
    b.reset();  // a second reset releases nothing
    CHECK(released == 2);
    b.replace(malloc(8), 8);
  }  // the destructor releases a held block
  CHECK(released == 3);
  {
    Block a;
    a.replace(malloc(8), 8);
    void* held = a.get();
    Block b(std::move(a));  // a moved-from owner holds nothing and releases nothing
    CHECK(!a.get() && a.bytes() == 0 && b.get() == held && b.bytes() == 8);
    a.reset();
    CHECK(released == 3);
    Block c;
    c.replace(malloc(4), 4);
    void* old = c.get();
    c = std::move(b);  // move assignment: what c held is released, b's block adopted
    CHECK(released == 4 && last_released == old && c.get() == held && !b.get());
  }  // a and b release nothing, c its block
  CHECK(released == 5);
  puts("owner ok");
}

static void growth() {
  const size_t cases[4][2] = {{0, 1}, {100, 100}, {100, 101}, {100, 250}};
  for (const auto& c : cases) {
    const size_t have = c[0], need = c[1];
    CHECK(gte_own::grow_exact(have, need) == need);
    CHECK(gte_own::grow_by_half(have, need) == need + need / 2);
    const size_t twice = 2 * have > need ? 2 * have : need;
    CHECK(gte_own::grow_doubling(have, need) == (have < need ? twice : have));
  }
  CHECK(gte_own::grow_doubling(0, 1) == 1 && gte_own::grow_doubling(100, 100) == 100);
  CHECK(gte_own::grow_doubling(100, 101) == 200 && gte_own::grow_doubling(100, 250) == 250);
  CHECK(gte_own::grow_by_half(100, 101) == 151 && gte_own::grow_by_half(0, 1) == 1);
  puts("growth ok");
}

int main(int argc, char** argv) {
  if (argc > 1 && argv[1][0] == 'l') {  // "leak": a block no owner holds at exit
    Block* forgotten = new Block;
    forgotten->replace(malloc(24), 24);
    forgotten = nullptr;
    puts("leaked one block");
    fflush(stdout);  // (LeakSanitizer ends the process without flushing)
    return 0;
  }
  owner();
  growth();
  return 0;
}
