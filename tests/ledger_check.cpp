// ledger_check.cpp — csrc/gte_ledger.h against a brute-force model, on the CPU (tests/test_ledger_cpu.py
// builds this with g++ and the sanitizers and runs it; nothing here touches a GPU).
//
//   ledger_check model     fixed-seed random sequences and scripted ones, ledger and model side by side
//   ledger_check threads   4 threads, one env each, overlapping ranges, the process-wide ledger (for TSan)
//
// The model is a 256-byte address space.  Per byte: the launch that wrote it last (env incarnation and serial
// number) and who wrote it inside a capture.  Per env and kind: the serial of the env's most recent launch,
// if that launch was an eager step or a reset that establishes (or, masked, carries on) the claim: 0 if not.
// SOUNDNESS: whenever the ledger says env E holds a claim over some ranges, every byte of them was last
// written by exactly that launch of E (so by no other launch since) and is not capture-tainted.
// The operations call the ledger in the order gte_api.hip does (the table in gte_ledger.h).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "gte_ledger.h"

using gte_ledger::FLAGS;
using gte_ledger::Kind;
using gte_ledger::Ledger;
using gte_ledger::Span;
using gte_ledger::WINDOW;

#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                          \
      fprintf(stderr, "\n");                                 \
      exit(1);                                               \
    }                                                        \
  } while (0)

namespace {

constexpr int SPACE = 256, ENVS = 3, NFLAGS = 8;
alignas(16) unsigned char g_space[SPACE];  // addresses only: never read or written

struct Range { int off, len; };
Span span(Range r) { return {g_space + r.off, (size_t)r.len}; }
// flag buffers (NFLAGS bytes each; 4 overlaps 0 and 8) and observation buffers (two pairs overlap; the
// last one lies over three of the flag buffers)
const Range FLAG_BUFS[] = {{0, NFLAGS}, {8, NFLAGS}, {16, NFLAGS}, {24, NFLAGS}, {32, NFLAGS}, {40, NFLAGS}, {4, NFLAGS}};
const Range OBS_BUFS[] = {{64, 48}, {96, 48}, {144, 48}, {192, 48}, {208, 48}, {20, 44}};
constexpr int N_FLAG_BUFS = 7, N_OBS_BUFS = 6;

struct Byte {
  long writer = 0;         // env incarnation of the launch that wrote it last (0: nobody)
  long serial = 0;         // ... and that launch's serial number
  unsigned captured_by = 0;  // living envs (bit per slot) that wrote it inside a capture
  bool captured_ever = false;
};

struct Env {
  bool alive = false;
  long incarnation = 0;
  Range term{}, trunc{}, obs{};
  bool sliding = false;
  long good[2] = {0, 0};  // [FLAGS, WINDOW], see the head of this file
};
int slot_of(Kind k) { return k == FLAGS ? 0 : 1; }

struct World {
  Ledger ledger;
  Byte bytes[SPACE];
  Env env[ENVS];
  long serial = 0, incarnations = 0;
  long asked[2] = {0, 0}, granted[2] = {0, 0};  // step queries of eager steps
  unsigned inner = 0;  // what the last rollout's own step launch was granted

  const void* key(int e) const { return &env[e]; }

  // ---- the model ---------------------------------------------------------------------------------
  void model_write(int e, Range r, long s, bool captured) {
    for (int i = r.off; i < r.off + r.len; ++i) {
      bytes[i].writer = env[e].incarnation;
      bytes[i].serial = s;
      if (captured) { bytes[i].captured_by |= 1u << e; bytes[i].captured_ever = true; }
    }
  }
  // does every byte of r hold what E's launch `good` of that kind wrote, untouched and untainted?
  bool model_true(int e, Kind k, Range r) const {
    const long good = env[e].good[slot_of(k)];
    if (!good) return false;
    for (int i = r.off; i < r.off + r.len; ++i) {
      const Byte& b = bytes[i];
      if (b.writer != env[e].incarnation || b.serial != good) return false;
      // FLAGS: never, as the ledger rules; WINDOW: not while the env that captured lives
      if (k == FLAGS ? b.captured_ever : b.captured_by != 0) return false;
    }
    return true;
  }
  // the ledger's answer, held against the model
  bool ask(int e, Kind k, Range a, Range b, const char* what) {
    const bool held = k == FLAGS ? ledger.holds(key(e), k, {span(a), span(b)}) : ledger.holds(key(e), k, {span(a)});
    if (held) {
      CHECK(model_true(e, k, a), "%s: env %d holds kind %u over [%d,+%d) and the model disagrees", what, e, (unsigned)k, a.off, a.len);
      if (k == FLAGS) CHECK(model_true(e, k, b), "%s: env %d holds FLAGS over [%d,+%d) and the model disagrees", what, e, b.off, b.len);
    }
    return held;
  }
  // soundness, for every env, both kinds, its bound buffers and a neighbouring choice of buffers
  void check(const char* what) {
    for (int e = 0; e < ENVS; ++e) {
      if (!env[e].alive) {
        CHECK(!ledger.holds(key(e), FLAGS, {span(FLAG_BUFS[0]), span(FLAG_BUFS[1])}), "%s: a dead env holds", what);
        continue;
      }
      ask(e, FLAGS, env[e].term, env[e].trunc, what);
      ask(e, FLAGS, env[e].trunc, env[e].term, what);  // (the same bytes, the other way round: other contents)
      ask(e, WINDOW, env[e].obs, {}, what);
      for (int i = 0; i + 1 < N_FLAG_BUFS; ++i) ask(e, FLAGS, FLAG_BUFS[i], FLAG_BUFS[i + 1], what);
      for (int i = 0; i < N_OBS_BUFS; ++i) ask(e, WINDOW, OBS_BUFS[i], {}, what);
    }
  }

  // ---- the entry points, as gte_api.hip calls the ledger -----------------------------------------
  void create(int e, Range term, Range trunc, Range obs, bool sliding) {
    CHECK(!env[e].alive, "create of a living env");
    env[e] = Env();
    env[e].alive = true;
    env[e].incarnation = ++incarnations;
    env[e].term = term; env[e].trunc = trunc; env[e].obs = obs; env[e].sliding = sliding;
    if (sliding) ledger.wrote(key(e), {span(obs)}, false, WINDOW);  // gte_bind_sliding_obs
    check("create");
  }
  void destroy(int e) {
    ledger.forget(key(e));
    env[e].alive = false;
    for (Byte& b : bytes) b.captured_by &= ~(1u << e);  // its graphs died with it
    check("destroy");
  }
  // enqueue_step into the env's own buffers; returns the kinds granted (sparse flags, slide)
  unsigned step(int e, bool captured) {
    Env& E = env[e];
    unsigned got = 0;
    // (the model is held against the answer at the very moment it is used)
    if (E.sliding && !captured) {
      ++asked[1];
      if (ask(e, WINDOW, E.obs, {}, "step")) { got |= WINDOW; ++granted[1]; }
    }
    if (!captured) {
      ++asked[0];
      if (ask(e, FLAGS, E.term, E.trunc, "step")) { got |= FLAGS; ++granted[0]; }
    }
    ledger.wrote(key(e), {span(E.obs), span(E.term), span(E.trunc)}, captured, FLAGS | WINDOW);
    ledger.establish(key(e), FLAGS, {span(E.term), span(E.trunc)}, captured);
    if (E.sliding) ledger.establish(key(e), WINDOW, {span(E.obs)}, captured);
    // the model: a step writes every flag and every window, in effect (a sparse or slide step leaves the
    // bytes it skips as they are, which is what it would have written)
    const long s = ++serial;
    model_write(e, E.obs, s, captured);
    model_write(e, E.term, s, captured);
    model_write(e, E.trunc, s, captured);
    E.good[0] = captured ? 0 : s;
    E.good[1] = captured || !E.sliding ? 0 : s;
    check(captured ? "captured step" : "step");
    return got;
  }
  void reset(int e, bool masked) {
    Env& E = env[e];
    const bool fresh_run = E.sliding && !masked;
    // a masked reset carries the window claim on only if it was true before
    const bool carried = masked && E.sliding && model_true(e, WINDOW, E.obs);
    ledger.wrote(key(e), {span(E.obs), span(E.term), span(E.trunc)}, false, fresh_run ? FLAGS | WINDOW : FLAGS);
    if (fresh_run) ledger.establish(key(e), WINDOW, {span(E.obs)}, false);
    const long s = ++serial;
    model_write(e, E.obs, s, false);
    model_write(e, E.term, s, false);
    model_write(e, E.trunc, s, false);
    E.good[0] = 0;  // (masked envs get zero flags: not what a step stored)
    E.good[1] = fresh_run || carried ? s : 0;
    check(masked ? "masked reset" : "reset");
  }
  // gte_rollout with per-step rows in `rows_*` (len 0: none), or gte_backtest (no rows); last_step: its
  // last step goes out as an ordinary launch into the env's own buffers (the state-only and backtest paths)
  void rollout(int e, Range rows_obs, Range rows_term, Range rows_trunc, bool captured, bool last_step) {
    Env& E = env[e];
    ledger.wrote(key(e), {span(rows_obs), span(rows_term), span(rows_trunc), span(E.term), span(E.trunc)}, captured,
                 WINDOW);
    long s = ++serial;
    for (Range r : {rows_obs, rows_term, rows_trunc, E.term, E.trunc}) model_write(e, r, s, captured);
    E.good[1] = 0;  // (the envs advanced and the own observation buffer was not written)
    // the fused kernels store the env's own flags densely (Params.flags_sparse is 0 in them) and keep flags_out
    // with them: what a dense step would have left, so a step launch of the rollout's own may store sparsely
    E.good[0] = captured ? 0 : s;
    check("rollout's fused launch");
    inner = last_step ? step(e, captured) : 0;
    ledger.withdraw(key(e), FLAGS);
    s = ++serial;  // the copies of the last row into the env's own flags
    model_write(e, E.term, s, captured);
    model_write(e, E.trunc, s, captured);
    E.good[0] = 0;
    check("rollout");
  }
  void bind_returns(int e, Range term, Range trunc) {
    ledger.withdraw(key(e), FLAGS);
    env[e].term = term; env[e].trunc = trunc;
    check("bind_returns");
  }
  void bind_outputs(int e, Range obs, Range term, Range trunc) {  // classic layout
    env[e].sliding = false;
    env[e].obs = obs; env[e].term = term; env[e].trunc = trunc;
    ledger.wrote(key(e), {span(obs)}, false, FLAGS | WINDOW);
    check("bind_outputs");
  }
  void bind_sliding(int e, Range obs) {
    env[e].sliding = true;
    env[e].obs = obs;
    ledger.wrote(key(e), {span(obs)}, false, WINDOW);
    check("bind_sliding_obs");
  }
  void set_schedule(int e) {
    ledger.withdraw(key(e), FLAGS | WINDOW);
    check("set_schedule");
  }
};

// ---- random sequences ------------------------------------------------------------------------------
void random_sequences(long totals_asked[2], long totals_granted[2]) {
  for (unsigned seed = 1; seed <= 300; ++seed) {
    std::mt19937 rng(seed);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    World w;
    auto flags_of = [&](int e, Range* term, Range* trunc) {
      // mostly a pair of its own, now and then any pair (shared or overlapping with another env's)
      if (pick(4)) { *term = FLAG_BUFS[2 * e]; *trunc = FLAG_BUFS[2 * e + 1]; }
      else { *term = FLAG_BUFS[pick(N_FLAG_BUFS)]; *trunc = FLAG_BUFS[pick(N_FLAG_BUFS)]; }
    };
    // (never over the env's OWN flag buffers t and u: no launch could write both and mean either)
    auto apart = [](Range a, Range b) { return a.off + a.len <= b.off || b.off + b.len <= a.off; };
    auto obs_of = [&](int e, Range t, Range u) {
      for (;;) {
        const Range o = pick(4) ? OBS_BUFS[e == 0 ? 0 : e == 1 ? 2 : 4] : OBS_BUFS[pick(N_OBS_BUFS)];
        if (apart(o, t) && apart(o, u)) return o;
      }
    };
    auto create = [&](int e) {
      Range t, u;
      flags_of(e, &t, &u);
      w.create(e, t, u, obs_of(e, t, u), pick(3) != 0);
      w.reset(e, false);
    };
    for (int e = 0; e < ENVS; ++e) create(e);
    for (int op = 0; op < 150; ++op) {
      const int e = pick(ENVS);
      const int r = pick(1000);  // (eager steps dominate; a capture spoils its ranges for good, so few of them)
      Range t, u;
      if (r < 720) w.step(e, false);
      else if (r < 725) { w.step(e, true); w.step(e, true); w.set_schedule(e); }  // a capture of two steps
      else if (r < 755) w.reset(e, true);
      else if (r < 780) w.reset(e, false);
      else if (r < 810) w.rollout(e, OBS_BUFS[pick(N_OBS_BUFS)], FLAG_BUFS[pick(N_FLAG_BUFS)], FLAG_BUFS[pick(N_FLAG_BUFS)], false, pick(2));
      else if (r < 840) w.rollout(e, {}, {}, {}, false, true);  // backtest
      else if (r < 842) w.rollout(e, {}, FLAG_BUFS[pick(N_FLAG_BUFS)], {}, true, pick(2));  // a captured rollout
      else if (r < 880) {
        do flags_of(e, &t, &u); while (!apart(t, w.env[e].obs) || !apart(u, w.env[e].obs));
        w.bind_returns(e, t, u);
      }
      else if (r < 910) { flags_of(e, &t, &u); w.bind_outputs(e, obs_of(e, t, u), t, u); }
      else if (r < 940) w.bind_sliding(e, obs_of(e, w.env[e].term, w.env[e].trunc));
      else if (r < 975) w.set_schedule(e);
      else { w.destroy(e); create(e); }
    }
    for (int k = 0; k < 2; ++k) { totals_asked[k] += w.asked[k]; totals_granted[k] += w.granted[k]; }
  }
}

// ---- scripted sequences: liveness ----------------------------------------------------------------
const Range T0 = FLAG_BUFS[0], U0 = FLAG_BUFS[1], T1 = FLAG_BUFS[2], U1 = FLAG_BUFS[3], T2 = FLAG_BUFS[4], U2 = FLAG_BUFS[5];
const Range O0 = OBS_BUFS[0], O1 = OBS_BUFS[2], O_OVER_0 = OBS_BUFS[1];

void scripted() {
  {  // from its second eager step on, an env stepping into the same buffers holds both claims
    World w;
    w.create(0, T0, U0, O0, true);
    // (no reset: nothing claimed yet)
    CHECK(w.step(0, false) == 0, "the first step is dense and full");
    for (int i = 0; i < 5; ++i) CHECK(w.step(0, false) == (FLAGS | WINDOW), "step %d", i + 2);
    // ... and after an unmasked reset the window claim is there at once, the flag claim after one step
    w.reset(0, false);
    CHECK(w.step(0, false) == WINDOW, "the step after a reset slides and stores its flags densely");
    CHECK(w.step(0, false) == (FLAGS | WINDOW), "the second step after a reset");
    w.reset(0, true);
    CHECK(w.step(0, false) == WINDOW, "a masked reset leaves the window claim standing");
  }
  {  // two envs on disjoint buffers do not disturb each other
    World w;
    w.create(0, T0, U0, O0, true);
    w.create(1, T1, U1, O1, true);
    w.step(0, false); w.step(1, false);
    for (int i = 0; i < 4; ++i) {
      CHECK(w.step(0, false) == (FLAGS | WINDOW), "env 0, round %d", i);
      CHECK(w.step(1, false) == (FLAGS | WINDOW), "env 1, round %d", i);
      w.reset(i & 1, false);
      w.rollout(i & 1, {}, {}, {}, false, true);
      w.step(i & 1, false);
    }
  }
  {  // after any withdrawal, one dense / full step re-establishes the claim
    World w;
    w.create(0, T0, U0, O0, true);
    w.create(1, T1, U1, O_OVER_0, false);  // (its classic observation buffer lies over env 0's sliding one)
    auto restored = [&](const char* after, unsigned lost) {
      CHECK((w.step(0, false) & lost) == 0, "%s: the next step is dense / full", after);
      CHECK(w.step(0, false) == (FLAGS | WINDOW), "%s: one step later both claims hold again", after);
    };
    w.step(0, false);
    w.set_schedule(0); restored("gte_set_schedule", FLAGS | WINDOW);
    w.rollout(0, O1, T2, U2, false, false); restored("gte_rollout with rows", FLAGS | WINDOW);
    w.rollout(0, {}, {}, {}, false, true); restored("gte_backtest", FLAGS);
    w.bind_returns(0, T0, U0); restored("gte_bind_returns", FLAGS);
    w.bind_sliding(0, O0); restored("gte_bind_sliding_obs", WINDOW);
    w.reset(0, false); restored("gte_reset", FLAGS);
    w.reset(0, true); restored("masked gte_reset", FLAGS);
    w.step(1, false); restored("another env's step into the observation buffer", WINDOW);
    w.reset(1, false); restored("another env's reset into the observation buffer", WINDOW);
    w.bind_outputs(0, O0, T0, U0);
    CHECK(w.step(0, false) == 0 && w.step(0, false) == FLAGS, "a classic buffer never slides");
  }
  {  // a backtest's own step launch: sparse flags (the fused kernels stored them densely), every window in full
    World w;
    w.create(0, T0, U0, O0, true);
    w.step(0, false); w.step(0, false);
    w.rollout(0, {}, {}, {}, false, true);
    CHECK(w.inner == FLAGS, "the step launch inside a backtest");
    CHECK(w.step(0, false) == WINDOW, "the step after it: dense flags, and it slides from the full write");
  }
  {  // an env sharing a flag buffer with another that steps in between never holds the flag claim
    World w;
    w.create(0, T0, U0, O0, true);
    w.create(1, T0, U0, O1, true);
    for (int i = 0; i < 6; ++i) {
      CHECK((w.step(0, false) & FLAGS) == 0, "env 0, round %d", i);
      CHECK((w.step(1, false) & FLAGS) == 0, "env 1, round %d", i);
    }
    w.create(2, FLAG_BUFS[6], T2, OBS_BUFS[3], false);  // (its terminated bytes overlap both of the others' buffers)
    for (int i = 0; i < 3; ++i) {
      w.step(0, false);
      CHECK((w.step(0, false) & FLAGS) != 0, "alone again");
      w.step(2, false);
      CHECK((w.step(0, false) & FLAGS) == 0, "a partial overlap counts");
    }
  }
  for (int slots : {2, 3}) {  // rotated return buffers never hold it: the pointers differ from the last step's
    World w;
    const Range T[3] = {T0, T1, T2}, U[3] = {U0, U1, U2};
    w.create(0, T[0], U[0], O0, true);
    for (int i = 0; i < 9; ++i) {
      w.bind_returns(0, T[i % slots], U[i % slots]);
      const unsigned got = w.step(0, false);
      CHECK((got & FLAGS) == 0, "%d slots, step %d", slots, i);
      CHECK(i == 0 || (got & WINDOW), "the window does not rotate");
    }
    // ... even without the rebind's withdrawal: a step into other buffers than the last one's is told no
    World v;
    v.create(0, T[0], U[0], O0, false);
    for (int i = 0; i < 9; ++i) {
      v.env[0].term = T[i % slots]; v.env[0].trunc = U[i % slots];
      CHECK(v.step(0, false) == 0, "%d slots unannounced, step %d", slots, i);
    }
  }
  {  // a range written by a captured step is never claimed again
    World w;
    w.create(0, T0, U0, O0, true);
    w.step(0, false);
    CHECK(w.step(0, false) == (FLAGS | WINDOW), "before the capture");
    CHECK(w.step(0, true) == 0 && w.step(0, true) == 0, "captured steps are dense and full");
    w.set_schedule(0);
    for (int i = 0; i < 4; ++i) CHECK(w.step(0, false) == 0, "eager step %d after the capture", i);
    // another env stepping into those buffers: no claim either
    w.create(1, T0, U0, O0, true);
    for (int i = 0; i < 3; ++i) CHECK(w.step(1, false) == 0, "another env, step %d", i);
    // the flag bytes stay out for good; the observation buffer comes back once the env that captured is gone
    w.destroy(0);
    w.step(1, false);
    CHECK(w.step(1, false) == WINDOW, "after the capturing env's destroy");
    // other buffers are as good as ever
    w.bind_returns(1, T1, U1);
    w.step(1, false);
    CHECK(w.step(1, false) == (FLAGS | WINDOW), "fresh flag buffers");
  }
}

// ---- threads --------------------------------------------------------------------------------------
void threads() {
  static int keys[4];
  std::vector<std::thread> pool;
  for (int t = 0; t < 4; ++t)
    pool.emplace_back([t] {
      Ledger& L = gte_ledger::ledger();
      const Span term = span(FLAG_BUFS[t]), trunc = span(FLAG_BUFS[t + 1]);  // each overlaps the next one's
      const Span obs = span(OBS_BUFS[t]);
      long held = 0;
      for (int i = 0; i < 20000; ++i) {
        held += L.holds(&keys[t], WINDOW, {obs}) + L.holds(&keys[t], FLAGS, {term, trunc});
        L.wrote(&keys[t], {obs, term, trunc}, false, FLAGS | WINDOW);
        L.establish(&keys[t], FLAGS, {term, trunc}, i % 997 == 0);
        L.establish(&keys[t], WINDOW, {obs}, false);
        if (i % 101 == 0) L.withdraw(&keys[t], FLAGS | WINDOW);
        if (i % 1009 == 0) L.forget(&keys[t]);
      }
      printf("thread %d: %ld claims held when asked\n", t, held);
    });
  for (std::thread& th : pool) th.join();
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "threads") {
    threads();
    printf("threads ok\n");
    return 0;
  }
  if (mode != "model") {
    fprintf(stderr, "usage: ledger_check model|threads\n");
    return 2;
  }
  scripted();
  printf("scripted ok\n");
  long asked[2] = {0, 0}, granted[2] = {0, 0};
  random_sequences(asked, granted);
  printf("flags granted %ld / asked %ld\n", granted[0], asked[0]);
  printf("window granted %ld / asked %ld\n", granted[1], asked[1]);
  printf("model ok\n");
  return 0;
}
