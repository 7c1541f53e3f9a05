// plan_check.cpp — csrc/gte_plan.h on the CPU (tests/test_plan_cpu.py builds this with g++ under ASan + UBSan).
//
//   plan_check replay tests/golden/launch_plans.json
//       every row of the fixture: a Chip that answers from the row's recording, in the recorded order, and aborts
//       on any other question; the plans after create, after the upload and after each lazy rollout choice equal
//       the recorded ones field for field, and every recorded question was asked.
//   plan_check model
//       a synthetic Chip over fixed-seed random shapes: what the rules guarantee, and nothing more.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <random>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "gte_plan.h"

using namespace gte_plan;

#define CHECK(cond, ...)                                          \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                               \
      fprintf(stderr, "\n");                                      \
      abort();                                                    \
    }                                                             \
  } while (0)

// --- the subset of JSON the fixture uses: objects, arrays, strings without escapes, integers
struct Json {
  enum Kind { INT, STR, ARR, OBJ } kind = INT;
  long long num = 0;
  std::string str;
  std::vector<Json> arr;
  std::vector<std::pair<std::string, Json>> obj;
  const Json& at(const char* key) const {
    for (const auto& kv : obj)
      if (kv.first == key) return kv.second;
    CHECK(false, "no key %s", key);
    return *this;
  }
  int i(const char* key) const { return (int)at(key).num; }
  bool has(const char* key) const {
    for (const auto& kv : obj)
      if (kv.first == key) return true;
    return false;
  }
};

// a row's Shape / Knobs hold what differs from the fixture's base
struct Over {
  const Json& row;
  const Json& base;
  int i(const char* key) const { return row.has(key) ? row.i(key) : base.i(key); }
};

struct Parser {
  const std::string& s;
  size_t p = 0;
  explicit Parser(const std::string& text) : s(text) {}
  void ws() { while (p < s.size() && strchr(" \n\r\t", s[p])) ++p; }
  char peek() { ws(); CHECK(p < s.size(), "unexpected end"); return s[p]; }
  void expect(char c) { CHECK(peek() == c, "expected %c at %zu, found %c", c, p, s[p]); ++p; }
  std::string string() {
    expect('"');
    const size_t e = s.find('"', p);
    CHECK(e != std::string::npos, "unterminated string");
    std::string out = s.substr(p, e - p);
    CHECK(out.find('\\') == std::string::npos, "escapes are not supported");
    p = e + 1;
    return out;
  }
  Json value() {
    Json j;
    const char c = peek();
    if (c == '{') {
      j.kind = Json::OBJ;
      ++p;
      if (peek() == '}') { ++p; return j; }
      for (;;) {
        std::string k = string();
        expect(':');
        j.obj.emplace_back(std::move(k), value());
        if (peek() == ',') { ++p; continue; }
        expect('}');
        return j;
      }
    }
    if (c == '[') {
      j.kind = Json::ARR;
      ++p;
      if (peek() == ']') { ++p; return j; }
      for (;;) {
        j.arr.push_back(value());
        if (peek() == ',') { ++p; continue; }
        expect(']');
        return j;
      }
    }
    if (c == '"') { j.kind = Json::STR; j.str = string(); return j; }
    size_t e = p;
    if (s[e] == '-') ++e;
    while (e < s.size() && s[e] >= '0' && s[e] <= '9') ++e;
    CHECK(e > p && s[e - 1] != '-', "expected an integer at %zu", p);
    j.num = atoll(s.substr(p, e - p).c_str());
    p = e;
    return j;
  }
};

// --- replay

// answers from one event's recording, strictly in order
struct ReplayChip final : Chip {
  const char* row;
  const std::vector<Json>* rec = nullptr;
  size_t next = 0;
  explicit ReplayChip(const char* name) : row(name) {}
  void begin(const Json& questions) {
    rec = &questions.arr;
    next = 0;
    if (!rec->empty()) n_cu = (int)answer("n_cu", {0});  // (the device the recording ran on was device 0)
  }
  void end() const { CHECK(next == rec->size(), "%s: %zu recorded questions, %zu asked", row, rec->size(), next); }
  long long answer(const char* what, std::initializer_list<long long> args) {
    CHECK(rec && next < rec->size(), "%s: question %s beyond the recording", row, what);
    const std::vector<Json>& q = (*rec)[next++].arr;
    CHECK(q.size() == args.size() + 2 && q[0].str == what, "%s: asked %s where %s was recorded", row, what,
          q[0].str.c_str());
    size_t k = 1;
    for (long long a : args) {
      CHECK(q[k].num == a, "%s: %s argument %zu is %lld, recorded %lld", row, what, k, a, q[k].num);
      ++k;
    }
    return q[k].num;
  }
  size_t step_lds_bytes(int epw, int stage) override { return (size_t)answer("step_lds_bytes", {epw, stage}); }
  int hot_per_cu(int store, size_t smem) override { return (int)answer("hot_per_cu", {store, (long long)smem}); }
  size_t resident_lds_bytes(int epb) override { return (size_t)answer("resident_lds_bytes", {epb}); }
  int resident_per_cu(int epb, int store) override { return (int)answer("resident_per_cu", {epb, store}); }
  int gather_per_cu(int epw, int store) override { return (int)answer("gather_per_cu", {epw, store}); }
};

static Shape shape_of(const Over& j) {
  Shape s;
  s.N = j.i("N"); s.D = j.i("D"); s.W = j.i("W"); s.has_window = j.i("has_window") != 0; s.Fobs = j.i("Fobs");
  s.nd = j.i("nd"); s.persist = j.i("persist") != 0; s.max_dur = j.i("max_dur"); s.final_obs = j.i("final_obs") != 0;
  s.log_steps = j.i("log_steps"); s.envs_per_wave = j.i("envs_per_wave"); s.nontemporal_obs = j.i("nontemporal_obs");
  s.obs_slack_rows = j.i("obs_slack_rows"); s.affinity_period = j.i("affinity_period");
  s.kernel_variant = j.i("kernel_variant"); s.debug_flags = j.i("debug_flags");
  return s;
}

static Knobs knobs_of(const Over& j) {
  Knobs k;
  k.slide_full_windows = j.i("slide_full_windows") != 0; k.slide_ab = j.i("slide_ab"); k.slide_store = j.i("slide_store");
  k.has_affinity_bins = j.i("has_affinity_bins") != 0; k.affinity_bins = j.i("affinity_bins");
  k.has_resident_epb = j.i("has_resident_epb") != 0; k.resident_epb = j.i("resident_epb");
  return k;
}

static void expect_plan(const char* row, const char* when, const LaunchPlan& L, const Json& want) {
  const std::pair<const char*, long long> got[] = {
      {"vec", L.vec}, {"blocks", L.blocks}, {"threads", L.threads}, {"coop", L.coop}, {"stage", L.stage},
      {"hot_per_cu", L.hot_per_cu}, {"store", L.store}, {"slide_store", L.slide_store}, {"hot_tu", L.hot_tu},
      {"fused_log", L.fused_log}, {"always_dense", L.always_dense}, {"slide_rows", L.slide_rows},
      {"full_windows", L.full_windows}, {"slide_ab", L.slide_ab}, {"fused_rollout", L.fused_rollout},
      {"resident_rollout", L.resident_rollout}, {"affinity_period", L.affinity_period},
      {"n_bins_per_ds", L.n_bins_per_ds}, {"state_epw", L.state_epw}, {"rollout_epw", L.rollout_epw}, {"epw", L.epw},
      {"lean_rows", L.lean_rows}, {"hot_lds", L.hot_lds}, {"debug", L.debug}};
  // every field of the recorded line is compared: the scalars above and the two arrays
  CHECK(want.obj.size() == sizeof got / sizeof got[0] + 2, "%s %s: %zu recorded fields", row, when, want.obj.size());
  for (const auto& g : got)
    CHECK(want.at(g.first).num == g.second, "%s %s: %s = %lld, recorded %lld", row, when, g.first, g.second,
          want.at(g.first).num);
  for (int k = 0; k < 3; ++k) {
    CHECK(want.at("resident_slots").arr[k].num == L.resident_slots[k], "%s %s: resident_slots[%d] = %d", row, when, k,
          L.resident_slots[k]);
    CHECK(want.at("resident_epb").arr[k].num == L.resident_epb[k], "%s %s: resident_epb[%d] = %d", row, when, k,
          L.resident_epb[k]);
  }
}

static int replay(const char* path) {
  std::ifstream in(path);
  CHECK(in.good(), "cannot open %s", path);
  std::stringstream text;
  text << in.rdbuf();
  const std::string s = text.str();
  Parser parser(s);
  const Json fixture = parser.value();
  const Json& rows = fixture.at("rows");
  const Json& base = fixture.at("base");
  size_t questions = 0;
  for (const Json& row : rows.arr) {
    const char* name = row.at("name").str.c_str();
    const Shape shape = shape_of(Over{row.at("shape"), base.at("shape")});
    const Knobs knobs = knobs_of(Over{row.at("knobs"), base.at("knobs")});
    ReplayChip chip(name);
    LaunchPlan L;
    bool created = false;
    for (const Json& ev : row.at("events").arr) {
      const std::string& when = ev.at("when").str;
      // (an event names its chip questions and its plan by index: each distinct one stands once)
      chip.begin(fixture.at("chips").arr.at((size_t)ev.i("chip")));
      CHECK(created == (when != "create"), "%s: event %s out of place", name, when.c_str());
      // gte_rollout's store policy of the rows it keeps: non-temporal where the caller left the policy automatic
      const int nt = (row.i("keep_obs") && shape.nontemporal_obs == 3) ? 1 : L.store;
      if (when == "create") {
        L = plan_create(shape, knobs, chip);
        created = true;
      } else if (when == "finalize") {
        affinity_after_upload(L, shape, (uint64_t)row.at("table_bytes").num);
      } else if (when == "resident") {
        choose_resident_epb(L, shape, knobs, chip, nt);
      } else if (when == "gather") {
        choose_rollout_epw(L, shape, chip, nt);
      } else {
        CHECK(false, "%s: unknown event %s", name, when.c_str());
      }
      chip.end();
      questions += chip.next;
      expect_plan(name, when.c_str(), L, fixture.at("plans").arr.at((size_t)ev.i("plan")));
    }
    CHECK(created, "%s: no create event", name);
    printf("replayed %s\n", name);
  }
  printf("replay ok: %zu rows, %zu questions\n", rows.arr.size(), questions);
  return 0;
}

// --- model

// A chip that could exist: LDS images as the kernels lay them out (the terms of the recorded answers: 100 bytes
// per env, 56 more with terminal observations, the staged rings; the resident kernel's window rows and about 48
// bytes per env), residency = what 160 KiB of LDS hold, capped by a register budget.
struct ModelChip final : Chip {
  Shape s;
  int hot_cap, nt_cap, resident_cap, gather_cap;
  size_t step_lds_bytes(int epw, int stage) override {
    const size_t EPB = (size_t)epw * GTE_WAVES;
    return EPB * (16 + 64 + 4 * GTE_MAX_DYN + 4) + (s.final_obs ? EPB * 56 : 0) +
           (stage ? EPB * (size_t)s.W * (size_t)(s.nd ? s.nd : 1) * 4 : 0);
  }
  static int fit(size_t smem, int cap) { return (int)std::min<size_t>(160 * 1024 / (smem ? smem : 1), (size_t)cap); }
  int hot_per_cu(int store, size_t smem) override { return fit(smem, store == 1 ? nt_cap : hot_cap); }
  size_t resident_lds_bytes(int epb) override {
    return (size_t)epb * 48 + 16 + (size_t)epb * (size_t)(s.W - 1) * (size_t)s.Fobs * 4;
  }
  int resident_per_cu(int epb, int) override { return fit(resident_lds_bytes(epb), resident_cap); }
  int gather_per_cu(int epw, int) override {
    return fit((size_t)epw * ROLLOUT_WAVES * (100 + (size_t)s.W * (size_t)(s.nd ? s.nd : 1) * 4), gather_cap);
  }
};

static int model() {
  std::mt19937_64 rng(20240607);
  auto pick = [&](long long lo, long long hi) { return (int)(lo + (long long)(rng() % (uint64_t)(hi - lo + 1))); };
  static const int kBits[] = {GTE_KV_PER_WAVE_PHASE_A, GTE_KV_NO_LDS_STAGING, GTE_KV_SHARED_TU, GTE_KV_ROLLOUT_PER_STEP,
                              GTE_KV_ROLLOUT_GATHER, GTE_KV_LOG_SEPARATE, GTE_KV_GENERIC_COPY, GTE_KV_RECORD_DIRECT,
                              GTE_KV_DENSE_FLAGS};
  int slid = 0, lean = 0, ordered = 0, resident = 0;
  const int kShapes = 4000;
  for (int it = 0; it < kShapes; ++it) {
    Shape s;
    // what validate() of gte_api.hip lets through: W * Fobs <= 2^18, W < 32768, Fobs <= 2048, n_dyn <= GTE_MAX_DYN
    const int scale = pick(0, 18);
    s.N = pick(1, (1ll << scale) + pick(0, 40000));
    s.D = pick(0, 3) ? 1 : pick(2, 200);
    s.has_window = pick(0, 7) != 0;
    s.W = !s.has_window ? 1 : (pick(0, 9) ? pick(1, 64) : pick(65, 4096));
    const int fmax = (int)std::min<long long>(2048, (1ll << 18) / s.W);
    s.Fobs = pick(0, 2) ? 4 * pick(1, std::max(1, std::min(fmax, 160) / 4)) : pick(1, fmax);
    s.nd = pick(0, std::min(s.Fobs, GTE_MAX_DYN));
    s.persist = pick(0, 9) == 0;
    s.max_dur = pick(0, 1) ? 0 : pick(2, 5000);
    s.final_obs = pick(0, 9) == 0;
    s.log_steps = pick(0, 7) ? 0 : pick(1, 256);
    s.envs_per_wave = pick(0, 2) ? 0 : pick(1, 64);
    s.nontemporal_obs = pick(0, 3);
    s.obs_slack_rows = pick(0, 3) ? 0 : pick(-1, 40);
    s.affinity_period = pick(0, 3) ? 0 : pick(-1, 64);
    s.kernel_variant = 0;
    for (int b : kBits)
      if (pick(0, 11) == 0) s.kernel_variant |= b;
    s.debug_flags = pick(0, 9) ? 0 : pick(1, 7);
    Knobs k;
    k.slide_full_windows = pick(0, 7) == 0;
    k.slide_ab = pick(0, 3) ? 0 : pick(1, 3);
    k.slide_store = pick(0, 3) ? -1 : pick(0, 2);
    k.has_affinity_bins = pick(0, 7) == 0;
    k.affinity_bins = pick(0, 100000);
    k.has_resident_epb = pick(0, 7) == 0;
    k.resident_epb = pick(1, 64);
    ModelChip chip;
    chip.s = s;
    chip.n_cu = pick(0, 3) ? 256 : pick(1, 304);
    chip.hot_cap = pick(1, 8); chip.nt_cap = pick(1, 8); chip.resident_cap = pick(0, 5); chip.gather_cap = pick(0, 4);

    LaunchPlan L = plan_create(s, k, chip);
    const long long vec_per_env = (long long)s.W * s.Fobs / L.vec;
    CHECK(L.threads == 256, "threads %d", L.threads);
    CHECK(L.epw >= 1 && L.epw <= 64, "epw %d", L.epw);
    const long long waves = ((long long)s.N + L.epw - 1) / L.epw;
    CHECK(L.blocks == (waves + 3) / 4, "blocks %d for %lld waves", L.blocks, waves);
    CHECK((long long)L.epw * vec_per_env <= (1 << 20), "epw %d x %lld vectors", L.epw, vec_per_env);
    CHECK(!L.coop || 4 * L.epw <= 64, "coop at epw %d", L.epw);
    if (L.slide_rows > 0)
      CHECK(L.vec == 4 && L.coop && L.stage == 1 && s.log_steps == 0 && !s.final_obs && !s.persist,
            "slide_rows %d off the hot shape", L.slide_rows);
    if (L.slide_rows == 0 || L.full_windows || (L.slide_ab & SLIDE_AB_STORE))
      CHECK(L.slide_store == L.store, "slide_store %d, store %d", L.slide_store, L.store);
    CHECK(!L.lean_rows || (L.vec == 4 && L.stage == 1), "lean_rows at vec %d stage %d", L.vec, L.stage);
    CHECK(L.store >= 0 && L.store <= 2 && L.slide_store >= 0 && L.slide_store <= 2, "store %d / %d", L.store, L.slide_store);
    // the order's slots: a permutation of 0 .. N-1, whether or not this plan keeps the order
    std::vector<int32_t> slots((size_t)s.N + 1, -7);
    fill_slot_of_rank(s, L.epw, slots.data());
    CHECK(slots[(size_t)s.N] == -7, "fill_slot_of_rank wrote past N entries");
    std::vector<char> seen((size_t)s.N, 0);
    for (int r = 0; r < s.N; ++r) {
      CHECK(slots[r] >= 0 && slots[r] < s.N && !seen[slots[r]], "slot_of_rank[%d] = %d", r, slots[r]);
      seen[slots[r]] = 1;
    }
    if (L.affinity_period > 0) CHECK(L.n_bins_per_ds >= 1 && L.n_bins_per_ds <= 4096, "bins %d", L.n_bins_per_ds);
    // after the upload, and the lazy rollout choices
    const int before = L.affinity_period;
    affinity_after_upload(L, s, (uint64_t)pick(0, 1) << 27);
    CHECK(L.affinity_period == before || (L.affinity_period == 0 && s.affinity_period == 0), "period %d -> %d", before,
          L.affinity_period);
    for (int nt = 0; nt < 3; ++nt) {
      choose_resident_epb(L, s, k, chip, nt);
      const int e = L.resident_epb[nt];
      CHECK(e == -1 || (e >= 1 && e <= 64), "resident_epb %d", e);
      if (e > 0) {
        CHECK(L.resident_rollout && (long long)e * (s.Fobs / 4) <= RES_NEW * RES_OWNERS &&
                  chip.resident_lds_bytes(e) <= RES_LDS_MAX && L.resident_slots[nt] > 0 &&
                  (!k.has_resident_epb || e == k.resident_epb), "resident geometry %d", e);
        ++resident;
      }
      choose_rollout_epw(L, s, chip, nt);
      CHECK(L.rollout_epw >= 1 && L.rollout_epw <= 64, "rollout_epw %d", L.rollout_epw);
    }
    slid += L.slide_rows > 0;
    lean += L.lean_rows != 0;
    ordered += before > 0;
  }
  // (no empty exercise)
  printf("shapes %d slid %d lean %d ordered %d resident %d\n", kShapes, slid, lean, ordered, resident);
  printf("model ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "replay")) return replay(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "model")) return model();
  fprintf(stderr, "usage: plan_check replay FIXTURE | plan_check model\n");
  return 2;
}
