// gte_plan.h — every launch choice of an env, decided from plain values.
//
// Plain C++17, host only: no HIP, no other file of csrc/ (tests/plan_check.cpp compiles it with g++, replays
// the plans recorded in tests/golden/launch_plans.json and checks what the rules guarantee over random shapes).
//
// The rules are functions of three things:
//   * Shape: integers and bools taken from gte_config (and what gte_create derives from it);
//   * Knobs: the environment switches as values.  This header calls getenv nowhere: gte_api.hip reads the
//     environment at the moments include/gte.h promises and hands the values in;
//   * Chip: the CU count and the five questions the rules put to the kernels' side (LDS image sizes, resident
//     workgroups per CU).  gte_api.hip answers them from the kernels and the HIP runtime; a test answers them
//     from a recording.
// gte_api.hip keeps the acts: it allocates what the plan asks for and launches.  It also owns what changes a
// plan at run time without a rule: a failed re-sort sets affinity_period to 0.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/gte.h"

// Wavefronts per workgroup of the step kernel (wave 0 runs phase A for the whole workgroup,
// every wave gathers its own p.epw envs).  4 is the product; other values are for A/B builds
// only (tools/waves_ab.sh): the rollout kernels assume 4.
#ifndef GTE_WAVES
#define GTE_WAVES 4
#endif
// lean copy loop (gte_step.h): the vectors in flight per lane (a wave copies whole passes of 64 * GTE_LEAN_U)
#ifndef GTE_LEAN_U
#define GTE_LEAN_U 4
#endif

namespace gte_plan {

// lean copy loop (gte_step.h): window rows of one wave's envs the in-place resolve holds in registers
constexpr int LEAN_MAX_ROWS = 512;
// rollout kernels (gte_rollout.hip): workgroups of four wavefronts, whatever GTE_WAVES is
constexpr int ROLLOUT_WAVES = 4;
// window-resident kernel: waves 1..3 (RES_OWNERS threads) carry the newest window rows of the workgroup's envs,
// at most RES_NEW vectors each; a geometry with more of them than RES_NEW * RES_OWNERS would drop some
constexpr int RES_NEW = 2;
constexpr int RES_OWNERS = 192;
constexpr size_t RES_LDS_MAX = 160 * 1024;  // LDS of a gfx950 CU: the most a workgroup's image may take

// GTE_SLIDE_AB (include/gte.h): what a set bit keeps as the sliding window's first version had it
enum { SLIDE_AB_ORDER = 1, SLIDE_AB_STORE = 2 };

// Which kernels an env launches, with what geometry: decided by plan_create (gte_create) and changed
// later only where noted.
struct LaunchPlan {
  int vec = 1, blocks = 0, threads = 256;
  bool coop = false;       // wave 0 of a workgroup runs phase A for the whole workgroup
  int stage = 0;           // dynamic columns: 0 global, 1 raw rings in LDS, 2 resolved in LDS
  int hot_per_cu = 0;      // resident workgroups per CU the geometry was sized for (0 = n/a)
  int store = 0;           // observation store policy (store_out): 0 plain, 1 nt, 2 sc1 (never 3)
  int slide_store = 0;     // the same for launches that store one row per env (p.slide); == store where none slide
  bool hot_tu = false;     // the step may go to the isolated hot instantiations (hot_tu_covers permitting)
  bool fused_log = false;  // the step kernel writes the trajectory row itself
  bool always_dense = false;     // every step stores all flags (gte_ledger.h)
  int slide_rows = 0;            // M: spare rows a sliding observation buffer may have (0 = this env never slides)
  bool full_windows = false;     // a sliding buffer moves its head but every step writes full windows (A/B)
  int slide_ab = 0;              // GTE_SLIDE_AB (include/gte.h): bits that keep the earlier slide launch (A/B)
  bool fused_rollout = false;    // gte_rollout may use the fused kernels ...
  bool resident_rollout = false; // ... and among them the window-resident one
  // L2-affinity processing order (gte_kernels.hip, "L2-affinity permutation")
  int affinity_period = 0;       // 0 = off (also set by affinity_after_upload and by a failed re-sort)
  int n_bins_per_ds = 0;
  int state_epw = 0;       // envs per wavefront of the from-registers kernels (state-only rollout, backtest)
  // rollout geometries, chosen by the first rollout that needs them
  int rollout_epw = 0;     // envs per wavefront of the fused rollout kernel (0 = not chosen yet)
  int resident_slots[3] = {0, 0, 0};  // workgroups of that geometry the chip holds at once
  int resident_epb[3] = {0, 0, 0};  // envs per workgroup of the window-resident rollout kernel per
                                    // store policy (0 = not chosen yet, -1 = shape not covered)
  // what the plan decides of Params (gte_device.h); gte_api.hip copies them there
  int epw = 0;        // environments per wavefront
  int lean_rows = 0;  // != 0: full waves of 16-byte-vector windows take the lean copy loop (gte_step.h)
  int hot_lds = 0;    // != 0: a step's record stores go through LDS, one 64-byte request per env (gte_kernel)
  int debug = 0;      // gte_config.debug_flags (timing ablations)
};

// What the rules read of an env: gte_config, and what gte_create derives from it (W = 1 without a window,
// Fobs = n_static + n_dyn).
struct Shape {
  int N = 0, D = 0, W = 1;
  bool has_window = false;
  int Fobs = 0, nd = 0;
  bool persist = false;    // dyn_persist
  int max_dur = 0;         // max_episode_duration
  bool final_obs = false;  // terminal observations are kept (the LDS image has a FinalJob per env then)
  int log_steps = 0;
  // the config's own knobs
  int envs_per_wave = 0, nontemporal_obs = 0, obs_slack_rows = 0, affinity_period = 0, kernel_variant = 0,
      debug_flags = 0;
};

// The environment switches (include/gte.h), as values.
struct Knobs {
  bool slide_full_windows = false;  // GTE_SLIDE_FULL_WINDOWS is set
  int slide_ab = 0;                 // GTE_SLIDE_AB
  int slide_store = -1;             // GTE_SLIDE_STORE = 0 | 1 | 2 (-1: unset, or not one of them)
  bool has_affinity_bins = false;   // GTE_AFFINITY_BINS is set ...
  int affinity_bins = 0;            // ... to this
  bool has_resident_epb = false;    // GTE_RESIDENT_EPB is set ...
  int resident_epb = 0;             // ... to this
  bool debug_geometry = false;      // GTE_DEBUG_GEOMETRY is set: the searches print their candidates
};

// The chip, as the rules see it.  The answers depend on the kernels' resource use, so they are asked, never
// computed here; a test substitutes recorded ones.
struct Chip {
  int n_cu = 0;
  // the step kernel's LDS image at epw envs per wavefront, dynamic columns staged as `stage` says.  Plan-time
  // value: the trajectory row a logging launch adds is NOT counted (the launch itself does count it)
  virtual size_t step_lds_bytes(int epw, int stage) = 0;
  // resident workgroups per CU of the isolated hot instantiation of store policy `store` (1 nt, else sc1)
  virtual int hot_per_cu(int store, size_t smem) = 0;
  // the window-resident rollout kernel: LDS image of epb envs per workgroup, workgroups per CU
  virtual size_t resident_lds_bytes(int epb) = 0;
  virtual int resident_per_cu(int epb, int store) = 0;
  // the gather-per-step rollout kernel: workgroups per CU at epw envs per wavefront
  virtual int gather_per_cu(int epw, int store) = 0;
  virtual ~Chip() = default;
};

// Step launch geometry: EPW environments per wavefront, 4 wavefronts per workgroup.  hot_ok: the
// config leaves the hot kernel's cooperative, LDS-staged shape on; lean_ok: the lean copy loop.
inline void step_geometry(LaunchPlan& L, const Shape& p, const Knobs& k, Chip& chip, bool hot_ok, bool lean_ok) {
  L.vec = (p.Fobs % 4 == 0) ? 4 : 1;
  const int64_t vpe = (int64_t)p.W * p.Fobs / L.vec;  // vectors per env
  int epw = p.envs_per_wave;
  if (epw == 0) {
    // windows of at least one wave instruction: 16 envs per wave (64 per workgroup, cooperative
    // phase A) measured best at every size tried; tiny windows may pack up to 64 per wave
    epw = (vpe >= 64) ? 16 : 64;
    // enough wavefronts to fill 256 CUs x 16 waves ...
    while (epw > 1 && ((int64_t)p.N + epw - 1) / epw < 4096) epw >>= 1;
    // ... but at least one full wave instruction (64 vectors) of copy work per wavefront
    // (small windows are latency-bound: 16 envs/wave with cooperative phase A measured
    // 5.4 us vs 7.5 us at 64 envs/wave on config 2, profiles/r01_tune_c2.log)
    while (epw < 64 && (int64_t)epw * vpe < 64) epw <<= 1;
    // Windowed shapes on the hot kernel.  Two regimes, both measured:
    //  * every workgroup resident at once, at least 16 waves on every CU: the launch ends when the
    //    BUSIEST CU is done (workgroups are dealt evenly: ceil(wgs / CUs) per CU), so take the
    //    envs-per-wave with the fewest envs on that CU; ties go to the bigger workgroup (fewer
    //    phase-A waves).  Config 3, us per step by envs on the busiest CU: 256 (16 per wave) 39.5,
    //    260 (13) 40.4, 264 (11) 40.5, 280 (14) 40.7, 288 (12) 42.0, 300 (15) 42.0; config 5:
    //    128 (8 per wave, 4 workgroups per CU) 36.3, 16 per wave on 2 per CU 43.5
    //    (profiles/r02_tune_epw.log, r02_waves_ab.log, r02_c5_sweep.log).
    //  * more workgroups than the chip holds (the observations stream to HBM): small workgroups —
    //    the phase A of those that start later hides behind the copies of those already running
    //    and the tail is one small workgroup.  Config 3 (profiles/r02_tune_epw_repeat.log, 3 passes
    //    each): 262 144 envs 16 per wave 156.4, 12: 154.7, 8: 149.2, 6: 143.8, 4: 142.6, 3: 145.5,
    //    2: 169.0; 131 072 envs 16: 86.7, 11: 83.3, 8: 80.1, 6: 79.0, 4: 78.2, 3: 79.8; 100 003 envs
    //    16: 74.5, 9: 62.1, 6: 60.0, 4: 61.6 -> about 640 vectors of copy work per wave (4 envs
    //    of 20x32), 960 below 120 000 envs.
    const bool residency_shape = L.vec == 4 && vpe >= 64 && p.nd > 0 && !p.persist && !p.final_obs &&
                                 (L.store == 1 || L.store == 2) && hot_ok;
    if (residency_shape) {
      const int64_t n_cu = chip.n_cu;
      int some_per_cu = 0;  // (residency of any candidate: the occupancy queries work)
      int64_t fewest = 0;
      int one_round_epw = 0, one_round_per_cu = 0;
      for (int e = 64 / GTE_WAVES; e >= 1; --e) {
        if ((int64_t)e * vpe < 64) break;
        // registers AND the workgroup's LDS (which shrinks with e) bound residency
        const size_t smem = chip.step_lds_bytes(e, 1);
        const int per_cu = chip.hot_per_cu(L.store, smem);
        if (per_cu <= 0) break;
        if (e <= 8 || !some_per_cu) some_per_cu = per_cu;
        const int64_t wgs = ((int64_t)p.N + GTE_WAVES * e - 1) / (GTE_WAVES * e);
        const int64_t busiest = (wgs + n_cu - 1) / n_cu;  // workgroups on the busiest CU
        if (k.debug_geometry)
          fprintf(stderr, "[gte] envs/wave %2d: LDS %5zu B, %d workgroups/CU resident, %lld workgroups, "
                          "%lld on the busiest CU\n", e, smem, per_cu, (long long)wgs, (long long)busiest);
        if (busiest <= per_cu && busiest * GTE_WAVES >= 16 && (fewest == 0 || busiest * e < fewest)) {
          fewest = busiest * e;
          one_round_epw = e;
          one_round_per_cu = per_cu;
        }
      }
      if (one_round_epw) {
        epw = one_round_epw;
        L.hot_per_cu = one_round_per_cu;
      } else if (some_per_cu) {
        L.hot_per_cu = some_per_cu;
        const int64_t target = (int64_t)p.N >= 120000 ? 640 : 960;
        int e = (int)((target + vpe / 2) / vpe);
        e = e < 1 ? 1 : (e > 64 / GTE_WAVES ? 64 / GTE_WAVES : e);
        while (e < 64 / GTE_WAVES && (int64_t)e * vpe < 64) ++e;
        epw = e;
        // Round 3: where the lean copy loop applies (whole passes of 4 wave instructions per wave,
        // gte_step.h) it beats the small workgroups above — 262 144 envs: 4 per wave 149 us,
        // 8: 139.8, 16: 137.8; 131 072: 4: 80, 8: 74, 16: 71-78; 100 003: 6: 62, 8: 58.7, 16: 60-67
        // (profiles/r03_epw_hbm.log) — so take the smallest envs-per-wave the lean loop accepts, twice
        // that from 200 000 envs on.
        if (lean_ok) {
          int lean_e = 0;
          for (int c = 1; c <= 64 / GTE_WAVES; ++c)
            if (((int64_t)c * vpe) % (64 * GTE_LEAN_U) == 0 && (int64_t)c * p.W <= LEAN_MAX_ROWS) { lean_e = c; break; }
          if (lean_e) {
            int c = lean_e;
            while (c * 2 <= 64 / GTE_WAVES && (int64_t)c * vpe < 1280 && (int64_t)c * 2 * p.W <= LEAN_MAX_ROWS) c *= 2;
            if ((int64_t)p.N >= 200000 && c * 2 <= 64 / GTE_WAVES && (int64_t)c * 2 * p.W <= LEAN_MAX_ROWS) c *= 2;
            epw = c;
          }
        }
      }
    }
  }
  while (epw > 1 && (int64_t)epw * vpe > (1 << 20)) epw >>= 1;  // keeps the index math in range
  // the LDS-staged dynamic columns must fit comfortably: shrink the workgroup's envs
  while (epw > 1 && (int64_t)epw * GTE_WAVES * p.W * (p.nd ? p.nd : 1) * 4 > 32 * 1024) epw >>= 1;
  L.epw = epw;
  const int64_t waves = ((int64_t)p.N + epw - 1) / epw;
  L.threads = 64 * GTE_WAVES;
  L.blocks = (int)((waves + GTE_WAVES - 1) / GTE_WAVES);
}

// L2-affinity order: only worth it when every XCD gets several workgroups and the
// windows are big enough to be bandwidth-bound.  Sets affinity_period and n_bins_per_ds; the caller allocates
// the order's buffers (N slots, N ranks, 2 * D * n_bins_per_ds bins) where affinity_period > 0.
inline void plan_affinity(LaunchPlan& L, const Shape& p, const Knobs& k) {
  // Default re-sort period: the order decays as envs jump to new start rows, i.e. with the
  // reset rate, about 1 / max_episode_duration of the envs per step once the episodes are out
  // of phase.  Measured at duration 500, episodes staggered (profiles/r02_tune_affinity_period.log):
  // every 128 steps 42.4 us per step, 64: 41.3, 32: 40.6, 16: 40.5, 8: 41.6 (a re-sort was four
  // small launches then, ~25 us) -> re-sort after ~6 % of the envs have moved; 128 when episodes
  // only end by the drawdown rule or at the end of the data.
  int auto_period = 128;
  if (p.max_dur > 0) {
    auto_period = p.max_dur / 16;
    auto_period = auto_period < 8 ? 8 : (auto_period > 128 ? 128 : auto_period);
  }
  const int period = p.affinity_period == 0 ? auto_period : p.affinity_period;
  const int EPB = L.epw * GTE_WAVES;
  const int n_wg = (p.N + EPB - 1) / EPB;
  if (!(period > 0 && n_wg >= 64 && (int64_t)p.W * p.Fobs * 4 >= 512)) return;
  int nb = 8192 / p.D;
  if (k.has_affinity_bins) nb = k.affinity_bins / p.D;  // tuning: total bins of the counting sort
  nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
  L.n_bins_per_ds = nb;
  L.affinity_period = period;
}

// slots in XCD-major order: workgroup b runs on XCD b % 8 (round-robin dispatch).  Writes N entries.
inline void fill_slot_of_rank(const Shape& p, int epw, int32_t* slot_of_rank) {
  const int64_t EPB = (int64_t)epw * GTE_WAVES;
  const int64_t n_wg = (p.N + EPB - 1) / EPB;
  for (int x = 0; x < 8; ++x)
    for (int64_t b = x; b < n_wg; b += 8)
      for (int64_t sl = b * EPB; sl < (b + 1) * EPB && sl < p.N; ++sl) *slot_of_rank++ = (int32_t)sl;
}

// Store policy of the launches that store one row per env (LaunchPlan::slide_store; plan_create has the
// rule and its evidence next to L.store's).  Called once store, the geometry, hot_tu, slide_rows and slide_ab
// are set.
inline int slide_store_policy(const LaunchPlan& L, const Shape& p, const Knobs& k, Chip& chip) {
  // (full_windows: the head moves, but no launch ever stores one row per env)
  if (L.slide_rows == 0 || L.full_windows || (L.slide_ab & SLIDE_AB_STORE)) return L.store;
  int s = p.nontemporal_obs;  // the caller's explicit word governs both kinds of launch
  if (s == 3) s = ((size_t)p.N * (p.W + L.slide_rows) * p.Fobs * sizeof(float) > ((size_t)190 << 20)) ? 1 : L.store;
  // step_geometry sized the workgroups by the occupancy of store's instantiation: the other isolated
  // instantiation must hold them all at once too, or slides keep store's
  if (s != L.store && L.hot_tu && s != 0) {
    const size_t smem = chip.step_lds_bytes(L.epw, L.stage);
    const int per_cu = chip.hot_per_cu(s, smem);
    if (per_cu < (L.blocks + chip.n_cu - 1) / chip.n_cu) s = L.store;
  }
  // tuning / tests: force it, whatever the rule and the residency check said (include/gte.h)
  if (k.slide_store >= 0) s = k.slide_store;
  return s;
}

// Every launch choice of the env (LaunchPlan).  The only reader of kernel_variant, whose bits select
// reference structures for A/B timing and the tests' twins (GTE_KV_*, include/gte.h).
inline LaunchPlan plan_create(const Shape& p, const Knobs& k, Chip& chip) {
  LaunchPlan L;
  const int kv = p.kernel_variant;
  // observation store policy (gte_step.h, store_out): while the observation buffer fits
  // the 256 MB Infinity Cache next to the feature table, sc1 stores keep it there (65 536 envs,
  // 168 MB: 42.5 us vs 45.8 us with nt); beyond that the stores are a pure stream and
  // non-temporal ones win (81 920 envs, 210 MB: 48 us vs 58 us; 262 144 envs: 162 us vs 261 us;
  // profiles/r01_tune_store_policy.log).  That is the rule of every launch that writes full windows:
  // wraps, resets, full steps after a withdrawn claim, rollout rows, captured steps, envs that do not
  // slide.  At c3 the wrap alone, kernel trace: sc1 40.2 / 37.5 us, non-temporal 43.4 us (r06, r07).
  // Launches that store one row per env have a policy of their own, slide_store (slide_store_policy):
  // they are a latency chain far from any memory limit, and what counts is the SLAB the rows are
  // scattered over, N x (W + M) rows: non-temporal once it exceeds the same 190 MB.  c3 (235 MB slab),
  // us per step, three interleaved passes (profiles/r07_slide_store_ab.log): slides sc1 17.57-17.79,
  // non-temporal 16.26-16.48, plain 17.93; kernel trace of the slide launch 14.36 -> 12.72 us.  Below
  // the threshold they keep `store`: at the 117 MB slabs (32 768 envs) non-temporal slides gain 0.25 us
  // on c4 without its gather (12.41 vs 12.67) but nothing outside the spread of the passes on c5.
  L.store = p.nontemporal_obs;
  if (L.store == 3) L.store = ((size_t)p.N * p.W * p.Fobs * sizeof(float) > ((size_t)190 << 20)) ? 1 : 2;
  step_geometry(L, p, k, chip, !(kv & (GTE_KV_PER_WAVE_PHASE_A | GTE_KV_NO_LDS_STAGING)), !(kv & GTE_KV_GENERIC_COPY));
  L.debug = p.debug_flags;
  L.coop = (L.epw * GTE_WAVES <= 64) && !(kv & GTE_KV_PER_WAVE_PHASE_A);
  L.stage = (p.nd > 0 && chip.step_lds_bytes(L.epw, 1) <= 48 * 1024 && !(kv & GTE_KV_NO_LDS_STAGING)) ? (p.persist ? 2 : 1) : 0;
  // the lean copy loop (gte_step.h): 16-byte vectors with the raw rings staged in LDS (stage 1;
  // dyn_persist takes stage 2)
  L.lean_rows = (L.vec == 4 && L.stage == 1 && !(kv & GTE_KV_GENERIC_COPY)) ? 1 : 0;
  L.hot_lds = (kv & GTE_KV_RECORD_DIRECT) ? 0 : 1;  // (A/B: the stepping lane stores its record itself)
  // the shape the isolated hot instantiations (gte_hot.hip) and the fused rollouts are written for
  const bool hot_launch_shape = L.vec == 4 && L.coop && L.stage == 1;
  L.hot_tu = hot_launch_shape && !(kv & GTE_KV_SHARED_TU);  // (A/B: the shared-TU instantiation instead)
  // With a trajectory log the step kernel writes the row itself (shared-TU instantiation): the lane
  // that stepped the env puts its 80-byte record into LDS and the copy waves write it out, five
  // lanes per env.  At the config-3 shape, us per step: 38.5 against 43.2 with the separate
  // gte_log_kernel launch (and 37.5 without a log; profiles/r03_log_ab.log).  (Rounds 1-2 kept the
  // log as twelve [L, N] columns: twelve scattered stores per env from the stepping lane, which
  // beyond 16 384 envs lost to the separate launch.)
  // GTE_KV_LOG_SEPARATE keeps the separate launch (A/B); GTE_KV_LOG_FUSED is the default now.
  L.fused_log = p.log_steps > 0 && !(kv & GTE_KV_LOG_SEPARATE);
  L.always_dense = (kv & GTE_KV_DENSE_FLAGS) != 0;  // (A/B of the sparse flag stores)
  // Sliding observation buffer (gte.h, gte_bind_sliding_obs): where the hot instantiation's shape runs —
  // 16-byte vectors, windows of at least one wave instruction, cooperative phase A, raw rings in LDS —
  // and nothing hot_tu_covers() excludes or that needs whole windows elsewhere (terminal observations, a
  // trajectory log and with it Python callables, T-deep dynamic columns, no window at all).
  // Automatic M = 2 W / 5: a period of M + 1 steps has one full write, and the buffer is (W + M) / W =
  // 1.4 x the classic one (8 spare rows at W = 20).
  L.slide_rows = 0;
  if (hot_launch_shape && (int64_t)p.W * p.Fobs / 4 >= 64 && p.has_window && !p.persist && !p.final_obs &&
      p.log_steps == 0 && p.obs_slack_rows >= 0)
    L.slide_rows = p.obs_slack_rows > 0 ? p.obs_slack_rows : 2 * p.W / 5;
  // A/B: the head still moves, every step writes full windows (an environment variable like
  // GTE_AFFINITY_BINS, not a GTE_KV_* bit: results and layout are the sliding ones)
  L.full_windows = k.slide_full_windows;  // (read at gte_create, once per env)
  // A/B: bit 1 keeps slide launches in the L2-affinity order (read the same way; include/gte.h)
  L.slide_ab = k.slide_ab;
  L.slide_store = slide_store_policy(L, p, k, chip);
  L.fused_rollout = hot_launch_shape && !p.final_obs && p.log_steps == 0 && !(kv & GTE_KV_ROLLOUT_PER_STEP);
  L.resident_rollout = p.W >= 2 && !(kv & GTE_KV_ROLLOUT_GATHER);
  // envs per wavefront from registers: full waves once every SIMD has one (65 536 envs: 5.8 us per step
  // with 64, 6.0 with 32, 9.2 with 16 — throughput of the scattered record / ring stores);
  // small batches are a latency chain and two half-filled waves overlap better (4 096 envs:
  // 3.5 us with 32, 3.9 with 64) — profiles/r02_state_epw.log
  L.state_epw = (p.N >= 64 * 1024) ? 64 : 32;
  plan_affinity(L, p, k);
  return L;
}

// The L2-affinity order pays when each XCD's 4 MiB L2 can hold its 1/8 share of the feature
// tables (config 3: 12.8 MB).  Tables far beyond the 32 MiB of aggregate L2 (config 5: 1.6 GB
// per GPU, L2 hit rate 0.16 either way) only pay for the re-sorts and for scattered
// observation stores: 39.4 us per step with the order, 36.8 without
// (profiles/r02_c5_sweep.log).  Automatic (affinity_period = 0) turns it off there.
// table_bytes: the uploaded feature tables of all datasets together.
inline void affinity_after_upload(LaunchPlan& L, const Shape& p, uint64_t table_bytes) {
  if (L.affinity_period > 0 && p.affinity_period == 0 && table_bytes > ((uint64_t)64 << 20)) L.affinity_period = 0;
}

// Window-resident kernel (gte_rollout.hip): each env's W-1 older rows stay in LDS for the
// whole launch.  Geometry: E envs per workgroup such that (a) the newest rows fit the owner
// threads, (b) as many envs as possible are resident per CU and (c) the workgroups fill a
// whole number of rounds (each workgroup runs all K steps, so a part-filled last round costs
// a full one): minimise rounds x max(phase A chain, the CU's observation bytes per step).
inline void choose_resident_epb(LaunchPlan& L, const Shape& p, const Knobs& k, Chip& chip, int nt) {
  L.resident_epb[nt] = -1;
  const int64_t FV = p.Fobs / 4;
  if (!L.resident_rollout) return;
  const int n_cu = chip.n_cu;
  double best = 0.0;
  for (int e = 64; e >= 1; --e) {
    if (k.has_resident_epb && k.resident_epb != e) continue;  // tuning: envs per group, no search
    if ((int64_t)e * FV > RES_NEW * RES_OWNERS) continue;  // newest-row vectors the owner threads carry
    const size_t smem = chip.resident_lds_bytes(e);
    if (smem > RES_LDS_MAX) continue;
    const int per_cu = chip.resident_per_cu(e, nt);
    if (per_cu <= 0) continue;
    const int64_t slots = (int64_t)per_cu * n_cu;
    const int64_t wgs = ((int64_t)p.N + e - 1) / e;
    // the launch is a work queue over the groups: "rounds" is a real number, at least one
    const double rounds = wgs > slots ? (double)wgs / (double)slots : 1.0;
    const double live = (double)(wgs < slots ? (wgs + n_cu - 1) / n_cu : per_cu);  // workgroups sharing a CU
    const double us_bw = live * e * (double)p.W * p.Fobs * 4.0 / 22.0e3;  // ~5.6 TB/s over 256 CUs
    // a workgroup's barriers and its state wave's latency are hidden by the OTHER workgroups
    // of its CU: prefer four of them
    // (measured at config 3, profiles/r02_resident_epb.log: 4 per CU 27.7 us per step, 3: 28.9,
    // 2: 30.3, 1: 47.2)
    static const double kAlone[5] = {1.7, 1.7, 1.10, 1.05, 1.0};
    const double alone = kAlone[per_cu < 4 ? per_cu : 4];
    const double cost = rounds * (us_bw > 3.0 ? us_bw : 3.0) * alone;
    if (k.debug_geometry)
      fprintf(stderr, "[gte] resident rollout, %2d envs/workgroup: LDS %6zu B, %d workgroups/CU, "
                      "%lld groups, %.2f round(s), cost %.1f\n", e, smem, per_cu, (long long)wgs, rounds, cost);
    if (best == 0.0 || cost < best * 0.999) {
      best = cost;
      L.resident_epb[nt] = e;
      L.resident_slots[nt] = (int)slots;
    }
  }
}

// The gather-per-step rollout kernel is a long-running loop: a workgroup that is not
// resident from the start runs all K steps after the others have finished.  It needs more
// registers than the step kernel, so it gets its own workgroup size, the smallest that
// keeps every workgroup resident.
inline void choose_rollout_epw(LaunchPlan& L, const Shape& p, Chip& chip, int nt) {
  L.rollout_epw = L.epw;
  if (p.envs_per_wave != 0) return;
  for (int e = 1; e <= 16; ++e) {
    if ((int64_t)e * p.W * p.Fobs / 4 < 64) continue;
    const int per_cu = chip.gather_per_cu(e, nt);
    const int64_t wgs = ((int64_t)p.N + ROLLOUT_WAVES * e - 1) / (ROLLOUT_WAVES * e);
    if (per_cu > 0 && wgs <= (int64_t)per_cu * chip.n_cu) { L.rollout_epw = e; break; }
    if (e == 16) L.rollout_epw = 16;  // more envs than one round holds: biggest workgroups
  }
}

// GTE_DEBUG_GEOMETRY: the whole plan as one line of key=value pairs (`when`: create, finalize, resident, gather).
// tests/test_gpu_launch_plans.py and tools/record_launch_plans.py read it.
inline void print_plan(FILE* out, const char* when, const LaunchPlan& L) {
  fprintf(out, "[gte] plan: when=%s vec=%d blocks=%d threads=%d coop=%d stage=%d hot_per_cu=%d store=%d slide_store=%d "
          "hot_tu=%d fused_log=%d always_dense=%d slide_rows=%d full_windows=%d slide_ab=%d fused_rollout=%d "
          "resident_rollout=%d affinity_period=%d n_bins_per_ds=%d state_epw=%d rollout_epw=%d resident_slots=%d,%d,%d "
          "resident_epb=%d,%d,%d epw=%d lean_rows=%d hot_lds=%d debug=%d\n", when, L.vec, L.blocks, L.threads,
          (int)L.coop, L.stage, L.hot_per_cu, L.store, L.slide_store, (int)L.hot_tu, (int)L.fused_log, (int)L.always_dense,
          L.slide_rows, (int)L.full_windows, L.slide_ab, (int)L.fused_rollout, (int)L.resident_rollout, L.affinity_period,
          L.n_bins_per_ds, L.state_epw, L.rollout_epw, L.resident_slots[0], L.resident_slots[1], L.resident_slots[2],
          L.resident_epb[0], L.resident_epb[1], L.resident_epb[2], L.epw, L.lean_rows, L.hot_lds, L.debug);
}

}  // namespace gte_plan
