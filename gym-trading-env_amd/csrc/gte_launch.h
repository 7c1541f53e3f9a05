// gte_launch.h — the interface BETWEEN the translation units of libgte, stated once: the structs that
// cross a file boundary by value into kernel arguments, the limits the host's geometry search shares
// with the kernels, and the prototype of every host function one .hip file defines and another calls.
// gte_api.hip and every defining file include it, so a definition cannot disagree with what its
// callers see (tests/test_host_cpu.py: no second struct body, no prototype elsewhere, every
// definition declared here with the same signature).  Device-side code stays in gte_device.h.
#pragma once
#include "gte_device.h"

namespace gte {

// the limits the kernels share with the host's planner are defined there (gte_plan.h, with GTE_WAVES and GTE_LEAN_U)
using gte_plan::LEAN_MAX_ROWS;
using gte_plan::RES_LDS_MAX;
using gte_plan::RES_NEW;
using gte_plan::RES_OWNERS;
using gte_plan::ROLLOUT_WAVES;
// how many workgroups of the rollout kernels give every env a lane at epw envs per wavefront
inline int rollout_blocks(int n_envs, int epw) {
  return (int)((((int64_t)n_envs + epw - 1) / epw + ROLLOUT_WAVES - 1) / ROLLOUT_WAVES);
}
constexpr size_t LDS_OPT_IN = 64 * 1024;    // dynamic LDS beyond this is opted into, per instantiation

// 40-bit magic of the kernels' divisions by a launch constant (fastdiv40, gte_step.h)
inline uint64_t magic40(uint32_t d) { return ((1ull << 40) + d - 1) / d; }

// --- gte_kernels.hip (shared translation unit): every step / reset shape, helper kernels
hipError_t launch_step(const Params& p, int vec, int nt, bool coop, int stage, int blocks, int threads,
                       hipStream_t stream);
hipError_t launch_reset(const Params& p, int vec, int nt, bool coop, int stage, int blocks, int threads,
                        hipStream_t stream);
size_t lds_bytes(const Params& p, int stage);
// the same from the fields it depends on (the planner asks before any of the buffers exists)
size_t lds_image_bytes(int epw, int W, int nd, bool final_obs, bool log_row, int stage);
hipError_t launch_add_orders(const Params& p, const int32_t* pos_index, const double* limit,
                             const uint8_t* persistent, hipStream_t stream);
hipError_t launch_affinity_rebuild(const Params& p, int32_t* bins, int n_bins_per_ds, const int32_t* slot_of_rank,
                                   int32_t* perm_out, hipStream_t stream);
struct StateSoA {  // struct-of-arrays views of the state for the host (gte_get_state)
  int32_t *idx, *step, *pos, *dsi, *start, *episode, *needs_reset;
  double *asset, *fiat, *ia, *ifi, *pv, *realpos;
};
hipError_t launch_extract_state(const EnvRec* rec, int n, const StateSoA& o, hipStream_t stream);
hipError_t launch_rewind_queue(EnvRec* rec, int n, hipStream_t stream);

// --- gte_hot.hip / gte_hot_nt.hip: the headline instantiation alone, sc1 / non-temporal stores
hipError_t launch_step_hot(const Params& p, int blocks, int threads, size_t smem, hipStream_t stream);
hipError_t launch_step_hot_nt(const Params& p, int blocks, int threads, size_t smem, hipStream_t stream);
int hot_blocks_per_cu(size_t smem);
int hot_blocks_per_cu_nt(size_t smem);

// --- gte_rollout.hip: K steps in one launch
struct RolloutArgs {
  const int32_t* actions;  // [K][N]
  int32_t K;
  float* obs;              // [K][N][W][Fobs] or nullptr (last step only, into p.obs)
  float* reward;           // [K][N] or nullptr (p.reward, overwritten every step)
  double* reward64;
  uint8_t *terminated, *truncated;
  double* valuation;       // [K][N] or nullptr
  int32_t epb;             // resident kernel: envs per workgroup
  int32_t n_groups;        // resident kernel: ceil(N / epb) groups of envs, handed out through ...
  int32_t* group_counter;  // ... this device counter (zeroed before the launch)
};
size_t resident_lds_bytes(const Params& p, int epb);
int resident_blocks_per_cu(const Params& p, int epb, int nt);
hipError_t launch_rollout_resident(const Params& p, const RolloutArgs& r, int nt, int blocks, hipStream_t stream);
hipError_t launch_rollout_state(const Params& p, const RolloutArgs& r, int n_steps, int epw, hipStream_t stream);
int rollout_blocks_per_cu(const Params& p, int nt);
hipError_t launch_rollout(const Params& p, const RolloutArgs& r, int nt, int blocks, hipStream_t stream);

// --- the backtest summaries (gte_backtest.hip, gte_exits.hip, gte_trades.hip, gte_periods.hip): K steps in one
// launch that keep per-env statistics instead of per-step rows
struct SignalTable {  // one dataset's signal table (gte_bind_signals): row s starts at base + s * stride
  const int8_t* base;  // null = none bound
  int64_t stride;      // bytes, a multiple of 16 and >= round_up(T, 16)
};
struct ExitRules {  // what a bind left: the caller's rules and map, the library's per-env state
  const gte_exit_rule* rules;  // device [n_rules]
  const int32_t* rule_of_env;  // device i32 [N], or null = strategy of the env % n_rules
  gte_exit_state* state;       // device [N]
  int32_t n_rules;
};
struct SummarySource {  // where a from-registers launch takes every step's action from
  const int32_t* actions;     // device i32 [K][N]; null: looked up in the signal tables, at the env's own row
  const SignalTable* tables;  // device array [p.D], all bound (gte_bind_signals)
  int32_t S;                  // strategies
  const int32_t* strategy;    // device i32 [N] or null = (env_id_base + e) % S
  const ExitRules* rules;     // exit rules decided next to the lookup (gte_bind_exit_rules), or null = none
};
struct PeriodRow {  // one dataset's period row (gte_bind_periods), library-owned
  const int8_t* base;  // null = none bound
  int32_t len;         // bytes: round_up(T, 16), the bytes past T hold -1
};
struct Periods {  // what the period kernels are given
  const PeriodRow* rows;      // device array [p.D], all bound
  gte_period_stats* records;  // device [N][B]
  int32_t B;                  // 1 .. GTE_MAX_PERIODS
};
// what every launcher below checks, written once
// a lookup needs tables and a strategy count
inline bool tables_usable(const SignalTable* tables, int S) { return tables && S >= 1; }
inline bool exit_rules_usable(const ExitRules& r) { return r.rules && r.n_rules >= 1 && r.state; }
// what the from-registers kernels do not do: trajectory rows (the step kernel writes them, gte_kernel); in
// same-step mode they need somewhere for the terminal records; epw envs per wavefront; and a source to read
inline bool summary_refused(const Params& p, const SummarySource& src, int epw) {
  return p.log.rows != nullptr || (p.autoreset == GTE_AUTORESET_SAME_STEP && p.final_rec == nullptr) || epw < 1 ||
         epw > 64 ||
         (!src.actions && (!tables_usable(src.tables, src.S) || (src.rules && !exit_rules_usable(*src.rules))));
}
// ONE step folded in from what an ordinary launch left needs the terminal records in same-step mode too
inline bool fold_refused(const Params& p) { return p.autoreset == GTE_AUTORESET_SAME_STEP && p.final_rec == nullptr; }

// --- gte_backtest.hip
// clear != 0: zero the records and anchor them at the envs' current state; else bring the
// bookkeeping fields up to date with the records (a gte_reset since the previous call)
hipError_t launch_backtest_begin(const Params& p, gte_backtest_stats* stats, int clear, hipStream_t stream);
// n_steps steps from registers (the geometry of launch_rollout_state) with src.actions, the [K][N] actions.
// p.final_rec must be set in same-step mode: the lane that wrote an env's terminal record reads the terminal
// valuation back
hipError_t launch_backtest_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats, int n_steps,
                                   int epw, hipStream_t stream);
// ... with every step's action looked up instead (src.actions null), at the env's own row; with src.rules the
// exits are decided as well (then through launch_exit_summary)
hipError_t launch_signal_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats, int n_steps,
                                 int epw, hipStream_t stream);
// ONE step into the records, from what an ordinary step launch left in p's buffers
hipError_t launch_backtest_fold(const Params& p, gte_backtest_stats* stats, hipStream_t stream);
// the action the tables give every env for its next step (tables: device array [p.D], all bound;
// S strategies; strategy: device i32 [N] or null = (env_id_base + e) % S) -> actions i32 [N]
hipError_t launch_signal_actions(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                                 int32_t* actions, hipStream_t stream);

// --- gte_exits.hip: the lookups with exit rules bound (gte_bind_exit_rules, include/gte.h)
// every state as a bind leaves it: the next decision sees a reset row
hipError_t launch_exit_init(gte_exit_state* state, int n, hipStream_t stream);
// launch_signal_actions that also brings the exit states up to date, decides the exits and keeps the memo
hipError_t launch_exit_actions(const Params& p, const SignalTable* tables, int S, const int32_t* strategy,
                               const ExitRules& rules, int32_t* actions, hipStream_t stream);
// launch_signal_summary's launch for a source with rules, the exit state of every env in registers next to its
// statistics: the kernel stays in this unit, so launch_signal_summary comes through here; not meant to be
// called from anywhere else
hipError_t launch_exit_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats, int n_steps,
                               int epw, hipStream_t stream);

// --- gte_trades.hip: the backtest launches above with the trade statistics (gte_track_trades, include/gte.h)
// kept as well: `trades` is the device array of the N trade records, next to `stats`
// launch_backtest_begin for both records
hipError_t launch_trade_begin(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades, int clear,
                              hipStream_t stream);
// launch_backtest_summary with the trade record in registers too, whatever the source
hipError_t launch_trade_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats,
                                gte_trade_stats* trades, int n_steps, int epw, hipStream_t stream);
// launch_backtest_fold for both records
hipError_t launch_trade_fold(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades,
                             hipStream_t stream);

// --- gte_trade_list.hip: the launches of gte_trades.hip with the trade list kept as well (gte_track_trade_list,
// include/gte.h), and the gather of gte_read_trade_list / gte_pack_trade_list
struct TradeList {  // what the list kernels are given, library-owned
  gte_trade* list;    // device [N][capacity], env-major
  int32_t* open_row;  // device i32 [N]: the row the open trade of every env was decided at
  int32_t capacity;   // 1 .. GTE_MAX_TRADE_LIST
};
// launch_trade_begin, and open_row where a record is cleared or takes a reset row
hipError_t launch_trade_list_begin(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades,
                                   const TradeList& tl, int clear, hipStream_t stream);
// launch_trade_summary whose closes write their record
hipError_t launch_trade_list_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats,
                                     gte_trade_stats* trades, const TradeList& tl, int n_steps, int epw,
                                     hipStream_t stream);
// launch_trade_fold whose closes write their record
hipError_t launch_trade_list_fold(const Params& p, gte_backtest_stats* stats, gte_trade_stats* trades,
                                  const TradeList& tl, hipStream_t stream);
// ids (device i32 [n_ids], or null = envs 0 .. n_ids-1) -> closed[j] (the env's `closed`; -1 for an id outside
// [0, n_envs)) and first[0 .. n_ids], the running sum of min(closed, capacity)
hipError_t launch_trade_list_scan(const gte_trade_stats* trades, const TradeList& tl, int n_envs, const int32_t* ids,
                                  int n_ids, int64_t* first, int32_t* closed, hipStream_t stream);
// ... and the valid records of request j to out[first[j] ..), those below max_out only
hipError_t launch_trade_list_pack(const TradeList& tl, int n_envs, const int32_t* ids, int n_ids, const int64_t* first,
                                  gte_trade* out, int64_t max_out, hipStream_t stream);

// --- gte_curves.hip: the backtest launches above that also write per-step rows (gte_backtest_curves, include/gte.h)
struct CurveCarry {  // the window of one env that is open between two launches of a call
  double reward, drawdown;  // its reward sum and drawdown maximum so far
  int32_t flags;            // ... and its GTE_CURVE_* bits
  int32_t reserved[3];      // -> two 16-byte pieces
};
struct Curves {  // what the curve kernels are given
  CurveCarry* carry;    // device [N], library-owned
  int32_t stride;       // steps per row, >= 1
  gte_curve_bufs bufs;  // the caller's columns [R][N], any of them null = not kept (last: DESIGN.md, "Curves")
};
// launch_backtest_summary / launch_signal_summary, whatever the source, with the rows of the windows that close
// inside the launch written and the window open at its end left in c.carry; the launch begins a call
hipError_t launch_curve_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats, const Curves& c,
                                int n_steps, int epw, hipStream_t stream);
// launch_backtest_fold for step k of a call of n_call steps: takes the open window from c.carry, writes the row
// where the step closes a window or is the call's last, else leaves the window in c.carry
hipError_t launch_curve_fold(const Params& p, gte_backtest_stats* stats, const Curves& c, int k, int n_call,
                             hipStream_t stream);

// --- gte_periods.hip: the backtest launches above with the period statistics (gte_track_periods, include/gte.h)
// launch_backtest_summary with the open period's record in registers, whatever the source
hipError_t launch_period_summary(const Params& p, const SummarySource& src, gte_backtest_stats* stats,
                                 const Periods& per, int n_steps, int epw, hipStream_t stream);
// launch_backtest_fold that also folds the step into records[e][b]
hipError_t launch_period_fold(const Params& p, gte_backtest_stats* stats, const Periods& per, hipStream_t stream);

// --- gte_signals.hip: signal tables written on the device from indicator rules (gte_build_signals,
// include/gte.h): table rows 0 .. n_rules-1, bytes 0 .. round_up(T, 16)-1 of each; the caller has checked
// alignments and strides
hipError_t launch_build_signals(const float* indicators, int n_indicators, int64_t ind_stride,
                                const gte_signal_rule* rules, int n_rules, int64_t T, int8_t* table,
                                int64_t row_stride, hipStream_t stream);

// --- gte_compose.hip: signal tables composed on the device from clause rows and a truth table per strategy
// (gte_compose_signals, include/gte.h): table rows 0 .. n_specs-1, bytes 0 .. round_up(T, 16)-1 of each;
// the caller has checked alignments, strides and that the clause table and the output are disjoint
hipError_t launch_compose_signals(const int8_t* clauses, int n_clause_rows, int64_t clause_stride,
                                  const gte_signal_compose* specs, int n_specs, int64_t T, int8_t* table,
                                  int64_t row_stride, hipStream_t stream);

// --- gte_indicators.hip: indicator banks written on the device from resident market data
// (gte_build_indicators, include/gte.h): bank rows 0 .. n_specs-1, floats 0 .. round_up(T, 16)-1 of each;
// the caller has checked alignments, strides and that input and bank are disjoint
hipError_t launch_build_indicators(const DatasetDesc& ds, int Fobs, int n_static, const gte_indicator_spec* specs,
                                   int n_specs, const float* input, int n_inputs, int64_t input_stride, float* bank,
                                   int64_t ind_stride, hipStream_t stream);

// --- gte_strategy.hip: strategy records from env records, and their ranking (gte_reduce_backtest_stats,
// gte_rank_strategies, include/gte.h); the caller has checked alignments and that the group pointers are
// both null (the default map over env_id_base) or both set
hipError_t launch_reduce_strategies(const gte_backtest_stats* records, int n_envs, int n_strategies,
                                    int64_t env_id_base, const int32_t* group_offsets, const int32_t* group_envs,
                                    gte_strategy_stats* out, hipStream_t stream);
// entries (a score and an index each) of candidate list `which` (0, 1) that ranking S strategies needs
int64_t rank_scratch_entries(int n_strategies, int which);
hipError_t launch_rank_strategies(const gte_strategy_stats* stats, int n_strategies, int metric, int64_t min_episodes,
                                  int k, int32_t* top_index, double* top_score, double* scores, double* const* cand_score,
                                  int32_t* const* cand_index, hipStream_t stream);
// its selection launches alone: the k best of the S candidates a score kernel left in list 0
hipError_t launch_rank_select(int n_strategies, int k, int32_t* top_index, double* top_score, double* const* cand_score,
                              int32_t* const* cand_index, hipStream_t stream);

// --- gte_trade_strategy.hip: the same for trade records (gte_reduce_trade_stats, gte_rank_trade_stats,
// include/gte.h); the caller has checked what it checks for the two launches above
hipError_t launch_reduce_trade_stats(const gte_trade_stats* records, int n_envs, int n_strategies, int64_t env_id_base,
                                     const int32_t* group_offsets, const int32_t* group_envs,
                                     gte_strategy_trade_stats* out, hipStream_t stream);
// the score kernel alone: candidate list 0 (cand_score, cand_index: S entries), launch_rank_select follows
hipError_t launch_trade_scores(const gte_strategy_trade_stats* stats, int n_strategies, int metric, int64_t min_trades,
                               double* scores, double* cand_score, int32_t* cand_index, hipStream_t stream);

// --- gte_period_strategy.hip: the same for period records (gte_reduce_period_stats, gte_rank_period_stats,
// include/gte.h): records [n_envs][n_periods] -> out [n_strategies][n_periods]
hipError_t launch_reduce_period_stats(const gte_period_stats* records, int n_envs, int n_periods, int n_strategies,
                                      int64_t env_id_base, const int32_t* group_offsets, const int32_t* group_envs,
                                      gte_strategy_period_stats* out, hipStream_t stream);
// the score kernel alone (period_mask: host, two words): candidate list 0, launch_rank_select follows
hipError_t launch_period_scores(const gte_strategy_period_stats* stats, int n_strategies, int n_periods,
                                const uint64_t period_mask[2], int metric, int64_t min_steps, double* scores,
                                double* cand_score, int32_t* cand_index, hipStream_t stream);

// --- the three leaderboard analyses below (gte_bootstrap.hip, gte_cscv.hip, gte_diversify.hip) and the trade Monte
// Carlo (gte_montecarlo.hip) each carve their
// library-owned scratch out of one allocation with this: take<T>(count) is the next piece, every piece 256-byte
// aligned; `at` ends as the bytes the pieces need, which is all a carver over a null base is asked for
struct ScratchCarver {
  char* base;
  size_t at;
  template <typename T>
  T* take(size_t count) {
    T* piece = (T*)(base + at);
    at += (sizeof(T) * count + 255) & ~(size_t)255;
    return piece;
  }
};

// --- gte_bootstrap.hip: the bootstrap reality check (gte_bootstrap_weights, gte_reality_check, include/gte.h);
// the caller has checked alignments
// w[R][n] of the stationary bootstrap: thr and always (block == 1.0) as include/gte.h states them
hipError_t launch_bootstrap_weights(int n, int n_resamples, uint32_t thr, int always, uint64_t seed, double* weights,
                                    hipStream_t stream);
// bytes of library-owned scratch one reality check of S strategies, n selected periods and R resamples needs
size_t reality_check_scratch_bytes(int n_strategies, int n, int n_resamples);
// gather, resample pass and close (period_mask: host, two words, n bits set, none at or above n_periods)
hipError_t launch_reality_check(const gte_strategy_period_stats* stats, int n_strategies, int n_periods,
                                const uint64_t period_mask[2], int n, const double* benchmark, const double* weights,
                                int n_resamples, const gte_reality_check_out& out, void* scratch,
                                hipStream_t stream);

// --- gte_spa.hip: the test for superior predictive ability and its step-down (gte_spa_test, include/gte.h); the
// caller has checked alignments, and launch_reality_check has been enqueued into `rc` on the same stream
// bytes of library-owned scratch one test of S strategies, n selected periods and R resamples needs
size_t spa_scratch_bytes(int n_strategies, int n, int n_resamples);
// prepare, round 0 with its three recentrings and max_rounds - 1 further rounds that return at once when the
// step-down has stopped (period_mask: host, two words, n bits set, none at or above n_periods)
hipError_t launch_spa(const gte_strategy_period_stats* stats, int n_strategies, int n_periods,
                      const uint64_t period_mask[2], int n, const double* benchmark, const double* weights,
                      int n_resamples, double threshold, int crit_rank, int max_rounds,
                      const gte_reality_check_out& rc, const gte_spa_out& out, void* scratch, hipStream_t stream);

// --- gte_cscv.hip: the probability of backtest overfitting (gte_cscv, include/gte.h); the caller has checked
// alignments and the three tables
// bytes of library-owned scratch one call with S strategies, G groups and C splits needs
size_t cscv_scratch_bytes(int n_strategies, int n_groups, int n_splits);
// bytes of the packed host tables: group_masks (G * 2 words), then is_groups (C words), then oos_groups (C words)
size_t cscv_table_bytes(int n_groups, int n_splits);
// the copy of the packed tables (host, read before this returns) and the six launches
hipError_t launch_cscv(const gte_strategy_period_stats* stats, int n_strategies, int n_periods, const void* tables,
                       int n_groups, int n_splits, int metric, const gte_cscv_out& out, void* scratch,
                       hipStream_t stream);

// --- gte_diversify.hip: the decorrelated leaderboard (gte_diversify, include/gte.h); the caller has checked
// alignments and the mask
// bytes of library-owned scratch one call with S strategies, n selected periods and k rounds needs
size_t diversify_scratch_bytes(int n_strategies, int n, int k);
// prepare, k rounds and close (period_mask: host, two words, n bits set, none at or above n_periods)
hipError_t launch_diversify(const gte_strategy_period_stats* stats, int n_strategies, int n_periods,
                            const uint64_t period_mask[2], int n, const double* scores, double max_corr, int k,
                            const gte_diversify_out& out, void* scratch, hipStream_t stream);

// --- gte_montecarlo.hip: the trade Monte Carlo (gte_pool_trades, gte_trade_monte_carlo, include/gte.h); the caller
// has checked alignments and that the group pointers are both null or both set
// strategies (device i32 [n_pools]) -> first[0 .. n_pools], the running sum of the pools' sizes, and truncated[q]
hipError_t launch_pool_count(const gte_trade_stats* trades, const TradeList& tl, int n_envs, int n_strategies,
                             int64_t env_id_base, const int32_t* group_offsets, const int32_t* group_envs,
                             const int32_t* strategies, int n_pools, int64_t* first, int32_t* truncated,
                             hipStream_t stream);
// ... and the factors of request q to factors[first[q] ..), those below max_factors only
hipError_t launch_pool_pack(const gte_trade_stats* trades, const TradeList& tl, int n_envs, int n_strategies,
                            int64_t env_id_base, const int32_t* group_offsets, const int32_t* group_envs,
                            const int32_t* strategies, int n_pools, const int64_t* first, double* factors,
                            int64_t max_factors, hipStream_t stream);
// bytes of library-owned scratch one resampling of n_pools pools, R resamples and n_levels drawdown levels needs
size_t monte_carlo_scratch_bytes(int n_pools, int n_resamples, int n_levels);
// the walk and the close (dd_levels: host, read before this returns)
hipError_t launch_trade_monte_carlo(const double* factors, const int64_t* first, const uint32_t* streams, int n_pools,
                                    int n_resamples, int path_len, uint64_t seed, double ruin_level,
                                    const double* dd_levels, int n_levels, const gte_mc_out& out, void* scratch,
                                    hipStream_t stream);

// --- gte_aux.hip: trajectory log, values computed outside the step kernel, packed reads
hipError_t launch_log(const EnvRec* rec, const double* reward64, const uint8_t* term, const uint8_t* trunc, int n,
                      const int64_t* cursor, int L, const LogArrays& o, const uint8_t* mask, hipStream_t stream);
hipError_t launch_set_log_reward(LogRow* rows, const int64_t* last, int L, int n, const double* reward,
                                 hipStream_t stream);
hipError_t launch_set_dynamic(const Params& p, const float* values, uint32_t mask, hipStream_t stream);
hipError_t launch_set_dynamic_columns(const Params& p, const void* const* cols, const int32_t* is_f64,
                                      hipStream_t stream);
hipError_t launch_apply_reward(const Params& p, const double* reward, LogRow* rows, const int64_t* last,
                               int terminal_view, hipStream_t stream);
struct LogPack {  // where gte_pack_log_kernel puts the logged episode of each listed env
  int32_t* n_rows;                 // [n_ids]
  int32_t *idx, *step, *pos, *dsi; // [n_ids, max_rows], rows 0 .. n_rows-1 valid, oldest first
  double *pv, *realpos, *reward, *asset, *fiat, *ia, *ifi;
  uint8_t* flags;
};
hipError_t launch_pack_log(const LogArrays& log, int N, int L, long long rows_written, const int32_t* ids,
                           int n_ids, int max_rows, int finished, int frozen_runs, const EnvRec* final_rec,
                           const double* reward64, const LogPack& o, hipStream_t stream);
hipError_t launch_snapshot(const EnvRec* rec, const double* reward64, const uint8_t* term, const uint8_t* trunc,
                           const float* obs, int64_t obs_elems, int64_t obs_stride, int first, int count, void* dst,
                           float* dst_obs, hipStream_t stream);

// --- gte_comm.hip: RCCL, bound at run time
const char* rccl_load();
const char* rccl_error(int code);
int rccl_unique_id(uint8_t* out128);
int rccl_comm_init(void** comm, const uint8_t* id128, int rank, int world);
int rccl_allgather_bytes(void* comm, const void* src, void* dst, size_t bytes, hipStream_t stream);
int rccl_comm_destroy(void* comm);

}  // namespace gte
