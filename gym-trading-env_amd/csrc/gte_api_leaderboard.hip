// gte_api_leaderboard.hip — the leaderboard entry points of include/gte.h: the reduce / rank pair of each record
// family, the bootstrap weights, the analyses (reality check, SPA test, CSCV, diversify, trade pools and their Monte
// Carlo).
#include "gte_host.h"

extern "C" {

static int check_reduce_args(gte_env* E, const char* who, const void* records, const int32_t* group_offsets,
                             const int32_t* group_envs, const void* out) {
  if (!out || ((uintptr_t)out & 15)) return fail(GTE_ERR_INVALID, "out_device must be a 16-byte aligned device array");
  if ((uintptr_t)records & 15) return fail(GTE_ERR_INVALID, "records must be 16-byte aligned");
  if ((group_offsets == nullptr) != (group_envs == nullptr))
    return fail(GTE_ERR_INVALID, "group_offsets and group_envs: both or neither");
  if (((uintptr_t)group_offsets & 3) || ((uintptr_t)group_envs & 3))
    return fail(GTE_ERR_INVALID, "the group lists must be 4-byte aligned");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "%s inside a stream capture", who);
  return GTE_OK;
}

// metric in [lo, hi], the family's first and last
static int check_rank_args(gte_env* E, const char* who, int32_t k, int32_t metric, int lo, int hi, const void* stats,
                           const int32_t* top_index, const double* top_score, const double* scores) {
  if (k < 1 || k > GTE_RANK_MAX) return fail(GTE_ERR_INVALID, "k must lie in [1, %d]", GTE_RANK_MAX);
  if (metric < lo || metric > hi) return fail(GTE_ERR_INVALID, "metric %d unknown", metric);
  TRY(check_stats(stats));
  if (!top_index || ((uintptr_t)top_index & 3) || !top_score || ((uintptr_t)top_score & 7))
    return fail(GTE_ERR_INVALID, "top_index_device (int32 [k]) and top_score_device (f64 [k]) must be aligned device arrays");
  if ((uintptr_t)scores & 7) return fail(GTE_ERR_INVALID, "scores_device must be 8-byte aligned");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "%s inside a stream capture", who);
  return GTE_OK;
}

int gte_reduce_backtest_stats(gte_env* E, const gte_backtest_stats* records_device, int32_t n_strategies,
                              const int32_t* group_offsets_device, const int32_t* group_envs_device,
                              gte_strategy_stats* out_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_reduce_args(E, "gte_reduce_backtest_stats", records_device, group_offsets_device, group_envs_device,
                        out_device));
  const gte_backtest_stats* const records = records_device ? records_device : E->backtest.stats;
  if (!records) return fail(GTE_ERR_STATE, "gte_reduce_backtest_stats before gte_backtest: the env has no records yet");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_reduce_strategies(records, E->p.N, n_strategies, E->cfg.env_id_base,
                                                     group_offsets_device, group_envs_device, out_device, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "strategy reduction launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

// the two candidate lists of the selection launches, grown to what S strategies need (gte_strategy.hip)
static int rank_scratch(gte_env* E, int32_t n_strategies) {
  for (int w = 0; w < 2; ++w) {
    const int64_t need = gte::rank_scratch_entries(n_strategies, w);
    if (E->rank.entries[w] >= need) continue;
    const int64_t entries = need > 2 * E->rank.entries[w] ? need : 2 * E->rank.entries[w];
    TRY(dev_alloc(E, &E->rank.score[w], (size_t)entries, false));
    TRY(dev_alloc(E, &E->rank.index[w], (size_t)entries, false));
    E->rank.entries[w] = entries;
  }
  return GTE_OK;
}

// how gte_rank_trade_stats and gte_rank_period_stats end: their score kernel (e: its launch) has filled
// candidate list 0, the selection launches of gte_strategy.hip follow
static int rank_select(gte_env* E, hipError_t e, const char* what, int32_t n_strategies, int32_t k, int32_t* top_index,
                       double* top_score) {
  if (e == hipSuccess)
    e = gte::launch_rank_select(n_strategies, k, top_index, top_score, E->rank.score, E->rank.index, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "%s ranking launch: %s", what, hipGetErrorString(e));
  return GTE_OK;
}

int gte_rank_strategies(gte_env* E, const gte_strategy_stats* stats_device, int32_t n_strategies, int32_t metric,
                        int64_t min_episodes, int32_t k, int32_t* top_index_device, double* top_score_device,
                        double* scores_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_rank_args(E, "gte_rank_strategies", k, metric, GTE_METRIC_MEAN_REWARD, GTE_METRIC_WORST_REWARD_SUM,
                      stats_device, top_index_device, top_score_device, scores_device));
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(rank_scratch(E, n_strategies));
  const hipError_t e = gte::launch_rank_strategies(stats_device, n_strategies, metric, min_episodes, k,
                                                   top_index_device, top_score_device, scores_device, E->rank.score,
                                                   E->rank.index, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "strategy ranking launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_reduce_trade_stats(gte_env* E, const gte_trade_stats* records_device, int32_t n_strategies,
                           const int32_t* group_offsets_device, const int32_t* group_envs_device,
                           gte_strategy_trade_stats* out_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_reduce_args(E, "gte_reduce_trade_stats", records_device, group_offsets_device, group_envs_device,
                        out_device));
  const gte_trade_stats* const records = records_device ? records_device : E->trades.stats;
  if (!records) return fail(GTE_ERR_STATE, "gte_reduce_trade_stats before gte_track_trades: the env has no trade records yet");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_reduce_trade_stats(records, E->p.N, n_strategies, E->cfg.env_id_base,
                                                      group_offsets_device, group_envs_device, out_device, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "trade reduction launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_rank_trade_stats(gte_env* E, const gte_strategy_trade_stats* stats_device, int32_t n_strategies, int32_t metric,
                         int64_t min_trades, int32_t k, int32_t* top_index_device, double* top_score_device,
                         double* scores_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_rank_args(E, "gte_rank_trade_stats", k, metric, GTE_TRADE_METRIC_WIN_RATE,
                      GTE_TRADE_METRIC_NEG_MAX_LOSS_STREAK, stats_device, top_index_device, top_score_device,
                      scores_device));
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(rank_scratch(E, n_strategies));
  const hipError_t e = gte::launch_trade_scores(stats_device, n_strategies, metric, min_trades, scores_device,
                                                E->rank.score[0], E->rank.index[0], E->stream);
  return rank_select(E, e, "trade", n_strategies, k, top_index_device, top_score_device);
}

int gte_reduce_period_stats(gte_env* E, const gte_period_stats* records_device, int32_t n_periods, int32_t n_strategies,
                            const int32_t* group_offsets_device, const int32_t* group_envs_device,
                            gte_strategy_period_stats* out_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  TRY(check_reduce_args(E, "gte_reduce_period_stats", records_device, group_offsets_device, group_envs_device,
                        out_device));
  if (!records_device && !E->periods.stats.get())
    return fail(GTE_ERR_STATE, "gte_reduce_period_stats before gte_track_periods: the env has no period records yet");
  if (!records_device && n_periods != E->periods.alloc_B)
    return fail(GTE_ERR_INVALID, "n_periods %d: the env's records have %d", n_periods, E->periods.alloc_B);
  const gte_period_stats* const records = records_device ? records_device : E->periods.stats.as<gte_period_stats>();
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_reduce_period_stats(records, E->p.N, n_periods, n_strategies, E->cfg.env_id_base,
                                                       group_offsets_device, group_envs_device, out_device, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "period reduction launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_rank_period_stats(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                          int32_t n_periods, const uint64_t period_mask[2], int32_t metric, int64_t min_steps, int32_t k,
                          int32_t* top_index_device, double* top_score_device, double* scores_device) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  TRY(check_period_mask(period_mask));
  TRY(check_rank_args(E, "gte_rank_period_stats", k, metric, GTE_PERIOD_METRIC_MEAN_REWARD,
                      GTE_PERIOD_METRIC_POSITIVE_SHARE, stats_device, top_index_device, top_score_device,
                      scores_device));
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(rank_scratch(E, n_strategies));
  const hipError_t e = gte::launch_period_scores(stats_device, n_strategies, n_periods, period_mask, metric, min_steps,
                                                 scores_device, E->rank.score[0], E->rank.index[0], E->stream);
  return rank_select(E, e, "period", n_strategies, k, top_index_device, top_score_device);
}

int gte_bootstrap_weights(gte_env* E, int32_t n, int32_t n_resamples, double block, uint64_t seed,
                          double* weights_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (n < 2 || n > GTE_MAX_PERIODS) return fail(GTE_ERR_INVALID, "n %d outside [2, %d]", n, GTE_MAX_PERIODS);
  TRY(check_n_resamples(n_resamples));
  if (!(block >= 1.0)) return fail(GTE_ERR_INVALID, "block must be >= 1.0");
  if (!weights_device || ((uintptr_t)weights_device & 7))
    return fail(GTE_ERR_INVALID, "weights_device must be an 8-byte aligned device array");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bootstrap_weights inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  double t = floor(4294967296.0 / block);
  if (t > 4294967295.0) t = 4294967295.0;
  return launched(gte::launch_bootstrap_weights(n, n_resamples, (uint32_t)t, block == 1.0 ? 1 : 0, seed,
                                                weights_device, E->stream),
                  "bootstrap weights");
}

// what gte_reality_check and gte_spa_test check of the arguments they share, in this order; `out`: the reality
// check's outputs under the name `what` they have in the call; n: the selected periods
static int check_reality_check_args(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                                    int32_t n_periods, const uint64_t period_mask[2], const double* benchmark_device,
                                    const double* weights_device, int32_t n_resamples,
                                    const gte_reality_check_out* out, const char* what, int* n) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  TRY(check_n_resamples(n_resamples));
  TRY(check_period_mask(period_mask));
  TRY(count_periods(period_mask, n_periods, n));
  if (*n < 2) return fail(GTE_ERR_INVALID, "period_mask selects %d periods: at least two are needed", *n);
  TRY(check_stats(stats_device));
  if (!weights_device || ((uintptr_t)weights_device & 7) || ((uintptr_t)benchmark_device & 7))
    return fail(GTE_ERR_INVALID, "weights_device (required) and benchmark_device must be 8-byte aligned device arrays");
  if (!out) return fail(GTE_ERR_INVALID, "%s is NULL", what);
  if (!all_aligned({out->mean, out->boot_sum, out->boot_sq_sum, out->max_stat, out->summary}, 7))
    return fail(GTE_ERR_INVALID, "%s: mean, boot_sum, boot_sq_sum, max_stat and summary must be 8-byte aligned device pointers", what);
  if (!all_aligned({out->count_ge, out->count_adj, out->max_index}, 3))
    return fail(GTE_ERR_INVALID, "%s: count_ge, count_adj and max_index must be 4-byte aligned device pointers", what);
  return GTE_OK;
}

int gte_reality_check(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                      int32_t n_periods, const uint64_t period_mask[2], const double* benchmark_device,
                      const double* weights_device, int32_t n_resamples, const gte_reality_check_out* out) {
  int n;
  TRY(check_reality_check_args(E, stats_device, n_strategies, n_periods, period_mask, benchmark_device, weights_device,
                               n_resamples, out, "out", &n));
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_reality_check inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->rank.boot_scratch, gte::reality_check_scratch_bytes(n_strategies, n, n_resamples)));
  return launched(gte::launch_reality_check(stats_device, n_strategies, n_periods, period_mask, n, benchmark_device,
                                            weights_device, n_resamples, *out, E->rank.boot_scratch.base, E->stream),
                  "reality check");
}

int gte_spa_test(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies, int32_t n_periods,
                 const uint64_t period_mask[2], const double* benchmark_device, const double* weights_device,
                 int32_t n_resamples, double threshold, int32_t crit_rank, int32_t max_rounds,
                 const gte_reality_check_out* rc, const gte_spa_out* out) {
  int n;
  TRY(check_reality_check_args(E, stats_device, n_strategies, n_periods, period_mask, benchmark_device, weights_device,
                               n_resamples, rc, "rc", &n));
  if (!(threshold >= 0.0)) return fail(GTE_ERR_INVALID, "threshold must be >= 0.0 (+inf allowed), not NaN");
  if (crit_rank < 0 || crit_rank >= n_resamples)
    return fail(GTE_ERR_INVALID, "crit_rank %d outside [0, %d]", crit_rank, n_resamples - 1);
  if (max_rounds < 1 || max_rounds > GTE_SPA_MAX_ROUNDS)
    return fail(GTE_ERR_INVALID, "max_rounds %d outside [1, %d]", max_rounds, GTE_SPA_MAX_ROUNDS);
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  if (!all_aligned({out->t_stat, out->std_error, out->max_stat, out->crit, out->summary}, 7))
    return fail(GTE_ERR_INVALID, "out: t_stat, std_error, max_stat, crit and summary must be 8-byte aligned device pointers");
  if (!all_aligned({out->count_adj, out->rejected_round, out->max_index, out->round_rejected}, 3))
    return fail(GTE_ERR_INVALID, "out: count_adj, rejected_round, max_index and round_rejected must be 4-byte aligned device pointers");
  if (!out->recentred) return fail(GTE_ERR_INVALID, "out: recentred is NULL");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_spa_test inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->rank.boot_scratch, gte::reality_check_scratch_bytes(n_strategies, n, n_resamples)));
  TRY(grow(E, &E->rank.spa_scratch, gte::spa_scratch_bytes(n_strategies, n, n_resamples)));
  hipError_t e = gte::launch_reality_check(stats_device, n_strategies, n_periods, period_mask, n, benchmark_device,
                                           weights_device, n_resamples, *rc, E->rank.boot_scratch.base, E->stream);
  if (e == hipSuccess)
    e = gte::launch_spa(stats_device, n_strategies, n_periods, period_mask, n, benchmark_device, weights_device,
                        n_resamples, threshold, crit_rank, max_rounds, *rc, *out, E->rank.spa_scratch.base, E->stream);
  return launched(e, "SPA test");
}

int gte_cscv(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies, int32_t n_periods,
             const uint64_t* group_masks, int32_t n_groups, const uint32_t* is_groups, const uint32_t* oos_groups,
             int32_t n_splits, int32_t metric, const gte_cscv_out* out) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  if (n_groups < 2 || n_groups > GTE_CSCV_MAX_GROUPS)
    return fail(GTE_ERR_INVALID, "n_groups %d outside [2, %d]", n_groups, GTE_CSCV_MAX_GROUPS);
  if (n_splits < 1 || n_splits > GTE_CSCV_MAX_SPLITS)
    return fail(GTE_ERR_INVALID, "n_splits %d outside [1, %d]", n_splits, GTE_CSCV_MAX_SPLITS);
  if (metric != GTE_PERIOD_METRIC_MEAN_REWARD && metric != GTE_PERIOD_METRIC_SHARPE &&
      metric != GTE_PERIOD_METRIC_REWARD_SUM)
    return fail(GTE_ERR_INVALID, "metric %d: gte_cscv scores by MEAN_REWARD, SHARPE or REWARD_SUM", metric);
  TRY(check_stats(stats_device));
  if (!all_aligned({group_masks}, 7)) return fail(GTE_ERR_INVALID, "group_masks must be an 8-byte aligned host array");
  if (!all_aligned({is_groups, oos_groups}, 3))
    return fail(GTE_ERR_INVALID, "is_groups and oos_groups must be 4-byte aligned host arrays");
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  if (!all_aligned({out->is_score, out->oos_score}, 7) || !all_aligned({out->summary}, 3))
    return fail(GTE_ERR_INVALID, "out: is_score and oos_score must be 8-byte, summary 4-byte aligned device pointers");
  if (!all_aligned({out->best, out->below, out->equal, out->ranked}, 3))
    return fail(GTE_ERR_INVALID, "out: best, below, equal and ranked must be 4-byte aligned device pointers");
  uint64_t seen[2] = {0, 0};
  for (int g = 0; g < n_groups; ++g) {
    const uint64_t w0 = group_masks[2 * g], w1 = group_masks[2 * g + 1];
    if (!(w0 | w1)) return fail(GTE_ERR_INVALID, "group %d is empty", g);
    for (int b = n_periods; b < 128; ++b)
      if (((b < 64 ? w0 : w1) >> (b & 63)) & 1)
        return fail(GTE_ERR_INVALID, "group %d selects period %d, at or above n_periods %d", g, b, n_periods);
    if ((w0 & seen[0]) | (w1 & seen[1])) return fail(GTE_ERR_INVALID, "group %d shares a period with an earlier group", g);
    seen[0] |= w0;
    seen[1] |= w1;
  }
  const uint32_t all = n_groups == 32 ? 0xFFFFFFFFu : (1u << n_groups) - 1u;
  for (int c = 0; c < n_splits; ++c) {
    const uint32_t a = is_groups[c], b = oos_groups[c];
    if (!a || !b) return fail(GTE_ERR_INVALID, "split %d has an empty %s side", c, !a ? "in-sample" : "out-of-sample");
    if ((a | b) & ~all) return fail(GTE_ERR_INVALID, "split %d uses a group at or above n_groups %d", c, n_groups);
    if (a & b) return fail(GTE_ERR_INVALID, "split %d has a group on both sides", c);
  }
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_cscv inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->rank.cscv_scratch, gte::cscv_scratch_bytes(n_strategies, n_groups, n_splits)));
  // the three tables packed as gte_launch.h lays them out, so that one copy stages them
  std::vector<uint8_t> tables(gte::cscv_table_bytes(n_groups, n_splits));
  memcpy(tables.data(), group_masks, 16 * (size_t)n_groups);
  memcpy(tables.data() + 16 * (size_t)n_groups, is_groups, 4 * (size_t)n_splits);
  memcpy(tables.data() + 16 * (size_t)n_groups + 4 * (size_t)n_splits, oos_groups, 4 * (size_t)n_splits);
  return launched(gte::launch_cscv(stats_device, n_strategies, n_periods, tables.data(), n_groups, n_splits, metric,
                                   *out, E->rank.cscv_scratch.base, E->stream),
                  "cscv");
}

int gte_diversify(gte_env* E, const gte_strategy_period_stats* stats_device, int32_t n_strategies, int32_t n_periods,
                  const uint64_t period_mask[2], const double* scores_device, double max_corr, int32_t k,
                  const gte_diversify_out* out) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_periods(n_periods, 1));
  if (k < 1 || k > GTE_RANK_MAX) return fail(GTE_ERR_INVALID, "k must lie in [1, %d]", GTE_RANK_MAX);
  TRY(check_period_mask(period_mask));
  int n;
  TRY(count_periods(period_mask, n_periods, &n));
  if (n < 3) return fail(GTE_ERR_INVALID, "period_mask selects %d periods: a correlation needs at least three", n);
  if (max_corr != max_corr) return fail(GTE_ERR_INVALID, "max_corr is NaN");
  TRY(check_stats(stats_device));
  if (!all_aligned({scores_device}, 7)) return fail(GTE_ERR_INVALID, "scores_device must be an 8-byte aligned device array");
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  if (!all_aligned({out->pick_score, out->owner_corr, out->pick_corr}, 7))
    return fail(GTE_ERR_INVALID, "out: pick_score, owner_corr and pick_corr must be 8-byte aligned device pointers");
  if (!all_aligned({out->pick, out->cluster_size, out->owner, out->summary}, 3))
    return fail(GTE_ERR_INVALID, "out: pick, cluster_size, owner and summary must be 4-byte aligned device pointers");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_diversify inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->rank.div_scratch, gte::diversify_scratch_bytes(n_strategies, n, k)));
  return launched(gte::launch_diversify(stats_device, n_strategies, n_periods, period_mask, n, scores_device, max_corr,
                                        k, *out, E->rank.div_scratch.base, E->stream),
                  "diversify");
}

int gte_pool_trades(gte_env* E, int32_t n_strategies, const int32_t* group_offsets_device,
                    const int32_t* group_envs_device, const int32_t* strategies_device, int32_t n_pools,
                    int64_t* first_device, int32_t* truncated_device, double* factors_device, int64_t max_factors) {
  TRY(check_strategies(E, n_strategies));
  TRY(check_n_pools(n_pools));
  if ((group_offsets_device == nullptr) != (group_envs_device == nullptr))
    return fail(GTE_ERR_INVALID, "group_offsets and group_envs: both or neither");
  if (((uintptr_t)group_offsets_device & 3) || ((uintptr_t)group_envs_device & 3))
    return fail(GTE_ERR_INVALID, "the group lists must be 4-byte aligned");
  if (!all_aligned({strategies_device, truncated_device}, 3))
    return fail(GTE_ERR_INVALID, "strategies_device and truncated_device (int32 [n_pools]) must be 4-byte aligned device pointers");
  if (!all_aligned({first_device}, 7))
    return fail(GTE_ERR_INVALID, "first_device (int64 [n_pools + 1]) must be an 8-byte aligned device pointer");
  if (max_factors < 0 || (max_factors > 0 && !factors_device) || ((uintptr_t)factors_device & 7))
    return fail(GTE_ERR_INVALID, "factors_device (f64 [max_factors]) is NULL or not 8-byte aligned, or max_factors < 0");
  TRY(trade_list_on(E, "gte_pool_trades"));
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_pool_trades inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  const gte::TradeList tl = {E->trades.list.as<gte_trade>(), E->trades.open_row.as<int32_t>(), E->trades.cap};
  hipError_t le = gte::launch_pool_count(E->trades.stats, tl, E->p.N, n_strategies, E->cfg.env_id_base,
                                         group_offsets_device, group_envs_device, strategies_device, n_pools,
                                         first_device, truncated_device, E->stream);
  if (le == hipSuccess && max_factors > 0)
    le = gte::launch_pool_pack(E->trades.stats, tl, E->p.N, n_strategies, E->cfg.env_id_base, group_offsets_device,
                               group_envs_device, strategies_device, n_pools, first_device, factors_device,
                               max_factors, E->stream);
  return launched(le, "trade pool");
}

int gte_trade_monte_carlo(gte_env* E, const double* factors_device, const int64_t* first_device,
                          const uint32_t* stream_device, int32_t n_pools, int32_t n_resamples, int32_t path_len,
                          uint64_t seed, double ruin_level, const double* dd_levels, int32_t n_levels,
                          const gte_mc_out* out) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  TRY(check_n_pools(n_pools));
  if (n_resamples < 1 || n_resamples > GTE_MC_MAX_RESAMPLES)
    return fail(GTE_ERR_INVALID, "n_resamples %d outside [1, %d]", n_resamples, GTE_MC_MAX_RESAMPLES);
  if (path_len < 0 || path_len > GTE_MC_MAX_PATH)
    return fail(GTE_ERR_INVALID, "path_len %d outside [0, %d]", path_len, GTE_MC_MAX_PATH);
  if (n_levels < 0 || n_levels > GTE_MC_MAX_LEVELS)
    return fail(GTE_ERR_INVALID, "n_levels %d outside [0, %d]", n_levels, GTE_MC_MAX_LEVELS);
  if (ruin_level != ruin_level) return fail(GTE_ERR_INVALID, "ruin_level is NaN");
  if (!all_aligned({factors_device, first_device}, 7))
    return fail(GTE_ERR_INVALID, "factors_device (f64) and first_device (int64 [n_pools + 1]) must be 8-byte aligned device pointers");
  if ((uintptr_t)stream_device & 3) return fail(GTE_ERR_INVALID, "stream_device must be 4-byte aligned");
  if (n_levels > 0 && !all_aligned({dd_levels}, 7))
    return fail(GTE_ERR_INVALID, "dd_levels must be an 8-byte aligned host array of n_levels doubles");
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  if (!all_aligned({out->pool}, 15)) return fail(GTE_ERR_INVALID, "out: pool must be a 16-byte aligned device pointer");
  if (((uintptr_t)out->final & 7) || ((uintptr_t)out->max_drawdown & 7) || ((uintptr_t)out->low & 7) ||
      ((uintptr_t)out->max_loss_streak & 3))
    return fail(GTE_ERR_INVALID, "out: final, max_drawdown and low must be 8-byte, max_loss_streak 4-byte aligned device pointers");
  if (((uintptr_t)out->dd_count & 3) || (n_levels > 0 && !out->dd_count))
    return fail(GTE_ERR_INVALID, "out: dd_count (int32 [n_pools * n_levels]) must be a 4-byte aligned device pointer");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_trade_monte_carlo inside a stream capture");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(grow(E, &E->rank.mc_scratch, gte::monte_carlo_scratch_bytes(n_pools, n_resamples, n_levels)));
  return launched(gte::launch_trade_monte_carlo(factors_device, first_device, stream_device, n_pools, n_resamples,
                                                path_len, seed, ruin_level, dd_levels, n_levels, *out,
                                                E->rank.mc_scratch.base, E->stream),
                  "trade Monte Carlo");
}

}  // extern "C"
