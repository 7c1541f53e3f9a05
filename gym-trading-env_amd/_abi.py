"""ctypes mirror of include/gte.h and the loader of libgte.so.

The product path has no CPU fallback: :func:`load_library` raises when the HIP
library has not been built, and every device entry point of the library
returns GTE_ERR_NO_DEVICE on a host without a gfx950 GPU, which
:func:`check` turns into :class:`GteError`.
"""
from __future__ import annotations

import ctypes as C
import os

GTE_ABI_VERSION = 5
GTE_MAX_POSITIONS = 32
GTE_MAX_DYN = 4
GTE_COMM_ID_BYTES = 128

GTE_OK = 0
GTE_ERR_INVALID = -1
GTE_ERR_NO_DEVICE = -2
GTE_ERR_HIP = -3
GTE_ERR_STATE = -4
GTE_ERR_OOM = -5

DYN_LAST_POSITION = 0
DYN_REAL_POSITION = 1

REWARD_LOG_RETURN = 0
REWARD_SCALED_LOG_RETURN = 1
REWARD_CLIPPED_LOG_RETURN = 2

AUTORESET_DISABLED = 0
AUTORESET_NEXT_STEP = 1
AUTORESET_SAME_STEP = 2

# gte_config.kernel_variant bits (enum gte_kernel_variant): reference structures of the kernels
KV_PER_WAVE_PHASE_A = 1
KV_NO_LDS_STAGING = 2
KV_RETIRED_OVERLAPPED = 4
KV_SHARED_TU = 64
KV_ROLLOUT_PER_STEP = 128
KV_ROLLOUT_GATHER = 256
KV_LOG_SEPARATE = 1024
KV_LOG_FUSED = 2048
KV_GENERIC_COPY = 4096
KV_RECORD_DIRECT = 8192
KV_DENSE_FLAGS = 16384

# enum gte_strategy_metric: the score gte_rank_strategies orders strategies by
METRIC_MEAN_REWARD = 0
METRIC_SHARPE = 1
METRIC_MEAN_EPISODE_RETURN = 2
METRIC_EPISODE_SHARPE = 3
METRIC_NEG_MAX_DRAWDOWN = 4
METRIC_WORST_REWARD_SUM = 5
#: the same by name, in enum order (StrategyStats.score / .top take either)
STRATEGY_METRICS = ("mean_reward", "sharpe", "mean_episode_return", "episode_sharpe", "neg_max_drawdown",
                    "worst_reward_sum")
GTE_RANK_MAX = 256

# enum gte_trade_metric: the score gte_rank_trade_stats orders strategies by
TRADE_METRIC_WIN_RATE = 0
TRADE_METRIC_PROFIT_FACTOR = 1
TRADE_METRIC_EXPECTANCY = 2
TRADE_METRIC_TRADE_SHARPE = 3
TRADE_METRIC_WORST_TRADE = 4
TRADE_METRIC_NEG_MAX_LOSS_STREAK = 5
#: the same by name, in enum order (StrategyTradeStats.score / .top take either)
TRADE_METRICS = ("win_rate", "profit_factor", "expectancy", "trade_sharpe", "worst_trade", "neg_max_loss_streak")

# enum gte_period_metric: the score gte_rank_period_stats orders strategies by, over a set of periods
PERIOD_METRIC_MEAN_REWARD = 0
PERIOD_METRIC_SHARPE = 1
PERIOD_METRIC_REWARD_SUM = 2
PERIOD_METRIC_PERIOD_SHARPE = 3
PERIOD_METRIC_WORST_PERIOD = 4
PERIOD_METRIC_POSITIVE_SHARE = 5
#: the same by name, in enum order (StrategyPeriodStats.score / .top take either)
PERIOD_METRICS = ("mean_reward", "sharpe", "reward_sum", "period_sharpe", "worst_period", "positive_share")
GTE_MAX_PERIODS = 128
# gte_reality_check: resamples per slab of the moment sums, and the most resamples of one call
GTE_BOOT_SLAB = 256
GTE_BOOT_MAX_RESAMPLES = 65536
GTE_SPA_MAX_ROUNDS = 64
# gte_cscv: the most groups and splits of one call, and the splits a workgroup takes
GTE_CSCV_MAX_GROUPS = 32
GTE_CSCV_MAX_SPLITS = 65536
GTE_CSCV_CHUNK = 256
#: the period metrics gte_cscv scores by
CSCV_METRICS = ("mean_reward", "sharpe", "reward_sum")
# gte_trade_monte_carlo: resamples per slab of the sums, the most resamples, pools, path length and drawdown levels of
# one call, and the largest pool the walk stages into LDS
GTE_MC_SLAB = 256
GTE_MC_MAX_RESAMPLES = 65536
GTE_MC_MAX_POOLS = 65536
GTE_MC_MAX_PATH = 1 << 20
GTE_MC_MAX_LEVELS = 8
GTE_MC_LDS_POOL = 8192


class GteError(RuntimeError):
    """A libgte call failed (status code + the library's message)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"libgte error {status}: {message}")
        self.status = status


class GteConfig(C.Structure):
    """struct gte_config (include/gte.h)."""

    _fields_ = [
        ("abi_version", C.c_int32),
        ("struct_bytes", C.c_int32),
        ("device", C.c_int32),
        ("n_envs", C.c_int32),
        ("n_datasets", C.c_int32),
        ("n_static", C.c_int32),
        ("n_dyn", C.c_int32),
        ("dyn_kind", C.c_int32 * GTE_MAX_DYN),
        ("window", C.c_int32),
        ("n_positions", C.c_int32),
        ("positions", C.c_double * GTE_MAX_POSITIONS),
        ("trading_fees", C.c_double),
        ("borrow_interest_rate", C.c_double),
        ("portfolio_initial_value", C.c_double),
        ("initial_position_index", C.c_int32),
        ("max_episode_duration", C.c_int32),
        ("reward_kind", C.c_int32),
        ("autoreset", C.c_int32),
        ("reward_param0", C.c_double),
        ("reward_param1", C.c_double),
        ("reward_param2", C.c_double),
        ("episodes_between_dataset_switch", C.c_int32),
        ("dyn_persist", C.c_int32),
        ("seed", C.c_uint64),
        ("env_id_base", C.c_int64),
        ("envs_per_wave", C.c_int32),
        ("nontemporal_obs", C.c_int32),
        ("kernel_variant", C.c_int32),
        ("debug_flags", C.c_int32),
        ("affinity_period", C.c_int32),
        ("log_steps", C.c_int32),
        ("reserved2", C.c_int32),
        ("final_obs", C.c_int32),
        ("obs_slack_rows", C.c_int32),
    ]


class GteEnvSnapshot(C.Structure):
    """struct gte_env_snapshot (include/gte.h)."""
    _fields_ = [(n, C.c_int32) for n in ("idx", "step", "position_index", "dataset_index",
                                         "start_idx", "episode", "needs_reset", "terminated",
                                         "truncated", "reserved")] + \
               [(n, C.c_double) for n in ("asset", "fiat", "interest_asset", "interest_fiat",
                                          "portfolio_valuation", "real_position", "reward")]


# numpy view of an array of gte_env_snapshot (gte_read_envs)
SNAPSHOT_DTYPE = [(n, "<i4") for n in ("idx", "step", "position_index", "dataset_index",
                                       "start_idx", "episode", "needs_reset", "terminated",
                                       "truncated", "reserved")] + \
                 [(n, "<f8") for n in ("asset", "fiat", "interest_asset", "interest_fiat",
                                       "portfolio_valuation", "real_position", "reward")]


class GteRolloutBufs(C.Structure):
    """struct gte_rollout_bufs (include/gte.h): optional per-step result arrays."""
    _fields_ = [("obs", C.c_void_p), ("reward", C.c_void_p), ("reward64", C.c_void_p),
                ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("valuation", C.c_void_p)]


#: struct gte_curve_bufs (include/gte.h), in declaration order, with the torch dtype name of each column
CURVE_COLUMNS = [("valuation", "float64"), ("drawdown", "float64"), ("reward", "float64"),
                 ("position", "int32"), ("row", "int32"), ("flags", "uint8")]
#: the bits of the `flags` column (GTE_CURVE_*, include/gte.h)
CURVE_TERMINATED, CURVE_TRUNCATED, CURVE_RESET, CURVE_FROZEN = 1, 2, 4, 8


class GteCurveBufs(C.Structure):
    """struct gte_curve_bufs (include/gte.h): the optional [R][N] columns of gte_backtest_curves."""
    _fields_ = [(n, C.c_void_p) for n, _ in CURVE_COLUMNS]


#: struct gte_backtest_stats (include/gte.h), in declaration order: one 128-byte record per env
BACKTEST_FIELDS = [("steps", "<i8")] + \
    [(n, "<f8") for n in ("reward_sum", "reward_sq_sum", "peak", "max_drawdown", "cur_return",
                          "ep_return_sum", "ep_return_sq_sum", "valuation_last", "prev_position")] + \
    [(n, "<i4") for n in ("trades", "episodes", "terminations", "ended", "episode_seen", "step_seen")]
#: numpy view of an array of gte_backtest_stats (gte_read_backtest_stats)
BACKTEST_DTYPE = BACKTEST_FIELDS + [("reserved", "<i4", (6,))]


class GteBacktestStats(C.Structure):
    """struct gte_backtest_stats (include/gte.h)."""
    _fields_ = [(n, {"<i8": C.c_int64, "<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in BACKTEST_FIELDS] + \
               [("reserved", C.c_int32 * 6)]


#: struct gte_trade_stats (include/gte.h), in declaration order: one 128-byte record per env
TRADE_FIELDS = [(n, "<f8") for n in ("open_value", "open_position", "last_valuation", "gross_profit", "gross_loss",
                                     "ret_sq_sum", "best_trade", "worst_trade")] + \
    [(n, "<i8") for n in ("exposure", "hold_sum")] + \
    [(n, "<i4") for n in ("closed", "wins", "losses", "forced", "reversals", "dropped", "open_len", "max_len",
                          "loss_streak", "max_loss_streak")]
#: numpy view of an array of gte_trade_stats (gte_read_trade_stats)
TRADE_DTYPE = TRADE_FIELDS + [("reserved", "<i4", (2,))]


class GteTradeStats(C.Structure):
    """struct gte_trade_stats (include/gte.h)."""
    _fields_ = [(n, {"<i8": C.c_int64, "<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in TRADE_FIELDS] + \
               [("reserved", C.c_int32 * 2)]


#: struct gte_trade (include/gte.h), in declaration order: one 48-byte record per closed trade of the trade list
TRADE_LIST_FIELDS = [(n, "<f8") for n in ("open_value", "close_value", "position")] + \
    [(n, "<i4") for n in ("entry_row", "exit_row", "hold", "dataset", "kind", "flags")]
#: numpy view of an array of gte_trade (gte_read_trade_list)
TRADE_LIST_DTYPE = TRADE_LIST_FIELDS
#: gte_trade.kind
TRADE_KIND_FLAT, TRADE_KIND_REVERSAL, TRADE_KIND_FORCED = 0, 1, 2
GTE_MAX_TRADE_LIST = 1 << 20


class GteTrade(C.Structure):
    """struct gte_trade (include/gte.h)."""
    _fields_ = [(n, {"<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in TRADE_LIST_FIELDS]


class GteTradeBatch(C.Structure):
    """struct gte_trade_batch (include/gte.h): what gte_read_trade_list leaves, pointers into library-owned host
    memory."""
    _fields_ = [("n_ids", C.c_int32), ("capacity", C.c_int32), ("n_trades", C.c_int64),
                ("first", C.POINTER(C.c_int64)), ("closed", C.POINTER(C.c_int32)), ("trades", C.POINTER(GteTrade))]


#: struct gte_strategy_trade_stats (include/gte.h), in declaration order: one 128-byte record per strategy
STRATEGY_TRADE_FIELDS = [(n, "<i8") for n in ("closed", "wins", "losses", "forced", "reversals", "exposure",
                                              "hold_sum")] + \
    [(n, "<f8") for n in ("gross_profit", "gross_loss", "ret_sq_sum", "best_trade", "worst_trade")] + \
    [(n, "<i4") for n in ("max_len", "max_loss_streak", "envs", "envs_traded")]
#: numpy view of an array of gte_strategy_trade_stats (gte_reduce_trade_stats)
STRATEGY_TRADE_DTYPE = STRATEGY_TRADE_FIELDS + [("reserved", "<i4", (4,))]


class GteStrategyTradeStats(C.Structure):
    """struct gte_strategy_trade_stats (include/gte.h)."""
    _fields_ = [(n, {"<i8": C.c_int64, "<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in STRATEGY_TRADE_FIELDS] + \
               [("reserved", C.c_int32 * 4)]


#: struct gte_period_stats (include/gte.h), in declaration order: one 32-byte record per (env, period)
PERIOD_FIELDS = [("reward_sum", "<f8"), ("reward_sq_sum", "<f8"), ("steps", "<i8"), ("trades", "<i4"), ("episodes", "<i4")]
#: numpy view of an array of gte_period_stats (gte_read_period_stats)
PERIOD_DTYPE = list(PERIOD_FIELDS)


class GtePeriodStats(C.Structure):
    """struct gte_period_stats (include/gte.h)."""
    _fields_ = [(n, {"<i8": C.c_int64, "<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in PERIOD_FIELDS]


#: struct gte_strategy_period_stats (include/gte.h), in declaration order: one 48-byte record per (strategy, period)
STRATEGY_PERIOD_FIELDS = [("reward_sum", "<f8"), ("reward_sq_sum", "<f8"), ("steps", "<i8"), ("trades", "<i8"),
                          ("episodes", "<i8"), ("envs_stepped", "<i4")]
#: numpy view of an array of gte_strategy_period_stats (gte_reduce_period_stats)
STRATEGY_PERIOD_DTYPE = STRATEGY_PERIOD_FIELDS + [("reserved", "<i4")]


class GteStrategyPeriodStats(C.Structure):
    """struct gte_strategy_period_stats (include/gte.h)."""
    _fields_ = [(n, {"<i8": C.c_int64, "<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in STRATEGY_PERIOD_FIELDS] + \
               [("reserved", C.c_int32)]


#: struct gte_reality_check_summary (include/gte.h), in declaration order: one 24-byte record
REALITY_CHECK_SUMMARY_DTYPE = [("best_mean", "<f8"), ("best", "<i4"), ("count_rc", "<i4"), ("eligible", "<i4"),
                               ("reserved", "<i4")]


class GteRealityCheckSummary(C.Structure):
    """struct gte_reality_check_summary (include/gte.h)."""
    _fields_ = [(n, {"<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in REALITY_CHECK_SUMMARY_DTYPE]


class GteRealityCheckOut(C.Structure):
    """struct gte_reality_check_out (include/gte.h): device pointers, kept as integers."""
    _fields_ = [(n, C.c_void_p) for n in ("mean", "boot_sum", "boot_sq_sum", "count_ge", "count_adj", "max_stat",
                                          "max_index", "summary")]


#: struct gte_spa_summary (include/gte.h), in declaration order: one 40-byte record
SPA_SUMMARY_DTYPE = [("statistic", "<f8")] + [(n, "<i4") for n in (
    "best", "count_lower", "count_consistent", "count_upper", "rounds_run", "num_rejected", "studentised", "reserved")]


class GteSpaSummary(C.Structure):
    """struct gte_spa_summary (include/gte.h)."""
    _fields_ = [(n, {"<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in SPA_SUMMARY_DTYPE]


class GteSpaOut(C.Structure):
    """struct gte_spa_out (include/gte.h): device pointers, kept as integers."""
    _fields_ = [(n, C.c_void_p) for n in ("t_stat", "std_error", "recentred", "count_adj", "rejected_round", "max_stat",
                                          "max_index", "crit", "round_rejected", "summary")]


#: struct gte_cscv_summary (include/gte.h), in declaration order: one 24-byte record
CSCV_SUMMARY_DTYPE = [(n, "<i4") for n in ("splits", "valid", "overfit", "loss", "eligible", "reserved")]


class GteCscvSummary(C.Structure):
    """struct gte_cscv_summary (include/gte.h)."""
    _fields_ = [(n, C.c_int32) for n, _ in CSCV_SUMMARY_DTYPE]


class GteCscvOut(C.Structure):
    """struct gte_cscv_out (include/gte.h): device pointers, kept as integers."""
    _fields_ = [(n, C.c_void_p) for n in ("best", "is_score", "oos_score", "below", "equal", "ranked", "summary")]


#: struct gte_diversify_summary (include/gte.h), in declaration order: one 20-byte record
DIVERSIFY_SUMMARY_DTYPE = [(n, "<i4") for n in ("picked", "candidates", "eligible", "remaining", "reserved")]


class GteDiversifySummary(C.Structure):
    """struct gte_diversify_summary (include/gte.h)."""
    _fields_ = [(n, C.c_int32) for n, _ in DIVERSIFY_SUMMARY_DTYPE]


class GteDiversifyOut(C.Structure):
    """struct gte_diversify_out (include/gte.h): device pointers, kept as integers."""
    _fields_ = [(n, C.c_void_p) for n in ("pick", "pick_score", "cluster_size", "owner", "owner_corr", "pick_corr",
                                          "summary")]


#: struct gte_mc_pool (include/gte.h), in declaration order: one 48-byte record per pool
MC_POOL_DTYPE = [(n, "<f8") for n in ("final_sum", "final_sq_sum", "mdd_sum", "mdd_sq_sum")] + \
    [(n, "<i4") for n in ("count_loss", "count_ruin", "pool_size", "path_len")]


class GteMcPool(C.Structure):
    """struct gte_mc_pool (include/gte.h)."""
    _fields_ = [(n, {"<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in MC_POOL_DTYPE]


class GteMcOut(C.Structure):
    """struct gte_mc_out (include/gte.h): device pointers, kept as integers; the four columns may be NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("final", "max_drawdown", "low", "max_loss_streak", "pool", "dd_count")]


#: struct gte_strategy_stats (include/gte.h), in declaration order: one 128-byte record per strategy
STRATEGY_FIELDS = [("steps", "<i8")] + \
    [(n, "<f8") for n in ("reward_sum", "reward_sq_sum", "ep_return_sum", "ep_return_sq_sum", "max_drawdown",
                          "best_reward_sum", "worst_reward_sum")] + \
    [(n, "<i8") for n in ("trades", "episodes", "terminations")] + \
    [(n, "<i4") for n in ("envs", "envs_stepped")]
#: numpy view of an array of gte_strategy_stats (gte_reduce_backtest_stats)
STRATEGY_DTYPE = STRATEGY_FIELDS + [("reserved", "<i4", (8,))]


class GteStrategyStats(C.Structure):
    """struct gte_strategy_stats (include/gte.h)."""
    _fields_ = [(n, {"<i8": C.c_int64, "<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in STRATEGY_FIELDS] + \
               [("reserved", C.c_int32 * 8)]


#: struct gte_indicator_spec (include/gte.h), in declaration order: 16 bytes per bank row
INDICATOR_FIELDS = [(n, "<i4") for n in ("kind", "source", "column", "n")]
#: numpy view of an array of gte_indicator_spec (gte_build_indicators)
INDICATOR_DTYPE = INDICATOR_FIELDS

#: struct gte_signal_compose (include/gte.h), in declaration order: 128 bytes per composed strategy
COMPOSE_FIELDS = [("in", "<i4", (4,)), ("n_in", "i1"), ("initial", "i1"), ("pos_invalid", "i1"), ("reserved0", "i1"),
                  ("lut", "i1", (81,)), ("reserved", "i1", (27,))]
#: numpy view of an array of gte_signal_compose (gte_compose_signals)
COMPOSE_DTYPE = COMPOSE_FIELDS
#: GTE_COMPOSE_KEEP
COMPOSE_KEEP = -128

#: struct gte_exit_rule (include/gte.h), in declaration order: 32 bytes per exit rule
EXIT_RULE_FIELDS = [("stop_loss", "<f4"), ("take_profit", "<f4"), ("trailing", "<f4"), ("max_hold", "<i4"),
                    ("exit_position", "i1"), ("reserved0", "i1", (3,)), ("reserved", "<i4", (3,))]
#: numpy view of an array of gte_exit_rule (gte_bind_exit_rules)
EXIT_RULE_DTYPE = EXIT_RULE_FIELDS
#: struct gte_exit_state (include/gte.h), in declaration order: 80 bytes per env
EXIT_STATE_FIELDS = [("entry", "<f8"), ("peak", "<f8"), ("v_seen", "<f8")] + \
    [(n, "<i4") for n in ("held", "latched", "latched_raw", "i_seen", "episode_seen", "step_seen", "decided",
                          "decided_action")]
#: numpy view of an array of gte_exit_state (gte_read_exit_state)
EXIT_STATE_DTYPE = EXIT_STATE_FIELDS + [("reserved", "<i4", (2,)), ("exits", "<i4", (4,))]
#: index of each exit kind in gte_exit_state.exits (GTE_EXIT_*)
EXIT_KINDS = ("stop", "trail", "target", "time")


class GteExitRule(C.Structure):
    """struct gte_exit_rule (include/gte.h)."""
    _fields_ = [("stop_loss", C.c_float), ("take_profit", C.c_float), ("trailing", C.c_float),
                ("max_hold", C.c_int32), ("exit_position", C.c_int8), ("reserved0", C.c_int8 * 3),
                ("reserved", C.c_int32 * 3)]


class GteExitState(C.Structure):
    """struct gte_exit_state (include/gte.h)."""
    _fields_ = [(n, {"<f8": C.c_double, "<i4": C.c_int32}[t]) for n, t in EXIT_STATE_FIELDS] + \
               [("reserved", C.c_int32 * 2), ("exits", C.c_int32 * 4)]


#: enum gte_indicator_kind / gte_indicator_source and GTE_IND_MAX_WINDOW (include/gte.h)
IND_KINDS = ("value", "sma", "std", "zscore", "max", "min", "diff", "roc", "ema", "rsi")
IND_SOURCES = ("close", "high", "low", "feature", "input")
IND_MAX_WINDOW = 4096


class GteOutputs(C.Structure):
    """struct gte_outputs: device pointers, kept as integers."""

    _fields_ = [
        ("obs", C.c_void_p),
        ("reward", C.c_void_p),
        ("reward64", C.c_void_p),
        ("terminated", C.c_void_p),
        ("truncated", C.c_void_p),
        ("term_count", C.c_void_p),
        ("term_ids", C.c_void_p),
        ("obs_elems_per_env", C.c_int64),
        ("term_slot", C.c_int32),
        ("reserved0", C.c_int32),
        ("final_obs", C.c_void_p),
    ]


class GteObsView(C.Structure):
    """struct gte_obs_view_t: where the current observation lives (sliding observation buffer)."""

    _fields_ = [("base", C.c_void_p), ("rows_per_env", C.c_int32), ("head", C.c_int32),
                ("sliding", C.c_int32), ("slack_rows", C.c_int32)]


class GteStateView(C.Structure):
    """struct gte_state_view: device pointers, kept as integers."""

    _fields_ = [
        ("idx", C.c_void_p),
        ("step", C.c_void_p),
        ("position_index", C.c_void_p),
        ("dataset_index", C.c_void_p),
        ("start_idx", C.c_void_p),
        ("episode", C.c_void_p),
        ("needs_reset", C.c_void_p),
        ("asset", C.c_void_p),
        ("fiat", C.c_void_p),
        ("interest_asset", C.c_void_p),
        ("interest_fiat", C.c_void_p),
        ("portfolio_valuation", C.c_void_p),
        ("real_position", C.c_void_p),
    ]


class GteLogView(C.Structure):
    """struct gte_log_view: device pointers of the trajectory log, kept as integers."""

    _fields_ = [("idx", C.c_void_p), ("step", C.c_void_p), ("position_index", C.c_void_p),
                ("dataset_index", C.c_void_p), ("portfolio_valuation", C.c_void_p),
                ("real_position", C.c_void_p), ("reward", C.c_void_p), ("flags", C.c_void_p),
                ("rows", C.c_int64), ("L", C.c_int32), ("N", C.c_int32),
                ("asset", C.c_void_p), ("fiat", C.c_void_p), ("interest_asset", C.c_void_p),
                ("interest_fiat", C.c_void_p), ("env_stride", C.c_int64), ("row_stride", C.c_int64),
                ("cursor", C.c_void_p), ("cursor_slot", C.c_int32), ("reserved0", C.c_int32)]


class GteSchedule(C.Structure):
    """struct gte_schedule: the host-side schedule a stream capture advances (StepGraph)."""

    _fields_ = [("log_rows", C.c_int64), ("term_slot", C.c_int32), ("steps_since_rebuild", C.c_int32)]


class GteLogBatch(C.Structure):
    """struct gte_log_batch: host pointers into the library's pinned buffer (gte_read_log_envs)."""

    _fields_ = [("n_ids", C.c_int32), ("max_rows", C.c_int32), ("n_rows", C.c_void_p),
                ("idx", C.c_void_p), ("step", C.c_void_p), ("position_index", C.c_void_p),
                ("dataset_index", C.c_void_p), ("portfolio_valuation", C.c_void_p),
                ("real_position", C.c_void_p), ("reward", C.c_void_p), ("asset", C.c_void_p),
                ("fiat", C.c_void_p), ("interest_asset", C.c_void_p), ("interest_fiat", C.c_void_p),
                ("flags", C.c_void_p)]


#: dtype of every log array
LOG_DTYPES = {"idx": "int32", "step": "int32", "position_index": "int32", "dataset_index": "int32",
              "portfolio_valuation": "float64", "real_position": "float64", "reward": "float64",
              "flags": "uint8", "asset": "float64", "fiat": "float64",
              "interest_asset": "float64", "interest_fiat": "float64"}

#: dtype of every gte_state_view member, in declaration order
STATE_DTYPES = {
    "idx": "int32", "step": "int32", "position_index": "int32",
    "dataset_index": "int32", "start_idx": "int32", "episode": "int32",
    "needs_reset": "int32", "asset": "float64", "fiat": "float64",
    "interest_asset": "float64", "interest_fiat": "float64",
    "portfolio_valuation": "float64", "real_position": "float64",
}

_P = C.POINTER

#: every symbol include/gte.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gte_create": (C.c_int, [_P(GteConfig), _P(C.c_void_p)]),
    "gte_upload_dataset": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int64]),
    "gte_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gte_set_autoreset_injection": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "gte_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "gte_get_schedule": (C.c_int, [C.c_void_p, _P(GteSchedule)]),
    "gte_set_schedule": (C.c_int, [C.c_void_p, _P(GteSchedule)]),
    "gte_advance_log": (C.c_int, [C.c_void_p, C.c_int64]),
    "gte_add_limit_orders": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gte_get_log": (C.c_int, [C.c_void_p, _P(GteLogView)]),
    "gte_read_log_portfolio": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
                               + [_P(C.c_int32)]),
    "gte_read_log_envs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    _P(GteLogBatch)]),
    "gte_set_log_reward": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gte_apply_reward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "gte_get_final_state": (C.c_int, [C.c_void_p, _P(GteStateView)]),
    "gte_set_dynamic_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "gte_set_dynamic_columns": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int32)]),
    "gte_read_log": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8 + [_P(C.c_int32)]),
    "gte_get_outputs": (C.c_int, [C.c_void_p, _P(GteOutputs)]),
    "gte_get_state": (C.c_int, [C.c_void_p, _P(GteStateView)]),
    "gte_bind_outputs": (C.c_int, [C.c_void_p, _P(GteOutputs)]),
    "gte_obs_view": (C.c_int, [C.c_void_p, _P(GteObsView)]),
    "gte_bind_sliding_obs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "gte_read_env": (C.c_int, [C.c_void_p, C.c_int32, _P(GteEnvSnapshot), C.c_void_p]),
    "gte_read_envs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gte_read_envs_view": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     _P(C.c_void_p), _P(C.c_void_p)]),
    "gte_rollout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _P(GteRolloutBufs)]),
    "gte_backtest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(C.c_void_p)]),
    "gte_read_backtest_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gte_bind_signals": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64]),
    "gte_signal_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gte_backtest_signals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(C.c_void_p)]),
    "gte_backtest_curves": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      _P(GteCurveBufs), _P(C.c_void_p)]),
    "gte_bind_exit_rules": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, _P(C.c_void_p)]),
    "gte_read_exit_state": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gte_track_trades": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "gte_read_trade_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gte_track_trade_list": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "gte_read_trade_list": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _P(GteTradeBatch)]),
    "gte_pack_trade_list": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "gte_reduce_trade_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gte_rank_trade_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "gte_bind_periods": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "gte_track_periods": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "gte_read_period_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gte_reduce_period_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "gte_rank_period_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(C.c_uint64), C.c_int32,
                                        C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gte_bootstrap_weights": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_uint64, C.c_void_p]),
    "gte_reality_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(C.c_uint64), C.c_void_p,
                                    C.c_void_p, C.c_int32, _P(GteRealityCheckOut)]),
    "gte_spa_test": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(C.c_uint64), C.c_void_p, C.c_void_p,
                               C.c_int32, C.c_double, C.c_int32, C.c_int32, _P(GteRealityCheckOut), _P(GteSpaOut)]),
    "gte_cscv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                           C.c_int32, C.c_int32, _P(GteCscvOut)]),
    "gte_diversify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _P(C.c_uint64), C.c_void_p, C.c_double,
                                C.c_int32, _P(GteDiversifyOut)]),
    "gte_pool_trades": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int64]),
    "gte_trade_monte_carlo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_uint64, C.c_double, _P(C.c_double), C.c_int32, _P(GteMcOut)]),
    "gte_build_signals": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_int64]),
    "gte_compose_signals": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_int64]),
    "gte_build_indicators": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64,
                                       C.c_void_p, C.c_int64]),
    "gte_reduce_backtest_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gte_rank_strategies": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "gte_bind_returns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gte_comm_unique_id": (C.c_int, [C.c_void_p]),
    "gte_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "gte_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "gte_allgather_returns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "gte_allgather_obs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "gte_comm_wait": (C.c_int, [C.c_void_p, C.c_int32]),
    "gte_comm_synchronize": (C.c_int, [C.c_void_p]),
    "gte_comm_destroy": (C.c_int, [C.c_void_p]),
    "gte_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gte_use_own_stream": (C.c_int, [C.c_void_p]),
    "gte_synchronize": (C.c_int, [C.c_void_p]),
    "gte_timer_start": (C.c_int, [C.c_void_p]),
    "gte_timer_stop": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "gte_read_obs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gte_copy_to_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "gte_get_launch_info": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32),
                                      _P(C.c_int32), _P(C.c_int32)]),
    "gte_destroy": (None, [C.c_void_p]),
    "gte_last_error": (C.c_char_p, []),
    "gte_abi_version": (C.c_int, []),
    "gte_device_count": (C.c_int, []),
}

_HERE = os.path.dirname(os.path.abspath(__file__))
# GTE_LIBRARY: another BUILD of libgte to load instead (A/B builds of the kernels, tools/)
LIB_PATH = os.environ.get("GTE_LIBRARY") or os.path.join(_HERE, "csrc", "libgte.so")
_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """Load libgte.so (the HIP build).  Fails loudly: there is no fallback."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            f"{p} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
            "gym-trading-env_amd/csrc`). There is no CPU fallback for the env.")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; libgte needs the same SONAME.  Two
    # HIP runtimes in one process do not share devices, so when torch is installed load
    # it FIRST: the dynamic linker then binds libgte to the runtime torch uses.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.gte_abi_version() != GTE_ABI_VERSION:
        raise ImportError(f"{p}: ABI {lib.gte_abi_version()} != {GTE_ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def check(lib: C.CDLL, status: int) -> None:
    if status != GTE_OK:
        msg = lib.gte_last_error()
        raise GteError(status, msg.decode() if msg else "unknown")
