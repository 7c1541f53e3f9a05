// gte_api_backtest.hip — the backtest entry points of include/gte.h (backtest() itself is in gte_api.hip, the unit
// of enqueue_step), signal tables and their builders, exit rules, trade tracking with the trade list and its two
// gathers, period rows and tracking, and the reads of the per-env records.
#include "gte_host.h"

namespace gte_host {

// Dataset d's signal table becomes t (base null = unbound), on the host and on the device; the
// caller has waited for the stream.  Nothing changes if the copy fails.
int publish_signal_table(gte_env* E, int32_t d, const gte::SignalTable& t) {
  const gte::SignalTable before = E->signals.h_tab[d];
  E->signals.h_tab[d] = t;
  const hipError_t e = hipMemcpy(E->signals.d_tab, E->signals.h_tab.data(), sizeof(gte::SignalTable) * E->signals.h_tab.size(),
                                 hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    E->signals.h_tab[d] = before;
    return fail(GTE_ERR_HIP, "publishing the signal table of dataset %d: %s", d, hipGetErrorString(e));
  }
  bool any = false;
  for (const gte::SignalTable& x : E->signals.h_tab) any = any || x.base != nullptr;
  if (!any) E->signals.S = 0;
  return GTE_OK;
}

// Dataset d's period row becomes `row` (empty = unbound), on the host and on the device, and the row it had is
// freed; the caller has waited for the stream.  Nothing changes if the copy fails (`row` stays the caller's).
int publish_period_row(gte_env* E, int32_t d, DeviceBlock&& row) {
  const gte::PeriodRow before = E->periods.h_row[d];
  E->periods.h_row[d] = gte::PeriodRow{row.as<const int8_t>(), (int32_t)row.bytes()};
  const hipError_t e = hipMemcpy(E->periods.d_row, E->periods.h_row.data(), sizeof(gte::PeriodRow) * E->periods.h_row.size(),
                                 hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    E->periods.h_row[d] = before;
    return fail(GTE_ERR_HIP, "publishing the period row of dataset %d: %s", d, hipGetErrorString(e));
  }
  E->periods.row_block[d] = std::move(row);
  // while tracking is on the next backtest call clears: its records would mix two period maps (off, nothing is
  // kept, and switching on marks the change itself: an untracked backtest keeps honouring its `clear`)
  if (E->periods.B > 0) E->periods.changed = true;
  return GTE_OK;
}

// what both gathers check first
int trade_list_on(gte_env* E, const char* who) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (E->trades.cap < 1 || !E->trades.list.get() || !E->trades.stats)
    return fail(GTE_ERR_STATE, "%s: the trade list is off (gte_track_trade_list)", who);
  // a switch of tracking, of the list or of its capacity since the last backtest call: `closed` still counts the
  // trades of before, and the list (fresh memory, never zeroed) holds none of them
  if (E->trades.changed)
    return fail(GTE_ERR_STATE, "%s: the trade list was switched and no backtest call has cleared the records since: "
                "it holds nothing yet", who);
  return GTE_OK;
}

}  // namespace gte_host
extern "C" {

int gte_backtest(gte_env* E, const int32_t* actions, int32_t n_steps, int32_t clear,
                 gte_backtest_stats** stats_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_backtest before gte_reset");
  if (!actions) return fail(GTE_ERR_INVALID, "actions is NULL");
  return backtest_entry(E, "gte_backtest", actions, nullptr, n_steps, clear, stats_device, nullptr);
}

// dataset d of a builder call -> its T: a builder runs outside a capture, on a dataset that was uploaded
static int builder_dataset(gte_env* E, const char* who, int32_t d, int64_t* T) {
  if (d < 0 || d >= E->p.D) return fail(GTE_ERR_INVALID, "dataset index %d out of range", d);
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "%s inside a stream capture", who);
  *T = E->h_ds[d].T;
  if (*T <= 0) return fail(GTE_ERR_STATE, "%s: dataset %d was never uploaded", who, d);
  return GTE_OK;
}

// rows first .. first + count - 1 of a per-env record array (`base`: row_bytes per env, or NULL before the call
// `before` made it) to the host, after everything enqueued on the env's stream
static int read_records(gte_env* E, const char* who, const char* before, const void* base, size_t row_bytes,
                        int32_t first, int32_t count, void* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!base) return fail(GTE_ERR_STATE, "%s before %s", who, before);
  if (first < 0 || count < 0 || (int64_t)first + count > E->p.N)
    return fail(GTE_ERR_INVALID, "env range [%d, %d) outside [0, %d)", first, first + count, E->p.N);
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));
  if (count > 0)
    HIPCHK(hipMemcpy(out, (const char*)base + (size_t)first * row_bytes, (size_t)count * row_bytes, hipMemcpyDeviceToHost));
  return GTE_OK;
}

int gte_bind_signals(gte_env* E, int32_t d, const int8_t* signals_device, int32_t n_strategies,
                     int64_t row_stride) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  const Params& p = E->p;
  if (d < 0 || d >= p.D) return fail(GTE_ERR_INVALID, "dataset index %d out of range", d);
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bind_signals inside a stream capture");
  if (signals_device) {
    const int64_t T = E->h_ds[d].T;
    if (T <= 0) return fail(GTE_ERR_STATE, "gte_bind_signals: dataset %d was never uploaded", d);
    if ((uintptr_t)signals_device & 15) return fail(GTE_ERR_INVALID, "signals must be 16-byte aligned");
    TRY(check_stride("row_stride", row_stride, sizeof(int8_t), T, d));
    if (n_strategies < 1) return fail(GTE_ERR_INVALID, "n_strategies must be >= 1");
    for (int o = 0; o < (int)E->signals.h_tab.size(); ++o)
      if (o != d && E->signals.h_tab[o].base && E->signals.S != n_strategies)
        return fail(GTE_ERR_INVALID, "n_strategies %d: the table of dataset %d has %d", n_strategies, o, E->signals.S);
  } else if (!E->signals.d_tab) {
    return GTE_OK;  // nothing was ever bound
  }
  HIPCHK(hipSetDevice(E->cfg.device));
  if (!E->signals.d_tab) {
    E->signals.h_tab.assign((size_t)p.D, gte::SignalTable{nullptr, 0});
    TRY(dev_alloc(E, &E->signals.d_tab, (size_t)p.D));
  }
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight read the descriptors
  TRY(publish_signal_table(E, d, signals_device ? gte::SignalTable{signals_device, row_stride}
                                                : gte::SignalTable{nullptr, 0}));
  if (signals_device) E->signals.S = n_strategies;
  return GTE_OK;
}

// every resident dataset has a table: the lookups may run
static int signals_ready(const gte_env* E, const char* who) {
  if (!E->was_reset) return fail(GTE_ERR_STATE, "%s before gte_reset", who);
  for (int d = 0; d < E->p.D; ++d)
    if (!E->signals.d_tab || !E->signals.h_tab[d].base)
      return fail(GTE_ERR_STATE, "%s: dataset %d has no signal table (gte_bind_signals)", who, d);
  return GTE_OK;
}

int gte_signal_actions(gte_env* E, const int32_t* strategy_device, int32_t* actions_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!actions_device) return fail(GTE_ERR_INVALID, "actions is NULL");
  TRY(signals_ready(E, "gte_signal_actions"));
  if (!stream_capturing(E)) HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = launch_lookup(E, strategy_device, actions_device);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "signal lookup launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_backtest_signals(gte_env* E, const int32_t* strategy_device, int32_t n_steps, int32_t clear,
                         gte_backtest_stats** stats_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  TRY(signals_ready(E, "gte_backtest_signals"));
  return backtest_entry(E, "gte_backtest_signals", nullptr, strategy_device, n_steps, clear, stats_device, nullptr);
}

int gte_backtest_curves(gte_env* E, const int32_t* actions, const int32_t* strategy_device, int32_t n_steps,
                        int32_t stride, int32_t clear, const gte_curve_bufs* bufs, gte_backtest_stats** stats_device) {
  const char* const who = "gte_backtest_curves";
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "%s before gte_reset", who);
  if (!bufs) return fail(GTE_ERR_INVALID, "%s: bufs is NULL", who);
  if (n_steps < 1) return fail(GTE_ERR_INVALID, "n_steps must be >= 1");
  if (stride < 1) return fail(GTE_ERR_INVALID, "%s: stride %d must be >= 1", who, stride);
  if (!bufs->valuation && !bufs->drawdown && !bufs->reward && !bufs->position && !bufs->row && !bufs->flags)
    return fail(GTE_ERR_INVALID, "%s: all six columns are NULL, nothing to keep", who);
  if (((uintptr_t)bufs->valuation | (uintptr_t)bufs->drawdown | (uintptr_t)bufs->reward) & 7)
    return fail(GTE_ERR_INVALID, "%s: valuation, drawdown and reward must be 8-byte aligned", who);
  if (((uintptr_t)bufs->position | (uintptr_t)bufs->row) & 3)
    return fail(GTE_ERR_INVALID, "%s: position and row must be 4-byte aligned", who);
  if (E->trades.on || E->periods.B > 0)
    return fail(GTE_ERR_STATE, "%s: %s tracking is on, and a launch keeps one tracker (gte_track_%s(env, 0, ...) first)",
                who, E->trades.on ? "trade" : "period", E->trades.on ? "trades" : "periods");
  if (!actions) TRY(signals_ready(E, who));
  // (the carry is the library's: backtest() allocates it, on the env's device, and fills it in)
  gte::Curves cv = {nullptr, stride, *bufs};
  return backtest_entry(E, who, actions, actions ? nullptr : strategy_device, n_steps, clear, stats_device, &cv);
}

int gte_bind_exit_rules(gte_env* E, const gte_exit_rule* rules_device, int32_t n_rules,
                        const int32_t* rule_of_env_device, gte_exit_state** state_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bind_exit_rules inside a stream capture");
  if (rules_device) {
    if ((uintptr_t)rules_device & 3) return fail(GTE_ERR_INVALID, "exit rules must be 4-byte aligned");
    if ((uintptr_t)rule_of_env_device & 3) return fail(GTE_ERR_INVALID, "rule_of_env must be 4-byte aligned");
    if (n_rules < 1) return fail(GTE_ERR_INVALID, "n_rules must be >= 1");
  }
  HIPCHK(hipSetDevice(E->cfg.device));
  if (rules_device && !E->signals.exits.state) TRY(dev_alloc_late(E, &E->signals.exits.state, (size_t)E->p.N));
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight read the rules and the state
  if (E->signals.exits.state) {
    const hipError_t e = gte::launch_exit_init(E->signals.exits.state, E->p.N, E->stream);
    if (e != hipSuccess) return fail(GTE_ERR_HIP, "exit state launch: %s", hipGetErrorString(e));
  }
  E->signals.exits.rules = rules_device;
  E->signals.exits.rule_of_env = rules_device ? rule_of_env_device : nullptr;
  E->signals.exits.n_rules = rules_device ? n_rules : 0;
  if (state_device) *state_device = E->signals.exits.state;
  return GTE_OK;
}

int gte_read_exit_state(gte_env* E, int32_t first, int32_t count, gte_exit_state* out) {
  return read_records(E, "gte_read_exit_state", "gte_bind_exit_rules", E ? E->signals.exits.state : nullptr,
                      sizeof(gte_exit_state), first, count, out);
}

int gte_build_signals(gte_env* E, int32_t d, const float* indicators_device, int32_t n_indicators,
                      int64_t ind_stride, const gte_signal_rule* rules_device, int32_t n_rules,
                      int8_t* table_device, int64_t row_stride) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  int64_t T;
  TRY(builder_dataset(E, "gte_build_signals", d, &T));
  if (!indicators_device || !rules_device || !table_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (((uintptr_t)indicators_device & 15) || ((uintptr_t)table_device & 15))
    return fail(GTE_ERR_INVALID, "the indicator bank and the table must be 16-byte aligned");
  if ((uintptr_t)rules_device & 3) return fail(GTE_ERR_INVALID, "rules must be 4-byte aligned");
  TRY(check_stride("row_stride", row_stride, sizeof(int8_t), T, d));
  TRY(check_stride("ind_stride", ind_stride, sizeof(float), T, d));
  if (n_indicators < 1) return fail(GTE_ERR_INVALID, "n_indicators must be >= 1");
  if (n_rules < 1) return fail(GTE_ERR_INVALID, "n_rules must be >= 1");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_build_signals(indicators_device, n_indicators, ind_stride, rules_device, n_rules,
                                                 T, table_device, row_stride, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "signal build launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_compose_signals(gte_env* E, int32_t d, const int8_t* clauses_device, int32_t n_clause_rows,
                        int64_t clause_stride, const gte_signal_compose* specs_device, int32_t n_specs,
                        int8_t* table_device, int64_t row_stride) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  int64_t T;
  TRY(builder_dataset(E, "gte_compose_signals", d, &T));
  if (!clauses_device || !specs_device || !table_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (((uintptr_t)clauses_device & 15) || ((uintptr_t)table_device & 15))
    return fail(GTE_ERR_INVALID, "the clause table and the table must be 16-byte aligned");
  if ((uintptr_t)specs_device & 3) return fail(GTE_ERR_INVALID, "specs must be 4-byte aligned");
  TRY(check_stride("row_stride", row_stride, sizeof(int8_t), T, d));
  TRY(check_stride("clause_stride", clause_stride, sizeof(int8_t), T, d));
  if (n_clause_rows < 1) return fail(GTE_ERR_INVALID, "n_clause_rows must be >= 1");
  if (n_specs < 1) return fail(GTE_ERR_INVALID, "n_specs must be >= 1");
  // what the kernel may read of the clause table and what it writes of the table: disjoint
  if (spans_overlap({clauses_device, n_clause_rows, clause_stride, sizeof(int8_t)},
                    {table_device, n_specs, row_stride, sizeof(int8_t)}, round_up_16(T)))
    return fail(GTE_ERR_INVALID, "the clause table and the table overlap");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_compose_signals(clauses_device, n_clause_rows, clause_stride, specs_device, n_specs,
                                                   T, table_device, row_stride, E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "signal compose launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_build_indicators(gte_env* E, int32_t d, const gte_indicator_spec* specs_device, int32_t n_specs,
                         const float* input_device, int32_t n_inputs, int64_t input_stride, float* bank_device,
                         int64_t ind_stride) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  int64_t T;
  TRY(builder_dataset(E, "gte_build_indicators", d, &T));
  if (T > INT32_MAX - 2 * GTE_IND_MAX_WINDOW)  // (the kernel indexes rows with 32 bits, like EnvRec.idx)
    return fail(GTE_ERR_INVALID, "gte_build_indicators: dataset %d has too many rows", d);
  if (!specs_device || !bank_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (n_inputs < 0) return fail(GTE_ERR_INVALID, "n_inputs must be >= 0");
  if ((input_device != nullptr) != (n_inputs > 0))
    return fail(GTE_ERR_INVALID, "input_device must be non-NULL exactly when n_inputs > 0");
  if (((uintptr_t)bank_device & 15) || ((uintptr_t)input_device & 15))
    return fail(GTE_ERR_INVALID, "the indicator bank and the input bank must be 16-byte aligned");
  if ((uintptr_t)specs_device & 3) return fail(GTE_ERR_INVALID, "specs must be 4-byte aligned");
  TRY(check_stride("ind_stride", ind_stride, sizeof(float), T, d));
  if (n_inputs > 0) TRY(check_stride("input_stride", input_stride, sizeof(float), T, d));
  if (n_specs < 1) return fail(GTE_ERR_INVALID, "n_specs must be >= 1");
  // what the kernel reads of the input and what it writes of the bank: disjoint
  if (n_inputs > 0 && spans_overlap({input_device, n_inputs, input_stride, sizeof(float)},
                                    {bank_device, n_specs, ind_stride, sizeof(float)}, round_up_16(T)))
    return fail(GTE_ERR_INVALID, "the input bank and the indicator bank overlap");
  HIPCHK(hipSetDevice(E->cfg.device));
  const hipError_t e = gte::launch_build_indicators(E->h_ds[d], E->p.Fobs, E->p.Fobs - E->p.nd, specs_device, n_specs,
                                                    input_device, n_inputs, input_stride, bank_device, ind_stride,
                                                    E->stream);
  if (e != hipSuccess) return fail(GTE_ERR_HIP, "indicator build launch: %s", hipGetErrorString(e));
  return GTE_OK;
}

int gte_read_backtest_stats(gte_env* E, int32_t first, int32_t count, gte_backtest_stats* out) {
  return read_records(E, "gte_read_backtest_stats", "gte_backtest", E ? E->backtest.stats : nullptr,
                      sizeof(gte_backtest_stats), first, count, out);
}

// the list turned off: its memory goes back (N * capacity * 48 bytes; the env's stream is idle), open_row stays
static void drop_trade_list(gte_env* E) {
  E->trades.list.reset();
  E->trades.cap = E->trades.alloc_cap = 0;
}

int gte_track_trades(gte_env* E, int32_t on, gte_trade_stats** records_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_track_trades before gte_reset");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_track_trades inside a stream capture");
  if (on && E->periods.B > 0)
    return fail(GTE_ERR_STATE, "gte_track_trades: period tracking is on, and trade and period records together are "
                "not implemented (gte_track_periods(env, 0, ...) first)");
  HIPCHK(hipSetDevice(E->cfg.device));
  if (on && !E->trades.stats) TRY(dev_alloc_late(E, &E->trades.stats, (size_t)E->p.N));
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight write the records
  if ((on != 0) != E->trades.on) E->trades.changed = true;
  E->trades.on = on != 0;
  if (!on && E->trades.cap > 0) {  // the list goes with the tracking
    drop_trade_list(E);
    E->trades.changed = true;
  }
  if (records_device) *records_device = E->trades.stats;
  return GTE_OK;
}

int gte_track_trade_list(gte_env* E, int32_t capacity, gte_trade** list_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (capacity < 0 || capacity > GTE_MAX_TRADE_LIST)
    return fail(GTE_ERR_INVALID, "gte_track_trade_list: capacity %d outside [0, %d]", capacity, GTE_MAX_TRADE_LIST);
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_track_trade_list before gte_reset");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_track_trade_list inside a stream capture");
  if (capacity > 0 && !E->trades.on)
    return fail(GTE_ERR_STATE, "gte_track_trade_list: trade tracking is off (gte_track_trades(env, 1, ...) first)");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight write the list
  if (capacity > 0 && capacity != E->trades.alloc_cap) {
    DeviceBlock fresh;  // (released again if open_row cannot be had)
    TRY(device_alloc(&fresh, sizeof(gte_trade) * (size_t)E->p.N * (size_t)capacity,
                     "trade list (%d envs x %d trades): %s", E->p.N, capacity));
    if (!E->trades.open_row.get())  // (written by the next backtest call's clearing: trades.changed)
      TRY(device_alloc(&E->trades.open_row, sizeof(int32_t) * (size_t)E->p.N, "trade list (%d envs x %d trades): %s",
                       E->p.N, capacity));
    E->trades.list = std::move(fresh);  // the old list is freed (the new one never zeroed: `closed` says what of it is valid)
    E->trades.alloc_cap = capacity;
  }
  if (capacity != E->trades.cap) E->trades.changed = true;
  E->trades.cap = capacity;
  if (capacity == 0) drop_trade_list(E);
  if (list_device) *list_device = E->trades.list.as<gte_trade>();
  return GTE_OK;
}

static size_t round_up_16z(size_t n) { return (n + 15) & ~(size_t)15; }

int gte_read_trade_list(gte_env* E, const int32_t* env_ids, int32_t n_ids, gte_trade_batch* out) {
  TRY(trade_list_on(E, "gte_read_trade_list"));
  if (!out) return fail(GTE_ERR_INVALID, "NULL argument");
  const int N = E->p.N;
  if (!env_ids) n_ids = N;
  if (n_ids < 0) return fail(GTE_ERR_INVALID, "n_ids must be >= 0");
  for (int32_t i = 0; env_ids && i < n_ids; ++i)
    if (env_ids[i] < 0 || env_ids[i] >= N) return fail(GTE_ERR_INVALID, "env_ids[%d] = %d out of range", i, env_ids[i]);
  HIPCHK(hipSetDevice(E->cfg.device));
  // the device block: [ids i32 n -> 16] [first i64 n+1 | closed i32 n -> 16] [trades]; the host copy: from `first` on
  const size_t n = (size_t)n_ids;
  const size_t ids_bytes = round_up_16z(4 * n), head = round_up_16z(8 * (n + 1) + 4 * n);
  const gte::TradeList tl = {E->trades.list.as<gte_trade>(), E->trades.open_row.as<int32_t>(), E->trades.cap};
  int64_t total = 0;
  char* b = nullptr;
  int64_t* first = nullptr;
  // count and scan; one read of the total; if the block cannot hold that many records it grows and is counted
  // into again; then the pack
  for (int pass = 0; pass < 2; ++pass) {
    const size_t need = ids_bytes + head + sizeof(gte_trade) * (size_t)total;
    if (pass == 1 && need <= E->trades.dev.bytes()) break;
    if (need > E->trades.dev.bytes()) {
      DeviceBlock fresh;
      const size_t bytes = gte_own::grow_by_half(E->trades.dev.bytes(), need);
      TRY(device_alloc(&fresh, bytes, "trade list block (%zu bytes): %s", bytes));
      HIPCHK(hipStreamSynchronize(E->stream));  // (a gather in flight writes the old block)
      E->trades.dev = std::move(fresh);
    }
    b = E->trades.dev.as<char>();
    first = (int64_t*)(b + ids_bytes);
    if (env_ids && n) HIPCHK(hipMemcpyAsync(b, env_ids, 4 * n, hipMemcpyHostToDevice, E->stream));
    const hipError_t le = gte::launch_trade_list_scan(E->trades.stats, tl, N, env_ids ? (const int32_t*)b : nullptr, n_ids,
                                                      first, (int32_t*)(first + n + 1), E->stream);
    if (le != hipSuccess) return fail(GTE_ERR_HIP, "trade list scan launch: %s", hipGetErrorString(le));
    if (pass == 0) {
      HIPCHK(hipMemcpyAsync(&total, first + n, 8, hipMemcpyDeviceToHost, E->stream));
      HIPCHK(hipStreamSynchronize(E->stream));
    }
  }
  if (total > 0) {
    const hipError_t le = gte::launch_trade_list_pack(tl, N, env_ids ? (const int32_t*)b : nullptr, n_ids, first,
                                                      (gte_trade*)(b + ids_bytes + head), total, E->stream);
    if (le != hipSuccess) return fail(GTE_ERR_HIP, "trade list pack launch: %s", hipGetErrorString(le));
  }
  const size_t bytes = head + sizeof(gte_trade) * (size_t)total;
  if (bytes > E->trades.host.bytes())
    TRY(pinned_alloc(&E->trades.host, gte_own::grow_by_half(E->trades.host.bytes(), bytes), hipHostMallocDefault));
  HIPCHK(hipMemcpyAsync(E->trades.host.get(), b + ids_bytes, bytes, hipMemcpyDeviceToHost, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));
  out->n_ids = n_ids;
  out->capacity = E->trades.cap;
  out->n_trades = total;
  out->first = E->trades.host.as<const int64_t>();
  out->closed = (const int32_t*)(out->first + n + 1);
  out->trades = (const gte_trade*)(E->trades.host.as<const char>() + head);
  return GTE_OK;
}

int gte_pack_trade_list(gte_env* E, const int32_t* env_ids_device, int32_t n_ids, int64_t* first_device,
                        int32_t* closed_device, gte_trade* trades_device, int64_t max_trades) {
  TRY(trade_list_on(E, "gte_pack_trade_list"));
  if (!env_ids_device) n_ids = E->p.N;
  if (n_ids < 0) return fail(GTE_ERR_INVALID, "n_ids must be >= 0");
  if (max_trades < 0 || (max_trades > 0 && !trades_device))
    return fail(GTE_ERR_INVALID, "trades_device (gte_trade [max_trades]) is NULL or max_trades < 0");
  if (!first_device || ((uintptr_t)first_device & 7) || (n_ids > 0 && !closed_device) ||
      ((uintptr_t)closed_device & 3) || ((uintptr_t)env_ids_device & 3))
    return fail(GTE_ERR_INVALID, "first_device (int64 [n_ids + 1]), closed_device and env_ids_device (int32 [n_ids]) "
                "must be aligned device pointers");
  if ((uintptr_t)trades_device & 15) return fail(GTE_ERR_INVALID, "trades_device must be 16-byte aligned");
  HIPCHK(hipSetDevice(E->cfg.device));
  const gte::TradeList tl = {E->trades.list.as<gte_trade>(), E->trades.open_row.as<int32_t>(), E->trades.cap};
  hipError_t le = gte::launch_trade_list_scan(E->trades.stats, tl, E->p.N, env_ids_device, n_ids, first_device,
                                              closed_device, E->stream);
  if (le == hipSuccess && max_trades > 0 && n_ids > 0)
    le = gte::launch_trade_list_pack(tl, E->p.N, env_ids_device, n_ids, first_device, trades_device, max_trades,
                                     E->stream);
  if (le != hipSuccess) return fail(GTE_ERR_HIP, "trade list gather launch: %s", hipGetErrorString(le));
  return GTE_OK;
}

int gte_read_trade_stats(gte_env* E, int32_t first, int32_t count, gte_trade_stats* out) {
  return read_records(E, "gte_read_trade_stats", "gte_track_trades", E ? E->trades.stats : nullptr,
                      sizeof(gte_trade_stats), first, count, out);
}

int gte_bind_periods(gte_env* E, int32_t d, const int8_t* period_of_row) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  const Params& p = E->p;
  if (d < 0 || d >= p.D) return fail(GTE_ERR_INVALID, "dataset index %d out of range", d);
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bind_periods inside a stream capture");
  const int64_t T = E->h_ds[d].T;
  if (period_of_row && T <= 0) return fail(GTE_ERR_STATE, "gte_bind_periods: dataset %d was never uploaded", d);
  if (!period_of_row && !E->periods.d_row) return GTE_OK;  // nothing was ever bound
  HIPCHK(hipSetDevice(E->cfg.device));
  if (!E->periods.d_row) {
    E->periods.h_row.assign((size_t)p.D, gte::PeriodRow{nullptr, 0});
    E->periods.row_block = std::vector<DeviceBlock>((size_t)p.D);
    TRY(dev_alloc(E, &E->periods.d_row, (size_t)p.D));
  }
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight read the rows
  if (!period_of_row) {
    if (E->periods.h_row[d].base) TRY(publish_period_row(E, d, DeviceBlock()));
    return GTE_OK;
  }
  const size_t T16 = (size_t)round_up_16(T);
  DeviceBlock row;  // (released by every return but a successful publish)
  TRY(device_alloc(&row, T16, "period row of dataset %d: %s", d));
  hipError_t e = hipMemset(row.get(), 0xFF, T16);  // the padding: -1, a row of no period
  if (e == hipSuccess) e = hipMemcpy(row.get(), period_of_row, (size_t)T, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP, "period row of dataset %d: %s", d,
                hipGetErrorString(e));
  return publish_period_row(E, d, std::move(row));
}

int gte_track_periods(gte_env* E, int32_t n_periods, gte_period_stats** records_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  TRY(check_n_periods(n_periods, 0));
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_track_periods before gte_reset");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_track_periods inside a stream capture");
  if (n_periods > 0 && E->trades.on)
    return fail(GTE_ERR_STATE, "gte_track_periods: trade tracking is on, and trade and period records together are "
                "not implemented (gte_track_trades(env, 0, ...) first)");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));  // launches in flight write the records
  if (n_periods > 0 && n_periods != E->periods.alloc_B) {
    // (allocated, then the old records freed; cleared by the next backtest call: periods.changed)
    TRY(device_alloc(&E->periods.stats, sizeof(gte_period_stats) * (size_t)E->p.N * (size_t)n_periods,
                     "period records (%d envs x %d periods): %s", E->p.N, n_periods));
    E->periods.alloc_B = n_periods;
  }
  if (n_periods != E->periods.B) E->periods.changed = true;
  E->periods.B = n_periods;
  if (records_device) *records_device = E->periods.stats.as<gte_period_stats>();
  return GTE_OK;
}

int gte_read_period_stats(gte_env* E, int32_t first, int32_t count, gte_period_stats* out) {
  return read_records(E, "gte_read_period_stats", "gte_track_periods", E ? E->periods.stats.get() : nullptr,
                      E ? sizeof(gte_period_stats) * (size_t)E->periods.alloc_B : 0, first, count, out);
}

}  // extern "C"
