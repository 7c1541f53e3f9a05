/*
 * gte.h — C ABI of libgte: the MI355X (gfx950) batched trading-environment
 * hot path.
 *
 * The reference (ten2net/Gym-Trading-Env) is pure Python and has no FFI; the
 * boundary it exposes is the Python class API of
 * src/gym_trading_env/environments.py.  This header is the C ABI that sits
 * directly under that class API: each entry point names the reference method
 * (file:line) whose per-environment work it performs for a whole batch of
 * environments resident in HBM.  The Python host layer
 * (the Python files under gym-trading-env_amd/) binds these with ctypes;
 * INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in any signature
 *     (a hipStream_t travels as void*);
 *   - every function returns 0 on success or a negative gte_status; the
 *     message for the last failure on the calling thread is gte_last_error();
 *   - the library owns all state, dataset and (unless gte_bind_outputs is
 *     used) output buffers; pointers handed out stay valid until
 *     gte_destroy; the host never frees them;
 *   - all work is stream-ordered on the env's stream (gte_set_stream) and
 *     asynchronous: gte_step returns after the launch;
 *   - there is NO CPU fallback: every entry point that needs the device fails
 *     with GTE_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef GTE_H_
#define GTE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTE_ABI_VERSION 5
#define GTE_MAX_POSITIONS 32
#define GTE_MAX_DYN 4

typedef enum gte_status {
  GTE_OK = 0,
  GTE_ERR_INVALID = -1,    /* bad argument / config (message says which)     */
  GTE_ERR_NO_DEVICE = -2,  /* no usable HIP device: there is no CPU fallback */
  GTE_ERR_HIP = -3,        /* a HIP runtime call failed                      */
  GTE_ERR_STATE = -4,      /* call order (e.g. step before upload/reset)     */
  GTE_ERR_OOM = -5
} gte_status;

/* dynamic features computable on device
 * (environments.py:20-24 dynamic_feature_last_position_taken / _real_position) */
typedef enum gte_dyn_kind {
  GTE_DYN_LAST_POSITION = 0,
  GTE_DYN_REAL_POSITION = 1
} gte_dyn_kind;

/* rewards computable on device (environments.py:17-18 basic_reward_function;
 * the clipped / scaled forms are the fork's luckymodel/envs/env.py:16-18) */
typedef enum gte_reward_kind {
  GTE_REWARD_LOG_RETURN = 0,         /* ln(pv_t / pv_{t-1})                    */
  GTE_REWARD_SCALED_LOG_RETURN = 1,  /* reward_param0 * ln(pv_t / pv_{t-1})    */
  GTE_REWARD_CLIPPED_LOG_RETURN = 2  /* clip(param0*ln(..), param1, param2)    */
} gte_reward_kind;

/* what a finished environment does on later steps.  The reference env never
 * resets itself; Gymnasium's vector wrappers do
 * (docs/source/vectorize_env.rst:17-33). */
typedef enum gte_autoreset {
  GTE_AUTORESET_DISABLED = 0,  /* caller resets (gte_reset with a mask)        */
  GTE_AUTORESET_NEXT_STEP = 1, /* the step after a terminal one resets: it
                                  ignores the action and returns the reset obs,
                                  reward 0, flags false (Gymnasium >= 1.0)     */
  GTE_AUTORESET_SAME_STEP = 2  /* terminal step returns the reset obs; flags
                                  and reward are the terminal step's           */
} gte_autoreset;

/* gte_config.kernel_variant: bits that select a reference structure of the kernels, for A/B
 * timing and for the tests' twins.  Results never depend on them; 0 is the product. */
typedef enum gte_kernel_variant {
  GTE_KV_PER_WAVE_PHASE_A = 1,   /* every wave runs phase A for its own envs (default: wave 0
                                    runs it for the whole workgroup, cooperative phase A)    */
  GTE_KV_NO_LDS_STAGING = 2,     /* no LDS staging of the dynamic columns                    */
  GTE_KV_RETIRED_OVERLAPPED = 4, /* accepted, ignored: was the overlapped step kernel
                                    (measured slower, removed)                               */
  GTE_KV_SHARED_TU = 64,         /* launch the shared-TU instantiation of the hot kernel
                                    instead of the isolated one (gte_hot.hip)                */
  GTE_KV_ROLLOUT_PER_STEP = 128, /* gte_rollout runs as one launch per step even where the
                                    fused kernels apply                                      */
  GTE_KV_ROLLOUT_GATHER = 256,   /* gte_rollout uses the gather-per-step fused kernel instead
                                    of the window-resident one                               */
  GTE_KV_LOG_SEPARATE = 1024,    /* gte_step appends the trajectory row with a separate small
                                    launch (default: the step kernel writes it, through LDS)  */
  GTE_KV_LOG_FUSED = 2048,       /* accepted, means that default                             */
  GTE_KV_GENERIC_COPY = 4096,    /* always the generic copy loop (not the lean one that full
                                    waves of 16-byte-vector windows take)                    */
  GTE_KV_RECORD_DIRECT = 8192,   /* the lane that stepped an env stores its record itself
                                    (default: the record's per-step half goes through LDS and
                                    the copy waves write it, one 64-byte request per env)    */
  GTE_KV_DENSE_FLAGS = 16384     /* every step stores every env's terminated / truncated
                                    (default: only the flags that change)                    */
} gte_kernel_variant;

/* Constructor arguments of TradingEnv (environments.py:79-93) for a batch. */
typedef struct gte_config {
  int32_t abi_version;      /* = GTE_ABI_VERSION                               */
  int32_t struct_bytes;     /* = sizeof(gte_config)                            */
  int32_t device;           /* HIP device ordinal                              */
  int32_t n_envs;           /* N environments in this shard                    */
  int32_t n_datasets;       /* D resident datasets (1 for TradingEnv)          */
  int32_t n_static;         /* F_s: static feature columns (:130-133)          */
  int32_t n_dyn;            /* dynamic features (:135-138), <= GTE_MAX_DYN     */
  int32_t dyn_kind[GTE_MAX_DYN];
  int32_t window;           /* W = `windows`; 0 means windows=None (:156-160)  */
  int32_t n_positions;      /* P = len(positions) (:98)                        */
  double  positions[GTE_MAX_POSITIONS];
  double  trading_fees;            /* :102 */
  double  borrow_interest_rate;    /* :103 */
  double  portfolio_initial_value; /* :104 */
  int32_t initial_position_index;  /* index into positions, or -1 = 'random' (:167) */
  int32_t max_episode_duration;    /* 0 = 'max' (:173,:250)                    */
  int32_t reward_kind;
  int32_t autoreset;
  double  reward_param0;
  double  reward_param1;
  double  reward_param2;
  /* MultiDatasetTradingEnv (:365-400) */
  int32_t episodes_between_dataset_switch; /* >= 1                             */
  int32_t dyn_persist;      /* 1: keep a full T-deep dynamic-feature column per
                               env across episodes, exactly like the in-place
                               write into _obs_array (:153-154); 0: W-deep ring,
                               rows before the episode start read as zero      */
  uint64_t seed;            /* device Philox key for reset draws               */
  int64_t  env_id_base;     /* global id of env 0 of this shard (RNG streams
                               are keyed by global env id, so a sharded run
                               equals the unsharded one)                       */
  int32_t envs_per_wave;    /* 0 = choose automatically (so that all workgroups are
                               resident at once where possible), else 1..64       */
  int32_t nontemporal_obs;  /* observation store policy: 0 plain, 1 non-temporal, 2 sc1
                               (1 and 2 keep the feature table in L2; see
                               store_out in csrc/gte_kernels.hip), 3 = automatic:
                               sc1 while the observation buffer fits the Infinity
                               Cache (<= 190 MB), non-temporal beyond             */
  int32_t kernel_variant;   /* 0 = auto, else GTE_KV_* bits (above): reference
                               structures for A/B timing and the tests' twins */
  int32_t debug_flags;      /* timing ablations only (results become wrong):
                               1 = skip the observation gather, 2 = skip the
                               dynamic-column patch, 8 = skip the window loads
                               (stores only)                                      */
  int32_t affinity_period;  /* L2-affinity processing order: every this many steps the
                               envs are re-sorted by (dataset, table region) so that
                               each XCD's L2 serves one region (speed only; results
                               do not depend on it).  0 = default (max_episode_duration
                               / 16 within [8, 128]; 128 for 'max'), -1 = off        */
  int32_t log_steps;        /* L > 0: keep the last L steps of every env in a device
                               trajectory log (what History records each step,
                               environments.py:253-264); 0 = off                  */
  int32_t reserved2;
  int32_t final_obs;        /* 1 (needs autoreset = same-step): keep the terminal
                               observation of every env that ends, in
                               gte_outputs.final_obs (Gymnasium `final_observation`,
                               SB3 `terminal_observation`)                        */
  int32_t obs_slack_rows;   /* M: spare rows per env of a sliding observation buffer
                               (gte_bind_sliding_obs).  0 = automatic (2 * W / 5), -1 = off,
                               > 0 = explicit.  Only read by gte_obs_view().slack_rows: an env
                               slides only once such a buffer is bound                 */
} gte_config;

/* Device pointers of the per-step return values of TradingEnv.step
 * (environments.py:272) for the whole batch. */
typedef struct gte_outputs {
  float*   obs;        /* f32 [N, W, F_obs] (or [N, F_obs] when window == 0)   */
  float*   reward;     /* f32 [N]                                              */
  double*  reward64;   /* f64 [N]  (the value the f32 one was rounded from)    */
  uint8_t* terminated; /* u8  [N]  `done` (:246)                               */
  uint8_t* truncated;  /* u8  [N]  (:248-251)                                  */
  int32_t* term_count; /* i32 [2]  two slots used alternately (so that no clearing
                          launch sits between steps); term_count[term_slot] is
                          the number of envs whose flags are raised after the
                          last step                                            */
  int32_t* term_ids;   /* i32 [N]  their ids, compacted (order unspecified)    */
  int64_t  obs_elems_per_env; /* W*F_obs                                       */
  int32_t  term_slot;  /* which slot the last launch used (set by gte_get_outputs) */
  int32_t  reserved0;
  float*   final_obs;  /* f32 [N, W, F_obs] or NULL: row e holds the terminal observation
                          of env e after a step in which e ended (same-step mode with
                          gte_config.final_obs); other rows keep older contents     */
} gte_outputs;

/* Device pointers of the per-env state (struct of arrays), i.e. the fields of
 * TradingEnv/Portfolio that History logs each step (:253-264). */
typedef struct gte_state_view {
  int32_t* idx;            /* _idx (:235)                                      */
  int32_t* step;           /* _step (:236)                                     */
  int32_t* position_index; /* index of _position in positions (:210)           */
  int32_t* dataset_index;  /* resident dataset the env trades                  */
  int32_t* start_idx;      /* _idx at the last reset (for Market Return :281)  */
  int32_t* episode;        /* number of resets so far                          */
  int32_t* needs_reset;    /* 1 after a terminal step until the env is reset   */
  double*  asset;          /* Portfolio.asset (portfolio.py:3)                 */
  double*  fiat;           /* Portfolio.fiat                                   */
  double*  interest_asset; /* Portfolio.interest_asset                         */
  double*  interest_fiat;  /* Portfolio.interest_fiat                          */
  double*  portfolio_valuation; /* valorisation at the current row (:241)      */
  double*  real_position;  /* Portfolio.real_position at the current row (:259)*/
} gte_state_view;

typedef struct gte_env gte_env;

/* TradingEnv.__init__ (environments.py:79-125): validates the arguments and
 * allocates HBM for N envs and D datasets.  No data yet. */
int gte_create(const gte_config* cfg, gte_env** out);

/* TradingEnv._set_df (environments.py:128-143): uploads one staged dataset.
 * feat  : host f32 [T, F_obs] row-major, F_obs = n_static + n_dyn, the n_dyn
 *         trailing columns zero — exactly `_obs_array` (:141);
 * close : host f64 [T] — `_price_array` (:143);
 * high/low : host f64 [T] or NULL (only the limit-order path reads them, :221). */
int gte_upload_dataset(gte_env* env, int32_t ds, const float* feat,
                       const double* close, const double* high,
                       const double* low, int64_t T);

/* TradingEnv.reset (environments.py:163-199) for the envs with mask[i] != 0
 * (mask == NULL: all).  All pointers are HOST arrays of length N or NULL.
 * inj_idx / inj_pos_index / inj_dataset >= 0 replace the random draws of
 * :174, :167 and :385 (parity mode); NULL or negative entries use the device
 * Philox stream. */
int gte_reset(gte_env* env, const uint8_t* mask, const int32_t* inj_idx,
              const int32_t* inj_pos_index, const int32_t* inj_dataset);

/* Queue values for the draws of later auto-resets: host i32 [N, n_episodes]
 * arrays (or NULL) indexed by [env][k], k = 0 for the first auto-reset after
 * this call.  Consumed in order; when exhausted the Philox stream takes over. */
int gte_set_autoreset_injection(gte_env* env, int32_t n_episodes,
                                const int32_t* inj_idx,
                                const int32_t* inj_pos_index,
                                const int32_t* inj_dataset);

/* TradingEnv.step (environments.py:233-272) for all N envs in one launch:
 * _take_action/_trade (:204-215) -> Portfolio.trade_to_position
 * (portfolio.py:18-43) -> idx/step advance (:235-236) -> update_interest
 * (portfolio.py:44-46) -> valorisation (portfolio.py:7-13) -> done/truncated
 * (:244-251) -> reward (:17-18,:265-267) -> _get_obs (:152-160).
 * actions: i32 [N] position indices, -1 = None (hold, :234); a host pointer,
 * or a device pointer when actions_on_device != 0.
 * Stream capture: with device-resident actions everything the call enqueues can be captured into
 * a HIP graph by the owner of the env's stream (gte_set_stream).  The terminal counter alternates
 * between its two slots per launch: capture an EVEN number of steps and replay the graph only when
 * gte_get_outputs().term_slot equals its value at capture time (it does after any number of
 * replays and after an even number of eager steps).  With log_steps > 0 the log's row index is
 * device state (gte_log_view.cursor), so a replay appends its rows where the log is; the host's
 * count of them (gte_log_view.rows) advances during the capture as if the steps had run: save the
 * schedule before the capture, restore it afterwards (also after a failed capture) and advance
 * the count by the captured steps after each replay (gte_get_schedule below).  A graph re-sorts
 * the processing order (gte_config.affinity_period) where the capture did. */
int gte_step(gte_env* env, const int32_t* actions, int32_t actions_on_device);

/* The host-side schedule of an env, which a stream capture advances although it runs nothing.
 * gte_get_schedule saves it; gte_set_schedule puts a saved one back (only to undo the bookkeeping
 * of launches that never ran: a capture) and makes the next step store every flag; after each
 * replay of a graph that appended k log rows, gte_advance_log(env, k) keeps gte_log_view.rows
 * exact. */
typedef struct gte_schedule {
  int64_t log_rows;             /* gte_log_view.rows                                  */
  int32_t term_slot;            /* gte_outputs.term_slot                              */
  int32_t steps_since_rebuild;  /* steps since the processing order was last re-sorted */
} gte_schedule;
int gte_get_schedule(gte_env* env, gte_schedule* out);
int gte_set_schedule(gte_env* env, const gte_schedule* schedule);
int gte_advance_log(gte_env* env, int64_t rows);

/* TradingEnv.add_limit_order (environments.py:227-231) for every env with
 * pos_index[i] >= 0 (HOST arrays of length N; persistent == NULL means all
 * non-persistent).  A pending order fills in gte_step at the new row when
 * low <= limit <= high and its target differs from the current position, trading
 * at the limit price (:217-223); gte_reset clears an env's orders (:168).  Needs
 * high/low in every uploaded dataset.  A filled non-persistent order is removed
 * (the reference deletes it while iterating and raises RuntimeError). */
int gte_add_limit_orders(gte_env* env, const int32_t* pos_index, const double* limit,
                         const uint8_t* persistent);

/* Dynamic features the device does not compute (a user's Python callable evaluated vectorised
 * over the batch, environments.py:152-154 `_obs_array[_idx, F_s + i] = f(history)`): overwrite
 * feature i, for every bit i of `mask`, of the CURRENT row of every env with values_device
 * (DEVICE f32 [N, n_dyn]) — in the env's dynamic-feature store, from where the windows of later
 * steps read it, and in the observation the last gte_step / gte_reset produced.  Stream-ordered;
 * call it after every step and reset. */
int gte_set_dynamic_features(gte_env* env, const float* values_device, uint32_t mask);
/* The same from n_dyn separate DEVICE columns, columns_device[i] = f32 or f64 [N] (is_f64[i]) or
 * NULL to leave feature i alone: what a vectorised callable returns per feature, cast to f32 by
 * the kernel the way the reference's assignment into its f32 _obs_array casts (:153-154).
 * Both arrays are HOST arrays of n_dyn entries. */
int gte_set_dynamic_columns(gte_env* env, const void* const* columns_device, const int32_t* is_f64);

/* Device trajectory log (gte_config.log_steps = L): after every gte_reset / gte_step one row per
 * env is appended (by the step kernel itself, or by a small launch) — except by a masked gte_reset
 * once the log has a row, which rewrites the masked envs' slot of the newest row in place.  The log is ONE array of
 * 80-byte records [L, N] (the step kernel writes a row as two requests per env); the pointers
 * below address column c of row 0, env 0, and element (r, e) of a column lives `row_stride`
 * bytes per row and `env_stride` bytes per env further: p + (r % L) * row_stride + e *
 * env_stride.  `rows` counts the rows written so far (the newest is rows - 1).  An episode of
 * env e is the run of rows whose `step` goes 0, 1, 2, ... (step 0 = the reset row).  The same
 * count lives on the device, where launches read it: cursor[cursor_slot] equals `rows` once
 * everything enqueued so far has run (a launch that appends a row reads one slot and writes the
 * count + 1 to the other). */
typedef struct gte_log_view {
  int32_t* idx;             /* i32 [L, N] _idx  (strided, see above)               */
  int32_t* step;            /* i32 [L, N] _step                                   */
  int32_t* position_index;  /* i32 [L, N]                                         */
  int32_t* dataset_index;   /* i32 [L, N]                                         */
  double*  portfolio_valuation; /* f64 [L, N]                                     */
  double*  real_position;   /* f64 [L, N]                                         */
  double*  reward;          /* f64 [L, N]                                         */
  uint8_t* flags;           /* u8  [L, N] bit0 terminated, bit1 truncated         */
  int64_t  rows;            /* rows written since gte_create                      */
  int32_t  L;
  int32_t  N;
  double*  asset;           /* f64 [L, N] Portfolio.asset / fiat / interest_asset /  */
  double*  fiat;            /*   interest_fiat: what `portfolio_distribution_*`      */
  double*  interest_asset;  /*   derives from (portfolio.py:49-57, History columns   */
  double*  interest_fiat;   /*   environments.py:262)                                */
  int64_t  env_stride;      /* bytes from env e to env e + 1 of the same row          */
  int64_t  row_stride;      /* bytes from row r to row r + 1 of the same env          */
  int64_t* cursor;          /* i64 [2] DEVICE: the rows written, see above              */
  int32_t  cursor_slot;     /* the slot of `cursor` the last enqueued append wrote      */
  int32_t  reserved0;
} gte_log_view;
int gte_get_log(gte_env* env, gte_log_view* out);
/* the last `n` (<= L) rows of ONE env, oldest first, into host arrays of length n (any may
 * be NULL); returns the number of rows copied through *n_out */
int gte_read_log(gte_env* env, int32_t env_id, int32_t n, int32_t* idx, int32_t* step,
                 int32_t* position_index, int32_t* dataset_index, double* portfolio_valuation,
                 double* real_position, double* reward, uint8_t* flags, int32_t* n_out);
/* the Portfolio columns of the same rows (asset, fiat, interest_asset, interest_fiat) */
int gte_read_log_portfolio(gte_env* env, int32_t env_id, int32_t n, double* asset, double* fiat,
                           double* interest_asset, double* interest_fiat, int32_t* n_out);
/* The logged EPISODE of each of n_ids envs (HOST array env_ids) in ONE transfer: one kernel packs
 * them into pinned host memory, one stream synchronisation — what History holds for those envs
 * (environments.py:253-264; the reference's add_metric / get_metrics functions and save_for_render
 * read it, :274-307).  Episode of an env = the last run of its logged rows whose `step` counts up
 * by one to the newest row (cut at the front when longer than the log or than max_rows; max_rows
 * <= 0 means L).  With auto-reset disabled, a run of equal `step` > 0 rows at the end (the copies
 * a frozen env logs until it is reset) counts as its first row.  finished != 0 (same-step auto-reset with final_obs, right after the step in
 * which the envs ended): the episode that just FINISHED — the rows before the newest one (which
 * already is the next episode's reset row) plus the terminal row from the env's terminal record
 * with that step's reward.  The arrays are [n_ids, max_rows] row-major, rows 0 .. n_rows[j]-1 of
 * env j valid, oldest first; they live in library-owned host memory and stay valid until the next
 * gte_read_log_envs / gte_destroy. */
typedef struct gte_log_batch {
  int32_t n_ids, max_rows;
  const int32_t* n_rows;            /* i32 [n_ids] */
  const int32_t* idx;               /* i32 [n_ids, max_rows] */
  const int32_t* step;
  const int32_t* position_index;
  const int32_t* dataset_index;
  const double*  portfolio_valuation; /* f64 [n_ids, max_rows] */
  const double*  real_position;
  const double*  reward;
  const double*  asset;
  const double*  fiat;
  const double*  interest_asset;
  const double*  interest_fiat;
  const uint8_t* flags;             /* u8 [n_ids, max_rows] bit0 terminated, bit1 truncated */
} gte_log_batch;
int gte_read_log_envs(gte_env* env, const int32_t* env_ids, int32_t n_ids, int32_t max_rows,
                      int32_t finished, gte_log_batch* out);
/* Overwrite the `reward` column of the NEWEST log row with device values f64 [N] — what the
 * reference does with a custom reward_function: `historical_info["reward", -1] = reward`
 * (environments.py:265-267).  Stream-ordered. */
int gte_set_log_reward(gte_env* env, const double* reward_device);
/* A custom reward_function's values for the whole batch (DEVICE f64 [N]), with the reference's
 * rules around them applied by one kernel: reward 0 where the step terminated (environments.py
 * :265: the function is not called when done) and on rows a reset wrote (:196), then written to
 * the f32 and f64 return buffers and to the newest log row (:267).  terminal_view != 0 (same-step
 * auto-reset): an env that ended was shown its terminal row, so its reset row does not zero the
 * reward.  Needs log_steps > 0.  Stream-ordered. */
int gte_apply_reward(gte_env* env, const double* reward_device, int32_t terminal_view);

/* Per-step results of gte_rollout, all device pointers, all optional (NULL = not kept).
 * Row k holds what the k-th gte_step of the sequence would have produced. */
typedef struct gte_rollout_bufs {
  float* obs;           /* f32 [K][N][W][F_obs]; NULL: only the last step's observation is
                           produced, in the env's own obs buffer (gte_get_outputs) */
  float* reward;        /* f32 [K][N] */
  double* reward64;     /* f64 [K][N] */
  uint8_t* terminated;  /* u8  [K][N] */
  uint8_t* truncated;   /* u8  [K][N] */
  double* valuation;    /* f64 [K][N]: portfolio_valuation after each step (environments.py:241) */
} gte_rollout_bufs;

/* n_steps consecutive TradingEnv.step calls (environments.py:233-272) for action sequences
 * known in advance — `actions` is a DEVICE pointer to int32 [n_steps][N], -1 = hold — fused
 * into one launch (gte_rollout.hip).  State, auto-resets, injected draws, limit-order fills and
 * the results are exactly those of n_steps gte_step calls; afterwards the env's own reward /
 * flag buffers and terminal list describe the last step, and its obs buffer holds the last
 * observation unless bufs->obs was given (then that is row n_steps-1 of bufs->obs).  Shapes the
 * fused kernel does not cover (dyn_persist, final_obs, log_steps, scalar-vector layouts) run as
 * n_steps launches of the step kernel with the same results.  Per-step observation rows are
 * written with non-temporal stores under the automatic store policy (they are a stream).
 * Tuning only (results do not depend on it): the environment variable GTE_RESIDENT_EPB = 1..64
 * fixes the envs per workgroup pass of the window-resident kernel instead of the geometry
 * search in gte_api.hip (profiles/r02_resident_epb.log). */
int gte_rollout(gte_env* env, const int32_t* actions, int32_t n_steps, const gte_rollout_bufs* bufs);

/* Running statistics of ONE env's backtest (gte_backtest): one 128-byte record per env, owned by
 * the env on the device and carried from call to call.  An env's timeline is a sequence of
 * episodes: a reset row (valuation v_0, position value p_0), then transitions t = 1, 2, ... with
 * the valuation v_t the step computed (environments.py:241, before any same-step reset), the
 * position value p_t = positions[position_index] after the step (limit-order fills included), the
 * f64 reward r_t and the two flags.  A TRANSITION is a step in which the env really advanced: a
 * next-step auto-reset step and a frozen step (a finished env on its last row, auto-reset off) are
 * none and change no statistic.  A reset of any kind (next-step, same-step inside a launch,
 * gte_reset between calls) sets peak = v_0 and prev_position = p_0.  Per transition, in this
 * order, every floating operation one IEEE f64 operation as written:
 *   steps += 1;  reward_sum += r_t;  reward_sq_sum += r_t * r_t;
 *   if (p_t != prev_position) trades += 1;  prev_position = p_t;
 *   if (v_t > peak) peak = v_t;  d = 1.0 - v_t / peak;  if (d > max_drawdown) max_drawdown = d;
 *   cur_return += r_t;
 *   at the FIRST transition of an episode that raises a flag:  episodes += 1;
 *     terminations += terminated;  ep_return_sum += cur_return;
 *     ep_return_sq_sum += cur_return * cur_return;  cur_return = 0.0;
 *   valuation_last = v_t;
 * (plain comparisons: a NaN valuation changes neither peak nor max_drawdown).  Transitions an env
 * goes on making after its episode ended without a reset (auto-reset off, rows left) count like
 * any other and end no further episode.  Clearing zeroes the record, then takes peak =
 * valuation_last = the env's current portfolio_valuation and prev_position = its current position
 * value. */
typedef struct gte_backtest_stats {
  int64_t steps;             /* transitions                                             */
  double  reward_sum;        /* sum of r_t, in step order                               */
  double  reward_sq_sum;     /* sum of r_t * r_t                                        */
  double  peak;              /* highest valuation of the current episode                */
  double  max_drawdown;      /* largest 1 - v_t / peak seen in any episode              */
  double  cur_return;        /* sum of r_t of the episode in progress                   */
  double  ep_return_sum;     /* sum over finished episodes of their return              */
  double  ep_return_sq_sum;  /* ... and of its square                                   */
  double  valuation_last;    /* v_t of the last transition                              */
  double  prev_position;     /* p_t of the last transition (or p_0 of the last reset)   */
  int32_t trades;            /* transitions whose position value differs from the one before */
  int32_t episodes;          /* finished episodes                                       */
  int32_t terminations;      /* ... of them, ended by `terminated` (the 0.7 rule, :246) */
  int32_t ended;             /* bookkeeping: 1 while the current episode has ended and no reset followed */
  int32_t episode_seen;      /* bookkeeping: the env's reset count the statistics are up to date with   */
  int32_t step_seen;         /* bookkeeping: the env's _step after the last step folded in              */
  int32_t reserved[6];       /* -> 128 bytes                                            */
} gte_backtest_stats;

/* n_steps consecutive TradingEnv.step calls exactly like gte_rollout(actions, n_steps, NULL) — no
 * per-step result is kept — that also maintain every env's gte_backtest_stats.  `actions` is a
 * DEVICE pointer to int32 [n_steps][N].  clear != 0: the records are cleared first (see above);
 * clear == 0: they continue, so a long backtest can be fed in chunks of actions (an env that was
 * reset by gte_reset since the previous call restarts peak and prev_position and keeps its sums).
 * The first call of an env always clears.  *stats_device (may be NULL) receives the DEVICE address
 * of the N records, which stays the same until gte_destroy.  Where gte_rollout fuses the steps,
 * n_steps - 1 of them run in one launch with state and statistics in registers
 * (gte_backtest.hip) and the last one as an ordinary step launch folded in by a small kernel;
 * elsewhere every step is a step launch plus that fold, with the same records bit for bit.
 * Afterwards state, dynamic rings, return buffers, terminal list and observation are those of
 * n_steps gte_step calls.  The buffers are allocated by the first call.  Refused inside a stream
 * capture (GTE_ERR_STATE): a backtest is one launch already. */
int gte_backtest(gte_env* env, const int32_t* actions, int32_t n_steps, int32_t clear,
                 gte_backtest_stats** stats_device);
/* Records first .. first+count-1 into HOST memory: waits for the env's stream, one transfer. */
int gte_read_backtest_stats(gte_env* env, int32_t first, int32_t count, gte_backtest_stats* out);

/* ---- backtests from SIGNAL TABLES: the action of a step looked up on the device by the market row
 * the env stands on, not by the step number.  A table is int8 [n_strategies][T] per resident
 * dataset: entry (s, t) is the position index strategy s wants while the env is on row t of that
 * dataset.  In the reference's terms, for env e before every step (environments.py:233-235; the
 * trade happens at the close of row _idx, :213-215):
 *     a = signals[dataset_index][strategy[e]][env._idx]
 *     env.step(a if 0 <= a < n_positions else None)
 * Any value outside [0, n_positions) means hold (None, :234); nothing in a table is validated and
 * no table content can index out of `positions`.  Env e follows strategy strategy[e] — a DEVICE
 * int32 [N] array with values in [0, n_strategies), which the kernels do not check: values outside
 * that range are the caller's contract (they would read outside the table) — or, with
 * strategy == NULL, strategy (env_id_base + e) % n_strategies, so the shards of a sharded run
 * follow the strategies the unsharded run gives the same envs.
 *
 * gte_bind_signals borrows caller-owned DEVICE memory for dataset `ds` (nothing is copied, like
 * gte_bind_outputs): row s starts at signals_device + s * row_stride.  Required: signals_device
 * 16-byte aligned, row_stride % 16 == 0 and row_stride >= round_up(T_ds, 16) — so an aligned 16-byte
 * load anywhere in a row is legal, which is what the fused kernel issues —, n_strategies >= 1 and
 * equal to that of the tables bound to the other datasets (GTE_ERR_INVALID otherwise).  The dataset
 * must have been uploaded (GTE_ERR_STATE): its T is what is checked, and a later gte_upload_dataset
 * of `ds` unbinds its table.  signals_device == NULL unbinds.  The call waits for the env's stream
 * and is refused inside a stream capture (GTE_ERR_STATE).  The caller keeps the memory alive while
 * launches that read it are in flight. */
int gte_bind_signals(gte_env* env, int32_t ds, const int8_t* signals_device, int32_t n_strategies,
                     int64_t row_stride);
/* One small launch that writes to actions_device (DEVICE int32 [N]) the action the tables give
 * every env for its NEXT step, from its current record: the table value at the env's _idx and
 * dataset_index if it lies in [0, n_positions), else -1 (hold) — the argument of the next
 * TradingEnv.step (environments.py:233-234).  Stream-ordered and capturable: the building block of
 * the step-by-step path, and what a caller uses to drive gte_step closed-loop.  GTE_ERR_STATE
 * before gte_reset or while a resident dataset has no table bound.  While exit rules are bound
 * (gte_bind_exit_rules, below) the launch decides the exits as well and updates the exit states. */
int gte_signal_actions(gte_env* env, const int32_t* strategy_device, int32_t* actions_device);
/* gte_backtest with that lookup in place of `actions`: n_steps TradingEnv.step calls
 * (environments.py:233-272), each with the action its table gives the env on the row it stands on
 * BEFORE the step.  A next-step auto-reset step ignores its action; a same-step reset happens
 * inside the step and the next step looks up at the new _idx / dataset (:393-400).  Records, their
 * order and roundings, `clear`, the post-state (records, rings, return buffers, terminal list,
 * observation of n_steps single steps), frozen envs, limit-order fills and injected draws are
 * exactly gte_backtest's.  Where gte_rollout fuses, n_steps - 1 steps run in one launch that keeps
 * the aligned 16-byte piece of the strategy's row around _idx in registers (gte_backtest.hip) and
 * the last one as gte_signal_actions + a step launch + the fold; elsewhere every step is that
 * triple, with the same records bit for bit.  The lookup writes a library-owned int32 [N] buffer
 * allocated by the first call.  GTE_ERR_STATE while a resident dataset has no table bound, before
 * gte_reset and inside a stream capture.  While exit rules are bound (gte_bind_exit_rules, below) the fused
 * launch is gte_backtest_exit_kernel (gte_exits.hip) and the lookup the exit-aware one. */
int gte_backtest_signals(gte_env* env, const int32_t* strategy_device, int32_t n_steps, int32_t clear,
                         gte_backtest_stats** stats_device);

/* ---- EXIT RULES: stop-loss, trailing stop, take-profit and time exits per strategy.  A signal table
 * decides by MARKET ROW; an exit decides by the ENV'S OWN PATH (the valuation it entered at, its best
 * valuation since, the steps it has held), so the same table row gives different answers to envs that
 * entered at different valuations.  An exit rule only chooses the argument of TradingEnv.step
 * (environments.py:233-234); trading arithmetic is untouched.  This text is the specification; the
 * reference has no counterpart.
 *
 * RULE.  32 bytes, 4-byte aligned.  No rule content makes a kernel read or index outside anything. */
typedef struct gte_exit_rule {
  float   stop_loss, take_profit, trailing;   /* fractions; <= 0 or NaN: that exit is off          */
  int32_t max_hold;                           /* transitions; <= 0: off                            */
  int8_t  exit_position;                      /* position INDEX to go to; outside [0, P): rule off */
  int8_t  reserved0[3];
  int32_t reserved[3];                        /* ignored                                           */
} gte_exit_rule;
/* EXIT STATE of one env: 80 bytes, five 16-byte pieces, owned by the library on the device. */
typedef struct gte_exit_state {
  double  entry;          /* valuation the env had when it decided the trade it is in (or v_0)        */
  double  peak;           /* highest valuation since then                                             */
  double  v_seen;         /* bookkeeping: valuation and ...                                           */
  int32_t held;           /* transitions since the position last changed (0 on a reset row; saturates) */
  int32_t latched;        /* 1 after an exit fired, until the table byte moves or the env is reset    */
  int32_t latched_raw;    /* the table byte the latch waits to see change                             */
  int32_t i_seen;         /* ... position index of the row the state is up to date with               */
  int32_t episode_seen;   /* bookkeeping: the env's reset count and ...                               */
  int32_t step_seen;      /* ... _step of that row                                                    */
  int32_t decided;        /* 1: decided_action is the decision for (episode_seen, step_seen)          */
  int32_t decided_action; /* that decision: a position index or -1 (hold)                             */
  int32_t reserved[2];
  int32_t exits[4];       /* exits fired so far: STOP, TRAIL, TARGET, TIME                            */
} gte_exit_state;
#define GTE_EXIT_STOP 0
#define GTE_EXIT_TRAIL 1
#define GTE_EXIT_TARGET 2
#define GTE_EXIT_TIME 3
#ifdef __cplusplus
static_assert(sizeof(gte_exit_rule) == 32 && sizeof(gte_exit_state) == 80, "exit rule: 32 bytes; exit state: five 16-byte pieces");
#endif
/* TIMELINE.  It is the one of gte_backtest_stats: a reset row has valuation v_0 and position index
 * i_0; transitions t = 1, 2, ... follow with v_t and i_t, the index after the step, limit-order fills
 * included.  A next-step auto-reset step and a frozen step are not transitions: their action is hold
 * and they change no exit state (the reset row a next-step reset produces is a reset row).
 *
 * AT A RESET ROW of any kind:  entry = peak = v_0;  held = 0;  latched = 0.  The counters exits[] go on.
 *
 * BEFORE TRANSITION t+1 the env stands on row _idx with v_t, i_t and its rule R; P = n_positions:
 *
 *     raw = the sign-extended table byte at (dataset, strategy, _idx)
 *     if needs_reset:                      action = hold                      (nothing below runs)
 *     if latched and raw != latched_raw:   latched = 0                        (the signal moved: re-armed)
 *     if latched:                          action = hold
 *     elif 0 <= R.exit_position < P and i_t != R.exit_position and some exit holds:
 *         k = the first in the order STOP, TRAIL, TARGET, TIME that holds
 *         latched = 1;  latched_raw = raw;  exits[k] += 1;  action = R.exit_position
 *     else:                                action = raw if 0 <= raw < P else hold
 *
 *     STOP    stop_loss   > 0 and v_t <= entry * (1.0 - (double)stop_loss)
 *     TRAIL   trailing    > 0 and v_t <= peak  * (1.0 - (double)trailing)
 *     TARGET  take_profit > 0 and v_t >= entry * (1.0 + (double)take_profit)
 *     TIME    max_hold    > 0 and held >= max_hold
 *
 * Every floating operation is one IEEE f64 operation as written; the comparisons are plain, so a NaN
 * valuation trips nothing.
 *
 * AFTER TRANSITION t+1:
 *
 *     if i_{t+1} != i_t:  entry = peak = v_t;  held = 1        (any change of position, fills included)
 *     else:               held += 1                            (saturating at INT32_MAX)
 *     if v_{t+1} > peak:  peak = v_{t+1}
 *
 * entry is the valuation the env had when it DECIDED the trade, so the trade's own fees count against
 * it.  A transition into a same-step reset is followed at once by that reset row, which overwrites all
 * the transition wrote.  An env that goes on stepping after its episode ended (auto-reset off, rows
 * left) keeps making transitions and, having needs_reset, keeps getting hold.
 *
 * STEP-BY-STEP PATH.  gte_signal_actions with rules bound first brings the state up to date from the
 * env record (episode, _step, pv, pos), then decides:
 *     decided and episode == episode_seen and _step == step_seen:  return decided_action, change nothing
 *       (a second call before the env has stepped: the call stays safe to repeat and to capture);
 *     episode != episode_seen:   a reset row with v_0 = pv;
 *     else _step != step_seen:   ONE transition from (v_seen, i_seen) to (pv, pos) over d = _step -
 *       step_seen steps: held = d where the position changed, else held += d (saturating);
 *     then (v_seen, i_seen, episode_seen, step_seen) = (pv, pos, episode, _step), the decision above, and
 *     decided = 1, decided_action = action (for an env with needs_reset too: hold).
 * The fused kernel keeps the same state in registers and runs the same update after every step; where the row
 * it starts on already has its decision (a gte_signal_actions call before it), its first step takes that memo
 * and decides nothing.  So both paths give the same records, env state and exit state bit for bit.
 *
 * RULE OF ENV e: rule_of_env[e] if that array was given — DEVICE int32 [N] with values in
 * [0, n_rules), the caller's contract like `strategy` — else strategy_of(e) % n_rules, strategy_of(e)
 * being what the lookup uses (strategy[e], or (env_id_base + e) % n_strategies).
 *
 * gte_bind_exit_rules borrows caller-owned DEVICE memory like gte_bind_signals (nothing is copied; the
 * caller keeps it alive while launches that read it are in flight); rules_device == NULL unbinds, and
 * gte_signal_actions / gte_backtest_signals then launch exactly the kernels they launch without this
 * feature.  The state is allocated by the first call; EVERY call re-initialises it (all zero,
 * episode_seen = -1), so the next decision sees a reset row.  *state_device (may be NULL) receives the
 * DEVICE address of the N states (NULL before one exists), which stays the same until gte_destroy.  The call
 * waits for the env's stream and is refused inside a stream capture (GTE_ERR_STATE).  GTE_ERR_INVALID
 * for rules_device or rule_of_env_device not 4-byte aligned and for n_rules < 1. */
int gte_bind_exit_rules(gte_env* env, const gte_exit_rule* rules_device, int32_t n_rules,
                        const int32_t* rule_of_env_device, gte_exit_state** state_device);
/* States first .. first+count-1 into HOST memory: waits for the env's stream, one transfer.
 * GTE_ERR_STATE before the first gte_bind_exit_rules. */
int gte_read_exit_state(gte_env* env, int32_t first, int32_t count, gte_exit_state* out);

/* ---- TRADE STATISTICS: round-trip figures per env (closed trades, wins and losses, gross profit and loss,
 * best and worst trade, holding time, time in the market, losing streaks), kept next to gte_backtest_stats
 * while a backtest steps.  Opt-in (gte_track_trades); with tracking off every call launches exactly the
 * kernels it launches without this feature.  This text is the specification; the reference has no counterpart.
 *
 * TIMELINE.  It is the one of gte_backtest_stats: reset rows (v_0, p_0) and transitions with v_t, the
 * position VALUE p_t after the step (fills included) and the step's flags; what is and what is not a
 * transition is stated there.  A TRADE is a maximal run of transitions of one episode with one constant
 * non-zero position value.
 *
 * PER TRANSITION.  `ended` below is the `ended` of the env's gte_backtest_stats BEFORE the transition (the
 * trade record has no bookkeeping fields of its own): a transition of an episode that has already ended
 * changes nothing.  Otherwise, every floating operation one IEEE f64 operation as written, comparisons plain:
 *
 *     if (p_t != open_position) {
 *         if (open_position != 0.0) {
 *             if (p_t == 0.0) close(v_t);                      left to flat: v_t is v_{t-1} less the fees of leaving
 *             else { close(last_valuation); reversals += 1; }  reversal / resize: the flip's fees count against the new trade
 *         }
 *         open_position = p_t;  open_value = last_valuation;  open_len = 0;
 *     }
 *     if (open_position != 0.0) { open_len += 1;  exposure += 1; }
 *     if (flags != 0 && open_position != 0.0) { close(v_t);  forced += 1;  open_position = 0.0; }
 *     last_valuation = v_t;
 *
 *     close(vc):  ret = vc / open_value - 1.0;  closed += 1;  hold_sum += open_len;
 *                 if (open_len > max_len) max_len = open_len;
 *                 if (ret > 0.0)      { wins += 1;  gross_profit += ret;  ret_sq_sum += ret * ret;  loss_streak = 0; }
 *                 else if (ret < 0.0) { losses += 1;  gross_loss += ret;  ret_sq_sum += ret * ret;  loss_streak += 1;
 *                                       if (loss_streak > max_loss_streak) max_loss_streak = loss_streak; }
 *                 if (ret > best_trade) best_trade = ret;  if (ret < worst_trade) worst_trade = ret;
 *
 * A zero or NaN ret counts in `closed` only and touches neither a sum nor the streak; an infinite ret is a
 * value like any other.  open_value is the valuation the trade was DECIDED at (like gte_exit_state.entry), so
 * the fees of entering count against the trade.
 *
 * AT A RESET ROW of any kind (next-step, same-step inside a launch, gte_reset between calls):
 *     if (open_position != 0.0) dropped += 1;      only a gte_reset in mid-episode: an episode's end closed its trade
 *     open_position = p_0;  open_value = last_valuation = v_0;  open_len = 0;        loss_streak carries on
 *
 * CLEARING: all fields zero, best_trade = -inf, worst_trade = +inf, open_position = the env's current position
 * value, open_value = last_valuation = its current portfolio_valuation.
 *
 * The record is defined by valuations, not rewards: it does not depend on the reward kind, and every f64
 * field is a function of state the kernels reproduce by value.
 *
 * THE TRADE LIST (gte_track_trade_list; opt-in on top of gte_track_trades): one 48-byte gte_trade per closed
 * trade next to the sums, list[N][capacity] env-major, owned by the env on the device.  ROWS: for a transition t,
 * row_t and ds_t are the market row (_idx) and the dataset the env stood on BEFORE the step; after the
 * transition it stands on row_t + 1; row_0 is the row a reset row put it on.  The env keeps one more value,
 * open_row (one int32 per env, owned by the library; NOT a field of gte_trade_stats, whose reserved words stay
 * zero), and the text above gains:
 *
 *     where it sets  open_value = last_valuation   (a position change), also   open_row = row_t;
 *     AT A RESET ROW of any kind, also            open_row = row_0;
 *     CLEARING, also                              open_row = the row the env stands on;
 *     close(vc) FIRST writes, if closed < capacity,
 *         list[e][closed] = { open_value, vc, open_position, open_row, exit_row, open_len, ds_t, kind, flags_t }
 *       and then does what it does above, with
 *         kind 0  left to flat:         exit_row = row_t       the order executes at that row's price
 *         kind 1  reversal / resize:    exit_row = row_t
 *         kind 2  forced by the end:    exit_row = row_t + 1   the trade is marked at the row the episode ended on
 *
 * So exit_row - entry_row == hold for every record, and a reversal on the terminal step writes two records,
 * kind 1 and then kind 2 with hold == 1.  The list keeps the FIRST `capacity` trades of an env since the last
 * clearing while `closed` goes on counting: min(closed, capacity) records are valid, closed > capacity means
 * truncated.  The list has no counter of its own and is never zeroed.  A trade's return is
 * close_value / open_value - 1.0, one f64 division and one subtraction: the ret of close() bit for bit. */
typedef struct gte_trade_stats {     /* 128 bytes, eight 16-byte pieces */
  double  open_value;       /* valuation the open trade was decided at                      */
  double  open_position;    /* position value of the open trade; 0.0: none open             */
  double  last_valuation;   /* valuation of the last row folded in, reset rows included     */
  double  gross_profit;     /* sum of ret over closes with ret > 0, in close order          */
  double  gross_loss;       /* sum of ret over closes with ret < 0  (<= 0)                  */
  double  ret_sq_sum;       /* sum of ret * ret over those same closes                      */
  double  best_trade;       /* largest ret  (-inf while none)                               */
  double  worst_trade;      /* smallest ret (+inf while none)                               */
  int64_t exposure;         /* transitions spent inside a trade                             */
  int64_t hold_sum;         /* sum of open_len over closed trades                           */
  int32_t closed, wins, losses, forced, reversals, dropped;
  int32_t open_len, max_len, loss_streak, max_loss_streak;
  int32_t reserved[2];      /* written as zero                                              */
} gte_trade_stats;
#ifdef __cplusplus
static_assert(sizeof(gte_trade_stats) == 128, "trade statistics: eight 16-byte pieces");
#endif
/* One record of the trade list (THE TRADE LIST, in the text above) */
typedef struct gte_trade {           /* 48 bytes, three 16-byte pieces */
  double  open_value;   /* valuation the trade was decided at (the record's open_value) */
  double  close_value;  /* the vc of close(vc)                                          */
  double  position;     /* position value held                                          */
  int32_t entry_row, exit_row;   /* market rows (_idx)                                  */
  int32_t hold;         /* open_len at the close                                        */
  int32_t dataset;      /* ds_t of the transition that closed it                        */
  int32_t kind;         /* 0 left to flat, 1 reversal / resize, 2 forced by the episode's end */
  int32_t flags;        /* flags of the transition that closed it (bit0 terminated, bit1 truncated) */
} gte_trade;
#ifdef __cplusplus
static_assert(sizeof(gte_trade) == 48, "trade list record: three 16-byte pieces");
#endif
#define GTE_MAX_TRADE_LIST (1 << 20)
/* on != 0: gte_backtest and gte_backtest_signals maintain BOTH records of every env from now on — with or
 * without exit rules bound, on the fused path (gte_trades.hip: the from-registers kernels with the trade
 * record in registers as well) and on the step-by-step path, in all three auto-reset modes — and the
 * gte_backtest_stats records, the env state and the exit state come out bit for bit as with tracking off.
 * on == 0: tracking stops, and the trade list (gte_track_trade_list) is turned off with it; the trade records keep
 * what they hold.  The FIRST backtest call after a change of
 * `on` clears both records whatever its `clear` says, so the two records always cover the same transitions.
 * The N trade records are allocated by the first call with on != 0; *records_device (may be NULL) receives
 * their DEVICE address (NULL before they exist), which stays the same until gte_destroy.  The call waits for
 * the env's stream and is refused before gte_reset and inside a stream capture (GTE_ERR_STATE). */
int gte_track_trades(gte_env* env, int32_t on, gte_trade_stats** records_device);
/* Trade records first .. first+count-1 into HOST memory: waits for the env's stream, one transfer.
 * GTE_ERR_STATE before the first gte_track_trades(env, 1, ...). */
int gte_read_trade_stats(gte_env* env, int32_t first, int32_t count, gte_trade_stats* out);
/* The trade list (the text above).  capacity in 1 .. GTE_MAX_TRADE_LIST: from now on the backtest calls write
 * every closed trade of an env into list[e][closed] as well, through the kernels of gte_trade_list.hip — the
 * kernels of gte_trades.hip with the list, on the fused and on the step-by-step path, in all three auto-reset
 * modes — and both records, the env state and the exit state come out bit for bit as with gte_track_trades
 * alone.  capacity == 0 turns the list off; gte_track_trades(env, 0, ...) turns it off too.  With the list off
 * every call launches exactly the kernels it launches without this feature.  The call allocates N * capacity *
 * 48 bytes on the first call and on a change of capacity (GTE_ERR_OOM on failure, with everything left as it
 * was; the old list is freed: an address an earlier call returned is dead from then on).  Turning the list off
 * frees it as well.  Any change — on, off, another capacity — makes the FIRST backtest call after it clear the
 * records whatever its `clear` says, like a switch of gte_track_trades; until that call the list holds nothing
 * (its memory is fresh and `closed` still counts the trades of before), so gte_read_trade_list and
 * gte_pack_trade_list are refused (GTE_ERR_STATE).  *list_device (may be NULL) receives the DEVICE address of
 * the list (NULL while it is off).  The call waits for the env's stream; it is refused unless trade tracking is on, before gte_reset
 * and inside a stream capture (GTE_ERR_STATE); GTE_ERR_INVALID for a capacity outside [0, GTE_MAX_TRADE_LIST]. */
int gte_track_trade_list(gte_env* env, int32_t capacity, gte_trade** list_device);
/* What gte_read_trade_list leaves: the valid records of the requested envs as ONE dense block, in request
 * order.  The trades of request j are trades[first[j] .. first[j+1]), min(closed[j], capacity) of them, in close
 * order; closed[j] is the env's `closed` (closed[j] > capacity: the list of that env is truncated). */
typedef struct gte_trade_batch {
  int32_t n_ids;            /* requests                                                  */
  int32_t capacity;         /* of the list as it stands                                  */
  int64_t n_trades;         /* records in `trades` == first[n_ids]                       */
  const int64_t* first;     /* [n_ids + 1]                                               */
  const int32_t* closed;    /* [n_ids]                                                   */
  const gte_trade* trades;  /* [n_trades]                                                */
} gte_trade_batch;
/* env_ids: HOST int32 [n_ids], in any order, repeats allowed; NULL: all envs 0 .. N-1 (n_ids is then ignored).
 * On the device a count-and-scan kernel computes first[] from min(closed, capacity) and a pack kernel copies each
 * requested env's valid records into the block, one wavefront per request in 16-byte pieces; then one read of the
 * total and one transfer.  `out` points into library-owned HOST memory, valid until the next call or
 * gte_destroy.  Waits for the env's stream.  GTE_ERR_STATE while the list is off, and between a switch of tracking,
 * of the list or of its capacity and the backtest call that clears the records; GTE_ERR_INVALID for an id
 * outside [0, N) and for n_ids < 0. */
int gte_read_trade_list(gte_env* env, const int32_t* env_ids, int32_t n_ids, gte_trade_batch* out);
/* The same pack with caller-provided DEVICE memory, enqueued on the env's stream without waiting:
 * env_ids_device int32 [n_ids] (NULL: all envs, n_ids is then ignored), first_device int64 [n_ids + 1],
 * closed_device int32 [n_ids], trades_device gte_trade [max_trades], 16-byte aligned.  Records that would lie at
 * or past max_trades are not written; first_device[n_ids] still holds the full total, so a caller may run the
 * call with trades_device == NULL and max_trades == 0 first, read the total, and size the block for a second
 * call.  An id outside [0, N) — the host cannot see it — gives an empty list with closed[j] == -1.
 * GTE_ERR_STATE as gte_read_trade_list; GTE_ERR_INVALID for misaligned or missing pointers. */
int gte_pack_trade_list(gte_env* env, const int32_t* env_ids_device, int32_t n_ids, int64_t* first_device,
                        int32_t* closed_device, gte_trade* trades_device, int64_t max_trades);

/* ---- PERIOD STATISTICS: the sums and counters of gte_backtest_stats split by MARKET PERIOD.  Every market row
 * carries a small period id (a calendar month, a walk-forward fold, train / embargo / test), and every backtest
 * path keeps one 32-byte record per (env, period), reduced while it steps: out-of-sample checks, period by
 * period returns and the [S, B] matrix everything further starts from, without per-step rows.  Opt-in
 * (gte_track_periods); with tracking off every call launches exactly the kernels it launches without this
 * feature.  This text is the specification; the reference has no counterpart.
 *
 * RECORDS.  gte_period_stats[N][B], env-major (record of env e and period b at e * B + b), owned by the env on
 * the device.  PERIOD ROWS.  One int8 row per resident dataset: period_of_row[d][i] is the period of market row i
 * of dataset d (gte_bind_periods).
 *
 * TIMELINE.  It is the one of gte_backtest_stats: the same transitions, the same r_t, position values p_t and
 * flags; what is and what is not a transition is stated there.  PER TRANSITION of env e, run directly before that
 * record's own update, so `prev_position` and `ended` below are the fields of the env's gte_backtest_stats
 * BEFORE the transition:
 *
 *     i = the row the env stood on before the step, d its dataset then
 *         (the row whose signal byte gte_backtest_signals looks up; after the step it is _idx - 1 of the env's
 *          record, or of its terminal record when the step reset it in same-step mode)
 *     b = period_of_row[d][i];   if (!(0 <= b && b < B)) nothing;      an embargo row, a warm-up row
 *     R = records[e][b]:
 *       R.steps += 1;  R.reward_sum += r_t;  R.reward_sq_sum += r_t * r_t;
 *       if (p_t != prev_position) R.trades += 1;
 *       if (flags != 0 && !ended) R.episodes += 1;
 *
 * Every floating operation is one IEEE f64 operation as written.  Each sum is the plain left-to-right sum over
 * that (env, period)'s transitions in step order since the last clear, whatever the launches, chunks and paths in
 * between: a kernel that keeps the open period's record in registers continues from the stored value when the
 * env enters a period.  A reset row changes no record.  No table byte can index outside the records.
 *
 * IDENTITIES.  With every row of every dataset in period 0 and B = 1, records[e][0].steps / reward_sum /
 * reward_sq_sum / trades / episodes are bit for bit the fields of env e's gte_backtest_stats.  With every row in
 * some period, the sums over b of steps, trades and episodes equal that record's counters exactly.
 *
 * CLEARING: all 32 bytes zero. */
#define GTE_MAX_PERIODS 128
typedef struct gte_period_stats {   /* 32 bytes, two 16-byte pieces */
  double  reward_sum;      /* sum of r_t over the period's transitions, in step order */
  double  reward_sq_sum;   /* sum of r_t * r_t                                         */
  int64_t steps;           /* transitions                                              */
  int32_t trades;          /* of them, those gte_backtest_stats.trades counts          */
  int32_t episodes;        /* of them, those gte_backtest_stats.episodes counts        */
} gte_period_stats;
#ifdef __cplusplus
static_assert(sizeof(gte_period_stats) == 32, "period statistics: two 16-byte pieces");
#endif
/* The period row of dataset ds: period_of_row is HOST int8 [T_ds], T_ds the rows of the dataset as uploaded.
 * Unlike gte_bind_signals the call COPIES (it is T bytes) into a library-owned device row padded to
 * round_up(T, 16) with -1, so an aligned 16-byte load anywhere in it is legal.  NULL unbinds; gte_upload_dataset
 * of ds unbinds too (T may have changed).  A bind, a re-bind or an unbind makes the first backtest call after it
 * clear the records like a change of tracking.  Waits for the env's stream; refused inside a stream capture and
 * for a dataset that was never uploaded (GTE_ERR_STATE); GTE_ERR_INVALID for ds outside [0, n_datasets). */
int gte_bind_periods(gte_env* env, int32_t ds, const int8_t* period_of_row);
/* n_periods in 1 .. GTE_MAX_PERIODS: gte_backtest and gte_backtest_signals maintain the period records from now
 * on, with B = n_periods — with or without exit rules bound, on the fused path (gte_periods.hip: the
 * from-registers kernels with the open period's record in registers) and on the step-by-step path, in all three
 * auto-reset modes — and the gte_backtest_stats records, the env state and the exit state come out bit for bit
 * as with tracking off.  n_periods == 0: tracking stops; the records keep what they hold.  The call allocates
 * N * B * 32 bytes (GTE_ERR_OOM on failure, with tracking left as it was) and allocates afresh when B changes
 * (the old records are freed: an address an earlier call returned is dead from then on, and so is every view
 * of it a caller kept).  The FIRST backtest call after a change — on, off, another B, a (re-)bind —
 * clears both kinds of record whatever its `clear` says, so they always cover the same transitions.  While
 * tracking is on, a backtest with a resident dataset that has no period row bound is refused (GTE_ERR_STATE).
 * Period tracking and trade tracking together are not implemented: whichever of gte_track_periods and
 * gte_track_trades would turn the second one on is refused (GTE_ERR_STATE).  *records_device (may be NULL)
 * receives the DEVICE address of the records (NULL before they exist).  The call waits for the env's stream and
 * is refused before gte_reset and inside a stream capture (GTE_ERR_STATE); GTE_ERR_INVALID for n_periods
 * outside [0, GTE_MAX_PERIODS]. */
int gte_track_periods(gte_env* env, int32_t n_periods, gte_period_stats** records_device);
/* The count * B records of envs first .. first+count-1 into HOST memory: waits for the env's stream, one
 * transfer.  B is that of the records as they stand, the n_periods of the last gte_track_periods(env, B >= 1,
 * ...): out holds count * B records of it, not of an earlier B.  GTE_ERR_STATE before the first such call. */
int gte_read_period_stats(gte_env* env, int32_t first, int32_t count, gte_period_stats* out);

/* ---- CURVES: a backtest that also keeps ROWS — the equity curve, the underwater curve and what goes with them,
 * one row per `stride` steps and env, written by the launch that holds the step in registers.  This text is the
 * specification; tests/curve_model.py states it as a per-env loop.
 *
 * A step of an env is one of three kinds (struct gte_backtest_stats, above): a TRANSITION (the env advanced:
 * TradingEnv.step, environments.py:233-272); a RESET ROW (next-step auto-reset: the env was reset instead of
 * stepping, TradingEnv.reset, :163-199); a FROZEN step (no auto-reset, the episode has ended and
 * _step did not move).  In same-step mode a transition that ends an episode is followed by a reset inside the
 * same step.
 *
 * WINDOW j of a call covers its steps j * stride .. min((j + 1) * stride, n_steps) - 1; the last window of a call
 * may be shorter, and no window reaches into the next call.  Row j of a column is at column[j * N + e], R =
 * ceil(n_steps / stride) rows; rows at and beyond R are not touched.  Every column is optional: a NULL pointer
 * means that column is not kept and costs nothing.
 *   valuation  Valuation of the window's LAST step.  Transition: the valuation v_t the statistics fold for it (in
 *              same-step mode at an episode end that is the terminal record's, not the new episode's).  Reset row:
 *              the new episode's start valuation.  Frozen: the env's valuation as it stands.
 *   position   Position INDEX that belongs to that valuation: the terminal one at a same-step episode end, the
 *              reset position on a reset row.
 *   row        Market row that valuation was taken at.  Transition: the row the env stood on before the step + 1.
 *              Reset row: the row the env landed on.  Frozen: unchanged.
 *   reward     m = 0.0; then m = m + r_t for every transition of the window, t ascending: one IEEE f64 addition
 *              each, starting from +0.0 — so a window whose only reward is -0.0 holds +0.0.
 *   drawdown   m = 0.0; for every transition of the window d = 1.0 - v_t / peak', where peak' is the record's
 *              running peak after `if (v_t > peak) peak = v_t` — the d of gte_backtest_stats —, then
 *              if (d > m) m = d.  A window without a transition holds 0.0; a NaN never enters (plain comparison,
 *              as in max_drawdown).
 *   flags      OR over the window's steps of the GTE_CURVE_* bits below; TERMINATED and TRUNCATED are the flags of
 *              its transitions.
 * The record's peak restarts at resets and is carried from call to call with clear == 0, as it is today: after a
 * call with clear != 0 the maximum of an env's drawdown column IS its max_drawdown, and at stride 1 adding its
 * reward column in row order gives its reward_sum, both to the bit. */
#define GTE_CURVE_TERMINATED 1 /* a transition of the window raised `terminated`                              */
#define GTE_CURVE_TRUNCATED 2  /* ... `truncated`                                                             */
#define GTE_CURVE_RESET 4      /* a reset happened in a step of the window: a next-step reset row, or the
                                  reset after a same-step episode end                                         */
#define GTE_CURVE_FROZEN 8     /* a step of the window was frozen                                             */
typedef struct gte_curve_bufs {
  double  *valuation, *drawdown, *reward; /* DEVICE f64 [R][N] each, 8-byte aligned, or NULL */
  int32_t *position, *row;                /* DEVICE i32 [R][N], 4-byte aligned, or NULL      */
  uint8_t *flags;                         /* DEVICE u8  [R][N], or NULL                      */
} gte_curve_bufs;
/* n_steps TradingEnv.step calls (environments.py:233-272) exactly like gte_backtest (actions != NULL: DEVICE int32
 * [n_steps][N]) or gte_backtest_signals (actions == NULL: the bound signal tables, and the exit rules while they
 * are bound; strategy_device as there, ignored with actions) — the same records bit for bit, `clear`, post-state,
 * *stats_device — that also write the rows above into bufs.  Where gte_rollout fuses, n_steps - 1 steps run in
 * one launch of gte_curves.hip (the from-registers kernels with a tracker that stores a row whenever a window
 * closes) and the last one as a step launch folded in by gte_curve_fold_kernel, which also closes the call's last
 * window; a window open where the two meet travels in a library-owned 32-byte scratch per env.  Elsewhere every
 * step is a step launch plus that fold.  The rows do not depend on the path.  Without this call every other call
 * launches the kernels it launched before.
 * Refused, with nothing launched and nothing written: GTE_ERR_INVALID for bufs == NULL or all six columns NULL,
 * stride < 1, n_steps < 1, a column not aligned to its element; GTE_ERR_STATE while trade tracking (the trade
 * list included) or period tracking is on — one tracker per launch, as trades and periods exclude each other —,
 * inside a stream capture, before gte_reset, and with actions == NULL while a resident dataset has no signal
 * table bound (as gte_backtest_signals).  The caller keeps the columns alive until the env's stream has run the
 * call. */
int gte_backtest_curves(gte_env* env, const int32_t* actions, const int32_t* strategy_device, int32_t n_steps,
                        int32_t stride, int32_t clear, const gte_curve_bufs* bufs, gte_backtest_stats** stats_device);

/* ---- SIGNAL TABLES BUILT ON THE DEVICE from indicator rules: a parameter sweep passes a small bank of
 * indicators and one 32-byte rule per strategy, and the device writes the int8 [n_rules][T] table that
 * gte_bind_signals accepts — no host table, no host-to-device copy of it.
 *
 * An INDICATOR BANK of a dataset is caller-owned DEVICE memory float [n_indicators][ind_stride]: row c
 * is indicator c over the dataset's rows t = 0 .. T-1 (an SMA, an EMA, an RSI, a feature column, a
 * constant: the library does not care).  A RULE compares one indicator, or the difference of two,
 * with two thresholds, optionally with a latch (hysteresis: enter above hi, leave below lo, keep the
 * state in between).  This text is the specification; the reference has no counterpart. */
typedef struct gte_signal_rule {
  int32_t a, b;          /* indicator rows; b == -1: compare a alone            */
  float   hi, lo;        /* thresholds on d                                     */
  int32_t warmup;        /* rows t < warmup: output -1 (hold), state untouched  */
  int8_t  pos_up, pos_down, pos_neutral;   /* table bytes written, not validated */
  uint8_t latch;         /* non-zero: keep the last non-zero zone               */
  int32_t reserved[2];   /* ignored                                             */
} gte_signal_rule;
/* Row s of the table is built from rule s for t = 0 .. T-1 in order, with state q = 0 before row 0
 * (x = the bank):
 *
 *     if t < warmup: out[t] = -1; continue              (q unchanged)
 *     d = x[a][t] - x[b][t]   (one IEEE f32 subtraction, subnormals kept)   or   x[a][t] when b == -1
 *     z = +1 if d > hi, else -1 if d < lo, else 0       (NaN anywhere gives 0; hi < lo: "up" wins)
 *     q = z if (z != 0 or not latch) else q
 *     out[t] = pos_up if q > 0, pos_down if q < 0, else pos_neutral
 *
 * A rule with a outside [0, n_indicators) or b outside [-1, n_indicators) gives a row of -1: no rule
 * content makes the kernel read outside the bank.  Bytes T .. round_up(T, 16) - 1 of every row are -1;
 * bytes of a row beyond round_up(T, 16), and everything outside rows 0 .. n_rules - 1, are not
 * touched.  What the bytes mean (hold outside [0, n_positions)) stays with the lookup.
 *
 * T is that of resident dataset `ds` (GTE_ERR_STATE if it was never uploaded).  The launch is ordered
 * on the env's stream and binds nothing: pass the table to gte_bind_signals afterwards (which waits
 * for the stream).  Refused inside a stream capture (GTE_ERR_STATE), like gte_bind_signals.
 * GTE_ERR_INVALID, with nothing launched, unless: table_device and indicators_device are 16-byte
 * aligned and rules_device 4-byte aligned; row_stride % 16 == 0 and row_stride >= round_up(T, 16)
 * (bytes); ind_stride % 4 == 0 and ind_stride >= round_up(T, 16) (floats), so that a 16-byte load
 * anywhere in the 16 rows of a piece is legal; n_indicators >= 1 and n_rules >= 1.  One wavefront
 * builds one row in pieces of 1 024 rows (gte_signals.hip); rules that read the same indicator rows
 * are best placed next to each other. */
int gte_build_signals(gte_env* env, int32_t ds,
                      const float* indicators_device, int32_t n_indicators, int64_t ind_stride,
                      const gte_signal_rule* rules_device, int32_t n_rules,
                      int8_t* table_device, int64_t row_stride);

/* ---- SIGNAL TABLES COMPOSED ON THE DEVICE from clause rows and a truth table: a gte_signal_rule is one
 * comparison; a strategy is usually several ("long while SMA(fast) > SMA(slow) AND RSI < 70", "enter on
 * a breakout, leave on a slower condition", "two of three filters agree").  A CLAUSE TABLE of a dataset
 * is caller-owned DEVICE memory int8 [n_clause_rows][clause_stride] of ZONE CODES 0 / 1 / 2 — what
 * gte_build_signals writes with pos_down / pos_neutral / pos_up = 0 / 1 / 2 — and one 128-byte spec per
 * strategy names up to four clause rows and gives the table byte for each of the 3^4 code tuples, or
 * KEEP: the state stays what it was.  The device writes the int8 [n_specs][T] table that
 * gte_bind_signals accepts.  This text is the specification; the reference has no counterpart. */
#define GTE_COMPOSE_KEEP (-128)
typedef struct gte_signal_compose {   /* 128 bytes, 4-byte aligned */
  int32_t in[4];        /* clause rows read; only in[0 .. n_in-1] are looked at        */
  int8_t  n_in;         /* 1 .. 4                                                      */
  int8_t  initial;      /* the state q before row 0 (a table byte, not validated)      */
  int8_t  pos_invalid;  /* byte written where some input is no code                    */
  int8_t  reserved0;    /* ignored                                                     */
  int8_t  lut[81];      /* entry c0 + 3 c1 + 9 c2 + 27 c3; a table byte, or KEEP       */
  int8_t  reserved[27]; /* ignored                                                     */
} gte_signal_compose;
/* Row s of the table is composed from spec s for t = 0 .. T-1 in order, with state q = initial before
 * row 0 (clauses = the clause table):
 *
 *     c_k = clauses[in[k]][t] for k < n_in;  c_k = 0 for k >= n_in
 *     if any c_k (k < n_in) is outside {0, 1, 2}:   out[t] = pos_invalid; continue     (q unchanged)
 *     e = lut[c_0 + 3 c_1 + 9 c_2 + 27 c_3]
 *     if e != GTE_COMPOSE_KEEP:  q = e
 *     out[t] = q
 *
 * So a clause's warm-up byte (-1), or any stray byte, makes the composed row pos_invalid there and leaves
 * the state alone; KEEP is what makes asymmetric entry / exit expressible; initial == KEEP is written as
 * the byte -128 until an entry decides.  A spec with n_in outside [1, 4], or with an in[k], k < n_in,
 * outside [0, n_clause_rows), gives a row of -1 and reads nothing: no spec content makes the kernel read
 * outside the clause table.  Bytes T .. round_up(T, 16) - 1 of every row are -1; bytes of a row beyond
 * round_up(T, 16), and everything outside rows 0 .. n_specs - 1, are not touched.  Output bytes are not
 * validated: what they mean (hold outside [0, n_positions)) stays with the lookup.  Because 0 / 1 / 2
 * are codes, a composed table is a legal clause table for a second call: trees deeper than four inputs.
 *
 * T is that of resident dataset `ds` (GTE_ERR_STATE if it was never uploaded).  The launch is ordered
 * on the env's stream and binds nothing: pass the table to gte_bind_signals afterwards (which waits
 * for the stream).  Refused inside a stream capture (GTE_ERR_STATE).  GTE_ERR_INVALID, with nothing
 * launched, unless: clauses_device and table_device are 16-byte aligned and specs_device 4-byte aligned;
 * clause_stride and row_stride (bytes) are multiples of 16 and >= round_up(T, 16), so that a 16-byte
 * load or store anywhere in the 16 bytes of a piece is legal; n_clause_rows >= 1 and n_specs >= 1; the
 * bytes read (rows 0 .. n_clause_rows - 1, round_up(T, 16) bytes of each) and the bytes written are
 * disjoint.  One wavefront composes one row in pieces of 1 024 bytes (gte_compose.hip); specs that read
 * the same clause rows are best placed next to each other. */
int gte_compose_signals(gte_env* env, int32_t ds,
                        const int8_t* clauses_device, int32_t n_clause_rows, int64_t clause_stride,
                        const gte_signal_compose* specs_device, int32_t n_specs,
                        int8_t* table_device, int64_t row_stride);

/* ---- INDICATOR BANKS BUILT ON THE DEVICE from the resident market data: the bank gte_build_signals
 * reads is itself written by the device, one row per 16-byte spec, in the layout gte_build_signals
 * reads in place — a sweep is specs, then rules, then table, then statistics, with no host array
 * larger than the specs and the rules.  This text is the specification; the reference has no
 * counterpart. */
enum gte_indicator_kind {
  GTE_IND_VALUE = 0, GTE_IND_SMA = 1, GTE_IND_STD = 2, GTE_IND_ZSCORE = 3, GTE_IND_MAX = 4,
  GTE_IND_MIN = 5, GTE_IND_DIFF = 6, GTE_IND_ROC = 7, GTE_IND_EMA = 8, GTE_IND_RSI = 9
};
enum gte_indicator_source {
  GTE_SRC_CLOSE = 0, GTE_SRC_HIGH = 1, GTE_SRC_LOW = 2, GTE_SRC_FEATURE = 3, GTE_SRC_INPUT = 4
};
#define GTE_IND_MAX_WINDOW 4096
typedef struct gte_indicator_spec {   /* 16 bytes */
  int32_t kind;     /* GTE_IND_* above                                              */
  int32_t source;   /* GTE_SRC_CLOSE 0, _HIGH 1, _LOW 2, _FEATURE 3, _INPUT 4       */
  int32_t column;   /* _FEATURE: static feature column; _INPUT: row of the input bank; else ignored */
  int32_t n;        /* window / span, 1 .. GTE_IND_MAX_WINDOW (4096); ignored by VALUE */
} gte_indicator_spec;
/* SOURCE SERIES.  x[t], t = 0 .. T-1, is the source converted to f64 (exact): the dataset's close /
 * high / low (f64); column `column` of its feature table (f32, stride F_obs, static columns
 * [0, F_obs - n_dyn) only); or row `column` of a caller-owned f32 input bank
 * float [n_inputs][input_stride] with the alignment and stride rules of the output, which must not
 * overlap the output — volume or any series the env does not hold, and chaining: the signal line of a
 * MACD is an EMA over a bank that an earlier call wrote.
 *
 * ARITHMETIC.  All of it is f64, each operation below rounded once, in the written order, with no
 * contraction; the result is rounded once to f32 at the store.  "NaN" is a quiet NaN of unspecified
 * payload.  Subnormals are kept.  Row s of the bank is y[t] of spec s:
 *
 *   kind      NaN for     y[t] otherwise
 *   VALUE     -           x[t]
 *   SMA       t < n-1     s = 0; for k = 0..n-1: s += x[t-n+1+k]; y = s / n               (oldest first)
 *   STD       t < n-1     m = the SMA above; q = 0; for k: d = x[t-n+1+k] - m; q += d*d; y = sqrt(q / n)
 *   ZSCORE    t < n-1     (x[t] - m) / sd, m and sd as above          (IEEE gives NaN for a flat window)
 *   MAX, MIN  t < n-1     NaN if any window value is NaN; otherwise m = x[t-n+1]; for later k:
 *                         if (v > m) m = v   (< for MIN).  Of equal values the oldest stays, which fixes
 *                         the sign of a zero.
 *   DIFF      t < n       x[t] - x[t-n]
 *   ROC       t < n       x[t] / x[t-n] - 1
 *   EMA       -           a = 2.0 / (n + 1.0); y[0] = x[0]; y[t] = y[t-1] + a * (x[t] - y[t-1])
 *                         (sub, mul, add).  Warm-up is the rule's `warmup`.
 *   RSI       t < n       (Wilder) change c[j] = x[j] - x[j-1], gain g = c > 0 ? c : 0, loss
 *                         l = c < 0 ? -c : 0; a NaN change counts as neither.  At t = n:
 *                         au = (sum of g[j], j = 1..n) / n, ad likewise, sums from 0 in order.  For
 *                         t > n: au = (au*(n-1) + g[t]) / n, ad likewise.  y = 100 - 100 / (1 + au / ad).
 *
 * INVALID SPECS.  A spec whose kind is unknown, whose n is outside [1, 4096] (VALUE excepted), whose
 * source is unknown, that asks for high / low of a dataset without them, or whose column is out of
 * range gives a row of NaN and reads nothing: no spec content makes the kernel read outside its
 * sources.  A window longer than T is legal: every row is NaN.
 *
 * PADDING.  Floats T .. round_up(T, 16) - 1 of every row are written 0 (the padding of a host-made
 * bank); nothing beyond that and nothing outside rows 0 .. n_specs - 1 is touched.
 *
 * T is that of resident dataset `ds` (GTE_ERR_STATE if it was never uploaded).  The launch is ordered
 * on the env's stream; refused inside a stream capture (GTE_ERR_STATE).  GTE_ERR_INVALID, with nothing
 * launched, unless: bank_device and input_device are 16-byte aligned and specs_device 4-byte aligned;
 * ind_stride and (with an input) input_stride are multiples of 4 floats and >= round_up(T, 16);
 * n_specs >= 1; n_inputs >= 0 and input_device non-NULL exactly when n_inputs > 0 (NULL, 0, 0: none);
 * the input and the output ranges are disjoint.  One wavefront builds one row in pieces of 256 rows
 * (gte_indicators.hip). */
int gte_build_indicators(gte_env* env, int32_t ds,
                         const gte_indicator_spec* specs_device, int32_t n_specs,
                         const float* input_device, int32_t n_inputs, int64_t input_stride, /* NULL, 0, 0: none */
                         float* bank_device, int64_t ind_stride);

/* ---- STRATEGY STATISTICS AND RANKING ON THE DEVICE: the N env records of a backtest folded into one
 * record per strategy, and the best k strategies by a stated score — the last stage of a sweep (specs,
 * rules, table, statistics, leaders) with no record copied to the host.  This text is the
 * specification; the reference has no counterpart.
 *
 * MEMBERS.  Strategy s, 0 <= s < n_strategies = S, has an ordered list of member envs:
 *   - group_offsets_device == group_envs_device == NULL, the library's map (the one gte_backtest_signals
 *     uses with strategy == NULL): e = ((s - env_id_base) mod S) + j * S for j = 0, 1, ... while e < N;
 *   - both non-NULL, a CSR list of DEVICE int32 arrays: group_offsets[S + 1] non-decreasing with
 *     0 <= offsets[s] <= offsets[S] <= N, and the members of s are group_envs[offsets[s] ..
 *     offsets[s + 1]) in that order.  An entry outside [0, N) holds its place in the list (see the sums)
 *     and is otherwise skipped: no list content makes the kernel read outside the records.  (Offsets are
 *     clamped into [0, N] and made non-decreasing before use.)
 * Member number j = 0, 1, ... of a list is x_j below; a skipped entry contributes to nothing.
 *
 * THE RECORD of strategy s over its members:
 *   steps, trades, episodes, terminations   exact 64-bit sums of the members' counters;
 *   envs            members that are not skipped;      envs_stepped   those of them with steps > 0;
 *   max_drawdown    m = 0.0; in member order: if (x > m) m = x;
 *   best_reward_sum   m = -inf; over the members with steps > 0, in member order: if (x > m) m = x;
 *   worst_reward_sum  m = +inf; likewise with  if (x < m) m = x
 *                   (plain comparisons: a NaN never wins, of equal values the first stays);
 *   reward_sum, reward_sq_sum, ep_return_sum, ep_return_sq_sum   f64 sums in ONE FIXED ORDER that
 *     depends on nothing but the member list: eight interleaved accumulators a_0 .. a_7, each starting
 *     from 0.0; a_i adds x_i, x_(i+8), x_(i+16), ... one after the other (a skipped entry adds nothing);
 *     the sum is ((((((a_0 + a_1) + a_2) + a_3) + a_4) + a_5) + a_6) + a_7.  Every + is one IEEE f64
 *     addition; the result is the same bit for bit for any launch geometry and either kernel.
 *     A NaN that a sum produces is a quiet NaN of unspecified payload.
 * A strategy without members gets zero sums and counters, max_drawdown 0.0, best -inf, worst +inf.
 * reserved is written as zero. */
typedef struct gte_strategy_stats {     /* 128 bytes, eight 16-byte pieces like gte_backtest_stats */
  int64_t steps;
  double  reward_sum, reward_sq_sum, ep_return_sum, ep_return_sq_sum;   /* sums over the members  */
  double  max_drawdown;                 /* largest member max_drawdown                            */
  double  best_reward_sum, worst_reward_sum;  /* over members with steps > 0                      */
  int64_t trades, episodes, terminations;     /* 64-bit: member counters are int32, sums are not   */
  int32_t envs, envs_stepped;           /* members; members with steps > 0                        */
  int32_t reserved[8];                  /* written as zero                                        */
} gte_strategy_stats;
/* records_device == NULL: the env's own N records (GTE_ERR_STATE before the first gte_backtest /
 * gte_backtest_signals); else a caller-owned DEVICE array of N gte_backtest_stats, 16-byte aligned —
 * records saved from earlier chunks or other runs.  out_device: DEVICE array of S records, 16-byte
 * aligned, all 128 bytes of each written.  One launch, ordered on the env's stream, no host
 * synchronisation; changes neither the env's records nor its state.  GTE_ERR_INVALID, with nothing
 * launched, for n_strategies < 1, a NULL or misaligned out_device, misaligned records, or exactly one
 * of the two group pointers NULL.  Refused inside a stream capture (GTE_ERR_STATE). */
int gte_reduce_backtest_stats(gte_env* env, const gte_backtest_stats* records_device,
                              int32_t n_strategies, const int32_t* group_offsets_device,
                              const int32_t* group_envs_device, gte_strategy_stats* out_device);

/* The score a strategy is ranked by, from its gte_strategy_stats; every operation one IEEE f64 operation
 * as written (an int64 converts to f64 first), sqrt correctly rounded:
 *   MEAN_REWARD          m = reward_sum / steps
 *   SHARPE               q = reward_sq_sum / steps;  v = q - m * m;  if (!(v > 0.0)) v = 0.0;  m / sqrt(v)
 *                        (mean / population standard deviation of the pooled step rewards; NaN when
 *                        both are 0, +-inf for a constant non-zero reward)
 *   MEAN_EPISODE_RETURN  ep_return_sum / episodes
 *   EPISODE_SHARPE       the SHARPE formulas over ep_return_sum, ep_return_sq_sum and episodes
 *   NEG_MAX_DRAWDOWN     -max_drawdown
 *   WORST_REWARD_SUM     worst_reward_sum */
typedef enum gte_strategy_metric {
  GTE_METRIC_MEAN_REWARD = 0,
  GTE_METRIC_SHARPE = 1,
  GTE_METRIC_MEAN_EPISODE_RETURN = 2,
  GTE_METRIC_EPISODE_SHARPE = 3,
  GTE_METRIC_NEG_MAX_DRAWDOWN = 4,
  GTE_METRIC_WORST_REWARD_SUM = 5
} gte_strategy_metric;
#define GTE_RANK_MAX 256
/* The k best of S strategies.  Strategy s is RANKED iff steps >= 1, episodes >= min_episodes and its
 * score is not NaN.  Ranked strategies are ordered by score, highest first (+-inf like any value;
 * -0.0 == 0.0, by comparison); equal scores by strategy index, lowest first.  top_index_device
 * (int32 [k]) and top_score_device (f64 [k]) receive the first k of that order; places beyond the
 * number of ranked strategies hold -1 and NaN.  1 <= k <= GTE_RANK_MAX; k may exceed S.
 * scores_device (f64 [S]) or NULL: every strategy's score as computed, ranked or not, NaN included.
 * stats_device: DEVICE array of S records, 16-byte aligned.  A score launch and a few selection launches
 * (the best 256 of every 1 024 candidates, repeated until one workgroup holds them all), ordered on the
 * env's stream, no host synchronisation; the candidate lists are library-owned scratch, allocated by
 * the first call (and again only when S grows: to at least twice the old size, and the old lists are freed
 * by gte_destroy, not before — launches in flight may read them — so an env ranked over ever larger S holds
 * up to about twice what its largest S needs).  GTE_ERR_INVALID, with nothing launched, for
 * n_strategies < 1, k outside [1, GTE_RANK_MAX], an unknown metric, a NULL or misaligned stats_device
 * (16 bytes), top_index_device (4), top_score_device (8) or a misaligned scores_device (8).  Refused
 * inside a stream capture (GTE_ERR_STATE). */
int gte_rank_strategies(gte_env* env, const gte_strategy_stats* stats_device, int32_t n_strategies,
                        int32_t metric, int64_t min_episodes, int32_t k,
                        int32_t* top_index_device, double* top_score_device,
                        double* scores_device /* [n_strategies] or NULL */);

/* ---- TRADE STATISTICS PER STRATEGY, AND THEIR RANKING: the N gte_trade_stats folded into one record per
 * strategy and the best k by a per-trade score, as above for gte_backtest_stats.  MEMBERS, the skipping rule
 * and the ONE FIXED ORDER of the f64 sums (eight interleaved accumulators) are those of
 * gte_reduce_backtest_stats.  THE RECORD of strategy s over its members:
 *   closed, wins, losses, forced, reversals, exposure, hold_sum   exact 64-bit sums of the members' counters;
 *   gross_profit, gross_loss, ret_sq_sum   f64 sums in the fixed order;
 *   best_trade    m = -inf; in member order: if (x > m) m = x;     worst_trade   m = +inf; if (x < m) m = x
 *                 (plain comparisons, of equal values the first stays; a member without a closed trade holds
 *                 -inf / +inf and never wins);
 *   max_len, max_loss_streak   the largest of the members';
 *   envs          members that are not skipped;      envs_traded   those of them with closed > 0.
 * A strategy without members gets zero sums and counters, best -inf, worst +inf.  reserved is written as zero.
 * The bits are the same for either launch geometry. */
typedef struct gte_strategy_trade_stats {     /* 128 bytes, eight 16-byte pieces */
  int64_t closed, wins, losses, forced, reversals, exposure, hold_sum;
  double  gross_profit, gross_loss, ret_sq_sum;
  double  best_trade, worst_trade;
  int32_t max_len, max_loss_streak, envs, envs_traded;
  int32_t reserved[4];
} gte_strategy_trade_stats;
#ifdef __cplusplus
static_assert(sizeof(gte_strategy_trade_stats) == 128, "strategy trade statistics: eight 16-byte pieces");
#endif
/* records_device == NULL: the env's own N trade records (GTE_ERR_STATE before gte_track_trades allocated
 * them); else a caller-owned DEVICE array of N gte_trade_stats, 16-byte aligned.  out_device, the group lists,
 * the launch (one, on the env's stream, no host synchronisation) and the error codes are those of
 * gte_reduce_backtest_stats. */
int gte_reduce_trade_stats(gte_env* env, const gte_trade_stats* records_device, int32_t n_strategies,
                           const int32_t* group_offsets_device, const int32_t* group_envs_device,
                           gte_strategy_trade_stats* out_device);
/* The score a strategy is ranked by, from its gte_strategy_trade_stats; every operation one IEEE f64
 * operation as written (an int64 converts to f64 first), sqrt correctly rounded:
 *   WIN_RATE             wins / closed
 *   PROFIT_FACTOR        gross_profit / (0.0 - gross_loss)
 *   EXPECTANCY           (gross_profit + gross_loss) / closed
 *   TRADE_SHARPE         the SHARPE formulas of gte_strategy_metric over gross_profit + gross_loss, ret_sq_sum
 *                        and closed:  m = (gross_profit + gross_loss) / closed;  q = ret_sq_sum / closed;
 *                        v = q - m * m;  if (!(v > 0.0)) v = 0.0;  m / sqrt(v)
 *   WORST_TRADE          worst_trade
 *   NEG_MAX_LOSS_STREAK  -(double)max_loss_streak */
typedef enum gte_trade_metric {
  GTE_TRADE_METRIC_WIN_RATE = 0,
  GTE_TRADE_METRIC_PROFIT_FACTOR = 1,
  GTE_TRADE_METRIC_EXPECTANCY = 2,
  GTE_TRADE_METRIC_TRADE_SHARPE = 3,
  GTE_TRADE_METRIC_WORST_TRADE = 4,
  GTE_TRADE_METRIC_NEG_MAX_LOSS_STREAK = 5
} gte_trade_metric;
/* gte_rank_strategies over trade records: strategy s is RANKED iff closed >= max(1, min_trades) and its score
 * is not NaN.  One score launch, then the selection launches of gte_rank_strategies on the same library-owned
 * scratch; order, ties, NaN, padding (-1 / NaN), k (1 <= k <= GTE_RANK_MAX, may exceed S), scores_device,
 * alignments and error codes are those of gte_rank_strategies. */
int gte_rank_trade_stats(gte_env* env, const gte_strategy_trade_stats* stats_device, int32_t n_strategies,
                         int32_t metric, int64_t min_trades, int32_t k, int32_t* top_index_device,
                         double* top_score_device, double* scores_device /* [n_strategies] or NULL */);

/* ---- PERIOD STATISTICS PER STRATEGY, AND THEIR RANKING OVER A SET OF PERIODS: the N * B gte_period_stats
 * folded into one record per (strategy, period), gte_strategy_period_stats[S][B] strategy-major, and the best k
 * strategies by a score taken over any subset of the periods — rank on the training periods, read the same
 * strategies on the test periods.  MEMBERS, the skipping rule and the ONE FIXED ORDER of the f64 sums (eight
 * interleaved accumulators over the member list, closed as ((a0 + a1) + a2) ...) are those of
 * gte_reduce_backtest_stats, applied per (strategy, period): the same records give the same bits for any launch
 * geometry.  THE RECORD of strategy s and period b over the members' records [e][b]:
 *   reward_sum, reward_sq_sum   f64 sums in the fixed order;
 *   steps, trades, episodes     exact 64-bit sums of the members' counters;
 *   envs_stepped                members that are not skipped and have steps > 0 in period b.
 * A strategy without members gets zeros.  reserved is written as zero. */
typedef struct gte_strategy_period_stats {     /* 48 bytes, three 16-byte pieces */
  double  reward_sum, reward_sq_sum;
  int64_t steps, trades, episodes;
  int32_t envs_stepped;
  int32_t reserved;
} gte_strategy_period_stats;
#ifdef __cplusplus
static_assert(sizeof(gte_strategy_period_stats) == 48, "strategy period statistics: three 16-byte pieces");
#endif
/* records_device == NULL: the env's own N * B records, n_periods being their B (GTE_ERR_STATE before
 * gte_track_periods allocated them, GTE_ERR_INVALID for another n_periods); else a caller-owned DEVICE array of
 * N * n_periods gte_period_stats, 16-byte aligned.  1 <= n_periods <= GTE_MAX_PERIODS.  out_device: DEVICE array
 * of S * n_periods records, 16-byte aligned, all 48 bytes of each written.  The group lists, the launch (one, on
 * the env's stream, no host synchronisation) and the other error codes are those of gte_reduce_backtest_stats.
 * One thread per (strategy, period), the threads of a strategy neighbours across its periods and 256 / B
 * strategies per 256-thread workgroup; they walk the member list together, one member after the other, so a
 * member's B records are one contiguous read. */
int gte_reduce_period_stats(gte_env* env, const gte_period_stats* records_device, int32_t n_periods,
                            int32_t n_strategies, const int32_t* group_offsets_device,
                            const int32_t* group_envs_device, gte_strategy_period_stats* out_device);
/* The score a strategy is ranked by, from its B gte_strategy_period_stats and a set of periods.  P is the set of
 * periods b < B whose bit is set in period_mask (bit b % 64 of word b / 64), in ascending order.  Every operation
 * is one IEEE f64 operation as written (an int64 converts to f64 first), sqrt correctly rounded, comparisons
 * plain:
 *     n  = the sum over P of steps (int64);
 *     s1 = 0.0; s2 = 0.0; over P: s1 = s1 + reward_sum_b;  s2 = s2 + reward_sq_sum_b;
 *     over the periods of P with steps_b > 0, x_b = reward_sum_b:
 *       c = their number;  t1 = 0.0; t2 = 0.0;  t1 = t1 + x_b;  t2 = t2 + x_b * x_b;
 *       lo = +inf;  if (x_b < lo) lo = x_b;      up = the number of them with x_b > 0.0
 *   MEAN_REWARD     s1 / n
 *   SHARPE          the GTE_METRIC_SHARPE formulas on s1, s2, n:  m = s1 / n;  q = s2 / n;  v = q - m * m;
 *                   if (!(v > 0.0)) v = 0.0;  m / sqrt(v)
 *   REWARD_SUM      s1
 *   PERIOD_SHARPE   the same formulas on t1, t2, c: mean / population deviation of the period returns
 *   WORST_PERIOD    lo, and NaN when c == 0
 *   POSITIVE_SHARE  up / c
 * A selection without a stepped period scores NaN under every metric but REWARD_SUM (0.0) and is not ranked
 * under any. */
typedef enum gte_period_metric {
  GTE_PERIOD_METRIC_MEAN_REWARD = 0,
  GTE_PERIOD_METRIC_SHARPE = 1,
  GTE_PERIOD_METRIC_REWARD_SUM = 2,
  GTE_PERIOD_METRIC_PERIOD_SHARPE = 3,
  GTE_PERIOD_METRIC_WORST_PERIOD = 4,
  GTE_PERIOD_METRIC_POSITIVE_SHARE = 5
} gte_period_metric;
/* gte_rank_strategies over period records: strategy s is RANKED iff n >= max(1, min_steps) and its score is not
 * NaN.  period_mask: HOST uint64 [2].  One score launch, then the selection launches of gte_rank_strategies on
 * the same library-owned scratch; order, ties, NaN, padding (-1 / NaN), k (1 <= k <= GTE_RANK_MAX, may exceed
 * S), scores_device, alignments and error codes are those of gte_rank_strategies; GTE_ERR_INVALID also for
 * n_periods outside [1, GTE_MAX_PERIODS] and a NULL period_mask. */
int gte_rank_period_stats(gte_env* env, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                          int32_t n_periods, const uint64_t period_mask[2], int32_t metric, int64_t min_steps,
                          int32_t k, int32_t* top_index_device, double* top_score_device,
                          double* scores_device /* [n_strategies] or NULL */);

/* ---- BOOTSTRAP REALITY CHECK OF A LEADERBOARD (White 2000): is the best of S strategies better than what luck
 * alone gives the best of S tries?  A bootstrap over time blocks of the MAXIMUM over all strategies of their
 * centred mean period return, from the [S, B] gte_strategy_period_stats on the device.  The [R, S] matrix of
 * resampled statistics is never written.  One fixed order of IEEE f64 operations, every one of them ONE operation
 * as written (no fused multiply-add): the same inputs give the same bits for any launch geometry.
 *
 * RESAMPLING WEIGHTS, gte_bootstrap_weights.  weights[r * n + i] (f64) is how many times position i of the n
 * selected periods is drawn in resample r; each row sums to n.  The stationary bootstrap (Politis & Romano 1994)
 * on the circular sequence 0 .. n-1 with mean block length `block`:
 *     thr = (uint32) min(floor(4294967296.0 / block), 4294967295.0)                       (host, once)
 *     draw j = 0 .. n-1 of resample r:
 *       o = philox4x32_10(counter = {r, j, 0, 0x424F4F54 'BOOT'}, key = {seed low word, seed high word})
 *       a new block starts iff j == 0 or block == 1.0 or o[0] < thr:    pos = mulhi32(o[1], n)
 *       otherwise:                                                       pos = (pos + 1) % n
 *       weights[r][pos] += 1.0
 * One thread per resample, one launch on the env's stream, no host synchronisation.  Writes the n_resamples * n
 * doubles of weights_device and nothing else.
 *
 * THE RESAMPLE PASS AND THE CLOSE, gte_reality_check.  P = p_0 < ... < p_{n-1}, the periods whose bit is set in
 * period_mask (bit b % 64 of word b / 64; HOST uint64 [2]).  weights_device: DEVICE f64 [n_resamples * n], made
 * by gte_bootstrap_weights or by the caller — any finite weights, zeros and non-integers included (a jackknife,
 * a circular block scheme).  benchmark_device: DEVICE f64 [n_periods] (buy-and-hold's period returns) or NULL.
 * Strategy s is ELIGIBLE iff for every b in P steps_b > 0 and reward_sum_b is finite; of a record only steps
 * and reward_sum are read, and only for b in P.  Per eligible strategy:
 *     d_i = reward_sum[s][p_i] - benchmark[p_i]            (no subtraction at all without a benchmark)
 *     t = 0.0; over i ascending: t = t + d_i;              mean_s = t / (double)n
 *     resample r:  a = 0.0; over i ascending: a = a + weights[r][i] * d_i;      c_rs = a / (double)n - mean_s
 * WRITTEN (all of every array, R = n_resamples):
 *     mean[s]          mean_s; NaN for an ineligible strategy
 *     max_stat[r]      m = -inf; over eligible s ascending: if (c_rs > m) m = c_rs        (a NaN never wins)
 *     max_index[r]     the s that set m last, the lowest that attains the maximum; -1 when none compared greater
 *     boot_sum[s], boot_sq_sum[s], count_ge[s]    resamples cut into slabs of GTE_BOOT_SLAB; within a slab
 *                      q1 = 0.0; q2 = 0.0; over r ascending: q1 = q1 + c_rs; q2 = q2 + c_rs * c_rs;
 *                      ge += (c_rs >= mean_s);  then from 0.0 the slabs' q1, q2, ge added in ascending slab order.
 *                      NaN, NaN, 0 for an ineligible strategy
 *     count_adj[s]     the number of r with max_stat[r] >= mean_s; 0 for an ineligible strategy
 *     summary          best: m = -inf; over eligible s ascending: if (mean_s > m) { m = mean_s; best = s; }, -1
 *                      when none compared greater; best_mean = mean[best] (NaN for best == -1);
 *                      count_rc = count_adj[best] (0 for best == -1); eligible = the number of eligible strategies
 * The Reality Check p-value is count_rc / R; the single-step adjusted p-value of strategy s is count_adj[s] / R,
 * its naive one count_ge[s] / R.
 * Five launches on the env's stream, no atomics, no host synchronisation; the staging array d[n][S] and the
 * partial results live in library-owned scratch, allocated by the first call and again when a call outgrows it
 * (as gte_rank_strategies keeps its lists).  The inputs are only read; the outputs must not overlap them or
 * each other.
 *
 * BOTH return GTE_ERR_INVALID, with nothing launched and nothing written, for: a NULL env or required pointer
 * (benchmark_device alone may be NULL) or one not aligned for its type (stats_device: 16 bytes); n < 2 or
 * n > GTE_MAX_PERIODS; a mask with fewer than two bits set, or a bit at or above n_periods; n_periods outside
 * [1, GTE_MAX_PERIODS]; n_resamples outside [1, GTE_BOOT_MAX_RESAMPLES]; block below 1.0 or NaN;
 * n_strategies < 1.  GTE_ERR_STATE inside a stream capture. */
#define GTE_BOOT_SLAB 256
#define GTE_BOOT_MAX_RESAMPLES 65536
int gte_bootstrap_weights(gte_env* env, int32_t n, int32_t n_resamples, double block, uint64_t seed,
                          double* weights_device /* [n_resamples * n] */);
typedef struct gte_reality_check_summary {   /* 24 bytes */
  double  best_mean;
  int32_t best;
  int32_t count_rc;
  int32_t eligible;
  int32_t reserved;        /* written as zero */
} gte_reality_check_summary;
typedef struct gte_reality_check_out {       /* DEVICE pointers, all required */
  double  *mean, *boot_sum, *boot_sq_sum;    /* f64 [n_strategies] */
  int32_t *count_ge, *count_adj;             /* i32 [n_strategies] */
  double  *max_stat;                         /* f64 [n_resamples] */
  int32_t *max_index;                        /* i32 [n_resamples] */
  gte_reality_check_summary* summary;        /* one record */
} gte_reality_check_out;
int gte_reality_check(gte_env* env, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                      int32_t n_periods, const uint64_t period_mask[2],
                      const double* benchmark_device /* [n_periods] or NULL */, const double* weights_device,
                      int32_t n_resamples, const gte_reality_check_out* out);

/* ---- TEST FOR SUPERIOR PREDICTIVE ABILITY (Hansen 2005) AND ITS STEP-DOWN (Hsu, Hsu, Kuan 2010, after Romano and
 * Wolf 2005): the Reality Check above, studentised — every strategy measured in its own bootstrap deviation, so that
 * a poor but noisy strategy no longer widens the null distribution — with the null recentred so that clearly poor
 * strategies do not contribute, and a step-down that says WHICH strategies beat the benchmark, not only whether the
 * best one does.  From the same [S, B] records, mask, benchmark and weights as gte_reality_check; the [R, S] matrix is
 * never written.  One fixed order of IEEE f64 operations, every one of them ONE operation as written.
 *
 * PASS 1 is gte_reality_check itself, unchanged, into `rc` (all of whose arrays are written as that call writes
 * them).  With eligible, d_i, mean_s, boot_sum, boot_sq_sum as defined there, R = n_resamples, dR = (double)R, per
 * eligible strategy:
 *     m1 = boot_sum[s] / dR;    v = boot_sq_sum[s] / dR - m1 * m1;    se_s = sqrt(v > 0 ? v : 0.0);    rse_s = 1.0 / se_s
 * Strategy s is STUDENTISED iff it is eligible, mean_s and se_s are finite and se_s > 0.  For a studentised strategy
 *     t_s = mean_s * rse_s
 *     g0_s = mean_s > 0 ? mean_s : 0.0          (lower: Hansen's SPA_l)
 *     g1_s = t_s >= -threshold ? mean_s : 0.0   (consistent: SPA_c; recentred[s] = 1 iff the first branch is taken)
 *     g2_s = mean_s                             (upper: SPA_u, the studentised Reality Check)
 * THE STATISTIC.  m = -inf, best = -1; over studentised s ascending: if (t_s > m) { m = t_s; best = s; }
 * statistic = m > 0.0 ? m : 0.0.
 * A PASS over a set `live` of strategies with recentring j, per resample r:
 *     q_rs = a / (double)n, a the chain of gte_reality_check (a = 0.0; over i ascending: a = a + weights[r][i] * d_i)
 *     z = (q_rs - gj_s) * rse_s          (a multiplication by the reciprocal, not a division by se_s)
 *     m = -inf, index = -1; over live s ascending: if (z > m) { m = z; index = s; }        (a NaN never wins)
 *     M_j[r] = m > 0.0 ? m : 0.0         (never NaN, never -0.0);   I_j[r] = index
 * ROUND 0 passes over live_0, the studentised strategies, with j = 0, 1, 2:  max_stat[j * R + r] = M_j[r],
 * max_index[j * R + r] = I_j[r] (all 0.0 and -1 when nothing is studentised).  When at least one strategy is
 * studentised:   count_lower, count_consistent, count_upper = #{r : M_j[r] >= statistic} for j = 0, 1, 2 (else 0);
 * the SPA p-values are count / R.   count_adj[s] = #{r : M_1[r] >= t_s} for a studentised s (else 0): its
 * single-step adjusted p-value is count_adj[s] / R.
 * THE STEP-DOWN, on the consistent recentring.  Round k = 0, 1, ... runs while live_k is not empty and
 * k < max_rounds:  M = M_1 of a pass over live_k (round 0: the one above);  crit[k] = the element of rank crit_rank
 * (0-based) of M[0 .. R-1] sorted ascending;  every s of live_k with t_s > crit[k] is rejected:
 * rejected_round[s] = k, and live_{k+1} is live_k without them;  round_rejected[k] = their number.  A round that
 * rejects nothing is the last.  rounds_run = the rounds that ran (0 when nothing is studentised), num_rejected the sum
 * of round_rejected.  With crit_rank = ceil((1 - alpha) * R) - 1 the rejected strategies are those whose mean is
 * above the benchmark's at family-wise level alpha.
 * WRITTEN (all of every array): t_stat[s] (t_s; NaN unless studentised), std_error[s] (se_s; NaN for an ineligible
 * strategy), recentred[s] (u8; 0 unless studentised), count_adj[s], rejected_round[s] (-1: not rejected),
 * max_stat, max_index [3 * R], crit [max_rounds] (NaN from rounds_run on), round_rejected [max_rounds] (0 from
 * rounds_run on), summary.
 * The launches of gte_reality_check, then 6 + 3 * (max_rounds - 1) on the env's stream: every later round is enqueued
 * unconditionally and returns at once when the step-down has stopped (a flag on the device); nothing visits the
 * host, no atomics.  Library-owned scratch of its own, grown as gte_reality_check's.  The inputs are only read; the
 * outputs must not overlap them or each other.
 * GTE_ERR_INVALID, with nothing launched and nothing written, for everything gte_reality_check refuses (`rc` and its
 * members as `out` there), a threshold that is NaN or negative (+inf is allowed: g1 = g2), crit_rank outside
 * [0, n_resamples - 1], max_rounds outside [1, GTE_SPA_MAX_ROUNDS], a NULL `out` or member of it, or one not aligned
 * for its type.  GTE_ERR_STATE inside a stream capture. */
#define GTE_SPA_MAX_ROUNDS 64
typedef struct gte_spa_summary {             /* 40 bytes */
  double  statistic;
  int32_t best;            /* -1 when no t_s compared greater than -inf */
  int32_t count_lower, count_consistent, count_upper;
  int32_t rounds_run, num_rejected;
  int32_t studentised;     /* the number of studentised strategies */
  int32_t reserved;        /* written as zero */
} gte_spa_summary;
typedef struct gte_spa_out {                 /* DEVICE pointers, all required */
  double  *t_stat, *std_error;               /* f64 [n_strategies] */
  uint8_t *recentred;                        /* u8  [n_strategies] */
  int32_t *count_adj, *rejected_round;       /* i32 [n_strategies] */
  double  *max_stat;                         /* f64 [3 * n_resamples] */
  int32_t *max_index;                        /* i32 [3 * n_resamples] */
  double  *crit;                             /* f64 [max_rounds] */
  int32_t *round_rejected;                   /* i32 [max_rounds] */
  gte_spa_summary* summary;                  /* one record */
} gte_spa_out;
int gte_spa_test(gte_env* env, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                 int32_t n_periods, const uint64_t period_mask[2],
                 const double* benchmark_device /* [n_periods] or NULL */, const double* weights_device,
                 int32_t n_resamples, double threshold, int32_t crit_rank, int32_t max_rounds,
                 const gte_reality_check_out* rc, const gte_spa_out* out);

/* ---- PROBABILITY OF BACKTEST OVERFITTING by combinatorially symmetric cross-validation, CSCV (Bailey, Borwein,
 * Lopez de Prado, Zhu 2017): how much does picking the best of S strategies overfit?  The periods are cut into G
 * groups; every split takes some groups as in-sample (IS) and others as out-of-sample (OOS), picks the IS winner
 * and looks where that winner ranks OOS among all strategies, from the [S, B] gte_strategy_period_stats on the
 * device.  The [C, S] matrices of scores are never written.  One fixed order of IEEE f64 operations, every one of
 * them ONE operation as written (no fused multiply-add): the same inputs give the same bits for any launch
 * geometry.
 *
 * GROUPS.  group_masks: HOST uint64 [n_groups][2]; group g is the set of periods whose bit is set in
 * group_masks[g] (bit b % 64 of word b / 64, as period_mask).  Groups are non-empty and pairwise disjoint;
 * 2 <= n_groups <= GTE_CSCV_MAX_GROUPS.  Per strategy and group, over the group's periods b ascending:
 *     a1 = 0.0; a1 = a1 + reward_sum_b;     a2 = 0.0; a2 = a2 + reward_sq_sum_b;     n_g = the sum of steps_b (int64)
 * Of a record only these three fields are read, and only for periods in some group.  Strategy s is ELIGIBLE iff
 * for every group n_g > 0 and a1, a2 are finite.
 * THE SCORE of a strategy over a set Q of groups, over g in Q ascending:
 *     s1 = 0.0; s1 = s1 + a1_g;     s2 = 0.0; s2 = s2 + a2_g;     n = the sum of n_g (int64)
 * and then the GTE_PERIOD_METRIC_MEAN_REWARD, _SHARPE or _REWARD_SUM formulas of gte_rank_period_stats on
 * (s1, s2, n), exactly as written there; the other three period metrics are refused.  When every group is a
 * single period this is bit for bit the score gte_rank_period_stats gives for the same periods.
 * SPLITS.  is_groups, oos_groups: HOST uint32 [n_splits]; split c has IS = the groups whose bit is set in
 * is_groups[c] and OOS = those of oos_groups[c].  Both are non-empty, disjoint, and use no bit at or above
 * n_groups; groups in neither are allowed (purging, an embargo).  1 <= n_splits <= GTE_CSCV_MAX_SPLITS.
 * WRITTEN (all of every array, C = n_splits), IS_cs and OOS_cs being the scores of strategy s over the two sides:
 *     best[c]       m = -inf; over eligible s ascending: if (IS_cs > m) { m = IS_cs; best = s; }; -1 when none
 *                   compared greater (a NaN never wins; of equal scores the lowest index)
 *     is_score[c]   m; NaN when best is -1
 *     oos_score[c]  OOS_cs of s = best; NaN when best is -1
 *     ranked[c]     the number of eligible s whose OOS_cs is not NaN
 *     below[c]      the number of those with OOS_cs < oos_score[c]
 *     equal[c]      the number of those with OOS_cs == oos_score[c], the winner included
 *                   A split is VALID iff best >= 0 and oos_score[c] is not NaN; an invalid one has below = equal = 0.
 *     summary       splits = C; valid = the number of valid splits; overfit = the number of valid splits with
 *                   2 * below + equal <= ranked, which is the winner's mid-rank relative rank
 *                   w = (below + (equal + 1) / 2) / (ranked + 1) being at most 1/2, as an integer comparison;
 *                   loss = the number of valid splits with oos_score < 0.0; eligible = the number of eligible
 *                   strategies
 * The probability of backtest overfitting is overfit / valid, the probability of an out-of-sample loss
 * loss / valid.
 * The three host tables are checked and copied by the call: they are the caller's again when it returns.  Six
 * launches on the env's stream after that copy (fold, IS/OOS pass, winners, rank pass, close, summary), no
 * atomics, no host synchronisation beyond what the copy of the tables needs; the group sums [G][S] and the
 * partial results [tiles][C] live in library-owned scratch, allocated by the first call and again when a call
 * outgrows it (as gte_reality_check keeps its own).  A workgroup takes GTE_CSCV_CHUNK splits.  The inputs are only
 * read; the outputs must not overlap them or each other.
 *
 * GTE_ERR_INVALID, with nothing launched and nothing written, for: a NULL env or pointer, or one not aligned for
 * its type (stats_device: 16 bytes); n_strategies < 1; n_periods outside [1, GTE_MAX_PERIODS]; n_groups or
 * n_splits outside their ranges; a metric other than the three; an empty group, one with a bit at or above
 * n_periods, one that shares a period with an earlier group; a split with an empty side, a bit at or above
 * n_groups, or a group on both sides — the message names the first offending group or split.  GTE_ERR_STATE
 * inside a stream capture. */
#define GTE_CSCV_MAX_GROUPS 32
#define GTE_CSCV_MAX_SPLITS 65536
#define GTE_CSCV_CHUNK 256
typedef struct gte_cscv_summary {            /* 24 bytes */
  int32_t splits, valid, overfit, loss, eligible;
  int32_t reserved;        /* written as zero */
} gte_cscv_summary;
typedef struct gte_cscv_out {                /* DEVICE pointers, all required */
  int32_t *best;                             /* i32 [n_splits] */
  double  *is_score, *oos_score;             /* f64 [n_splits] */
  int32_t *below, *equal, *ranked;           /* i32 [n_splits] */
  gte_cscv_summary* summary;                 /* one record */
} gte_cscv_out;
int gte_cscv(gte_env* env, const gte_strategy_period_stats* stats_device, int32_t n_strategies, int32_t n_periods,
             const uint64_t* group_masks /* HOST [n_groups][2] */, int32_t n_groups,
             const uint32_t* is_groups /* HOST [n_splits] */, const uint32_t* oos_groups /* HOST [n_splits] */,
             int32_t n_splits, int32_t metric, const gte_cscv_out* out);

/* ---- A DECORRELATED LEADERBOARD, PICKED GREEDILY: the best k of a sweep are usually k parameterisations of one
 * bet.  Take the best strategy by the caller's scores, drop every strategy whose period returns correlate with it
 * above max_corr, take the best of what is left, and so on for k rounds, from the [S, B] gte_strategy_period_stats
 * on the device.  The picks are a diversified shortlist, what a pick dropped is its cluster, and when nothing is
 * left the number of picks is the number of independent strategies the sweep held at that threshold.  No [S, S]
 * matrix is written.  One fixed order of IEEE f64 operations, every one of them ONE operation as written (no fused
 * multiply-add), sqrt and division correctly rounded: the same inputs give the same bits for any launch geometry.
 *
 * PERIODS AND ELIGIBILITY.  P = p_0 < ... < p_{n-1}, the periods whose bit is set in period_mask (bit b % 64 of word
 * b / 64; HOST uint64 [2]), 3 <= n <= GTE_MAX_PERIODS.  Strategy s is ELIGIBLE iff for every b in P steps_b > 0 and
 * reward_sum_b is finite (the rule of gte_reality_check), and its q below is finite and q > 0.0 (a constant row has no
 * correlation).  Of a record only steps and reward_sum are read, and only for b in P.
 * THE STANDARDISED ROW of an eligible strategy, x_i = reward_sum[s][p_i]:
 *     t = 0.0; over i ascending: t = t + x_i;              m = t / (double)n
 *     e_i = x_i - m
 *     q = 0.0; over i ascending: q = q + e_i * e_i;        norm = sqrt(q)
 *     u_i = e_i / norm
 * THE CORRELATION of s with j:   c = 0.0; over i ascending: c = c + u_i[s] * u_i[j]
 * CANDIDATES.  scores_device: DEVICE f64 [S], any score vector of the caller's (the scores_device of a gte_rank_*
 * call, a negated p-value).  s is a CANDIDATE iff it is eligible and scores_device[s] is not NaN; +-inf are values
 * like any other.
 * THE GREEDY ROUNDS, r = 0 .. k-1, 1 <= k <= GTE_RANK_MAX.  All candidates start LIVE.
 *     pick[r]       the live candidate with the highest score; equal scores go to the lowest index (-0.0 == 0.0, by
 *                   comparison, as gte_rank_strategies orders).  With no candidate live: pick[r] = -1,
 *                   pick_score[r] = NaN, cluster_size[r] = 0, and the same for every later round
 *     otherwise, for every live s: c_s = the correlation of s with pick[r]; s LEAVES the live set iff s == pick[r]
 *                   or c_s > max_corr (a NaN compares false and stays); then owner[s] = r and owner_corr[s] = c_s —
 *                   for the pick itself too, whose owner_corr is the formula's own value, not a literal 1.0
 *     cluster_size[r]   the number that left in round r
 * WRITTEN (all of every array):
 *     pick i32 [k], pick_score f64 [k] (scores_device[pick[r]] as it stands), cluster_size i32 [k]
 *     owner i32 [S]       the round that claimed s; -1 for a candidate still live after k rounds; -2 for a strategy
 *                         that is no candidate
 *     owner_corr f64 [S]  NaN where owner < 0
 *     pick_corr f64 [k][k]   the correlation of pick[a] with pick[b] by the formula above, for both orders (a
 *                         multiplication commutes: the matrix is symmetric to the bit); NaN where either pick is -1
 *     summary             picked = the number of rounds with a pick; candidates, eligible = the numbers of such
 *                         strategies; remaining = the candidates still live after the last round; reserved = 0.
 *                         remaining == 0: picked is the number of clusters at this threshold
 * max_corr is any value but NaN: above 1 a round drops its pick alone, -inf makes round 0 take every candidate.
 * k + 2 launches on the env's stream (prepare, one per round, close); the pick of a round never visits the host.  No
 * atomics, no host synchronisation; the staging array u[n][S], the live bytes, two lists of the workgroups' best
 * remaining candidates and the workgroups' counts live in library-owned scratch, allocated by the first call and
 * again when a call outgrows it (as gte_reality_check keeps its own).  The inputs are only read; the outputs must not
 * overlap them or each other.
 *
 * GTE_ERR_INVALID, with nothing launched and nothing written, for: a NULL env or pointer, or one not aligned for its
 * type (stats_device: 16 bytes; f64: 8; i32 and the summary: 4); n_strategies < 1; n_periods outside
 * [1, GTE_MAX_PERIODS]; k outside [1, GTE_RANK_MAX]; a mask with fewer than three bits set, or a bit at or above
 * n_periods; a NaN max_corr.  GTE_ERR_STATE inside a stream capture. */
typedef struct gte_diversify_summary {       /* 20 bytes */
  int32_t picked, candidates, eligible, remaining;
  int32_t reserved;        /* written as zero */
} gte_diversify_summary;
typedef struct gte_diversify_out {           /* DEVICE pointers, all required */
  int32_t *pick;                             /* i32 [k] */
  double  *pick_score;                       /* f64 [k] */
  int32_t *cluster_size;                     /* i32 [k] */
  int32_t *owner;                            /* i32 [n_strategies] */
  double  *owner_corr;                       /* f64 [n_strategies] */
  double  *pick_corr;                        /* f64 [k * k] */
  gte_diversify_summary* summary;            /* one record */
} gte_diversify_out;
int gte_diversify(gte_env* env, const gte_strategy_period_stats* stats_device, int32_t n_strategies,
                  int32_t n_periods, const uint64_t period_mask[2], const double* scores_device /* [n_strategies] */,
                  double max_corr, int32_t k, const gte_diversify_out* out);

/* ---- TRADE MONTE CARLO: how bad can a chosen strategy get?  Its realised maximum drawdown and losing streak are
 * ONE ordering of its closed trades.  Draw trades with replacement from its trade list, compound them, and read the
 * distribution of final equity, maximum drawdown, lowest equity and losing streak — for many strategies at once, on
 * the device.  One fixed order of IEEE f64 operations, every one of them ONE operation as written (no fused
 * multiply-add), comparisons plain: the same inputs give the same bits for any launch geometry.  The walk step, the
 * index mapping and the slab tree below are also stated as plain C++ in include/gte_mc.h, which a host program can
 * compile to replay them.
 *
 * THE POOLS, gte_pool_trades.  Builds the pool of trade factors of each requested strategy from the env's live
 * trade list (gte_track_trade_list).  MEMBERS and the skipping rule are exactly those of gte_reduce_backtest_stats
 * (both group pointers NULL = the library's map over env_id_base; an entry that names no env in [0, N) is skipped).
 * The pool of request q: the members of strategy strategies[q] in member order; of each member its first
 * min(closed, capacity) list records in close order; each record contributes
 *     factor = close_value / open_value                    (one f64 division; NaN, inf, 0 and negatives kept as they are)
 * A strategy id outside [0, n_strategies) — the -1 padding of a ranking — gives an empty pool.  WRITTEN:
 *     first[q], q = 0 .. n_pools    the running sum of the pools' sizes; first[n_pools] is always the full total
 *     truncated[q]                  the number of members with closed > capacity (their lists kept the first ones)
 *     factors[first[q] ..)          the pool of request q; a factor at or past max_factors is not written
 * The two-pass protocol of gte_pack_trade_list: factors_device NULL with max_factors 0 counts only.  One
 * count-and-scan launch and one pack launch on the env's stream, no atomics, no host synchronisation.
 * GTE_ERR_INVALID, with nothing launched, for: a NULL env; n_pools outside [1, GTE_MC_MAX_POOLS]; n_strategies < 1;
 * exactly one group pointer NULL; a NULL strategies_device, first_device or truncated_device; max_factors < 0, or
 * > 0 with a NULL factors_device; a pointer not aligned for its type (i32: 4, i64 and f64: 8).  GTE_ERR_STATE
 * exactly where gte_pack_trade_list returns it (the list is off, or was switched and not cleared since), and inside
 * a stream capture.
 *
 * THE RESAMPLING, gte_trade_monte_carlo.  No tie to the trade list: factors_device / first_device are any pools — the
 * ones above, a caller's own returns, a synthetic test.  Pool q is factors[first[q] .. first[q + 1]), its size
 * P = first[q + 1] - first[q].  A pool with first[q + 1] < first[q], with P >= 2^31, or that reaches outside
 * [first[0], first[n_pools]) is treated as EMPTY (P = 0): no content of `first` makes a kernel read outside
 * factors[first[0] .. first[n_pools]).  THE CALLER'S OBLIGATION: first_device holds n_pools + 1 entries, and
 * factors_device[first[0]] .. factors_device[first[n_pools] - 1] is readable device memory.  L = path_len if it is positive, else
 * min(P, GTE_MC_MAX_PATH); L = 0 for an empty pool.  stream[q] is stream_device[q], or q when that is NULL.
 * Per resample r = 0 .. n_resamples-1:
 *     e = 1.0; peak = 1.0; mdd = 0.0; low = 1.0; streak = 0; max_streak = 0
 *     for i = 0 .. L-1:
 *         o = philox4x32_10(counter = {i >> 2, r, stream[q], 0x54524D43 'TRMC'}, key = {seed low word, seed high word})
 *         j = mulhi32(o[i & 3], P);  f = factors[first[q] + j]
 *         e = e * f
 *         if (e > peak) peak = e
 *         d = 1.0 - e / peak;  if (d > mdd) mdd = d
 *         if (e < low) low = e
 *         if (f < 1.0) { streak += 1; if (streak > max_streak) max_streak = streak; } else streak = 0
 * Row r depends on (seed, stream[q], r, i) and the pool alone: not on n_resamples, not on the slot q.
 * WRITTEN, R = n_resamples:
 *     final, max_drawdown, low [q * R + r]   e, mdd, low after the walk (f64); max_loss_streak [q * R + r] max_streak
 *                      (i32).  Each of the four may be NULL: it is then not written and costs no store.
 *     pool[q]          final_sum, final_sq_sum (of final * final), mdd_sum, mdd_sq_sum (of mdd * mdd): resamples cut
 *                      into slabs of GTE_MC_SLAB; within a slab 256 places hold x of resample slab * 256 + i, a
 *                      place past R holds 0.0, then for h = 128, 64, ..., 1: x[i] = x[i] + x[i + h] for i < h; the
 *                      slabs' x[0] added from 0.0 in ascending slab order.  count_loss: resamples with
 *                      final < 1.0; count_ruin: with low <= ruin_level; pool_size = P; path_len = L.  Counts exact.
 *     dd_count[q * n_levels + k]    resamples with mdd >= dd_levels[k]   (dd_levels: HOST f64 [n_levels], read
 *                      before the call returns; may be NULL when n_levels is 0)
 * A walk launch (one workgroup of 256 lanes = one slab of one pool, a lane a resample; a pool of at most
 * GTE_MC_LDS_POOL factors is staged into LDS once, a larger one is read from global memory — the same bits either
 * way) and a close launch on the env's stream; no atomics, no host synchronisation; the slabs' partial results live
 * in library-owned scratch, allocated by the first call and again when a call outgrows it (as gte_reality_check
 * keeps its own).  The inputs are only read; the outputs must not overlap them or each other.
 * GTE_ERR_INVALID, with nothing launched and nothing written, for: a NULL env, factors_device, first_device, out,
 * out->pool, or out->dd_count with n_levels > 0, or dd_levels with n_levels > 0; a pointer not aligned for its type
 * (f64 and i64: 8; i32 and u32: 4; pool: 16); n_pools outside [1, GTE_MC_MAX_POOLS]; n_resamples outside
 * [1, GTE_MC_MAX_RESAMPLES]; path_len outside [0, GTE_MC_MAX_PATH]; n_levels outside [0, GTE_MC_MAX_LEVELS]; a NaN
 * ruin_level.  GTE_ERR_STATE inside a stream capture. */
#define GTE_MC_SLAB 256
#define GTE_MC_MAX_RESAMPLES 65536
#define GTE_MC_MAX_POOLS 65536
#define GTE_MC_MAX_PATH (1 << 20)
#define GTE_MC_MAX_LEVELS 8
#define GTE_MC_LDS_POOL 8192
int gte_pool_trades(gte_env* env, int32_t n_strategies, const int32_t* group_offsets_device,
                    const int32_t* group_envs_device, const int32_t* strategies_device /* [n_pools] */,
                    int32_t n_pools, int64_t* first_device /* [n_pools + 1] */,
                    int32_t* truncated_device /* [n_pools] */, double* factors_device /* [max_factors] or NULL */,
                    int64_t max_factors);
typedef struct gte_mc_pool {                 /* 48 bytes, three 16-byte pieces */
  double  final_sum, final_sq_sum;
  double  mdd_sum, mdd_sq_sum;
  int32_t count_loss, count_ruin, pool_size, path_len;
} gte_mc_pool;
typedef struct gte_mc_out {                  /* DEVICE pointers */
  double  *final, *max_drawdown, *low;       /* f64 [n_pools * n_resamples], each may be NULL */
  int32_t *max_loss_streak;                  /* i32 [n_pools * n_resamples], may be NULL */
  gte_mc_pool* pool;                         /* [n_pools], required */
  int32_t *dd_count;                         /* i32 [n_pools * n_levels], required when n_levels > 0 */
} gte_mc_out;
int gte_trade_monte_carlo(gte_env* env, const double* factors_device, const int64_t* first_device,
                          const uint32_t* stream_device /* [n_pools] or NULL: q */, int32_t n_pools,
                          int32_t n_resamples, int32_t path_len /* 0: the pool's size */, uint64_t seed,
                          double ruin_level, const double* dd_levels /* HOST [n_levels] */, int32_t n_levels,
                          const gte_mc_out* out);

/* Where the results of the last gte_step / gte_reset live (device pointers). */
int gte_get_outputs(gte_env* env, gte_outputs* out);
/* Same-step auto-reset with gte_config.final_obs: struct-of-arrays snapshot (device pointers,
 * extracted like gte_get_state) of every env's record AS IT WAS WHEN ITS LAST EPISODE ENDED —
 * the state `TradingEnv.step` reported in `info` before the wrapper reset the env
 * (Gymnasium `final_info`).  Row e is meaningful for the envs listed in term_ids after a step.
 * `episode` / `needs_reset` of the view are not meaningful here. */
int gte_get_final_state(gte_env* env, gte_state_view* out);

/* Snapshot of the per-env state as struct-of-arrays device buffers.  Internally the
 * state is one 128-byte record per env; this call enqueues a small extraction
 * kernel on the env's stream, so the views reflect every launch enqueued before
 * it.  Call it again after later steps (the pointers stay the same). */
int gte_get_state(gte_env* env, gte_state_view* out);

/* Everything the reference's step()/reset() hand back for ONE env (environments.py:253-272:
 * the History row and the return tuple), fetched with one device->host transfer. */
typedef struct gte_env_snapshot {
  int32_t idx, step, position_index, dataset_index;
  int32_t start_idx, episode, needs_reset, terminated, truncated, reserved;
  double asset, fiat, interest_asset, interest_fiat;   /* Portfolio, portfolio.py:1-6 */
  double portfolio_valuation, real_position;           /* :241, :259 */
  double reward;                                       /* f64, :265-267 */
} gte_env_snapshot;

/* State + returns + observations of envs first .. first+count-1 after the last step/reset,
 * into HOST memory: a small kernel (one workgroup per env) packs them into pinned host memory
 * on the env's stream, then the stream is synchronised once.  `out` receives `count` snapshots,
 * `obs` (count * W*F_obs floats) may be NULL.  This is what the host-array ("numpy") mode of
 * the Python classes calls once per step instead of one copy per field. */
int gte_read_envs(gte_env* env, int32_t first, int32_t count, gte_env_snapshot* out, float* obs);
/* The same without the final copy: *out / *obs point INTO the library's pinned host staging
 * buffer (`count` snapshots; `count` * W*F_obs floats, or NULL when want_obs == 0) and stay
 * valid until the next gte_read_envs / gte_read_envs_view / gte_read_env / gte_destroy on this
 * env.  For host-array consumers that can live with buffers being reused every step (what
 * Gymnasium's vector envs call copy=False). */
int gte_read_envs_view(gte_env* env, int32_t first, int32_t count, int32_t want_obs,
                       const gte_env_snapshot** out, const float** obs);
/* gte_read_envs for one env (the N=1 drop-in TradingEnv's per-step call). */
int gte_read_env(gte_env* env, int32_t env_index, gte_env_snapshot* out, float* obs);

/* Use caller-owned device buffers for the outputs (e.g. torch tensors that are
 * then all-gathered over RCCL).  NULL members keep the library's buffer.  The library's own
 * observation buffers ([N, W, F_obs], and the final_obs one) are allocated on first need —
 * the first gte_reset or gte_get_outputs that finds none bound — so a caller that binds its
 * own before resetting never pays for a second copy. */
int gte_bind_outputs(gte_env* env, const gte_outputs* bufs);

/* Sliding observation buffer.  A step moves every window one row forward and, for an env that
 * merely advanced, differs from the previous observation in ONE row; a classic [N, W, F_obs]
 * buffer still rewrites all W.  Give every env W + M rows instead: the observation of env e is
 * rows head .. head + W - 1 of its slab, with ONE head for the whole batch,
 *     obs(e) = base + (e * rows_per_env + head) * F_obs,     W * F_obs floats, chronological,
 * i.e. a strided [N, W, F_obs] tensor with strides (rows_per_env * F_obs, F_obs, 1).  A step
 * that finds head < M moves the head up by one and stores only row head + W - 1 of the envs that
 * advanced (full windows for those that reset or stand frozen); at head == M, and whenever the
 * library cannot prove that the buffer holds this env's previous observation at the current
 * head (a rebind, a rollout, a stream capture, another env writing the buffer), the step writes
 * every window in full at head 0.  A masked gte_reset writes the masked envs' windows at the
 * current head; an unmasked one returns to head 0.  The values are those of the classic buffer,
 * bit for bit.
 *
 * gte_obs_view reports where the current observation is; slack_rows is the M this env may use
 * (0: the shape or the configuration does not slide — anything but 16-byte-vector windows of at
 * least 64 vectors on the cooperative LDS-staged step kernel, dyn_persist, final_obs, a
 * trajectory log, window == 0, obs_slack_rows == -1).  gte_bind_sliding_obs binds a caller-owned,
 * 16-byte-aligned f32 [N, rows_per_env, F_obs] buffer with rows_per_env == W + slack_rows
 * (GTE_ERR_STATE where slack_rows is 0); gte_bind_outputs, with or without an obs pointer, returns
 * to the classic layout.  While a sliding buffer is bound gte_get_outputs().obs is the BASE of the
 * buffer (use gte_obs_view for the window), the gte_read_* calls return the current window, and
 * gte_allgather_obs fails (RCCL sends a contiguous buffer).
 *
 * A/B and twin runs: with GTE_SLIDE_FULL_WINDOWS set in the environment when gte_create runs, the env
 * keeps the sliding layout and the moving head, but every step writes every window in full (the
 * enum gte_kernel_variant keeps its values: tests pin them; this is a tuning switch like
 * GTE_AFFINITY_BINS).
 *
 * GTE_SLIDE_AB, read the same way, is a bit mask.  Bit 1 keeps slide launches (steps that store one row per
 * env) in the L2-affinity order, with a due re-sort run at once, as the sliding window's first version did;
 * by default they run in env order and a re-sort that falls due waits for the next launch that writes full
 * windows.  Bit 2 makes slide launches store with the policy of the launches that write full windows (below),
 * as they did before they had one of their own; it outranks GTE_SLIDE_STORE.  Results never depend on either.
 * The other bits are reserved and ignored.
 *
 * Store policy per launch kind.  nontemporal_obs (gte_config) names the observation store policy; left
 * automatic (3), the launches that write full windows — wraps, resets, full steps after a withdrawn claim,
 * GTE_SLIDE_FULL_WINDOWS, rollout rows, captured steps, every env that does not slide — take sc1 while the
 * classic N x W x F_obs x 4 bytes stay below 190 MB and non-temporal stores beyond, and slide launches take
 * non-temporal stores once the slab, N x (W + M) x F_obs x 4 bytes, exceeds 190 MB (else the same policy).
 * An explicit 0, 1 or 2 governs both kinds.  Where the two differ, slide launches keep their own only if its
 * kernel instantiation holds the plan's workgroups resident at once as the other does.
 * GTE_SLIDE_STORE=0|1|2 in the environment when gte_create runs forces the slide launches' policy (a tuning
 * switch like GTE_AFFINITY_BINS; no effect on an env that never slides).  gte_get_launch_info reports both. */
typedef struct gte_obs_view_t {
  float*  base;          /* the bound observation buffer (NULL before one exists)            */
  int32_t rows_per_env;  /* W + M while sliding, else W                                      */
  int32_t head;          /* first row of the current window in every env's slab              */
  int32_t sliding;       /* 1 while a sliding buffer is bound                                */
  int32_t slack_rows;    /* the M gte_bind_sliding_obs accepts for this env, 0 = none        */
} gte_obs_view_t;
int gte_obs_view(gte_env* env, gte_obs_view_t* out);
int gte_bind_sliding_obs(gte_env* env, float* base, int32_t rows_per_env);
/* Redirect ONLY the per-step returns (reward f32[N], terminated u8[N], truncated u8[N]) of
 * the steps enqueued AFTER this call; nothing is synchronised and nothing already
 * enqueued changes.  A sharded run rotates between two (or more) caller-owned return
 * buffers with it, so that the RCCL all-gather of step t's returns (environments.py:272,
 * the `reward, done, truncated` a caller gets back) overlaps step t+1 on another stream.
 * All three pointers are required; the caller keeps the buffers alive while steps that
 * write them or collectives that read them are in flight. */
int gte_bind_returns(gte_env* env, float* reward, uint8_t* terminated, uint8_t* truncated);

/* ---- multi-GPU: the ONE exchange of the sharded path.  Environments shard over
 * the GPUs of a node with no data-path collective; what a caller of the reference's vector env
 * gets back from step() — `reward, done, truncated` for ALL environments (environments.py:272,
 * docs/source/vectorize_env.rst:55-65) — is assembled by an RCCL all-gather over xGMI of the
 * packed per-shard records (reward f32 [N] | terminated u8 [N] | truncated u8 [N], the layout the
 * step kernel writes), and on request of the observations.  One process per GPU; RCCL is bound
 * at run time (no link-time dependency). */
#define GTE_COMM_ID_BYTES 128
/* rank 0 creates the id (ncclGetUniqueId) and hands it to every rank by any host channel */
int gte_comm_unique_id(uint8_t* id_out /* [GTE_COMM_ID_BYTES] */);
/* every rank, collectively: one communicator per env (equal n_envs on every rank) */
int gte_comm_init(gte_env* env, const uint8_t* id, int32_t rank, int32_t world);
/* all-gather `bytes_per_rank` bytes from src_device into dst_device [world * bytes_per_rank]
 * (rank r's block at offset r * bytes_per_rank).  mode 0: on the env's stream — stream-ordered
 * between two steps, no host synchronisation (the synchronous per-step form); mode 1: on the
 * library's communication stream behind an event on the env's stream, overlapping the launches
 * enqueued afterwards (the caller keeps src intact meanwhile: gte_bind_returns rotates return
 * buffers; a block of K rotated rows is one contiguous src) — join with gte_comm_wait(env, back)
 * (orders the env's stream after the mode-1 gather issued `back` gathers ago, 0 = the last one,
 * up to 3: with two rotating return buffers, `gte_comm_wait(env, 1)` before step t makes the
 * gather of step t-2 release the buffer step t rewrites while the gather of step t-1 still
 * overlaps it) or gte_comm_synchronize (blocks the host). */
int gte_allgather(gte_env* env, const void* src_device, void* dst_device,
                  uint64_t bytes_per_rank, int32_t mode);
/* the packed returns of the last step: 6N bytes per rank -> u8 [world, 6N] in dst_device, or in
 * a library-owned buffer when dst_device is NULL (*gathered receives the address used) */
int gte_allgather_returns(gte_env* env, void* dst_device, int32_t mode, const void** gathered);
/* the observations of the last step -> f32 [world * N, W, F_obs] (xGMI-bound at the headline
 * shape: 168 MB per rank and step) */
int gte_allgather_obs(gte_env* env, float* dst_device, int32_t mode);
int gte_comm_wait(gte_env* env, int32_t back);
int gte_comm_synchronize(gte_env* env);
int gte_comm_destroy(gte_env* env); /* also done by gte_destroy */

/* Run on exactly this hipStream_t; NULL is HIP's null (default) stream, which is
 * what PyTorch's default stream is.  A new env runs on a private non-blocking
 * stream until this is called; gte_use_own_stream goes back to it. */
int gte_set_stream(gte_env* env, void* hip_stream);
int gte_use_own_stream(gte_env* env);
int gte_synchronize(gte_env* env);

/* HIP-event timing on the env's stream, for bench.py's roofline figure. */
int gte_timer_start(gte_env* env);
/* elapsed_ms != NULL: record the end event (unless already marked), wait for it, return the
 * span.  elapsed_ms == NULL: only record the end event, asynchronously ("mark"); a later call
 * with a pointer reads it — so that a wall-clock bracket around the same steps does not also
 * pay for the event wait. */
int gte_timer_stop(gte_env* env, float* elapsed_ms);

/* Synchronous device -> host copies (the N=1 drop-in and the tests use them;
 * the batched path keeps everything on the device). */
int gte_read_obs(gte_env* env, int32_t first_env, int32_t n, float* host_dst);
/* device_src must be a pointer obtained from gte_get_outputs / gte_get_state
 * (plus an offset inside that array); waits for the env's stream first. */
int gte_copy_to_host(gte_env* env, const void* device_src, void* host_dst,
                     uint64_t bytes);

/* kernel geometry actually used (for DESIGN.md / bench output).  *vector_bytes = bytes per
 * copy vector + 1000 * flags: bit 0 cooperative phase A, bits 1-2 staging of the dynamic
 * columns (0 none, 1 raw rings in LDS, 2 resolved in LDS), bit 3 unused, bits 4-5
 * the observation store policy in use (0 plain, 1 nt, 2 sc1; never 3), bits 6-9 the resident
 * workgroups per CU the automatic geometry was sized for (0 = not applicable), bits 10-11 the
 * store policy of slide launches (same values; equal to bits 4-5 while no sliding buffer is bound). */
int gte_get_launch_info(gte_env* env, int32_t* envs_per_wave,
                        int32_t* threads_per_block, int32_t* n_blocks,
                        int32_t* vector_bytes);

void gte_destroy(gte_env* env);
const char* gte_last_error(void);
int gte_abi_version(void);
int gte_device_count(void); /* usable HIP devices (0 on a CPU-only host)    */

#ifdef __cplusplus
}
#endif
#endif /* GTE_H_ */
