// gte_api.hip — host side of libgte: the C ABI declared in include/gte.h.  This unit: create / destroy, datasets,
// the step path with all that launches through it (step, rollout, backtest()), outputs, state, the error channel;
// the other entry points in gte_api_backtest / _leaderboard / _read.hip and gte_comm.hip (shared: gte_host.h).
//
// Owns the HBM-resident datasets, per-env state and outputs, validates the
// arguments the way the reference constructor / reset do
// (environments.py:79-125,163-199) and launches the kernels of
// the other units (gte_launch.h).  No CPU path exists: without a gfx950 device every entry
// point that needs one fails with GTE_ERR_NO_DEVICE.
#include "gte_host.h"

static int validate(const gte_config* c) {
  if (!c) return fail(GTE_ERR_INVALID, "config is NULL");
  if (c->abi_version != GTE_ABI_VERSION || c->struct_bytes != (int32_t)sizeof(gte_config))
    return fail(GTE_ERR_INVALID, "ABI mismatch: header version %d / %d bytes, library %d / %zu",
                c->abi_version, c->struct_bytes, GTE_ABI_VERSION, sizeof(gte_config));
  if (c->n_envs <= 0) return fail(GTE_ERR_INVALID, "n_envs must be > 0");
  if (c->n_datasets <= 0) return fail(GTE_ERR_INVALID, "n_datasets must be > 0");
  if (c->n_static < 0 || c->n_dyn < 0 || c->n_dyn > GTE_MAX_DYN)
    return fail(GTE_ERR_INVALID, "n_static >= 0 and 0 <= n_dyn <= %d required", GTE_MAX_DYN);
  if (c->n_static + c->n_dyn <= 0) return fail(GTE_ERR_INVALID, "observation has no columns");
  if (c->n_static + c->n_dyn > 2048) return fail(GTE_ERR_INVALID, "F_obs > 2048 unsupported");
  for (int i = 0; i < c->n_dyn; ++i)
    if (c->dyn_kind[i] != GTE_DYN_LAST_POSITION && c->dyn_kind[i] != GTE_DYN_REAL_POSITION)
      return fail(GTE_ERR_INVALID, "dyn_kind[%d] = %d unknown", i, c->dyn_kind[i]);
  if (c->window < 0) return fail(GTE_ERR_INVALID, "window must be >= 0");
  if (c->window >= 32768)  // JobRec.meta keeps the zero-row count of a window in 15 bits
    return fail(GTE_ERR_INVALID, "window must be < 32768");
  const int64_t W = c->window > 0 ? c->window : 1;
  if (W * (c->n_static + c->n_dyn) > (1 << 18))
    return fail(GTE_ERR_INVALID, "window * F_obs > 2^18 floats unsupported");
  if (c->n_positions <= 0 || c->n_positions > GTE_MAX_POSITIONS)
    return fail(GTE_ERR_INVALID, "1..%d positions required", GTE_MAX_POSITIONS);
  if (c->initial_position_index < -1 || c->initial_position_index >= c->n_positions)
    return fail(GTE_ERR_INVALID,
                "The 'initial_position' parameter must be 'random' or a position mentionned "
                "in the 'position' parameter.");  // environments.py:106
  if (c->max_episode_duration < 0 || c->max_episode_duration == 1)
    return fail(GTE_ERR_INVALID, "max_episode_duration must be 0 ('max') or >= 2");
  if (!(c->portfolio_initial_value > 0.0))
    return fail(GTE_ERR_INVALID, "portfolio_initial_value must be > 0");
  if (c->reward_kind < 0 || c->reward_kind > GTE_REWARD_CLIPPED_LOG_RETURN)
    return fail(GTE_ERR_INVALID, "reward_kind %d unknown", c->reward_kind);
  if (c->autoreset < 0 || c->autoreset > GTE_AUTORESET_SAME_STEP)
    return fail(GTE_ERR_INVALID, "autoreset %d unknown", c->autoreset);
  if (c->episodes_between_dataset_switch < 1)
    return fail(GTE_ERR_INVALID, "episodes_between_dataset_switch must be >= 1");
  if (c->nontemporal_obs < 0 || c->nontemporal_obs > 3)
    return fail(GTE_ERR_INVALID, "nontemporal_obs must be 0 (plain), 1 (nt), 2 (sc1) or 3 (automatic)");
  if (c->log_steps < 0) return fail(GTE_ERR_INVALID, "log_steps must be >= 0");
  if (c->final_obs && c->autoreset != GTE_AUTORESET_SAME_STEP)
    return fail(GTE_ERR_INVALID, "final_obs needs autoreset = same-step");
  if (c->envs_per_wave < 0 || c->envs_per_wave > 64)
    return fail(GTE_ERR_INVALID, "envs_per_wave must be 0 (automatic) or 1..64");
  if (c->obs_slack_rows < -1 || c->obs_slack_rows > 32768)
    return fail(GTE_ERR_INVALID, "obs_slack_rows must be -1 (off), 0 (automatic) or 1..32768");
  return GTE_OK;
}

// *n_cu: the device's compute units, which the launch planner sizes by
static int require_device(int device, int* n_cu) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(GTE_ERR_NO_DEVICE,
                "no HIP device available (%s): libgte has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "0 devices");
  if (device < 0 || device >= n)
    return fail(GTE_ERR_NO_DEVICE, "device %d out of range (have %d)", device, n);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(GTE_ERR_NO_DEVICE, "device %d is %s; libgte is built for gfx950 (MI355X) only",
                device, prop.gcnArchName);
  if (prop.multiProcessorCount <= 0)
    return fail(GTE_ERR_NO_DEVICE, "device %d reports no compute units", device);
  *n_cu = prop.multiProcessorCount;
  return GTE_OK;
}

static int alloc_soa(gte_env* E, gte::StateSoA* o, size_t N) {
  for (int32_t** a : {&o->idx, &o->step, &o->pos, &o->dsi, &o->start, &o->episode, &o->needs_reset})
    TRY(dev_alloc(E, a, N));
  for (double** a : {&o->asset, &o->fiat, &o->ia, &o->ifi, &o->pv, &o->realpos}) TRY(dev_alloc(E, a, N));
  return GTE_OK;
}

// gte_create's way out once the env exists: free it, keep the message of the failure
static int create_failed(gte_env* E, int rc) {
  const std::string keep = g_err;
  gte_destroy(E);
  g_err = keep;
  return rc;
}

// --- launch planning: the rules are in gte_plan.h; here are what they are given and what is done with the result

static gte_plan::Shape plan_shape(const gte_env* E) {
  const Params& p = E->p;
  const gte_config& c = E->cfg;
  gte_plan::Shape s;
  s.N = p.N; s.D = p.D; s.W = p.W; s.has_window = p.has_window != 0; s.Fobs = p.Fobs; s.nd = p.nd;
  s.persist = p.persist != 0; s.max_dur = p.max_dur; s.final_obs = c.final_obs != 0; s.log_steps = c.log_steps;
  s.envs_per_wave = c.envs_per_wave; s.nontemporal_obs = c.nontemporal_obs; s.obs_slack_rows = c.obs_slack_rows;
  s.affinity_period = c.affinity_period; s.kernel_variant = c.kernel_variant; s.debug_flags = c.debug_flags;
  return s;
}

static bool debug_geometry() { return getenv("GTE_DEBUG_GEOMETRY") != nullptr; }

// The environment switches, read at the moments include/gte.h promises (tests set them between two gte_create
// calls of one process): the slide switches and the bins at gte_create, GTE_RESIDENT_EPB at the first rollout
// that chooses a resident geometry for a store policy, GTE_DEBUG_GEOMETRY whenever a line would be printed.
enum KnobsMoment { KNOBS_CREATE, KNOBS_ROLLOUT };
static gte_plan::Knobs read_knobs(KnobsMoment when) {
  gte_plan::Knobs k;
  k.debug_geometry = debug_geometry();
  if (when == KNOBS_CREATE) {
    k.slide_full_windows = getenv("GTE_SLIDE_FULL_WINDOWS") != nullptr;
    if (const char* o = getenv("GTE_SLIDE_AB")) k.slide_ab = atoi(o);
    if (const char* o = getenv("GTE_SLIDE_STORE"))
      if (o[0] >= '0' && o[0] <= '2' && o[1] == '\0') k.slide_store = o[0] - '0';
    if (const char* o = getenv("GTE_AFFINITY_BINS")) { k.has_affinity_bins = true; k.affinity_bins = atoi(o); }
  } else if (const char* o = getenv("GTE_RESIDENT_EPB")) {
    k.has_resident_epb = true;
    k.resident_epb = atoi(o);
  }
  return k;
}

// The chip as the planner sees it: the kernels' LDS images and what the HIP runtime says of their residency.
// Every answer is asked afresh (the resident query opts its kernel into large LDS as a side effect).
// GTE_DEBUG_GEOMETRY: each question prints its arguments and its answer.
struct DeviceChip final : gte_plan::Chip {
  const gte_env* E;
  explicit DeviceChip(const gte_env* env) : E(env) { n_cu = said(env->n_cu, "n_cu device=%d", env->cfg.device); }
  template <typename T>
  static T said(T answer, const char* fmt, ...) {
    if (debug_geometry()) {
      char q[128];
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(q, sizeof q, fmt, ap);
      va_end(ap);
      fprintf(stderr, "[gte] chip: %s -> %lld\n", q, (long long)answer);
    }
    return answer;
  }
  size_t step_lds_bytes(int epw, int stage) override {
    // (no trajectory row: planning has always run before a launch sets p.log)
    return said(gte::lds_image_bytes(epw, E->p.W, E->p.nd, E->cfg.final_obs != 0, false, stage),
                "step_lds_bytes epw=%d stage=%d", epw, stage);
  }
  int hot_per_cu(int store, size_t smem) override {
    return said(store == 1 ? gte::hot_blocks_per_cu_nt(smem) : gte::hot_blocks_per_cu(smem),
                "hot_per_cu store=%d smem=%zu", store, smem);
  }
  size_t resident_lds_bytes(int epb) override {
    return said(gte::resident_lds_bytes(E->p, epb), "resident_lds_bytes epb=%d", epb);
  }
  int resident_per_cu(int epb, int store) override {
    return said(gte::resident_blocks_per_cu(E->p, epb, store), "resident_per_cu epb=%d store=%d", epb, store);
  }
  int gather_per_cu(int epw, int store) override {
    Params q = E->p;
    q.epw = epw;
    return said(gte::rollout_blocks_per_cu(q, store), "gather_per_cu epw=%d store=%d", epw, store);
  }
};

// GTE_DEBUG_GEOMETRY: the whole plan on one line, after every moment that decides some of it
static void report_plan(const gte_env* E, const char* when) {
  if (debug_geometry()) gte_plan::print_plan(stderr, when, E->plan);
}

// gte_create: plan every launch, copy what the plan decides of Params, allocate what it asks for
static int plan_launches(gte_env* E) {
  LaunchPlan& L = E->plan;
  Params& p = E->p;
  const gte_plan::Shape shape = plan_shape(E);
  DeviceChip chip(E);
  L = gte_plan::plan_create(shape, read_knobs(KNOBS_CREATE), chip);
  p.epw = L.epw; p.lean_rows = L.lean_rows; p.hot_lds = L.hot_lds; p.debug = L.debug;
  if (L.affinity_period > 0) {
    const size_t N = (size_t)p.N;
    std::vector<int32_t> slot_of_rank(N);
    gte_plan::fill_slot_of_rank(shape, L.epw, slot_of_rank.data());
    TRY(dev_alloc(E, &E->d_perm, N, false));
    TRY(dev_alloc(E, &E->d_slot_of_rank, N, false));
    TRY(dev_alloc(E, &E->d_bins, (size_t)2 * p.D * L.n_bins_per_ds));  // histogram (zero-filled) + cursors
    if (hipMemcpy(E->d_slot_of_rank, slot_of_rank.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice) !=
        hipSuccess)
      return fail(GTE_ERR_HIP, "copying slot_of_rank failed");
  }
  return GTE_OK;
}

extern "C" {

int gte_abi_version(void) { return GTE_ABI_VERSION; }

const char* gte_last_error(void) { return g_err.c_str(); }

int gte_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gte_create(const gte_config* cfg, gte_env** out) {
  if (!out) return fail(GTE_ERR_INVALID, "out is NULL");
  *out = nullptr;
  TRY(validate(cfg));
  int n_cu = 0;
  TRY(require_device(cfg->device, &n_cu));
  HIPCHK(hipSetDevice(cfg->device));
  gte_env* E = new (std::nothrow) gte_env();
  if (!E) return fail(GTE_ERR_OOM, "host allocation failed");
  E->cfg = *cfg;
  E->n_cu = n_cu;
  memset(&E->p, 0, sizeof(Params));
  memset(&E->owned, 0, sizeof(gte_outputs));
  Params& p = E->p;
  p.N = cfg->n_envs;
  p.D = cfg->n_datasets;
  p.Fs = cfg->n_static;
  p.nd = cfg->n_dyn;
  p.Fobs = p.Fs + p.nd;
  p.has_window = cfg->window > 0;
  p.W = p.has_window ? cfg->window : 1;
  p.P = cfg->n_positions;
  for (int i = 0; i < GTE_MAX_DYN; ++i) p.dyn_kind[i] = cfg->dyn_kind[i];
  p.init_pos_index = cfg->initial_position_index;
  p.max_dur = cfg->max_episode_duration;
  p.reward_kind = cfg->reward_kind;
  p.autoreset = cfg->autoreset;
  p.switch_every = cfg->episodes_between_dataset_switch;
  p.persist = cfg->dyn_persist ? 1 : 0;
  p.fees = cfg->trading_fees;
  p.rate = cfg->borrow_interest_rate;
  p.V0 = cfg->portfolio_initial_value;
  p.rp0 = cfg->reward_param0;
  p.rp1 = cfg->reward_param1;
  p.rp2 = cfg->reward_param2;
  p.seed = cfg->seed;
  p.env_id_base = cfg->env_id_base;

  int rc = GTE_OK;
  auto chk = [&](int r) { if (rc == GTE_OK) rc = r; };
  const size_t N = (size_t)p.N;
  chk(hipStreamCreateWithFlags(&E->own_stream, hipStreamNonBlocking) == hipSuccess
          ? GTE_OK : fail(GTE_ERR_HIP, "hipStreamCreate failed"));
  E->stream = E->own_stream;
  chk(hipEventCreate(&E->ev0) == hipSuccess && hipEventCreate(&E->ev1) == hipSuccess
          ? GTE_OK : fail(GTE_ERR_HIP, "hipEventCreate failed"));
  chk(dev_alloc(E, &p.rec, N));  // zero-filled: every counter starts at 0
  // the datasets each env has picked in its current round of D (gte_device.h, pick_dataset)
  if (p.D > 1) {
    const size_t words = N * (size_t)((p.D + 31) / 32);
    chk(words <= 0xFFFFFFFFull ? GTE_OK : fail(GTE_ERR_INVALID, "n_envs x ceil(n_datasets / 32) must be < 2^32"));
    chk(dev_alloc(E, &p.ds_used, words));
  }
  chk(alloc_soa(E, &E->soa, N));
  // (the library's own observation buffers are allocated on first use, ensure_owned_obs: a caller
  // that binds its own — the torch path — never pays for a second copy of [N, W, F_obs])
  if (cfg->final_obs) {
    chk(dev_alloc(E, &p.final_rec, N));
    chk(alloc_soa(E, &E->fsoa, N));
  }
  {  // reward f32 [N] | terminated u8 [N] | truncated u8 [N] in ONE buffer of 6N bytes: the
     // layout a sharded run all-gathers as it is (gte_allgather_returns), no packing kernel
    uint8_t* packed = nullptr;
    chk(dev_alloc(E, &packed, 6 * N + 16));
    E->owned.reward = (float*)packed;
    E->owned.terminated = packed ? packed + 4 * N : nullptr;
    E->owned.truncated = packed ? packed + 5 * N : nullptr;
  }
  chk(dev_alloc(E, &E->owned.reward64, N));
  chk(dev_alloc(E, &E->owned.term_count, 2)); chk(dev_alloc(E, &E->owned.term_ids, N));
  chk(dev_alloc(E, &E->d_actions, N)); chk(dev_alloc(E, &E->d_mask, N));
  chk(dev_alloc(E, &E->d_inj_idx, N)); chk(dev_alloc(E, &E->d_inj_pos, N));
  chk(dev_alloc(E, &E->d_inj_ds, N));
  if (cfg->log_steps > 0) {
    const size_t LN = (size_t)cfg->log_steps * N;
    chk(dev_alloc(E, &E->log.rows, LN));  // 80 B per (row, env)
    chk(dev_alloc(E, &E->log_cursor, 2));  // (hipMalloc: 256-byte aligned, as the slot pair needs)
    p.log_L = cfg->log_steps;
  }
  double* d_pos = nullptr;
  chk(dev_alloc(E, &d_pos, GTE_MAX_POSITIONS));
  chk(dev_alloc(E, &E->d_ds, (size_t)p.D));
  if (rc == GTE_OK &&
      hipMemcpy(d_pos, cfg->positions, sizeof(double) * p.P, hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(GTE_ERR_HIP, "copying positions failed");
  if (rc != GTE_OK) return create_failed(E, rc);
  p.positions = d_pos;
  p.ds = E->d_ds;
  E->owned.obs_elems_per_env = (int64_t)p.W * p.Fobs;
  // the observation buffers come later (ensure_owned_obs / gte_bind_outputs)
  p.final_obs = nullptr;
  p.obs = nullptr; p.reward = E->owned.reward; p.reward64 = E->owned.reward64;
  p.obs_rows = p.W; p.obs_head = 0; p.slide = 0;  // classic layout until gte_bind_sliding_obs
  p.terminated = E->owned.terminated; p.truncated = E->owned.truncated;
  E->term_base = E->owned.term_count; p.term_ids = E->owned.term_ids;
  E->h_ds.assign((size_t)p.D, DatasetDesc{nullptr, nullptr, nullptr, nullptr, 0});
  for (auto& v : E->ds_allocs) v = std::vector<DeviceBlock>((size_t)p.D);

  rc = plan_launches(E);
  if (rc != GTE_OK) return create_failed(E, rc);
  // the zero-fills above ran on the null stream; the env's stream is non-blocking
  if (hipDeviceSynchronize() != hipSuccess)
    return create_failed(E, fail(GTE_ERR_HIP, "hipDeviceSynchronize failed after allocation"));
  report_plan(E, "create");
  *out = E;
  return GTE_OK;
}

int gte_upload_dataset(gte_env* E, int32_t d, const float* feat, const double* close,
                       const double* high, const double* low, int64_t T) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  const Params& p = E->p;
  if (d < 0 || d >= p.D) return fail(GTE_ERR_INVALID, "dataset index %d out of range", d);
  if (!feat || !close) return fail(GTE_ERR_INVALID, "feat and close are required");
  if (T <= 0 || T > 0x7FFFFFF0ll) return fail(GTE_ERR_INVALID, "T out of range");
  // the conditions under which the reference's reset/step are defined (:171-177)
  const int64_t idx0 = p.has_window ? p.W - 1 : 0;
  if (T < idx0 + 2) return fail(GTE_ERR_INVALID, "dataset of %lld rows is too short for windows=%d",
                                (long long)T, p.W);
  if (p.max_dur > 0 && T - p.max_dur - idx0 <= idx0)
    return fail(GTE_ERR_INVALID, "low >= high: %lld rows cannot host episodes of %d steps",
                (long long)T, p.max_dur);
  if (E->finalized && p.persist && T > p.depth)
    return fail(GTE_ERR_STATE, "dyn_persist: cannot upload a longer dataset after the first reset");
  // After a reset envs may sit anywhere in the old table: a shorter replacement would leave
  // their next step reading rows past the new allocation.  (The reference's own _set_df is only
  // ever followed by reset(); MultiDatasetTradingEnv's drop-in builds a fresh batch per dataset.)
  if (E->was_reset && T < E->h_ds[d].T)
    return fail(GTE_ERR_STATE, "dataset %d: cannot replace %lld rows by %lld after gte_reset "
                "(running environments may be past the new end); create a new env instead",
                d, (long long)E->h_ds[d].T, (long long)T);
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));
  const void* srcs[4] = {feat, close, high, low};
  const size_t bytes[4] = {sizeof(float) * (size_t)T * p.Fobs, sizeof(double) * (size_t)T,
                           sizeof(double) * (size_t)T, sizeof(double) * (size_t)T};
  // new buffers first; the old ones stay in the descriptor table (and valid) until the new
  // table has been published, so a failure on the way leaves the env exactly as it was
  DeviceBlock dev[4];  // (a return on the way releases them)
  for (int k = 0; k < 4; ++k) {
    if (!srcs[k]) continue;
    TRY(device_alloc(&dev[k], bytes[k], "uploading dataset %d: %s", d));
    if (getenv("GTE_DEBUG_ALLOC"))
      fprintf(stderr, "[gte] dataset %d column %d at %p, %zu bytes\n", d, k, dev[k].get(), bytes[k]);
    const hipError_t e = hipMemcpy(dev[k].get(), srcs[k], bytes[k], hipMemcpyHostToDevice);
    if (e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? GTE_ERR_OOM : GTE_ERR_HIP, "uploading dataset %d: %s", d,
                  hipGetErrorString(e));
  }
  const DatasetDesc before = E->h_ds[d];
  E->h_ds[d] = DatasetDesc{dev[0].as<const float>(), dev[1].as<const double>(), dev[2].as<const double>(),
                           dev[3].as<const double>(), T};
  const hipError_t e = hipMemcpy(E->d_ds, E->h_ds.data(), sizeof(DatasetDesc) * p.D, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    E->h_ds[d] = before;
    return fail(GTE_ERR_HIP, "publishing the descriptor of dataset %d: %s", d, hipGetErrorString(e));
  }
  for (int k = 0; k < 4; ++k) E->ds_allocs[k][d] = std::move(dev[k]);  // the old column is freed, the new one kept
  // T may have changed: the dataset's signal table was checked against the old one
  if (E->signals.d_tab && E->signals.h_tab[d].base) TRY(publish_signal_table(E, d, gte::SignalTable{nullptr, 0}));
  if (E->periods.d_row && E->periods.h_row[d].base) TRY(publish_period_row(E, d, DeviceBlock()));  // and its period row
  return GTE_OK;
}

static int finalize(gte_env* E) {
  if (E->finalized) return GTE_OK;
  Params& p = E->p;
  int64_t maxT = 0;
  for (int d = 0; d < p.D; ++d) {
    if (E->h_ds[d].T <= 0) return fail(GTE_ERR_STATE, "dataset %d was never uploaded", d);
    if (E->h_ds[d].T > maxT) maxT = E->h_ds[d].T;
  }
  p.depth = p.persist ? maxT : p.W;
  size_t table_bytes = 0;
  for (int d = 0; d < p.D; ++d) table_bytes += (size_t)E->h_ds[d].T * p.Fobs * sizeof(float);
  gte_plan::affinity_after_upload(E->plan, plan_shape(E), table_bytes);
  TRY(dev_alloc(E, &p.ring, (size_t)p.N * p.depth * (p.nd ? p.nd : 1)));
  HIPCHK(hipDeviceSynchronize());
  report_plan(E, "finalize");
  E->finalized = true;
  return GTE_OK;
}

// injected draws come from the caller: refuse values the kernel would use as
// out-of-range row / position / dataset indices
static int check_injection(const gte_env* E, size_t count, const int32_t* idx, const int32_t* pos,
                           const int32_t* ds) {
  const Params& p = E->p;
  int64_t maxT = 0, minT = INT64_MAX;
  for (int d = 0; d < p.D; ++d) {
    if (E->h_ds[d].T > maxT) maxT = E->h_ds[d].T;
    if (E->h_ds[d].T > 0 && E->h_ds[d].T < minT) minT = E->h_ds[d].T;
  }
  const int64_t idx0 = p.has_window ? p.W - 1 : 0;
  for (size_t i = 0; i < count; ++i) {
    if (pos && pos[i] >= p.P) return fail(GTE_ERR_INVALID, "injected position index %d >= %d", pos[i], p.P);
    if (ds && ds[i] >= p.D) return fail(GTE_ERR_INVALID, "injected dataset %d >= %d", ds[i], p.D);
    if (idx && idx[i] >= 0) {
      // an env needs at least one row after its start row; its dataset is known only when
      // it is injected too, otherwise the shortest dataset bounds it
      const int64_t T = (ds && ds[i] >= 0) ? E->h_ds[ds[i]].T : minT;
      if (idx[i] < idx0 || idx[i] > T - 2)
        return fail(GTE_ERR_INVALID, "injected start row %d outside [%lld, %lld]", idx[i],
                    (long long)idx0, (long long)(T - 2));
    }
  }
  return GTE_OK;
}

// append one trajectory row per env (after a reset or a step, whose Params p were; term_slot is
// the launch's slot).  mask (a masked reset once the log has a row): no row is appended, the masked
// envs' slot of the newest row is rewritten with their reset row, and the count stays.
static int append_log(gte_env* E, const Params& p, const uint8_t* mask = nullptr) {
  if (E->cfg.log_steps <= 0) return GTE_OK;
  if (E->log_rows == 0) mask = nullptr;
  HIPCHK(gte::launch_log(p.rec, p.reward64, p.terminated, p.truncated, p.N, E->log_cursor + (E->term_slot ^ 1),
                         E->cfg.log_steps, E->log, mask, E->stream));
  if (!mask) E->log_rows += 1;
  return GTE_OK;
}

// Before the host resets term_slot: log_cursor[slot] is the slot the next appending launch will
// read, so copy the count there from the slot the last launch wrote (stream-ordered, device to
// device: the count never passes through the host).
static int park_cursor(gte_env* E, int slot) {
  if (!E->log_cursor || E->term_slot == slot) return GTE_OK;
  HIPCHK(hipMemcpyAsync(E->log_cursor + slot, E->log_cursor + E->term_slot, sizeof(int64_t),
                        hipMemcpyDeviceToDevice, E->stream));
  return GTE_OK;
}

static int stage(gte_env* E, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, E->stream));
  return GTE_OK;
}

// The library's own observation buffers, on first need: nobody bound one (gte_bind_outputs) by
// the first gte_reset / gte_get_outputs, or a binding was withdrawn.
static int ensure_owned_obs(gte_env* E) {
  Params& p = E->p;
  const size_t elems = (size_t)p.N * (size_t)p.W * (size_t)p.Fobs;
  bool fresh = false;
  if (!p.obs) {
    if (!E->owned.obs) { TRY(dev_alloc(E, &E->owned.obs, elems)); fresh = true; }
    p.obs = E->owned.obs;
  }
  if (E->cfg.final_obs && !p.final_obs) {
    if (!E->owned.final_obs) { TRY(dev_alloc(E, &E->owned.final_obs, elems)); fresh = true; }
    p.final_obs = E->owned.final_obs;
  }
  if (fresh) HIPCHK(hipDeviceSynchronize());  // zero-filled on the null stream; E->stream is non-blocking
  return GTE_OK;
}

// Re-sort the processing order (gte_kernels.hip, "L2-affinity permutation").  The histogram is
// zero between re-sorts only because the scan kernel clears it: if a launch fails part-way it may be
// left counting, and a later scatter would hand out ranks past N.  So a failure turns the re-sort off
// for good and the env goes on in identity order (results do not depend on the order).
static int resort(gte_env* E) {
  E->steps_since_rebuild = 0;
  const hipError_t e = gte::launch_affinity_rebuild(E->p, E->d_bins, E->plan.n_bins_per_ds,
                                                    E->d_slot_of_rank, E->d_perm, E->stream);
  if (e != hipSuccess) {
    E->plan.affinity_period = 0;
    E->p.perm = nullptr;
    return fail(GTE_ERR_HIP, "re-sort of the processing order: %s", hipGetErrorString(e));
  }
  E->p.perm = E->d_perm;
  return GTE_OK;
}

int gte_reset(gte_env* E, const uint8_t* mask, const int32_t* inj_idx,
              const int32_t* inj_pos_index, const int32_t* inj_dataset) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(ensure_owned_obs(E));
  TRY(finalize(E));
  TRY(check_injection(E, (size_t)E->p.N, inj_idx, inj_pos_index, inj_dataset));
  Params p = E->p;  // (a masked reset writes the masked envs' windows at the current head)
  const bool fresh_run = E->sliding && !mask;  // every window is written: a fresh run of slides from head 0
  if (fresh_run) p.obs_head = 0;
  // masked envs get zero flags, flags_out untouched: the next step stores densely.  The window claim stands
  // through a masked reset; a fresh run gives it up until the launch below has gone out (a failed reset
  // proves nothing)
  ledger().wrote(E, {obs_span(E), flag_span(E, p.terminated), flag_span(E, p.truncated)}, false,
                 fresh_run ? FLAGS | WINDOW : FLAGS);
  const size_t N = (size_t)p.N;
  p.mask = nullptr; p.inj_idx = p.inj_pos = p.inj_ds = nullptr;
  if (mask) { TRY(stage(E, E->d_mask, mask, N)); p.mask = E->d_mask; }
  if (inj_idx) { TRY(stage(E, E->d_inj_idx, inj_idx, 4 * N)); p.inj_idx = E->d_inj_idx; }
  if (inj_pos_index) { TRY(stage(E, E->d_inj_pos, inj_pos_index, 4 * N)); p.inj_pos = E->d_inj_pos; }
  if (inj_dataset) { TRY(stage(E, E->d_inj_ds, inj_dataset, 4 * N)); p.inj_ds = E->d_inj_ds; }
  HIPCHK(hipMemsetAsync(E->term_base, 0, 2 * sizeof(int32_t), E->stream));
  TRY(park_cursor(E, 1));  // the reset's log row (slot 0) reads the count from slot 1
  E->term_slot = 0;
  p.term_count = E->term_base;
  p.term_count_next = E->term_base + 1;
  const LaunchPlan& L = E->plan;
  HIPCHK(gte::launch_reset(p, L.vec, L.store, L.coop, L.stage, L.blocks, L.threads, E->stream));
  if (fresh_run) {  // the buffer holds every env's window at head 0 now
    E->p.obs_head = 0;
    ledger().establish(E, WINDOW, {obs_span(E)}, false);
  }
  TRY(append_log(E, p, p.mask));
  if (L.affinity_period > 0) TRY(resort(E));  // new start rows: re-sort the processing order
  // host staging buffers may be reused by the caller right away: pageable copies above
  // are complete on return, but keep the contract simple and explicit
  HIPCHK(hipStreamSynchronize(E->stream));
  E->was_reset = true;
  return GTE_OK;
}

int gte_set_autoreset_injection(gte_env* E, int32_t n, const int32_t* inj_idx,
                                const int32_t* inj_pos_index, const int32_t* inj_dataset) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (n < 0) return fail(GTE_ERR_INVALID, "n_episodes must be >= 0");
  for (int d = 0; d < E->p.D; ++d)
    if (E->h_ds[d].T <= 0) return fail(GTE_ERR_STATE, "upload every dataset before queueing draws");
  TRY(check_injection(E, (size_t)E->p.N * (size_t)n, inj_idx, inj_pos_index, inj_dataset));
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(hipStreamSynchronize(E->stream));
  Params& p = E->p;
  const size_t count = (size_t)p.N * (size_t)n;
  // the queues of an earlier call are released here (the stream is idle: nothing reads them)
  auto put = [&](DeviceBlock* slot, const int32_t* src, const int32_t** param) -> int {
    *param = nullptr;
    slot->reset();  // (freed BEFORE the new queue is allocated)
    if (!src || n == 0) return GTE_OK;
    TRY(device_alloc(slot, sizeof(int32_t) * count, "queue of %zu injected draws: %s", count));
    void* const dev = slot->get();
    HIPCHK(hipMemcpy(dev, src, sizeof(int32_t) * count, hipMemcpyHostToDevice));
    *param = (const int32_t*)dev;
    return GTE_OK;
  };
  TRY(put(&E->d_q_idx, inj_idx, &p.q_idx));
  TRY(put(&E->d_q_pos, inj_pos_index, &p.q_pos));
  TRY(put(&E->d_q_ds, inj_dataset, &p.q_ds));
  p.q_n = n;
  HIPCHK(gte::launch_rewind_queue(p.rec, p.N, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));
  HIPCHK(hipDeviceSynchronize());
  return GTE_OK;
}

// two-slot terminal counter: this launch adds to one slot (cleared by the previous
// launch or by gte_reset) and clears the other, so no memset sits between steps
static void advance_term_slot(gte_env* E, Params& p) {
  E->term_slot ^= 1;
  p.term_count = E->term_base + E->term_slot;
  p.term_count_next = E->term_base + (E->term_slot ^ 1);
}

// What one step launch reads and writes: the env's own buffers (gte_step) or one row of a
// rollout's per-step buffers.  The actions are on the device.
struct StepTargets {
  const int32_t* actions;
  float *obs, *reward;
  double* reward64;
  uint8_t *terminated, *truncated;
  bool own_obs;  // obs is the env's own buffer (its layout and its window claim apply), not a rollout's row
};

static StepTargets own_targets(const gte_env* E, const int32_t* actions) {
  return {actions, E->p.obs, E->p.reward, E->p.reward64, E->p.terminated, E->p.truncated, true};
}

// The processing order ages with every step, fused or not: re-sort once it is due
static int age_order(gte_env* E, int32_t steps) {
  if (E->plan.affinity_period > 0 && (E->steps_since_rebuild += steps) >= E->plan.affinity_period) {
    // envs drift one row per step and ~1/duration of them jump at a reset: re-sort now and
    // then (3 tiny launches, stream-ordered between two steps)
    TRY(resort(E));
  }
  return GTE_OK;
}

// The one place a step is launched (gte_step; gte_rollout and gte_backtest one launch per step), with
// store policy `store`, or the plan's slide_store where the launch stores one row per env.  terminal_rec: terminal records for this launch where the env keeps none
// (gte_backtest in same-step mode).
static int enqueue_step(gte_env* E, const StepTargets& t, int store, bool capturing,
                        EnvRec* terminal_rec = nullptr) {
  const LaunchPlan& L = E->plan;
  const bool slides_own = t.own_obs && E->sliding;
  gte_ledger::Span obs = obs_span(E);
  // slide while the buffer provably holds this env's windows (its window claim) at a head below M;
  // otherwise (and at head M: the wrap) every window in full at head 0, which makes it so again
  const bool slide = slides_own && !capturing && ledger().holds(E, WINDOW, {obs}) && E->p.obs_head < L.slide_rows;
  // A launch that stores one row per env runs in env order: the L2-affinity order exists so that the
  // full-window gathers of one XCD hit its L2, and a slide reads one 128-byte table row per env; what the
  // order costs it is the hop perm[slot] -> rec[env] at the head of phase A and 64 scattered addresses per
  // wave instruction for every per-env store (reward, ring, flags).  Results do not depend on the order
  // (resort()); term_ids has no order contract (its users sort or scatter by id: terminal_ids() sorts).
  // A re-sort that falls due in a run of such launches waits for the next launch that writes full
  // windows — the wrap, or a full step after a withdrawn claim; steps_since_rebuild keeps counting.
  const bool env_order = slide && !L.full_windows && !(L.slide_ab & SLIDE_AB_ORDER);
  if (env_order) { if (L.affinity_period > 0) E->steps_since_rebuild += 1; }
  else TRY(age_order(E, 1));
  Params p = E->p;  // (after the re-sort: it sets p.perm)
  if (env_order) p.perm = nullptr;
  if (terminal_rec) p.final_rec = terminal_rec;
  p.actions = t.actions; p.obs = t.obs; p.reward = t.reward; p.reward64 = t.reward64;
  p.terminated = t.terminated; p.truncated = t.truncated;
  if (!t.own_obs) {  // a rollout's per-step row: a classic [N, W, F_obs] block
    p.obs_rows = p.W; p.obs_head = 0;
    obs = {t.obs, sizeof(float) * (size_t)p.N * p.W * p.Fobs};
  } else if (E->sliding) {
    if (slide) {
      E->p.obs_head += 1;
      // JOB_SLIDES shares bit 1 of the job record with dyn_persist's "zero the store" (gte_device.h):
      // plan_create (gte_plan.h) never grants slide_rows with dyn_persist, and only this launch ever sets p.slide
      if (p.persist || p.final_obs)
        return fail(GTE_ERR_STATE, "internal: a sliding step with dyn_persist or final_obs (the planner grants neither)");
      p.slide = L.full_windows ? 0 : 1;
    } else {
      E->p.obs_head = 0;
    }
    p.obs_head = E->p.obs_head;
  }
  advance_term_slot(E, p);
  if (L.fused_log) {
    p.log = E->log;
    p.log_cursor = E->log_cursor + (E->term_slot ^ 1);
  }
  // terminated / truncated: only the changed ones, where the env's flag claim proves the buffers hold the
  // previous step's flags (dense inside a capture: a replay cannot rely on what ran before it)
  const gte_ledger::Span term = flag_span(E, p.terminated), trunc = flag_span(E, p.truncated);
  p.flags_sparse = !capturing && !L.always_dense && ledger().holds(E, FLAGS, {term, trunc}) ? 1 : 0;
  // what this launch writes; its own claims hold again once it has gone out
  ledger().wrote(E, {obs, term, trunc}, capturing, FLAGS | WINDOW);
  // (hot_tu_covers: the isolated instantiations have no terminal records and no trajectory row)
  const bool hot = L.hot_tu && gte::hot_tu_covers(p);
  if (p.slide) store = L.slide_store;  // one row per env: the policy of its own (gte_plan.h)
  if (hot && store == 2)
    HIPCHK(gte::launch_step_hot(p, L.blocks, L.threads, gte::lds_bytes(p, L.stage), E->stream));
  else if (hot && store == 1)
    HIPCHK(gte::launch_step_hot_nt(p, L.blocks, L.threads, gte::lds_bytes(p, L.stage), E->stream));
  else
    HIPCHK(gte::launch_step(p, L.vec, store, L.coop, L.stage, L.blocks, L.threads, E->stream));
  ledger().establish(E, FLAGS, {term, trunc}, capturing);
  if (slides_own) ledger().establish(E, WINDOW, {obs}, capturing);
  if (L.fused_log) E->log_rows += 1;
  else TRY(append_log(E, p));
  return GTE_OK;
}

int gte_step(gte_env* E, const int32_t* actions, int32_t actions_on_device) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_step before gte_reset");
  if (!actions) return fail(GTE_ERR_INVALID, "actions is NULL");
  const bool capturing = stream_capturing(E);
  if (capturing && !actions_on_device)
    return fail(GTE_ERR_STATE, "gte_step on a capturing stream needs device-resident actions "
                               "(a copy from pageable host memory cannot be captured)");
  if (!actions_on_device) {
    TRY(stage(E, E->d_actions, actions, sizeof(int32_t) * (size_t)E->p.N));
    actions = E->d_actions;
  }
  return enqueue_step(E, own_targets(E, actions), E->plan.store, capturing);
}

// The host schedule a stream capture advances without running anything (term_slot, log_rows,
// steps_since_rebuild): saved before a capture and put back after it, whether it succeeded or not.
int gte_get_schedule(gte_env* E, gte_schedule* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  out->log_rows = E->log_rows;
  out->term_slot = E->term_slot;
  out->steps_since_rebuild = E->steps_since_rebuild;
  return GTE_OK;
}

int gte_set_schedule(gte_env* E, const gte_schedule* s) {
  if (!E || !s) return fail(GTE_ERR_INVALID, "NULL argument");
  if ((s->term_slot != 0 && s->term_slot != 1) || s->log_rows < 0 || s->steps_since_rebuild < 0)
    return fail(GTE_ERR_INVALID, "not a schedule gte_get_schedule returned");
  E->log_rows = s->log_rows;
  E->term_slot = s->term_slot;
  E->steps_since_rebuild = s->steps_since_rebuild;
  // captured steps may have been recorded as run: the next step stores densely, full windows at head 0
  ledger().withdraw(E, FLAGS | WINDOW);
  return GTE_OK;
}

int gte_advance_log(gte_env* E, int64_t rows) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  if (rows < 0) return fail(GTE_ERR_INVALID, "rows must be >= 0");
  E->log_rows += rows;
  return GTE_OK;
}

// GTE_DEBUG_GEOMETRY: name the path each gte_rollout call takes (the tests assert it)
static void report_rollout_path(const char* path, int32_t n_steps) {
  if (debug_geometry()) fprintf(stderr, "[gte] rollout path: %s, %d steps\n", path, n_steps);
}

// gte_rollout's launches, after its checks
static int rollout(gte_env* E, const int32_t* actions, int32_t n_steps, const gte_rollout_bufs* b) {
  const size_t N = (size_t)E->p.N;
  const size_t V = (size_t)E->p.W * (size_t)E->p.Fobs;
  const LaunchPlan& L = E->plan;
  // per-step observation rows are written once and not read back by the kernels: a stream
  // (non-temporal stores where the caller left the policy automatic)
  const int nt = (b->obs && E->cfg.nontemporal_obs == 3) ? 1 : L.store;
  const bool capturing = stream_capturing(E);
  // The fused kernels write the per-step rows and advance the envs without writing the env's own observation
  // buffer: the window claim goes (a step that goes out as an ordinary launch into the own buffer below
  // establishes it again).  They store the env's own flags densely, flags_out with them, so the flag claim
  // stands for the ordinary step launches below; gte_rollout withdraws it after the copies that follow them.
  const size_t rows = (size_t)n_steps * N;
  ledger().wrote(E, {{b->obs, sizeof(float) * rows * V}, {b->terminated, rows}, {b->truncated, rows},
                     flag_span(E, E->p.terminated), flag_span(E, E->p.truncated)}, capturing, WINDOW);
  // one step as its own launch, writing row k of every per-step buffer (what the unfused path
  // does for every step, and the backtest path for its last one)
  auto step_row = [&](int32_t k) -> int {
    StepTargets t = own_targets(E, actions + (size_t)k * N);
    if (b->obs) { t.obs = b->obs + (size_t)k * N * V; t.own_obs = false; }
    if (b->reward) t.reward = b->reward + (size_t)k * N;
    if (b->reward64) t.reward64 = b->reward64 + (size_t)k * N;
    if (b->terminated) t.terminated = b->terminated + (size_t)k * N;
    if (b->truncated) t.truncated = b->truncated + (size_t)k * N;
    TRY(enqueue_step(E, t, nt, capturing));
    if (b->valuation) {
      hipError_t e = gte::launch_extract_state(E->p.rec, E->p.N, E->soa, E->stream);
      if (e == hipSuccess)
        e = hipMemcpyAsync(b->valuation + (size_t)k * N, E->soa.pv, 8 * N, hipMemcpyDeviceToDevice,
                           E->stream);
      if (e != hipSuccess) return fail(GTE_ERR_HIP, "rollout: %s", hipGetErrorString(e));
    }
    return GTE_OK;
  };
  if (!L.fused_rollout) {
    // same results, one launch per step
    report_rollout_path("per-step", n_steps);
    for (int32_t k = 0; k < n_steps; ++k) TRY(step_row(k));
  } else if (!b->obs) {
    // Backtest: no observation is kept but the last one.  n_steps - 1 steps of pure state machine
    // from registers (gte_rollout_state_kernel), then the last step as an ordinary launch, which
    // also produces the observation and the terminal list.
    report_rollout_path(n_steps > 1 ? "state-only" : "per-step", n_steps);
    if (n_steps > 1) {
      TRY(age_order(E, n_steps - 1));
      gte::RolloutArgs r = {actions, n_steps - 1, nullptr, b->reward, b->reward64, b->terminated,
                            b->truncated, b->valuation, 0, 0, nullptr};
      // identity order: with no window to gather, the L2-affinity order would only scatter the
      // per-env loads and stores (actions, rewards, flags) that are coalesced in env order
      Params ps = E->p;
      ps.perm = nullptr;
      const hipError_t le = gte::launch_rollout_state(ps, r, n_steps - 1, L.state_epw, E->stream);
      if (le != hipSuccess) return fail(GTE_ERR_HIP, "rollout launch: %s", hipGetErrorString(le));
    }
    TRY(step_row(n_steps - 1));
  } else {
    TRY(age_order(E, n_steps));
    Params p = E->p;
    if (L.resident_epb[nt] == 0) {
      DeviceChip chip(E);
      gte_plan::choose_resident_epb(E->plan, plan_shape(E), read_knobs(KNOBS_ROLLOUT), chip, nt);
      report_plan(E, "resident");
    }
    advance_term_slot(E, p);
    report_rollout_path(L.resident_epb[nt] > 0 ? "resident" : "gather", n_steps);
    if (L.resident_epb[nt] > 0) {
      // identity processing order: the L2-affinity order exists for the table reads of the
      // per-step gather; here one row per env and step is read, and consecutive envs make each
      // workgroup's observation stores one contiguous run
      p.perm = nullptr;
      if (!E->d_group_counter) TRY(dev_alloc_late(E, &E->d_group_counter, 4));
      HIPCHK(hipMemsetAsync(E->d_group_counter, 0, sizeof(int32_t), E->stream));
      const int epb = L.resident_epb[nt];
      const int n_groups = (p.N + epb - 1) / epb;
      gte::RolloutArgs r = {actions, n_steps, b->obs, b->reward, b->reward64, b->terminated,
                            b->truncated, b->valuation, epb, n_groups, E->d_group_counter};
      const int blocks = n_groups < L.resident_slots[nt] ? n_groups : L.resident_slots[nt];
      const hipError_t le = gte::launch_rollout_resident(p, r, nt, blocks, E->stream);
      if (le != hipSuccess) return fail(GTE_ERR_HIP, "rollout launch: %s", hipGetErrorString(le));
    } else {
      if (L.rollout_epw == 0) {
        DeviceChip chip(E);
        gte_plan::choose_rollout_epw(E->plan, plan_shape(E), chip, nt);
        report_plan(E, "gather");
      }
      p.epw = L.rollout_epw;
      const int r_blocks = gte::rollout_blocks(p.N, p.epw);
      gte::RolloutArgs r = {actions, n_steps, b->obs, b->reward, b->reward64, b->terminated,
                            b->truncated, b->valuation, 0, 0, nullptr};
      const hipError_t le = gte::launch_rollout(p, r, nt, r_blocks, E->stream);
      if (le != hipSuccess) return fail(GTE_ERR_HIP, "rollout launch: %s", hipGetErrorString(le));
    }
  }
  // the env's own return buffers describe the last step
  const size_t last = (size_t)(n_steps - 1) * N;
  if (b->reward) HIPCHK(hipMemcpyAsync(E->p.reward, b->reward + last, 4 * N, hipMemcpyDeviceToDevice, E->stream));
  if (b->reward64) HIPCHK(hipMemcpyAsync(E->p.reward64, b->reward64 + last, 8 * N, hipMemcpyDeviceToDevice, E->stream));
  if (b->terminated) HIPCHK(hipMemcpyAsync(E->p.terminated, b->terminated + last, N, hipMemcpyDeviceToDevice, E->stream));
  if (b->truncated) HIPCHK(hipMemcpyAsync(E->p.truncated, b->truncated + last, N, hipMemcpyDeviceToDevice, E->stream));
  return GTE_OK;
}

int gte_rollout(gte_env* E, const int32_t* actions, int32_t n_steps, const gte_rollout_bufs* b) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_rollout before gte_reset");
  if (!actions) return fail(GTE_ERR_INVALID, "actions is NULL");
  if (n_steps < 1) return fail(GTE_ERR_INVALID, "n_steps must be >= 1");
  static const gte_rollout_bufs none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (!b) b = &none;
  if (b->obs && ((uintptr_t)b->obs & 15)) return fail(GTE_ERR_INVALID, "obs must be 16-byte aligned");
  HIPCHK(hipSetDevice(E->cfg.device));
  const int rc = rollout(E, actions, n_steps, b);
  ledger().withdraw(E, FLAGS);  // (the copies into the env's own flags follow the last step's launch)
  return rc;
}

}  // extern "C"
namespace gte_host {

thread_local std::string g_err = "";

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// gte_backtest's launches, after its checks: the steps of gte_rollout(actions, n_steps, NULL), each
// folded into the statistics records
// With actions == NULL (gte_backtest_signals) each step's actions are looked up in the bound signal tables
// for `strategy` instead.
// the lookup of gte_signal_actions, with the exits decided as well while rules are bound
hipError_t launch_lookup(gte_env* E, const int32_t* strategy, int32_t* actions) {
  if (E->signals.exits.rules)
    return gte::launch_exit_actions(E->p, E->signals.d_tab, E->signals.S, strategy, E->signals.exits, actions, E->stream);
  return gte::launch_signal_actions(E->p, E->signals.d_tab, E->signals.S, strategy, actions, E->stream);
}

// With `cv` (gte_backtest_curves) the launches are those of gte_curves.hip, which write the rows as well.
static int backtest(gte_env* E, const int32_t* actions, const int32_t* strategy, int32_t n_steps, int32_t clear,
                    gte::Curves* cv = nullptr) {
  const size_t N = (size_t)E->p.N;
  const LaunchPlan& L = E->plan;
  const bool signals = actions == nullptr;
  // the summary kernels advance the envs without writing observations: the window claim goes (the ordinary
  // step launches below establish it again).  They store the env's own flags densely, so the flag claim
  // stands for those launches; backtest_entry withdraws it afterwards
  ledger().wrote(E, {flag_span(E, E->p.terminated), flag_span(E, E->p.truncated)}, false, WINDOW);
  if (signals && !E->backtest.sig_actions) TRY(dev_alloc_late(E, &E->backtest.sig_actions, N));
  if (cv) {  // the window that is open between two launches of a call (gte_curves.hip), allocated by the first such call
    if (!E->backtest.carry) TRY(dev_alloc_late(E, &E->backtest.carry, N));
    cv->carry = E->backtest.carry;
  }
  if (!E->backtest.stats) {
    if (E->p.autoreset == GTE_AUTORESET_SAME_STEP && !E->p.final_rec) TRY(dev_alloc(E, &E->backtest.final_rec, N));
    TRY(dev_alloc_late(E, &E->backtest.stats, N));  // (its wait covers the fill before it too)
    clear = 1;
  }
  // tracking was switched since the last call: both records start afresh, so that they cover the same transitions
  if (E->trades.changed) clear = 1;
  E->trades.changed = false;
  gte_trade_stats* const trades = E->trades.on ? E->trades.stats : nullptr;
  // ... with the trade list on, through the unit that writes it as well (gte_trade_list.hip)
  const bool listed = trades && E->trades.cap > 0;
  const gte::TradeList tl = {E->trades.list.as<gte_trade>(), E->trades.open_row.as<int32_t>(), E->trades.cap};
  // the same for period tracking (never on together with trades: gte_track_periods, gte_track_trades)
  if (E->periods.changed) clear = 1;
  E->periods.changed = false;
  const bool periods = E->periods.B > 0;
  const gte::Periods per = {E->periods.d_row, E->periods.stats.as<gte_period_stats>(), E->periods.B};
  // same-step mode: the terminal valuation comes from the terminal records, the env's or our own
  EnvRec* const terminal = E->p.final_rec ? E->p.final_rec : E->backtest.final_rec;
  Params ps = E->p;
  ps.perm = nullptr;  // identity order, as in the state-only rollout: per-env loads and stores coalesce
  ps.final_rec = terminal;
  hipError_t le = listed   ? gte::launch_trade_list_begin(ps, E->backtest.stats, trades, tl, clear, E->stream)
                  : trades ? gte::launch_trade_begin(ps, E->backtest.stats, trades, clear, E->stream)
                           : gte::launch_backtest_begin(ps, E->backtest.stats, clear, E->stream);
  if (le != hipSuccess) return fail(GTE_ERR_HIP, "backtest launch: %s", hipGetErrorString(le));
  if (periods && clear)  // a cleared period record is all zero, and a reset row changes none
    HIPCHK(hipMemsetAsync(per.records, 0, sizeof(gte_period_stats) * N * (size_t)E->periods.B, E->stream));
  // one step as an ordinary launch (it also produces the observation and the terminal list), then
  // its results into the records
  auto step_and_fold = [&](int32_t k) -> int {
    if (signals) {
      const hipError_t se = launch_lookup(E, strategy, E->backtest.sig_actions);
      if (se != hipSuccess) return fail(GTE_ERR_HIP, "backtest launch: %s", hipGetErrorString(se));
    }
    const int32_t* const row = signals ? E->backtest.sig_actions : actions + (size_t)k * N;
    TRY(enqueue_step(E, own_targets(E, row), L.store, false, E->backtest.final_rec));
    const hipError_t fe = cv        ? gte::launch_curve_fold(ps, E->backtest.stats, *cv, k, n_steps, E->stream)
                          : listed  ? gte::launch_trade_list_fold(ps, E->backtest.stats, trades, tl, E->stream)
                          : trades  ? gte::launch_trade_fold(ps, E->backtest.stats, trades, E->stream)
                          : periods ? gte::launch_period_fold(ps, E->backtest.stats, per, E->stream)
                                    : gte::launch_backtest_fold(ps, E->backtest.stats, E->stream);
    if (fe != hipSuccess) return fail(GTE_ERR_HIP, "backtest launch: %s", hipGetErrorString(fe));
    return GTE_OK;
  };
  if (!L.fused_rollout) {
    report_rollout_path(cv ? "backtest curves per-step" : signals ? "backtest signals per-step" : "backtest per-step",
                        n_steps);
    for (int32_t k = 0; k < n_steps; ++k) TRY(step_and_fold(k));
    return GTE_OK;
  }
  if (cv) report_rollout_path(n_steps > 1 ? "backtest curves summary" : "backtest curves per-step", n_steps);
  else if (signals) report_rollout_path(n_steps > 1 ? "backtest signals summary" : "backtest signals per-step", n_steps);
  else report_rollout_path(n_steps > 1 ? "backtest summary" : "backtest per-step", n_steps);
  if (n_steps > 1) {
    TRY(age_order(E, n_steps - 1));
    // one launch, its actions from `src`; with a tracker on, the unit that keeps that record in registers as well
    const gte::SummarySource src = {actions, E->signals.d_tab, E->signals.S, strategy, E->signals.exits.rules ? &E->signals.exits : nullptr};
    const int32_t k = n_steps - 1, epw = L.state_epw;
    le = cv        ? gte::launch_curve_summary(ps, src, E->backtest.stats, *cv, k, epw, E->stream)
         : listed  ? gte::launch_trade_list_summary(ps, src, E->backtest.stats, trades, tl, k, epw, E->stream)
         : trades  ? gte::launch_trade_summary(ps, src, E->backtest.stats, trades, k, epw, E->stream)
         : periods ? gte::launch_period_summary(ps, src, E->backtest.stats, per, k, epw, E->stream)
         : signals ? gte::launch_signal_summary(ps, src, E->backtest.stats, k, epw, E->stream)
                   : gte::launch_backtest_summary(ps, src, E->backtest.stats, k, epw, E->stream);
    if (le != hipSuccess) return fail(GTE_ERR_HIP, "backtest launch: %s", hipGetErrorString(le));
  }
  return step_and_fold(n_steps - 1);
}

// what gte_backtest and gte_backtest_signals (`who`) share once their own arguments are checked
int backtest_entry(gte_env* E, const char* who, const int32_t* actions, const int32_t* strategy,
                          int32_t n_steps, int32_t clear, gte_backtest_stats** stats_device,
                   gte::Curves* cv) {
  if (n_steps < 1) return fail(GTE_ERR_INVALID, "n_steps must be >= 1");
  if (stream_capturing(E))
    return fail(GTE_ERR_STATE, "%s inside a stream capture: a backtest is one launch already, run it eagerly", who);
  if (E->periods.B > 0)
    for (int d = 0; d < E->p.D; ++d)
      if (!E->periods.d_row || !E->periods.h_row[d].base)
        return fail(GTE_ERR_STATE, "%s: period tracking is on and dataset %d has no period row (gte_bind_periods)", who, d);
  HIPCHK(hipSetDevice(E->cfg.device));
  const int rc = backtest(E, actions, strategy, n_steps, clear, cv);
  ledger().withdraw(E, FLAGS);  // (as after a rollout: the next step stores densely)
  if (stats_device) *stats_device = E->backtest.stats;
  return rc;
}

}  // namespace gte_host
extern "C" {

int gte_add_limit_orders(gte_env* E, const int32_t* pos_index, const double* limit,
                         const uint8_t* persistent) {
  if (!E || !pos_index || !limit) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_add_limit_orders before gte_reset");
  Params& p = E->p;
  for (int d = 0; d < p.D; ++d)
    if (!E->h_ds[d].high || !E->h_ds[d].low)
      return fail(GTE_ERR_STATE, "limit orders need high/low columns in dataset %d", d);
  const size_t N = (size_t)p.N;
  for (size_t i = 0; i < N; ++i)
    if (pos_index[i] >= p.P) return fail(GTE_ERR_INVALID, "pos_index[%zu] out of range", i);
  HIPCHK(hipSetDevice(E->cfg.device));
  if (!p.lo_pos) {  // first use: allocate the order tables (the counts live in EnvRec)
    int32_t* lo_pos = nullptr;
    TRY(dev_alloc(E, &lo_pos, N * p.P));
    TRY(dev_alloc(E, &p.lo_limit, N * p.P));
    TRY(dev_alloc(E, &p.lo_persist, N * p.P));
    TRY(dev_alloc(E, &E->d_lo_limit_in, N));
    TRY(dev_alloc(E, &E->d_lo_persist_in, N));
    HIPCHK(hipDeviceSynchronize());
    p.lo_pos = lo_pos;
  }
  TRY(stage(E, E->d_inj_pos, pos_index, 4 * N));
  TRY(stage(E, E->d_lo_limit_in, limit, 8 * N));
  if (persistent) TRY(stage(E, E->d_lo_persist_in, persistent, N));
  HIPCHK(gte::launch_add_orders(p, E->d_inj_pos, E->d_lo_limit_in,
                                persistent ? E->d_lo_persist_in : nullptr, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));  // host arrays and staging buffers are free again
  return GTE_OK;
}

int gte_get_outputs(gte_env* E, gte_outputs* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(E->cfg.device));
  TRY(ensure_owned_obs(E));
  const Params& p = E->p;
  out->obs = p.obs;  // (the BASE of a sliding buffer: gte_obs_view says where the window is)
  out->reward = p.reward; out->reward64 = p.reward64;
  out->terminated = p.terminated; out->truncated = p.truncated;
  out->term_count = E->term_base; out->term_ids = p.term_ids;
  out->obs_elems_per_env = (int64_t)p.W * p.Fobs;
  out->term_slot = E->term_slot;
  out->reserved0 = 0;
  out->final_obs = p.final_obs;
  return GTE_OK;
}

int gte_bind_outputs(gte_env* E, const gte_outputs* b) {
  if (!E || !b) return fail(GTE_ERR_INVALID, "NULL argument");
  HIPCHK(hipStreamSynchronize(E->stream));
  Params& p = E->p;
  if (b->obs && ((uintptr_t)b->obs & 15)) return fail(GTE_ERR_INVALID, "obs must be 16-byte aligned");
  E->sliding = false;  // back to the classic layout, whatever was bound
  p.obs_rows = p.W; p.obs_head = 0;
  p.obs = b->obs;  // NULL: back to the library's own buffers (allocated on first need)
  ledger().wrote(E, {obs_span(E)}, false, FLAGS | WINDOW);  // (other envs that slide in that buffer stop)
  if (E->cfg.final_obs) p.final_obs = b->final_obs;
  if (E->was_reset) TRY(ensure_owned_obs(E));
  p.reward = b->reward ? b->reward : E->owned.reward;
  p.reward64 = b->reward64 ? b->reward64 : E->owned.reward64;
  p.terminated = b->terminated ? b->terminated : E->owned.terminated;
  p.truncated = b->truncated ? b->truncated : E->owned.truncated;
  E->term_base = b->term_count ? b->term_count : E->owned.term_count;  // i32 [2]
  HIPCHK(hipMemset(E->term_base, 0, 2 * sizeof(int32_t)));
  TRY(park_cursor(E, 0));  // the next step (slot 1) reads the log's count from slot 0
  HIPCHK(hipDeviceSynchronize());
  E->term_slot = 0;
  p.term_ids = b->term_ids ? b->term_ids : E->owned.term_ids;
  return GTE_OK;
}

int gte_obs_view(gte_env* E, gte_obs_view_t* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  out->base = E->p.obs;
  out->rows_per_env = E->p.obs_rows;
  out->head = E->p.obs_head;
  out->sliding = E->sliding ? 1 : 0;
  out->slack_rows = E->plan.slide_rows;
  return GTE_OK;
}

int gte_bind_sliding_obs(gte_env* E, float* base, int32_t rows_per_env) {
  if (!E || !base) return fail(GTE_ERR_INVALID, "NULL argument");
  const LaunchPlan& L = E->plan;
  if (L.slide_rows <= 0)
    return fail(GTE_ERR_STATE, "this env does not slide (gte_obs_view().slack_rows is 0): bind a classic buffer");
  Params& p = E->p;
  if (rows_per_env != p.W + L.slide_rows)
    return fail(GTE_ERR_INVALID, "rows_per_env must be window + slack_rows = %d", p.W + L.slide_rows);
  if ((uintptr_t)base & 15) return fail(GTE_ERR_INVALID, "obs must be 16-byte aligned");
  if (stream_capturing(E)) return fail(GTE_ERR_STATE, "gte_bind_sliding_obs inside a stream capture");
  HIPCHK(hipStreamSynchronize(E->stream));
  p.obs = base;
  p.obs_rows = rows_per_env;
  p.obs_head = 0;
  E->sliding = true;
  // the next step writes every window in full at head 0 (and other envs that slide in that buffer stop)
  ledger().wrote(E, {obs_span(E)}, false, WINDOW);
  return GTE_OK;
}

int gte_bind_returns(gte_env* E, float* reward, uint8_t* terminated, uint8_t* truncated) {
  if (!E || !reward || !terminated || !truncated) return fail(GTE_ERR_INVALID, "NULL argument");
  // Params travel by value with every launch: later launches see the new pointers,
  // launches already enqueued keep the old ones.
  ledger().withdraw(E, FLAGS);  // (rotated buffers hold an older step's flags: the next step stores densely)
  E->p.reward = reward;
  E->p.terminated = terminated;
  E->p.truncated = truncated;
  return GTE_OK;
}

// the state lives in 128-byte records; snapshot it into struct-of-arrays mirrors
// (stream-ordered: the views reflect every launch enqueued before this call)
static int state_view(gte_env* E, const EnvRec* rec, const gte::StateSoA& o, gte_state_view* out) {
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_extract_state(rec, E->p.N, o, E->stream));
  out->idx = o.idx; out->step = o.step; out->position_index = o.pos;
  out->dataset_index = o.dsi; out->start_idx = o.start; out->episode = o.episode;
  out->needs_reset = o.needs_reset; out->asset = o.asset; out->fiat = o.fiat;
  out->interest_asset = o.ia; out->interest_fiat = o.ifi;
  out->portfolio_valuation = o.pv; out->real_position = o.realpos;
  return GTE_OK;
}

int gte_get_state(gte_env* E, gte_state_view* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  return state_view(E, E->p.rec, E->soa, out);
}

int gte_set_dynamic_features(gte_env* E, const float* values_device, uint32_t mask) {
  if (!E || !values_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_set_dynamic_features before gte_reset");
  if (E->p.nd <= 0 || (mask >> E->p.nd) != 0u)
    return fail(GTE_ERR_INVALID, "mask 0x%x names features beyond n_dyn = %d", mask, E->p.nd);
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_set_dynamic(E->p, values_device, mask, E->stream));
  return GTE_OK;
}

int gte_set_dynamic_columns(gte_env* E, const void* const* columns_device, const int32_t* is_f64) {
  if (!E || !columns_device || !is_f64) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_set_dynamic_columns before gte_reset");
  if (E->p.nd <= 0) return fail(GTE_ERR_INVALID, "the env has no dynamic features");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_set_dynamic_columns(E->p, columns_device, is_f64, E->stream));
  return GTE_OK;
}

int gte_get_final_state(gte_env* E, gte_state_view* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->p.final_rec) return fail(GTE_ERR_STATE, "created without final_obs");
  return state_view(E, E->p.final_rec, E->fsoa, out);
}

int gte_set_stream(gte_env* E, void* hip_stream) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipStreamSynchronize(E->stream));
  E->stream = (hipStream_t)hip_stream;  // NULL = the null stream, used as such
  return GTE_OK;
}

int gte_use_own_stream(gte_env* E) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipStreamSynchronize(E->stream));
  E->stream = E->own_stream;
  return GTE_OK;
}

int gte_synchronize(gte_env* E) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipStreamSynchronize(E->stream));
  return GTE_OK;
}

int gte_timer_start(gte_env* E) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  HIPCHK(hipEventRecord(E->ev0, E->stream));
  return GTE_OK;
}

int gte_timer_stop(gte_env* E, float* elapsed_ms) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!elapsed_ms) {  // mark only: record the end now (asynchronous), read it with a later call
    HIPCHK(hipEventRecord(E->ev1, E->stream));
    E->timer_marked = true;
    return GTE_OK;
  }
  if (!E->timer_marked) HIPCHK(hipEventRecord(E->ev1, E->stream));
  E->timer_marked = false;
  HIPCHK(hipEventSynchronize(E->ev1));
  HIPCHK(hipEventElapsedTime(elapsed_ms, E->ev0, E->ev1));
  return GTE_OK;
}

int gte_get_launch_info(gte_env* E, int32_t* envs_per_wave, int32_t* threads_per_block,
                        int32_t* n_blocks, int32_t* vector_bytes) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (envs_per_wave) *envs_per_wave = E->p.epw;
  const LaunchPlan& L = E->plan;
  if (threads_per_block) *threads_per_block = L.threads;
  if (n_blocks) *n_blocks = L.blocks;
  if (vector_bytes)
    *vector_bytes = L.vec * 4 + 1000 * ((L.coop ? 1 : 0) + 2 * L.stage + 16 * L.store + 64 * (L.hot_per_cu & 15) +
                                        1024 * (E->sliding ? L.slide_store : L.store));
  return GTE_OK;
}

#ifdef GTE_STAMPS
// diagnostic build only: device buffer of u64 [n_blocks, 8] for the kernel's time stamps
int gte_debug_set_stamps(gte_env* E, void* device_buf) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  E->p.inj_ds = (const int32_t*)device_buf;
  return GTE_OK;
}
#endif

void gte_destroy(gte_env* E) {
  if (!E) return;
  (void)hipSetDevice(E->cfg.device);
  (void)gte_comm_destroy(E);
  (void)hipStreamSynchronize(E->stream);
  if (E->own_stream) (void)hipStreamSynchronize(E->own_stream);
  for (void* ptr : E->allocs) if (ptr) device_free(ptr);
  if (E->ev0) (void)hipEventDestroy(E->ev0);
  if (E->ev1) (void)hipEventDestroy(E->ev1);
  if (E->own_stream) (void)hipStreamDestroy(E->own_stream);
  ledger().forget(E);
  delete E;  // (with every block the env may replace: the owners of gte_host.h)
}

}  // extern "C"
