// gte_api_read.hip — the read-back entry points of include/gte.h: the trajectory log (its view, its host-side
// reads, the reward written into it) and the env snapshots, observations and plain copies to the host.
#include "gte_host.h"

extern "C" {

int gte_get_log(gte_env* E, gte_log_view* out) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  gte::LogRow* r = E->log.rows;  // the columns as strided views of the [L, N] rows
  out->idx = &r->idx; out->step = &r->step; out->position_index = &r->pos;
  out->dataset_index = &r->dsi; out->portfolio_valuation = &r->pv;
  out->real_position = &r->realpos; out->reward = &r->reward; out->flags = &r->flags;
  out->rows = E->log_rows; out->L = E->cfg.log_steps; out->N = E->p.N;
  out->asset = &r->asset; out->fiat = &r->fiat;
  out->interest_asset = &r->ia; out->interest_fiat = &r->ifi;
  out->env_stride = (int64_t)sizeof(gte::LogRow);
  out->row_stride = (int64_t)sizeof(gte::LogRow) * E->p.N;
  out->cursor = E->log_cursor; out->cursor_slot = E->term_slot; out->reserved0 = 0;
  return GTE_OK;
}

// rows first .. first+n-1 (mod L) of ONE env, oldest first: at most two strided 2-D copies per array
static int pull_log_column(gte_env* E, int32_t env_id, int64_t first, int32_t n, void* host,
                           size_t offset, size_t elem) {
  if (!host) return GTE_OK;
  const int N = E->p.N, L = E->cfg.log_steps;
  const size_t pitch = sizeof(gte::LogRow) * (size_t)N;  // the same env, one row later
  const char* col = (const char*)E->log.rows + offset + sizeof(gte::LogRow) * (size_t)env_id;
  const int64_t run1 = (first + n <= L) ? n : (L - first);
  HIPCHK(hipMemcpy2D(host, elem, col + (size_t)first * pitch, pitch, elem, (size_t)run1,
                     hipMemcpyDeviceToHost));
  if (run1 < n)
    HIPCHK(hipMemcpy2D((char*)host + run1 * elem, elem, col, pitch, elem, (size_t)(n - run1),
                       hipMemcpyDeviceToHost));
  return GTE_OK;
}

static int log_window(gte_env* E, int32_t env_id, int32_t* n, int32_t* n_out, int64_t* first) {
  if (!E || !n_out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  const int N = E->p.N, L = E->cfg.log_steps;
  if (env_id < 0 || env_id >= N) return fail(GTE_ERR_INVALID, "env_id out of range");
  const int64_t have = E->log_rows < L ? E->log_rows : L;
  if (*n > have) *n = (int32_t)have;
  if (*n < 0) *n = 0;
  *n_out = *n;
  *first = *n ? (E->log_rows - *n) % L : 0;
  if (*n) {
    HIPCHK(hipSetDevice(E->cfg.device));
    HIPCHK(hipStreamSynchronize(E->stream));
  }
  return GTE_OK;
}

int gte_read_log(gte_env* E, int32_t env_id, int32_t n, int32_t* idx, int32_t* step,
                 int32_t* position_index, int32_t* dataset_index, double* portfolio_valuation,
                 double* real_position, double* reward, uint8_t* flags, int32_t* n_out) {
  int64_t first = 0;
  TRY(log_window(E, env_id, &n, n_out, &first));
  if (n == 0) return GTE_OK;
  TRY(pull_log_column(E, env_id, first, n, idx, offsetof(gte::LogRow, idx), 4));
  TRY(pull_log_column(E, env_id, first, n, step, offsetof(gte::LogRow, step), 4));
  TRY(pull_log_column(E, env_id, first, n, position_index, offsetof(gte::LogRow, pos), 4));
  TRY(pull_log_column(E, env_id, first, n, dataset_index, offsetof(gte::LogRow, dsi), 4));
  TRY(pull_log_column(E, env_id, first, n, portfolio_valuation, offsetof(gte::LogRow, pv), 8));
  TRY(pull_log_column(E, env_id, first, n, real_position, offsetof(gte::LogRow, realpos), 8));
  TRY(pull_log_column(E, env_id, first, n, reward, offsetof(gte::LogRow, reward), 8));
  TRY(pull_log_column(E, env_id, first, n, flags, offsetof(gte::LogRow, flags), 1));
  return GTE_OK;
}

int gte_read_log_portfolio(gte_env* E, int32_t env_id, int32_t n, double* asset, double* fiat,
                           double* interest_asset, double* interest_fiat, int32_t* n_out) {
  int64_t first = 0;
  TRY(log_window(E, env_id, &n, n_out, &first));
  if (n == 0) return GTE_OK;
  TRY(pull_log_column(E, env_id, first, n, asset, offsetof(gte::LogRow, asset), 8));
  TRY(pull_log_column(E, env_id, first, n, fiat, offsetof(gte::LogRow, fiat), 8));
  TRY(pull_log_column(E, env_id, first, n, interest_asset, offsetof(gte::LogRow, ia), 8));
  TRY(pull_log_column(E, env_id, first, n, interest_fiat, offsetof(gte::LogRow, ifi), 8));
  return GTE_OK;
}

int gte_read_log_envs(gte_env* E, const int32_t* env_ids, int32_t n_ids, int32_t max_rows,
                      int32_t finished, gte_log_batch* out) {
  if (!E || !env_ids || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  if (n_ids < 0) return fail(GTE_ERR_INVALID, "n_ids must be >= 0");
  if (finished && !E->p.final_rec)
    return fail(GTE_ERR_STATE, "finished episodes need autoreset = same-step with final_obs");
  const int N = E->p.N, L = E->cfg.log_steps;
  if (max_rows <= 0 || max_rows > L) max_rows = L;
  for (int32_t i = 0; i < n_ids; ++i)
    if (env_ids[i] < 0 || env_ids[i] >= N) return fail(GTE_ERR_INVALID, "env_ids[%d] = %d out of range", i, env_ids[i]);
  memset(out, 0, sizeof *out);
  out->n_ids = n_ids; out->max_rows = max_rows;
  if (n_ids == 0) return GTE_OK;
  HIPCHK(hipSetDevice(E->cfg.device));
  // [ids i32 n | n_rows i32 n | pad -> 16] [7 f64 columns] [4 i32 columns] [u8 column]
  const size_t cells = (size_t)n_ids * (size_t)max_rows;
  const size_t head = (((size_t)n_ids * 8) + 15) & ~(size_t)15;
  const size_t need = head + cells * (7 * 8 + 4 * 4 + 1);
  if (need > E->readback.logpack.bytes())  // pinned and mapped: the kernel writes host memory directly
    TRY(pinned_alloc(&E->readback.logpack, gte_own::grow_by_half(E->readback.logpack.bytes(), need), hipHostMallocMapped));
  char* b = E->readback.logpack.as<char>();
  int32_t* ids = (int32_t*)b;
  memcpy(ids, env_ids, sizeof(int32_t) * (size_t)n_ids);
  gte::LogPack o;
  o.n_rows = ids + n_ids;
  double* f = (double*)(b + head);
  o.pv = f; o.realpos = f + cells; o.reward = f + 2 * cells; o.asset = f + 3 * cells;
  o.fiat = f + 4 * cells; o.ia = f + 5 * cells; o.ifi = f + 6 * cells;
  int32_t* w = (int32_t*)(f + 7 * cells);
  o.idx = w; o.step = w + cells; o.pos = w + 2 * cells; o.dsi = w + 3 * cells;
  o.flags = (uint8_t*)(w + 4 * cells);
  HIPCHK(gte::launch_pack_log(E->log, N, L, (long long)E->log_rows, ids, n_ids, max_rows, finished ? 1 : 0,
                              E->cfg.autoreset == GTE_AUTORESET_DISABLED ? 1 : 0,
                              E->p.final_rec, E->p.reward64, o, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));
  out->n_rows = o.n_rows;
  out->idx = o.idx; out->step = o.step; out->position_index = o.pos; out->dataset_index = o.dsi;
  out->portfolio_valuation = o.pv; out->real_position = o.realpos; out->reward = o.reward;
  out->asset = o.asset; out->fiat = o.fiat; out->interest_asset = o.ia; out->interest_fiat = o.ifi;
  out->flags = o.flags;
  return GTE_OK;
}

int gte_set_log_reward(gte_env* E, const double* reward_device) {
  if (!E || !reward_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  if (E->log_rows <= 0) return fail(GTE_ERR_STATE, "the log is empty");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_set_log_reward(E->log.rows, E->log_cursor + E->term_slot, E->cfg.log_steps, E->p.N,
                                    reward_device, E->stream));
  return GTE_OK;
}

int gte_apply_reward(gte_env* E, const double* reward_device, int32_t terminal_view) {
  if (!E || !reward_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (E->cfg.log_steps <= 0) return fail(GTE_ERR_STATE, "created with log_steps = 0");
  if (E->log_rows <= 0) return fail(GTE_ERR_STATE, "the log is empty");
  HIPCHK(hipSetDevice(E->cfg.device));
  HIPCHK(gte::launch_apply_reward(E->p, reward_device, E->log.rows, E->log_cursor + E->term_slot,
                                  terminal_view ? 1 : 0, E->stream));
  return GTE_OK;
}

static_assert(sizeof(gte_env_snapshot) == 96, "gte_env_snapshot layout");

static int read_envs_impl(gte_env* E, int32_t first, int32_t count, int32_t want_obs,
                          const gte_env_snapshot** out, const float** obs, bool hands_out_views) {
  if (!E || !out) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->was_reset) return fail(GTE_ERR_STATE, "gte_read_envs before gte_reset");
  if (first < 0 || count < 1 || (int64_t)first + count > E->p.N)
    return fail(GTE_ERR_INVALID, "envs %d..%lld out of range", first, (long long)first + count - 1);
  if (want_obs && !obs) return fail(GTE_ERR_INVALID, "obs is NULL");
  HIPCHK(hipSetDevice(E->cfg.device));
  const size_t elems = (size_t)E->p.W * (size_t)E->p.Fobs;
  const size_t head = sizeof(gte_env_snapshot) * (size_t)count;  // 96 B each: 16-byte aligned
  const size_t need = head + (want_obs ? sizeof(float) * elems * (size_t)count : 0);
  // Callers may hold views into the staging buffer: once it exists at full size it is never
  // reallocated, so size it for the whole batch the first time a buffer is made.
  const size_t full = (sizeof(gte_env_snapshot) + sizeof(float) * elems) * (size_t)E->p.N;
  if (hands_out_views) E->readback.view_reads = true;
  const size_t want = E->readback.view_reads ? full : need;
  if (want > E->readback.snap.bytes())  // pinned and mapped: the kernel writes host memory directly
    TRY(pinned_alloc(&E->readback.snap, gte_own::grow_exact(E->readback.snap.bytes(), want), hipHostMallocMapped));
  float* h_obs = (float*)(E->readback.snap.as<char>() + head);
  HIPCHK(gte::launch_snapshot(E->p.rec, E->p.reward64, E->p.terminated, E->p.truncated, obs_window0(E->p),
                              (int64_t)elems, obs_env_stride(E->p), first, count, E->readback.snap.get(),
                              want_obs ? h_obs : nullptr, E->stream));
  HIPCHK(hipStreamSynchronize(E->stream));
  *out = E->readback.snap.as<const gte_env_snapshot>();
  if (obs) *obs = want_obs ? h_obs : nullptr;
  return GTE_OK;
}

int gte_read_envs_view(gte_env* E, int32_t first, int32_t count, int32_t want_obs,
                       const gte_env_snapshot** out, const float** obs) {
  return read_envs_impl(E, first, count, want_obs, out, obs, true);
}

int gte_read_envs(gte_env* E, int32_t first, int32_t count, gte_env_snapshot* out, float* obs) {
  if (!out) return fail(GTE_ERR_INVALID, "NULL argument");
  const gte_env_snapshot* snaps = nullptr;
  const float* h_obs = nullptr;
  TRY(read_envs_impl(E, first, count, obs ? 1 : 0, &snaps, &h_obs, false));
  memcpy(out, snaps, sizeof(gte_env_snapshot) * (size_t)count);
  if (obs) memcpy(obs, h_obs, sizeof(float) * (size_t)E->p.W * (size_t)E->p.Fobs * (size_t)count);
  return GTE_OK;
}

int gte_read_env(gte_env* E, int32_t e, gte_env_snapshot* out, float* obs) {
  return gte_read_envs(E, e, 1, out, obs);
}

int gte_read_obs(gte_env* E, int32_t first_env, int32_t n, float* host_dst) {
  if (!E || !host_dst) return fail(GTE_ERR_INVALID, "NULL argument");
  const Params& p = E->p;
  if (first_env < 0 || n < 0 || (int64_t)first_env + n > p.N)
    return fail(GTE_ERR_INVALID, "env range [%d, %d) out of [0, %d)", first_env, first_env + n, p.N);
  const size_t per = (size_t)p.W * p.Fobs;
  if (!p.obs) return fail(GTE_ERR_STATE, "gte_read_obs before gte_reset (no observation exists yet)");
  HIPCHK(hipStreamSynchronize(E->stream));
  const size_t stride = (size_t)obs_env_stride(p);
  const float* src = obs_window0(p) + stride * first_env;
  if (stride == per || n == 0)  // classic buffer: one contiguous copy
    HIPCHK(hipMemcpy(host_dst, src, sizeof(float) * per * n, hipMemcpyDeviceToHost));
  else
    HIPCHK(hipMemcpy2D(host_dst, sizeof(float) * per, src, sizeof(float) * stride, sizeof(float) * per, (size_t)n,
                       hipMemcpyDeviceToHost));
  return GTE_OK;
}

int gte_copy_to_host(gte_env* E, const void* device_src, void* host_dst, uint64_t bytes) {
  if (!E || !device_src || !host_dst) return fail(GTE_ERR_INVALID, "NULL argument");
  HIPCHK(hipStreamSynchronize(E->stream));
  HIPCHK(hipMemcpy(host_dst, device_src, (size_t)bytes, hipMemcpyDeviceToHost));
  return GTE_OK;
}

}  // extern "C"
