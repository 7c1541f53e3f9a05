// gte_kernels.hip — the step / reset kernels of libgte (gfx950 / CDNA4 only).
//
// One launch advances every environment of the shard by one step
// (TradingEnv.step, reference environments.py:233-272) or resets the masked
// ones (TradingEnv.reset, :163-199).  Workgroup = 256 threads = 4 wavefronts =
// 64 environments at windowed shapes; two kinds of work:
//
//   phase A  one lane per environment: the scalar fp64 state machine
//            (_take_action/_trade -> Portfolio.trade_to_position ->
//            limit-order fills -> update_interest -> valorisation ->
//            done/truncated -> reward), auto-reset with Philox or injected
//            draws, wave-level compaction of the terminal mask (__ballot +
//            popcount prefix, one atomic per wave).  The per-env state is one
//            128-byte record, reached through the L2-affinity permutation.
//   gather   _get_obs (:152-160): the window of env e is ONE contiguous block of
//            W*F_obs floats of the row-major feature table, moved with 16-byte
//            loads / non-temporal stores (1 KiB per wave instruction) and patched
//            in flight with the dynamic columns, which the wave first stages in
//            LDS with one coalesced pass over its envs' small dynamic stores.
//
// Kernels:  gte_kernel<MODE,...>     phase A (gte_phase_a.h), LDS barrier, gather (gte_step.h, with the
//                                    template): every step and reset shape is instantiated and launched
//                                    here (the headline instantiation is compiled alone in
//                                    gte_hot.hip / gte_hot_nt.hip, from gte_hot_body.h);
//           gte_rollout.hip          K steps in one launch: gte_rollout_resident_kernel (windows
//                                    resident in LDS), gte_rollout_state_kernel (no observations),
//                                    gte_rollout_kernel (gather per step; shapes LDS cannot hold);
//           gte_backtest.hip         K steps in one launch into per-env statistics (phase A alone);
//           gte_affinity_*           counting sort of the envs by table region
//                                    (processing order, speed only);
//           gte_add_orders / gte_extract_state / gte_rewind_queue: small helpers.
//
// The path is HBM-bound (no contraction, so no MFMA): >= 97 % of its bytes are the
// window gather + observation store.  See DESIGN.md for roofline and measurements.
#include "gte_step.h"

namespace gte {

// TradingEnv.add_limit_order, environments.py:227-231: `orders[position] = {...}` — an
// existing key (a position VALUE) keeps its place in the iteration order, a new one
// goes last.  One thread per env.
__global__ void gte_add_orders_kernel(const Params p, const int32_t* pos_index,
                                      const double* limit, const uint8_t* persistent) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  const int32_t pi = pos_index[e];
  if (pi < 0) return;
  int32_t* lp = p.lo_pos + (int64_t)e * p.P;
  const int n = p.rec[e].lo_n;
  int j = 0;
  while (j < n && p.positions[lp[j]] != p.positions[pi]) ++j;
  if (j == n) p.rec[e].lo_n = n + 1;  // n < P: at most one order per distinct position value
  lp[j] = pi;
  p.lo_limit[(int64_t)e * p.P + j] = limit[e];
  p.lo_persist[(int64_t)e * p.P + j] = persistent ? persistent[e] : 0;
}

// ---------------------------------------------------------------------------
// L2-affinity permutation.  Workgroups are dealt round-robin over the 8 XCDs, each
// with a private 4 MiB L2 (workgroup b and b+8 share one; observed behaviour, used
// for speed only).  A 12.8 MB feature table does not fit one L2, and with random
// starts every XCD reads all of it (measured: 146 MB of L2 misses per step).  If the
// envs processed by XCD x all sit in the x-th eighth of the (dataset, row) space,
// each L2 only has to hold 1/8 of the table and the window reads hit it (measured
// 42 us vs 54 us per step, profiles/r01_tune_affinity_potential.log).  perm[slot] =
// env is a counting sort of the envs by (dataset, row bucket), laid out so that the
// r-th env in sorted order goes to the r-th slot in XCD-major order (slot_of_rank,
// built on the host).  Results do not depend on the permutation; only speed does.
__global__ void gte_affinity_hist_kernel(const Params p, int32_t* hist, int n_bins_per_ds) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  const int d = p.rec[e].dsi;
  const int64_t T = p.ds[d].T;
  int b = (int)(((int64_t)p.rec[e].idx * n_bins_per_ds) / T);
  b = b < 0 ? 0 : (b >= n_bins_per_ds ? n_bins_per_ds - 1 : b);
  atomicAdd(&hist[d * n_bins_per_ds + b], 1);
}

// exclusive scan of `hist` (n_bins <= 1024 * per_thread) by one workgroup, into `cursor`; the
// histogram is left ZEROED for the next re-sort (no memset launch per re-sort: the array is
// zero-filled when it is allocated, and this kernel is its only reader)
__global__ __launch_bounds__(1024) void gte_affinity_scan_kernel(int32_t* hist, int32_t* cursor, int n_bins) {
  __shared__ int32_t part[1024];
  const int t = threadIdx.x;
  const int per = (n_bins + 1023) / 1024;
  const int lo = t * per, hi = min(n_bins, lo + per);
  int32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += hist[i];
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const int32_t v = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int32_t run = part[t] - sum;  // exclusive prefix of this thread's chunk
  for (int i = lo; i < hi; ++i) {
    const int32_t c = hist[i];
    hist[i] = 0;
    cursor[i] = run;
    run += c;
  }
}

__global__ void gte_affinity_scatter_kernel(const Params p, int32_t* cursor, int n_bins_per_ds,
                                            const int32_t* slot_of_rank, int32_t* perm_out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  const int d = p.rec[e].dsi;
  const int64_t T = p.ds[d].T;
  int b = (int)(((int64_t)p.rec[e].idx * n_bins_per_ds) / T);
  b = b < 0 ? 0 : (b >= n_bins_per_ds ? n_bins_per_ds - 1 : b);
  const int rank = atomicAdd(&cursor[d * n_bins_per_ds + b], 1);
  perm_out[slot_of_rank[rank]] = e;
}

hipError_t launch_affinity_rebuild(const Params& p, int32_t* bins, int n_bins_per_ds,
                                   const int32_t* slot_of_rank, int32_t* perm_out,
                                   hipStream_t stream) {
  // bins: [0, n_bins) the histogram (zero between re-sorts), [n_bins, 2 n_bins) the scatter's cursors
  const int n_bins = p.D * n_bins_per_ds;
  const int blocks = (p.N + 255) / 256;
  hipLaunchKernelGGL(gte_affinity_hist_kernel, dim3(blocks), dim3(256), 0, stream, p, bins,
                     n_bins_per_ds);
  hipLaunchKernelGGL(gte_affinity_scan_kernel, dim3(1), dim3(1024), 0, stream, bins, bins + n_bins, n_bins);
  hipLaunchKernelGGL(gte_affinity_scatter_kernel, dim3(blocks), dim3(256), 0, stream, p, bins + n_bins,
                     n_bins_per_ds, slot_of_rank, perm_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// struct-of-arrays views of the state for the host (gte_get_state): StateSoA, gte_launch.h
__global__ void gte_extract_state_kernel(const EnvRec* rec, int n, StateSoA o) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const EnvRec r = rec[e];
  o.idx[e] = r.idx; o.step[e] = r.step; o.pos[e] = r.pos; o.dsi[e] = r.dsi;
  o.start[e] = r.start; o.episode[e] = r.episode; o.needs_reset[e] = r.needs_reset;
  o.asset[e] = r.asset; o.fiat[e] = r.fiat; o.ia[e] = r.ia; o.ifi[e] = r.ifi;
  o.pv[e] = r.pv; o.realpos[e] = r.realpos;
}

hipError_t launch_extract_state(const EnvRec* rec, int n, const StateSoA& o, hipStream_t stream) {
  hipLaunchKernelGGL(gte_extract_state_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, rec, n, o);
  return hipGetLastError();
}

__global__ void gte_rewind_queue_kernel(EnvRec* rec, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) rec[e].q_head = 0;
}

hipError_t launch_rewind_queue(EnvRec* rec, int n, hipStream_t stream) {
  hipLaunchKernelGGL(gte_rewind_queue_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, rec, n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// launchers (called from gte_api.hip)

size_t lds_image_bytes(int epw, int W, int nd, bool final_obs, bool log_row, int stage) {
  const size_t EPB = (size_t)epw * GTE_WAVES;
  size_t b = EPB * (16 + 64 + 4 * GTE_MAX_DYN + 4) + (final_obs ? EPB * sizeof(FinalJob) : 0) +
             (log_row ? EPB * sizeof(LogRow) : 0);
  if (stage) b += EPB * (size_t)W * (size_t)(nd ? nd : 1) * 4;
  return b;
}

size_t lds_bytes(const Params& p, int stage) {
  return lds_image_bytes(p.epw, p.W, p.nd, p.final_obs != nullptr, p.log.rows != nullptr, stage);
}

template <int MODE>
static hipError_t launch_mode(const Params& p, int vec, int nt, bool coop, int stage,
                              int blocks, int threads, hipStream_t stream) {
  const uint32_t V = (uint32_t)(p.W * p.Fobs);
  const uint64_t vm = magic40(V / vec), fm = magic40((uint32_t)p.Fobs / vec);
  const uint64_t wm = magic40((uint32_t)(p.W * (p.nd ? p.nd : 1)));
  const size_t smem = lds_bytes(p, stage);
#define GTE_L(VEC, NT, CO, ST) \
  hipLaunchKernelGGL((gte_kernel<MODE, VEC, NT, CO, ST>), dim3(blocks), dim3(threads), smem, \
                     stream, p, vm, fm, wm)
#define GTE_L_ST(VEC, NT, CO) do { if (stage == STAGE_RAW) GTE_L(VEC, NT, CO, STAGE_RAW); \
    else if (stage == STAGE_LATE) GTE_L(VEC, NT, CO, STAGE_LATE); else GTE_L(VEC, NT, CO, STAGE_NONE); } while (0)
#define GTE_L_CO(VEC, NT) do { if (coop) GTE_L_ST(VEC, NT, true); else GTE_L_ST(VEC, NT, false); } while (0)
#define GTE_L_NT(VEC) do { if (nt == 2) GTE_L_CO(VEC, 2); else if (nt == 1) GTE_L_CO(VEC, 1); \
                           else GTE_L_CO(VEC, 0); } while (0)
  if (vec == 4) GTE_L_NT(4); else GTE_L_NT(1);
#undef GTE_L_NT
#undef GTE_L_CO
#undef GTE_L_ST
#undef GTE_L
  return hipGetLastError();
}

hipError_t launch_add_orders(const Params& p, const int32_t* pos_index, const double* limit,
                             const uint8_t* persistent, hipStream_t stream) {
  hipLaunchKernelGGL(gte_add_orders_kernel, dim3((p.N + 255) / 256), dim3(256), 0, stream, p,
                     pos_index, limit, persistent);
  return hipGetLastError();
}

hipError_t launch_step(const Params& p, int vec, int nt, bool coop, int stage, int blocks,
                       int threads, hipStream_t stream) {
  return launch_mode<MODE_STEP>(p, vec, nt, coop, stage, blocks, threads, stream);
}

hipError_t launch_reset(const Params& p, int vec, int nt, bool coop, int stage, int blocks,
                        int threads, hipStream_t stream) {
  return launch_mode<MODE_RESET>(p, vec, nt, coop, stage, blocks, threads, stream);
}

}  // namespace gte
