// gte_step.h — the step / reset kernel template: phase A (gte_phase_a.h), LDS barrier, phase B (the
// window gather: fastdiv40, store_out, ring staging, the copy loops, final_windows) and
// gte_kernel<MODE, VEC, NT, COOP, STAGE> itself.  Instantiated by gte_kernels.hip (every shape),
// gte_hot.hip / gte_hot_nt.hip (the headline one alone) and gte_rollout.hip (its device functions).
#pragma once
#include "gte_phase_a.h"

namespace gte {


// ---------------------------------------------------------------------------
// phase B

__device__ inline uint32_t fastdiv40(uint32_t k, uint64_t magic) {
  return (uint32_t)(((uint64_t)k * magic) >> 40);
}

// Observation store policy (gte_config.nontemporal_obs): 0 plain, 1 non-temporal,
// 2 sc1.  tools/store_bench.hip on MI355X, 168 MB store-only: plain 26 us, nt 33 us,
// sc1 23-24 us; plain stores evict the feature table from L2, nt/sc1 do not (an sc1
// store drops the line from L2).  sc1 needs inline asm: the compiler does not count it
// on vmcnt, so every place that relies on "my stores are done" waits explicitly.
template <int NT, typename T>
__device__ inline void store_out(T* dst, const T& v) {
  if constexpr (NT == 2 && sizeof(T) == 16) {
    // no "memory" clobber: nothing in the kernel reads obs back, and volatile asms keep
    // their order among themselves (the s_waitcnt before the barrier stays behind them)
    // s_nop 1: a VMEM store of more than 64 bits reads its data registers for a couple of cycles
    // after it issues; a VALU write to them in that window corrupts the stored value (gfx9 / CDNA
    // hazard "VMEM store > 8 bytes followed by a write of the VGPRs holding the data").  hipcc pads
    // its own stores, but it does not look inside inline asm: without the two wait states here the
    // lean copy loop stored the next address computation's low words in place of x, y.
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v));
  } else if constexpr (NT == 2) {
    const float f = __builtin_bit_cast(float, v);  // 1-element vector: plain VGPR operand
    asm volatile("global_store_dword %0, %1, off sc1" ::"v"(dst), "v"(f));
  } else if constexpr (NT == 1) {
    __builtin_nontemporal_store(v, dst);
  } else {
    *dst = v;
  }
}

// The window's source pointer travels through LDS as a 64-bit integer, which makes the
// compiler forget that it points to global memory: it then emits flat_load, and flat
// loads count on vmcnt AND lgkmcnt (every LDS read in the loop waits for them).  Cast
// back to the global address space explicitly.
template <typename T>
__device__ inline T load_global(uint64_t base, int64_t index) {
  typedef const T __attribute__((address_space(1))) * gptr_t;
  return ((gptr_t)base)[index];
}

// Put nd dynamic values x[0..nd) into vector v, which is the LAST vector of a window row.
// With 16-byte vectors F_obs % 4 == 0 and nd <= 4, so the dynamic columns are exactly the
// last nd components of that vector: a wave-uniform switch, no per-component compares.
__device__ inline void set_tail(float __attribute__((ext_vector_type(4))) & v, int nd,
                                const float x[GTE_MAX_DYN]) {
  switch (nd) {  // wave-uniform
    case 1: v[3] = x[0]; break;
    case 2: v[2] = x[0]; v[3] = x[1]; break;
    case 3: v[1] = x[0]; v[2] = x[1]; v[3] = x[2]; break;
    default: v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3]; break;
  }
}

// LDS image of a workgroup: the jobs phase A hands to phase B (one per env of the
// workgroup) and, when STAGE, the dynamic-column values of every window row.
// One 16-byte job record per env of the workgroup: a single ds_read_b128 per vector in
// the copy loop (five separate LDS reads measurably throttled the loop).
struct alignas(16) JobRec {
  uint64_t src;   // first row of the window in the feature table
  int32_t env;    // env id processed in this slot (perm[slot], or the slot itself); -1 = none
  uint32_t meta;  // bit0 copy the window, bit1 zero the env's dynamic store (dyn_persist) / JOB_SLIDES,
                  // bits 2..16 n_zero (W < 32768, gte_create checks), bits 17..31 slot0 of the
                  // W-deep ring (meaningless with dyn_persist: dyn_value uses the row itself)
};
__device__ inline uint32_t pack_meta(int flags, int n_zero, int slot0) {
  return (uint32_t)(flags & 3) | ((uint32_t)n_zero << 2) | ((uint32_t)slot0 << 17);
}
__device__ inline int meta_flags(uint32_t m) { return (int)(m & 3u); }
__device__ inline int meta_n_zero(uint32_t m) { return (int)((m >> 2) & 0x7FFFu); }
__device__ inline int meta_slot0(uint32_t m) { return (int)(m >> 17); }

// LDS image of a workgroup: the jobs phase A hands to phase B (one per env of the
// workgroup) and, when staged, the dynamic-column values of every window row.
struct WgLds {
  JobRec* job;      // [EPB]
  unsigned char* hot;  // [EPB][64] the records' hot halves as phase A leaves them (flush_hot_records)
  int32_t* idx;     // [EPB] current row (persist mode's zero-fill needs it)
  float* cur;       // [EPB][GTE_MAX_DYN] dynamic features of the current row
  FinalJob* fin;    // [EPB] terminal windows (only when p.final_obs)
  unsigned char* logrow;  // [EPB][sizeof(LogRow)] the step's trajectory rows (only when p.log.rows; flush_log_rows)
  float* staged;    // [EPB][W][nd]: the raw rings; the lean copy loop resolves a wave's part IN
                    // PLACE into window order (rotation / zero rows / current row applied)
};

__device__ inline WgLds carve_lds(unsigned char* base, int EPB, bool with_final, bool with_log) {
  WgLds L;
  L.job = (JobRec*)base;                   base += 16 * EPB;
  L.hot = base;                            base += 64 * EPB;
  L.cur = (float*)base;                    base += 4 * GTE_MAX_DYN * EPB;
  L.idx = (int32_t*)base;                  base += 4 * EPB;
  L.logrow = base;                         base += with_log ? sizeof(LogRow) * EPB : 0;  // (16-byte aligned here)
  L.fin = (FinalJob*)base;                 base += with_final ? sizeof(FinalJob) * EPB : 0;
  L.staged = (float*)base;
  return L;
}

// The records' hot halves, from the LDS image phase A left (store_state_lds) to the records: four
// lanes per env, i.e. one 64-byte request per env where the lane that stepped the env issued four
// 16-byte stores to 64 different lines each.
__device__ inline void flush_hot_records(const Params& p, const WgLds& L, int s_first, int n_env, int lane) {
  typedef float __attribute__((ext_vector_type(4))) f4;
  for (int i = lane; i < n_env * 4; i += 64) {  // (one pass with 16 envs per wave)
    const int sl = s_first + (i >> 2), part = i & 3;
    const int env = L.job[sl].env;  // (>= 0 for the first n_env slots)
    const f4 v = *reinterpret_cast<const f4*>(L.hot + 64 * sl + 16 * part);
    *(reinterpret_cast<f4*>(&p.rec[env]) + part) = v;
  }
}

// The step's trajectory rows, from the LDS image phase A's lanes left to the log: five lanes per env
// (80 contiguous bytes, two requests per env where the twelve columns were twelve).
__device__ inline void flush_log_rows(const Params& p, const WgLds& L, int s_first, int n_env, int lane) {
  typedef float __attribute__((ext_vector_type(4))) f4;
  const int64_t row_base = log_row(*p.log_cursor, p.log_L) * (int64_t)p.N;  // env 0 of the row (uniform)
  for (int i = lane; i < n_env * 5; i += 64) {
    const int q = i / 5, part = i - q * 5;
    const int sl = s_first + q;
    const int env = L.job[sl].env;  // (>= 0 for the first n_env slots)
    const f4 v = *reinterpret_cast<const f4*>(L.logrow + sizeof(LogRow) * sl + 16 * part);
    *(reinterpret_cast<f4*>(&p.log.rows[row_base + env]) + part) = v;
  }
}

// phase A's lane publishes its env's job (the env id was written at kernel start)
__device__ inline void publish_job(const WgLds& L, int slot, const ObsJob& job) {
  L.job[slot].src = (uint64_t)job.src;
  L.job[slot].meta = pack_meta(job.flags, job.n_zero, job.slot0);
  L.idx[slot] = job.idx;
#pragma unroll
  for (int i = 0; i < GTE_MAX_DYN; ++i) L.cur[slot * GTE_MAX_DYN + i] = job.cur[i];
}

// value of dynamic feature i in window row w of the env in LDS slot `s` (generic form:
// reads the env's store in global memory; used by the persist-mode staging and when
// nothing is staged)
__device__ inline float dyn_value(const Params& p, const WgLds& L, int s, const float* ring_e,
                                  int w, int i) {
  if (w == p.W - 1) return L.cur[s * GTE_MAX_DYN + i];  // current row: from phase A
  const uint32_t m = L.job[s].meta;
  if (w < meta_n_zero(m)) return 0.0f;                   // never written: reads as zero
  int32_t slot;
  if (p.persist) {
    // T-deep column: the slot IS the table row, which does not fit JobRec.meta's 15 bits
    // (rows >= 32768 used to alias): take it from the current row published next to the job
    slot = L.idx[s] - p.W + 1 + w;
  } else {
    slot = meta_slot0(m) + w;
    if (slot >= p.W) slot -= p.W;
  }
  return ring_e[(int64_t)slot * p.nd + i];
}

// The wave gathers, once and coalesced, the dynamic-column values of all window rows
// of its envs into LDS (W*nd floats per env: 160 B at the headline shape), so that the
// copy loop patches from LDS instead of issuing divergent global loads per vector.
__device__ inline void stage_dynamic(const Params& p, const WgLds& L, int s_first,
                                     int n_env, int lane, uint64_t wnd_magic) {
  const uint32_t WND = (uint32_t)(p.W * p.nd);
  const uint32_t total = (uint32_t)n_env * WND;
  for (uint32_t k = (uint32_t)lane; k < total; k += 64u) {
    const uint32_t el = fastdiv40(k, wnd_magic);
    const uint32_t r = k - el * WND;
    const uint32_t w = r / (uint32_t)p.nd;
    const int i = (int)(r - w * (uint32_t)p.nd);
    const int s = s_first + (int)el;
    const float* ring_e = p.ring + (int64_t)L.job[s].env * p.depth * p.nd;
    L.staged[(uint32_t)s * WND + r] = dyn_value(p, L, s, ring_e, (int)w, i);
  }
}

// STAGE_RAW: at kernel start every wave copies the W-deep rings of its envs — one
// contiguous block of EPW*W*nd floats — into LDS (coalesced, and its latency hides
// behind phase A); the slot rotation / zero rows / current row are resolved when a
// vector is patched.  STAGE_LATE (dyn_persist: the rows sit at idx-dependent offsets
// of a T-deep column): gathered after phase A, already resolved (stage_dynamic).
enum { STAGE_NONE = 0, STAGE_RAW = 1, STAGE_LATE = 2 };

__device__ inline void stage_raw_rings(const Params& p, const WgLds& L, int s_first, int n_env,
                                       int lane, uint64_t wnd_magic) {
  const uint32_t WND = (uint32_t)(p.W * p.nd);
  const uint32_t total = (uint32_t)n_env * WND;
  float* dst = L.staged + (uint32_t)s_first * WND;
  for (uint32_t k = (uint32_t)lane; k < total; k += 64u) {
    const uint32_t el = fastdiv40(k, wnd_magic);
    const uint32_t r = k - el * WND;
    dst[k] = p.ring[(int64_t)L.job[s_first + (int)el].env * WND + r];  // depth == W here
  }
}

// Overwrite the dynamic columns that vector `v` (columns col .. col+VEC-1 of window
// row w of the env in LDS slot s, job meta m) covers.  Straight-line code under ONE
// branch: nested divergent branches here cost ~250 instructions and a dozen
// s_waitcnt per vector.  Every index into v is a compile-time constant after
// unrolling: a run-time index would put v in scratch memory (measured: one scratch
// store per observation store, 2x WRITE_SIZE).
template <int VEC, int STAGE, typename vec_t>
__device__ inline void patch_dynamic(const Params& p, const WgLds& L, vec_t& v, int s, uint32_t m,
                                     const float* ring_e, int w, int col) {
  if (col + VEC <= p.Fs || (p.debug & 2)) return;  // all static columns
  const bool is_cur = (w == p.W - 1);
  int32_t slot = meta_slot0(m) + w;
  if (STAGE == STAGE_RAW) slot -= (slot >= p.W) ? p.W : 0;
  const bool zero = !is_cur && w < meta_n_zero(m);
  float x[GTE_MAX_DYN];
#pragma unroll
  for (int i = 0; i < GTE_MAX_DYN; ++i) {
    x[i] = 0.0f;
    if (i < p.nd) {  // wave-uniform
      if (STAGE == STAGE_RAW) {        // raw rings in LDS: pick the address, one LDS read
        const float* a = is_cur ? &L.cur[s * GTE_MAX_DYN + i] : &L.staged[(s * p.W + slot) * p.nd + i];
        x[i] = zero ? 0.0f : *a;
      } else if (STAGE == STAGE_LATE) {  // already resolved per window row
        x[i] = L.staged[(s * p.W + w) * p.nd + i];
      } else {
        x[i] = dyn_value(p, L, s, ring_e, w, i);
      }
    }
  }
  if constexpr (VEC == 4) {
    set_tail(v, p.nd, x);  // col + 4 > Fs  <=>  this is the row's last vector
  } else {
    const int i = col - p.Fs;  // VEC == 1: this element is dynamic feature i
    float r = x[0];
#pragma unroll
    for (int k = 1; k < GTE_MAX_DYN; ++k) r = (i == k) ? x[k] : r;
    v = r;
  }
}

// Window gather.  The wave's n_env*VPE vectors form one index space; lane l of
// iteration t handles vector t*64+l, so every wave instruction loads/stores 64*VEC*4
// contiguous, fully used bytes whatever the window size (also when an env's window is
// smaller than one wave instruction, e.g. windows=None).  The env differs per lane:
// its job is read from LDS.  U independent loads are in flight per lane.
// [k_lo, k_hi): the part of the index space to copy (a chunk claimed by the rollout kernel;
// everything by default).
template <int VEC, int NT, int STAGE, int U>
__device__ inline void phase_b(const Params& p, const WgLds& L, int s_first,
                               int n_env, int lane, uint64_t vpe_magic, uint64_t fv_magic,
                               uint32_t k_lo = 0u, uint32_t k_hi = 0xFFFFFFFFu) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const uint32_t V = (uint32_t)(p.W * p.Fobs);
  const uint32_t VPE = V / VEC;                // vectors per env
  const uint32_t FV = (uint32_t)p.Fobs / VEC;  // vectors per row
  const uint32_t total = min((uint32_t)n_env * VPE, k_hi);
  float* const obs0 = obs_window0(p);
  const int64_t ES = obs_env_stride(p);

  for (uint32_t k0 = k_lo; k0 < total; k0 += 64u * U) {
    vec_t v[U];
    uint32_t jj[U], ee[U], mm[U];
    int32_t env[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t k = k0 + (uint32_t)u * 64u + (uint32_t)lane;
      const bool in = k < total;
      const uint32_t kk = in ? k : 0u;
      ee[u] = fastdiv40(kk, vpe_magic);
      jj[u] = kk - ee[u] * VPE;
      const JobRec j = L.job[s_first + (int)ee[u]];  // one ds_read_b128
      mm[u] = j.meta;
      env[u] = j.env;
      ok[u] = in && (j.meta & 1u);
      if (ok[u]) { if (p.debug & 8) v[u] = (vec_t)(float)jj[u]; else v[u] = load_global<vec_t>(j.src, (int64_t)jj[u]); }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
      const uint32_t w = fastdiv40(jj[u], fv_magic);
      const int col = (int)(jj[u] - w * FV) * VEC;
      const int s = s_first + (int)ee[u];
      const float* ring_e = p.ring + (int64_t)env[u] * p.depth * p.nd;
      patch_dynamic<VEC, STAGE>(p, L, v[u], s, mm[u], ring_e, (int)w, col);
      store_out<NT>((vec_t*)(obs0 + (int64_t)env[u] * ES + (int64_t)jj[u] * VEC), v[u]);
    }
  }
}

// ---------------------------------------------------------------------------
// Lean copy loop (round 3).  The SQ counters show the step kernel's SIMDs ~75 % issue-busy: the
// generic loop above spends ~67 VALU instructions per wave-vector (two 40-bit magic divisions,
// 64-bit address arithmetic, per-vector branches, the dynamic-column patch executed by all 64 lanes
// because every wave instruction contains some row's last vector), i.e. the copy is bound by
// instruction issue as much as by memory.  For the common case — a full wave of envs that all copy,
// whole number of passes — this version does the same copy with a third of the instructions:
//   * the dynamic values of every window row are resolved ONCE per env into LDS (rotation, zero
//     rows, current row; already placed in the vector components they occupy), so patching a
//     vector is one ds_read_b128 and a per-lane select, no branch;
//   * a lane walks its vectors k = lane + 64 q with running (env, vector-in-env, row, vector-in-row)
//     counters instead of dividing;
//   * no per-vector validity branches (the caller checks the whole wave once).
// Results are the generic loop's, bit for bit (the parity suite runs through it).
// (LEAN_MAX_ROWS and GTE_LEAN_U, the vectors in flight per lane, are in gte_plan.h: the host's geometry search uses them)
template <int ND>
__device__ inline void resolve_dynamic_rows(const Params& p, const WgLds& L, int s_first, int n_env,
                                            int lane, uint64_t wnd_magic) {
  const uint32_t W = (uint32_t)p.W;
  const uint32_t rows = (uint32_t)n_env * W;  // <= LEAN_MAX_ROWS (the caller checks)
  float x[LEAN_MAX_ROWS / 64][ND];
  // every value is read (from the raw rings / the current-row values) before any is written back:
  // a wave's envs own a contiguous part of L.staged that no other wave touches
#pragma unroll
  for (int q = 0; q < LEAN_MAX_ROWS / 64; ++q) {
    if (64u * (uint32_t)q >= rows) break;  // wave-uniform
    const uint32_t r = (uint32_t)lane + 64u * (uint32_t)q;
    const bool in = r < rows;
    const uint32_t rr = in ? r : 0u;
    const uint32_t el = fastdiv40(rr * (uint32_t)ND, wnd_magic);  // rr / W  (wnd_magic divides by W * nd)
    const uint32_t w = rr - el * W;
    const int s = s_first + (int)el;
    const uint32_t m = L.job[s].meta;
    int32_t slot = meta_slot0(m) + (int32_t)w;
    if (slot >= (int32_t)W) slot -= (int32_t)W;
    const bool is_cur = (w == W - 1u);
    const bool zero = !is_cur && (int)w < meta_n_zero(m);
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const float* a = is_cur ? &L.cur[s * GTE_MAX_DYN + i] : &L.staged[((uint32_t)s * W + (uint32_t)slot) * ND + i];
      x[q][i] = (zero || !in) ? 0.0f : *a;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int q = 0; q < LEAN_MAX_ROWS / 64; ++q) {
    const uint32_t r = (uint32_t)lane + 64u * (uint32_t)q;
    if (r < rows) {  // row r of the wave's part, in window order: env r / W, row r % W
#pragma unroll
      for (int i = 0; i < ND; ++i) L.staged[((uint32_t)s_first * W + r) * ND + i] = x[q][i];
    }
  }
}

template <int NT, int ND>
__device__ inline void phase_b_lean(const Params& p, const WgLds& L, int s_first, int n_env, int lane) {
  constexpr int U = GTE_LEAN_U;
  const uint32_t W = (uint32_t)p.W, FV = (uint32_t)p.Fobs / 4u, VPE = W * FV;
  const uint32_t total = (uint32_t)n_env * VPE;          // a multiple of 64 * U (checked by the caller)
  const uint32_t SB = (uint32_t)obs_env_stride(p) * 4u;   // bytes from env to env (VPE * 16 in a classic buffer)
  // running position of this lane's vector: env slot `ee`, vector in env `jj`, row `w`, vector in row `r`
  uint32_t ee = (uint32_t)lane / VPE;                     // VPE >= 64: 0
  uint32_t jj = (uint32_t)lane - ee * VPE;
  uint32_t w = jj / FV, r = jj - w * FV;
  const uint32_t w_inc = 64u / FV, r_inc = 64u - w_inc * FV;  // one step of 64 vectors
  char* const obs = (char*)obs_window0(p);
  // (one fixed pass shape, the loop written out: as a generic lambda with a tail pass for other
  // multiples of 64 the same code compiled 5 % slower at config 5)
  for (uint32_t k0 = 0u; k0 < total; k0 += 64u * U) {
    float4_t v[U];
    float t[U][ND];
    uint32_t jj16[U];
    int32_t env[U];
    bool last[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s_first + (int)ee;
      const JobRec j = L.job[s];                           // one ds_read_b128
#pragma unroll
      for (int c = 0; c < ND; ++c) t[u][c] = L.staged[((uint32_t)s * W + w) * ND + c];  // one LDS read
      env[u] = j.env;
      jj16[u] = jj * 16u;
      last[u] = (r == FV - 1u);
      v[u] = load_global<float4_t>(j.src, (int64_t)jj);
      // advance by 64 vectors
      jj += 64u; w += w_inc; r += r_inc;
      if (r >= FV) { r -= FV; w += 1u; }
      if (jj >= VPE) { jj -= VPE; ee += 1u; w -= W; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float4_t o = v[u];
      // the dynamic columns are the last ND components of a row's last vector
#pragma unroll
      for (int c = 0; c < ND; ++c) o[4 - ND + c] = last[u] ? t[u][c] : o[4 - ND + c];
      store_out<NT>((float4_t*)(obs + (uint64_t)(uint32_t)env[u] * SB + jj16[u]), o);
    }
  }
}

// Slide loop (a launch with p.slide): the window of an env that merely advanced (JOB_SLIDES) is, at the
// new head, the one at the old head moved up a row — already in the buffer — plus the newest row.  The
// wave moves that row alone for those envs: n_env * F_obs / 4 vectors (128 for 16 envs of 32 columns
// where the full windows are 2 560), the row's last vector patched with phase A's current values.
// Neither the staged rings nor resolve_dynamic_rows are needed.  Two vectors in flight per lane.  The
// wave's other envs (a reset, a frozen env) get their full windows from the caller.
template <int NT>
__device__ inline void phase_b_slide(const Params& p, const WgLds& L, int s_first, int n_env, int lane,
                                     uint64_t fv_magic) {
  const uint32_t FV = (uint32_t)p.Fobs / 4u;
  const uint32_t total = (uint32_t)n_env * FV;
  const int64_t row = (int64_t)(p.W - 1) * FV;  // the newest row, in vectors from the window's start
  float4_t* const obs0 = (float4_t*)obs_window0(p) + row;
  const int64_t ES4 = obs_env_stride(p) / 4;
  for (uint32_t k0 = 0u; k0 < total; k0 += 128u) {
    float4_t v[2];
    uint32_t rr[2];
    int32_t env[2], sl[2];
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t k = k0 + (uint32_t)u * 64u + (uint32_t)lane;
      ok[u] = k < total;
      const uint32_t kk = ok[u] ? k : 0u;
      const uint32_t el = fastdiv40(kk, fv_magic);
      rr[u] = kk - el * FV;
      sl[u] = s_first + (int)el;
      const JobRec j = L.job[sl[u]];
      env[u] = j.env;
      ok[u] = ok[u] && (j.meta & (uint32_t)JOB_SLIDES);
      if (ok[u]) v[u] = load_global<float4_t>(j.src, row + (int64_t)rr[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!ok[u]) continue;
      if (rr[u] == FV - 1u) {
        float x[GTE_MAX_DYN];
#pragma unroll
        for (int i = 0; i < GTE_MAX_DYN; ++i) x[i] = L.cur[sl[u] * GTE_MAX_DYN + i];
        set_tail(v[u], p.nd, x);
      }
      store_out<NT>(obs0 + (int64_t)env[u] * ES4 + (int64_t)rr[u], v[u]);
    }
  }
}

// zero the dynamic store of envs that switched dataset in persist mode (the
// reference rebuilds _obs_array in _set_df), except the current row's slot
__device__ inline void zero_fresh_stores(const Params& p, const WgLds& L,
                                         int s_first, int n_env, int lane) {
  for (int el = 0; el < n_env; ++el) {
    const int s = s_first + el;
    if (!(L.job[s].meta & 2u)) continue;
    const int idx = L.idx[s];
    float* ring_e = p.ring + (int64_t)L.job[s].env * p.depth * p.nd;
    const int64_t n = p.depth * p.nd;
    const int64_t keep_lo = (int64_t)idx * p.nd, keep_hi = keep_lo + p.nd;
    for (int64_t k = lane; k < n; k += 64)
      if (k < keep_lo || k >= keep_hi) ring_e[k] = 0.0f;
  }
}

// Terminal observations (same-step auto-reset + final_obs): the wave copies the terminal
// window of each of its envs that ended in this launch into final_obs[env].  Rare, so one
// env at a time.  Earlier rows' dynamic values come from the env's ring in global memory,
// except the terminal row itself (fin.cur) and the slot the reset overwrote (fin.clob).
template <int VEC>
__device__ inline void final_windows(const Params& p, const WgLds& L, int s_first, int n_env,
                                     int lane, uint64_t fv_magic) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  const uint32_t V = (uint32_t)(p.W * p.Fobs), VPE = V / VEC, FV = (uint32_t)p.Fobs / VEC;
  // which of the wave's envs ended: one LDS read and a ballot (a loop that looked at one env's
  // flag after the other cost every wave 16 dependent LDS round trips at the tail of the launch:
  // 43.4 us per step against 39.9 without terminal observations, profiles/r02_mode_bench.log)
  unsigned long long ended = __ballot(lane < n_env && (L.fin[s_first + lane].flags & 1));
  while (ended) {  // wave-uniform
    const int el = __ffsll((long long)ended) - 1;
    ended &= ended - 1ull;
    const int s = s_first + el;
    const FinalJob f = L.fin[s];
    const int64_t env = L.job[s].env;
    const float* ring_e = p.ring + env * p.depth * p.nd;
    float* dst = p.final_obs + env * V;
    for (uint32_t j = (uint32_t)lane; j < VPE; j += 64u) {
      vec_t v = load_global<vec_t>((uint64_t)f.src, (int64_t)j);
      const uint32_t w = fastdiv40(j, fv_magic);
      const int col = (int)(j - w * FV) * VEC;
      if (col + VEC > p.Fs) {
        int32_t slot = f.slot0 + (int32_t)w;
        if (!p.persist && slot >= p.W) slot -= p.W;
        float x[GTE_MAX_DYN];
#pragma unroll
        for (int i = 0; i < GTE_MAX_DYN; ++i) {
          x[i] = 0.0f;
          if (i < p.nd) {
            if ((int)w == p.W - 1) x[i] = f.cur[i];
            else if ((int)w < f.n_zero) x[i] = 0.0f;
            else if (slot == f.clob_slot) x[i] = f.clob[i];
            else x[i] = ring_e[(int64_t)slot * p.nd + i];
          }
        }
        if constexpr (VEC == 4) {
          set_tail(v, p.nd, x);
        } else {
          const int i = col - p.Fs;
          float r = x[0];
#pragma unroll
          for (int k = 1; k < GTE_MAX_DYN; ++k) r = (i == k) ? x[k] : r;
          v = r;
        }
      }
      *(vec_t*)(dst + (int64_t)j * VEC) = v;
    }
  }
}

// COOP: wave 0 of the workgroup runs phase A for all 4*EPW (<= 64) envs of the
//       workgroup, one per lane at full lane utilisation (phase A is VALU-issue bound:
//       ~3 000 cycles of fp64 per wave whatever the number of active lanes); otherwise
//       every wave runs phase A for its own EPW envs.
// STAGE: how the dynamic-column values reach the copy loop (STAGE_* above).
#ifndef GTE_GATHER_U
#define GTE_GATHER_U 4  // independent 16-byte loads in flight per lane in the gather
#endif
template <int MODE, int VEC, int NT, bool COOP, int STAGE>
__global__ __launch_bounds__(256) void gte_kernel(const Params p, const uint64_t vpe_magic,
                                                  const uint64_t fv_magic,
                                                  const uint64_t wnd_magic) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gte_smem[];
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;  // wave in block
  // the terminal counter has two slots used alternately, so no memset launch is
  // needed between steps: this launch clears the slot the NEXT launch will use
  if (MODE == MODE_STEP && blockIdx.x == 0 && threadIdx.x == 0) p.term_count_next[0] = 0;
#ifndef GTE_HOT_ONLY  // p.log: hot_tu_covers() keeps such launches off the isolated TUs
  // this launch appends one log row: the next launch finds the count in the other cursor slot
  if (MODE == MODE_STEP && p.log.rows && blockIdx.x == 0 && threadIdx.x == 0)
    *log_cursor_other(p.log_cursor) = *p.log_cursor + 1;
#endif
  const int EPB = p.epw * GTE_WAVES;  // envs per workgroup
  const int wg_first = blockIdx.x * EPB;
  if (wg_first >= p.N) return;  // whole workgroup exits together (before any barrier)
  const int n_wg = min(EPB, p.N - wg_first);
  GTE_STAMP(0);
  const WgLds L = carve_lds(gte_smem, EPB, p.final_obs != nullptr, p.log.rows != nullptr);
  const int s_first = wib * p.epw;
  const int n_env = min(p.epw, n_wg - s_first);
  // Which env each slot processes (identity, or the L2-affinity permutation), and the raw
  // rings into LDS.  With cooperative phase A wave 0 goes straight to the state machine
  // (the in-kernel timeline showed it spending 2.8 us staging its own rings first): wave 1
  // covers wave 0's slots as well as its own.
  auto prepare = [&](int first, int count) {
    if (lane < p.epw) {
      const int slot = wg_first + first + lane;
      L.job[first + lane].env = (lane < count) ? (p.perm ? p.perm[slot] : slot) : -1;
    }
    if (STAGE == STAGE_RAW && count > 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      stage_raw_rings(p, L, first, count, lane, wnd_magic);
    }
  };
  if (!COOP) {
    prepare(s_first, n_env);
  } else if (wib >= 1) {
    prepare(s_first, n_env);
    if (wib == 1) prepare(0, min(p.epw, n_wg));
  }
  GTE_STAMP(1);  // env ids (perm) + rings arrived
#ifdef GTE_STAMPS_HWID
  GTE_STAMP_HWID(1);  // (diagnostic of the diagnostic: replaces stamp 1)
#endif

  // ---- phase A
  if (!COOP || wib == 0) {  // wave-uniform
    const int s = COOP ? lane : wib * p.epw + lane;  // LDS slot = env within the workgroup
    const bool owns = COOP ? (lane < EPB) : (lane < p.epw);
    const bool active = owns && s < n_wg;
    const int e = active ? (p.perm ? p.perm[wg_first + s] : wg_first + s) : 0;
    ObsJob job;
    FinalJob fin;
    // a step's record stores: into the LDS image (one 64-byte request per env after the barrier)
    const lds_byte_ptr hot = (MODE == MODE_STEP && p.hot_lds) ? (lds_byte_ptr)(L.hot + 64 * s) : (lds_byte_ptr) nullptr;
#ifndef GTE_HOT_ONLY  // p.log: hot_tu_covers() keeps such launches off the isolated TUs
    if (MODE == MODE_STEP && p.log.rows) {
      // gte_step with log_steps: the lane that stepped the env also produces its trajectory row —
      // what History.add records (environments.py:253-264) — from its registers, instead of a
      // second launch reading everything back; the row goes to LDS and the copy waves write it
      // out, five lanes per env (flush_log_rows)
      StepOut so = {};
      phase_a<MODE>(p, e, active, lane, job, p.final_obs ? &fin : nullptr, true, nullptr, nullptr, nullptr,
                    true, nullptr, &so, hot);
      if (active) {
        typedef int4_t __attribute__((address_space(3))) * li4;
        typedef double2_t __attribute__((address_space(3))) * ld2;
        const lds_byte_ptr w = (lds_byte_ptr)(L.logrow + sizeof(LogRow) * s);
        int4_t a = {so.idx, so.step, so.pos, so.dsi};
        double2_t d0 = {so.pv, so.realpos};
        double2_t d1 = {(so.step == 0) ? 0.0 : so.reward, so.asset};  // reset rows: reward 0 (:196)
        double2_t d2 = {so.fiat, so.ia};
        double2_t d3 = {so.ifi, __longlong_as_double((long long)(so.flags & 0xff))};  // flags byte + zero padding
        *(li4)w = a;
        *(ld2)(w + 16) = d0;
        *(ld2)(w + 32) = d1;
        *(ld2)(w + 48) = d2;
        *(ld2)(w + 64) = d3;
      }
    } else
#endif
    phase_a<MODE>(p, e, active, lane, job, p.final_obs ? &fin : nullptr, true, nullptr, nullptr, nullptr, true,
                  nullptr, nullptr, hot);
    if (owns) publish_job(L, s, job);  // slots past the last env get flags = 0
    if (owns && p.final_obs) L.fin[s] = fin;
  }
  // Only LDS has to be visible across the barrier (jobs, env ids, staged rings): nothing
  // after it reads global memory written before it in this launch.  __syncthreads() would
  // also drain wave 0's global stores (record, outputs, ring: 2.5 us in the timeline).
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  GTE_STAMP(6);

  // ---- phase B: each wave writes out the records of its own EPW envs and gathers their windows
  if (MODE == MODE_STEP && p.hot_lds && n_env > 0) flush_hot_records(p, L, s_first, n_env, lane);
#ifndef GTE_HOT_ONLY  // p.log: hot_tu_covers() keeps such launches off the isolated TUs
  if (MODE == MODE_STEP && p.log.rows && n_env > 0) flush_log_rows(p, L, s_first, n_env, lane);
#endif
  if (n_env <= 0 || (p.debug & 1)) return;
  if (p.persist) zero_fresh_stores(p, L, s_first, n_env, lane);
  if (STAGE == STAGE_LATE) {
    stage_dynamic(p, L, s_first, n_env, lane, wnd_magic);
    // LDS operations of one wave execute in order; this only stops the compiler from
    // moving the LDS reads of phase B above the staging writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  bool lean = false;
  if constexpr (MODE == MODE_STEP && VEC == 4) {
    // p.slide: the envs that merely advanced store their newest row alone (about 97 % of the waves at
    // one reset per 500 steps have no other env); an env that reset or stands frozen gets its full window
    // at the new head, one env at a time (rare) through the generic loop
    if (p.slide && !p.debug) {
      phase_b_slide<NT>(p, L, s_first, n_env, lane, fv_magic);
      const uint32_t m = L.job[s_first + (lane < n_env ? lane : 0)].meta;
      unsigned long long full = __ballot(lane < n_env && (m & 1u) && !(m & (uint32_t)JOB_SLIDES));
      const uint32_t VPE = (uint32_t)(p.W * p.Fobs) / 4u;
      while (full) {  // wave-uniform
        const uint32_t el = (uint32_t)(__ffsll((long long)full) - 1);
        full &= full - 1ull;
        phase_b<VEC, NT, STAGE, GTE_GATHER_U>(p, L, s_first, n_env, lane, vpe_magic, fv_magic, el * VPE,
                                              (el + 1u) * VPE);
      }
      GTE_STAMP(7);
      return;  // (p.final_obs is null in a launch that slides)
    }
  }
  if constexpr (MODE == MODE_STEP && VEC == 4 && STAGE == STAGE_RAW) {
    // the lean loop takes whole waves of envs that all copy, in whole passes of U wave instructions
    // (windows of at least one wave instruction: the running counters wrap at most once per step of 64)
    if (p.lean_rows > 0 && n_env == p.epw && n_env * p.W <= LEAN_MAX_ROWS && p.W * p.Fobs / 4 >= 64 &&
        ((uint32_t)n_env * (uint32_t)(p.W * p.Fobs / 4)) % (64u * GTE_LEAN_U) == 0u && !p.debug &&
        __ballot(lane < n_env && !(L.job[s_first + (lane < n_env ? lane : 0)].meta & 1u)) == 0ull) {
      switch (p.nd) {  // wave-uniform, outside the loops
        case 1: resolve_dynamic_rows<1>(p, L, s_first, n_env, lane, wnd_magic); break;
        case 2: resolve_dynamic_rows<2>(p, L, s_first, n_env, lane, wnd_magic); break;
        case 3: resolve_dynamic_rows<3>(p, L, s_first, n_env, lane, wnd_magic); break;
        default: resolve_dynamic_rows<4>(p, L, s_first, n_env, lane, wnd_magic); break;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (this wave's own LDS writes, read back below)
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      switch (p.nd) {
        case 1: phase_b_lean<NT, 1>(p, L, s_first, n_env, lane); break;
        case 2: phase_b_lean<NT, 2>(p, L, s_first, n_env, lane); break;
        case 3: phase_b_lean<NT, 3>(p, L, s_first, n_env, lane); break;
        default: phase_b_lean<NT, 4>(p, L, s_first, n_env, lane); break;
      }
      lean = true;
    }
  }
  if (!lean) phase_b<VEC, NT, STAGE, GTE_GATHER_U>(p, L, s_first, n_env, lane, vpe_magic, fv_magic);
  GTE_STAMP(7);
  if (MODE == MODE_STEP && p.final_obs) final_windows<VEC>(p, L, s_first, n_env, lane, fv_magic);
}

}  // namespace gte
