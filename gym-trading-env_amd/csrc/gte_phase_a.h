// gte_phase_a.h — phase A of a step, for every translation unit that runs it (gte_step.h and through
// it the step and rollout units; gte_backtest.hip directly): one lane per environment, the scalar fp64
// state machine.  EnvRegs and the load / store of an env's record, store_flags, trading, limit-order
// fills, resets, StepOut, PriceCarry and phase_a<MODE>.  A unit that defines GTE_HOT_ONLY before the
// include compiles the features out that hot_tu_covers() names (gte_device.h).
#pragma once
#include "gte_launch.h"

namespace gte {


typedef float float4_t __attribute__((ext_vector_type(4)));

enum { MODE_STEP = 0, MODE_RESET = 1 };

// Diagnostic build only (-DGTE_STAMPS, libgte_stamps.so, never shipped): lane 0 of a
// workgroup's wave 0 records s_memrealtime (100 MHz) at a few points of the step kernel into
// the buffer whose address the host passes in p.inj_ds (unused by a step).
#ifdef GTE_STAMPS
#define GTE_STAMP(k)                                                                          \
  do {                                                                                        \
    if (MODE == MODE_STEP && p.inj_ds) {                                                      \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); /* mark data ARRIVAL */      \
      if (threadIdx.x == 0)                                                                   \
        ((unsigned long long*)p.inj_ds)[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); \
    }                                                                                         \
  } while (0)
// slot k = where the calling wave runs instead of a time: HW_ID (SIMD_ID bits 5:4, CU_ID 11:8,
// SH_ID 12, SE_ID 15:13) | XCC_ID << 32
#define GTE_STAMP_HWID(k)                                                                     \
  do {                                                                                        \
    if (MODE == MODE_STEP && p.inj_ds && threadIdx.x == 0)                                    \
      ((unsigned long long*)p.inj_ds)[blockIdx.x * 8 + (k)] =                                 \
          (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |                     \
          ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);             \
  } while (0)
#else
#define GTE_STAMP(k) do {} while (0)
#define GTE_STAMP_HWID(k) do {} while (0)
#endif

// The part of an env's record a step works on, in registers.  The fields only a reset touches
// (episode, eps_on_ds, n_picks, q_head) stay in the record and are read / written there, inside
// the rare reset branches: carried through the fp64 state machine they cost the step kernel
// four more VGPRs, i.e. an occupancy step.
struct EnvRegs {
  int32_t idx, step, pos, dsi, start, needs_reset, lo_n, flags_out;
  Portfolio q;
  double pv, realpos;
};

__device__ inline void load_state(const Params& p, int e, EnvRegs& s) {
  const EnvRec* r = &p.rec[e];  // 128-byte aligned record: six 16-byte loads
  const int4* ri = reinterpret_cast<const int4*>(r);
  const int4 a = ri[0];  // idx, step, pos, dsi
  const double2* rd = reinterpret_cast<const double2*>(&r->asset);  // offset 16
  const double2 d0 = rd[0], d1 = rd[1], d2 = rd[2];
  const int4 b = ri[4];  // start, (episode), needs_reset, (eps_on_ds)
  const int4 c = ri[5];  // (n_picks), (q_head), lo_n, flags_out
  s.idx = a.x; s.step = a.y; s.pos = a.z; s.dsi = a.w;
  s.start = b.x; s.needs_reset = b.z; s.lo_n = c.z; s.flags_out = c.w;
  s.q.asset = d0.x; s.q.fiat = d0.y; s.q.ia = d1.x; s.q.ifi = d1.y;
  s.pv = d2.x; s.realpos = d2.y;
}

// The record's hot half (EnvRec).  start, lo_n and needs_reset are written where they change
// (do_reset, fill_limit_orders, the episode end in phase_a).
__device__ inline void store_state_at(EnvRec* r, const EnvRegs& s) {
  *reinterpret_cast<int4*>(&r->idx) = make_int4(s.idx, s.step, s.pos, s.dsi);
  double2* d = reinterpret_cast<double2*>(&r->asset);
  d[0] = make_double2(s.q.asset, s.q.fiat);
  d[1] = make_double2(s.q.ia, s.q.ifi);
  d[2] = make_double2(s.pv, s.realpos);
}
// The same 64 bytes into the workgroup's LDS image (slot = env of the workgroup): the gather waves
// write them out, four lanes per env (flush_hot_records).  The pointer keeps its address space in its
// type (as a generic pointer these would be flat stores).
typedef int __attribute__((ext_vector_type(4))) int4_t;
typedef double __attribute__((ext_vector_type(2))) double2_t;
typedef unsigned char __attribute__((address_space(3))) * lds_byte_ptr;
__device__ inline void store_state_lds(lds_byte_ptr h, const EnvRegs& s) {
  typedef int4_t __attribute__((address_space(3))) * li4;
  typedef double2_t __attribute__((address_space(3))) * ld2;
  int4_t a = {s.idx, s.step, s.pos, s.dsi};
  double2_t d0 = {s.q.asset, s.q.fiat}, d1 = {s.q.ia, s.q.ifi}, d2 = {s.pv, s.realpos};
  *(li4)h = a;
  *(ld2)(h + 16) = d0;
  *(ld2)(h + 32) = d1;
  *(ld2)(h + 48) = d2;
}
__device__ inline void store_state(const Params& p, int e, const EnvRegs& s) { store_state_at(&p.rec[e], s); }

// A step's terminated / truncated bytes (f: bit0 terminated, bit1 truncated).  About N/500 envs end
// per step, so the flags of all but a few envs repeat the previous step's; each of the two scattered
// byte stores costs wave 0 a request per env.  With p.flags_sparse the host has established that the
// two buffers hold exactly what each env's previous step stored there (EnvRec.flags_out; gte_step):
// only a change is stored.  A dense launch stores every env's flags and brings flags_out up to date,
// so one dense step makes any buffer and record consistent again.
__device__ inline void store_flags(const Params& p, int e, EnvRegs& s, int32_t f) {
  if (!p.flags_sparse || f != s.flags_out) {
    p.terminated[e] = (uint8_t)(f & 1);
    p.truncated[e] = (uint8_t)(f >> 1);
  }
  if (f != s.flags_out) { s.flags_out = f; p.rec[e].flags_out = f; }
}

// MultiDatasetTradingEnv.next_dataset, environments.py:380-391
__device__ inline void next_dataset(const Params& p, int e, int32_t inj_ds, EnvRegs& s,
                                    bool& fresh) {
  EnvRec* r = &p.rec[e];
  const int32_t n = r->n_picks;
  r->n_picks = n + 1;
  s.dsi = pick_dataset(p, e, n, inj_ds);
  r->eps_on_ds = 0;                 // :381
  if (p.persist) fresh = true;      // _set_df rebuilds _obs_array (:135-141)
}

// TradingEnv.reset, environments.py:163-199 (+ MultiDataset reset :393-400)
__device__ inline void do_reset(const Params& p, int e, int32_t inj_idx, int32_t inj_pos,
                                int32_t inj_ds, EnvRegs& s, bool& fresh) {
  EnvRec* rec = &p.rec[e];
  if (p.D > 1) {  // :394-398
    const int32_t eps = rec->eps_on_ds + 1;
    rec->eps_on_ds = eps;  // (next_dataset, if it runs, clears it afterwards)
    if (eps % p.switch_every == 0) next_dataset(p, e, inj_ds, s, fresh);
  }
  uint32_t r[4];
  const int32_t episode = rec->episode;
  reset_draws(p, e, episode, 0x52534554u, r);
  rec->episode = episode + 1;
  s.step = 0;  // :166
  s.lo_n = 0;  // :168 self._limit_orders = {}
  int32_t pi = p.init_pos_index;  // :167
  if (pi < 0) pi = (inj_pos >= 0) ? inj_pos : bounded(r[0], p.P);
  s.pos = pi;
  int32_t idx = p.has_window ? p.W - 1 : 0;  // :171-172
  const DatasetDesc d = p.ds[s.dsi];
  if (p.max_dur > 0) {  // :173-177 randint(low=idx, high=T - max_dur - idx)
    const int32_t low = idx;
    const int32_t high = (int32_t)d.T - p.max_dur - idx;
    idx = (inj_idx >= 0) ? inj_idx : low + bounded(r[1], high - low);
  }
  s.idx = idx;
  s.start = idx;
  rec->start = idx;
  rec->lo_n = 0;
  const double position = p.positions[pi];  // TargetPortfolio, portfolio.py:59-66
  const double price = d.close[idx];
  s.q.asset = position * p.V0 / price;
  s.q.fiat = (1.0 - position) * p.V0;
  s.q.ia = 0.0;
  s.q.ifi = 0.0;
  s.pv = p.V0;          // :194
  s.realpos = position; // :192
  s.needs_reset = 0;
  rec->needs_reset = 0;
}

// TradingEnv._take_action_order_limit, environments.py:217-223: every pending order
// whose target differs from the current position and whose limit lies inside
// [low, high] of the NEW row trades at the limit price, in insertion order.  A filled
// non-persistent order is removed (the reference deletes it while iterating its dict
// and raises RuntimeError; the intended behaviour is implemented).
__device__ inline void fill_limit_orders(const Params& p, int e, const DatasetDesc* d,
                                         EnvRegs& s) {
  const int n = s.lo_n;
  if (n <= 0) return;
  int32_t* lp = p.lo_pos + (int64_t)e * p.P;
  double* ll = p.lo_limit + (int64_t)e * p.P;
  uint8_t* lper = p.lo_persist + (int64_t)e * p.P;
  const double hi = d->high[s.idx], lo = d->low[s.idx];
  int k = 0;
  for (int j = 0; j < n; ++j) {
    const int32_t pi = lp[j];
    const double limit = ll[j];
    const uint8_t per = lper[j];
    bool keep = true;
    const double position = p.positions[pi];
    if (position != p.positions[s.pos] && limit <= hi && limit >= lo) {
      trade_to_position(s.q, position, limit, p.fees);  // _trade(position, price=limit)
      s.pos = pi;
      if (!per) keep = false;
    }
    if (keep) {
      if (k != j) { lp[k] = pi; ll[k] = limit; lper[k] = per; }
      ++k;
    }
  }
  s.lo_n = k;
  p.rec[e].lo_n = k;
}

__device__ inline void pop_injection(const Params& p, int e, EnvRegs& s, int32_t& qi,
                                     int32_t& qp, int32_t& qd) {
  qi = qp = qd = -1;
  if (p.q_n <= 0) return;
  const int32_t h = p.rec[e].q_head;
  if (h >= p.q_n) return;
  p.rec[e].q_head = h + 1;
  const int64_t k = (int64_t)e * p.q_n + h;
  if (p.q_idx) qi = p.q_idx[k];
  if (p.q_pos) qp = p.q_pos[k];
  if (p.q_ds) qd = p.q_ds[k];
}

// Dynamic features of the current row (:153-154) -> the env's store, and the
// description of the window copy for phase B.
__device__ inline void make_job(const Params& p, int e, const EnvRegs& s, bool fresh,
                                ObsJob& job) {
#pragma unroll
  for (int i = 0; i < GTE_MAX_DYN; ++i) {
    float v = 0.0f;
    if (i < p.nd) {
      const double x = (p.dyn_kind[i] == GTE_DYN_REAL_POSITION) ? s.realpos   // :23-24
                                                                : p.positions[s.pos];  // :20-21
      v = (float)x;
      const int64_t slot = p.persist ? (int64_t)s.idx : (int64_t)(s.idx % p.W);
      p.ring[((int64_t)e * p.depth + slot) * p.nd + i] = v;
    }
    job.cur[i] = v;
  }
  const int32_t first = s.idx - p.W + 1;  // first row of the window (:159)
  job.src = p.ds[s.dsi].feat + (int64_t)first * p.Fobs;
  job.slot0 = p.persist ? first : (s.idx + 1) % p.W;
  int32_t nz;
  if (fresh) nz = p.W - 1;            // brand-new _obs_array: only the current row is set
  else if (p.persist) nz = 0;
  else {
    nz = s.start - first;             // rows before the episode start were never written
    nz = nz < 0 ? 0 : (nz > p.W - 1 ? p.W - 1 : nz);
  }
  job.n_zero = nz;
  job.idx = s.idx;
  job.flags = 1 | ((fresh && p.persist) ? 2 : 0);
}

// ---------------------------------------------------------------------------
// phase A

// Prices a fused rollout carries from step to step (one lane = one env): a step trades at
// close[idx] — the price the previous step valued the portfolio at — and values at close[idx+1],
// which the previous step already asked for; the load that would head every step's dependency
// chain is issued a step early instead.  Invalid (idx < 0) after anything but a plain step.
// What a step returned for one env, for a caller that also writes the trajectory row.
struct StepOut {
  double reward, pv, realpos, asset, fiat, ia, ifi;  // reward of the step; the rest: state after it
  int32_t idx, step, pos, dsi;
  int32_t flags;  // bit0 terminated, bit1 truncated
};

struct PriceCarry {
  double cur, next;  // close[idx], close[idx + 1] of dataset dsi
  int32_t idx, dsi;
};

// compact: add the envs whose episode ended to the terminal list (off for the inner steps
// of a fused rollout, which keeps per-step flags instead); pv_out: the valuation after the step.
// carried: the env's registers live across calls (the fused rollout keeps them there for all K
// steps: no record load per step; the record is still written through); action_in: the action
// was loaded ahead of time.  Both are nullptr — and fold away — in the per-step kernels.
template <int MODE>
__device__ inline void phase_a(const Params& p, int e, bool active, int lane, ObsJob& job,
                               FinalJob* fin = nullptr, bool compact = true,
                               double* pv_out = nullptr, EnvRegs* carried = nullptr,
                               const int32_t* action_in = nullptr, bool write_record = true,
                               PriceCarry* pc = nullptr, StepOut* so = nullptr,
                               lds_byte_ptr hot = nullptr) {
  // write_record = false (fused rollouts, with `carried`): the record is not written through on
  // this step — the caller stores it once, after its last step (fields a reset or a limit-order
  // fill changes are written where they change, whatever this flag says)
  if (fin) fin->flags = 0;
  job.src = nullptr; job.slot0 = 0; job.n_zero = 0; job.idx = 0; job.flags = 0;
#pragma unroll
  for (int i = 0; i < GTE_MAX_DYN; ++i) job.cur[i] = 0.0f;
  bool ended = false;

  if (MODE == MODE_RESET) {
    if (active && (p.mask == nullptr || p.mask[e] != 0)) {
      EnvRegs s;
      load_state(p, e, s);
      bool fresh = false;
      const int32_t ii = p.inj_idx ? p.inj_idx[e] : -1;
      const int32_t ip = p.inj_pos ? p.inj_pos[e] : -1;
      const int32_t id = p.inj_ds ? p.inj_ds[e] : -1;
      if (p.D > 1 && p.rec[e].n_picks == 0) next_dataset(p, e, id, s, fresh);  // ctor pick, :378
      do_reset(p, e, ii, ip, id, s, fresh);
      store_state(p, e, s);
      p.reward[e] = 0.0f; p.reward64[e] = 0.0;
      p.terminated[e] = 0; p.truncated[e] = 0;
      make_job(p, e, s, fresh, job);
    }
    return;
  }

  // MODE_STEP — TradingEnv.step, environments.py:233-272
  if (active) {
    EnvRegs s_own;
    EnvRegs& s = carried ? *carried : s_own;
    if (!carried) load_state(p, e, s);
    int32_t action = action_in ? *action_in : p.actions[e];
    GTE_STAMP(2);  // record + action arrived
    // positions[position_index] raises IndexError in the reference (:234); a device-side
    // action cannot raise, so an out-of-range index is treated as None (hold), never read
    if (action >= p.P) action = -1;
    bool fresh = false;
    bool stepped = true;
    bool slides = false;  // this call is a plain advance (same dataset, idx + 1, no reset, not frozen)
    if (s.needs_reset) {
      if (p.autoreset == GTE_AUTORESET_NEXT_STEP) {
        int32_t qi, qp, qd;
        pop_injection(p, e, s, qi, qp, qd);
        do_reset(p, e, qi, qp, qd, s, fresh);
        if (pc) pc->idx = -1;
        p.reward[e] = 0.0f; p.reward64[e] = 0.0;
        store_flags(p, e, s, 0);
        if (so) { so->reward = 0.0; so->flags = 0; }
        stepped = false;
      } else if (s.idx >= (int32_t)p.ds[s.dsi].T - 1) {
        // no auto-reset and no row left: the reference raises IndexError (:239);
        // the batch leaves such an env frozen, flags still raised
        p.reward[e] = 0.0f; p.reward64[e] = 0.0;
        // its flags stay raised (stored again by a dense step: a rollout writes every step's
        // flags to a fresh row): the valuation has not moved since the 0.7 test (:246), and
        // being on the last row is the truncation rule itself (:248)
        store_flags(p, e, s, ((s.pv / p.V0) <= 0.7 ? 1 : 0) | 2);
        if (so) { so->reward = 0.0; so->flags = ((s.pv / p.V0) <= 0.7 ? 1 : 0) | 2; }
        stepped = false;
        ended = true;  // so it stays in the terminal list
      }
    }
    if (stepped) {
      // only the fields this path needs (the whole 40-byte descriptor held in registers
      // across the fp64 state machine costs the kernel an occupancy step)
      const DatasetDesc* dp = p.ds + s.dsi;
      const double* d_close = dp->close;
      const int32_t d_T = (int32_t)dp->T;
      const bool carried_prices = pc && pc->idx == s.idx && pc->dsi == s.dsi;
      if (action >= 0) {  // :234 -> :213-215: trade only when the position VALUE differs
        const double position = p.positions[action];
        if (position != p.positions[s.pos]) {
          trade_to_position(s.q, position, carried_prices ? pc->cur : d_close[s.idx], p.fees);  // :204-209
          s.pos = action;                                            // :210
        }
      }
      s.idx += 1;   // :235
      s.step += 1;  // :236
      if (p.lo_pos) fill_limit_orders(p, e, dp, s);  // :238
      const double price = carried_prices ? pc->next : d_close[s.idx];  // :239
      if (pc) {  // this step's valuation price is the next step's trade price; ask for the one after
        pc->cur = price;
        pc->idx = s.idx;
        pc->dsi = s.dsi;
        pc->next = (s.idx + 1 < d_T) ? d_close[s.idx + 1] : price;
      }
      GTE_STAMP(3);  // descriptor, positions, trade, price at the new row arrived
      s.q.ia = pymax0(-s.q.asset) * p.rate;   // update_interest, portfolio.py:44-46
      s.q.ifi = pymax0(-s.q.fiat) * p.rate;
      const double pv = valorisation(s.q, price);  // :241
      const bool done = (pv / p.V0) <= 0.7;        // :246
      bool trunc = s.idx >= d_T - 1;               // :248
      if (p.max_dur > 0 && s.step >= p.max_dur - 1) trunc = true;  // :250
      s.realpos = (s.q.asset - s.q.ia) * price / valorisation(s.q, price);  // :259
      double rew = 0.0;                            // :263, stays 0 when done (:265)
      if (!done) rew = reward_of(p, pv, s.pv);
      s.pv = pv;
      p.reward64[e] = rew;
      p.reward[e] = (float)rew;
      store_flags(p, e, s, (done ? 1 : 0) | (trunc ? 2 : 0));
      if (so) { so->reward = rew; so->flags = (done ? 1 : 0) | (trunc ? 2 : 0); }
      ended = done || trunc;
      slides = !(ended && p.autoreset == GTE_AUTORESET_SAME_STEP);
      if (ended) { s.needs_reset = 1; p.rec[e].needs_reset = 1; }
      if (ended && p.autoreset == GTE_AUTORESET_SAME_STEP) {
        // the reference's step() runs _get_obs (:272) before any wrapper resets the env:
        // write the terminal row's dynamic features, remember the terminal window
#ifndef GTE_HOT_ONLY  // p.final_rec: hot_tu_covers() keeps such launches off the isolated TUs
        if (p.final_rec) {  // what the wrapper's `final_info` reports (state before the reset)
          store_state_at(&p.final_rec[e], s);
          p.final_rec[e].needs_reset = s.needs_reset;
          p.final_rec[e].start = s.start;
        }
#endif
        ObsJob term;
        make_job(p, e, s, false, term);
        int32_t qi, qp, qd;
        pop_injection(p, e, s, qi, qp, qd);
        do_reset(p, e, qi, qp, qd, s, fresh);
        if (pc) pc->idx = -1;
        if (fin && p.final_obs) {
          fin->src = term.src; fin->slot0 = term.slot0; fin->n_zero = term.n_zero; fin->flags = 1;
          // the reset's current row is about to overwrite one ring slot the terminal window
          // may still need: keep its old content (this lane wrote/reads it in program order)
          const int64_t cs = p.persist ? (int64_t)s.idx : (int64_t)(s.idx % p.W);
          fin->clob_slot = (int32_t)cs;
#pragma unroll
          for (int i = 0; i < GTE_MAX_DYN; ++i) {
            fin->cur[i] = term.cur[i];
            fin->clob[i] = (i < p.nd) ? p.ring[((int64_t)e * p.depth + cs) * p.nd + i] : 0.0f;
          }
        }
      }
    }
    GTE_STAMP(4);  // state machine done, outputs issued
    if (pv_out) *pv_out = s.pv;
    if (write_record) {
      if (hot) store_state_lds(hot, s);  // (written out by the gather waves: flush_hot_records)
      else store_state(p, e, s);
    }
    if (so) {
      so->idx = s.idx; so->step = s.step; so->pos = s.pos; so->dsi = s.dsi;
      so->pv = s.pv; so->realpos = s.realpos;
      so->asset = s.q.asset; so->fiat = s.q.fiat; so->ia = s.q.ia; so->ifi = s.q.ifi;
    }
    make_job(p, e, s, fresh, job);
    // the window moved up one row and nothing else: with p.slide its newest row is all that changed
    // (JOB_SLIDES shares bit 1 with "zero the dynamic store", which only dyn_persist raises; the host
    // never sets p.slide with dyn_persist)
    if (slides && p.slide) job.flags |= JOB_SLIDES;
    GTE_STAMP(5);  // record, ring and job stores done
  }

  // terminal-mask compaction: one atomic per wave, ids in lane order within a wave
  const unsigned long long m = __ballot(ended);
  if (compact && m != 0ull) {
    const int cnt = __popcll(m);
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(p.term_count, cnt);
    base = __shfl(base, leader);
    if (ended) {
      const int my = __popcll(m & ((1ull << lane) - 1ull));
      p.term_ids[base + my] = e;
    }
  }
}

}  // namespace gte
