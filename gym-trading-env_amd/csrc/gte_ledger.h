// gte_ledger.h — the host's proof that device memory still holds what an env's last launch wrote.
//
// Plain C++17, host only: no HIP, no other file of csrc/ (tests/ledger_check.cpp compiles it with g++ and
// checks it against a byte-by-byte model).
//
// The step kernel has two shortcuts that read nothing back from the device:
//   * sparse flag stores (Params.flags_sparse; store_flags, gte_phase_a.h): only the terminated / truncated
//     bytes that change are stored.  Right only if the two buffers hold exactly what this env's previous
//     eager step stored there;
//   * slide steps (Params.slide; phase_b_slide, gte_step.h): only the newest observation row is stored.  Right
//     only if the sliding buffer holds, at the current head, the windows this env's previous reset or step wrote.
// Either proof is a CLAIM: "env E holds that these byte ranges contain exactly what E's own last launch
// wrote there".  There are two kinds, FLAGS (two ranges: terminated, truncated) and WINDOW (one: the sliding
// buffer).  Buffers may be shared or rotated between envs, so the claims are kept process-wide, behind one
// mutex:
//   * a launch of E that writes ranges withdraws every claim, of either kind, of every OTHER env that overlaps
//     them (wrote);
//   * E's claim is established by the launch that writes every byte of it: a step (both kinds) or an
//     unmasked reset (WINDOW), once the launch has gone out (establish).  One dense / full step therefore
//     restores a claim whatever happened before;
//   * a range written inside a stream capture is TAINTED: a replay writes it at times the host does not see,
//     so it is never claimed again.  Captured steps themselves store densely and in full, so a replay is
//     right whatever ran before it.  A taint blocks a FLAGS claim for good; it blocks a WINDOW claim while
//     the env that captured lives (a graph cannot outlive the env whose state it steps, and observation
//     buffers are large allocations whose addresses come back);
//   * a claim is held over exactly the ranges it was established over: a step into other buffers (rotated
//     return slots) asks about other ranges and is told no (holds).
// What the ledger does not know: gte_env, Params, heads (a slide also needs head < M), whether a stream is
// capturing, plan.always_dense, plan.full_windows.  Those stay in gte_api.hip, which says once per launch
// what the launch writes and which of the env's own claims it leaves standing:
//
//   entry point            ranges written                          the env's own claims
//   ---------------------  --------------------------------------  ------------------------------------------
//   gte_reset, no mask     obs buffer, terminated, truncated       FLAGS withdrawn; WINDOW withdrawn, and
//                                                                  established once the launch is out (sliding)
//   gte_reset, masked      the same                                FLAGS withdrawn; WINDOW stands (the masked
//                                                                  envs' windows are written at the same head)
//   a step launch          obs (own buffer or a rollout's row),    both withdrawn before the launch; after it
//   (enqueue_step:         terminated, truncated (own or a         FLAGS established over the two ranges, WINDOW
//   gte_step, and the      rollout's row)                          over the env's own sliding buffer; captured:
//   steps of the two                                               tainted, nothing established
//   below that go out as
//   ordinary launches)
//   gte_rollout            per-step rows of obs / terminated /     WINDOW withdrawn before its launches (the fused
//                          truncated, own terminated, truncated    kernels advance the envs without writing the
//                                                                  obs buffer) and established again by a step
//                                                                  launch of its own into the own buffer; FLAGS
//                                                                  stands through its launches (the fused kernels
//                                                                  store the own flags densely: a step launch of
//                                                                  its own into them may be sparse) and is
//                                                                  withdrawn after them (copies follow)
//   gte_backtest,          own terminated, truncated               as gte_rollout
//   gte_backtest_signals
//   gte_set_schedule       none (undoes what a capture recorded    both withdrawn
//                          as run)
//   gte_bind_outputs       none; the bound obs buffer counts as    both withdrawn
//                          written (other envs sliding there stop)
//   gte_bind_sliding_obs   none; the bound buffer likewise         WINDOW withdrawn
//   gte_bind_returns       none                                    FLAGS withdrawn
//   gte_destroy            none                                    forgotten (claims, and the env's name on
//                                                                  its taints)
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <mutex>
#include <vector>

namespace gte_ledger {

enum Kind : unsigned { FLAGS = 1u, WINDOW = 2u };  // (bits: several kinds may be named at once)

struct Span {  // [ptr, ptr + bytes); a null or empty one stands for nothing
  const void* ptr;
  size_t bytes;
};
using Spans = std::initializer_list<Span>;

class Ledger {
 public:
  // Record a write: env's launch writes `written` (captured: inside a stream capture).  Every claim of every
  // other env that overlaps is withdrawn, and so are env's own claims of the kinds in `withdraw_own`
  // (captured: and its own of any kind that overlap, with the range tainted).
  void wrote(const void* env, Spans written, bool captured, unsigned withdraw_own = 0) {
    std::lock_guard<std::mutex> lock(mu_);
    drop(env, withdraw_own);
    for (const Span& s : written) clobber(env, s, captured);
  }

  // Establish env's claim of `kind` over `ranges`, which its launch (gone out by now) wrote in full.  The
  // write is recorded once more, as by wrote(), under the same lock that makes the claim: another thread's
  // env may have claimed the ranges since this launch's wrote(), and two envs never hold overlapping claims.
  // The claim replaces env's earlier one of that kind.  Captured, or over a tainted range: no claim.
  void establish(const void* env, Kind kind, Spans ranges, bool captured) {
    std::lock_guard<std::mutex> lock(mu_);
    drop(env, kind);
    for (const Span& s : ranges) clobber(env, s, captured);
    if (captured) return;
    for (const Span& s : ranges)
      for (const Taint& t : taints_)
        if (real(s) && overlap(lo(s), hi(s), t.lo, t.hi) && (kind == FLAGS || t.env)) return;
    for (const Span& s : ranges)
      if (real(s)) claims_.push_back({env, kind, lo(s), hi(s)});
  }

  // Withdraw env's own claims of `kinds`
  void withdraw(const void* env, unsigned kinds) {
    std::lock_guard<std::mutex> lock(mu_);
    drop(env, kinds);
  }

  // Ask: does env hold a claim of `kind` over exactly `ranges` (the same ranges in the same order)?
  bool holds(const void* env, Kind kind, Spans ranges) {
    std::lock_guard<std::mutex> lock(mu_);
    auto c = claims_.begin();
    size_t matched = 0;
    for (const Span& s : ranges) {
      if (!real(s)) continue;
      while (c != claims_.end() && !(c->env == env && c->kind == kind)) ++c;
      if (c == claims_.end() || c->lo != lo(s) || c->hi != hi(s)) return false;
      ++c;
      ++matched;
    }
    for (; c != claims_.end(); ++c)
      if (c->env == env && c->kind == kind) return false;  // (the claim has a range that was not asked about)
    return matched > 0;
  }

  // Forget env (destroyed): its claims go, and its taints stay without its name
  void forget(const void* env) {
    std::lock_guard<std::mutex> lock(mu_);
    drop(env, FLAGS | WINDOW);
    for (Taint& t : taints_)
      if (t.env == env) t.env = nullptr;
  }

 private:
  struct Held { const void* env; unsigned kind; uintptr_t lo, hi; };  // one range of a claim, in the order given
  struct Taint { const void* env; uintptr_t lo, hi; };                // env: who captured (null once destroyed)

  static bool real(const Span& s) { return s.ptr && s.bytes; }
  static uintptr_t lo(const Span& s) { return (uintptr_t)s.ptr; }
  static uintptr_t hi(const Span& s) { return (uintptr_t)s.ptr + s.bytes; }
  static bool overlap(uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi) {
    return a_lo < b_hi && b_lo < a_hi;
  }
  // (mu_ held) env's claims of `kinds` go
  void drop(const void* env, unsigned kinds) {
    size_t k = 0;
    for (const Held& c : claims_)
      if (!(c.env == env && (c.kind & kinds))) claims_[k++] = c;
    claims_.resize(k);
  }
  // (mu_ held) env's launch writes s: whole claims of other envs that touch it go; captured, its own as well
  // (nobody holds a claim over a tainted range)
  void clobber(const void* env, const Span& s, bool captured) {
    if (!real(s)) return;
    for (size_t i = 0; i < claims_.size();) {
      const Held c = claims_[i];
      if ((c.env != env || captured) && overlap(lo(s), hi(s), c.lo, c.hi)) {
        drop(c.env, c.kind);
        i = 0;  // (the vector changed under the loop: from the start again)
      } else {
        ++i;
      }
    }
    if (!captured) return;
    for (const Taint& t : taints_)
      if (t.env == env && t.lo == lo(s) && t.hi == hi(s)) return;  // (a graph's steps write the same ranges)
    taints_.push_back({env, lo(s), hi(s)});
  }

  std::mutex mu_;
  std::vector<Held> claims_;
  std::vector<Taint> taints_;
};

// the process-wide one
inline Ledger& ledger() {
  static Ledger the_ledger;
  return the_ledger;
}

}  // namespace gte_ledger
