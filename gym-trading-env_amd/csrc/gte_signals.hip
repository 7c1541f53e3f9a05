// gte_signals.hip — signal tables written on the device (gte_build_signals, include/gte.h): one row of
// int8 [T] per gte_signal_rule, from a caller-owned bank of f32 indicators.  Own translation unit: a
// kernel added to an existing unit perturbs its neighbours' register allocation (DESIGN.md §4
// "Auxiliary kernels").
//
//   gte_build_signals_kernel   ONE WAVEFRONT PER RULE.  The wave walks its row in pieces of 1 024 rows:
//                              lane l owns rows 16 l .. 16 l + 15 of the piece, loads them from indicator
//                              rows a and b as four 16-byte loads each (the next piece's are issued
//                              before this piece is worked on), computes their 16 zones, and stores its
//                              16 table bytes with one 16-byte (non-temporal) store — so one wave instruction stores one
//                              contiguous 1 KiB of the row.  The rule is read wave-uniformly.
//
// The latch makes a row a scan along T.  Inside a lane it is a walk over 16 registers; across lanes it
// is closed with a ballot of "my 16 rows hold a non-zero zone" and ONE cross-lane read of the last
// non-zero zone of the nearest such lane below; lanes with none below start from the state the wave
// carries from piece to piece, a wave-uniform value.  No LDS, no barrier, no scratch memory.
//
// What may be read: lane l of a piece reads 16 floats at a * ind_stride + base + 16 l only when
// base + 16 l < T, and ind_stride >= round_up(T, 16) (checked by gte_build_signals), so the 64 bytes
// lie inside row a of the bank; a and b are checked against [0, C) / [-1, C) before any load, and a
// rule that fails the check loads nothing.  What is written: bytes 0 .. round_up(T, 16) - 1 of rows
// 0 .. n_rules - 1, nothing else.
//
// f32 subnormals are kept (the kernel descriptor's float_denorm_mode_32 = 3, hipcc's default, which the
// Makefile's flags do not change), and -ffp-contract=off leaves the one subtraction alone.
#include "gte_launch.h"

namespace gte {

typedef float sig_f4 __attribute__((ext_vector_type(4)));
typedef unsigned int sig_u4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(gte_signal_rule) == 32 && offsetof(gte_signal_rule, hi) == 8 &&
              offsetof(gte_signal_rule, warmup) == 16 && offsetof(gte_signal_rule, pos_up) == 20 &&
              offsetof(gte_signal_rule, latch) == 23, "gte_signal_rule: 32 bytes (include/gte.h)");

constexpr int SIG_WAVES = 4;        // wavefronts (rules) per workgroup
constexpr int SIG_PIECE = 64 * 16;  // rows of one piece: 16 per lane

// the 16 floats of lane `lane` in the piece that starts at row `base` of indicator row `x`
__device__ __forceinline__ void sig_load(const float* x, int64_t base, int lane, sig_f4 (&v)[4]) {
  const sig_f4* q = reinterpret_cast<const sig_f4*>(x + base + 16 * lane);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = q[i];
}

// the 16 table bytes of a lane: a non-temporal store (plain C++, the compiler pads it).  The table is
// written once and read by nobody here, and the bank rows are what L2 should keep: against a plain
// store 2-5 % faster, against write-through (sc1) faster with sorted rules and level with random ones
// (profiles/signal_build_store_ab.log).  -DGTE_SIG_STORE=0 plain, =2 sc1: the builds of that A/B.
#ifndef GTE_SIG_STORE
#define GTE_SIG_STORE 1
#endif
__device__ __forceinline__ void sig_store(sig_u4* dst, sig_u4 v) {
#if GTE_SIG_STORE == 2
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
#elif GTE_SIG_STORE == 1
  __builtin_nontemporal_store(v, dst);
#else
  *dst = v;
#endif
}

__global__ __launch_bounds__(64 * SIG_WAVES) void gte_build_signals_kernel(
    const float* __restrict__ bank, int C, int64_t ind_stride, const gte_signal_rule* __restrict__ rules, int n_rules,
    int64_t T, int8_t* __restrict__ table, int64_t row_stride) {
  const int lane = threadIdx.x & 63;
  const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SIG_WAVES + (threadIdx.x >> 6)));
  if (s >= n_rules) return;
  const gte_signal_rule r = rules[s];
  const bool valid = r.a >= 0 && r.a < C && r.b >= -1 && r.b < C;
  const bool pair = valid && r.b >= 0;
  const bool latch = r.latch != 0;
  // an invalid rule is all warm-up: every byte -1, nothing loaded
  const int64_t warm = valid ? (int64_t)r.warmup : INT64_MAX;
  const float* xa = bank + (valid ? (int64_t)r.a * ind_stride : 0);
  const float* xb = bank + (pair ? (int64_t)r.b * ind_stride : 0);
  const unsigned up = (uint8_t)r.pos_up, down = (uint8_t)r.pos_down, neutral = (uint8_t)r.pos_neutral;
  int8_t* const row = table + (int64_t)s * row_stride;
  const int r0 = 16 * lane;  // this lane's first row inside a piece

  sig_f4 na[4] = {}, nb[4] = {};
  if (valid && r0 < T) sig_load(xa, 0, lane, na);
  if (pair && r0 < T) sig_load(xb, 0, lane, nb);
  int carry = 0;  // the latch state before the piece's first row: wave-uniform
  for (int64_t base = 0; base < T; base += SIG_PIECE) {
    sig_f4 va[4], vb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { va[i] = na[i]; vb[i] = nb[i]; }
    const int64_t next = base + SIG_PIECE;
    if (valid && next + r0 < T) sig_load(xa, next, lane, na);
    if (pair && next + r0 < T) sig_load(xb, next, lane, nb);
    // rows of this piece below w are warm-up, rows from n on do not exist (padding up to 16)
    const int n = (int)(T - base < SIG_PIECE ? T - base : SIG_PIECE);
    const int w = (int)(warm - base < 0 ? 0 : warm - base > SIG_PIECE ? SIG_PIECE : warm - base);
    int z[16];
    int last = 0;  // the last non-zero zone of this lane's rows
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float a = va[j >> 2][j & 3], b = vb[j >> 2][j & 3];
      const float d = pair ? a - b : a;
      const int t = r0 + j;
      const bool held = t < w || t >= n;
      z[j] = held ? 0 : d > r.hi ? 1 : d < r.lo ? -1 : 0;
      last = z[j] != 0 ? z[j] : last;
    }
    // the state this lane starts from: the last non-zero zone of the nearest lane below that has
    // one, else the wave's carry
    const unsigned long long some = __ballot(last != 0);
    const unsigned long long below = some & ((1ull << lane) - 1ull);
    const int from = below ? 63 - __builtin_clzll(below) : lane;
    const int theirs = __shfl(last, from, 64);
    int q = below ? theirs : carry;
    if (some) carry = __shfl(last, 63 - __builtin_clzll(some), 64);

    sig_u4 out;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      q = (z[j] != 0 || !latch) ? z[j] : q;
      const int t = r0 + j;
      const bool held = t < w || t >= n;
      const unsigned byte = held ? 0xffu : q > 0 ? up : q < 0 ? down : neutral;
      if ((j & 3) == 0) out[j >> 2] = byte;
      else out[j >> 2] |= byte << (8 * (j & 3));
    }
    if (r0 < n) sig_store(reinterpret_cast<sig_u4*>(row + base + r0), out);  // (a lane past the row's end stores nothing)
  }
}

hipError_t launch_build_signals(const float* indicators, int n_indicators, int64_t ind_stride,
                                const gte_signal_rule* rules, int n_rules, int64_t T, int8_t* table,
                                int64_t row_stride, hipStream_t stream) {
  if (!indicators || !rules || !table || n_indicators < 1 || n_rules < 1 || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_build_signals_kernel, dim3((n_rules + SIG_WAVES - 1) / SIG_WAVES), dim3(64 * SIG_WAVES), 0,
                     stream, indicators, n_indicators, ind_stride, rules, n_rules, T, table, row_stride);
  return hipGetLastError();
}

}  // namespace gte
