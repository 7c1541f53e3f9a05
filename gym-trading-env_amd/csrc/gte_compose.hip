// gte_compose.hip — signal tables composed on the device (gte_compose_signals, include/gte.h): one row of
// int8 [T] per gte_signal_compose, from a caller-owned table of clause rows (zone codes 0 / 1 / 2, as
// gte_build_signals writes them with pos_down / pos_neutral / pos_up = 0 / 1 / 2) and an 81-entry truth
// table per strategy.  Own translation unit, for the reason gte_signals.hip states at its top.
//
//   gte_compose_signals_kernel   ONE WAVEFRONT PER SPEC, in the shape gte_build_signals_kernel was
//                                measured with.  The wave walks its row in pieces of 1 024 rows: lane l owns
//                                bytes 16 l .. 16 l + 15 of the piece, loads them from each of its n_in
//                                clause rows with one 16-byte load (the next piece's are issued before this
//                                piece is worked on), looks its 16 truth-table entries up, and stores its 16
//                                table bytes with one 16-byte non-temporal store — one wave instruction
//                                stores one contiguous 1 KiB of the row.
//
// Four bytes at a time where the rule allows it: "some input byte is no code" is (w & 0xFC) | (bit 0 &
// bit 1) of every byte of an input dword, OR-ed over the inputs; the truth-table index is the sum of
// (w & 0x03030303) * 3^k, at most 3 * 40 = 120 per byte, so no byte carries into its neighbour whatever
// the input holds.  The entry itself is one byte read per table byte from a WAVE-PRIVATE copy of
// lut[81] + reserved[27] in LDS, padded to 128 bytes: an index of a byte that is no code (<= 120) still
// reads inside the copy, and what it reads is masked out.  Every wave of the workgroup reaches the one
// barrier after that copy; a wave past n_specs idles until then and returns after it.
//
// KEEP makes a row a scan along T.  An entry that decides nothing (KEEP, an invalid input byte, a byte
// past the row's end) is the byte 0x80 = KEEP itself: no decided value equals it.  Inside a lane the scan
// is a walk over 16 bytes; across lanes it is closed like the latch of gte_signals.hip: a ballot of "my
// 16 bytes decided something" and ONE cross-lane read of the last decided value of the nearest such lane
// below; lanes with none below start from the state the wave carries from piece to piece, wave-uniform.
//
// What may be read: lane l of a piece reads 16 bytes at in[k] * clause_stride + base + 16 l only when
// base + 16 l < T, and clause_stride >= round_up(T, 16) (checked by gte_compose_signals), so they lie
// inside row in[k] of the clause table; n_in and in[0 .. n_in-1] are checked before any load, and a spec
// that fails the check loads nothing.  What is written: bytes 0 .. round_up(T, 16) - 1 of rows
// 0 .. n_specs - 1, nothing else, all of it with vector stores from plain C++.
#include "gte_launch.h"

namespace gte {

typedef unsigned int cmp_u4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(gte_signal_compose) == 128 && offsetof(gte_signal_compose, n_in) == 16 &&
              offsetof(gte_signal_compose, initial) == 17 && offsetof(gte_signal_compose, pos_invalid) == 18 &&
              offsetof(gte_signal_compose, lut) == 20 && offsetof(gte_signal_compose, reserved) == 101,
              "gte_signal_compose: 128 bytes (include/gte.h)");
static_assert((uint8_t)GTE_COMPOSE_KEEP == 0x80, "KEEP is the byte 0x80");

constexpr int CMP_WAVES = 4;        // wavefronts (specs) per workgroup
constexpr int CMP_PIECE = 64 * 16;  // bytes of one piece: 16 per lane
constexpr int CMP_LUT_WORDS = 32;   // the wave's truth table in LDS: 27 dwords of the spec, padded to 128 bytes
constexpr unsigned CMP_KEEP4 = 0x80808080u;

// the 16 bytes of lane `lane` in the piece that starts at byte `base` of clause row `x`
__device__ __forceinline__ cmp_u4 cmp_load(const int8_t* x, int64_t base, int lane) {
  return *reinterpret_cast<const cmp_u4*>(x + base + 16 * lane);
}

// 0xff in every byte of `w` that is not zero
__device__ __forceinline__ unsigned cmp_nonzero_bytes(unsigned w) {
  const unsigned high = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & CMP_KEEP4;
  return (high >> 7) * 0xffu;
}

__global__ __launch_bounds__(64 * CMP_WAVES) void gte_compose_signals_kernel(
    const int8_t* __restrict__ clauses, int R, int64_t clause_stride, const gte_signal_compose* __restrict__ specs,
    int n_specs, int64_t T, int8_t* __restrict__ table, int64_t row_stride) {
  __shared__ uint32_t lut_lds[CMP_WAVES][CMP_LUT_WORDS];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * CMP_WAVES + wave));
  const bool live = s < n_specs;
  if (live && lane < CMP_LUT_WORDS) {  // lut[81] + reserved[27] are dwords 5 .. 31 of the spec
    const uint32_t* words = reinterpret_cast<const uint32_t*>(specs + s);
    lut_lds[wave][lane] = lane < 27 ? words[5 + lane] : CMP_KEEP4;
  }
  __syncthreads();  // (every wave of the workgroup is here: none has returned)
  if (!live) return;

  const gte_signal_compose* const sp = specs + s;
  const int n_in = sp->n_in;
  bool valid = n_in >= 1 && n_in <= 4;
  const int8_t* x[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = sp->in[k];
    const bool inside = r >= 0 && r < R;
    if (k < n_in && !inside) valid = false;
    x[k] = clauses + (inside ? (int64_t)r * clause_stride : 0);
  }
  int8_t* const row = table + (int64_t)s * row_stride;
  const int r0 = 16 * lane;  // this lane's first byte inside a piece

  if (!valid) {  // a row of -1, nothing loaded
    const cmp_u4 hold = {~0u, ~0u, ~0u, ~0u};
    for (int64_t base = 0; base + r0 < T; base += CMP_PIECE)
      __builtin_nontemporal_store(hold, reinterpret_cast<cmp_u4*>(row + base + r0));
    return;
  }

  const unsigned pos_invalid4 = (unsigned)(uint8_t)sp->pos_invalid * 0x01010101u;
  const uint8_t* const lut = reinterpret_cast<const uint8_t*>(lut_lds[wave]);
  cmp_u4 nx[4] = {};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n_in && r0 < T) nx[k] = cmp_load(x[k], 0, lane);
  unsigned carry = (uint8_t)sp->initial;  // the state before the piece's first byte: wave-uniform
  for (int64_t base = 0; base < T; base += CMP_PIECE) {
    cmp_u4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = nx[k];
    const int64_t next = base + CMP_PIECE;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n_in && next + r0 < T) nx[k] = cmp_load(x[k], next, lane);
    // bytes of this piece from n on do not exist (padding up to 16); `mine` of this lane's 16 do
    const int n = (int)(T - base < CMP_PIECE ? T - base : CMP_PIECE);
    const int mine = n - r0 < 0 ? 0 : n - r0 > 16 ? 16 : n - r0;

    unsigned entry[4], invalid[4], beyond[4];  // per dword: the entries (KEEP where nothing is decided), masks
    unsigned last = CMP_KEEP4 & 0xffu;         // the last decided value of this lane's bytes, or KEEP
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned no_code = 0, index = 0;
#pragma unroll
      for (int k = 0, weight = 1; k < 4; ++k, weight *= 3) {
        if (k < n_in) {
          const unsigned w = v[k][i];
          no_code |= (w & 0xfcfcfcfcu) | (w & (w >> 1) & 0x01010101u);
          index += (w & 0x03030303u) * (unsigned)weight;
        }
      }
      invalid[i] = cmp_nonzero_bytes(no_code);
      const int have = mine - 4 * i;
      beyond[i] = have >= 4 ? 0u : have <= 0 ? ~0u : ~0u << (8 * have);
      unsigned e = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) e |= (unsigned)lut[(index >> (8 * j)) & 0xffu] << (8 * j);
      const unsigned silent = invalid[i] | beyond[i];
      entry[i] = (e & ~silent) | (CMP_KEEP4 & silent);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned b = (entry[i] >> (8 * j)) & 0xffu;
        last = b != 0x80u ? b : last;
      }
    }
    // the state this lane starts from: the last decided value of the nearest lane below that has one,
    // else the wave's carry
    const unsigned long long some = __ballot(last != 0x80u);
    const unsigned long long below = some & ((1ull << lane) - 1ull);
    const int from = below ? 63 - __builtin_clzll(below) : lane;
    const unsigned theirs = (unsigned)__shfl((int)last, from, 64);
    unsigned q = below ? theirs : carry;
    if (some) carry = (unsigned)__shfl((int)last, 63 - __builtin_clzll(some), 64);

    cmp_u4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned o = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned b = (entry[i] >> (8 * j)) & 0xffu;
        q = b != 0x80u ? b : q;
        o |= q << (8 * j);
      }
      out[i] = (((o & ~invalid[i]) | (pos_invalid4 & invalid[i])) & ~beyond[i]) | beyond[i];
    }
    if (r0 < n) __builtin_nontemporal_store(out, reinterpret_cast<cmp_u4*>(row + base + r0));  // (a lane past the row's end stores nothing)
  }
}

hipError_t launch_compose_signals(const int8_t* clauses, int n_clause_rows, int64_t clause_stride,
                                  const gte_signal_compose* specs, int n_specs, int64_t T, int8_t* table,
                                  int64_t row_stride, hipStream_t stream) {
  if (!clauses || !specs || !table || n_clause_rows < 1 || n_specs < 1 || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_compose_signals_kernel, dim3((n_specs + CMP_WAVES - 1) / CMP_WAVES), dim3(64 * CMP_WAVES), 0,
                     stream, clauses, n_clause_rows, clause_stride, specs, n_specs, T, table, row_stride);
  return hipGetLastError();
}

}  // namespace gte
