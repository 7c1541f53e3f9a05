// gte_indicators.hip — indicator banks written on the device (gte_build_indicators, include/gte.h): one
// row of f32 [T] per gte_indicator_spec, from the resident market data of a dataset (close / high / low,
// a static feature column) or a caller-owned input bank, in the layout gte_build_signals reads in place.
// Own translation unit, like gte_signals.hip (DESIGN.md §4 "Auxiliary kernels").
//
//   gte_build_indicators_kernel   ONE WAVEFRONT PER SPEC, four per workgroup.  The wave walks its row in
//                                 pieces of 256 rows: lane l owns rows 4 l .. 4 l + 3 of the piece and
//                                 stores them as one 16-byte store, so one wave instruction stores one
//                                 contiguous 1 KiB of the row.  The spec is read wave-uniformly.
//
// All arithmetic is f64 in the order include/gte.h writes, rounded once to f32 at the store;
// -ffp-contract=off keeps a*b + c two roundings.
//
// Windowed kinds (SMA, STD, ZSCORE, MAX, MIN): a lane runs the n-term loop for its four rows at once.
// Row t0 + j needs x[t0 + j - n + 1 + k] at term k, so the four rows' terms are four NEIGHBOURING source
// rows that move up by one per term: the lane keeps them in registers, shifts, and loads ONE new value
// per term for four accumulators.  Across the wave the loads of a term are 64 values 4 rows apart (one
// contiguous 1 - 2 KiB span), and term k + 1 reads the same lines again: L1 hits.
//
// Recurrences (EMA, RSI) are one dependent chain along T.  The wave loads the piece's 256 source rows
// (lane l rows 4 l .. 4 l + 3, coalesced), then EVERY lane runs the same chain over them, the value of
// each row read from its lane with v_readlane; the state is wave-uniform and carried from piece to piece;
// lane l keeps what the chain held at its rows.  RSI's two divisions of the output are not part of the
// chain: each lane does them for its own four rows afterwards.
//
// What may be read: source row i of the dataset only for 0 <= i < T (an index outside is clamped into
// that range BEFORE an address is formed; what it loads reaches only rows that are NaN by the table in
// include/gte.h or lie beyond T); feature column / input row `column` only after the spec passed its
// check, and a spec that fails it loads nothing.  What is written: floats 0 .. round_up(T, 16) - 1 of
// rows 0 .. n_specs - 1, nothing else.  No LDS, no barrier, no scratch memory.
#include "gte_launch.h"

namespace gte {

typedef float ind_f4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(gte_indicator_spec) == 16 && offsetof(gte_indicator_spec, source) == 4 &&
              offsetof(gte_indicator_spec, column) == 8 && offsetof(gte_indicator_spec, n) == 12,
              "gte_indicator_spec: 16 bytes (include/gte.h)");

constexpr int IND_WAVES = 4;        // wavefronts (specs) per workgroup
constexpr int IND_PIECE = 64 * 4;   // rows of one piece: 4 per lane
constexpr int IND_BLOCK = 8;        // terms of a window whose loads are in flight together

// source row i: element i of a series whose elements lie `step` bytes apart, f64 or f32
template <bool F64>
__device__ __forceinline__ double ind_at(const char* p, int step, int i, int T) {
  const int ic = i < 0 ? 0 : i >= T ? T - 1 : i;  // in [0, T) before the address is formed
  const char* q = p + (int64_t)ic * step;
  if (F64) return *reinterpret_cast<const double*>(q);
  return (double)*reinterpret_cast<const float*>(q);
}

// the n-term loop of four neighbouring rows: f(j, k, x[t0 + j - n + 1 + k]) for k = 0 .. n-1 in order
template <bool F64, class F>
__device__ __forceinline__ void ind_sweep(const char* p, int step, int T, int t0, int n, F f) {
  const int p0 = t0 - n + 1;
  // w[0 .. 2] and cur[] hold source rows p0 + k .. p0 + k + 2 + IND_BLOCK; the loads of the NEXT block of
  // terms are issued before this block's arithmetic, so a load's latency is paid once per block, not
  // once per term (one wave per SIMD has nobody else to hide it behind)
  double w[3 + IND_BLOCK], nx[IND_BLOCK];
#pragma unroll
  for (int u = 0; u < 3; ++u) w[u] = ind_at<F64>(p, step, p0 + u, T);
  int k = 0;
  if (n >= IND_BLOCK) {
#pragma unroll
    for (int u = 0; u < IND_BLOCK; ++u) nx[u] = ind_at<F64>(p, step, p0 + 3 + u, T);
  }
  for (; k + IND_BLOCK <= n; k += IND_BLOCK) {
#pragma unroll
    for (int u = 0; u < IND_BLOCK; ++u) w[3 + u] = nx[u];
    if (k + 2 * IND_BLOCK <= n) {
#pragma unroll
      for (int u = 0; u < IND_BLOCK; ++u) nx[u] = ind_at<F64>(p, step, p0 + k + IND_BLOCK + 3 + u, T);
    }
#pragma unroll
    for (int u = 0; u < IND_BLOCK; ++u) {
      f(0, k + u, w[u]); f(1, k + u, w[u + 1]); f(2, k + u, w[u + 2]); f(3, k + u, w[u + 3]);
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) w[u] = w[IND_BLOCK + u];
  }
  for (; k < n; ++k) {  // the last n % IND_BLOCK terms, one by one
    const double w3 = ind_at<F64>(p, step, p0 + k + 3, T);
    f(0, k, w[0]); f(1, k, w[1]); f(2, k, w[2]); f(3, k, w3);
    w[0] = w[1]; w[1] = w[2]; w[2] = w3;
  }
}

__device__ __forceinline__ double ind_readlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

template <bool F64>
__device__ __forceinline__ void ind_row(int kind, const char* p, int step, int n, int T, float* __restrict__ row,
                                        int lane) {
  const float nanf_ = __builtin_nanf("");
  const double nd = (double)n;
  // the recurrences' state before the piece's first row: wave-uniform
  double ema = 0.0, prev = 0.0, su = 0.0, sd = 0.0, au = 0.0, ad = 0.0;
  const double alpha = 2.0 / (nd + 1.0), nm1 = (double)(n - 1);
  const int first = (kind == GTE_IND_DIFF || kind == GTE_IND_ROC || kind == GTE_IND_RSI) ? n
                    : (kind == GTE_IND_VALUE || kind == GTE_IND_EMA) ? 0 : n - 1;  // rows below are NaN
  for (int base = 0; base < T; base += IND_PIECE) {
    const int t0 = base + 4 * lane;
    const int rows = T - base < IND_PIECE ? T - base : IND_PIECE;  // rows of this piece that exist
    double y[4] = {0.0, 0.0, 0.0, 0.0};
    if (kind == GTE_IND_EMA || kind == GTE_IND_RSI) {
      double x4[4], ka[4] = {0.0, 0.0, 0.0, 0.0}, kb[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < 4; ++j) x4[j] = ind_at<F64>(p, step, t0 + j, T);
      const int nq = (rows + 3) >> 2;
      if (kind == GTE_IND_EMA) {
        for (int q = 0; q < nq; ++q) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double xv = ind_readlane(x4[j], q);
            const int t = base + 4 * q + j;
            const double d = xv - ema;
            const double m = alpha * d;
            ema = t == 0 ? xv : ema + m;
            if (lane == q) ka[j] = ema;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = ka[j];
      } else {
        for (int q = 0; q < nq; ++q) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double xv = ind_readlane(x4[j], q);
            const int t = base + 4 * q + j;
            const double c = xv - prev;
            prev = xv;
            const double g = c > 0.0 ? c : 0.0, l = c < 0.0 ? -c : 0.0;  // a NaN change: neither
            if (t >= 1 && t <= n) {
              su = su + g;
              sd = sd + l;
              if (t == n) { au = su / nd; ad = sd / nd; }
            } else if (t > n) {
              const double pu = au * nm1, pd = ad * nm1;
              const double qu = pu + g, qd = pd + l;
              au = qu / nd;
              ad = qd / nd;
            }
            if (lane == q) { ka[j] = au; kb[j] = ad; }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double rs = ka[j] / kb[j];
          const double den = 1.0 + rs;
          const double frac = 100.0 / den;
          y[j] = 100.0 - frac;
        }
      }
    } else if (base + rows - 1 < first) {
      // every row of the piece is NaN: nothing to read
    } else if (kind == GTE_IND_VALUE) {
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = ind_at<F64>(p, step, t0 + j, T);
    } else if (kind == GTE_IND_DIFF || kind == GTE_IND_ROC) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double a = ind_at<F64>(p, step, t0 + j, T), b = ind_at<F64>(p, step, t0 + j - n, T);
        if (kind == GTE_IND_DIFF) y[j] = a - b;
        else { const double r = a / b; y[j] = r - 1.0; }
      }
    } else if (kind == GTE_IND_MAX || kind == GTE_IND_MIN) {
      double m[4] = {0.0, 0.0, 0.0, 0.0};
      bool bad[4] = {false, false, false, false};
      const bool mx = kind == GTE_IND_MAX;
      ind_sweep<F64>(p, step, T, t0, n, [&](int j, int k, double v) {
        bad[j] = bad[j] || v != v;
        m[j] = (k == 0 || (mx ? v > m[j] : v < m[j])) ? v : m[j];  // of equal values the oldest stays
      });
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = bad[j] ? (double)nanf_ : m[j];
    } else {  // SMA, STD, ZSCORE
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      ind_sweep<F64>(p, step, T, t0, n, [&](int j, int, double v) { s[j] = s[j] + v; });
      double m[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = s[j] / nd;
      if (kind == GTE_IND_SMA) {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = m[j];
      } else {
        double qq[4] = {0.0, 0.0, 0.0, 0.0};
        ind_sweep<F64>(p, step, T, t0, n, [&](int j, int, double v) {
          const double d = v - m[j];
          const double d2 = d * d;
          qq[j] = qq[j] + d2;
        });
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double var = qq[j] / nd;
          const double dev = __builtin_sqrt(var);
          if (kind == GTE_IND_STD) y[j] = dev;
          else {
            const double num = ind_at<F64>(p, step, t0 + j, T) - m[j];
            y[j] = num / dev;
          }
        }
      }
    }
    ind_f4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + j;
      out[j] = t >= T ? 0.0f : t < first ? nanf_ : (float)y[j];  // (padding up to 16 is 0: pad_bank's)
    }
    if (t0 < base + ((rows + 15) & ~15)) *reinterpret_cast<ind_f4*>(row + t0) = out;
  }
}

__global__ __launch_bounds__(64 * IND_WAVES) void gte_build_indicators_kernel(
    DatasetDesc ds, int Fobs, int n_static, const gte_indicator_spec* __restrict__ specs, int n_specs,
    const float* __restrict__ input, int n_inputs, int64_t input_stride, float* __restrict__ bank,
    int64_t ind_stride) {
  const int lane = threadIdx.x & 63;
  const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * IND_WAVES + (threadIdx.x >> 6)));
  if (s >= n_specs) return;
  const gte_indicator_spec sp = specs[s];
  const int T = (int)ds.T;
  float* const row = bank + (int64_t)s * ind_stride;
  const int kind = sp.kind;
  const int n = kind == GTE_IND_VALUE ? 1 : sp.n;
  // checked before any address of the source is formed
  bool valid = kind >= GTE_IND_VALUE && kind <= GTE_IND_RSI && n >= 1 && n <= GTE_IND_MAX_WINDOW;
  const char* p = nullptr;
  int step = 0;
  bool f64 = true;
  if (valid) {
    switch (sp.source) {
      case GTE_SRC_CLOSE: p = reinterpret_cast<const char*>(ds.close); step = 8; break;
      case GTE_SRC_HIGH: p = reinterpret_cast<const char*>(ds.high); step = 8; break;
      case GTE_SRC_LOW: p = reinterpret_cast<const char*>(ds.low); step = 8; break;
      case GTE_SRC_FEATURE:
        if (sp.column >= 0 && sp.column < n_static) p = reinterpret_cast<const char*>(ds.feat + sp.column);
        step = 4 * Fobs;
        f64 = false;
        break;
      case GTE_SRC_INPUT:
        if (sp.column >= 0 && sp.column < n_inputs)
          p = reinterpret_cast<const char*>(input + (int64_t)sp.column * input_stride);
        step = 4;
        f64 = false;
        break;
      default: break;
    }
    valid = p != nullptr;
  }
  if (!valid) {  // a row of NaN, nothing read
    const float nanf_ = __builtin_nanf("");
    const int T16 = (T + 15) & ~15;
    for (int t0 = 4 * lane; t0 < T16; t0 += IND_PIECE) {
      ind_f4 out;
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = t0 + j < T ? nanf_ : 0.0f;
      *reinterpret_cast<ind_f4*>(row + t0) = out;
    }
    return;
  }
  if (f64) ind_row<true>(kind, p, step, n, T, row, lane);
  else ind_row<false>(kind, p, step, n, T, row, lane);
}

hipError_t launch_build_indicators(const DatasetDesc& ds, int Fobs, int n_static, const gte_indicator_spec* specs,
                                   int n_specs, const float* input, int n_inputs, int64_t input_stride, float* bank,
                                   int64_t ind_stride, hipStream_t stream) {
  if (!specs || !bank || n_specs < 1 || ds.T < 1 || !ds.close || !ds.feat) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gte_build_indicators_kernel, dim3((n_specs + IND_WAVES - 1) / IND_WAVES), dim3(64 * IND_WAVES),
                     0, stream, ds, Fobs, n_static, specs, n_specs, input, n_inputs, input_stride, bank, ind_stride);
  return hipGetLastError();
}

}  // namespace gte
