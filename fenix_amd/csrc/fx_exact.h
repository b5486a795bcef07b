// The exact distance of one corpus row as the single-query scan computes it,
// bit for bit, for the kernels that rescore the batched filter's candidates
// (knn_exact.hip, knn_select.hip), and the host-side dispatch from a runtime
// (dtype, metric) to their <T, METRIC> instantiations.
#pragma once

#include "fx_internal.h"
#include "fx_wave.h"

namespace fx {

// The single-query scan's f32 distance of one row, computed by a 16-lane
// group (lane jl of the group): 16-B loads of the row and the query, the
// scan's per-lane fmaf chain over slots jl, jl+16, ... (knn_scan.hip
// tile_accumulate), its sum16 reduction and its distance formula
// (tile_finish): bit for bit the scan's value.  Every lane of the wave must
// call it (sum16 is a cross-lane reduction); live = false contributes zeros.
//
// quint8 codes (T = uint8_t, d % 16 == 0): the scan's code-unit arithmetic
// instead, tile_accumulate's sizeof(T) == 1, W == 16 branch and tile_finish's
// quint8 branch operation for operation.  Lane jl takes the 16-code slots
// jl, jl + 16, ...; per slot the 8 packed pairs go through fma into a2 (b2:
// the cosine's sum of squares), then acc += a2.x + a2.y.  qv is what the scan
// keeps in LDS: q' = shift + q / scale for L2 (launch_qu8_query wrote it with
// scan_begin's own f32 expression), q itself otherwise.  A slot past the row
// (the scan pads with the zero-point code against q' = shift, or q = 0) adds
// +0 to a sum that is never -0: skipped.
template <int METRIC>
__device__ __forceinline__ float exact_distance16_qu8(const uint8_t* __restrict__ xr,
                                                      const float* __restrict__ qv, int d, int jl,
                                                      bool live, float qnorm, Quant z) {
  typedef uint8_t u8x16 __attribute__((ext_vector_type(16)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef float f16v __attribute__((ext_vector_type(16)));
  float acc = 0.f, acc2 = 0.f;
  const f2 z2 = {z.shift, z.shift};
  if (live) {
    for (int k = jl * 16; k < d; k += 256) {
      const f16v xf = __builtin_convertvector(*reinterpret_cast<const u8x16*>(xr + k), f16v);
      f4 q4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) q4[i] = *reinterpret_cast<const f4*>(qv + k + 4 * i);
      f2 a2 = {0.f, 0.f}, b2 = {0.f, 0.f};
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const f2 x2 = {xf[2 * p], xf[2 * p + 1]};
        const f2 q2 = {q4[p >> 1][2 * (p & 1)], q4[p >> 1][2 * (p & 1) + 1]};
        if constexpr (METRIC == 0) {
          const f2 df = x2 - q2;
          a2 = __builtin_elementwise_fma(df, df, a2);
        } else {
          const f2 df = x2 - z2;
          a2 = __builtin_elementwise_fma(df, q2, a2);
          if constexpr (METRIC == 2) b2 = __builtin_elementwise_fma(df, df, b2);
        }
      }
      acc += a2.x + a2.y;
      if constexpr (METRIC == 2) acc2 += b2.x + b2.y;
    }
  }
  const float s1 = sum16(acc);
  if constexpr (METRIC == 0) {
    return z.scale * sqrtf(s1);
  } else if constexpr (METRIC == 1) {
    return -(z.scale * s1);
  } else {
    const float s2 = sum16(acc2);
    const float nx = fmaxf(z.scale * sqrtf(s2), 1e-12f);
    return 0.5f - 0.5f * ((z.scale * s1) / (nx * qnorm));
  }
}

template <typename T, int METRIC>
__device__ __forceinline__ float exact_distance16(const T* __restrict__ xr,
                                                  const float* __restrict__ qv, int d, int jl,
                                                  bool live, float qnorm) {
  // the scan's 16-B slots: 4 floats (f32) or 8 halves (f16), lane jl takes
  // slots jl, jl + 16, ... (knn_scan.hip plan_scan: W = 16 / sizeof(T))
  constexpr int W = 16 / sizeof(T);
  constexpr int S = 16 * W;  // elements between a lane's slots
  typedef T vT __attribute__((ext_vector_type(W)));
  typedef float vF __attribute__((ext_vector_type(W)));
  float acc = 0.f, acc2 = 0.f;
  auto slot = [&](const vT& xv, const vF& yv) {
#pragma unroll
    for (int t = 0; t < W; ++t) {
      const float x = (float)xv[t];
      const float y = yv[t];
      if constexpr (METRIC == 0) {
        const float df = x - y;
        acc = fmaf(df, df, acc);
      } else if constexpr (METRIC == 1) {
        acc = fmaf(x, y, acc);
      } else {
        acc = fmaf(x, y, acc);
        acc2 = fmaf(x, x, acc2);
      }
    }
  };
  // NS slots of the lane loaded at once (all of a 768-d f32 or a 1024-d f16
  // row), then multiplied in the scan's order
  constexpr int NS = W == 4 ? 12 : 8;
  if (live) {
    for (int base = jl * W; base < d; base += NS * S) {
      vT xv[NS];
      vF yv[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int k = base + i * S;
        if (k < d) {
          xv[i] = *reinterpret_cast<const vT*>(xr + k);
          yv[i] = *reinterpret_cast<const vF*>(qv + k);
        }
      }
#pragma unroll
      for (int i = 0; i < NS; ++i)
        if (base + i * S < d) slot(xv[i], yv[i]);
    }
  }
  const float s1 = sum16(acc);  // the scan's reduction: bit-identical distances
  if constexpr (METRIC == 0) {
    return sqrtf(s1);
  } else if constexpr (METRIC == 1) {
    return -s1;
  } else {
    const float s2 = sum16(acc2);
    const float nx = fmaxf(sqrtf(s2), 1e-12f);
    return 0.5f - 0.5f * (s1 / (nx * qnorm));
  }
}

// The row's scan distance by its type: exact_distance16 for f32 / f16 rows
// (z unused), exact_distance16_qu8 for quint8 codes
template <typename T, int METRIC>
__device__ __forceinline__ float row_distance16(const T* __restrict__ xr,
                                                const float* __restrict__ qv, int d, int jl,
                                                bool live, float qnorm, Quant z) {
  if constexpr (sizeof(T) == 1) {
    return exact_distance16_qu8<METRIC>(xr, qv, d, jl, live, qnorm, z);
  } else {
    return exact_distance16<T, METRIC>(xr, qv, d, jl, live, qnorm);
  }
}

// A row type and a metric (0 L2, 1 IP, 2 cosine) as one compile-time value,
// and with_exact_kind: f(ExactKind<T, METRIC>()) for a source's runtime dtype
// and metric, so a launcher writes its kernel launch once, in a generic lambda.
template <typename T, int METRIC>
struct ExactKind {
  using Row = T;
  static constexpr int kMetric = METRIC;
  static const T* rows(const ExactSource& s) { return reinterpret_cast<const T*>(s.X); }
};

template <typename F>
int with_exact_kind(const ExactSource& s, F&& f) {
  auto by_metric = [&](auto row) {
    using T = decltype(row);
    return s.metric == FX_METRIC_COS  ? f(ExactKind<T, 2>())
           : s.metric == FX_METRIC_IP ? f(ExactKind<T, 1>())
                                      : f(ExactKind<T, 0>());
  };
  return s.dtype == FX_DTYPE_QU8   ? by_metric(uint8_t())
         : s.dtype == FX_DTYPE_F16 ? by_metric(_Float16())
                                   : by_metric(float());
}

}  // namespace fx
