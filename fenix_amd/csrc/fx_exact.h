// The arithmetic of an exact distance, written once: a lane's sums over a
// row's slots (slot_accumulate, slot_accumulate_qu8) and the step from the 16
// lanes' sums to the distance (sums_distance).  The single-query scan
// (knn_scan.hip: register tiles, stream ring, DMA ring) and the kernels that
// rescore the batched filter's candidates (knn_exact.hip, knn_select.hip)
// all compute through it, so a row's distance has the same bits on every
// path.  Also the host-side dispatch from a runtime (dtype, metric) to
// <T, METRIC> instantiations.
#pragma once

#include "fx_internal.h"
#include "fx_wave.h"

namespace fx {

typedef float f2 __attribute__((ext_vector_type(2)));

template <int W, typename V>
__device__ __forceinline__ float elem(const V& v, int e) {
  if constexpr (W == 1) {
    return (float)v;
  } else {
    return (float)v[e];
  }
}

// One slot of W elements of an f32 / f16 row (16 B, or one element) against
// the matching query elements qv[0..W), in ascending element order: every
// path sums a row in the same order, so its distance has the same bits.
template <int W, int METRIC, typename V, typename Q>
__device__ __forceinline__ void slot_accumulate(const V& v, const Q& qv, float& acc, float& acc2) {
#pragma unroll
  for (int e = 0; e < W; ++e) {
    const float x = elem<W>(v, e);
    if constexpr (METRIC == 0) {
      const float d = x - qv[e];
      acc = fmaf(d, d, acc);
    } else if constexpr (METRIC == 1) {
      acc = fmaf(x, qv[e], acc);
    } else {
      acc = fmaf(x, qv[e], acc);
      acc2 = fmaf(x, x, acc2);
    }
  }
}

// One slot of 16 quint8 codes, value = scale * (code - shift), in code units.
// Per element one ubyte->f32 convert and packed fp32 ops on pairs (v_pk_add /
// v_pk_fma), 2-2.5 VALU ops per byte instead of the 5-6 of dequantise-then-
// compute (the scan was VALU-bound at 3.6 TB/s):
//   L2   d = code - q'  with q' = shift + q / scale (the query transformed
//        once: scan_begin, launch_qu8_query), sum d^2
//   IP   sum (code - shift) q
//   cos  sum (code - shift) q and (code - shift)^2
// The 8 pairs go through fma into a2 (b2: the cosine's sum of squares), then
// acc += a2.x + a2.y: that order is the row's sum.  z2 is {shift, shift},
// built once by the caller.  q2(p) returns the query's
// pair p by value, from wherever the caller keeps it (taking the pairs as an
// array or a pointer here makes the compiler split every packed subtract of
// the L2 kernels into two scalar ones).
template <int METRIC, typename X16, typename Q2>
__device__ __forceinline__ void slot_accumulate_qu8(X16 codes, Q2&& q2, f2 z2, float& acc,
                                                    float& acc2) {
  typedef float f16v __attribute__((ext_vector_type(16)));
  const f16v xf = __builtin_convertvector(codes, f16v);
  f2 a2 = {0.f, 0.f}, b2 = {0.f, 0.f};
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const f2 x2 = {xf[2 * p], xf[2 * p + 1]};
    if constexpr (METRIC == 0) {
      const f2 d = x2 - q2(p);
      a2 = __builtin_elementwise_fma(d, d, a2);
    } else {
      const f2 d = x2 - z2;
      a2 = __builtin_elementwise_fma(d, q2(p), a2);
      if constexpr (METRIC == 2) b2 = __builtin_elementwise_fma(d, d, b2);
    }
  }
  acc += a2.x + a2.y;
  if constexpr (METRIC == 2) acc2 += b2.x + b2.y;
}

// A row's distance from the 16 lanes' partial sums (every lane of the wave
// must call it: sum16 is a cross-lane reduction).  QU8: the sums are in code
// units and take the codes' scale.  The cosine's floors are F.normalize's eps
// (coder.py:43-44); qnorm is max(||q||, 1e-12).
template <int METRIC, bool QU8>
__device__ __forceinline__ float sums_distance(float acc, float acc2, float qnorm, float scale) {
  auto scaled = [&](float v) {
    if constexpr (QU8) {
      return scale * v;
    } else {
      return v;
    }
  };
  const float s1 = sum16(acc);
  if constexpr (METRIC == 0) {
    return scaled(sqrtf(s1));
  } else if constexpr (METRIC == 1) {
    return -scaled(s1);
  } else {
    const float s2 = sum16(acc2);
    const float nx = fmaxf(scaled(sqrtf(s2)), 1e-12f);
    return 0.5f - 0.5f * (scaled(s1) / (nx * qnorm));
  }
}

// One row's distance by a 16-lane group (lane jl of the group), for the
// kernels that rescore candidates: lane jl takes the row's 16-B slots jl,
// jl + 16, ... as the scan's lanes do.  live = false contributes zeros.
//
// quint8 codes (d % 16 == 0): qv is what the scan keeps in LDS, q' for L2
// (launch_qu8_query), q itself otherwise.  A slot past the row (the scan pads
// with the zero-point code against q' = shift, or q = 0) adds +0 to a sum that
// is never -0: skipped.
template <int METRIC>
__device__ __forceinline__ float exact_distance16_qu8(const uint8_t* __restrict__ xr,
                                                      const float* __restrict__ qv, int d, int jl,
                                                      bool live, float qnorm, Quant z) {
  typedef uint8_t u8x16 __attribute__((ext_vector_type(16)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  float acc = 0.f, acc2 = 0.f;
  const f2 z2 = {z.shift, z.shift};
  if (live) {
    for (int k = jl * 16; k < d; k += 256) {
      f4 q4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) q4[i] = *reinterpret_cast<const f4*>(qv + k + 4 * i);
      auto q2 = [&](int p) { return f2{q4[p >> 1][2 * (p & 1)], q4[p >> 1][2 * (p & 1) + 1]}; };
      slot_accumulate_qu8<METRIC>(*reinterpret_cast<const u8x16*>(xr + k), q2, z2, acc, acc2);
    }
  }
  return sums_distance<METRIC, true>(acc, acc2, qnorm, z.scale);
}

template <typename T, int METRIC>
__device__ __forceinline__ float exact_distance16(const T* __restrict__ xr,
                                                  const float* __restrict__ qv, int d, int jl,
                                                  bool live, float qnorm) {
  constexpr int W = 16 / sizeof(T);  // elements per 16-B slot
  constexpr int S = 16 * W;          // elements between a lane's slots
  typedef T vT __attribute__((ext_vector_type(W)));
  typedef float vF __attribute__((ext_vector_type(W)));
  float acc = 0.f, acc2 = 0.f;
  // NS slots of the lane loaded at once (all of a 768-d f32 or a 1024-d f16
  // row), then multiplied in slot order
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
        if (base + i * S < d) slot_accumulate<W, METRIC>(xv[i], yv[i], acc, acc2);
    }
  }
  return sums_distance<METRIC, false>(acc, acc2, qnorm, 1.f);
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
// and with_kind: f(ExactKind<T, METRIC>()) for a runtime dtype and metric, so
// a launcher writes its kernel launch, or a selection its kernel's name, once
// in a generic lambda.  Returns what f returns.
template <typename T, int METRIC>
struct ExactKind {
  using Row = T;
  static constexpr int kMetric = METRIC;
  static constexpr int kSlot = 16 / sizeof(T);  // elements per 16-B slot
  static const T* rows(const ExactSource& s) { return reinterpret_cast<const T*>(s.X); }
};

template <typename F>
auto with_kind(int dtype, int metric, F&& f) {
  auto by_metric = [&](auto row) {
    using T = decltype(row);
    return metric == FX_METRIC_COS  ? f(ExactKind<T, 2>())
           : metric == FX_METRIC_IP ? f(ExactKind<T, 1>())
                                    : f(ExactKind<T, 0>());
  };
  return dtype == FX_DTYPE_QU8   ? by_metric(uint8_t())
         : dtype == FX_DTYPE_F16 ? by_metric(_Float16())
                                 : by_metric(float());
}

template <typename F>
int with_exact_kind(const ExactSource& s, F&& f) {
  return with_kind(s.dtype, s.metric, f);
}

}  // namespace fx
