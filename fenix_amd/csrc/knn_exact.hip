// Exact distances for the batched filter's candidates: the query norm and the
// quint8 query transform the scan's formulas need, the rescoring of a
// candidate buffer in place, and the exact k-th of a query's k best rows.
// Every distance is row_distance16 (fx_exact.h), the scan's own arithmetic.
#include "fx_exact.h"

namespace fx {

// cosine: max(||q||, 1e-12) per query (F.normalize eps, coder.py:43-44)
__global__ void qnorm_kernel(const float* __restrict__ Q, int64_t nq, int d,
                             float* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= nq) return;
  float s = 0.f;
  for (int i = lane; i < d; i += 64) s = fmaf(Q[q * d + i], Q[q * d + i], s);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0) out[q] = fmaxf(sqrtf(s), 1e-12f);
}

int launch_qnorm(const float* Q, int64_t nq, int d, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(qnorm_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, stream, Q, nq, d,
                     out);
  return check_launch("qnorm_kernel");
}

// The quint8 L2 scan's query q' = shift + q / scale, element by element in
// the f32 expression scan_begin (knn_scan.hip) evaluates on its way into LDS:
// the rescoring reads it back instead of dividing per candidate, and
// launch_qprep8 takes the filter's effective query from the same bits.
__global__ void qu8_query_kernel(const float* __restrict__ Q, int64_t count, Quant z,
                                 float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) out[i] = z.shift + Q[i] / z.scale;
}

int launch_qu8_query(const float* Q, int64_t nq, int d, Quant z, float* out, hipStream_t stream) {
  const int64_t count = nq * d;
  hipLaunchKernelGGL(qu8_query_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream,
                     Q, count, z, out);
  return check_launch("qu8_query_kernel");
}

// Exact distance of each appended candidate (row_distance16); the key is
// replaced in place (row unchanged).  With thr, a candidate whose
// (lower-bound) key is above the query's threshold key is dropped (kEmpty)
// unread.  Each wave takes 64 slots at a time, one per lane, and rescores the
// kept ones 4 at a time (a 16-lane group each, the kept lanes taken in order
// from the wave's ballot): dropped candidates cost one load and no group.
// Small query counts (kRescoreDenseMaxQ), whose candidates are mostly kept:
// every 16-lane group takes its own slot (4 per wave per step), so a few
// thousand candidates cost one round trip each across the whole grid
// instead of up to 16 rounds per wave (single query, 3.3 K candidates: ~25
// -> a few us).
constexpr unsigned kRescoreDenseMaxQ = 2;
template <typename T, int METRIC>
__global__ void __launch_bounds__(256) rescore_dense_kernel(const T* __restrict__ X, int64_t n,
                                                            int d, int64_t row_base,
                                                            const float* __restrict__ Q,
                                                            const float* __restrict__ qnorm,
                                                            const uint32_t* __restrict__ count,
                                                            uint64_t* __restrict__ cand, int cap,
                                                            const uint64_t* __restrict__ thr,
                                                            Quant z) {
  const int64_t q = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int grp = lane >> 4, jl = lane & 15;
  const uint32_t cq = count[q * kCountStride];
  const int64_t cnt = cq < (uint32_t)cap ? cq : (uint32_t)cap;
  const uint32_t tkey = thr != nullptr ? (uint32_t)(thr[q] >> 32) : 0xffffffffu;
  const float* qv = Q + q * (int64_t)d;
  const float qn = METRIC == 2 ? qnorm[q] : 0.f;
  uint64_t* cl = cand + q * (int64_t)cap;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + wv) * 4; base < cnt;
       base += (int64_t)gridDim.x * 16) {  // wave-uniform trip count
    const int64_t i = base + grp;
    const uint64_t c = i < cnt ? cl[i] : kEmpty;
    const int64_t row = (int64_t)(c & 0xffffffffull) - row_base;
    const bool keep = c != kEmpty && (uint32_t)(c >> 32) <= tkey && row >= 0 && row < n;
    const float dist =
        row_distance16<T, METRIC>(X + (keep ? row : 0) * (int64_t)d, qv, d, jl, keep, qn, z);
    if (jl == 0 && c != kEmpty)
      cl[i] = keep ? make_comp(dist, (uint32_t)(c & 0xffffffffull)) : kEmpty;
  }
}

template <typename T, int METRIC>
__global__ void __launch_bounds__(256) rescore_kernel(const T* __restrict__ X, int64_t n, int d,
                                                      int64_t row_base,
                                                      const float* __restrict__ Q,
                                                      const float* __restrict__ qnorm,
                                                      const uint32_t* __restrict__ count,
                                                      uint64_t* __restrict__ cand, int cap,
                                                      const uint64_t* __restrict__ thr, Quant z) {
  const int64_t q = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int grp = lane >> 4, jl = lane & 15;
  const uint32_t cq = count[q * kCountStride];
  const int64_t cnt = cq < (uint32_t)cap ? cq : (uint32_t)cap;
  const uint32_t tkey = thr != nullptr ? (uint32_t)(thr[q] >> 32) : 0xffffffffu;
  const float* qv = Q + q * (int64_t)d;
  const float qn = METRIC == 2 ? qnorm[q] : 0.f;
  uint64_t* cl = cand + q * (int64_t)cap;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + wv) * 64; base < cnt;
       base += (int64_t)gridDim.x * 256) {  // wave-uniform trip count
    const int64_t i = base + lane;
    const uint64_t c = i < cnt ? cl[i] : kEmpty;
    const int64_t row = (int64_t)(c & 0xffffffffull) - row_base;
    const bool keep = c != kEmpty && (uint32_t)(c >> 32) <= tkey && row >= 0 && row < n;
    if (c != kEmpty && !keep) cl[i] = kEmpty;
    uint64_t m = __ballot(keep);
    while (m != 0ull) {  // wave-uniform: groups 0..3 take the next 4 kept lanes
      int src = -1;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int l = m != 0ull ? __builtin_ctzll(m) : -1;
        if (m != 0ull) m &= m - 1ull;
        if (g == grp) src = l;
      }
      const int from = src >= 0 ? src : 0;
      const uint32_t lo = __shfl((uint32_t)c, from), hi = __shfl((uint32_t)(c >> 32), from);
      const uint64_t cs = ((uint64_t)hi << 32) | lo;
      const int64_t rs = (int64_t)lo - row_base;
      const bool live = src >= 0;
      const float dist =
          row_distance16<T, METRIC>(X + (live ? rs : 0) * (int64_t)d, qv, d, jl, live, qn, z);
      if (jl == 0 && live) cl[base + src] = make_comp(dist, (uint32_t)(cs & 0xffffffffull));
    }
  }
}

// Exact threshold from a query's k best candidates by upper bound (rows
// [nq][k], the select's out_row, -1 = missing): their exact distances
// (row_distance16) are k rows' scan distances, so the largest composite
// bounds the k-th smallest from above; thr[q] = min(thr[q], it).  Two
// launches: exact_kth_kernel replaces each row in place by its exact
// composite (a missing row by the largest composite, so a query with fewer
// than k candidates keeps its threshold), grid (ceil(k / 16), nq), one row
// per 16-lane group; kth_max_kernel folds a query's k composites, one wave
// per query.  (One launch with a per-query block ticket behind a
// __threadfence took ~100 us for 256 x 100 rows: the blocks' fences and
// returning atomics, not the row loads, set its time.)
template <typename T, int METRIC>
__global__ void __launch_bounds__(256) exact_kth_kernel(const T* __restrict__ X, int64_t n, int d,
                                                        int64_t row_base,
                                                        const float* __restrict__ Q,
                                                        const float* __restrict__ qnorm, int k,
                                                        int64_t* __restrict__ rows, Quant z) {
  const int64_t q = blockIdx.y;
  const int grp = threadIdx.x >> 4, jl = threadIdx.x & 15;
  const int j = blockIdx.x * 16 + grp;
  const int64_t grow = j < k ? rows[q * (int64_t)k + j] : 0;
  const int64_t row = grow - row_base;
  const bool live = j < k && grow >= 0 && row >= 0 && row < n;
  const float qn = METRIC == 2 ? qnorm[q] : 0.f;
  const float dist = row_distance16<T, METRIC>(X + (live ? row : 0) * (int64_t)d,
                                               Q + q * (int64_t)d, d, jl, live, qn, z);
  if (jl == 0 && j < k)
    rows[q * (int64_t)k + j] = live ? (int64_t)make_comp(dist, (uint32_t)grow) : (int64_t)kEmpty;
}

__global__ void __launch_bounds__(256) kth_max_kernel(const uint64_t* __restrict__ comps,
                                                      int64_t nq, int k,
                                                      uint64_t* __restrict__ thr) {
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= nq) return;
  uint64_t m = 0ull;
  for (int j = lane; j < k; j += 64) {
    const uint64_t c = comps[q * (int64_t)k + j];
    m = c > m ? c : m;
  }
  m = wave_max_u64(m);
  if (lane == 0 && m < thr[q]) thr[q] = m;
}

int launch_rescore(const ExactSource& src, int64_t nq, const uint32_t* count, uint64_t* cand,
                   int cap, const uint64_t* thr, hipStream_t stream) {
  int cus = 0;
  int rc = device_cus(&cus);
  if (rc) return rc;
  // enough blocks for ~8 per CU over the batch, at most one per 256 slots
  int64_t bx = ((int64_t)cus * 8 + nq - 1) / (nq > 0 ? nq : 1);
  if (bx > ((int64_t)cap + 255) / 256) bx = ((int64_t)cap + 255) / 256;
  if (bx < 1) bx = 1;
  // (dense: one slot per 16-lane group, 16 K slots per grid step, fewer blocks
  // when the buffer is smaller)
  const int64_t need = ((int64_t)cap + 15) / 16;
  const unsigned dense_bx = (unsigned)(need < 1024 ? need : 1024);
  return for_query_chunks(nq, [&](int64_t q0, int64_t qn) {
    const ExactSource s = src.from_query(q0);
    const uint64_t* t = thr != nullptr ? thr + q0 : nullptr;
    const uint32_t* cn = count + q0 * kCountStride;
    uint64_t* cd = cand + q0 * (int64_t)cap;
    with_exact_kind(s, [&](auto kind) {
      using K = decltype(kind);
      if (qn <= kRescoreDenseMaxQ)
        hipLaunchKernelGGL((rescore_dense_kernel<typename K::Row, K::kMetric>),
                           dim3(dense_bx, (unsigned)qn), dim3(256), 0, stream, K::rows(s), s.n,
                           s.d, s.row_base, s.Q, s.qnorm, cn, cd, cap, t, s.z);
      else
        hipLaunchKernelGGL((rescore_kernel<typename K::Row, K::kMetric>),
                           dim3((unsigned)bx, (unsigned)qn), dim3(256), 0, stream, K::rows(s),
                           s.n, s.d, s.row_base, s.Q, s.qnorm, cn, cd, cap, t, s.z);
      return FX_OK;
    });
    return check_launch("rescore_kernel");
  });
}

int launch_exact_kth(const ExactSource& src, int64_t nq, int k, int64_t* rows, uint64_t* thr,
                     hipStream_t stream) {
  int rc = for_query_chunks(nq, [&](int64_t q0, int64_t qn) {
    const ExactSource s = src.from_query(q0);
    with_exact_kind(s, [&](auto kind) {
      using K = decltype(kind);
      hipLaunchKernelGGL((exact_kth_kernel<typename K::Row, K::kMetric>),
                         dim3((unsigned)((k + 15) / 16), (unsigned)qn), dim3(256), 0, stream,
                         K::rows(s), s.n, s.d, s.row_base, s.Q, s.qnorm, k, rows + q0 * k, s.z);
      return FX_OK;
    });
    return check_launch("exact_kth_kernel");
  });
  if (rc) return rc;
  hipLaunchKernelGGL(kth_max_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, stream,
                     reinterpret_cast<const uint64_t*>(rows), nq, k, thr);
  return check_launch("kth_max_kernel");
}

}  // namespace fx
