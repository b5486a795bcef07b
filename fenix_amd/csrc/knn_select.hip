// The selects of the int8-image search: one workgroup per query streams the
// query's candidate keys through LDS and keeps the k smallest, then
//   exact_threshold_kernel: their exact distances set the query's threshold
//     (and the overflow gate runs on it in the same workgroup);
//   sample_threshold_kernel: the k-th smallest key is the threshold;
//   final_select_kernel: sorted and decoded, the search's result;
//   prune_kernel: before any of these over a large buffer, one workgroup per
//     16 K slice keeps the slice's k smallest, and the select reads those
//     k-lists instead of every entry.
// Also the stand-alone overflow gate and the planning of the prune scratch.
#include "fx_exact.h"
#include "fx_select.h"

namespace fx {

constexpr int kSelectThreads = 1024;
constexpr int kSelectEntries = 16384;  // LDS chunk (128 KB), and the prune pass's slice

// Dynamic LDS of every select: the reduction words, the k kept so far (P2
// slots: k rounded up to a power of two, for the bitonic sort) and one chunk
struct SelectLds {
  MergeShared* ms;
  uint64_t* res;
  uint64_t* s;
};
__device__ __forceinline__ SelectLds select_lds(int P2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* res = reinterpret_cast<uint64_t*>(smem + sizeof(MergeShared));
  return SelectLds{reinterpret_cast<MergeShared*>(smem), res, res + P2};
}

// s[0..cnt) = src[0..cnt), 8 loads in flight per thread, each entry folded
// into the thread's OR / AND (block_or_and)
__device__ __forceinline__ void stage_chunk(const uint64_t* src, int cnt, uint64_t* s,
                                            uint64_t& v_or, uint64_t& v_and) {
  const int tid = threadIdx.x;
  for (int base = tid; base < cnt; base += kSelectThreads * 8) {
    uint64_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = base + j * kSelectThreads;
      e[j] = i < cnt ? src[i] : kEmpty;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = base + j * kSelectThreads;
      if (i < cnt) {
        s[i] = e[j];
        v_or |= e[j];
        v_and &= e[j];
      }
    }
  }
}

// The k smallest of src[0..m) into l.res, in no order: a streaming
// block_keep_k over LDS-sized chunks, the k kept so far carried into the next
// chunk (any m).  Returns how many there are, min(m, k).
__device__ __forceinline__ int stream_keep_k(const uint64_t* src, int64_t m, int k,
                                             const SelectLds& l) {
  const int tid = threadIdx.x;
  int nres = 0;
  const int64_t chunk = kSelectEntries - k;
  for (int64_t off = 0; off < m || (off == 0 && m == 0); off += chunk) {  // (uniform)
    const int cnt = (int)((m - off) < chunk ? (m - off) : chunk);
    block_reset(l.ms);
    __syncthreads();
    uint64_t v_or = 0, v_and = ~0ull;
    stage_chunk(src + off, cnt, l.s, v_or, v_and);
    for (int i = tid; i < nres; i += kSelectThreads) {  // the k kept so far
      const uint64_t e = l.res[i];
      l.s[cnt + i] = e;
      v_or |= e;
      v_and &= e;
    }
    const int t = cnt + nres;
    block_or_and(v_or, v_and, l.ms);
    __syncthreads();
    if (t > k) {
      block_keep_k<kSelectThreads>(l.s, t, k, l.res, l.ms);
      nres = k;
    } else {
      for (int i = tid; i < t; i += kSelectThreads) l.res[i] = l.s[i];
      nres = t;
    }
    __syncthreads();
    if (m == 0) break;
  }
  return nres;
}

// After a prune pass over the query's m entries (pre non-null): the k-lists
// of their slices, [nq][pre_p][k], in place of the entries themselves
__device__ __forceinline__ void read_pruned(const uint64_t* pre, int pre_p, int64_t q, int k,
                                            const uint64_t*& src, int64_t& m) {
  if (pre == nullptr) return;
  src = pre + q * pre_p * (int64_t)k;
  m = (m + kSelectEntries - 1) / kSelectEntries * k;
}

__device__ __forceinline__ void write_result(uint64_t e, float* out_dist, int64_t* out_row) {
  *out_dist = e == kEmpty ? __builtin_nanf("") : key_float((uint32_t)(e >> 32));
  *out_row = e == kEmpty ? -1 : (int64_t)(e & 0xffffffffull);
}

// k <= 128: one wave sorts the (at most 128) kept entries in registers, two
// per lane (positions lane and lane + 64), the bitonic network of
// lds_sort_decode with shuffles instead of its 28 block barriers
__device__ __forceinline__ void wave_sort_decode(const uint64_t* res, int nres, int k,
                                                 float* out_dist, int64_t* out_row) {
  const int tid = threadIdx.x;
  if (tid >= kWave) return;
  uint64_t a = tid < nres ? res[tid] : kEmpty;
  uint64_t b = tid + kWave < nres ? res[tid + kWave] : kEmpty;
  for (int size = 2; size <= 2 * kWave; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride == kWave) {  // partners in one lane; size 128: ascending
        const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
        a = lo;
        b = hi;
      } else {
        const uint64_t pa = shfl_xor_u64(a, stride), pb = shfl_xor_u64(b, stride);
        const bool lower = (tid & stride) == 0;
        const bool asc_a = (tid & size) == 0, asc_b = ((tid + kWave) & size) == 0;
        a = (lower == asc_a) ? (a < pa ? a : pa) : (a < pa ? pa : a);
        b = (lower == asc_b) ? (b < pb ? b : pb) : (b < pb ? pb : b);
      }
    }
  }
  const uint64_t e2[2] = {a, b};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = tid + h * kWave;
    if (i < k) write_result(e2[h], out_dist + i, out_row + i);
  }
}

// bitonic sort of res[0..P2) in LDS (entries past nres: kEmpty), the first k decoded
__device__ __forceinline__ void lds_sort_decode(uint64_t* res, int nres, int k, int P2,
                                                float* out_dist, int64_t* out_row) {
  const int tid = threadIdx.x;
  for (int i = nres + tid; i < P2; i += kSelectThreads) res[i] = kEmpty;
  __syncthreads();
  for (int size = 2; size <= P2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (P2 >> 1); i += kSelectThreads) {
        const int lo = (i / stride) * 2 * stride + (i % stride);
        const int hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const uint64_t x = res[lo], y = res[hi];
        if ((x > y) == asc) {
          res[lo] = y;
          res[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += kSelectThreads) write_result(res[i], out_dist + i, out_row + i);
}

// Final-pass overflow prediction for query q, by a whole workgroup of
// kSelectThreads (barriers inside; tot: a word of LDS): of its c appended lb
// composites of cand [nq][cap], those that pass the threshold thrq, scaled
// by num / den (the remaining tiles over the sample's), plus c; a query
// predicted past cap gets count = cap + 1.  8 loads in flight per thread
// (k = 1 000: ~50 K F1 candidates per query, 63 -> ~10 us).
__device__ __forceinline__ void overflow_gate(const uint64_t* __restrict__ cand,
                                              uint32_t* __restrict__ count, int64_t q, uint32_t c,
                                              int64_t cap, uint64_t thrq, int64_t num, int64_t den,
                                              uint32_t* tot) {
  if (c > (uint32_t)cap) return;  // (uniform; already overflowing: recomputed anyway)
  const int tid = threadIdx.x;
  if (tid == 0) *tot = 0u;
  __syncthreads();
  const uint32_t t = (uint32_t)(thrq >> 32);
  const uint64_t* cq = cand + q * cap;
  uint32_t mine = 0u;
  for (uint32_t b = tid; b < c; b += kSelectThreads * 8) {
    uint64_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t i = b + j * kSelectThreads;
      e[j] = i < c ? cq[i] : kEmpty;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) mine += b + j * kSelectThreads < c && (uint32_t)(e[j] >> 32) <= t;
  }
  for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
  if ((tid & 63) == 0) atomicAdd(tot, mine);
  __syncthreads();
  if (tid == 0) {
    const uint64_t predicted =
        (uint64_t)c + ((uint64_t)*tot * (uint64_t)num + (uint64_t)den - 1) / (uint64_t)den;
    if (predicted > (uint64_t)cap) count[q * kCountStride] = (uint32_t)cap + 1u;
  }
}

// The gate on its own, one workgroup per query: after a threshold that the
// select's workgroup did not compute itself (rows out, launch_exact_kth)
__global__ void __launch_bounds__(kSelectThreads) overflow_gate_kernel(
    const uint64_t* __restrict__ cand, uint32_t* __restrict__ count,
    const uint64_t* __restrict__ thr, int cap, int64_t num, int64_t den) {
  __shared__ uint32_t tot;
  const int64_t q = blockIdx.x;
  overflow_gate(cand, count, q, count[q * kCountStride], cap, thr[q], num, den, &tot);
}

int launch_overflow_gate(const uint64_t* cand, uint32_t* count, const uint64_t* thr, int64_t nq,
                         int cap, int64_t num, int64_t den, hipStream_t stream) {
  if (nq <= 0) return FX_OK;
  if (nq > 0x7fffffffll || den <= 0) {
    set_error("overflow gate: nq=%lld den=%lld", (long long)nq, (long long)den);
    return FX_EINVAL;
  }
  hipLaunchKernelGGL(overflow_gate_kernel, dim3((unsigned)nq), dim3(kSelectThreads), 0, stream,
                     cand, count, thr, cap, num, den);
  return check_launch("overflow_gate_kernel");
}

// Exact threshold: the k smallest of the query's first count[q] keys of keys
// [nq][cap] (upper bounds), then
//   out_row null: their exact distances (row_distance16, 64 groups of 16
//     lanes) and thr[q] = min(thr[q], the largest exact composite); with
//     gate_cand, the overflow gate on that threshold follows in the same
//     workgroup (saves the gate's own launch, ~5 us per search,
//     profiles/r06_cfg1_img8_timeline.txt);
//   out_row given: their rows to out_row[q][k] (-1 = missing), rescored by
//     the whole chip (launch_exact_kth); no threshold and no gate here.
// A query with fewer than k candidates keeps its threshold.  zero_count
// resets the count once every thread has read it.
template <typename T, int METRIC>
__global__ void __launch_bounds__(kSelectThreads)
    exact_threshold_kernel(const T* __restrict__ X, int64_t n, int d, int64_t row_base,
                           const float* __restrict__ Q, const float* __restrict__ qnorm,
                           const uint64_t* __restrict__ keys, int64_t cap,
                           uint32_t* __restrict__ count, int zero_count, int k, int P2,
                           uint64_t* __restrict__ thr, int64_t* __restrict__ out_row,
                           const uint64_t* __restrict__ pre, int pre_p,
                           const uint64_t* __restrict__ gate_cand, int64_t gate_num,
                           int64_t gate_den, Quant z) {
  const SelectLds l = select_lds(P2);
  MergeShared* ms = l.ms;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t q = blockIdx.y;
  const uint32_t c = count[q * kCountStride];
  int64_t m = (int64_t)c < cap ? (int64_t)c : cap;
  const uint64_t* src = keys + q * cap;
  __syncthreads();
  if (zero_count && tid == 0) count[q * kCountStride] = 0u;
  if (m < k) {  // (uniform) fewer than k candidates: no threshold
    if (out_row != nullptr) {
      for (int i = tid; i < k; i += kSelectThreads) out_row[q * k + i] = -1;
    } else if (gate_cand != nullptr) {
      overflow_gate(gate_cand, count, q, c, cap, thr[q], gate_num, gate_den, &ms->ctr_eq);
    }
    return;
  }
  read_pruned(pre, pre_p, q, k, src, m);
  const int nres = stream_keep_k(src, m, k, l);
  if (out_row != nullptr) {
    for (int j = tid; j < k; j += kSelectThreads) {
      const uint64_t e = j < nres ? l.res[j] : kEmpty;
      out_row[q * k + j] = e == kEmpty ? -1 : (int64_t)(e & 0xffffffffull);
    }
    return;
  }
  if (tid == 0) ms->shmax = 0ull;
  __syncthreads();
  const int grp = tid >> 4, jl = tid & 15;
  const float* qv = Q + q * (int64_t)d;
  const float qn = METRIC == 2 ? qnorm[q] : 0.f;
  uint64_t mx = 0ull;
  for (int j0 = 0; j0 < k; j0 += kSelectThreads / 16) {  // (uniform trip count)
    const int j = j0 + grp;
    const uint64_t e = j < nres ? l.res[j] : kEmpty;
    const int64_t grow = (int64_t)(e & 0xffffffffull);
    const int64_t row = grow - row_base;
    const bool live = j < nres && e != kEmpty && row >= 0 && row < n;
    const float dist =
        row_distance16<T, METRIC>(X + (live ? row : 0) * (int64_t)d, qv, d, jl, live, qn, z);
    // a missing or out-of-shard row: the largest composite (no threshold)
    const uint64_t comp = live ? make_comp(dist, (uint32_t)grow) : kEmpty;
    if (j < k) mx = comp > mx ? comp : mx;
  }
  mx = wave_max_u64(mx);
  if (lane == 0) atomicMax(&ms->shmax, (unsigned long long)mx);
  __syncthreads();
  if (tid == 0) {
    const uint64_t old = thr[q];
    const uint64_t nt = ms->shmax < old ? (uint64_t)ms->shmax : old;
    thr[q] = nt;
    ms->shmax = nt;  // (the gate's threshold)
  }
  if (gate_cand != nullptr) {
    __syncthreads();
    overflow_gate(gate_cand, count, q, c, cap, ms->shmax, gate_num, gate_den, &ms->ctr_eq);
  }
}

// Sample threshold: thr[q] = min(thr[q], the k-th smallest of the query's
// first count[q] keys) when it has at least k.  zero_count as above.
__global__ void __launch_bounds__(kSelectThreads)
    sample_threshold_kernel(const uint64_t* __restrict__ keys, int64_t cap,
                            uint32_t* __restrict__ count, int zero_count, int k, int P2,
                            uint64_t* __restrict__ thr, const uint64_t* __restrict__ pre,
                            int pre_p) {
  const SelectLds l = select_lds(P2);
  MergeShared* ms = l.ms;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t q = blockIdx.y;
  const uint32_t c = count[q * kCountStride];
  int64_t m = (int64_t)c < cap ? (int64_t)c : cap;
  const uint64_t* src = keys + q * cap;
  __syncthreads();
  if (zero_count && tid == 0) count[q * kCountStride] = 0u;
  if (m < k) return;  // (uniform) fewer than k candidates: no threshold
  read_pruned(pre, pre_p, q, k, src, m);
  const int nres = stream_keep_k(src, m, k, l);
  uint64_t mx = 0ull;  // (nres == k: m >= k)
  for (int i = tid; i < nres; i += kSelectThreads) mx = l.res[i] > mx ? l.res[i] : mx;
  mx = wave_max_u64(mx);
  if (tid == 0) ms->shmax = 0ull;
  __syncthreads();
  if (lane == 0) atomicMax(&ms->shmax, (unsigned long long)mx);
  __syncthreads();
  if (tid == 0 && ms->shmax < thr[q]) thr[q] = ms->shmax;
}

// Final select: the k smallest of the query's first count[q] keys (exact
// composites after launch_rescore), bitonic-sorted and decoded to (distance,
// row).  A query whose count exceeds alt_gate (it overflowed the buffer)
// selects from its alt_m entries of alt instead (the overflow fallback scan's
// lists, [nq][alt_m]), whatever the prune pass wrote for it.
__global__ void __launch_bounds__(kSelectThreads)
    final_select_kernel(const uint64_t* __restrict__ keys, int64_t cap,
                        const uint32_t* __restrict__ count, int k, int P2,
                        float* __restrict__ out_dist, int64_t* __restrict__ out_row,
                        const uint64_t* __restrict__ alt, int64_t alt_m, int64_t alt_gate,
                        const uint64_t* __restrict__ pre, int pre_p) {
  const SelectLds l = select_lds(P2);
  const int64_t q = blockIdx.y;
  const uint32_t c = count[q * kCountStride];
  int64_t m = (int64_t)c < cap ? (int64_t)c : cap;
  const uint64_t* src = keys + q * cap;
  if (alt != nullptr && (int64_t)c > alt_gate) {
    m = alt_m;
    src = alt + q * alt_m;
  } else {
    read_pruned(pre, pre_p, q, k, src, m);
  }
  const int nres = stream_keep_k(src, m, k, l);
  if (P2 <= 2 * kWave) {
    wave_sort_decode(l.res, nres, k, out_dist + q * k, out_row + q * k);
  } else {
    lds_sort_decode(l.res, nres, k, P2, out_dist + q * k, out_row + q * k);
  }
}

// Prune pass, before a select over many candidates: grid (pre_p, nq),
// workgroup p keeps the k smallest of the query's entries [p, p + 1) *
// kSelectEntries and writes them (kEmpty-padded) to pre[q][p][k]; the select
// given the same pre then reads the ceil(m / kSelectEntries) k-lists instead
// of streaming all m entries through one workgroup (k = 1 000, ~100 K
// candidates: the one-workgroup select took 160-230 us).  The buffer of a
// query that overflowed is pruned like any other; the final select ignores
// that output in favour of the fallback lists.
__global__ void __launch_bounds__(kSelectThreads)
    prune_kernel(const uint64_t* __restrict__ keys, int64_t cap,
                 const uint32_t* __restrict__ count, int k, int P2, uint64_t* __restrict__ pre,
                 int pre_p) {
  const SelectLds l = select_lds(P2);
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.y;
  const uint32_t c = count[q * kCountStride];
  const int64_t m = (int64_t)c < cap ? (int64_t)c : cap;
  const int64_t lo = (int64_t)blockIdx.x * kSelectEntries;
  if (lo >= m) return;  // (uniform)
  const int cnt = (int)((m - lo) < kSelectEntries ? (m - lo) : kSelectEntries);
  uint64_t* out = pre + (q * pre_p + blockIdx.x) * (int64_t)k;
  block_reset(l.ms);
  __syncthreads();
  uint64_t v_or = 0, v_and = ~0ull;
  stage_chunk(keys + q * cap + lo, cnt, l.s, v_or, v_and);
  block_or_and(v_or, v_and, l.ms);
  __syncthreads();
  if (cnt > k) {
    block_keep_k<kSelectThreads>(l.s, cnt, k, out, l.ms);
  } else {
    for (int i = tid; i < k; i += kSelectThreads) out[i] = i < cnt ? l.s[i] : kEmpty;
  }
}

// The prune pass is used for k >= kPruneMinK when the buffer holds more than
// two slices (int8-image plans at k ~ 1 000: ~100 K candidates per query).
// k-lists per query, 0 = off.  Read by the planner alone (option
// "select_prune"): the launchers below take the plan's PruneScratch.
constexpr int kPruneMinK = 512;
int select_prune_lists(int64_t k, int64_t cap) {
  const int64_t o = option(kOptSelectPrune);
  if (o == 0 || (o == 1 && k < kPruneMinK) || cap <= 2 * (int64_t)kSelectEntries) return 0;
  return (int)((cap + kSelectEntries - 1) / kSelectEntries);
}

size_t select_prune_bytes(int64_t nq, int64_t k, int prune_lists) {
  return (size_t)nq * (size_t)prune_lists * (size_t)k * 8;
}

// P2 and the dynamic LDS of a select at k (select_lds); k within kSelectMaxK
struct SelectShape {
  int P2 = 1;
  size_t smem;
  explicit SelectShape(int k) {
    while (P2 < k) P2 <<= 1;
    smem = sizeof(MergeShared) + ((size_t)P2 + kSelectEntries) * 8;
  }
};
static int check_select_k(const char* what, int k, int64_t limit = kSelectMaxK) {
  if (k <= kSelectMaxK && k <= limit) return FX_OK;
  set_error("%s: k %d above %lld", what, k, (long long)(limit < kSelectMaxK ? limit : kSelectMaxK));
  return FX_EUNSUPPORTED;
}

// The prune pass over keys when the plan has one; the select that follows is
// given the same scratch
static int launch_prune(const uint64_t* keys, int64_t nq, int64_t cap, const uint32_t* count,
                        int k, PruneScratch prune, hipStream_t stream) {
  if (!prune.on()) return FX_OK;
  if (int rc = allow_lds((const void*)prune_kernel)) return rc;
  const SelectShape sh(k);
  return for_query_chunks(nq, [&](int64_t q0, int64_t qn) {
    hipLaunchKernelGGL(prune_kernel, dim3((unsigned)prune.count, (unsigned)qn),
                       dim3(kSelectThreads), sh.smem, stream, keys + q0 * cap, cap,
                       count + q0 * kCountStride, k, sh.P2, prune.from_query(q0, k), prune.count);
    return check_launch("prune_kernel");
  });
}

int launch_exact_threshold(const ExactSource& src, int64_t nq, const uint64_t* keys, int64_t cap,
                           uint32_t* count, bool zero_count, int k, uint64_t* thr,
                           PruneScratch prune, int64_t* topr, OverflowGate gate,
                           hipStream_t stream) {
  if (int rc = check_select_k("exact threshold", k, cap)) return rc;
  if (gate.cand != nullptr && (nq > 0x7fffffffll || gate.den <= 0 || zero_count)) {
    set_error("exact threshold gate: nq=%lld den=%lld zero=%d", (long long)nq,
              (long long)gate.den, (int)zero_count);
    return FX_EINVAL;
  }
  // large k: the pruned select writes the k rows, the chip rescores them
  // (one workgroup rescoring 1 000 rows of 3 KB took ~40 us of its time)
  const bool rows_out = prune.on() && topr != nullptr;
  const OverflowGate fused = rows_out ? OverflowGate() : gate;
  int rc = launch_prune(keys, nq, cap, count, k, prune, stream);
  if (rc) return rc;
  const SelectShape sh(k);
  rc = with_exact_kind(src, [&](auto kind) {
    using K = decltype(kind);
    const auto fn = exact_threshold_kernel<typename K::Row, K::kMetric>;
    if (int e = allow_lds((const void*)fn)) return e;
    return for_query_chunks(nq, [&](int64_t q0, int64_t qn) {
      const ExactSource s = src.from_query(q0);
      hipLaunchKernelGGL(fn, dim3(1u, (unsigned)qn), dim3(kSelectThreads), sh.smem, stream,
                         K::rows(s), s.n, s.d, s.row_base, s.Q, s.qnorm, keys + q0 * cap, cap,
                         count + q0 * kCountStride, zero_count ? 1 : 0, k, sh.P2, thr + q0,
                         rows_out ? topr + q0 * k : nullptr, prune.from_query(q0, k), prune.count,
                         fused.cand != nullptr ? fused.cand + q0 * cap : nullptr, fused.num,
                         fused.den, s.z);
      return check_launch("exact_threshold_kernel");
    });
  });
  if (rc || !rows_out) return rc;
  rc = launch_exact_kth(src, nq, k, topr, thr, stream);
  if (rc || gate.cand == nullptr) return rc;
  return launch_overflow_gate(gate.cand, count, thr, nq, (int)cap, gate.num, gate.den, stream);
}

int launch_sample_threshold(const uint64_t* keys, int64_t nq, int64_t cap, uint32_t* count,
                            bool zero_count, int k, uint64_t* thr, PruneScratch prune,
                            hipStream_t stream) {
  int rc = check_select_k("sample threshold", k);
  if (rc == FX_OK) rc = launch_prune(keys, nq, cap, count, k, prune, stream);
  if (rc) return rc;
  if ((rc = allow_lds((const void*)sample_threshold_kernel))) return rc;
  const SelectShape sh(k);
  return for_query_chunks(nq, [&](int64_t q0, int64_t qn) {
    hipLaunchKernelGGL(sample_threshold_kernel, dim3(1u, (unsigned)qn), dim3(kSelectThreads),
                       sh.smem, stream, keys + q0 * cap, cap, count + q0 * kCountStride,
                       zero_count ? 1 : 0, k, sh.P2, thr + q0, prune.from_query(q0, k),
                       prune.count);
    return check_launch("sample_threshold_kernel");
  });
}

int launch_final_select(const uint64_t* keys, int64_t nq, int64_t cap, const uint32_t* count,
                        int k, float* out_dist, int64_t* out_row, const uint64_t* alt,
                        int64_t alt_m, int64_t alt_gate, PruneScratch prune, hipStream_t stream) {
  int rc = check_select_k("final select", k);
  if (rc == FX_OK) rc = launch_prune(keys, nq, cap, count, k, prune, stream);
  if (rc) return rc;
  if ((rc = allow_lds((const void*)final_select_kernel))) return rc;
  const SelectShape sh(k);
  return for_query_chunks(nq, [&](int64_t q0, int64_t qn) {
    hipLaunchKernelGGL(final_select_kernel, dim3(1u, (unsigned)qn), dim3(kSelectThreads), sh.smem,
                       stream, keys + q0 * cap, cap, count + q0 * kCountStride, k, sh.P2,
                       out_dist + q0 * k, out_row + q0 * k,
                       alt != nullptr ? alt + q0 * alt_m : nullptr, alt_m, alt_gate,
                       prune.from_query(q0, k), prune.count);
    return check_launch("final_select_kernel");
  });
}

}  // namespace fx
