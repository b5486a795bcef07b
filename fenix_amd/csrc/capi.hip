// extern "C" entry points declared in include/fenix_knn.h and the phase
// drivers of the batched filter (plans: knn_plan.hip; errors, options and
// device properties: fx_runtime.hip; the exact-scan entry points: capi_ex.hip).
#include <atomic>

#include "fx_plan.h"

namespace fx {

// host-blocking synchronisations performed (fx_host_sync_count); searches
// perform none, and any added one must go through host_sync
static std::atomic<uint64_t> g_host_syncs{0};

// The fallback scan's arguments: top-k lists into ws, each workgroup gated
// on its query's count (> gate_cap: recompute)
static ScanArgs fallback_args(const SearchLayout& s, const fx_corpus& c, int64_t k,
                              const RowMasks& mask, int64_t gate_cap, char* ws) {
  ScanArgs a = scan_args(s.scan, c, nullptr, 0, mask, k, kModeTopk);
  a.out_lists = reinterpret_cast<uint64_t*>(ws);
  a.gate_cap = gate_cap;
  return a;
}

// The fallback's gated scan alone over all nq queries (s.fb_queries >= nq):
// per overflowing query nlists lists of k composites at *lists, [nq][nlists k]
static int fallback_scan(const SearchLayout& s, const fx_corpus& c, const float* queries,
                         int64_t nq, int64_t k, const RowMasks& mask, const uint32_t* count,
                         int64_t gate_cap, char* ws, hipStream_t st, const uint64_t** lists) {
  ScanArgs a = fallback_args(s, c, k, mask, gate_cap, ws);
  a.q = queries;
  a.gate = count;
  *lists = a.out_lists;
  return launch_scan(s.scan, a, nq, st);
}

// Batched-path fallback: the exact single-query scan + merge of every query
// whose final candidates overflowed the buffer (count[q] > gate_cap; all of
// them when gate_cap < 0), in rounds of s.fb_queries.  Decided on the device:
// each workgroup reads its query's count and returns at once when it did not
// overflow, so nothing waits for the host; the merge writes only the
// recomputed queries' results.
static int fallback_search(const SearchLayout& s, const fx_corpus& c, const float* queries,
                           int64_t nq, int64_t k, const RowMasks& mask, const uint32_t* count,
                           int64_t gate_cap, char* ws, float* out_dist, int64_t* out_row,
                           hipStream_t st) {
  ScanArgs a = fallback_args(s, c, k, mask, gate_cap, ws);
  for (int64_t q0 = 0; q0 < nq; q0 += s.fb_queries) {
    const int64_t qn = (nq - q0) < s.fb_queries ? (nq - q0) : s.fb_queries;
    a.q = queries + (size_t)q0 * c.d;
    a.mask = mask.from_query(q0).mask;  // (per-query masks: the round's first query's)
    a.gate = count + (size_t)q0 * kCountStride;
    int rc = launch_scan(s.scan, a, qn, st);
    if (rc) return rc;
    rc = run_merge(s.merge, a.out_lists, qn, k, ws + s.lists_bytes, out_dist + (size_t)q0 * k,
                   out_row + (size_t)q0 * k, st, nullptr, a.gate, gate_cap);
    if (rc) return rc;
  }
  return FX_OK;
}

// fp16 filter phases (knn_filter.hip; the rescoring: knn_exact.hip).
// Sampling phases append the UPPER bound of every row whose lower bound
// reaches the threshold; the k-th upper bound of any row subset bounds the global k-th distance from above, so it is
// the next phase's threshold.  The final phase (every row) appends lower and
// upper bounds; the k-th upper bound among its candidates is a tighter
// threshold, and only candidates whose lower bound reaches it are rescored
// exactly (the rest are dropped unread).  fx_knn_reduce then selects the top k
// of the exact keys and recomputes overflowing queries.
// With an fp16 filter image of an f32 corpus (fx_filter_image) the phases
// stream the image (half the bytes) and the rescoring reads the f32 rows.
// (An int8 filter image has phases of its own: filter_phases_i8.)
static int filter_phases(const BatchLayout& b, const fx_corpus& c, const void* image,
                         const float* rowinfo, const float* Q, int64_t nq, int metric, int64_t k,
                         const uint32_t* mask, void* ws, hipStream_t st) {
  const BatchWorkspace w(b, ws);
  const ExactSource src = {c.data, c.dtype, c.n, (int)c.d, c.row_base, Q, w.qnorm, metric, Quant()};
  uint16_t* qh = reinterpret_cast<uint16_t*>(w.qh);
  int rc = launch_qprep(Q, nq, b.nq_pad, src.d, b.dq, metric, qh, w.qinfo, st);
  if (rc) return rc;
  if (metric == FX_METRIC_COS) {  // the scan's max(|q|, 1e-12) for the rescoring
    rc = launch_qnorm(Q, nq, src.d, w.qnorm, st);
    if (rc) return rc;
  }
  hipError_t e = hipMemsetAsync(w.thr, 0xFF, (size_t)nq * 8, st);
  // a one-level threshold merge resets the counts it read, so only the first
  // phase needs a fill (each fill is a ~5 us launch)
  const bool merge_zeroes = b.merge.levels == 1;
  for (int ph = 0; ph < b.nphases && e == hipSuccess; ++ph) {
    const bool last = ph + 1 == b.nphases;
    // (the lists are read up to count only: no fill of the candidate buffers)
    if (ph == 0 || !merge_zeroes)
      e = hipMemsetAsync(w.count, 0, (size_t)nq * 4 * kCountStride, st);
    if (e != hipSuccess) break;
    FilterArgs a = {};
    a.X = image != nullptr ? image : c.data;
    a.dtype = image != nullptr ? FX_DTYPE_F16 : c.dtype;
    a.rowinfo = image != nullptr ? rowinfo : nullptr;
    a.n = c.n;
    a.d = src.d;
    a.row_base = c.row_base;
    a.Qh = qh;
    a.dq = b.dq;
    a.qstride = b.nq_pad;
    a.all_pass = ph == 0 ? 1 : 0;  // (thr was just filled with the empty key)
    // sampling phases need only the k smallest upper bounds of their rows:
    // the k rows behind the previous threshold are in this (nested) sample
    // with upper bounds at or below it, so no row whose upper bound exceeds
    // it is among them (option "batch_ub_test" = 0: the lower-bound test)
    a.ub_test = ph > 0 && !last && option(kOptBatchUbTest) != 0 ? 1 : 0;
    a.qinfo = w.qinfo;
    a.nq = nq;
    a.mask = mask;
    a.tile_start = b.start[ph];
    a.tile_stride = b.stride[ph];
    a.num_tiles = b.num[ph];
    a.thr = w.thr;
    a.count = w.count;
    a.cand = w.cand;
    a.cand_ub = last ? w.cand_ub : nullptr;
    a.cap = (int)b.cap;
    a.diag = diag_env("FX_FILTER_DIAG", 0);
    rc = launch_filter(a, metric, st);
    if (rc) return rc;
    // option "filter_hold" (test switch): the last pass's bounds, counts and
    // the threshold it tested against stay in the workspace
    if (last && option(kOptFilterHold) != 0) return FX_OK;
    // the k-th upper bound of this phase's candidates: next threshold
    rc = run_merge(b.merge, last ? w.cand_ub : w.cand, nq, k, w.merge, nullptr, nullptr, st,
                   w.thr, nullptr, 0, w.count, !last);
    if (rc) return rc;
  }
  if (e != hipSuccess) {
    set_error("batched memset: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  return launch_rescore(src, nq, w.count, w.cand, (int)b.cap, w.thr, st);
}

// The int8 image's phases (fx_filter_image8; rows in image8_perm order, so
// every sample is equidistributed over the corpus):
//   sampling phases 0 .. m-3: phase 0 appends every pair of its <= cap rows,
//     later ones the upper bounds at or below the previous threshold; the k-th
//     upper bound is the next threshold, and after phase m-3 the exact
//     distances of the k best upper bounds (launch_exact_kth) set it;
//   F1 (phase m-2, the last sample's prefix of tiles): every pair whose lower bound
//     reaches that threshold, appended with both bounds into the final
//     candidate buffer; the exact k-th of its k best upper bounds is the
//     next, much tighter threshold;
//   overflow gate: F1's candidates under the new threshold, scaled to the
//     tiles left, predict the final count; a query predicted past cap skips
//     the final pass and goes to the exact scan (fx_knn_reduce's fallback);
//   F2 (phase m-1): the tiles after F1's prefix, lower bound against the
//     new threshold, appended after F1's candidates.  Each image row is
//     read once by F1 or F2 (the sampling phases re-read 1/r1 (1/r2 + ...)
//     of them);
//   the exact k-th of all candidates' k best upper bounds is the final
//     threshold (batches of more than kI8RescoreAllMaxQ queries; smaller ones
//     keep F1's), and the candidates whose lower bound reaches it are
//     rescored exactly (launch_rescore), fx_knn_reduce selects the top k.
// quint8 codes (dtype FX_DTYPE_QU8, z their scale and zero point; the image
// is image8_qu8_kernel's): the exact distances repeat the quint8 scan, whose
// L2 form reads q' = zp + q / scale.  q' is computed once into the workspace
// (launch_qu8_query); the rescoring reads it, and the filter bounds the scan's
// effective query scale * (q' - zp) (launch_qprep8; the derivation is beside
// image8_qu8_kernel, knn_filter.hip).  IP and cosine take the queries as they are.
static constexpr int64_t kI8RescoreAllMaxQ = 2;

// Per-query row masks (mask.qstride != 0; the plan's BatchLayout::qmask): every
// filter pass tests the pair's admission bit from the packed matrix
// mask.qmask (launch_filter: filter_img6_kernel<., true>); the selects, the
// gate and the rescoring see only appended candidates.
static int filter_phases_i8(const BatchLayout& b, const fx_corpus& c, const void* image,
                            const float* rowinfo, const float* Q, int64_t nq, int metric,
                            int64_t k, const RowMasks& mask, void* ws, hipStream_t st) {
  const BatchWorkspace w(b, ws);
  const bool per_query = mask.qstride != 0;
  if (per_query && (!b.qmask || mask.qmask == nullptr || (uintptr_t)mask.qmask % 16 != 0 ||
                    mask.qwords < qmask_words(nq))) {
    set_error("per-query masks: no packed bit matrix (fx_qmask_pack), or not 16-byte aligned");
    return FX_EINVAL;
  }
  const Quant z = {c.scale, (float)c.zero_point};
  const int d = (int)c.d;
  const int64_t nq_pad8 = (nq + 255) / 256 * 256;
  int rc;
  const bool qu8_l2 = c.dtype == FX_DTYPE_QU8 && metric == FX_METRIC_L2;
  if (qu8_l2) {  // from here on Q is the quint8 scan's q' (L2 needs no |q|)
    rc = launch_qu8_query(Q, nq, d, z, w.qt, st);
    if (rc) return rc;
    Q = w.qt;
  }
  const ExactSource src = {c.data, c.dtype, c.n, d, c.row_base, Q, w.qnorm, metric, z};
  // (the query prep also empties thr and zeroes the counts)
  rc = launch_qprep8(Q, nq, nq_pad8, d, b.dq, metric, reinterpret_cast<int8_t*>(w.qh), w.qinfo,
                     st, w.thr, w.count, qu8_l2 ? &z : nullptr);
  if (rc) return rc;
  if (metric == FX_METRIC_COS) {  // the scan's max(|q|, 1e-12) for the exact distances
    rc = launch_qnorm(Q, nq, d, w.qnorm, st);
    if (rc) return rc;
  }
  auto args = [&](int ph) {
    FilterArgs a = {};
    a.X = image;
    a.dtype = FX_DTYPE_F16;
    a.rowinfo = rowinfo;
    a.n = c.n;
    a.d = d;
    a.row_base = c.row_base;
    a.Qh = reinterpret_cast<const uint16_t*>(w.qh);
    a.dq = b.dq;
    a.qstride = nq_pad8;
    a.img8 = 1;
    a.perm_a = image8_perm(c.n);
    a.qinfo = w.qinfo;
    a.nq = nq;
    a.mask = per_query ? nullptr : mask.mask;
    a.qmask = per_query ? mask.qmask : nullptr;
    a.qmask_words = per_query ? mask.qwords : 0;
    a.tile_start = b.start[ph];
    a.tile_stride = b.stride[ph];
    a.num_tiles = b.num[ph];
    a.thr = w.thr;
    a.count = w.count;
    a.cand = w.cand;
    a.cap = (int)b.cap;
    a.diag = diag_env("FX_FILTER_DIAG", 0);
    return a;
  };
  // the exact k-th of the k best upper bounds in `keys` -> thr (one fused
  // launch when the buffer fits one workgroup's LDS)
  auto exact_threshold = [&](const uint64_t* keys, bool zero, OverflowGate gate = OverflowGate()) {
    return launch_exact_threshold(src, nq, keys, b.cap, w.count, zero, (int)k, w.thr, w.prune,
                                  w.topr, gate, st);
  };
  const int m = b.nphases;
  for (int ph = 0; ph + 2 < m; ++ph) {  // sampling phases: thresholds only
    FilterArgs a = args(ph);
    a.all_pass = ph == 0 ? 1 : 0;
    a.ub_test = ph > 0 && option(kOptBatchUbTest) != 0 ? 1 : 0;
    rc = launch_filter(a, metric, st);
    if (rc) return rc;
    // (both reset the counts they read: the next phase appends from 0)
    rc = ph + 3 == m ? exact_threshold(w.cand, true)
                     : launch_sample_threshold(w.cand, nq, b.cap, w.count, true, (int)k, w.thr,
                                               w.prune, st);
    if (rc) return rc;
  }
  // F1: the last sample's tiles (with one phase: every tile), both bounds
  FilterArgs f1 = args(m >= 2 ? m - 2 : 0);
  f1.all_pass = m <= 2 ? 1 : 0;
  f1.cand_ub = w.cand_ub;
  rc = launch_filter(f1, metric, st);
  if (rc) return rc;
  // option "filter_hold" (test switch): return after the last filter pass, its
  // bounds, counts and the threshold it tested against left in the workspace
  const bool hold = option(kOptFilterHold) != 0;
  if (m >= 2) {
    const int64_t t1 = b.num[m - 2], t2 = b.tiles - t1;
    if (hold && t2 <= 0) return FX_OK;
    // F1's threshold, then (t2 > 0) the overflow gate on it (launch_overflow_gate's
    // prediction, run by the select's own workgroups)
    rc = t2 > 0 ? exact_threshold(w.cand_ub, false, OverflowGate{w.cand, t2, t1})
                : exact_threshold(w.cand_ub, false);
    if (rc) return rc;
    if (t2 > 0) {
      // F2: the tiles after F1's prefix
      FilterArgs f2 = args(m - 1);
      f2.tile_start = t1;
      f2.num_tiles = t2;
      f2.cand_ub = w.cand_ub;
      f2.skip_full = 1;
      rc = launch_filter(f2, metric, st);
      if (rc) return rc;
    }
  }
  if (hold) return FX_OK;
  // the final threshold only pays for itself on a batch: one or two queries
  // rescore every candidate under F1's threshold instead (a few thousand 3 KB
  // rows, ~3-6 us spread over the chip, against a ~25 us one-workgroup select)
  if (m < 2 || nq > kI8RescoreAllMaxQ) {
    rc = exact_threshold(w.cand_ub, false);
    if (rc) return rc;
  }
  return launch_rescore(src, nq, w.count, w.cand, (int)b.cap, w.thr, st);
}

}  // namespace fx

using namespace fx;

extern "C" {

int fx_version(void) { return 104; }

const char* fx_last_error(void) { return last_error(); }

int fx_set_option(const char* name, int64_t value) { return set_option(name, value); }

int fx_get_option(const char* name, int64_t* out) { return get_option(name, out); }

uint64_t fx_host_sync_count(void) { return g_host_syncs.load(std::memory_order_relaxed); }

int fx_device_count(int* out) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
    *out = 0;
    return FX_EHIP;
  }
  *out = c;
  return FX_OK;
}

int64_t fx_max_k(void) { return kMaxK; }

int fx_knn_workspace_bytes(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k,
                           size_t* out_bytes) {
  return fx_knn_workspace_bytes_img8(n, d, dtype, nq, k, 1, out_bytes);
}

int fx_knn_workspace_bytes_img8(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k,
                                int img8, size_t* out_bytes) {
  if (!out_bytes) {
    set_error("out_bytes is null");
    return FX_EINVAL;
  }
  int rc = validate(n, d, dtype, nq, k, FX_METRIC_L2, true);
  if (rc) return rc;
  size_t best = 0;
  for (int metric = 0; metric < 3; ++metric) {
    for (int aligned = 0; aligned < 2; ++aligned) {
      // with an int8 image a search may still plan without it (k above
      // i8_max_k): the larger of both; without one, the image-free plan only
      // (and a search with per-query masks may plan exact where the plain
      // one plans the filter)
      for (int with8 = 0; with8 < (img8 ? 2 : 1); ++with8) {
        for (int qm = 0; qm < 2; ++qm) {
          SearchLayout s;
          rc = plan_search(n, d, dtype, nq, k, metric, aligned != 0, with8 != 0, &s, qm != 0);
          if (rc) return rc;
          if (s.total > best) best = s.total;
        }
      }
    }
  }
  *out_bytes = best;
  return FX_OK;
}

}  // extern "C"

// One call's plan: arguments checked (shape, k, then null pointers), planned
// once from the options as they are now, and held against the workspace the
// call brought.  img8: the call supplies an int8 filter image.  qu8: the
// entry point takes quint8 codes (a descriptor with their scale and zero
// point, or a call that only reads the plan).
static int search_layout(const fx_corpus& c, int64_t nq, int metric, int64_t k, bool img8,
                         const void* ws, size_t ws_bytes, SearchLayout* s, bool qu8 = false,
                         bool qmask = false) {
  int rc = validate(c.n, c.d, c.dtype, nq, k, metric, qu8);
  if (rc) return rc;
  rc = validate_quant(c);
  if (rc) return rc;
  if (!c.data || !ws) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  rc = plan_search(c.n, c.d, c.dtype, nq, k, metric, ((uintptr_t)c.data % 16) == 0, img8, s,
                   qmask);
  if (rc) return rc;
  if (ws_bytes < s->total) {
    set_error("workspace too small: %zu < %zu", ws_bytes, s->total);
    return FX_EINVAL;
  }
  return FX_OK;
}

// a filter image applies to rows of whole 16-B pieces (d % 8 == 0) through
// the filter: an int8 image where the plan took it (BatchLayout::img8, any
// dtype), an fp16 image to f32 rows
static bool image_applies(const SearchLayout& s, const fx_corpus& c, bool img8) {
  if (!s.batched) return false;
  return img8 ? s.batch.img8 : c.d % 8 == 0 && c.dtype == FX_DTYPE_F32;
}

static int scan_impl(const SearchLayout& s, const fx_corpus& c, const void* image,
                     const float* rowinfo, bool img8, const float* queries, int64_t nq,
                     int metric, int64_t k, const RowMasks& mask, void* ws, hipStream_t st) {
  if (!queries) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if (c.row_base < 0 || c.row_base + c.n >= 0xffffffffll) {
    set_error("global rows [%lld, %lld) exceed the 32-bit row space", (long long)c.row_base,
              (long long)(c.row_base + c.n));
    return FX_EUNSUPPORTED;
  }
  if (s.batched) {
    const bool img = image != nullptr && image_applies(s, c, img8);
    if (img && (rowinfo == nullptr || (uintptr_t)image % 16 != 0)) {
      set_error("filter image: null row info or image not 16-byte aligned");
      return FX_EINVAL;
    }
    if (img && img8)
      return filter_phases_i8(s.batch, c, image, rowinfo, queries, nq, metric, k, mask, ws, st);
    if (c.dtype == FX_DTYPE_QU8) {  // (unreachable: quint8 batches are planned on an image)
      set_error("quint8 batch without an int8 filter image");
      return FX_EINVAL;
    }
    if (mask.qstride != 0) {  // (unreachable: per-query masks plan an int8 image or exact)
      set_error("per-query masks without an int8 filter image");
      return FX_EINVAL;
    }
    return filter_phases(s.batch, c, img ? image : nullptr, rowinfo, queries, nq, metric, k,
                         mask.mask, ws, st);
  }
  char* w = reinterpret_cast<char*>(ws);
  if (s.large) {
    ScanArgs a = scan_args(s.scan, c, nullptr, 0, mask, 1, kModeDist);
    a.q = queries;
    return large_scan(s.scan, a, nq, s.lg, w, st);
  }
  ScanArgs a = scan_args(s.scan, c, nullptr, 0, mask, k, kModeTopk);
  a.q = queries;
  a.out_lists = reinterpret_cast<uint64_t*>(ws);
  return launch_scan_queries(s.scan, a, nq, st);
}

// The scan half of a search call: plan, then run (fx_knn_scan*)
static int scan_call(const fx_corpus& c, const void* image, const float* rowinfo, bool img8,
                     const float* queries, int64_t nq, int metric, int64_t k,
                     const RowMasks& mask, void* ws, size_t ws_bytes, void* stream,
                     bool qu8 = false) {
  SearchLayout s;
  int rc = search_layout(c, nq, metric, k, img8 && image != nullptr, ws, ws_bytes, &s, qu8,
                         mask.qstride != 0);
  if (rc) return rc;
  return scan_impl(s, c, image, rowinfo, img8, queries, nq, metric, k, mask, ws,
                   reinterpret_cast<hipStream_t>(stream));
}

static int reduce_impl(const SearchLayout& s, const fx_corpus& c, const float* queries,
                       int64_t nq, int64_t k, const RowMasks& mask, void* ws, float* out_dist,
                       int64_t* out_row, hipStream_t st) {
  if (!out_dist || !out_row) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  char* w = reinterpret_cast<char*>(ws);
  if (s.large) return large_reduce(c.n, nq, k, s.lg, w, out_dist, out_row, st);
  if (!s.batched) {
    const uint64_t* lists = reinterpret_cast<const uint64_t*>(ws);
    return run_merge(s.merge, lists, nq, k, w + s.lists_bytes, out_dist, out_row, st);
  }
  // batched: final select over the last phase's candidates
  const BatchLayout& b = s.batch;
  const BatchWorkspace bw(b, ws);
  // queries whose candidates overflowed `cap` are recomputed exactly, gated
  // on the device ("force_fallback" (test switch): every query)
  const int64_t gate_cap = option(kOptForceFallback) != 0 ? -1 : b.cap;
  int rc;
  if (b.img8 && s.fb_queries >= nq) {
    // one round: the gated scan's lists feed the final select of the
    // overflowing queries (no merge levels of their own)
    const uint64_t* lists = nullptr;
    rc = fallback_scan(s, c, queries, nq, k, mask, bw.count, gate_cap, w + s.single_off, st,
                       &lists);
    if (rc) return rc;
    return launch_final_select(bw.cand, nq, b.cap, bw.count, (int)k, out_dist, out_row, lists,
                               s.scan.nlists * k, gate_cap, bw.prune, st);
  }
  // (the fallback gate reads the counts next: kept)
  rc = b.img8 ? launch_final_select(bw.cand, nq, b.cap, bw.count, (int)k, out_dist, out_row,
                                    nullptr, 0, 0, bw.prune, st)
              : run_merge(b.merge, bw.cand, nq, k, bw.merge, out_dist, out_row, st, nullptr,
                          nullptr, 0, bw.count);
  if (rc) return rc;
  return fallback_search(s, c, queries, nq, k, mask, bw.count, gate_cap, w + s.single_off,
                         out_dist, out_row, st);
}

// The reduce half of a search call (fx_knn_reduce*): its own plan, which
// equals the scan half's as long as no option changed in between
static int reduce_call(const fx_corpus& c, bool img8, const float* queries, int64_t nq, int metric,
                       int64_t k, const RowMasks& mask, void* ws, size_t ws_bytes, float* out_dist,
                       int64_t* out_row, void* stream, bool qu8 = false) {
  SearchLayout s;
  int rc = search_layout(c, nq, metric, k, img8, ws, ws_bytes, &s, qu8, mask.qstride != 0);
  if (rc) return rc;
  return reduce_impl(s, c, queries, nq, k, mask, ws, out_dist, out_row,
                     reinterpret_cast<hipStream_t>(stream));
}

// A whole search (fx_knn_search*): one plan runs both halves
static int search_call(const fx_corpus& c, const void* image, const float* rowinfo, bool img8,
                       const float* queries, int64_t nq, int metric, int64_t k,
                       const RowMasks& mask, void* ws, size_t ws_bytes, float* out_dist,
                       int64_t* out_row, void* stream, bool qu8 = false) {
  if (!out_dist || !out_row) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  SearchLayout s;
  int rc = search_layout(c, nq, metric, k, img8 && image != nullptr, ws, ws_bytes, &s, qu8,
                         mask.qstride != 0);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  rc = scan_impl(s, c, image, rowinfo, img8, queries, nq, metric, k, mask, ws, st);
  if (rc) return rc;
  return reduce_impl(s, c, queries, nq, k, mask, ws, out_dist, out_row, st);
}

extern "C" {

int fx_knn_scan(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                const float* queries, int64_t nq, int metric, int64_t k,
                const uint32_t* mask, void* ws, size_t ws_bytes, void* stream) {
  return scan_call(corpus_of(corpus, dtype, n, d, row_base), nullptr, nullptr, false, queries, nq, metric,
                   k, mask, ws, ws_bytes, stream);
}

int fx_knn_scan_img(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                    const void* image, const float* rowinfo, const float* queries, int64_t nq,
                    int metric, int64_t k, const uint32_t* mask, void* ws, size_t ws_bytes,
                    void* stream) {
  return scan_call(corpus_of(corpus, dtype, n, d, row_base), image, rowinfo, false, queries, nq, metric,
                   k, mask, ws, ws_bytes, stream);
}

int fx_knn_scan_img8(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                     const void* image, const float* rowinfo, const float* queries, int64_t nq,
                     int metric, int64_t k, const uint32_t* mask, void* ws, size_t ws_bytes,
                     void* stream) {
  return scan_call(corpus_of(corpus, dtype, n, d, row_base), image, rowinfo, true, queries, nq, metric,
                   k, mask, ws, ws_bytes, stream);
}

int fx_filter_image_bytes(int64_t n, int64_t d, size_t* image_bytes, size_t* rowinfo_bytes) {
  if (!image_bytes || !rowinfo_bytes) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if (n < 0 || d < 8 || d % 8 != 0) {
    set_error("filter image: n=%lld d=%lld (d must be a positive multiple of 8)", (long long)n,
              (long long)d);
    return FX_EUNSUPPORTED;
  }
  *image_bytes = image_tiled() ? (size_t)((n + 31) / 32) * (size_t)((d + 15) / 16) * 1024
                               : (size_t)n * (size_t)d * 2;
  *rowinfo_bytes = (size_t)n * 4;
  return FX_OK;
}

int fx_filter_image(const float* corpus, int64_t n, int64_t d, void* image, float* rowinfo,
                    void* stream) {
  size_t ib = 0, rb = 0;
  int rc = fx_filter_image_bytes(n, d, &ib, &rb);
  if (rc) return rc;
  if (n > 0 && (!corpus || !image || !rowinfo)) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if ((uintptr_t)corpus % 16 != 0 || (uintptr_t)image % 16 != 0) {
    set_error("filter image: corpus and image must be 16-byte aligned");
    return FX_EINVAL;
  }
  if (d > 0x7fffffffll) {
    set_error("filter image: d=%lld too large", (long long)d);
    return FX_EUNSUPPORTED;
  }
  return launch_image(corpus, n, (int)d, image, rowinfo, reinterpret_cast<hipStream_t>(stream));
}

int fx_filter_image8_bytes(int64_t n, int64_t d, size_t* image_bytes, size_t* rowinfo_bytes) {
  if (!image_bytes || !rowinfo_bytes) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if (n < 0 || d < 8 || d % 8 != 0) {
    set_error("filter image: n=%lld d=%lld (d must be a positive multiple of 8)", (long long)n,
              (long long)d);
    return FX_EUNSUPPORTED;
  }
  *image_bytes = (size_t)((n + 31) / 32) * (size_t)((d + 31) / 32) * 1024;
  *rowinfo_bytes = (size_t)n * kI8RowInfo * 4;
  return FX_OK;
}

int fx_filter_image8_perm(int64_t n, uint64_t* mult) {
  if (!mult || n < 0) {
    set_error("fx_filter_image8_perm: n=%lld", (long long)n);
    return FX_EINVAL;
  }
  *mult = image8_perm(n);
  return FX_OK;
}

int fx_filter_image8(const float* corpus, int64_t n, int64_t d, void* image, float* rowinfo,
                     void* stream) {
  return fx_filter_image8_typed(corpus, FX_DTYPE_F32, n, d, image, rowinfo, stream);
}

int fx_filter_image8_typed(const void* corpus, int dtype, int64_t n, int64_t d, void* image,
                           float* rowinfo, void* stream) {
  if (dtype != FX_DTYPE_F32 && dtype != FX_DTYPE_F16) {
    set_error("filter image: dtype %d is not float32 or float16", dtype);
    return FX_EINVAL;
  }
  size_t ib = 0, rb = 0;
  int rc = fx_filter_image8_bytes(n, d, &ib, &rb);
  if (rc) return rc;
  if (n > 0 && (!corpus || !image || !rowinfo)) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if ((uintptr_t)corpus % 16 != 0 || (uintptr_t)image % 16 != 0 || (uintptr_t)rowinfo % 16 != 0) {
    set_error("filter image: corpus, image and row info must be 16-byte aligned");
    return FX_EINVAL;
  }
  if (d > 0x7fffffffll) {
    set_error("filter image: d=%lld too large", (long long)d);
    return FX_EUNSUPPORTED;
  }
  return launch_image8(corpus, dtype, n, (int)d, image, rowinfo,
                       reinterpret_cast<hipStream_t>(stream));
}

int fx_filter_image_used(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric,
                         int* out) {
  if (!out) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  *out = 0;
  int rc = validate(n, d, dtype, nq, k, metric, true);
  if (rc) return rc;
  SearchLayout s;
  // (the int8 image, the host's default, also serves single queries over
  // large corpora: use_batched)
  const bool img8 = option(kOptFilterImage) == 8;
  rc = plan_search(n, d, dtype, nq, k, metric, true, img8, &s);
  if (rc) return rc;
  *out = image_applies(s, corpus_of(nullptr, dtype, n, d, 0), img8) ? 1 : 0;
  return FX_OK;
}

int fx_knn_filter_state(const void* corpus, int dtype, int64_t n, int64_t d, int64_t nq,
                        int metric, int64_t k, int img8, const void* ws, size_t ws_bytes,
                        uint64_t* out_thr, uint64_t* out_cand, uint64_t* out_cand_ub,
                        void* stream) {
  SearchLayout s;
  int rc = search_layout(corpus_of(corpus, dtype, n, d, 0), nq, metric, k, img8 != 0, ws,
                         ws_bytes, &s, true);
  if (rc) return rc;
  if (!s.batched) {
    set_error("fx_knn_filter_state: the search did not run the filter");
    return FX_EINVAL;
  }
  const BatchWorkspace w(s.batch, const_cast<void*>(ws));  // (read only)
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t cb = (size_t)nq * s.batch.cap * 8;
  hipError_t e = hipSuccess;
  if (out_thr) e = hipMemcpyAsync(out_thr, w.thr, (size_t)nq * 8, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && out_cand)
    e = hipMemcpyAsync(out_cand, w.cand, cb, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && out_cand_ub)
    e = hipMemcpyAsync(out_cand_ub, w.cand_ub, cb, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) {
    set_error("fx_knn_filter_state: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  return FX_OK;
}

int fx_knn_filter_counts(const void* corpus, int dtype, int64_t n, int64_t d, int64_t nq,
                         int metric, int64_t k, int img8, const void* ws, size_t ws_bytes,
                         uint32_t* out_counts, int64_t* out_cap, void* stream) {
  SearchLayout s;
  int rc = search_layout(corpus_of(corpus, dtype, n, d, 0), nq, metric, k, img8 != 0, ws,
                         ws_bytes, &s, true);
  if (rc) return rc;
  if (!out_counts || !out_cap) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if (!s.batched) {
    *out_cap = -1;
    return FX_OK;
  }
  *out_cap = s.batch.cap;
  const BatchWorkspace w(s.batch, const_cast<void*>(ws));  // (read only)
  hipError_t e = hipMemcpy2DAsync(out_counts, 4, w.count, 4 * kCountStride, 4, (size_t)nq,
                                  hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) {
    set_error("fx_knn_filter_counts: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  return FX_OK;
}

int fx_knn_reduce(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                  const float* queries, int64_t nq, int metric, int64_t k,
                  const uint32_t* mask, void* ws, size_t ws_bytes, float* out_dist,
                  int64_t* out_row, void* stream) {
  return reduce_call(corpus_of(corpus, dtype, n, d, row_base), false, queries, nq, metric, k, mask,
                     ws, ws_bytes, out_dist, out_row, stream);
}

int fx_knn_reduce_img8(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                       const void* image, const float* queries, int64_t nq, int metric, int64_t k,
                       const uint32_t* mask, void* ws, size_t ws_bytes, float* out_dist,
                       int64_t* out_row, void* stream) {
  return reduce_call(corpus_of(corpus, dtype, n, d, row_base), image != nullptr, queries, nq,
                     metric, k, mask, ws, ws_bytes, out_dist, out_row, stream);
}

int fx_knn_search(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                  const float* queries, int64_t nq, int metric, int64_t k,
                  const uint32_t* mask, void* ws, size_t ws_bytes, float* out_dist,
                  int64_t* out_row, void* stream) {
  return search_call(corpus_of(corpus, dtype, n, d, row_base), nullptr, nullptr, false, queries,
                     nq, metric, k, mask, ws, ws_bytes, out_dist, out_row, stream);
}

int fx_knn_search_img(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                      const void* image, const float* rowinfo, const float* queries, int64_t nq,
                      int metric, int64_t k, const uint32_t* mask, void* ws, size_t ws_bytes,
                      float* out_dist, int64_t* out_row, void* stream) {
  return search_call(corpus_of(corpus, dtype, n, d, row_base), image, rowinfo, false, queries, nq,
                     metric, k, mask, ws, ws_bytes, out_dist, out_row, stream);
}

int fx_knn_search_img8(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                       const void* image, const float* rowinfo, const float* queries, int64_t nq,
                       int metric, int64_t k, const uint32_t* mask, void* ws, size_t ws_bytes,
                       float* out_dist, int64_t* out_row, void* stream) {
  return search_call(corpus_of(corpus, dtype, n, d, row_base), image, rowinfo, true, queries, nq,
                     metric, k, mask, ws, ws_bytes, out_dist, out_row, stream);
}

// The descriptor forms of the int8-image entry points: any dtype, and the
// only ones that take quint8 codes (their scale and zero point travel in the
// fx_corpus).  Same plans and drivers as the plain-argument forms.
static const fx_corpus* checked_corpus(const fx_corpus* c) {
  if (c == nullptr || c->data == nullptr) {
    set_error("null corpus");
    return nullptr;
  }
  return c;
}

int fx_filter_image8_ex(const fx_corpus* c, void* image, float* rowinfo, void* stream) {
  if (!checked_corpus(c)) return FX_EINVAL;
  if (c->dtype != FX_DTYPE_QU8)
    return fx_filter_image8_typed(c->data, c->dtype, c->n, c->d, image, rowinfo, stream);
  size_t ib = 0, rb = 0;
  int rc = fx_filter_image8_bytes(c->n, c->d, &ib, &rb);
  if (rc) return rc;
  if (c->d % 16 != 0 || c->d > 0x7fffffffll) {
    set_error("filter image: quint8 rows need d %% 16 == 0, d=%lld", (long long)c->d);
    return FX_EUNSUPPORTED;
  }
  rc = validate_quant(*c);
  if (rc) return rc;
  if (c->n > 0 && (!image || !rowinfo)) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if ((uintptr_t)c->data % 16 != 0 || (uintptr_t)image % 16 != 0 || (uintptr_t)rowinfo % 16 != 0) {
    set_error("filter image: corpus, image and row info must be 16-byte aligned");
    return FX_EINVAL;
  }
  return launch_image8(c->data, c->dtype, c->n, (int)c->d, image, rowinfo,
                       reinterpret_cast<hipStream_t>(stream), Quant{c->scale, (float)c->zero_point});
}

int fx_knn_scan_img8_ex(const fx_corpus* c, const void* image, const float* rowinfo,
                        const float* queries, int64_t nq, int metric, int64_t k,
                        const uint32_t* mask, void* ws, size_t ws_bytes, void* stream) {
  if (!checked_corpus(c)) return FX_EINVAL;
  return scan_call(*c, image, rowinfo, true, queries, nq, metric, k, mask, ws, ws_bytes, stream,
                   true);
}

int fx_knn_reduce_img8_ex(const fx_corpus* c, const void* image, const float* queries, int64_t nq,
                          int metric, int64_t k, const uint32_t* mask, void* ws, size_t ws_bytes,
                          float* out_dist, int64_t* out_row, void* stream) {
  if (!checked_corpus(c)) return FX_EINVAL;
  return reduce_call(*c, image != nullptr, queries, nq, metric, k, mask, ws, ws_bytes, out_dist,
                     out_row, stream, true);
}

int fx_knn_search_img8_ex(const fx_corpus* c, const void* image, const float* rowinfo,
                          const float* queries, int64_t nq, int metric, int64_t k,
                          const uint32_t* mask, void* ws, size_t ws_bytes, float* out_dist,
                          int64_t* out_row, void* stream) {
  if (!checked_corpus(c)) return FX_EINVAL;
  return search_call(*c, image, rowinfo, true, queries, nq, metric, k, mask, ws, ws_bytes,
                     out_dist, out_row, stream, true);
}

// Per-query row masks (include/fenix_knn.h "Per-query row masks"): the
// *_img8_ex triple with every query's own bitmap, masks + q * mask_stride, and
// their packed bit matrix (fx_qmask_pack) for the filter passes.  masks NULL:
// every query admits every row (the plain search).
int64_t fx_qmask_words(int64_t nq) { return qmask_words(nq); }

int fx_qmask_pack(const uint32_t* masks, int64_t mask_stride, int64_t nq, int64_t n, uint32_t* out,
                  void* stream) {
  if (nq < 1 || n < 1 || n >= 0xffffffffll || mask_stride < (n + 31) / 32) {
    set_error("fx_qmask_pack: nq=%lld n=%lld mask_stride=%lld", (long long)nq, (long long)n,
              (long long)mask_stride);
    return FX_EINVAL;
  }
  if (!masks || !out || (uintptr_t)out % 16 != 0) {
    set_error("fx_qmask_pack: null pointer argument, or out not 16-byte aligned");
    return FX_EINVAL;
  }
  return launch_qmask_pack(masks, mask_stride, nq, n, out, reinterpret_cast<hipStream_t>(stream));
}

static int qmask_row_masks(const fx_corpus* c, const uint32_t* masks, int64_t mask_stride,
                           const uint32_t* qmask, int64_t nq, int64_t k, RowMasks* m) {
  if (!checked_corpus(c)) return FX_EINVAL;
  if (k > kMaxK) {
    set_error("per-query masks: k=%lld outside [1, %lld]", (long long)k, (long long)kMaxK);
    return FX_EUNSUPPORTED;
  }
  *m = RowMasks();
  if (masks == nullptr) return FX_OK;
  if (mask_stride < (c->n + 31) / 32 || mask_stride > 0x7fffffffll) {
    set_error("per-query masks: mask_stride=%lld below the %lld words of a bitmap",
              (long long)mask_stride, (long long)((c->n + 31) / 32));
    return FX_EINVAL;
  }
  m->mask = masks;
  m->qstride = mask_stride;
  m->qmask = qmask;
  m->qwords = qmask_words(nq);
  return FX_OK;
}

int fx_qmask_filter_used(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric,
                         int* out) {
  if (!out) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  *out = 0;
  int rc = validate(n, d, dtype, nq, k, metric, true);
  if (rc) return rc;
  SearchLayout s;
  rc = plan_search(n, d, dtype, nq, k, metric, true, option(kOptFilterImage) == 8, &s, true);
  if (rc) return rc;
  if (s.batched && s.batch.qmask) *out = filter_qmask_kind(s.batch.dq, nq);
  return FX_OK;
}

int fx_knn_scan_qmask_ex(const fx_corpus* c, const void* image, const float* rowinfo,
                         const float* queries, int64_t nq, int metric, int64_t k,
                         const uint32_t* masks, int64_t mask_stride, const uint32_t* qmask,
                         void* ws, size_t ws_bytes, void* stream) {
  RowMasks m;
  if (int rc = qmask_row_masks(c, masks, mask_stride, qmask, nq, k, &m)) return rc;
  return scan_call(*c, image, rowinfo, true, queries, nq, metric, k, m, ws, ws_bytes, stream,
                   true);
}

int fx_knn_reduce_qmask_ex(const fx_corpus* c, const void* image, const float* queries,
                           int64_t nq, int metric, int64_t k, const uint32_t* masks,
                           int64_t mask_stride, const uint32_t* qmask, void* ws, size_t ws_bytes,
                           float* out_dist, int64_t* out_row, void* stream) {
  RowMasks m;
  if (int rc = qmask_row_masks(c, masks, mask_stride, qmask, nq, k, &m)) return rc;
  return reduce_call(*c, image != nullptr, queries, nq, metric, k, m, ws, ws_bytes, out_dist,
                     out_row, stream, true);
}

int fx_knn_search_qmask_ex(const fx_corpus* c, const void* image, const float* rowinfo,
                           const float* queries, int64_t nq, int metric, int64_t k,
                           const uint32_t* masks, int64_t mask_stride, const uint32_t* qmask,
                           void* ws, size_t ws_bytes, float* out_dist, int64_t* out_row,
                           void* stream) {
  RowMasks m;
  if (int rc = qmask_row_masks(c, masks, mask_stride, qmask, nq, k, &m)) return rc;
  return search_call(*c, image, rowinfo, true, queries, nq, metric, k, m, ws, ws_bytes, out_dist,
                     out_row, stream, true);
}

// merges of lists longer than the fused path's k go through the radix sort
static bool merge_is_large(int64_t kin, int64_t k) { return k > kMaxK || kin > kMaxK; }

int fx_topk_merge_workspace_bytes(int64_t nq, int64_t parts, int64_t kin, int64_t k,
                                  size_t* out_bytes) {
  if (!out_bytes || nq < 1 || parts < 1 || kin < 1 || k < 1 || k > kLargeMaxK ||
      parts * kin > kLargeMaxK) {
    set_error("invalid merge shape");
    return FX_EINVAL;
  }
  if (merge_is_large(kin, k)) {
    *out_bytes = plan_large(parts * kin, nq).total;
    return FX_OK;
  }
  MergePlan mp;
  int rc = plan_merge(nq, parts, kin, k, &mp);
  if (rc) return rc;
  *out_bytes = align256((size_t)nq * parts * kin * 8) + mp.ws_bytes;
  return FX_OK;
}

int fx_topk_merge(const float* in_dist, const int64_t* in_row, int64_t nq, int64_t parts,
                  int64_t kin, int64_t k, void* ws, size_t ws_bytes, float* out_dist,
                  int64_t* out_row, void* stream) {
  size_t need = 0;
  int rc = fx_topk_merge_workspace_bytes(nq, parts, kin, k, &need);
  if (rc) return rc;
  if (!in_dist || !in_row || !ws || !out_dist || !out_row) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if (ws_bytes < need) {
    set_error("workspace too small: %zu < %zu", ws_bytes, need);
    return FX_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (merge_is_large(kin, k)) {
    const LargeLayout l = plan_large(parts * kin, nq);
    char* w = reinterpret_cast<char*>(ws);
    rc = launch_encode(in_dist, in_row, nq * parts * kin,
                       reinterpret_cast<uint64_t*>(w + l.off_keys), st);
    if (rc) return rc;
    return large_reduce(parts * kin, nq, k, l, w, out_dist, out_row, st);
  }
  MergePlan mp;
  rc = plan_merge(nq, parts, kin, k, &mp);
  if (rc) return rc;
  uint64_t* comp = reinterpret_cast<uint64_t*>(ws);
  void* mws = reinterpret_cast<char*>(ws) + align256((size_t)nq * parts * kin * 8);
  rc = launch_encode(in_dist, in_row, nq * parts * kin, comp, st);
  if (rc) return rc;
  return run_merge(mp, comp, nq, k, mws, out_dist, out_row, st);
}

int fx_fill_normal(void* x, int dtype, int64_t n, int64_t d, uint64_t seed, int64_t row_base,
                   int64_t cluster, void* stream) {
  if (!x || n < 0 || d < 1 || (dtype != FX_DTYPE_F32 && dtype != FX_DTYPE_F16)) {
    set_error("invalid fill arguments");
    return FX_EINVAL;
  }
  return launch_fill(x, dtype, n, d, seed, row_base, cluster,
                     reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
