// The planner (fx_plan.h): argument validation, which path a search takes,
// its workspace layout, and the exact-scan driver.  Host code only, no kernel.
#include "fx_plan.h"

namespace fx {

int validate(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric, bool qu8) {
  if (n < 1 || d < 1 || nq < 1) {
    set_error("invalid shape n=%lld d=%lld nq=%lld", (long long)n, (long long)d, (long long)nq);
    return FX_EINVAL;
  }
  if (d > (1 << 20)) {
    set_error("d=%lld too large", (long long)d);
    return FX_EUNSUPPORTED;
  }
  if (dtype != FX_DTYPE_F32 && dtype != FX_DTYPE_F16 && !(qu8 && dtype == FX_DTYPE_QU8)) {
    set_error("unsupported dtype %d", dtype);
    return FX_EINVAL;
  }
  if (metric < FX_METRIC_L2 || metric > FX_METRIC_COS) {
    set_error("unsupported metric %d", metric);
    return FX_EINVAL;
  }
  if (k < 1 || k > kLargeMaxK) {
    set_error("k=%lld outside [1, %lld]", (long long)k, (long long)kLargeMaxK);
    return FX_EUNSUPPORTED;
  }
  return FX_OK;
}

int validate_quant(const fx_corpus& c) {
  if (c.dtype == FX_DTYPE_QU8 && (c.zero_point < 0 || c.zero_point > 255 || !(c.scale > 0.f) ||
                                  c.scale == __builtin_inff())) {
    set_error("quint8 zero_point %d / scale %g out of range", c.zero_point, (double)c.scale);
    return FX_EINVAL;
  }
  return FX_OK;
}

// ---------------------------------------------------------------- batched --
//
// Batched queries (use_batched) run the MFMA filter (knn_filter.hip, kernels
// in filter/*.inc) in phases over growing row samples.  The filter brackets
// every (row, query) distance between a rigorous lower and upper bound and
// appends the pairs whose lower bound reaches the query's threshold to the
// query's candidate buffer of `cap` slots:
//   phase 0: a sample of <= cap rows, no threshold -> every (row, query) kept;
//   phase i: a sample ~cap/(4k) times larger (plan_phases; an int8 image:
//            plan_phases_i8's prefixes), threshold = the k-th upper bound of
//            phase i-1 (an upper bound of the global k-th distance: the k-th
//            of any row subset is), so it keeps ~cap/4 candidates per query;
//   last:    every row against the last threshold.
// The kept candidates are rescored exactly, in the single-query scan's own
// arithmetic (knn_exact.hip), before any result is taken from them, and the
// top k of the exact keys is the answer (run_merge; an int8 image: the
// selects of knn_select.hip, which also tighten the thresholds with exact
// distances between the phases).  The drivers are filter_phases and
// filter_phases_i8 (capi.hip).
// A query whose final candidates overflow `cap` is recomputed exactly by the
// single-query scan, gated on the device (fx_knn_reduce: no host sync).
static constexpr int64_t kListLen = 4096;  // candidate buffer viewed as lists

// A single query over an f32 corpus of at least this many bytes takes the
// batched path when an int8 filter image is supplied (the *_img8 entry
// points, option "single_query_image"): 10M x 768 1.41 vs 4.34 ms; the
// filter path's fixed cost (~0.25 ms of small launches) loses below ~2.4 GB
static constexpr int64_t kSingleImageMinBytes = (int64_t)4 << 30;
// Int8 images serve k <= option "i8_max_k" (1 024 = kMaxK, every k the
// filter plans).  Round 3's 64 K slots overflowed at k = 1 000 (6.25M x 1536
// fp16 IP, profiles/r03_f16_int8_image.log); with the 4x buffer (256 K slots
// at k = 1 000), the pruned selects (prune_kernel) and the shared LDS
// append segments, 60 single queries (normal, near, clustered corpus) kept
// 94-122 K candidates, none overflowed, 1.67 vs 2.84 ms for the exact scan,
// bit-identical (profiles/r06_k1000_sweep*.json); batches at k 300-1 000 are
// faster too (profiles/r06_kbatch_i8_max_k.jsonl).
static int64_t i8_max_k() { return option(kOptI8MaxK); }

// quint8 codes have no filter kernel of their own: a batch of them runs the
// int8-MFMA filter over an int8 image of the dequantised rows
// (image8_qu8_kernel) and is rescored from the codes in the quint8 scan's
// arithmetic (exact_distance16_qu8, whole 16-code slots: d % 16 == 0).  A
// single query stays on the scan (784 image bytes per 768 code bytes: nothing
// to gain), and so does a batch of less than option "qu8_batch_min_work"
// code bytes, nq * n * d: the filter's fixed cost (about 0.1 ms of small
// launches) loses against a few scans of a small shard.  The default is the
// smallest measured work from which the image path won at every point of
// tools/qu8_batch_sweep.py at or above it (profiles/qu8_batch_sweep.json: 16
// queries over 100 k x 128, 0.124 vs 0.130 ms; lost at 2 queries over
// 100 k x 768, 0.127 vs 0.073 ms; 10M x 768: 1.27 / 1.33 / 1.39 / 2.67 ms for
// 2 / 16 / 64 / 256 queries against 2.4 / 18.4 / 72.5 / 289 ms).
static bool use_batched_qu8(int64_t nq, int64_t d, bool aligned, int64_t n, bool img8, int64_t k) {
  const int64_t min_q = option(kOptBatchMinQ) >= 2 ? option(kOptBatchMinQ) : 2;
  if (!img8 || nq < min_q || !aligned || d % 16 != 0 || k > i8_max_k()) return false;
  return (double)nq * (double)n * (double)d >= (double)option(kOptQu8BatchMinWork);
}

static bool use_batched(int64_t nq, int dtype, int64_t d, bool aligned, int64_t n, bool img8,
                        int64_t k) {
  if (option(kOptBatched) == 0) return false;
  if (dtype == FX_DTYPE_QU8) return use_batched_qu8(nq, d, aligned, n, img8, k);
  // 2 queries: 6.5 ms vs 2 x 4.5 ms (10Mx768); "batch_min_queries" = 1 also
  // sends every single query through the filter
  int64_t min_q = option(kOptBatchMinQ) >= 1 ? option(kOptBatchMinQ) : 2;
  if (nq == 1 && img8 && k <= i8_max_k() && option(kOptSingleImage) != 0 && d % 8 == 0 &&
      n * d * (dtype == FX_DTYPE_F32 ? 4 : 2) >= kSingleImageMinBytes)
    min_q = 1;
  if (nq < min_q || !aligned) return false;
  // the rescoring repeats the scan's 16-B slot order: f32 rows need d % 4 == 0,
  // f16 rows d % 8 == 0
  if (dtype == FX_DTYPE_F32) return d % 4 == 0;
  return dtype == FX_DTYPE_F16 && d % 8 == 0;
}

// Nested row samples of the batched phases: phase i scans every stride_i-th
// tile of tr rows, each stride a multiple r of the next, the first at most
// cap rows, the last every tile.
static int plan_phases(BatchLayout* b, int64_t tr, int64_t r) {
  int64_t strides[16];
  int m = 0;
  strides[m++] = 1;
  while ((b->tiles + strides[m - 1] - 1) / strides[m - 1] * tr > b->cap) {
    if (m >= 15) {
      set_error("batched sampling plan too deep");
      return FX_EUNSUPPORTED;
    }
    strides[m] = strides[m - 1] * r;
    ++m;
  }
  b->nphases = m;
  for (int i = 0; i < m; ++i) {
    const int64_t st = strides[m - 1 - i];
    b->stride[i] = st;
    b->start[i] = 0;
    b->num[i] = (b->tiles + st - 1) / st;
  }
  return FX_OK;
}

// The int8 image's plan (filter_phases_i8).  The image stores its rows in a
// permuted order (image8_perm: a Weyl sequence over the corpus), so any
// PREFIX of its tiles is an equidistributed sample of the corpus: the
// samples are nested prefixes, read as contiguous runs.  The last sample F1
// holds ceil(tiles / r1) tiles (F2 reads the rest), the ones before it
// shrink by r2 (their appends stay far below cap: about r2 k upper bounds
// per query), the first holds at most cap rows.  10M x 768, r1 = 8, r2 = 16:
// 20, 306, 4 883 tiles, then F2's 34 180.
static int plan_phases_i8(BatchLayout* b, int64_t tr, int64_t r1, int64_t r2) {
  int64_t nums[16];
  int m = 0;
  nums[m++] = b->tiles;
  int64_t r = r1;
  while (nums[m - 1] * tr > b->cap) {
    if (m >= 15) {
      set_error("batched sampling plan too deep");
      return FX_EUNSUPPORTED;
    }
    nums[m] = (nums[m - 1] + r - 1) / r;
    ++m;
    r = r2;
  }
  b->nphases = m;
  for (int i = 0; i < m; ++i) {
    b->num[i] = nums[m - 1 - i];
    b->start[i] = 0;
    b->stride[i] = 1;
  }
  return FX_OK;
}

static int plan_batched(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, bool img8,
                        BatchLayout* b) {
  b->img8 = img8;
  const int64_t tr = filter_tile_rows(dtype);
  b->cap = 64 * k > 16384 ? 64 * k : 16384;
  // int8 images: 4x the buffer.  Their bounds keep whole clusters of a
  // clustered corpus against a generic query (10M x 768, x + 10 x0 per
  // 1 000 rows, 256 cosine queries: median 10 K, largest 33 K candidates);
  // every consumer reads only the count it was given (the selects stream
  // any count), so the larger buffer costs memory, not time
  if (b->img8) b->cap *= 4;
  if (option(kOptBatchCap) >= 16 * k) b->cap = option(kOptBatchCap);  // test: small buffers
  b->cap = (b->cap + kListLen - 1) / kListLen * kListLen;
  b->tiles = (n + tr - 1) / tr;
  // nested samples: phase i scans every stride_i-th tile, each stride a
  // multiple of the next, so every sample contains the previous one and has
  // at least k rows under the previous threshold; ~cap/4 appends per query.
  const int64_t rmax = b->cap / (4 * k);  // >= 16 for k <= 1024
  const int64_t v = option(kOptBatchRatio);  // test switch: denser samples (never sparser)
  int rc;
  if (b->img8) {
    // int8 image: the final pass's sample F1 takes every r1-th tile, the
    // samples before it grow by r2 (options "i8_sample_ratio", default 8, and
    // "i8_grow_ratio", default 16; the test switch: any ratio up to rmax)
    const int64_t o1 = option(kOptI8SampleRatio) >= 2 ? option(kOptI8SampleRatio) : 2;
    const int64_t o2 = option(kOptI8GrowRatio) >= 2 ? option(kOptI8GrowRatio) : 2;
    int64_t r1 = rmax < o1 ? rmax : o1;
    int64_t r2 = rmax < o2 ? rmax : o2;
    if (v >= 2) r1 = r2 = v < rmax ? v : rmax;
    rc = plan_phases_i8(b, tr, r1, r2);
  } else {
    rc = plan_phases(b, tr, v >= 2 && v < rmax ? v : rmax);
  }
  if (rc) return rc;
  rc = plan_merge(nq, b->cap / kListLen, kListLen, k, &b->merge);
  if (rc) return rc;
  size_t off = 0;
  b->off_qnorm = off;
  off += align256((size_t)nq * 4);
  b->off_thr = off;
  off += align256((size_t)nq * 8);
  b->off_count = off;
  off += align256((size_t)nq * 4 * kCountStride);
  b->off_cand = off;
  off += align256((size_t)nq * b->cap * 8);
  b->off_merge = off;
  off += align256(b->merge.ws_bytes);
  b->dq = filter_dq((int)d);
  b->nq_pad = (nq + filter_query_pad(nq) - 1) / filter_query_pad(nq) * filter_query_pad(nq);
  b->off_cand_ub = off;
  off += align256((size_t)nq * b->cap * 8);
  // fp16 query tiles, or int8 ones padded to 256 queries (int8 filter images)
  const size_t q16 = (size_t)b->nq_pad * b->dq * 2, q8 = (size_t)((nq + 255) / 256 * 256) * b->dq;
  b->off_qh = off;
  off += align256(q16 > q8 ? q16 : q8);
  b->off_qinfo = off;
  off += align256((size_t)nq * 16);
  // the rows of the k best candidates by upper bound (int8 images: exact thresholds)
  b->off_topr = off;
  off += align256((size_t)nq * k * 8);
  // quint8: the L2 scan's transformed queries (launch_qu8_query)
  b->off_qt = off;
  if (dtype == FX_DTYPE_QU8) off += align256((size_t)nq * d * 4);
  // the selects' prune scratch (int8 plans at large k): the slice count is
  // fixed here, once, and every select of this plan is launched with it
  b->prune_lists = b->img8 ? select_prune_lists(k, b->cap) : 0;
  b->off_prune = off;
  off += align256(select_prune_bytes(nq, k, b->prune_lists));
  b->total = off;
  return FX_OK;
}

// ----------------------------------------------------------- exact search --
static int plan_single(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric,
                       bool aligned, SearchLayout* s) {
  int rc = plan_scan(n, d, dtype, k, metric, aligned, &s->scan);
  if (rc) return rc;
  rc = plan_merge(nq, s->scan.nlists, k, k, &s->merge);
  if (rc) return rc;
  s->lists_bytes = align256((size_t)nq * s->scan.nlists * k * 8);
  s->total = s->lists_bytes + s->merge.ws_bytes;
  s->batched = false;
  return FX_OK;
}

static int plan_large_search(int64_t n, int64_t d, int dtype, int64_t nq, int metric,
                             bool aligned, SearchLayout* s) {
  int rc = plan_scan(n, d, dtype, 1, metric, aligned, &s->scan);
  if (rc) return rc;
  s->large = true;
  s->batched = false;
  s->lg = plan_large(n, nq);
  s->lists_bytes = 0;
  s->total = s->lg.total;
  return FX_OK;
}

int plan_exact(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric, bool aligned,
               SearchLayout* s) {
  return k > kMaxK ? plan_large_search(n, d, dtype, nq, metric, aligned, s)
                   : plan_single(n, d, dtype, nq, k, metric, aligned, s);
}

// The overflow fallback of the batched path runs the single-query plan over
// rounds of fq queries; its candidate lists take at most this many bytes.
static constexpr size_t kFallbackListBytes = (size_t)256 << 20;

// Its scan takes at most kFallbackBlocks blocks per query: the gated launch
// covers every query of a round, and an empty block still occupies its CU's
// LDS while it starts and exits (256 blocks x 256 queries of 10M x 768: 99 us
// with nothing to do; 16 per query: a few us, and an overflowing query still
// streams its rows from 16 CUs).
// Small batches spread the same total over more workgroups per query (4 096
// workgroups in all, at least 16 per query): a single query that overflows is
// rescanned at the full scan's width (256 workgroups, ~4.4 ms for 10M x 768)
// instead of by 16 CUs (~38 ms).
static constexpr int64_t kFallbackBlocks = 16;
static constexpr int64_t kFallbackTotalBlocks = 4096;

static int plan_fallback(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric,
                         bool aligned, SearchLayout* s, int64_t* fq) {
  int rc = plan_scan(n, d, dtype, k, metric, aligned, &s->scan);
  if (rc) return rc;
  const int64_t per_q = kFallbackTotalBlocks / (nq > 0 ? nq : 1);
  limit_scan_blocks(&s->scan, n, per_q > kFallbackBlocks ? per_q : kFallbackBlocks);
  const size_t per_query = (size_t)s->scan.nlists * k * 8;
  int64_t f = (int64_t)(kFallbackListBytes / (per_query > 0 ? per_query : 1));
  if (f > nq) f = nq;
  if (f > 65535) f = 65535;
  if (f < 1) f = 1;
  *fq = f;
  rc = plan_merge(f, s->scan.nlists, k, k, &s->merge);
  if (rc) return rc;
  s->lists_bytes = align256((size_t)f * s->scan.nlists * k * 8);
  s->total = s->lists_bytes + s->merge.ws_bytes;
  s->batched = false;
  return FX_OK;
}

int plan_search(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric, bool aligned,
                bool img8, SearchLayout* s, bool qmask) {
  if (k > kMaxK || !use_batched(nq, dtype, d, aligned, n, img8, k))
    return plan_exact(n, d, dtype, nq, k, metric, aligned, s);
  // per-query masks: only the int8 image's resident-slice kernel tests an
  // admission bit per pair; everything else scans exactly with each query's
  // own bitmap
  if (qmask && (!img8 || nq < 2 || k > i8_max_k() || d % 8 != 0 ||
                filter_qmask_kind(filter_dq((int)d), nq) == 0))
    return plan_exact(n, d, dtype, nq, k, metric, aligned, s);
  // the single-query plan over fb_queries queries serves overflowing queries
  int64_t fq = 1;
  int rc = plan_fallback(n, d, dtype, nq, k, metric, aligned, s, &fq);
  if (rc) return rc;
  const size_t single_total = s->total;
  rc = plan_batched(n, d, dtype, nq, k,
                    img8 && k <= i8_max_k() && d % 8 == 0, &s->batch);
  if (rc) return rc;
  s->batched = true;
  s->batch.qmask = qmask;
  s->fb_queries = fq;
  s->single_off = s->batch.total;
  s->total = s->batch.total + single_total;
  return FX_OK;
}

// ------------------------------------------------------------- exact scan --
ScanArgs scan_args(const ScanPlan& p, const fx_corpus& c, const int32_t* rows, int64_t nrows,
                   const RowMasks& mask, int64_t k, int mode) {
  ScanArgs a = {};
  a.X = c.data;
  a.n = rows != nullptr ? nrows : c.n;
  a.d = (int)c.d;
  a.row_base = c.row_base;
  a.mask = mask.mask;
  a.mask_qstride = mask.mask != nullptr ? (int)mask.qstride : 0;
  a.rows = rows;
  a.rows_per_block = p.rows_per_block;
  a.k = (int)k;
  a.cap = p.cap;
  a.qbytes = p.qbytes;
  a.mode = mode;
  a.qscale = c.dtype == FX_DTYPE_QU8 ? c.scale : 1.f;
  a.qshift = c.dtype == FX_DTYPE_QU8 ? (float)c.zero_point : 0.f;
  return a;
}

int launch_scan_queries(const ScanPlan& p, ScanArgs a, int64_t nq, hipStream_t st) {
  constexpr int64_t kGridQueries = 65535;  // gridDim.y
  const size_t lists = (size_t)(a.list_stride > 0 ? a.list_stride : p.nlists) * a.k;
  for (int64_t q0 = 0; q0 < nq; q0 += kGridQueries) {
    const int64_t qn = (nq - q0) < kGridQueries ? (nq - q0) : kGridQueries;
    int rc = launch_scan(p, a, qn, st);
    if (rc) return rc;
    a.q += (size_t)qn * a.d;
    if (a.mask != nullptr) a.mask += qn * (int64_t)a.mask_qstride;
    if (a.out_lists != nullptr) a.out_lists += (size_t)qn * lists;
    if (a.out_dist != nullptr) a.out_dist += (size_t)qn * a.n;
  }
  return FX_OK;
}

}  // namespace fx
