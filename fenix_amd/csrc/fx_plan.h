// Host-side plans of a search (knn_plan.hip): argument validation, the
// workspace layouts and the exact-scan driver the entry points of capi.hip
// and capi_ex.hip share.  A plan reads the process options once; whatever it
// decided travels in the layout, and no launcher re-derives it.
#pragma once

#include "fx_internal.h"

namespace fx {

constexpr int64_t kMaxK = 1024;  // fused path; larger k: knn_large.hip
constexpr int64_t kLargeMaxK = 0x7fffffffll;

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// shape, dtype (qu8: FX_DTYPE_QU8 too), metric, then k in [1, kLargeMaxK];
// an entry point without a k passes 1
int validate(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric, bool qu8);
// a quint8 descriptor's zero point in [0, 255] and scale positive and finite
// (other dtypes: nothing to check)
int validate_quant(const fx_corpus& c);

struct BatchLayout {
  int64_t cap = 0, tiles = 0, nq_pad = 0;
  int nphases = 0;
  bool filter = false;  // fp16-MFMA filter + exact rescoring (knn_filter.hip)
  bool img8 = false;    // planned for an int8 filter image (filter_phases_i8)
  int dq = 0;
  int prune_lists = 0;  // img8: k-lists of the selects' prune pass (select_prune_lists), 0 = none
  int64_t start[16], stride[16], num[16];
  MergePlan merge;
  size_t off_qnorm, off_thr, off_count, off_cand, off_merge, off_cand_ub, off_qh, off_qinfo,
      off_topr, off_qt, off_prune, total;
};

struct SearchLayout {
  ScanPlan scan;
  MergePlan merge;
  size_t lists_bytes, total;
  bool large = false;  // k > kMaxK: distance-mode scan + radix sort (knn_large.hip)
  LargeLayout lg;
  bool batched;
  BatchLayout batch;
  size_t single_off;   // batched: workspace of the overflow fallback
  int64_t fb_queries;  // batched: queries per fallback round (scan + merge over fb_queries)
};

// The exact scan + merge over n rows (plan_single, k <= kMaxK), or the
// distance-mode scan + radix sort (plan_large_search, larger k).
int plan_exact(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric, bool aligned,
               SearchLayout* s);
// fx_knn_search and its halves: the batched filter where it applies
// (use_batched), plan_exact otherwise.  img8: the call supplies an int8
// filter image (single queries may take the batched path); a scan and its
// reduce must plan with the same flag.
int plan_search(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric, bool aligned,
                bool img8, SearchLayout* s);

// the corpus of an entry point that takes it as plain arguments (f32 / f16)
inline fx_corpus corpus_of(const void* data, int dtype, int64_t n, int64_t d, int64_t row_base) {
  return fx_corpus{data, dtype, n, d, row_base, 1.f, 0};
}

// The exact scan's arguments from its plan and the corpus: n rows of the row
// list, or the corpus's own when rows is null.  Query, outputs, gate and list
// placement are the caller's.
ScanArgs scan_args(const ScanPlan& p, const fx_corpus& c, const int32_t* rows, int64_t nrows,
                   const uint32_t* mask, int64_t k, int mode);
// launch_scan over any number of queries: a grid holds at most 65 535 of
// them, so a.q, a.out_lists and a.out_dist (query 0's) advance per chunk
int launch_scan_queries(const ScanPlan& p, ScanArgs a, int64_t nq, hipStream_t st);

}  // namespace fx
