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
  bool img8 = false;    // planned for an int8 filter image (filter_phases_i8)
  bool qmask = false;   // planned for per-query row masks (filter_img6_kernel<., true>)
  int dq = 0;
  int prune_lists = 0;  // img8: k-lists of the selects' prune pass (select_prune_lists), 0 = none
  int64_t start[16], stride[16], num[16];
  MergePlan merge;
  size_t off_qnorm, off_thr, off_count, off_cand, off_merge, off_cand_ub, off_qh, off_qinfo,
      off_topr, off_qt, off_prune, total;
};

// The batched workspace as typed pointers: what a layout's offsets mean,
// carved once for the phase drivers, the reduce and the test read-backs.
struct BatchWorkspace {
  float* qnorm;         // [nq] cosine: max(|q|, 1e-12)
  uint64_t* thr;        // [nq] thresholds
  uint32_t* count;      // [nq * kCountStride] appends per query
  uint64_t* cand;       // [nq][cap] candidates (lower bounds, then exact composites)
  char* merge;          // run_merge's scratch (fp16 filter plans)
  uint64_t* cand_ub;    // [nq][cap] upper bounds of the final passes
  void* qh;             // the filter's query tiles (fp16 or int8)
  float* qinfo;         // the filter's per-query terms
  int64_t* topr;        // [nq][k] rows of the k best upper bounds
  float* qt;            // quint8 L2: the scan's transformed queries
  PruneScratch prune;   // the selects' prune pass (none: off)
  BatchWorkspace(const BatchLayout& b, void* ws) {
    char* w = reinterpret_cast<char*>(ws);
    qnorm = reinterpret_cast<float*>(w + b.off_qnorm);
    thr = reinterpret_cast<uint64_t*>(w + b.off_thr);
    count = reinterpret_cast<uint32_t*>(w + b.off_count);
    cand = reinterpret_cast<uint64_t*>(w + b.off_cand);
    merge = w + b.off_merge;
    cand_ub = reinterpret_cast<uint64_t*>(w + b.off_cand_ub);
    qh = w + b.off_qh;
    qinfo = reinterpret_cast<float*>(w + b.off_qinfo);
    topr = reinterpret_cast<int64_t*>(w + b.off_topr);
    qt = reinterpret_cast<float*>(w + b.off_qt);
    if (b.prune_lists > 0)
      prune = PruneScratch{reinterpret_cast<uint64_t*>(w + b.off_prune), b.prune_lists};
  }
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
// qmask: the search brings per-query row masks (fx_knn_search_qmask_ex): an
// int8-image plan whose filter passes run the resident-slice kernel's QMASK
// build, or, where that does not apply (no image, k above "i8_max_k", rows not
// of whole 16-B image pieces, a single query, a row length neither slice
// build fits: filter_qmask_kind), the exact plan, whose scans read each
// query's own bitmap.
int plan_search(int64_t n, int64_t d, int dtype, int64_t nq, int64_t k, int metric, bool aligned,
                bool img8, SearchLayout* s, bool qmask = false);

// The row masks of a search: one bitmap shared by every query (or none), or
// per-query bitmaps mask + q * qstride together with their packed bit matrix
// (fx_qmask_pack) for the filter.
struct RowMasks {
  const uint32_t* mask = nullptr;
  int64_t qstride = 0;              // words between queries' bitmaps; 0: one shared bitmap
  const uint32_t* qmask = nullptr;  // [n][qwords], per-query masks only
  int64_t qwords = 0;
  RowMasks() = default;
  RowMasks(const uint32_t* shared) : mask(shared) {}
  RowMasks from_query(int64_t q0) const {
    RowMasks m = *this;
    if (m.mask != nullptr) m.mask += q0 * qstride;
    return m;
  }
};

// the corpus of an entry point that takes it as plain arguments (f32 / f16)
inline fx_corpus corpus_of(const void* data, int dtype, int64_t n, int64_t d, int64_t row_base) {
  return fx_corpus{data, dtype, n, d, row_base, 1.f, 0};
}

// The exact scan's arguments from its plan and the corpus: n rows of the row
// list, or the corpus's own when rows is null.  Query, outputs, gate and list
// placement are the caller's.
ScanArgs scan_args(const ScanPlan& p, const fx_corpus& c, const int32_t* rows, int64_t nrows,
                   const RowMasks& mask, int64_t k, int mode);
// launch_scan over any number of queries: a grid holds at most 65 535 of
// them, so a.q, a.out_lists, a.out_dist and per-query masks (query 0's)
// advance per chunk
int launch_scan_queries(const ScanPlan& p, ScanArgs a, int64_t nq, hipStream_t st);

}  // namespace fx
