// The exact-scan entry points: a corpus descriptor (include/fenix_knn.h
// fx_corpus: every dtype including FX_DTYPE_QU8, quint8 codes dequantised in
// the scan's registers, ex/arrow/quint8/quint8.py:81-84; optional row list
// and mask), its plain-argument forms fx_knn_search_rows / fx_knn_distances,
// and several shards under one merge.  Same plans and kernels as fx_knn_search
// (knn_plan.hip plan_exact).  Nothing here runs the batched filter: a batch
// over quint8 codes takes it through the descriptor forms of the int8-image
// entry points (capi.hip fx_knn_search_img8_ex), which fall back to these
// plans when the gate says no.
#include <vector>

#include "fx_plan.h"

namespace fx {
namespace {

bool rows_fit(int64_t row_base, int64_t n) {
  if (row_base >= 0 && n >= 0 && row_base + n < 0xffffffffll && n <= 0x7fffffffll) return true;
  set_error("global rows [%lld, %lld) exceed the 32-bit row space", (long long)row_base,
            (long long)(row_base + n));
  return false;
}

int check_corpus(const fx_corpus* c, int64_t nq, int64_t k, int metric) {
  if (c == nullptr || c->data == nullptr) {
    set_error("null corpus");
    return FX_EINVAL;
  }
  int rc = validate(c->n, c->d, c->dtype, nq, k, metric, true);
  if (rc) return rc;
  rc = validate_quant(*c);
  if (rc) return rc;
  return rows_fit(c->row_base, c->n) ? FX_OK : FX_EUNSUPPORTED;
}

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// Exact top-k over the corpus's rows, or over a row list of it (checked
// arguments): plan, scan, then the merge (k <= kMaxK) or the radix sort
int exact_search(const fx_corpus& c, const int32_t* rows, int64_t nrows, const float* queries,
                 int64_t nq, int metric, int64_t k, const uint32_t* mask, void* ws,
                 size_t ws_bytes, float* out_dist, int64_t* out_row, void* stream) {
  const int64_t n = rows != nullptr ? nrows : c.n;
  SearchLayout s;
  int rc = plan_exact(n, c.d, c.dtype, nq, k, metric, aligned16(c.data), &s);
  if (rc) return rc;
  if (ws_bytes < s.total) {
    set_error("workspace too small: %zu < %zu", ws_bytes, s.total);
    return FX_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* w = reinterpret_cast<char*>(ws);
  ScanArgs a = scan_args(s.scan, c, rows, nrows, mask, s.large ? 1 : k,
                         s.large ? kModeDist : kModeTopk);
  a.q = queries;
  if (s.large) {
    rc = large_scan(s.scan, a, nq, s.lg, w, st);
    if (rc) return rc;
    return large_reduce(n, nq, k, s.lg, w, out_dist, out_row, st);
  }
  a.out_lists = reinterpret_cast<uint64_t*>(ws);
  rc = launch_scan_queries(s.scan, a, nq, st);
  if (rc) return rc;
  return run_merge(s.merge, a.out_lists, nq, k, w + s.lists_bytes, out_dist, out_row, st);
}

// Every distance [nq][c.n] (checked arguments)
int exact_distances(const fx_corpus& c, const float* queries, int64_t nq, int metric,
                    const uint32_t* mask, float* out, void* stream) {
  ScanPlan p;
  int rc = plan_scan(c.n, c.d, c.dtype, 1, metric, aligned16(c.data), &p);
  if (rc) return rc;
  ScanArgs a = scan_args(p, c, nullptr, 0, mask, 1, kModeDist);
  a.row_base = 0;
  a.q = queries;
  a.out_dist = out;
  return launch_scan_queries(p, a, nq, reinterpret_cast<hipStream_t>(stream));
}

// fx_knn_search_shards: every shard's scan plan, and where its lists start
// in the one list buffer [nq][lists][k] the merge reads
constexpr int kMaxShards = 4096;

struct ShardsPlan {
  std::vector<ScanPlan> scan;
  std::vector<int64_t> base;
  int64_t lists = 0;
  MergePlan merge;
  size_t lists_bytes = 0, total = 0;
};

int check_shards(const fx_corpus* s, int ns, int64_t nq, int64_t k, int metric) {
  if (s == nullptr || ns < 1 || ns > kMaxShards) {
    set_error("fx_knn_search_shards: %d shards (1 .. %d)", ns, kMaxShards);
    return FX_EINVAL;
  }
  if (k < 1 || k > kMaxK) {
    set_error("fx_knn_search_shards: k=%lld outside [1, %lld]", (long long)k, (long long)kMaxK);
    return FX_EUNSUPPORTED;
  }
  for (int i = 0; i < ns; ++i) {
    int rc = check_corpus(&s[i], nq, k, metric);
    if (rc) return rc;
    if (s[i].d != s[0].d || s[i].dtype != s[0].dtype) {
      set_error("fx_knn_search_shards: shard %d has d=%lld dtype %d, shard 0 d=%lld dtype %d", i,
                (long long)s[i].d, s[i].dtype, (long long)s[0].d, s[0].dtype);
      return FX_EINVAL;
    }
  }
  return FX_OK;
}

int plan_shards(const fx_corpus* s, int ns, int64_t nq, int64_t k, int metric, ShardsPlan* p) {
  p->scan.resize(ns);
  p->base.resize(ns);
  p->lists = 0;
  for (int i = 0; i < ns; ++i) {
    int rc = plan_scan(s[i].n, s[i].d, s[i].dtype, k, metric, aligned16(s[i].data), &p->scan[i]);
    if (rc) return rc;
    p->base[i] = p->lists;
    p->lists += p->scan[i].nlists;
  }
  int rc = plan_merge(nq, p->lists, k, k, &p->merge);
  if (rc) return rc;
  p->lists_bytes = align256((size_t)nq * p->lists * k * 8);
  p->total = p->lists_bytes + p->merge.ws_bytes;
  return FX_OK;
}

}  // namespace
}  // namespace fx

using namespace fx;

extern "C" {

int fx_knn_search_rows_workspace_bytes(int64_t nrows, int64_t d, int dtype, int64_t nq,
                                       int64_t k, size_t* out_bytes) {
  if (!out_bytes) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  int rc = validate(nrows, d, dtype, nq, k, FX_METRIC_L2, false);
  if (rc) return rc;
  SearchLayout s;
  rc = plan_exact(nrows, d, dtype, nq, k, FX_METRIC_L2, true, &s);
  if (rc) return rc;
  *out_bytes = s.total;
  return FX_OK;
}

int fx_knn_search_rows(const void* corpus, int dtype, int64_t n, int64_t d, int64_t row_base,
                       const int32_t* rows, int64_t nrows, const float* queries, int64_t nq,
                       int metric, int64_t k, void* ws, size_t ws_bytes, float* out_dist,
                       int64_t* out_row, void* stream) {
  int rc = validate(nrows, d, dtype, nq, k, metric, false);
  if (rc) return rc;
  if (!corpus || !ws || !queries || !out_dist || !out_row || !rows) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if (!rows_fit(row_base, n)) return FX_EUNSUPPORTED;
  return exact_search(corpus_of(corpus, dtype, n, d, row_base), rows, nrows, queries, nq, metric,
                      k, nullptr, ws, ws_bytes, out_dist, out_row, stream);
}

int fx_knn_distances(const void* corpus, int dtype, int64_t n, int64_t d,
                     const float* queries, int64_t nq, int metric, const uint32_t* mask,
                     float* out, void* stream) {
  int rc = validate(n, d, dtype, nq, 1, metric, false);
  if (rc) return rc;
  if (!corpus || !queries || !out) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  return exact_distances(corpus_of(corpus, dtype, n, d, 0), queries, nq, metric, mask, out,
                         stream);
}

int fx_knn_search_ex_workspace_bytes(const fx_corpus* c, int64_t nrows, int64_t nq, int64_t k,
                                     size_t* out_bytes) {
  int rc = check_corpus(c, nq, k, FX_METRIC_L2);
  if (rc) return rc;
  if (out_bytes == nullptr) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  const int64_t rows = nrows >= 0 ? nrows : c->n;
  if (rows < 1) {
    set_error("empty row list");
    return FX_EINVAL;
  }
  SearchLayout s;
  rc = plan_exact(rows, c->d, c->dtype, nq, k, FX_METRIC_L2, aligned16(c->data), &s);
  if (rc) return rc;
  *out_bytes = s.total;
  return FX_OK;
}

int fx_knn_search_ex(const fx_corpus* c, const int32_t* rows, int64_t nrows,
                     const float* queries, int64_t nq, int metric, int64_t k,
                     const uint32_t* mask, void* ws, size_t ws_bytes, float* out_dist,
                     int64_t* out_row, void* stream) {
  int rc = check_corpus(c, nq, k, metric);
  if (rc) return rc;
  if (!queries || !ws || !out_dist || !out_row) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  if (rows != nullptr && nrows < 1) {
    set_error("empty row list");
    return FX_EINVAL;
  }
  return exact_search(*c, rows, nrows, queries, nq, metric, k, mask, ws, ws_bytes, out_dist,
                      out_row, stream);
}

int fx_knn_distances_ex(const fx_corpus* c, const float* queries, int64_t nq, int metric,
                        const uint32_t* mask, float* out, void* stream) {
  int rc = check_corpus(c, nq, 1, metric);
  if (rc) return rc;
  if (!queries || !out) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  return exact_distances(*c, queries, nq, metric, mask, out, stream);
}

int fx_knn_search_shards_workspace_bytes(const fx_corpus* shards, int nshards, int64_t nq,
                                         int64_t k, size_t* out_bytes) {
  if (out_bytes == nullptr) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  int rc = check_shards(shards, nshards, nq, k, FX_METRIC_L2);
  if (rc) return rc;
  size_t best = 0;
  for (int metric = FX_METRIC_L2; metric <= FX_METRIC_COS; ++metric) {  // (plans are per metric)
    ShardsPlan p;
    rc = plan_shards(shards, nshards, nq, k, metric, &p);
    if (rc) return rc;
    if (p.total > best) best = p.total;
  }
  *out_bytes = best;
  return FX_OK;
}

int fx_knn_search_shards(const fx_corpus* shards, int nshards, const float* queries, int64_t nq,
                         int metric, int64_t k, const uint32_t* const* masks, void* ws,
                         size_t ws_bytes, float* out_dist, int64_t* out_row, void* stream) {
  int rc = check_shards(shards, nshards, nq, k, metric);
  if (rc) return rc;
  if (!queries || !ws || !out_dist || !out_row) {
    set_error("null pointer argument");
    return FX_EINVAL;
  }
  ShardsPlan p;
  rc = plan_shards(shards, nshards, nq, k, metric, &p);
  if (rc) return rc;
  if (ws_bytes < p.total) {
    set_error("workspace too small: %zu < %zu", ws_bytes, p.total);
    return FX_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint64_t* lists = reinterpret_cast<uint64_t*>(ws);
  for (int i = 0; i < nshards; ++i) {
    ScanArgs a = scan_args(p.scan[i], shards[i], nullptr, 0, masks != nullptr ? masks[i] : nullptr,
                           k, kModeTopk);
    a.q = queries;
    a.out_lists = lists;
    a.list_stride = p.lists;
    a.list_base = p.base[i];
    rc = launch_scan_queries(p.scan[i], a, nq, st);
    if (rc) return rc;
  }
  return run_merge(p.merge, lists, nq, k, reinterpret_cast<char*>(ws) + p.lists_bytes, out_dist,
                   out_row, st);
}

}  // extern "C"
