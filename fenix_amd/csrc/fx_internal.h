// Internal declarations shared by the kernel translation units and the C ABI.
#pragma once

#include "../../include/fenix_knn.h"
#include "fx_common.h"

namespace fx {

constexpr int kModeTopk = 0;
constexpr int kModeDist = 1;
// Per-query append counters of the batched kernels sit 128 B apart: every
// counter in its own cache line, so the L2 channels serialise fewer atomics.
constexpr int kCountStride = 32;
// largest k of the one-workgroup selects (knn_select.hip): their LDS holds a
// 16 384-entry chunk plus the k kept so far rounded up to a power of two, which
// fits the 160 KB of a CU up to 2 048; also the bound of option "i8_max_k"
constexpr int kSelectMaxK = 2048;

// Process-wide options (fx_set_option, include/fenix_knn.h); relaxed atomics
// (fx_runtime.hip).  One line per option: enumerator, name, default; the enum,
// the names fx_set_option accepts and the defaults all come from this list, in
// this order (_lib.OPTIONS repeats the names; tests/test_abi.py compares).
//   filter_image         filter image bits for f32 corpora (engine policy): 8, 16 or 0 (none)
//   batch_ub_test        sampling phases append by upper bound (0: by lower bound, test switch)
//   single_query_image   single queries over large f32 corpora through a supplied int8 image
//   i8_max_k             largest k an int8 filter image serves
//   img6                 int8 images: resident-query-slice kernel (1: <= 128 queries, 2: all, 0: off)
//   img8                 int8 images: queries-in-registers kernel for > 128 queries, d <= 768 (0: off)
//   i8_sample_ratio      int8 images: F1 holds every r1-th tile (filter_phases_i8)
//   i8_grow_ratio        int8 images: the samples before F1 shrink by r2 each
//   select_prune         int8 images: 1: selects at k >= 512 prune first; 2: any k; 0: never
//   scan_stream          plain f32 / f16 scans: 1: streaming kernel, 0: register tiles, -1: by class
//   filter_hold          1: the filter phases stop after their last filter pass, the bounds left
//                        in the workspace for fx_knn_filter_state (test switch; no reduce follows)
//   qu8_batch_min_work   quint8 batches go through an int8 image from nq * n * d code bytes on
//                        (use_batched: below it a few exact scans beat the filter's fixed cost)
//   qmask_batch_min_ratio  in hundredths: concurrent filtered searches run as one per-query-mask
//                        batch when one by one they would read at least this many times the
//                        batch's bytes (host policy: engine.qmask_batch_pays; 1.23: the smallest
//                        measured ratio from which the batch won, profiles/qmask_batch_sweep.json)
//   device_filter_min_rows  filters the predicate compiler accepts are evaluated on the device
//                        (fx_pred_eval) for tables of at least this many rows (host policy:
//                        io.index.call; 10 000: the smallest measured row count, from which the
//                        device path's median beat the host path's at every point,
//                        profiles/filter_pushdown.json)
#define FX_OPTIONS(FX_OPTION)                               \
  FX_OPTION(kOptBatched, "batched", 1)                      \
  FX_OPTION(kOptBatchMinQ, "batch_min_queries", 2)          \
  FX_OPTION(kOptBatchCap, "batch_cap", 0)                   \
  FX_OPTION(kOptBatchRatio, "batch_sample_ratio", 0)        \
  FX_OPTION(kOptForceFallback, "force_fallback", 0)         \
  FX_OPTION(kOptScanInterleave, "scan_interleave", -1)      \
  FX_OPTION(kOptQ8Dma, "q8_dma", 1)                         \
  FX_OPTION(kOptFilterImage, "filter_image", 8)             \
  FX_OPTION(kOptBatchUbTest, "batch_ub_test", 1)            \
  FX_OPTION(kOptSingleImage, "single_query_image", 1)       \
  FX_OPTION(kOptI8MaxK, "i8_max_k", 1024)                   \
  FX_OPTION(kOptImg6, "img6", 1)                            \
  FX_OPTION(kOptImg8, "img8", 1)                            \
  FX_OPTION(kOptI8SampleRatio, "i8_sample_ratio", 8)        \
  FX_OPTION(kOptI8GrowRatio, "i8_grow_ratio", 16)           \
  FX_OPTION(kOptSelectPrune, "select_prune", 1)             \
  FX_OPTION(kOptScanStream, "scan_stream", -1)             \
  FX_OPTION(kOptFilterHold, "filter_hold", 0)               \
  FX_OPTION(kOptQu8BatchMinWork, "qu8_batch_min_work", 204800000) \
  FX_OPTION(kOptQmaskBatchMinRatio, "qmask_batch_min_ratio", 123) \
  FX_OPTION(kOptDeviceFilterMinRows, "device_filter_min_rows", 10000)
enum Option : int {
#define FX_OPTION_ENUM(id, name, dflt) id,
  FX_OPTIONS(FX_OPTION_ENUM)
#undef FX_OPTION_ENUM
  kOptCount
};
int64_t option(Option o);
// fx_set_option / fx_get_option / fx_last_error (unknown name: FX_EINVAL)
int set_option(const char* name, int64_t value);
int get_option(const char* name, int64_t* out);
const char* last_error();

// Diagnostic builds for tools/ (make diag: -DFX_DIAG_BUILD) read a few
// variant and tuning switches from the environment; the product library
// compiles the rejected variants out and takes the defaults.
#ifdef FX_DIAG_BUILD
int diag_env(const char* name, int dflt);
#else
constexpr int diag_env(const char*, int dflt) { return dflt; }
#endif

struct ScanArgs {
  const void* X;          // [n][d] corpus shard
  int64_t n;
  int d;
  int64_t row_base;       // global row of local row 0
  const float* q;         // [nq][d]
  const uint32_t* mask;   // bitmap or null
  const int32_t* rows;    // [n] corpus rows to scan (n = list length) or null: rows 0..n-1
  int64_t rows_per_block;
  int k;
  int cap;                // per-wave candidate list capacity
  size_t qbytes;          // LDS bytes reserved for the query
  int mode;               // kModeTopk / kModeDist
  uint64_t* out_lists;    // topk: [nq][list_stride][k] composites (one list per block,
                          // block b at list list_base + b)
  int64_t list_stride;    // lists per query in out_lists (0: gridDim.x)
  int64_t list_base;      // this launch's first list (fx_knn_search_shards: the shard's)
  float* out_dist;        // dist: [nq][n]
  float qscale, qshift;   // FX_DTYPE_QU8: value = qscale * (code - qshift)
  // bit 0 clear: block b scans rows [b * rows_per_block, ...) in order; set:
  // block steps of 16U rows dealt round-robin over the grid.  Bit 1: no
  // software pipeline (one tile per wave in flight).  Set by launch_scan.
  int interleave;
  // Per-query masks: query qi reads the bitmap mask + qi * mask_qstride (words,
  // < 2^27 for 2^32 rows); 0: one bitmap shared by every query.  (In the
  // padding before the next pointer: no other field moves.)
  int mask_qstride;
  // Device-side gate (the batched path's overflow fallback): when non-null, a
  // workgroup of query qi returns at once unless gate[qi * kCountStride] >
  // gate_cap (gate_cap < 0: every query runs).
  const uint32_t* gate;
  int64_t gate_cap;
};

typedef void (*ScanKernelFn)(ScanArgs);

struct ScanPlan {
  ScanKernelFn fn;  // register tiles: serves every scan
  int W, L, U, cap;
  size_t qbytes, smem;
  int64_t blocks, rows_per_block, nlists;
  int interleave;  // ScanArgs::interleave
  // Plain scans (no mask, no row list) where a ring kernel applies and is not
  // switched off, else null: f32 / f16 rows of exactly 16 L slots streamed
  // through a register ring (smem_plain == smem), quint8 rows staged by
  // LDS-DMA (smem_plain: smem plus the ring).  Same grid and rows_per_block
  // as fn (the DMA ring's U divides it).  plain_name: the kernel for
  // check_launch.
  ScanKernelFn fn_plain;
  size_t smem_plain;
  const char* plain_name;
};

int plan_scan(int64_t n, int64_t d, int dtype, int64_t k, int metric, bool aligned, ScanPlan* p);
// at most max_blocks blocks per query (rows_per_block, blocks, nlists recomputed)
void limit_scan_blocks(ScanPlan* p, int64_t n, int64_t max_blocks);
int launch_scan(const ScanPlan& p, const ScanArgs& a, int64_t nq, hipStream_t stream);

// Merge of candidate lists: [nq][nlists][kin] composites -> top-k.
struct MergePlan {
  int levels;
  int64_t group[16];      // lists per block at each level
  int64_t lists[17];      // list count entering each level (lists[levels] == 1)
  int64_t klen[17];       // list length entering each level
  size_t ws_bytes;        // ping-pong scratch for intermediate levels
};
int plan_merge(int64_t nq, int64_t nlists, int64_t kin, int64_t k, MergePlan* p);
// out_dist/out_row may be null; out_kth (optional) receives each query's k-th
// smallest composite (kEmpty if fewer than k candidates).
// gate/gate_cap: as ScanArgs::gate, per query of the merge.
// count (optional): appended lists, query q's entries are its first
// count[q * kCountStride] slots (capped at nlists * kin; the rest unread).
// zero_count: reset each query's count once read (only a one-level plan,
// where one workgroup per query reads it; ignored otherwise).
int run_merge(const MergePlan& p, const uint64_t* in, int64_t nq, int64_t k, void* ws,
              float* out_dist, int64_t* out_row, hipStream_t stream,
              uint64_t* out_kth = nullptr, const uint32_t* gate = nullptr,
              int64_t gate_cap = 0, uint32_t* count = nullptr, bool zero_count = false);

// FX_DTYPE_QU8 rows: value = scale * (code - shift), as ScanArgs::qscale / qshift
// (f32 / f16 rows: unused)
struct Quant {
  float scale = 1.f, shift = 0.f;
};

// gridDim.y holds at most 65 535 queries: f(q0, qn) launches queries
// [q0, q0 + qn) of a batch, chunk by chunk, until one fails
template <typename F>
int for_query_chunks(int64_t nq, F&& f) {
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {
    if (int rc = f(q0, (nq - q0) < 65535 ? (nq - q0) : 65535)) return rc;
  }
  return FX_OK;
}

// Where the exact distances of a batched search come from: the corpus shard
// and the queries as the single-query scan would read them.  The phase
// drivers (capi.hip) build it once; the rescoring launchers (knn_exact.hip)
// and the exact-threshold select (knn_select.hip) take it.
struct ExactSource {
  const void* X;       // [n][d] rows of dtype, whole 16-B slots (quint8: d % 16 == 0)
  int dtype;
  int64_t n;
  int d;
  int64_t row_base;    // global row of local row 0
  const float* Q;      // [nq][d] the queries as the scan keeps them in LDS: for quint8
                       // L2 launch_qu8_query's q', the queries themselves otherwise
  const float* qnorm;  // [nq] max(|q|, 1e-12) as the scan computes it (read for cosine only)
  int metric;
  Quant z;             // quint8: the corpus's scale and zero point
  // the same source for the queries from q0 on
  ExactSource from_query(int64_t q0) const {
    ExactSource s = *this;
    s.Q += q0 * d;
    if (s.qnorm != nullptr) s.qnorm += q0;
    return s;
  }
};

// out [nq][d] = shift + q / scale: the quint8 L2 scan's query (scan_begin's expression)
int launch_qu8_query(const float* Q, int64_t nq, int d, Quant z, float* out, hipStream_t stream);
// out [nq] = max(|q|, 1e-12) (cosine)
int launch_qnorm(const float* Q, int64_t nq, int d, float* out, hipStream_t stream);
// Replace each candidate's key by its exact distance (the single-query scan's
// summation order: bit-identical).  thr (optional): candidates whose key is
// above the query's thr key are dropped (kEmpty) without being read.
int launch_rescore(const ExactSource& src, int64_t nq, const uint32_t* count, uint64_t* cand,
                   int cap, const uint64_t* thr, hipStream_t stream);
// thr[q] = min(thr[q], the largest exact composite of the query's k rows
// [nq][k] (global, -1 = missing: the query keeps its threshold)); rows is
// overwritten
int launch_exact_kth(const ExactSource& src, int64_t nq, int k, int64_t* rows, uint64_t* thr,
                     hipStream_t stream);

// The selects (knn_select.hip, where each kernel is described): one workgroup
// per query over its first count[q] entries of keys [nq][cap], any cap.
//
// A plan that prunes first keeps the k smallest of every LDS-sized slice in
// parallel (prune_kernel).  The plan fixes the slice count once
// (BatchLayout::prune_lists = select_prune_lists(k, cap), 0 = none) and
// reserves select_prune_bytes of scratch; the launchers take both, together.
struct PruneScratch {
  uint64_t* lists = nullptr;  // [nq][count][k]
  int count = 0;              // k-lists per query
  bool on() const { return lists != nullptr && count > 0; }
  uint64_t* from_query(int64_t q0, int k) const {
    return on() ? lists + q0 * (int64_t)count * k : nullptr;
  }
};
int select_prune_lists(int64_t k, int64_t cap);
size_t select_prune_bytes(int64_t nq, int64_t k, int prune_lists);
// launch_overflow_gate(cand, count, thr, nq, cap, num, den) to follow a new
// threshold; cand null: no gate
struct OverflowGate {
  const uint64_t* cand = nullptr;
  int64_t num = 0, den = 1;
};
// thr[q] = min(thr[q], the largest exact composite of the k smallest keys'
// rows): exact_threshold_kernel, or (a pruning plan with topr [nq][k]) the
// select writes the rows and launch_exact_kth rescores them; then the gate.
int launch_exact_threshold(const ExactSource& src, int64_t nq, const uint64_t* keys, int64_t cap,
                           uint32_t* count, bool zero_count, int k, uint64_t* thr,
                           PruneScratch prune, int64_t* topr, OverflowGate gate,
                           hipStream_t stream);
// thr[q] = min(thr[q], the k-th smallest of the query's first count[q] keys)
// when it has at least k
int launch_sample_threshold(const uint64_t* keys, int64_t nq, int64_t cap, uint32_t* count,
                            bool zero_count, int k, uint64_t* thr, PruneScratch prune,
                            hipStream_t stream);
// the final top-k of each query's exact composites, sorted and decoded; a
// query whose count exceeds alt_gate: of its alt_m entries of alt [nq][alt_m]
int launch_final_select(const uint64_t* keys, int64_t nq, int64_t cap, const uint32_t* count,
                        int k, float* out_dist, int64_t* out_row, const uint64_t* alt,
                        int64_t alt_m, int64_t alt_gate, PruneScratch prune, hipStream_t stream);

// Batched filter on the fp16 matrix cores (knn_filter.hip: the entry points
// and the fp16 error bound; the kernels: filter/*.inc, compiled into the
// variants knn_filter_q256.hip, _h256, _q128, _q64, _q64i): appends every
// (row, query) whose rigorous lower bound reaches the query's threshold.
struct FilterArgs {
  const void* X;          // [n][d] corpus shard (f32 or f16)
  int dtype;              // FX_DTYPE_F32 / FX_DTYPE_F16
  int64_t n;
  int d;
  int64_t row_base;
  const uint16_t* Qh;     // fp16 queries scaled by a power of two, in blocks of 32
                          // components: (q, k) at ((k / 32) * qstride + q) * 32 + k % 32
  int dq;                 // components per query, padded (a multiple of 64)
  int64_t qstride;        // queries per block row (nq_pad)
  const float* qinfo;     // [nq][4] {1/scale, norm term, A, B}
  int64_t nq;
  const uint32_t* mask;
  int64_t tile_start, tile_stride, num_tiles;  // which 256-row tiles to scan
  const uint64_t* thr;    // [nq] append when order_key(lb) <= thr >> 32
  uint32_t* count;        // [nq * kCountStride] appends (may exceed cap: overflow)
  uint64_t* cand;         // [nq][cap] ub composites (cand_ub null) or lb composites
  uint64_t* cand_ub;      // [nq][cap] ub composites, or null (sampling phases)
  int cap;
  const float* rowinfo;   // [n] row sums of squares of the f32 rows when X is their fp16
                          // filter image (dtype F16), NaN = forced; null otherwise;
                          // img8: [n][kI8RowInfo] (launch_image8)
  int img8;               // X is the int8 filter image (launch_image8), Qh/qinfo from
                          // launch_qprep8
  int all_pass;           // no query has a threshold yet (thr all empty): img8 appends
                          // every live pair without the test
  int skip_full;          // a workgroup whose queries all hold count > cap returns at once
  uint64_t perm_a;        // img8: image row i holds corpus row (perm_a * i) % n (image8_perm)
  int ub_test;            // sampling phase after the first: append when the UPPER bound
                          // reaches the threshold (only the k-th upper bound is needed)
  int diag;               // FX_FILTER_DIAG (diagnostic builds only): 1 no appends, 2 no epilogue,
                          // 4 no MFMA, 8 no query loads, 16 no LDS stores,
                          // 32 no append atomics, 64 no append stores
  const uint32_t* qmask;  // per-query row masks (fx_qmask_pack: [n][qmask_words], bit q & 31
                          // of word q >> 5 of CORPUS row r: query q admits r) or null;
                          // int8 images through filter_img6_kernel<., true> only
  int64_t qmask_words;    // words per row of qmask (fx_qmask_words(nq))
};
int launch_filter(const FilterArgs& a, int metric, hipStream_t stream);
// which resident-slice build serves a batch with per-query row masks
// (FilterArgs::qmask): 64 (q64i: nq <= 64, or slices of 64 where a q128 slice
// does not fit the row length), 128 (q128 slices), 0: neither fits
int filter_qmask_kind(int dq, int64_t nq);
// fx_qmask_pack (knn_qmask.hip): nq row bitmaps -> the bit matrix [n][qw]
int64_t qmask_words(int64_t nq);
int launch_qmask_pack(const uint32_t* masks, int64_t mask_stride, int64_t nq, int64_t n,
                      uint32_t* out, hipStream_t stream);
// the LDS-DMA ring variant (filter/ring.inc ring_kernel) with FX_FILTER_RING=1
// (the register-staged kernel, filter/staged.inc, otherwise)
bool filter_ring();
// filter images in MFMA fragment order (filter/img2.inc filter_img2_kernel);
// FX_IMAGE_TILED=0: row-major
bool image_tiled();
// int8 filter images (built in knn_filter.hip): per row kI8RowInfo floats {w, 1/s,
// N/s, n2/s, 0...} (launch_image8), per query kI8QInfo floats {s_q, R', n_q^2,
// |q|, 0...} (launch_qprep8); kI8Kappa bounds P/R' (the two query error terms,
// see filter/tiled.inc "int8 filter image")
constexpr int kI8RowInfo = 4;
constexpr int kI8QInfo = 4;
constexpr float kI8Kappa = 128.f;
// (FX_DTYPE_QU8: codes with z's scale and zero point, d % 16 == 0; same image
// layout and row terms for the rows scale * (code - zero point))
int launch_image8(const void* X, int dtype, int64_t n, int d, void* img, float* rowinfo,
                  hipStream_t stream, Quant z = Quant());
// The int8 image stores its rows in the order of an affine permutation of the
// corpus: image row i holds corpus row (a * i) % n, a ~ 0.618 n coprime with n
// (a Weyl sequence).  The filter's nested samples take every r-th tile of the
// IMAGE, so they are equidistributed over the corpus whatever its order: a
// corpus stored in clusters (the reference test's x + 10 x0 per 1 000-row
// batch) or sorted by any key no longer hides its nearest rows from the
// samples.  1 for n <= 2.
uint64_t image8_perm(int64_t n);
__device__ __forceinline__ uint32_t perm_row(uint64_t a, int64_t n, int64_t i) {
  return (uint32_t)((a * (uint64_t)i) % (uint64_t)n);
}
// Final-pass overflow prediction (img8): per query, the appended candidates of
// the last sample (count, cand: lb composites) that pass the new threshold thr,
// scaled by num / den (the remaining tiles over the sample's), plus count: a
// query predicted to exceed cap gets count = cap + 1 (the final pass skips it
// and the exact scan recomputes it, fx_knn_reduce's gated fallback).
// knn_select.hip, beside the exact-threshold select that fuses it.
int launch_overflow_gate(const uint64_t* cand, uint32_t* count, const uint64_t* thr, int64_t nq,
                         int cap, int64_t num, int64_t den, hipStream_t stream);
// (thr, count: when given, each query's threshold is set empty and its append
// count zeroed in the same launch)
// (qe, quint8 L2: Q holds launch_qu8_query's q', and the query the filter
// bounds is the scan's effective one, qe->scale * (q' - qe->shift))
int launch_qprep8(const float* Q, int64_t nq, int64_t nq_pad, int d, int dq, int metric,
                  int8_t* Qb, float* qinfo, hipStream_t stream, uint64_t* thr = nullptr,
                  uint32_t* count = nullptr, const Quant* qe = nullptr);
int launch_qprep(const float* Q, int64_t nq, int64_t nq_pad, int d, int dq, int metric,
                 uint16_t* Qh, float* qinfo, hipStream_t stream);
// rows per tile of every filter kernel (FilterArgs::tile_start ...)
constexpr int kFilterTileRows = 256;
int filter_tile_rows(int dtype);
// fp16 filter image + row sums of squares of an f32 corpus (knn_filter.hip)
int launch_image(const float* X, int64_t n, int d, void* img, float* rowinfo, hipStream_t stream);
int filter_query_pad(int64_t nq);
int filter_dq(int d);
int launch_encode(const float* dist, const int64_t* row, int64_t count, uint64_t* out,
                  hipStream_t stream);
int launch_fill(void* x, int dtype, int64_t n, int64_t d, uint64_t seed, int64_t row_base,
                int64_t cluster, hipStream_t stream);

// error / device helpers (fx_runtime.hip)
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int check_launch(const char* what);
int device_cus(int* out);
// false on a host with no HIP device (plans are then answered for the target, plan_scan)
bool device_present();
int kernel_occupancy(const void* fn, int block, size_t smem, int* out);
// raise the dynamic-LDS limit of fn to 160 KB on the current device (once per device)
int allow_lds(const void* fn);

// k above the fused path (knn_large.hip): all distances + radix sort.
struct LargeLayout {
  size_t off_dist, off_keys, off_sorted, off_temp, temp_bytes, total;
};
LargeLayout plan_large(int64_t n, int64_t nq);
// distances (distance-mode scan with plan p) + composites into ws
int large_scan(const ScanPlan& p, ScanArgs a, int64_t nq, const LargeLayout& l, char* ws,
               hipStream_t st);
int large_reduce(int64_t n, int64_t nq, int64_t k, const LargeLayout& l, char* ws,
                 float* out_dist, int64_t* out_row, hipStream_t st);

}  // namespace fx
