// Batched-query candidate filter on the fp16 matrix cores.
//
// configs[2] (10M x 768 f32 cosine, 256 queries) is a dense GEMM S = X . Q^T
// (reference: 256 separate per-chunk UDF searches, src/fenix/io/index/
// index.py:137-162 -> src/fenix/io/coder/coder.py:42-48).  On fp32 MFMA it is
// compute-bound (3.93 TFLOP at 157 TF/s = 25 ms).  This kernel evaluates the
// GEMM on the fp16 matrix cores (16x the rate), where one pass over the f32
// corpus is HBM-bound again, and uses each product only as a FILTER: with a
// rigorous bound e on |fp16 estimate - the single-query scan's f32 distance|
// every (row, query) gets an interval [lb, ub] that contains the distance the
// scan computes.  Rows are kept when lb can reach the query's threshold, and
// every kept candidate is rescored exactly (knn_exact.hip rescore_kernel: the
// scan's own summation order) before a result is taken.  No precision is given
// up: the returned distances and rows are bit-identical to the f32 scan.
//
// Error bound (u = 2^-11 fp16 unit roundoff, g = 2^-24):
//   x_i -> fp16: |dx_i| <= u |x_i| + 2^-14 (normal range; the absolute term
//   also covers subnormals flushed to zero); q is scaled by a power of two so
//   that max|q_i| lies in [2^14, 2^15) before rounding, |dq_i| <= u |q_i| +
//   2^-26 max|q|; fp16 x fp16 products are exact in fp32; the fp32 sums of the
//   estimate and of the scan are each within (d + 2) g sum|x_i q_i|.  Hence
//     |dot_est - dot_scan| <= (2u + u^2 + 2^-26 sqrt(d) + (4d + 16) g) |x||q|
//                             + 2^-14 sqrt(d) |q|
//   and per metric (slack 1.25 for the roundings of the bound itself):
//     IP   e = A |x| + B                 (A, B carry |q|)
//     L2   e = A (|x|^2 + |q|^2) + B     on the squared distance (the scan's
//          direct sum of (x - q)^2 is within 2 (d + 2) g of it; covered)
//     cos  e = A + B / max(|x|, 1e-12)   on 0.5 - 0.5 cos
//   A component of magnitude >= 65520 (rounds to an fp16 infinity, so the
//   product comes out non-finite), a non-finite sum of squares or a query with
//   a non-finite norm forces the pair through (lb = -inf, ub = NaN, i.e. above
//   every number).  Components in [65504, 65520) round to 65504 within u.
//
// Tile: 256 corpus rows x 256 queries per 512-thread workgroup, one per CU
// (8 waves, 2 per SIMD: 4 row groups of 64 x 2 query groups of 128; each wave
// holds 2 x 4 accumulators of v_mfma_f32_32x32x16_f16).  K chunks of 32: the
// f32 rows stream in through buffer loads (non-temporal) two chunks ahead,
// are converted to fp16 on their way into a double-buffered LDS tile (rows
// padded by 16 B: conflict-free ds_read_b128 fragments); the pre-scaled fp16
// query tile (L2-resident, 393 KB for 256 x 768) is staged alongside, one
// chunk ahead.  Per-row sums of squares and fp16-overflow flags come from the
// same registers.  Measured (10M x 768, 256 queries: 8.5 ms per batch,
// tools/filter_diag.py switching parts off): the X stream alone runs at
// 6.8 TB/s (4.6 ms for all phases); re-reading the query tile from L2 for
// every 256-row tile and the LDS staging add ~1.3 ms, the MFMAs (~19 % of the
// dense fp16 peak, not overlapped with the stream inside one workgroup per
// CU) ~1 ms, the bound/test epilogue ~0.6 ms, the appends ~0.9 ms.  The
// 64-query variant: 4 row groups x 2 query groups of 32, K chunks of 64.
//
// This file holds what is compiled once: launch_filter (which variant a batch
// goes to), query preparation, the image builders and the overflow gate.  The
// kernels themselves are in filter/*.inc, one file per kernel family, and are
// compiled into five variant translation units (knn_filter_q256.hip, _h256,
// _q128, _q64, _q64i: one tile shape and namespace each; the header of each
// says which kernels it holds and which batches come to it).  The packed
// per-query row masks the QMASK builds read are made in knn_qmask.hip.
#include "fx_internal.h"

namespace fx {
namespace q256 {
int launch(const FilterArgs& a, int metric, hipStream_t stream);  // knn_filter_q256.hip
}
namespace q64 {
int launch(const FilterArgs& a, int metric, hipStream_t stream);  // knn_filter_q64.hip
}
namespace q128 {
int launch(const FilterArgs& a, int metric, hipStream_t stream);  // knn_filter_q128.hip
int launch_img6(const FilterArgs& a, int metric, hipStream_t stream);
bool img6_fits(int dq);
bool img6_fits_qmask(int dq);
}
namespace q64i {  // knn_filter_q64i.hip
int launch(const FilterArgs& a, int metric, hipStream_t stream);
int launch_img6(const FilterArgs& a, int metric, hipStream_t stream);
bool img6_fits(int dq);
bool img6_fits_qmask(int dq);
}
namespace h256 {
int launch(const FilterArgs& a, int metric, hipStream_t stream);  // knn_filter_h256.hip
}

// The register-staged kernel (measured faster for both row types: 8.5 vs
// 10.1 ms for configs[2]; see DESIGN.md for fp16) and filter images in MFMA
// fragment order (filter_img2_kernel).  Diagnostic builds keep the rejected
// LDS-DMA ring (FX_FILTER_RING=1) and row-major images (FX_IMAGE_TILED=0;
// read when an image is built and when it is searched: both must happen
// under the same setting).
bool image_tiled() { return diag_env("FX_IMAGE_TILED", 1) != 0; }

bool filter_ring() { return diag_env("FX_FILTER_RING", 0) != 0; }

// Batches of <= 64 queries take the 64-query tiles, 65..128 the 128-query ones
// (their Qh is padded to 64 / 128, filter_query_pad)
int launch_filter(const FilterArgs& a, int metric, hipStream_t stream) {
  // int8 images: a batch that fits one resident slice (<= 128 queries) runs
  // filter_img6_kernel (option "img6" 1; configs[1] 1.29 vs 1.34 ms, 128 L2
  // queries 1.81 vs 1.93 ms), larger ones filter_img3_kernel with 256-query
  // tiles (256 cosine queries: 2.97 ms against 3.34 ms for two img6 slices;
  // option 2 forces the slices, 0 disables img6)
  // per-query row masks: always the resident-slice kernel's QMASK build, the
  // only one that tests an admission bit per pair (plan_search planned the
  // filter only where filter_qmask_kind found a build that fits)
  if (a.qmask != nullptr) {
    const int kind = a.img8 ? filter_qmask_kind(a.dq, a.nq) : 0;
    if (kind == 0) {
      set_error("filter: per-query masks need an int8 image whose query slice fits (dq=%d)", a.dq);
      return FX_EUNSUPPORTED;
    }
    return kind == 128 ? q128::launch_img6(a, metric, stream) : q64i::launch_img6(a, metric, stream);
  }
  if (a.img8) {
    const int64_t i6 = option(kOptImg6);
    if (a.nq <= 64) {
      if (i6 >= 1 && q64i::img6_fits(a.dq)) return q64i::launch_img6(a, metric, stream);
      return q64i::launch(a, metric, stream);
    }
    if (a.nq <= 128) {
      if (i6 >= 1 && q128::img6_fits(a.dq)) return q128::launch_img6(a, metric, stream);
      return q128::launch(a, metric, stream);
    }
    if (i6 >= 2 && q128::img6_fits(a.dq)) return q128::launch_img6(a, metric, stream);
    return q256::launch(a, metric, stream);
  }
  if (a.nq <= 64) return q64::launch(a, metric, stream);
  if (a.nq <= 128 && !filter_ring()) return q128::launch(a, metric, stream);
  // tiled images: K chunks of 32 (5.07-5.10 vs 5.48-5.49 ms for configs[2]
  // in the 64-wide h256 build, profiles/r02_filter_img_bk32.log)
  if (a.rowinfo != nullptr && image_tiled()) return q256::launch(a, metric, stream);
  if (a.dtype == FX_DTYPE_F16 && !filter_ring()) return h256::launch(a, metric, stream);
  return q256::launch(a, metric, stream);
}

int filter_qmask_kind(int dq, int64_t nq) {
  if (nq > 64 && q128::img6_fits_qmask(dq)) return 128;
  return q64i::img6_fits_qmask(dq) ? 64 : 0;
}

// rows per tile of the kernel launch_filter picks for the dtype (every variant
// tiles rows alike)
int filter_tile_rows(int dtype) {
  (void)dtype;
  return kFilterTileRows;
}

int filter_query_pad(int64_t nq) { return nq <= 64 ? 64 : nq <= 128 && !filter_ring() ? 128 : 256; }
int filter_dq(int d) { return (d + 63) / 64 * 64; }  // covers every variant's K chunk

// Per query: the fp16 image scaled by 2^s (max|q| in [2^14, 2^15)), zero-padded
// to dq halves, and the bound constants {2^-s, norm term, A, B} (see the
// header).  The norm term is the scan's: sum of squares in the scan's order
// (lane-strided fmaf chain + xor butterfly, knn_scan.hip) -> |q|^2 (L2),
// |q| (IP), max(|q|, 1e-12) (cosine, coder.py:43-44).  Queries beyond nq
// (up to the padded count) are zero.  One wave per query.
__global__ void qprep_kernel(const float* __restrict__ Q, int64_t nq, int64_t nq_pad, int d, int dq,
                             int metric, uint16_t* __restrict__ Qh, float* __restrict__ qinfo) {
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= nq_pad) return;
  // blocks of 32 components, query-major inside a block (FilterArgs::Qh):
  // a K chunk of a query tile is one contiguous run of whole cache lines
  _Float16* out = reinterpret_cast<_Float16*>(Qh) + q * 32;
  auto at = [&](int i) -> _Float16& { return out[(int64_t)(i >> 5) * nq_pad * 32 + (i & 31)]; };
  if (q >= nq) {
    for (int i = lane; i < dq; i += 64) at(i) = (_Float16)0.f;
    return;
  }
  const float* qv = Q + q * (int64_t)d;
  float s = 0.f, m = 0.f;
  for (int i = lane; i < d; i += 64) {
    s = fmaf(qv[i], qv[i], s);
    m = fmaxf(m, fabsf(qv[i]));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s += __shfl_xor(s, o);
    m = fmaxf(m, __shfl_xor(m, o));
  }
  // power-of-two scale: exact, so the fp16 rounding is the only query error
  int ex = 0;
  if (m > 0.f && m <= 3.4e38f) (void)frexpf(m, &ex);  // m in [2^(ex-1), 2^ex)
  const int sh = 15 - ex;
  const float scale = ldexpf(1.f, sh > 126 ? 126 : (sh < -126 ? -126 : sh));
  for (int i = lane; i < dq; i += 64) at(i) = (_Float16)(i < d ? qv[i] * scale : 0.f);
  if (lane == 0) {
    const double u = 1.0 / 2048.0, g = 5.9604644775390625e-08;
    const double sd = sqrt((double)d);
    const double rel = 1.25 * (2.0 * u + u * u + sd * 1.4901161193847656e-08 + (4.0 * d + 16.0) * g);
    const double abs_ = 1.25 * sd * 6.103515625e-05 * (1.0 + 1.0 / 1024.0);
    const float qn = sqrtf(s);
    float a, b, t;
    if (metric == FX_METRIC_L2) {
      t = s;
      a = (float)rel;
      b = (float)(2.0 * abs_ * (double)qn);
    } else if (metric == FX_METRIC_IP) {
      t = qn;
      a = (float)(rel * (double)qn);
      b = (float)(abs_ * (double)qn);
    } else {
      t = fmaxf(qn, 1e-12f);
      a = (float)(0.5 * rel);
      b = (float)(0.5 * abs_);
    }
    if (!(s <= 3.4e38f) || !(m <= 3.4e38f)) a = __builtin_inff();  // forced query
    float* info = qinfo + q * 4;
    info[0] = 1.f / scale;
    info[1] = t;
    info[2] = a;
    info[3] = b;
  }
}

int launch_qprep(const float* Q, int64_t nq, int64_t nq_pad, int d, int dq, int metric,
                 uint16_t* Qh, float* qinfo, hipStream_t stream) {
  hipLaunchKernelGGL(qprep_kernel, dim3((unsigned)((nq_pad + 3) / 4)), dim3(256), 0, stream, Q,
                     nq, nq_pad, d, dq, metric, Qh, qinfo);
  return check_launch("qprep_kernel");
}

// The fp16 filter image of an f32 corpus (fx_filter_image): every component
// converted exactly as the f32 filter converts it in registers (round to
// nearest even), plus per row the f32 sum of squares of the original
// components, NaN when the row must be forced through (non-finite, or a
// component >= 65520 that becomes an fp16 infinity).  The filter then streams
// 2 bytes per component instead of 4 and skips its in-loop conversion and row
// sums; candidates are still rescored from the f32 rows, so results do not
// change.  One wave per row, grid-stride.
typedef float img_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 img_f16x4 __attribute__((ext_vector_type(4)));
#ifdef FX_DIAG_BUILD  // row-major images (FX_IMAGE_TILED=0)
__global__ void __launch_bounds__(256) image_kernel(const float* __restrict__ X, int64_t n, int d,
                                                    _Float16* __restrict__ img,
                                                    float* __restrict__ rowinfo) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += nw) {
    const img_f32x4* xr = reinterpret_cast<const img_f32x4*>(X + r * d);
    img_f16x4* ir = reinterpret_cast<img_f16x4*>(img + r * d);
    float s = 0.f, m = 0.f;
    for (int i = lane; i < d / 4; i += 64) {
      const img_f32x4 v = __builtin_nontemporal_load(xr + i);
      ir[i] = __builtin_convertvector(v, img_f16x4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s = fmaf(v[e], v[e], s);
        m = fmaxf(m, fabsf(v[e]));
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      s += __shfl_xor(s, o);
      m = fmaxf(m, __shfl_xor(m, o));
    }
    if (lane == 0) rowinfo[r] = (s <= 3.4e38f && m < 65520.f) ? s : __builtin_nanf("");
  }
}
#endif  // FX_DIAG_BUILD

// The image in MFMA fragment order (FX_IMAGE_TILED): one wave per 32-row
// tile, grid-stride.  Each k-step, lane l reads components 16 s + 8 (l / 32)
// .. + 7 of row 32 t + l % 32 (two 16-B loads; the other half of each line is
// read by the next k-step, from L2) and the wave writes the k-step's KB of
// the image as one contiguous store.  Padding rows and components are written
// as zeros (no memset).  d % 8 == 0 (fx_filter_image checks).
typedef _Float16 img_f16x8 __attribute__((ext_vector_type(8)));
__global__ void __launch_bounds__(256) image_tiled_kernel(const float* __restrict__ X, int64_t n,
                                                          int d, _Float16* __restrict__ img,
                                                          float* __restrict__ rowinfo) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int64_t nt = (n + 31) / 32;
  const int ksteps = (d + 15) / 16;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += nw) {
    const int64_t r = t * 32 + (lane & 31);
    const bool live = r < n;
    const float* xr = X + (live ? r : 0) * (int64_t)d;
    img_f16x8* out = reinterpret_cast<img_f16x8*>(img) + t * ksteps * 64 + lane;
    float s = 0.f, m = 0.f;
#pragma unroll 4
    for (int ks = 0; ks < ksteps; ++ks) {
      // loads without a branch (several k-steps in flight): padding reads a
      // valid address and is zeroed after
      const int k0 = 16 * ks + 8 * h;
      const bool ok = live && k0 < d;
      const float* p = xr + (k0 < d ? k0 : 0);
      // (plain loads: the line's other half is read at the next k-step, from L2;
      // nontemporal loads had it refetched, 2x the bytes)
      img_f32x4 a = *reinterpret_cast<const img_f32x4*>(p);
      img_f32x4 b = *reinterpret_cast<const img_f32x4*>(p + 4);
      if (!ok) {
        a = img_f32x4(0.f);
        b = img_f32x4(0.f);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s = fmaf(a[e], a[e], s);
        s = fmaf(b[e], b[e], s);
        m = fmaxf(m, fmaxf(fabsf(a[e]), fabsf(b[e])));
      }
      const img_f16x4 ca = __builtin_convertvector(a, img_f16x4);
      const img_f16x4 cb = __builtin_convertvector(b, img_f16x4);
      out[ks * 64] = __builtin_shufflevector(ca, cb, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    s += __shfl_xor(s, 32);
    m = fmaxf(m, __shfl_xor(m, 32));
    if (h == 0 && live) rowinfo[r] = (s <= 3.4e38f && m < 65520.f) ? s : __builtin_nanf("");
  }
}

int launch_image(const float* X, int64_t n, int d, void* img, float* rowinfo,
                 hipStream_t stream) {
  if (n <= 0) return FX_OK;
  int cus = 0;
  int rc = device_cus(&cus);
  if (rc) return rc;
  if (image_tiled()) {
    int64_t blocks = ((n + 31) / 32 + 3) / 4;
    if (blocks > (int64_t)cus * 8) blocks = (int64_t)cus * 8;
    hipLaunchKernelGGL(image_tiled_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, X, n, d,
                       reinterpret_cast<_Float16*>(img), rowinfo);
    return check_launch("image_tiled_kernel");
  }
#ifdef FX_DIAG_BUILD
  int64_t blocks = (n + 3) / 4;
  if (blocks > (int64_t)cus * 32) blocks = (int64_t)cus * 32;
  hipLaunchKernelGGL(image_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, X, n, d,
                     reinterpret_cast<_Float16*>(img), rowinfo);
  return check_launch("image_kernel");
#else
  return FX_EUNSUPPORTED;  // (unreachable: image_tiled() is constant)
#endif
}

// ---- int8 filter image (filter_img3_kernel<METRIC, true>, filter_img6_kernel,
// filter_img8_kernel; the bounds are derived in filter/tiled.inc, "int8 filter
// image").  Rows and queries are scaled so that
// their integer images have norm <= 2048 (|x~ . q~| <= 2^22):
//   s = max(max|x| / 127, |x| / (2046 - sqrt(d) / 2)).
__device__ __forceinline__ float i8_norm_cap(int d) { return 2046.f - 0.5f * sqrtf((float)d); }

typedef float img_f32x16 __attribute__((ext_vector_type(16)));

// The image in MFMA fragment order: [ceil(n / 32) row tiles][ceil(d / 32)
// k-steps][64 lanes][16 B]: lane l holds components 32 s + 16 (l / 32) .. + 15
// of row 32 t + l % 32 (the v_mfma_i32_32x32x32_i8 A operand), and per row
// {omega = w + kappa v, 1/s, N/s, n^2/s} (NaN omega: forced).  One wave per
// 32-row tile: a pass for max |x| and n^2, a pass that quantizes, writes and
// accumulates the residual (|x - s x~|^2 in f32 with (d + 8) u slack) and
// w^2 (exact in integers).  d % 8 == 0 (fx_filter_image8 checks).
// T: the corpus's value type, float or _Float16 (the values are the same
// reals in f32, so the bounds below are unchanged; the candidates are rescored
// from the T rows in the scan's order)
// Image row r holds corpus row perm_row(pa, n, r) (image8_perm): the tile's
// 32 rows come from 32 places of the corpus, each still read as whole
// 128-B lines.
template <typename T>
__global__ void __launch_bounds__(256) image8_kernel(const T* __restrict__ X, int64_t n, int d,
                                                    int8_t* __restrict__ img,
                                                    float* __restrict__ rowinfo, uint64_t pa) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int64_t nt = (n + 31) / 32;
  const int ksteps = (d + 31) / 32;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const float u = 5.9604644775390625e-08f;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += nw) {
    const int64_t r = t * 32 + (lane & 31);
    const bool live = r < n;
    const T* xr = X + (live ? (int64_t)perm_row(pa, n, r) : 0) * (int64_t)d;
    auto load = [&](int ks) {  // components 32 ks + 16 h .. + 15 (zeros past d)
      img_f32x16 v;
      const int k0 = 32 * ks + 16 * h;
      if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + 4 * j;
          const img_f32x4 q4 = (live && k < d) ? *reinterpret_cast<const img_f32x4*>(xr + k)
                                                : img_f32x4(0.f);
          v[4 * j] = q4[0];
          v[4 * j + 1] = q4[1];
          v[4 * j + 2] = q4[2];
          v[4 * j + 3] = q4[3];
        }
      } else {  // 8 halves per 16-B load (d % 8 == 0)
        typedef _Float16 img_f16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int k = k0 + 8 * j;
          const img_f16x8 h8 = (live && k < d) ? *reinterpret_cast<const img_f16x8*>(xr + k)
                                                : img_f16x8((_Float16)0.f);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[8 * j + e] = (float)h8[e];
        }
      }
      return v;
    };
    float m = 0.f, n2 = 0.f;
    for (int ks = 0; ks < ksteps; ++ks) {
      const img_f32x16 v = load(ks);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        n2 = fmaf(v[e], v[e], n2);
        m = fmaxf(m, fabsf(v[e]));
      }
    }
    n2 += __shfl_xor(n2, 32);
    m = fmaxf(m, __shfl_xor(m, 32));
    const bool finite = m <= 3.4e38f && n2 <= 3.4e38f;
    const float nrm = sqrtf(n2);
    float sc = fmaxf(m * (1.f / 127.f), nrm / i8_norm_cap(d));
    if (!(sc > 1e-30f) || !finite) sc = 1.f;  // zero / tiny / non-finite rows (forced below)
    const float is = 1.f / sc;
    int w2 = 0;
    float e2 = 0.f;
    int8_t* out = img + (t * ksteps) * 1024 + lane * 16;
    for (int ks = 0; ks < ksteps; ++ks) {
      const img_f32x16 v = load(ks);
      int32_t packed[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float x = v[4 * j + b];
          float qf = rintf(x * is);
          qf = fminf(fmaxf(qf, -127.f), 127.f);
          if (!finite) qf = 0.f;
          const int qi = (int)qf;
          w2 += qi * qi;
          const float res = fmaf(-sc, qf, x);
          e2 = fmaf(res, res, e2);
          word |= ((uint32_t)qi & 0xffu) << (8 * b);
        }
        packed[j] = (int32_t)word;
      }
      *reinterpret_cast<int4*>(out + ks * 1024) = make_int4(packed[0], packed[1], packed[2], packed[3]);
    }
    w2 += __shfl_xor(w2, 32);
    e2 += __shfl_xor(e2, 32);
    if (h == 0 && live) {
      const float e = sqrtf(e2 * (1.f + 2.f * (float)(d + 8) * u)) * (1.f + 4.f * u);
      const float w = sqrtf((float)w2) * (1.f + 2.f * u);
      const float v = e * is * (1.f + 4.f * u);
      float om = (w + kI8Kappa * v) * (1.f + 4.f * u);
      const bool tiny = !(m == 0.f) && !(fmaxf(m * (1.f / 127.f), nrm / i8_norm_cap(d)) > 1e-30f);
      if (!finite || tiny || w > 2048.f || !(om <= 3.4e38f)) om = __builtin_nanf("");
      const float nn = fmaxf(nrm, 1e-12f);
      img_f32x4 info = {om, is, nn * is, n2 * is};
      *reinterpret_cast<img_f32x4*>(rowinfo + r * kI8RowInfo) = info;
    }
  }
}

// The same image and row terms for quint8 codes (FX_DTYPE_QU8): the rows are
// x = sigma y with y = code - zero point, integers in [-255, 255], and the
// quint8 scan (fx_exact.h slot_accumulate_qu8, sums_distance) never forms x:
// it sums in code units and multiplies by sigma at the end.  Everything below is derived from the integers.
//
// Row terms.  Y2 = sum y^2 is an exact integer.  The row is quantised in code
// units, t = max(max|y| / 127, sqrt(Y2) / i8_norm_cap(d)), x~ = rint(y / t)
// clamped to [-127, 127] (however t and x~ came out, the terms describe the x~
// that was written), so its scale is s = sigma t and
//   x - s x~ = sigma (y - t x~).
// t x~ has at most 31 significant bits and y - t x~ is exact in double for
// t >= 2^-22 (t >= 1/127 for a non-zero row), so e_c = |y - t x~| comes from
// a double sum of exact squares (relative error d 2^-53, covered by 1e-12),
// and w^2 = sum x~^2 is an exact integer.  sigma cancels in v = e / s = e_c / t:
//   omega = w + kappa e_c / t         (double, rounded up to f32)
//   1/s   = 1 / (sigma t),   N/s = sqrt(Y2) / t,   n^2/s = sigma Y2 / t
// each the f32 nearest to its double value (N = max(sigma sqrt(Y2), 1e-12)):
// one rounding u per term, where the f32 builder above carries the f32 sums'
// g in n^2 and N; the kernels' constants (filter/tiled.inc) allow g + 16 u.
// A zero row takes s = 1 like the f32 builder's.  Forced (omega = NaN): a row
// whose integer image exceeds norm 2048, or one of whose terms leaves the f32
// range (sigma below ~1e-30 or above ~1e30); no quint8 row is non-finite.
//
// What the bounds are held against (filter/tiled.inc, "int8 filter image";
// u = 2^-24, g = (d + 2) u 1.01; d % 16 == 0, so d >= 16).  Every term of the
// scan's sums passes 8 fmas of its pair chain, the a2.x + a2.y add, at most
// ceil(d / 256) adds into acc and the 4 of sum16: r = 13 + ceil(d / 256)
// roundings, and r + 3 <= d + 2 for every d >= 16.
//   IP   s1 = sum y q (1 + th_i), |th_i| <= r u (y = code - zp is exact), and
//        the distance is -fl(sigma s1): within (r + 1) u (1 + u) |x||q| <= g |x||q|
//        of -x.q, the budget launch_qprep8 puts into P and R.  q is the query.
//   cos  the same s1, s2 = sum y^2 within r u, then sigma s1, sigma sqrt(s2),
//        the product of the norms, the division and 0.5 - 0.5 r: under
//        2 r u + 8 u, plus the g / 2 of the scan's f32 |q| as for f32 rows,
//        on 0.5 - 0.5 cos against the constant c = 3 g + 16 u.
//        The cosine of sigma y is the cosine of y.  q is the query.
//   L2   the scan compares codes with q' = fl(zp + fl(q / sigma)), so what it
//        measures is the distance to the EFFECTIVE query qe = sigma (q' - zp):
//        sigma^2 sum (code - q')^2 = |x - qe|^2 exactly.  Against the raw q
//        the two differ by u (sigma zp sqrt(d) + |q|), absolute, which no
//        relative slack covers when zp is far from the codes or q is almost a
//        row.  launch_qprep8 is therefore given qe, evaluated in double from
//        the scan's own q' bits (launch_qu8_query; the product rounds to
//        2^-53, below R' >= P / kappa by 2^-46).  What is left is relative:
//        fl(code - q') twice per square (2 u), the sums (r u), the square root
//        and the final sigma multiply (4 u on the square): (r + 6) u < g2 =
//        2 g + 8 u on |x - qe|^2.  n_q^2 and |q| of the record are qe's.
// So the quint8 image needs no wider omega or query record than the f32 one:
// the constants of filter/tiled.inc are untouched.
__global__ void __launch_bounds__(256) image8_qu8_kernel(const uint8_t* __restrict__ X, int64_t n,
                                                        int d, int8_t* __restrict__ img,
                                                        float* __restrict__ rowinfo, uint64_t pa,
                                                        Quant z) {
  typedef uint8_t u8x16 __attribute__((ext_vector_type(16)));
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int64_t nt = (n + 31) / 32;
  const int ksteps = (d + 31) / 32;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int zp = (int)z.shift;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += nw) {
    const int64_t r = t * 32 + (lane & 31);
    const bool live = r < n;
    const uint8_t* xr = X + (live ? (int64_t)perm_row(pa, n, r) : 0) * (int64_t)d;
    // y of components 32 ks + 16 h .. + 15 (zeros past d and in padding rows)
    auto load = [&](int ks, int (&y)[16]) {
      const int k0 = 32 * ks + 16 * h;
      const bool ok = live && k0 < d;
      const u8x16 c = *reinterpret_cast<const u8x16*>(xr + (ok ? k0 : 0));
#pragma unroll
      for (int e = 0; e < 16; ++e) y[e] = ok ? (int)c[e] - zp : 0;
    };
    int my = 0;
    unsigned long long y2 = 0ull;
    for (int ks = 0; ks < ksteps; ++ks) {
      int y[16];
      load(ks, y);
      unsigned part = 0u;  // (16 squares of at most 255^2)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        part += (unsigned)(y[e] * y[e]);
        my = max(my, abs(y[e]));
      }
      y2 += part;
    }
    y2 += __shfl_xor(y2, 32);
    my = max(my, __shfl_xor(my, 32));
    const double ny = sqrt((double)y2);
    float tc = fmaxf((float)my * (1.f / 127.f), (float)(ny / (double)i8_norm_cap(d)) * (1.f + 1e-6f));
    if (my == 0) tc = 1.f;  // zero row: x~ = 0 under any scale
    const float it = 1.f / tc;
    int w2 = 0;
    double e2 = 0.0;
    int8_t* out = img + (t * ksteps) * 1024 + lane * 16;
    for (int ks = 0; ks < ksteps; ++ks) {
      int y[16];
      load(ks, y);
      int32_t packed[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int yi = y[4 * j + b];
          const float qf = fminf(fmaxf(rintf((float)yi * it), -127.f), 127.f);
          const int qi = (int)qf;
          w2 += qi * qi;
          const double res = (double)yi - (double)tc * (double)qi;  // exact
          e2 = fma(res, res, e2);
          word |= ((uint32_t)qi & 0xffu) << (8 * b);
        }
        packed[j] = (int32_t)word;
      }
      *reinterpret_cast<int4*>(out + ks * 1024) = make_int4(packed[0], packed[1], packed[2], packed[3]);
    }
    w2 += __shfl_xor(w2, 32);
    e2 += __shfl_xor(e2, 32);
    if (h == 0 && live) {
      const double w = sqrt((double)w2);
      const double ec = sqrt(e2) * (1.0 + 1e-12);
      const double om = (w + (double)kI8Kappa * (ec / (double)tc)) * (1.0 + 1e-12);
      const double s = my == 0 ? 1.0 : (double)z.scale * (double)tc;
      const double nn = fmax((double)z.scale * ny, 1e-12);
      const float is = (float)(1.0 / s), y1n = (float)(nn / s);
      const float y1l = (float)((double)z.scale * (double)z.scale * (double)y2 / s);
      float omf = __double2float_ru(om);
      if (w > 2048.0 || !(s > 1e-30) || !(is <= 3.4e38f) || !(y1n <= 3.4e38f) ||
          !(y1l <= 3.4e38f) || !(omf <= 3.4e38f))
        omf = __builtin_nanf("");
      const img_f32x4 info = {omf, is, y1n, y1l};
      *reinterpret_cast<img_f32x4*>(rowinfo + r * kI8RowInfo) = info;
    }
  }
}

static uint64_t gcd64(uint64_t a, uint64_t b) {
  while (b != 0) {
    const uint64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

uint64_t image8_perm(int64_t n) {
  if (n <= 2) return 1;
  uint64_t a = (uint64_t)((double)n * 0.6180339887498949) | 1u;
  while (gcd64(a, (uint64_t)n) != 1) a += 2;
  return a % (uint64_t)n;
}

int launch_image8(const void* X, int dtype, int64_t n, int d, void* img, float* rowinfo,
                  hipStream_t stream, Quant z) {
  if (n <= 0) return FX_OK;
  int cus = 0;
  int rc = device_cus(&cus);
  if (rc) return rc;
  int64_t blocks = ((n + 31) / 32 + 3) / 4;
  if (blocks > (int64_t)cus * 8) blocks = (int64_t)cus * 8;
  const uint64_t pa = image8_perm(n);
  if (dtype == FX_DTYPE_QU8)
    hipLaunchKernelGGL(image8_qu8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
                       reinterpret_cast<const uint8_t*>(X), n, d, reinterpret_cast<int8_t*>(img),
                       rowinfo, pa, z);
  else if (dtype == FX_DTYPE_F16)
    hipLaunchKernelGGL(image8_kernel<_Float16>, dim3((unsigned)blocks), dim3(256), 0, stream,
                       reinterpret_cast<const _Float16*>(X), n, d, reinterpret_cast<int8_t*>(img),
                       rowinfo, pa);
  else
    hipLaunchKernelGGL(image8_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream,
                       reinterpret_cast<const float*>(X), n, d, reinterpret_cast<int8_t*>(img),
                       rowinfo, pa);
  return check_launch("image8_kernel");
}

// Per query (one wave): q~ = rint(q / s_q) in int8, zero-padded to dq, in
// 64-component chunks, query-major inside a chunk (chunk c of query q: 64 B
// at (c * nq_pad + q) * 64), and {s_q, R', n_q^2, |q|} with
// R' = max(R, P / kappa) (see "int8 filter image"); sums in double (products
// of f32 and of f32 x int8 are exact there).  A non-finite query, or one whose
// integer image exceeds norm 2048: R' = +inf (forced).
// QE (quint8 L2, see image8_qu8_kernel): Q holds the scan's q', and the
// query is qe = ze.scale * (q' - ze.shift) in double (q' - shift is exact,
// the product rounds to 2^-53: with the residual's subtraction below, far
// inside R' >= P / kappa and its 1e-6).
template <bool QE>
__global__ void qprep8_kernel(const float* __restrict__ Q, int64_t nq, int64_t nq_pad, int d,
                              int dq, int metric, int8_t* __restrict__ Qb,
                              float* __restrict__ qinfo, uint64_t* __restrict__ thr,
                              uint32_t* __restrict__ count, Quant ze) {
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= nq_pad) return;
  if (q < nq && lane == 0) {  // (the search's threshold and append count, when given)
    if (thr != nullptr) thr[q] = ~0ull;
    if (count != nullptr) count[q * kCountStride] = 0u;
  }
  auto at = [&](int i) -> int8_t& {
    return Qb[((int64_t)(i >> 6) * nq_pad + q) * 64 + (i & 63)];
  };
  if (q >= nq) {
    for (int i = lane; i < dq; i += 64) at(i) = 0;
    return;
  }
  const float* qv = Q + q * (int64_t)d;
  auto val = [&](int i) -> double {
    if constexpr (QE) return (double)ze.scale * ((double)qv[i] - (double)ze.shift);
    return (double)qv[i];
  };
  double s2 = 0.0;
  float m = 0.f;
  for (int i = lane; i < d; i += 64) {
    s2 = fma(val(i), val(i), s2);
    m = fmaxf(m, QE ? __double2float_ru(fabs(val(i))) : fabsf(qv[i]));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s2 += __shfl_xor(s2, o);
    m = fmaxf(m, __shfl_xor(m, o));
  }
  const bool finite = m <= 3.4e38f && s2 <= 1e76;
  const double nq_ = sqrt(s2);
  float sc = fmaxf(m * (1.f / 127.f), (float)(nq_ / (double)i8_norm_cap(d)) * (1.f + 1e-6f));
  const bool tiny = m != 0.f && !(sc > 1e-30f);
  if (!(sc > 1e-30f) || !finite) sc = 1.f;
  const float is = 1.f / sc;
  double e2 = 0.0;
  int w2 = 0;
  for (int i = lane; i < dq; i += 64) {
    int qi = 0;
    if (i < d && finite) {
      float qf = rintf((QE ? (float)val(i) : qv[i]) * is);
      qf = fminf(fmaxf(qf, -127.f), 127.f);
      qi = (int)qf;
      const double r = val(i) - (double)sc * (double)qi;  // exact (QE: to 2^-53)
      e2 = fma(r, r, e2);
    }
    w2 += qi * qi;
    at(i) = (int8_t)qi;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    e2 += __shfl_xor(e2, o);
    w2 += __shfl_xor(w2, o);
  }
  if (lane == 0) {
    const double u = 5.9604644775390625e-08;
    const double g = (double)(d + 2) * u * 1.01;
    const double eq = sqrt(e2) * (1.0 + 1e-12);
    double P = nq_ / sc, R = eq / sc;
    if (metric == FX_METRIC_IP) {
      R += g * nq_ / sc;
      P *= 1.0 + g;
    }
    double rp = R > P / (double)kI8Kappa ? R : P / (double)kI8Kappa;
    rp *= 1.0 + 1e-6;
    if (!finite || tiny || sqrt((double)w2) > 2048.0) rp = __builtin_inf();
    float* info = qinfo + q * kI8QInfo;
    info[0] = sc;
    info[1] = __double2float_ru(rp);
    info[2] = (float)s2;
    info[3] = (float)nq_;
  }
}

int launch_qprep8(const float* Q, int64_t nq, int64_t nq_pad, int d, int dq, int metric,
                  int8_t* Qb, float* qinfo, hipStream_t stream, uint64_t* thr, uint32_t* count,
                  const Quant* qe) {
  const dim3 grid((unsigned)((nq_pad + 3) / 4));
  if (qe != nullptr)
    hipLaunchKernelGGL(qprep8_kernel<true>, grid, dim3(256), 0, stream, Q, nq, nq_pad, d, dq,
                       metric, Qb, qinfo, thr, count, *qe);
  else
    hipLaunchKernelGGL(qprep8_kernel<false>, grid, dim3(256), 0, stream, Q, nq, nq_pad, d, dq,
                       metric, Qb, qinfo, thr, count, Quant());
  return check_launch("qprep8_kernel");
}


}  // namespace fx
