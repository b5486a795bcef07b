// Per-query row masks for the int8 filter (fx_qmask_pack): nq ordinary row
// bitmaps, masks[q][row >> 5] bit row & 31, become one row-major bit matrix
// out[n][qw], bit q & 31 of word q >> 5 of row r set when query q admits
// row r (qw = qmask_words(nq): whole 16-B groups of 128 queries, padding
// bits zero).  Row-major by CORPUS row: filter_img6_kernel<., true> reads a
// row's query bits with one 16-B load beside the shared mask's word, at
// crow = perm_row(image row), so nothing is permuted into image order.
//
// One workgroup transposes 1 024 rows x 128 queries: the 128 x 32 input words
// come in as 128-B runs per query (coalesced), every (32 rows, 32 queries)
// block is transposed in registers by 32 ballots (lane i of a half-wave holds
// query i's word; ballot r collects bit r of all 32 queries, which is row r's
// output word), and the 1 024 x 16 B of output leave as one contiguous run
// when qw == 4 (16-B pieces qw words apart otherwise).  Traffic: nq n / 8
// bytes in and out.
//
// fx_code_qmask (below) builds the same two forms for a batch of probe
// searches straight from the row codes, in one pass over them.
#include "fx_internal.h"
#include "fx_wave.h"

namespace fx {

constexpr int kQpRows = 1024;  // rows per workgroup (32 input words)
constexpr int kQpQueries = 128;  // queries per workgroup (4 output words)

__global__ void __launch_bounds__(256)
    qmask_pack_kernel(const uint32_t* __restrict__ masks, int64_t mask_stride, int64_t nq,
                      int64_t n, uint32_t* __restrict__ out, int64_t qw) {
  __shared__ uint32_t in[kQpQueries][33];
  __shared__ uint4 ot[kQpRows];
  const int tid = threadIdx.x;
  const int64_t w0 = (int64_t)blockIdx.x * 32, q0 = (int64_t)blockIdx.y * kQpQueries;
  const int64_t nwords = (n + 31) / 32;
  for (int i = tid; i < kQpQueries * 32; i += 256) {
    const int q = i >> 5, j = i & 31;
    const int64_t gq = q0 + q, w = w0 + j;
    in[q][j] = gq < nq && w < nwords ? masks[gq * mask_stride + w] : 0u;
  }
  __syncthreads();
  const int half = tid >> 5, l = tid & 31;
  uint32_t* otw = reinterpret_cast<uint32_t*>(ot);
  for (int it = 0; it < 16; ++it) {  // 32 words x 4 query groups over 8 half-waves
    const int p = it * 8 + half;
    const int u = p & 3, j = p >> 2;
    const uint32_t v = in[u * 32 + l][j];
    uint32_t res = 0u;
#pragma unroll
    for (int r = 0; r < 32; ++r) {
      const uint64_t b = __ballot((v >> r) & 1u);
      const uint32_t mine = (half & 1) ? (uint32_t)(b >> 32) : (uint32_t)b;
      if (l == r) res = mine;
    }
    otw[(j * 32 + l) * 4 + u] = res;
  }
  __syncthreads();
  for (int i = tid; i < kQpRows; i += 256) {
    const int64_t r = w0 * 32 + i;  // (rows >= n inside the last input word: not written)
    if (r < n) *reinterpret_cast<uint4*>(out + r * qw + (int64_t)blockIdx.y * 4) = ot[i];
  }
}

int64_t qmask_words(int64_t nq) { return nq < 1 ? 0 : ((nq + 31) / 32 + 3) / 4 * 4; }

int launch_qmask_pack(const uint32_t* masks, int64_t mask_stride, int64_t nq, int64_t n,
                      uint32_t* out, hipStream_t stream) {
  const int64_t qw = qmask_words(nq);
  const int64_t bx = (n + kQpRows - 1) / kQpRows, by = qw / 4;
  if (bx > 0x7fffffffll || by > 65535) {
    set_error("fx_qmask_pack: n=%lld nq=%lld too large", (long long)n, (long long)nq);
    return FX_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(qmask_pack_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, stream,
                     masks, mask_stride, nq, n, out, qw);
  return check_launch("qmask_pack_kernel");
}

// ---- row codes -> the per-query masks of a probe batch (fx_code_qmask)
//
// The tile of qmask_pack_kernel run the other way: a workgroup takes 1 024 rows
// x one 128-query group.  The probe sets arrive code-major, selT[ncodes][qw]
// (launch_qmask_pack over `sel`, codes in the role of rows: bit q of row c set
// when target q selected code c; 2 MB for 65 536 codes x 256 targets, L2
// resident), so a row's admission bits for the group are ONE 16-B gather at
// its code.  The piece is cleared by the filter bit or a code outside
// [0, ncodes), stored as the row's 16 B of out_qmask (one contiguous run per
// workgroup when qw == 4), and transposed from the same registers into the row
// bitmaps: a 64-lane ballot of query b's bit is two words of out_masks[b];
// lane b of the wave keeps ballot b, so 64 queries leave as one 8-B LDS store
// per lane into a 128 x 32-word tile, which is written as 128-B runs per
// query.  Kept rows: popcounts of the tile's words, summed per thread over the
// workgroup's tiles (thread <-> (query, word) is the same for every tile),
// reduced over half-waves into partial[group][workgroup][128]; count_kernel
// sums the partials (integer sums: deterministic, no atomics).
// Traffic: row_code and filter once per query group; nothing of size nq n read.
constexpr int kCqBlocks = 2048;  // workgroups per query group at most (grid-stride over tiles)
constexpr int kCqRow = 34;       // LDS tile row: 32 words + 2 (8-B aligned rows)

__global__ void __launch_bounds__(256)
    code_qmask_kernel(const int64_t* __restrict__ code, int64_t n,
                      const uint32_t* __restrict__ selT, int64_t qw, int64_t nq, int64_t ncodes,
                      const uint32_t* __restrict__ filter, uint32_t* __restrict__ out_masks,
                      int64_t mask_stride, uint32_t* __restrict__ out_qmask,
                      uint32_t* __restrict__ partial) {
  __shared__ __attribute__((aligned(8))) uint32_t tile[kQpQueries][kCqRow];
  __shared__ uint32_t sums[kQpQueries];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t g = blockIdx.y, q0 = g * kQpQueries;
  const int64_t nwords = (n + 31) / 32;
  const int64_t tiles = (n + kQpRows - 1) / kQpRows;
  const bool bitmaps = out_masks != nullptr || partial != nullptr;
  const int live = (int)(nq - q0 < kQpQueries ? nq - q0 : kQpQueries);  // queries of this group
  uint32_t cnt[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) cnt[t] = 0u;
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t r0 = ti * kQpRows + tid;
    int64_t c[4];
    bool ok[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int64_t r = r0 + it * 256;
      c[it] = r < n ? code[r] : -1;
      ok[it] = true;
      if (filter != nullptr && r < n) ok[it] = (filter[r >> 5] >> (r & 31)) & 1u;
    }
    uint4 p[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      p[it] = make_uint4(0u, 0u, 0u, 0u);
      if (ok[it] && c[it] >= 0 && c[it] < ncodes)
        p[it] = *reinterpret_cast<const uint4*>(selT + c[it] * qw + g * 4);
    }
    if (out_qmask != nullptr) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int64_t r = r0 + it * 256;
        if (r < n) *reinterpret_cast<uint4*>(out_qmask + r * qw + g * 4) = p[it];
      }
    }
    if (!bitmaps) continue;
    __syncthreads();  // the previous tile has been written out
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const uint32_t w[4] = {p[it].x, p[it].y, p[it].z, p[it].w};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        uint64_t mine = 0ull;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          // only the group's live queries are balloted, eight at a time (the
          // bound is wave-uniform; a padding query's bits are zero in selT)
          const uint32_t word = w[h * 2 + s];
          const int left = live - (h * 64 + s * 32);
          for (int b0 = 0; b0 < left && b0 < 32; b0 += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const uint64_t bal = __ballot((word >> (b0 + u)) & 1u);
              if (lane == s * 32 + b0 + u) mine = bal;
            }
          }
        }
        // rows it * 256 + wv * 64 .. + 63 of the tile: words it * 8 + wv * 2, + 1
        *reinterpret_cast<uint64_t*>(&tile[h * 64 + lane][it * 8 + wv * 2]) = mine;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (8 * t >= live) break;  // (workgroup-uniform: eight queries per step)
      const int q = (tid >> 5) + 8 * t, j = tid & 31;
      const uint32_t v = tile[q][j];  // (queries >= nq: selT's padding bits are zero)
      const int64_t gq = q0 + q, wd = ti * 32 + j;
      if (out_masks != nullptr && gq < nq && wd < nwords) out_masks[gq * mask_stride + wd] = v;
      cnt[t] += (uint32_t)__popc(v);
    }
  }
  if (partial == nullptr) return;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    uint32_t s = cnt[t];
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if ((tid & 31) == 0) sums[(tid >> 5) + 8 * t] = s;
  }
  __syncthreads();
  if (tid < kQpQueries)
    partial[(g * gridDim.x + blockIdx.x) * kQpQueries + tid] = sums[tid];
}

// one wave per query: the sum of its workgroup partials
__global__ void __launch_bounds__(256)
    code_qmask_count_kernel(const uint32_t* __restrict__ partial, int64_t blocks, int64_t nq,
                            unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  const uint32_t* p = partial + (q / kQpQueries) * blocks * kQpQueries + q % kQpQueries;
  uint64_t s = 0;
  for (int64_t b = lane; b < blocks; b += 64) s += p[b * kQpQueries];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += shfl_xor_u64(s, m);
  if (lane == 0) out[q] = s;
}

namespace {

struct CodeQmaskLayout {
  int64_t qw, groups;
  size_t off_part, total;
};

constexpr size_t kCqMaxTable = (size_t)1 << 30;  // selT above 1 GiB: the per-target route

int code_qmask_layout(int64_t nq, int64_t ncodes, CodeQmaskLayout* l) {
  l->qw = qmask_words(nq);
  l->groups = l->qw / 4;
  if (l->groups > 65535 || ncodes > 0x7fffffffll ||
      (size_t)ncodes > kCqMaxTable / ((size_t)l->qw * 4)) {
    set_error("fx_code_qmask: %lld codes x %lld targets exceed the code-major table's 1 GiB",
              (long long)ncodes, (long long)nq);
    return FX_EUNSUPPORTED;
  }
  const size_t table = (size_t)ncodes * l->qw * 4;
  l->off_part = (table + 255) / 256 * 256;
  l->total = l->off_part + (size_t)l->groups * kCqBlocks * kQpQueries * 4;
  return FX_OK;
}

}  // namespace

}  // namespace fx

using namespace fx;

extern "C" {

int fx_code_qmask_workspace_bytes(int64_t nq, int64_t ncodes, size_t* out_bytes) {
  if (out_bytes == nullptr || nq < 1 || ncodes < 1) {
    set_error("fx_code_qmask_workspace_bytes: invalid arguments");
    return FX_EINVAL;
  }
  CodeQmaskLayout l;
  int rc = code_qmask_layout(nq, ncodes, &l);
  if (rc) return rc;
  *out_bytes = l.total;
  return FX_OK;
}

int fx_code_qmask(const int64_t* row_code, int64_t n, const uint32_t* sel, int64_t sel_stride,
                  int64_t nq, int64_t ncodes, const uint32_t* filter, void* ws, size_t ws_bytes,
                  uint32_t* out_masks, int64_t mask_stride, uint32_t* out_qmask,
                  uint64_t* out_counts, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (nq < 1 || ncodes < 1 || n < 0) {
    set_error("fx_code_qmask: nq=%lld ncodes=%lld n=%lld", (long long)nq, (long long)ncodes,
              (long long)n);
    return FX_EINVAL;
  }
  if (sel == nullptr || ws == nullptr || (n > 0 && row_code == nullptr)) {
    set_error("fx_code_qmask: null pointer argument");
    return FX_EINVAL;
  }
  if (out_masks == nullptr && out_qmask == nullptr && out_counts == nullptr) {
    set_error("fx_code_qmask: no output");
    return FX_EINVAL;
  }
  if (sel_stride < (ncodes + 31) / 32 || (out_masks != nullptr && mask_stride < (n + 31) / 32)) {
    set_error("fx_code_qmask: sel_stride=%lld mask_stride=%lld below %lld / %lld words",
              (long long)sel_stride, (long long)mask_stride, (long long)((ncodes + 31) / 32),
              (long long)((n + 31) / 32));
    return FX_EINVAL;
  }
  if ((uintptr_t)out_qmask % 16 != 0 || (uintptr_t)ws % 16 != 0) {
    set_error("fx_code_qmask: out_qmask or workspace not 16-byte aligned");
    return FX_EINVAL;
  }
  CodeQmaskLayout l;
  int rc = code_qmask_layout(nq, ncodes, &l);
  if (rc) return rc;
  if (ws_bytes < l.total) {
    set_error("workspace too small: %zu < %zu", ws_bytes, l.total);
    return FX_EINVAL;
  }
  if (n == 0) {
    if (out_counts == nullptr) return FX_OK;
    hipError_t e = hipMemsetAsync(out_counts, 0, (size_t)nq * 8, stream);
    if (e != hipSuccess) {
      set_error("code qmask memset: %s", hipGetErrorString(e));
      return FX_EHIP;
    }
    return FX_OK;
  }
  char* w = reinterpret_cast<char*>(ws);
  uint32_t* selT = reinterpret_cast<uint32_t*>(w);
  uint32_t* partial = out_counts != nullptr ? reinterpret_cast<uint32_t*>(w + l.off_part) : nullptr;
  rc = launch_qmask_pack(sel, sel_stride, nq, ncodes, selT, stream);
  if (rc) return rc;
  const int64_t tiles = (n + kQpRows - 1) / kQpRows;
  const int64_t blocks = tiles < kCqBlocks ? tiles : kCqBlocks;
  hipLaunchKernelGGL(code_qmask_kernel, dim3((unsigned)blocks, (unsigned)l.groups), dim3(256), 0,
                     stream, row_code, n, selT, l.qw, nq, ncodes, filter, out_masks, mask_stride,
                     out_qmask, partial);
  rc = check_launch("code_qmask_kernel");
  if (rc || out_counts == nullptr) return rc;
  hipLaunchKernelGGL(code_qmask_count_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, stream,
                     partial, blocks, nq, reinterpret_cast<unsigned long long*>(out_counts));
  return check_launch("code_qmask_count_kernel");
}

}  // extern "C"
