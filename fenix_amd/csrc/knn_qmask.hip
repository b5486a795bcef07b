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
#include "fx_internal.h"

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

}  // namespace fx
