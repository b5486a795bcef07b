// filter_img2_kernel: tiled fp16 filter images, the query tile staged through
// registers (after filter/tile.inc).
#ifndef FX_I2_SEG // LDS append segment per query (0: a global atomic per lane and query);
                   // 64-query tiles only: 16 entries in the 256-query build (the most
                   // its LDS holds) measured 3.5 % slower (DESIGN.md 3.6)
#define FX_I2_SEG (FX_FILTER_BQ >= 256 ? 0 : 32)
#endif
//
// The fp16 image of an f32 corpus in MFMA fragment order (FX_IMAGE_TILED,
// default on), [ceil(n / 32) row tiles][ceil(d / 16) k-steps][64 lanes][8
// halves]: lane l holds row 32 t + l % 32, components 16 s + 8 (l / 32) ..
// + 7, i.e. one v_mfma_f32_32x32x16_f16 A operand, one contiguous KB per wave
// load.  Each of the 8 waves owns one 32-row tile of the 256-row tile against
// all the queries and loads its A fragments straight into registers (two
// chunks ahead); only the query tile goes through LDS.
struct Img2Shared {
  _Float16 qs[2][fBQ * fLds];
  float rinfo[fBM];
  float rterm[fBM];
  uint32_t rflags[2][kRowFlagWords];
  f32x4 qtab[fBQ];
  float2 qab[fBQ];
#if FX_I2_SEG > 0
  uint32_t seg[fBQ + 3 * fBQ * FX_I2_SEG];  // counters, then entries (filter_epilogue_seg)
  uint32_t segbase[fBQ];
#endif
};
static_assert(sizeof(Img2Shared) <= 160 * 1024, "filter_img2_kernel: LDS over 160 KB");
static_assert(fWaves * 32 == fBM, "tiled image: one 32-row tile per wave");

template <int METRIC>
__global__ void __launch_bounds__(fThreads, fWaves / 4) filter_img2_kernel(FilterArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Img2Shared* sh = reinterpret_cast<Img2Shared*>(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  const int64_t q0 = (int64_t)blockIdx.y * fBQ;
  const int nch = (a.d + fBK - 1) / fBK;
  const int ksteps = (a.d + 15) / 16;
  const int64_t ntile32 = (a.n + 31) / 32;
#ifdef FX_DIAG_BUILD
  const int diag = a.diag;
#else
  constexpr int diag = 0;
#endif
  filter_query_table<METRIC>(a, q0, sh->qtab, sh->qab, tid, fThreads);
#if FX_I2_SEG > 0
  for (int q = tid; q < fBQ; q += fThreads) sh->seg[q] = 0u;  // (ordered by the tile barriers)
#endif

  FilterAddr ad;  // the query tile (as filter_tiles)
  {
    const uint16_t* qb = a.Qh + q0 * 32;
    const uint64_t qp = reinterpret_cast<uint64_t>(qb);
    const uint32_t qlo = __builtin_amdgcn_readfirstlane((uint32_t)qp);
    const uint32_t qhi = __builtin_amdgcn_readfirstlane((uint32_t)(qp >> 32));
    const int qnb = __builtin_amdgcn_readfirstlane(
        (int)(((int64_t)(a.dq / 32 - 1) * a.qstride + fBQ) * 64));
    ad.qr = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>(((uint64_t)qhi << 32) | qlo), 0, qnb, 0x00020000);
    ad.d = a.d;
    ad.xs = 0;
    ad.qs = (uint32_t)(fThreads / fQC) * 64u;
    ad.qb = (uint32_t)a.qstride * 64u;
    ad.dq = a.dq;
  }
  FilterOff o = {};
  {
    const unsigned t = opaque(tid);
    o.qg = (t / fQC) * 64 + (t % fQC) % 4 * 16 + (t % fQC) / 4 * ad.qb;
  }
  const uint32_t qw = ((tid / fQC) * fLds + (tid % fQC) * 8) * 2;  // this thread's Q stores
  const uint32_t qr = (l32 * fLds + 8 * h) * 2;                    // this lane's B fragments

  auto store_q = [&](const FilterPreQ& pq, auto buf) {
    constexpr int B = decltype(buf)::value;
#pragma unroll
    for (int i = 0; i < fQP; ++i)
      lds_at<i32x4>(smem, B * kQB + qw + i * (fThreads / fQC) * fLds * 2) = pq.q[i];
  };
  typedef f16x8 XA[kI2KS];
  int par = 0;
  for (int64_t ti = blockIdx.x; ti < a.num_tiles; ti += gridDim.x, par ^= 1) {
    const int64_t r0 = (a.tile_start + ti * a.tile_stride) * fBM;
    if (tid < kRowFlagWords) sh->rflags[par][tid] = 0u;
#ifndef FX_I2_RPF
#define FX_I2_RPF 1
#endif
    // this thread's row sum, loaded before the stream (not a dependent HBM
    // load between the last MFMA and the epilogue's barrier)
    float rsum = 0.f;
    if (FX_I2_RPF && tid < fBM && r0 + tid < a.n) rsum = a.rowinfo[r0 + tid];
    // this wave's 32-row tile: its k-steps, one KB each (a tile past the end
    // reads zeros through the descriptor size)
    __amdgpu_buffer_rsrc_t xr;
    {
      const int64_t t32 = r0 / 32 + wid;
      const int64_t live = t32 < ntile32 ? 1 : 0;
      const unsigned char* base = reinterpret_cast<const unsigned char*>(a.X) +
                                  (live ? t32 : 0) * (int64_t)ksteps * 1024;
      const uint64_t xp = reinterpret_cast<uint64_t>(base);
      const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)xp);
      const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(xp >> 32));
      const int nb = __builtin_amdgcn_readfirstlane((int)(live * ksteps * 1024));
      xr = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0,
                                             nb, 0x00020000);
    }
    const uint32_t xl = (uint32_t)opaque(lane) * 16u;
    auto load_x = [&](XA& xa, int c) {
#pragma unroll
      for (int s = 0; s < kI2KS; ++s) {
        const int ks = c * kI2KS + s;  // wave-uniform: past the row end reads zeros
        const uint32_t off = ks < ksteps ? xl : 0x7fff0000u;
        xa[s] = __builtin_bit_cast(
            f16x8, __builtin_amdgcn_raw_buffer_load_b128(xr, off, ks * 1024, 2 /* nt */));
      }
    };
    f32x16 acc[1][kI2QT];
#pragma unroll
    for (int u = 0; u < kI2QT; ++u) acc[0][u] = f32x16(0.f);
    auto compute = [&](const XA& xa, auto buf) {
      constexpr int B = decltype(buf)::value;
      if (diag & 4) {  // (diagnostics: no MFMA; the row loads stay live)
        if (xa[0][0] == (_Float16)1.2345f && xa[kI2KS - 1][7] == (_Float16)2.f) a.count[0] = 7;
        return;
      }
#pragma unroll
      for (int s = 0; s < kI2KS; ++s) {
#pragma unroll
        for (int u = 0; u < kI2QT; ++u) {
          const f16x8 bv = lds_at<f16x8>(smem, B * kQB + qr + (u * 32 * fLds + 16 * s) * 2);
          acc[0][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[s], bv, acc[0][u], 0, 0, 0);
        }
      }
    };
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    FilterPreQ pq;
    XA xa0, xa1;
    filter_load_q(pq, ad, o, 0, diag);
    load_x(xa0, 0);
    load_x(xa1, 1);
    store_q(pq, B0{});
    filter_load_q(pq, ad, o, 1, diag);
    __syncthreads();
    // step c: multiply chunk c (registers xa[c & 1], query buffer c & 1),
    // store query chunk c + 1, load query chunk c + 2 and rows chunk c + 2
    auto step = [&](int c, XA& xa, auto buf) {
      constexpr int B = decltype(buf)::value;
      compute(xa, buf);
      store_q(pq, std::integral_constant<int, B ^ 1>{});
      filter_load_q(pq, ad, o, c + 2, diag);
      load_x(xa, c + 2);
      __syncthreads();
    };
    int c = 0;
    for (; c + 2 < nch; c += 2) {
      step(c, xa0, B0{});
      step(c + 1, xa1, B1{});
    }
    const bool two = c + 1 < nch;
    if (two) store_q(pq, B1{});
    __syncthreads();
    compute(xa0, B0{});
    if (two) compute(xa1, B1{});

    if (tid < fBM) {  // one thread per row: bound factor, flags
      const int lr = tid;
      const int64_t row = r0 + lr;
      bool ok = row < a.n;
      const float s = ok ? (FX_I2_RPF ? rsum : a.rowinfo[row]) : 0.f;
      if (ok && a.mask != nullptr) ok = (a.mask[row >> 5] >> (row & 31)) & 1u;
      float rv;
      if constexpr (METRIC == 0) {
        rv = s;
      } else if constexpr (METRIC == 1) {
        rv = sqrtf(s);
      } else {
        rv = fmaxf(sqrtf(s), 1e-12f);
      }
      if (!(s <= 3.4e38f)) rv = __builtin_nanf("");
      filter_note_row<METRIC, 1>(sh->rinfo, sh->rterm, sh->rflags[par], lr, rv, ok);
    }
    __syncthreads();
    if (diag & 2) {
      if (acc[0][0][0] == 1.2345f) a.count[0] = 7;
      continue;
    }
#if FX_I2_SEG > 0
    filter_epilogue_seg<METRIC, kI2QT, 1, FX_I2_SEG>(acc, sh->rinfo, sh->rterm, sh->rflags[par],
                                                 sh->qtab, sh->qab, a, q0, r0, wid, 0, h, l32,
                                                 diag, sh->seg);
#else
    filter_epilogue<METRIC, kI2QT, 1>(acc, sh->rinfo, sh->rterm, sh->rflags[par], sh->qtab,
                                      sh->qab, a, q0, r0, wid, 0, h, l32, diag);
#endif
  }
#if FX_I2_SEG > 0
  filter_flush_segments<FX_I2_SEG>(sh->seg, sh->segbase, a, q0, tid);
#endif
}

static int launch_img2(const FilterArgs& a, int metric, hipStream_t stream) {
  const void* fn = metric == FX_METRIC_COS ? (const void*)filter_img2_kernel<2>
                   : metric == FX_METRIC_IP ? (const void*)filter_img2_kernel<1>
                                            : (const void*)filter_img2_kernel<0>;
  if (int rc = allow_lds(fn)) return rc;
  int cus = 0;
  if (int rc = device_cus(&cus)) return rc;
  int64_t bx = cus;
  if (bx > a.num_tiles) bx = a.num_tiles;
  return launch_query_tiles(fn, "filter_img2_kernel", a, fThreads, sizeof(Img2Shared), bx, fBQ, 4,
                            stream);
}
