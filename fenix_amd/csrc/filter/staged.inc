// The register-staged filter_kernel (after filter/tile.inc; the kernel's
// description heads knn_filter.hip): f32 or fp16 rows stream through registers
// into a double-buffered LDS tile, the query tile alongside.  Serves row-major
// corpora of either type, and in diagnostic builds row-major fp16 filter
// images (IMG).  A variant names the row types it instantiates as
// launch_staged's template argument.
#ifndef FX_FILTER_BPC
#define FX_FILTER_BPC 1     // workgroups per CU (LDS and registers permitting)
#endif
// Cross-tile prefetch (see filter_tiles): measured faster for the 64-query
// tiles (16 queries, 10M x 768 image: 2.73 -> 2.65 ms), slower for the
// 256-query ones (5.99 -> 6.1 ms BK 32, 6.35 ms BK 64: register pressure)
#ifndef FX_FILTER_XPF
#define FX_FILTER_XPF (FX_FILTER_BQ == 64)
#endif
constexpr bool kXpf = FX_FILTER_XPF;
// Rows of type XT (float or _Float16) come in 16-B pieces of E elements;
// C pieces per row per chunk (the lanes sharing a row), P per thread.
template <typename XT>
struct XPiece {
  static constexpr int E = 16 / (int)sizeof(XT);
  static constexpr int C = fBK / E;
  static constexpr int P = fBM * C / fThreads;
  static_assert(P >= 1 && fThreads % C == 0, "row staging");
};
static_assert(fBQ * fQC / fThreads >= 1 && fBK % 16 == 0,
              "filter_kernel: at least one query piece per thread and chunk");
struct FilterShared {
  _Float16 xs[2][fBM * fLds];
  _Float16 qs[2][fBQ * fLds];
  float rinfo[fBM];  // per-row bound factor (see the epilogue)
  float rterm[fBM];  // cosine: 1 / rinfo (the appends' bound term)
  uint32_t rflags[2][kRowFlagWords];
  f32x4 qtab[fBQ];   // per query: the bound's constants {c1, c0, A, B}
  float2 qab[fBQ];   // per query: pass iff product >= a * row value + b
};
constexpr uint32_t kXB = sizeof(_Float16) * fBM * fLds;  // one LDS X buffer, bytes (kQB: Q)
constexpr uint32_t kQOff = 2 * kXB;                      // FilterShared::qs
static_assert(__builtin_offsetof(FilterShared, qs) == kQOff, "LDS layout");

template <typename XT>
struct FilterPre {  // one K chunk of X rows in flight
  i32x4 x[XPiece<XT>::P];
};

template <typename XT>
__device__ __forceinline__ FilterOff filter_offsets(unsigned t, const FilterAddr& ad) {
  using X = XPiece<XT>;
  FilterOff o;
  o.kc = (int)(t % X::C) * X::E;
  o.xg = ((t / X::C) * (unsigned)ad.d + (t % X::C) * X::E) * (unsigned)sizeof(XT);
  // query piece p = t % fQC of a chunk: block p / 4, 16 B p % 4 of the query's 64
  o.qg = (t / fQC) * 64 + (t % fQC) % 4 * 16 + (t % fQC) / 4 * ad.qb;
  o.xw = ((t / X::C) * fLds + (t % X::C) * X::E) * 2;
  o.qw = kQOff + ((t / fQC) * fLds + (t % fQC) * 8) * 2;
  const unsigned lane = t & 63, wid = t >> 6;
  const unsigned rg = wid % fRG, qg = wid / fRG, h = lane >> 5, l32 = lane & 31;
  o.xr = ((rg * 64 + l32) * fLds + 8 * h) * 2;
  o.qr = kQOff + ((qg * fQT * 32 + l32) * fLds + 8 * h) * 2;
  return o;
}

template <typename XT>
__device__ __forceinline__ void filter_load(FilterPre<XT>& p, const FilterAddr& ad,
                                            const FilterOff& o, int c) {
  const int k0 = c * fBK;
  // past the row end: an offset beyond the buffer (reads zeros)
  const uint32_t base = k0 + o.kc < ad.d ? o.xg : 0x7fff0000u;
#pragma unroll
  for (int i = 0; i < XPiece<XT>::P; ++i)
    p.x[i] = __builtin_bit_cast(
        i32x4, __builtin_amdgcn_raw_buffer_load_b128(ad.xr, base + i * ad.xs,
                                                     k0 * (int)sizeof(XT), 2 /* nt */));
}

// Stage one chunk into LDS buffer BUF: f32 rows to fp16 (with their sums of
// squares, as float pairs so the packed fma reads the loaded registers
// directly, and the max |x| for the fp16-overflow test), fp16 rows as they
// are (sums of squares of the exact f32 values; an fp16 row cannot overflow,
// an infinity or NaN shows in the sum), the query pieces as they are.
// IMG: the rows are the fp16 filter image of an f32 corpus (fx_filter_image);
// their row values come from FilterArgs::rowinfo instead.
template <typename XT, int BUF, bool IMG>
__device__ __forceinline__ void filter_store(const FilterPre<XT>& p, const FilterPreQ& pq,
                                             unsigned char* smem, const FilterOff& o,
                                             f32x2 (&sq)[XPiece<XT>::P],
                                             float (&mx)[XPiece<XT>::P]) {
  using X = XPiece<XT>;
#pragma unroll
  for (int i = 0; i < X::P; ++i) {
    const uint32_t at = o.xw + BUF * kXB + i * (fThreads / X::C) * fLds * 2;
    if constexpr (sizeof(XT) == 4) {
      const f32x4 v = __builtin_bit_cast(f32x4, p.x[i]);
      lds_at<f16x4>(smem, at) = __builtin_convertvector(v, f16x4);
      const f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
      sq[i] = __builtin_elementwise_fma(lo, lo, sq[i]);
      sq[i] = __builtin_elementwise_fma(hi, hi, sq[i]);
      mx[i] = fmaxf(mx[i],
                    fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    } else {
      lds_at<i32x4>(smem, at) = p.x[i];
      if constexpr (!IMG) {
        const f16x8 h = __builtin_bit_cast(f16x8, p.x[i]);
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const f32x2 v = {(float)h[e], (float)h[e + 1]};
          sq[i] = __builtin_elementwise_fma(v, v, sq[i]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < fQP; ++i)
    lds_at<i32x4>(smem, o.qw + BUF * kQB + i * (fThreads / fQC) * fLds * 2) = pq.q[i];
}

template <int BUF>
__device__ __forceinline__ void filter_compute(f32x16 (&acc)[2][fQT], unsigned char* smem,
                                               const FilterOff& o) {
#pragma unroll
  for (int s = 0; s < fBK / 16; ++s) {
    f16x8 av[2], bv[fQT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
      av[t] = lds_at<f16x8>(smem, o.xr + BUF * kXB + (t * 32 * fLds + 16 * s) * 2);
#pragma unroll
    for (int u = 0; u < fQT; ++u)
      bv[u] = lds_at<f16x8>(smem, o.qr + BUF * kQB + (u * 32 * fLds + 16 * s) * 2);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < fQT; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[t], bv[u], acc[t][u], 0, 0, 0);
  }
}

// The tile loop of filter_kernel.  Every wave multiplies chunk c, then stores
// chunk c + 1 and issues its loads (half of the workgroup taking the other
// order, so that SIMD partners alternate, measured slower: DESIGN.md
// Appendix A).
template <typename XT, int METRIC, bool IMG, typename Diag>
__device__ __forceinline__ void filter_tiles(const FilterArgs& a, unsigned char* smem, int tid,
                                             Diag diag) {
  using X = XPiece<XT>;
  FilterShared* sh = reinterpret_cast<FilterShared*>(smem);
  const int lane = tid & 63, wid = tid >> 6;
  const int rg = wid % fRG, qg = wid / fRG;  // 64-row group, fQT*32-query group
  const int h = lane >> 5, l32 = lane & 31;
  const int64_t q0 = (int64_t)blockIdx.y * fBQ;
  const int nch = (a.d + fBK - 1) / fBK;

  // the buffer descriptor of the X rows of the tile at row r0 (rows past n,
  // or a tile past the end, read as zeros)
  auto x_rsrc = [&](int64_t r0) {
    int64_t rows = a.n - r0 < fBM ? a.n - r0 : fBM;
    if (rows < 0) rows = 0;
    const XT* xb = reinterpret_cast<const XT*>(a.X) + (rows > 0 ? r0 : 0) * (int64_t)a.d;
    const uint64_t xp = reinterpret_cast<uint64_t>(xb);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)xp);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(xp >> 32));
    const int nb = __builtin_amdgcn_readfirstlane((int)(rows * a.d * (int64_t)sizeof(XT)));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0,
                                             nb, 0x00020000);
  };
  auto tile_r0 = [&](int64_t ti) { return (a.tile_start + ti * a.tile_stride) * fBM; };
  FilterAddr ad;
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
    ad.xs = (uint32_t)(fThreads / X::C) * (uint32_t)a.d * (uint32_t)sizeof(XT);
    ad.qs = (uint32_t)(fThreads / fQC) * 64u;
    ad.qb = (uint32_t)a.qstride * 64u;
    ad.dq = a.dq;
  }

  // Two register stages: chunks c + 2 and c + 3 of X are in flight while
  // chunk c is multiplied (stage j % 2 holds chunk j), the query tile one
  // chunk ahead.  Loads are issued unconditionally (chunks past the row end
  // read as zeros through the descriptor bounds): a load under a branch
  // makes the compiler wait for it where the branch joins.  With kXpf a
  // tile's first two X chunks and first query chunk are issued before the
  // previous tile's epilogue (the stages are free by then), so they stream
  // in while it runs.
  FilterPre<XT> pf[2];
  FilterPreQ pq;
  int64_t ti = blockIdx.x;
  if constexpr (kXpf) {
    ad.xr = x_rsrc(tile_r0(ti));
    const FilterOff o = filter_offsets<XT>(opaque(tid), ad);
    filter_load_q(pq, ad, o, 0, diag);
    filter_load(pf[0], ad, o, 0);
    filter_load(pf[1], ad, o, 1);
  }
  int par = 0;  // tile parity: which rflags words this tile's epilogue reads
  for (; ti < a.num_tiles; ti += gridDim.x, par ^= 1) {
    const int64_t r0 = tile_r0(ti);
    // (last read by the epilogue two tiles back: every wave has passed the
    // previous tile's barriers since)
    if (tid < kRowFlagWords) sh->rflags[par][tid] = 0u;

    f32x16 acc[2][fQT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < fQT; ++u) acc[t][u] = f32x16(0.f);
    f32x2 sq[X::P];
    float mx[X::P];
#pragma unroll
    for (int i = 0; i < X::P; ++i) {
      sq[i] = f32x2(0.f);
      mx[i] = 0.f;
    }

    ad.xr = x_rsrc(r0);
    const FilterOff o = filter_offsets<XT>(opaque(tid), ad);
    if constexpr (!kXpf) {
      filter_load_q(pq, ad, o, 0, diag);
      filter_load(pf[0], ad, o, 0);
      filter_load(pf[1], ad, o, 1);
    }
    filter_store<XT, 0, IMG>(pf[0], pq, smem, o, sq, mx);
    // Q one chunk ahead, issued before the X load of the same step: vmcnt
    // retires loads in issue order, so waiting for Q(c + 1) at step c waits
    // for X(c + 1) (needed there anyway) and nothing issued later.
    filter_load_q(pq, ad, o, 1, diag);
    filter_load(pf[0], ad, o, 2);
    __syncthreads();
    // One K step: multiply chunk c (LDS buffer c & 1 = B), store chunk c + 1
    // from its stage p into the other buffer, refill p with chunk c + 3.  The
    // main loop runs only full steps, with no branch inside (a conditional
    // store or load makes the waitcnt pass merge pending-load states at the
    // join and wait for every load in flight, draining the stream).
    auto step = [&](int c, FilterPre<XT>& p, auto buf) {
      constexpr int B = decltype(buf)::value;
      if (!(diag & 4)) filter_compute<B>(acc, smem, o);
      if (!(diag & 16)) filter_store<XT, B ^ 1, IMG>(p, pq, smem, o, sq, mx);
      filter_load_q(pq, ad, o, c + 2, diag);
      filter_load(p, ad, o, c + 3);
      __syncthreads();
    };
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    int c = 0;
    for (; c + 2 < nch; c += 2) {
      step(c, pf[1], B0{});
      step(c + 1, pf[0], B1{});
    }
    // the last one or two chunks (c is even: chunk c sits in buffer 0, chunk
    // c + 1, if any, in stage 1); one-sided branches only, so the
    // accumulators need no copies at a join
    const bool two = c + 1 < nch;
    if (two && !(diag & 16)) filter_store<XT, 1, IMG>(pf[1], pq, smem, o, sq, mx);
    __syncthreads();
    // kXpf: the rows' image sums and mask words for the epilogue, issued
    // before the last chunks' MFMAs and the next tile's loads, so they are in
    // when it starts without waiting for those
    float img_sq[X::P];
    uint32_t mword[X::P];
    if constexpr (kXpf) {
#pragma unroll
      for (int i = 0; i < X::P; ++i) {
        const int lr = (i * fThreads + tid) / X::C;
        const int64_t row = r0 + lr < a.n ? r0 + lr : a.n - 1;
        if constexpr (IMG) img_sq[i] = a.rowinfo[row];
        mword[i] = a.mask != nullptr ? a.mask[row >> 5] : ~0u;
      }
    }
    if (!(diag & 4)) filter_compute<0>(acc, smem, o);
    if (two && !(diag & 4)) filter_compute<1>(acc, smem, o);
    if constexpr (kXpf) {  // the next tile's first chunks (past the end: an empty descriptor)
      const int64_t tn = ti + gridDim.x;
      ad.xr = x_rsrc(tn < a.num_tiles ? tile_r0(tn) : a.n);
      const FilterOff on = filter_offsets<XT>(opaque(tid), ad);
      filter_load_q(pq, ad, on, 0, diag);
      filter_load(pf[0], ad, on, 0);
      filter_load(pf[1], ad, on, 1);
    }

    // per-row value rv from |x|^2 (the fRowLanes lanes of a row hold partials;
    // IMG: the f32 row's, precomputed): cosine max(|x|, 1e-12), IP |x|, L2
    // |x|^2; NaN = forced through (fp16 overflow: a component >= 65520;
    // non-finite); -1 = skipped (past n or masked out)
    float sqs[X::P];
#pragma unroll
    for (int i = 0; i < X::P; ++i) {
      sqs[i] = sq[i][0] + sq[i][1];
      if constexpr (!IMG) {
#pragma unroll
        for (int m = 1; m < X::C; m <<= 1) {
          sqs[i] += __shfl_xor(sqs[i], m);
          mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], m));
        }
      }
    }
#pragma unroll
    for (int i = 0; i < X::P; ++i) {
      if (tid % X::C == 0) {
        const int lr = (i * fThreads + tid) / X::C;
        const int64_t row = r0 + lr;
        bool ok = row < a.n;
        if constexpr (kXpf) {
          if constexpr (IMG) sqs[i] = ok ? img_sq[i] : 0.f;
          if (ok) ok = (mword[i] >> (row & 31)) & 1u;
        } else {
          if constexpr (IMG) sqs[i] = ok ? a.rowinfo[row] : 0.f;
          if (ok && a.mask != nullptr) ok = (a.mask[row >> 5] >> (row & 31)) & 1u;
        }
        float rv;
        if constexpr (METRIC == 0) {
          rv = sqs[i];
        } else if constexpr (METRIC == 1) {
          rv = sqrtf(sqs[i]);
        } else {
          rv = fmaxf(sqrtf(sqs[i]), 1e-12f);
        }
        if (!(sqs[i] <= 3.4e38f) || mx[i] >= 65520.f) rv = __builtin_nanf("");
        filter_note_row<METRIC>(sh->rinfo, sh->rterm, sh->rflags[par], lr, rv, ok);
      }
    }
    __syncthreads();

    // ---- epilogue: [lb, ub] per (row, query), threshold test, append
    if (diag & 2) {
      if (acc[0][0][0] == 1.2345f && acc[1][fQT - 1][5] == 2.f) a.count[0] = 7;
      continue;
    }

    filter_epilogue<METRIC, fQT>(acc, sh->rinfo, sh->rterm, sh->rflags[par], sh->qtab, sh->qab, a,
                                 q0, r0, rg, qg, h, l32, diag);
  }
}

template <typename XT, int METRIC, bool IMG>
__global__ void __launch_bounds__(fThreads, fWaves * FX_FILTER_BPC / 4) filter_kernel(FilterArgs a) {
  static_assert(!IMG || sizeof(XT) == 2, "the filter image is fp16");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  FilterShared* sh = reinterpret_cast<FilterShared*>(smem);
  const int tid = threadIdx.x;
  filter_query_table<METRIC>(a, (int64_t)blockIdx.y * fBQ, sh->qtab, sh->qab, tid, fThreads);
  // (the first tile's barriers order these writes before the epilogue reads)
#ifdef FX_DIAG_BUILD
  const int diag = a.diag;
#else
  constexpr int diag = 0;
#endif
  filter_tiles<XT, METRIC, IMG>(a, smem, tid, diag);
}

template <typename XT, bool IMG>
static const void* staged_fn(int metric) {
  return metric == FX_METRIC_COS  ? (const void*)filter_kernel<XT, 2, IMG>
         : metric == FX_METRIC_IP ? (const void*)filter_kernel<XT, 1, IMG>
                                  : (const void*)filter_kernel<XT, 0, IMG>;
}

// ROWS: the row types the variant instantiates (kRowsF32 | kRowsF16; fp16
// includes, in diagnostic builds, row-major filter images, rejected: the
// tiled image is 7-10 % faster)
constexpr int kRowsF32 = 1, kRowsF16 = 2;
template <int ROWS>
static int launch_staged(const FilterArgs& a, int metric, hipStream_t stream) {
  const bool f16 = a.dtype == FX_DTYPE_F16;
  const void* fn = nullptr;
  if (a.rowinfo != nullptr) {
#ifdef FX_DIAG_BUILD
    if constexpr ((ROWS & kRowsF16) != 0)
      if (f16) fn = staged_fn<_Float16, true>(metric);
#endif
  } else if (f16) {
    if constexpr ((ROWS & kRowsF16) != 0) fn = staged_fn<_Float16, false>(metric);
  } else {
    if constexpr ((ROWS & kRowsF32) != 0) fn = staged_fn<float, false>(metric);
  }
  if (fn == nullptr) {
    set_error("filter: row type not compiled into this variant");
    return FX_EUNSUPPORTED;
  }
  if (int rc = allow_lds(fn)) return rc;
  int cus = 0;
  if (int rc = device_cus(&cus)) return rc;
  int64_t bx = (int64_t)cus * FX_FILTER_BPC;
  if (bx > a.num_tiles) bx = a.num_tiles;
  return launch_query_tiles(fn, "filter_kernel", a, fThreads, sizeof(FilterShared), bx, fBQ, 4,
                            stream);
}
