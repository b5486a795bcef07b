// filter_img6_kernel: int8 image, a resident query slice (after
// filter/tile.inc and filter/tiled.inc; slices of at most 128 queries).
//
// filter_img3_kernel streams the query tile through an LDS ring: every
// 64-component chunk of every 256-row tile DMAs the tile's queries again
// (as many bytes per chunk as the image itself) behind a workgroup barrier,
// so the 8 waves run in lockstep and the MFMAs add to the image stream
// instead of hiding under it (DESIGN.md 3.6b).  Here a workgroup holds its
// slice of 128 queries (the q128 build; 64 in q64i) in LDS for the whole
// kernel (96 KB at 768-d, XOR-swizzled for conflict-free ds_read_b128) and
// each of its waves runs its own 32-row tiles with FX_I6_XS image k-steps in
// flight in registers across tile ends, its own rows' terms and flags in
// LDS, and the same epilogue (i8_epilogue: pass test, bounds, LDS append
// segments shared through LDS atomics); the only barrier of the tile loop
// is the one before the epilogue (see there).  Default for batches of up to
// 128 queries (launch_filter).  With option img6 = 2 a larger batch runs its
// slices on different CUs over the same tiles at the same time --
// workgroup (x, y) takes slice y and tiles x, x + G, ... with G = CUs /
// slices, so the partners share an XCD (x + G y = x mod 8) and the second
// read of a tile can come from its L2 or the Infinity Cache; measured slower
// than filter_img3_kernel's 256-query tiles (3.34 vs 2.97 ms), so off.
#ifndef FX_I6_XS
#define FX_I6_XS 8
#endif
constexpr int kI6Waves = 8;
constexpr int kI6Threads = 64 * kI6Waves;
constexpr int kI6BM = 32 * kI6Waves;
static_assert(kI6BM == fBM, "one plan tile per workgroup tile");
static_assert(fBQ <= 128, "filter_img6_kernel: the resident slice holds at most 128 queries");
constexpr int kI6SEG = FX_I3_SEG;
constexpr int kI6SliceBatch = 12;  // 768-d, 128 queries: every piece of the slice in one batch
struct Img6Shared {
  float rinfo[kI6BM];
  float rterm[kI6BM];
  float rext[kI6BM];
  uint32_t rrow[kI6BM];
  uint32_t rflags[kRowFlagWords];
  f32x4 qtab[fBQ];
  f32x4 qinf[fBQ];
  uint32_t seg[fBQ + 3 * fBQ * kI6SEG];
  uint32_t segbase[fBQ];
};
// The QMASK build (per-query row masks, FilterArgs::qmask): each row's slice
// of query bits beside its terms, fBQ / 32 words per row
constexpr int kI6QW = fBQ / 32;
typedef uint32_t i6_qbits __attribute__((ext_vector_type(kI6QW)));
struct Img6SharedQ : Img6Shared {
  i6_qbits rqmask[kI6BM];
};
// the query slice follows: (dq / 64) chunks x 128 queries x 64 B
static size_t img6_smem(int dq, bool qmask = false) {
  return (qmask ? sizeof(Img6SharedQ) : sizeof(Img6Shared)) + (size_t)(dq / 64) * fBQ * 64;
}
bool img6_fits(int dq) { return img6_smem(dq) <= 160 * 1024; }
bool img6_fits_qmask(int dq) { return img6_smem(dq, true) <= 160 * 1024; }

// QMASK: a (row, query) pair is appended only where bit q of the row's words
// a.qmask[crow * a.qmask_words ..] is set (fx_qmask_pack's matrix, indexed by
// CORPUS row like a.mask); a row no query of the slice admits is skipped like
// a row the shared mask excludes.
template <int METRIC, bool QMASK = false>
__global__ void __launch_bounds__(kI6Threads, 1) filter_img6_kernel(FilterArgs a) {
  constexpr int XS = FX_I6_XS, SEG = kI6SEG;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Shared = std::conditional_t<QMASK, Img6SharedQ, Img6Shared>;
  Shared* sh = reinterpret_cast<Shared*>(smem);
  unsigned char* qslice = smem + sizeof(Shared);
#ifdef FX_DIAG_BUILD
  const int diag = a.diag;
#else
  constexpr int diag = 0;
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  const int64_t q0 = (int64_t)blockIdx.y * fBQ;
  const int ksteps = (a.d + 31) / 32;
  const int nks = (ksteps + XS - 1) / XS * XS;  // (past the row end the image reads zeros)
  const int ngroups = nks / XS;
  const int64_t ntile32 = (a.n + 31) / 32;
  const int64_t ntiles = a.num_tiles;
  if ((int64_t)blockIdx.x >= ntiles) return;
  if (a.skip_full) {  // every query of the slice predicted to overflow (the gate): the
                      // exact scan recomputes them, so the final pass has nothing to do
    bool full = true;
    for (int q = tid; q < fBQ; q += kI6Threads)
      if (q0 + q < a.nq && a.count[(q0 + q) * kCountStride] <= (uint32_t)a.cap) full = false;
    if (__syncthreads_and(full)) return;
  }
  i8_query_table<METRIC>(a, q0, sh->qtab, sh->qinf, tid, kI6Threads);
  for (int q = tid; q < fBQ; q += kI6Threads) sh->seg[q] = 0u;
  // the slice's live queries share all fBQ * SEG segment entries (one query:
  // 1 536 instead of 24, so a k = 1 000 search's ~200 appends per workgroup
  // and phase stay in LDS instead of each lane taking a slot from the one
  // global counter of the query: F1 429 us at 6.25M x 1536)
  const int64_t nlive = a.nq - q0 < fBQ ? a.nq - q0 : fBQ;
  const int segcap = (fBQ * SEG) / (int)(nlive > 0 ? nlive : 1);
  {  // the slice: chunk c of query Q at (c * 128 + Q) * 64, piece p at (p ^ ((Q >> 2) & 3)) * 16
    // (kI6SliceBatch loads in flight per thread before their stores: one
    // load, wait, store per iteration cost ~1.5 us each, ~18 us per launch)
    const int total = a.dq / 64 * fBQ * 4;
    const unsigned char* qb = reinterpret_cast<const unsigned char*>(a.Qh);
    for (int i0 = tid; i0 < total; i0 += kI6SliceBatch * kI6Threads) {
      i32x4 v[kI6SliceBatch];
#pragma unroll
      for (int j = 0; j < kI6SliceBatch; ++j) {
        const int i = i0 + j * kI6Threads;
        const int c = i / (fBQ * 4), Q = (i / 4) % fBQ, pc = i % 4;
        if (i < total)
          v[j] = *reinterpret_cast<const i32x4*>(qb + ((int64_t)c * a.qstride + q0 + Q) * 64 +
                                                 pc * 16);
      }
#pragma unroll
      for (int j = 0; j < kI6SliceBatch; ++j) {
        const int i = i0 + j * kI6Threads;
        const int c = i / (fBQ * 4), Q = (i / 4) % fBQ, pc = i % 4;
        if (i < total)
          *reinterpret_cast<i32x4*>(qslice + ((c * fBQ + Q) * 64 + ((pc ^ ((Q >> 2) & 3)) * 16))) =
              v[j];
      }
    }
  }
  __syncthreads();
  // B fragment of query tile u at k-step ks: query Q = 32 u + l32, piece
  // 2 (ks & 1) + h of chunk ks / 2 (bits 2-3 of Q do not depend on u)
  const int bsw = (l32 >> 2) & 3;
  auto bfrag = [&](int ks, int u) {
    const int Q = 32 * u + l32;
    return *reinterpret_cast<const f16x8*>(
        qslice + ((ks >> 1) * fBQ + Q) * 64 + (((2 * (ks & 1) + h) ^ bsw) * 16));
  };
  auto tile_r0 = [&](int64_t ti) { return (a.tile_start + ti * a.tile_stride) * fBM; };
  auto x_rsrc = [&](int64_t ti) {
    const int64_t t32 = tile_r0(ti) / 32 + wid;
    const int64_t live = (ti < ntiles && t32 < ntile32) ? 1 : 0;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(a.X) +
                                (live ? t32 : 0) * (int64_t)ksteps * 1024;
    const uint64_t xp = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)xp);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(xp >> 32));
    const int nb = __builtin_amdgcn_readfirstlane((int)(live * ksteps * 1024));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0,
                                             nb, 0x00020000);
  };
  const uint32_t xl = (uint32_t)opaque(lane) * 16u;
  auto load_a = [&](__amdgpu_buffer_rsrc_t xr, int ks) {
    const uint32_t off = ks < ksteps ? xl : 0x7fff0000u;
    return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(xr, off, ks * 1024, 2));
  };
  f32x16 acc[kI2QT];
  const f32x16 acc0 = f32x16(kI8Magic);
  auto mfma = [&](int u, const f16x8& xv, const f16x8& bv, bool start) {
    typedef int i32x16 __attribute__((ext_vector_type(16)));
    const f32x16 cin = start ? acc0 : acc[u];
    acc[u] = __builtin_bit_cast(f32x16, __builtin_amdgcn_mfma_i32_32x32x32_i8(
        __builtin_bit_cast(i32x4, xv), __builtin_bit_cast(i32x4, bv),
        __builtin_bit_cast(i32x16, cin), 0, 0, 0));
  };
  // one k-step: its B fragments first (one LDS wait), then the MFMAs.  The
  // previous k-step's fragments stay allocated until this k-step's reads are
  // issued, so the new fragments never land in registers an MFMA issued just
  // ahead (and possibly still queued behind the partner wave's MFMAs) reads.
  // Defensive only: the measured hazard was the epilogue's (below); without
  // this (FX_I6_BPREV=0) 0 of 88 repetitions moved and the times were equal
  // (profiles/r04_img6_bprev_sweep.jsonl)
#ifndef FX_I6_BPREV
#define FX_I6_BPREV 1
#endif
  f16x8 bprev[kI2QT];
#pragma unroll
  for (int u = 0; u < kI2QT; ++u) bprev[u] = f16x8(0);
  auto kstep = [&](const f16x8& xv, int ks, bool start) {
    f16x8 bv[kI2QT];
#pragma unroll
    for (int u = 0; u < kI2QT; ++u) bv[u] = bfrag(ks, u);
    if constexpr (FX_I6_BPREV != 0) {
#pragma unroll
      for (int u = 0; u < kI2QT; ++u) asm volatile("" ::"v"(bprev[u]));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kI2QT; ++u) mfma(u, xv, bv[u], start);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kI2QT; ++u) bprev[u] = bv[u];
  };
  const int lr = wid * 32 + l32;  // the wave's row this lane notes (lanes 0-31)
  int64_t ti = blockIdx.x;
  __amdgpu_buffer_rsrc_t xr = x_rsrc(ti);
  f16x8 xa[XS];
#pragma unroll
  for (int s = 0; s < XS; ++s) xa[s] = load_a(xr, s);
  for (; ti < ntiles; ti += gridDim.x) {
    const int64_t r0 = tile_r0(ti);
    const int64_t tn = ti + gridDim.x;
    const __amdgpu_buffer_rsrc_t xn = x_rsrc(tn);
    // this tile's row terms, early (lanes 0-31: row r0 + wid * 32 + l32)
    const int64_t row = r0 + lr;
    const int64_t rowc = row < a.n ? row : a.n - 1;
    const f32x4 rsum = *reinterpret_cast<const f32x4*>(a.rowinfo + rowc * kI8RowInfo);
    const uint32_t crow = perm_row(a.perm_a, a.n, rowc);
    const uint32_t mword = a.mask != nullptr ? a.mask[crow >> 5] >> (crow & 31) : 1u;
    i6_qbits qm = i6_qbits(0u);  // the row's query bits of this slice (crow < n: in bounds)
    if constexpr (QMASK)
      qm = *reinterpret_cast<const i6_qbits*>(a.qmask + (int64_t)crow * a.qmask_words +
                                              (int64_t)blockIdx.y * kI6QW);
    // k-step groups of XS: the first starts the accumulators, the last
    // refills from the next tile
    for (int g = 0; g < ngroups; ++g) {
      const bool last = g + 1 == ngroups;
#pragma unroll
      for (int s = 0; s < XS; ++s) {
        const int ks = g * XS + s;
        kstep(xa[s], ks, ks == 0);
        xa[s] = last ? load_a(xn, s) : load_a(xr, ks + XS);
      }
    }
    // the wave's 32 rows: terms, corpus rows and flags into its own LDS words
    if (lane < 4) sh->rflags[(lane >> 1) * 16 + wid * 2 + (lane & 1)] = 0u;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (h == 0) {
      bool ok = row < a.n && (mword & 1u);
      if constexpr (QMASK) {
        uint32_t anyq = 0u;
#pragma unroll
        for (int u = 0; u < kI6QW; ++u) anyq |= qm[u];
        ok = ok && anyq != 0u;
        sh->rqmask[lr] = qm;
      }
      const float y1 = METRIC == 1 ? rsum[1] : METRIC == 2 ? rsum[2] : rsum[3];
      i8_note_row(sh->rinfo, sh->rterm, sh->rext, sh->rflags, lr, rsum[0], y1, rsum[1], ok);
      sh->rrow[lr] = (uint32_t)a.row_base + crow;
    }
    // Every wave of the workgroup past its last MFMA before any epilogue
    // reads its accumulators.  Without this barrier the waves ran free and
    // the epilogue now and then read a product of the tile's last k-step
    // before the MFMA had written it: the same search repeated appended one
    // more or one fewer row for query lanes 16-31 of a tile (no padding of
    // s_nop after the MFMAs removed it, so the MFMA was still queued behind
    // the partner wave's on the SIMD's matrix pipe).  tools/race_check.py:
    // 0 of 88 repetitions move with it, 201 of 232 without; it costs
    // nothing on a single query (1.295 vs 1.300 ms for configs[1]).
#ifndef FX_I6_PRE_EPI  // experiment switch (tools/race_check.py builds, DESIGN.md §3.6e):
#define FX_I6_PRE_EPI 1  // 0 no barrier, 1 barrier, 2 own loads drained, 3 64 wait states
#endif
    if constexpr (FX_I6_PRE_EPI == 1)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else if constexpr (FX_I6_PRE_EPI == 2)
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    else if constexpr (FX_I6_PRE_EPI == 3)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" :::
                   "memory");
    else
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (!(diag & 2)) {
      if constexpr (QMASK)
        i8_epilogue<METRIC, true>(acc, sh->rinfo, sh->rterm, sh->rext, sh->rrow, sh->rflags,
                                  sh->qtab, sh->qinf, a, q0, wid, h, l32, sh->seg, diag, segcap,
                                  reinterpret_cast<const uint32_t*>(sh->rqmask));
      else
        i8_epilogue<METRIC>(acc, sh->rinfo, sh->rterm, sh->rext, sh->rrow, sh->rflags, sh->qtab,
                            sh->qinf, a, q0, wid, h, l32, sh->seg, diag, segcap);
    }
    xr = xn;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  filter_flush_segments<SEG, kI6Threads>(sh->seg, sh->segbase, a, q0, tid, segcap);
}

int launch_img6(const FilterArgs& a, int metric, hipStream_t stream) {
  if (a.num_tiles <= 0) return FX_OK;
  const bool qm = a.qmask != nullptr;
  if (qm && (a.qmask_words < (a.nq + fBQ - 1) / fBQ * kI6QW || a.qmask_words % 4 != 0)) {
    set_error("filter_img6_kernel: %lld qmask words for %lld queries", (long long)a.qmask_words,
              (long long)a.nq);
    return FX_EINVAL;
  }
  const void* fn =
      qm ? (metric == FX_METRIC_COS  ? (const void*)filter_img6_kernel<2, true>
            : metric == FX_METRIC_IP ? (const void*)filter_img6_kernel<1, true>
                                     : (const void*)filter_img6_kernel<0, true>)
         : (metric == FX_METRIC_COS  ? (const void*)filter_img6_kernel<2>
            : metric == FX_METRIC_IP ? (const void*)filter_img6_kernel<1>
                                     : (const void*)filter_img6_kernel<0>);
  if (int rc = allow_lds(fn)) return rc;
  int cus = 0;
  if (int rc = device_cus(&cus)) return rc;
  const int64_t slices = (a.nq + fBQ - 1) / fBQ;
  // every slice's workgroups co-resident (one per CU): slices x G <= CUs
  int64_t bx = cus / (slices < cus ? slices : cus);
  if (bx < 1) bx = 1;
  if (bx > a.num_tiles) bx = a.num_tiles;
  return launch_query_tiles(fn, "filter_img6_kernel", a, kI6Threads, img6_smem(a.dq, qm), bx, fBQ,
                            kI8QInfo, stream);
}

