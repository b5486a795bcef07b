// Tiled filter images, fp16 or int8, the query tile by LDS-DMA ring (after
// filter/tile.inc and filter/tiled.inc).
//
// filter_img3_kernel:filter_img2_kernel's tiling (8 waves, wave w owns the
// 32-row tile w of a 256-row tile against all 256 queries, A fragments
// straight from the tiled image into registers) with the query tile moved by
// LDS-DMA (buffer_load ... lds) instead of through registers and ds_write:
//   * the K chunks of the query tile are the same for every row tile, so the
//     chunk sequence runs on across tiles in one ring of FX_I3_QA + 1 slots,
//     FX_I3_QA chunks in flight, one raw s_barrier per chunk behind a counted
//     vmcnt (cdna_hip_programming.md: pipelining across barriers);
//   * 16-B pieces XOR-swizzled by query ((q >> 2) & 3) on the global side:
//     the B-fragment ds_read_b128 are conflict-free without row padding;
//   * the image stream runs on across tiles too: FX_I3_XS register stages,
//     the next tile's first chunks issued as the current tile's last ones
//     are multiplied, so they stream in during its epilogue;
//   * the rows' image sums (and mask words) are loaded at the tile's first
//     chunk, every thread the same count (counted waits stay exact);
//   * appends go to per-query LDS segments (no returning global atomic,
//     which would wait for the prefetched stream: vmcnt retires in order),
//     flushed at the end;
//   * the pass test is packed: per pair of rows one v_pk_fma_f32 gives
//     RN(x - a rv) and one v_pk_add_f32 subtracts b; the sign collects the
//     fail bit (2 instructions per (row, query) instead of 3).
#ifndef FX_I3_QA
#define FX_I3_QA 3   // query chunks in flight (ring of FX_I3_QA + 1 slots)
#endif
#ifndef FX_I3_XS
#define FX_I3_XS 4   // image chunks in flight per wave (register stages; 2 and 3
                     // measured 1-2 % slower, tools/ab_i8x.sh)
#endif
#ifndef FX_I3_BPF
#define FX_I3_BPF 1   // B-fragment reads of a k-step ahead of its MFMAs (see compute)
#endif
#ifndef FX_I3_XPF
#define FX_I3_XPF 0   // 1: the next tile's first image chunks in flight during the
                      // epilogue (equal with 4 stages, 1-2 % faster with 2)
#endif
#ifndef FX_I3_PAIR
#define FX_I3_PAIR 1  // 1: the ring refilled two chunks at a time, one barrier per
                      // two steps (the ring then holds two pairs; FX_I3_QA unused)
#endif
#ifndef FX_I3_WAVES
#define FX_I3_WAVES 8  // waves per workgroup: 8 (one 256-row workgroup per CU) or 4
                       // (two independent 128-row workgroups per CU)
#endif
constexpr int kI3Waves = FX_I3_WAVES;
constexpr int kI3Threads = 64 * kI3Waves;
constexpr int kI3BM = 32 * kI3Waves;    // rows per workgroup tile (one 32-row tile per wave)
constexpr int kI3Sub = fBM / kI3BM;     // workgroup tiles per fBM-row tile of the phase plan
#ifndef FX_I3_BPC
#define FX_I3_BPC (fWaves / FX_I3_WAVES)  // workgroups per CU in the launch
#endif
constexpr int kI3Slots = FX_I3_QA + 1;
constexpr int kI3QBytes = fBQ * fBK * 2;               // one slot: 16 KB (256 queries)
constexpr int kI3QDmaAll = kI3QBytes / 1024;           // 1-KB DMAs per chunk
// 1-KB DMAs per wave per chunk: every wave the same count, or (64-query tiles:
// 4 KB per chunk) one each on the first kI3QDmaAll waves and none on the rest
constexpr int kI3QDma = kI3QDmaAll >= kI3Waves ? kI3QDmaAll / kI3Waves : 1;
static_assert((kI3QDmaAll >= kI3Waves ? kI3QDma * kI3Waves : kI3QDmaAll) == kI3QDmaAll &&
                  kI3QDmaAll * 1024 == kI3QBytes && fBK == 32,
              "query ring");
static_assert(kI3Sub * kI3BM == fBM && kI3Waves <= fWaves, "workgroup tile");
struct Img3Shared {
  unsigned char qring[kI3Slots][kI3QBytes];
  float rinfo[kI3BM];
  float rterm[kI3BM];
  uint32_t rflags[2][kRowFlagWords];
  f32x4 qtab[fBQ];
  float2 qab[fBQ];
  uint32_t seg[fBQ + 3 * fBQ * FX_I3_SEG];  // counters, then entries {lb key, ub key, row}
  uint32_t segbase[fBQ];
  float rext[kI3BM];  // int8 image: 1 / s of the row
  f32x4 qinf[fBQ];   // int8 image: the query's launch_qprep8 record
  uint32_t rrow[kI3BM];  // int8 image: the global corpus row of the tile row (image8_perm)
};
static_assert(sizeof(Img3Shared) * (fWaves / kI3Waves) <= 160 * 1024,
              "filter_img3_kernel: LDS over 160 KB per CU");

// The pass test and appends of one wave's 32-row tile (RT = 1) against all
// kI2QT query tiles; appends into LDS segments (filter_epilogue_seg's layout).
template <int METRIC>
__device__ __forceinline__ void i3_epilogue(const f32x16 (&acc)[kI2QT], const float* rinfo,
                                            const float* rterm, const uint32_t* flags,
                                            const f32x4* qtab, const float2* qab,
                                            const FilterArgs& a, int64_t q0, int64_t r0, int wid,
                                            int h, int l32, uint32_t* seg, int diag) {
  constexpr int SEG = FX_I3_SEG;
  // row j of the lane (accumulator element j) is local row lr0 + (j & 3) + 8 (j >> 2)
  const int lr0 = wid * 32 + 4 * h;
  f32x4 rv4[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) rv4[g] = *reinterpret_cast<const f32x4*>(rinfo + lr0 + 8 * g);
  const uint32_t fmask = flags[wid * 2 + h], smask = flags[16 + wid * 2 + h];
  uint32_t pm[kI2QT];
#pragma unroll
  for (int u = 0; u < kI2QT; ++u) {
    const float2 ab = qab[u * 32 + l32];
    const f32x2 na = {-ab.x, -ab.x}, nb = {-ab.y, -ab.y};
    // fail bit j = sign of RN(RN(x_j - a rv_j) - b): set exactly when x_j -
    // a rv_j rounds below b; bit j enters last-in at bit 0
    uint32_t fail = 0u;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
      const f32x4 r = rv4[i >> 1];
      const f32x2 rp = (i & 1) ? f32x2{r[2], r[3]} : f32x2{r[0], r[1]};
      const f32x2 xp = {acc[u][2 * i], acc[u][2 * i + 1]};
      const f32x2 dd = __builtin_elementwise_fma(na, rp, xp) + nb;
      fail = __builtin_amdgcn_alignbit(fail, __float_as_uint(dd[1]), 31);
      fail = __builtin_amdgcn_alignbit(fail, __float_as_uint(dd[0]), 31);
    }
    // (b = -inf: no threshold yet or a forced query, every row passes whatever
    // the sign of a NaN product, filter_epilogue)
    const uint32_t qall = ab.y == -__builtin_inff() ? ~0u : 0u;
    pm[u] = (diag & 1) ? 0u : (~fail | fmask | qall) & ~smask & 0xffffu;
    if (q0 + u * 32 + l32 >= a.nq) pm[u] = 0u;
  }
  uint32_t any = 0u;
#pragma unroll
  for (int u = 0; u < kI2QT; ++u) any |= pm[u];
  if (__ballot(any != 0u) == 0ull) return;
  // Appends (a few per wave and tile): per query tile with a pass, a loop
  // over the lane's set bits; the row's accumulator element is selected by
  // a cndmask tree (a dynamic index would put the accumulators in scratch,
  // and a scratch load waits for the whole prefetched stream), its row
  // value re-read from LDS.  static_for over u for the same reason.
  static_for<kI2QT>([&](auto uc) {
    constexpr int u = decltype(uc)::value;
    if (__ballot(pm[u] != 0u) == 0ull) return;
    const int qi = u * 32 + (int)opaque((unsigned)l32);  // (not hoisted: spilled)
    const int64_t gq = q0 + qi;
    uint32_t bits = pm[u];
    uint32_t p = bits != 0u ? lds_add_rtn_u32(&seg[qi], (uint32_t)__popc(bits)) : 0u;
    const f32x4 qc = qtab[qi];
    const float qc1 = qc[0], qc0 = qc[1], qA = qc[2], qB = qc[3];
    const bool fq = !(qA <= 3.4e38f);
    uint32_t gp = ~0u;
    while (bits != 0u) {
      const int j = __builtin_ctz(bits);
      const uint32_t rest = bits;
      bits &= bits - 1u;
      // (bit-field selects, v_bfi_b32: a ?: select tree is turned back into
      // a dynamic index, i.e. scratch)
      auto pick = [](float lo, float hi, uint32_t m) {
        return __uint_as_float((__float_as_uint(hi) & m) | (__float_as_uint(lo) & ~m));
      };
      const uint32_t m0 = 0u - ((uint32_t)j & 1u), m1 = 0u - (((uint32_t)j >> 1) & 1u);
      const uint32_t m2 = 0u - (((uint32_t)j >> 2) & 1u), m3 = 0u - (((uint32_t)j >> 3) & 1u);
      float v8[8], v4[4], v2[2];
#pragma unroll
      for (int i = 0; i < 8; ++i) v8[i] = pick(acc[u][2 * i], acc[u][2 * i + 1], m0);
#pragma unroll
      for (int i = 0; i < 4; ++i) v4[i] = pick(v8[2 * i], v8[2 * i + 1], m1);
#pragma unroll
      for (int i = 0; i < 2; ++i) v2[i] = pick(v4[2 * i], v4[2 * i + 1], m2);
      const float x = pick(v2[0], v2[1], m3);
      const int lr = lr0 + (j & 3) + 8 * (j >> 2);
      const float rv = rinfo[lr];
      float lb, ub;
      if constexpr (METRIC == 0) {
        const float s2 = rv + qc0;
        const float d2 = fmaf(x, qc1, s2);
        const float e = fmaf(qA, s2, qB);
        lb = sqrtf(fmaxf(d2 - e, 0.f));
        ub = sqrtf(d2 + e);
      } else if constexpr (METRIC == 1) {
        const float e = fmaf(qA, rv, qB);
        lb = fmaf(x, qc1, -e);
        ub = fmaf(x, qc1, e);
      } else {
        const float rt = rterm[lr];
        const float dist = fmaf(x * rt, qc1, 0.5f);
        const float e = fmaf(qB, rt, qA);
        lb = dist - e;
        ub = dist + e;
      }
      if (fq || rv != rv) {  // forced: below / above every key
        lb = -__builtin_inff();
        ub = __builtin_nanf("");
      }
      const uint32_t grow = (uint32_t)(a.row_base + r0) + (uint32_t)lr;
      if (p < (uint32_t)SEG) {
        lds_write3_u32(seg + fBQ + 3 * (qi * SEG + p), order_key(lb), order_key(ub), grow);
      } else {  // rare: past the segment, global slots for the lane's remaining passes
        if (gp == ~0u) gp = atomicAdd(&a.count[gq * kCountStride], (uint32_t)__popc(rest));
        if (gp < (uint32_t)a.cap) {
          const size_t slot = (size_t)gq * a.cap + gp;
          if (a.cand_ub != nullptr) {
            a.cand[slot] = make_comp(lb, grow);
            a.cand_ub[slot] = make_comp(ub, grow);
          } else {
            a.cand[slot] = make_comp(ub, grow);
          }
        }
        ++gp;
      }
      ++p;
    }
  });
}

template <int METRIC, bool I8>
__global__ void __launch_bounds__(kI3Threads, 2) filter_img3_kernel(FilterArgs a) {
  constexpr int XS = FX_I3_XS, SEG = FX_I3_SEG;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Img3Shared* sh = reinterpret_cast<Img3Shared*>(smem);
#ifdef FX_DIAG_BUILD  // FX_FILTER_DIAG: 1 no appends, 2 no epilogue, 4 no MFMA,
                      // 8 no query DMA, 16 no step barrier, 32 no image loads
  const int diag = a.diag;
#else
  constexpr int diag = 0;
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  const int64_t q0 = (int64_t)blockIdx.y * fBQ;
  // chunks per tile, padded to a multiple of the register stages (past the
  // row end the image reads zeros and the query tile is zero-padded to dq)
  // (int8 image: 64 components per chunk, 32 per k-step, the same bytes)
  constexpr int CK = I8 ? 2 * fBK : fBK;
  const int nch = ((a.d + CK - 1) / CK + XS - 1) / XS * XS;
  const int ksteps = I8 ? (a.d + 31) / 32 : (a.d + 15) / 16;
  const int64_t ntile32 = (a.n + 31) / 32;
  // workgroup tiles: kI3Sub per fBM-row tile of the plan (a.tile_start, ...)
  const int64_t ntiles = a.num_tiles * kI3Sub;
  auto tile_r0 = [&](int64_t ti) {
    return (a.tile_start + (ti / kI3Sub) * a.tile_stride) * fBM + (ti % kI3Sub) * kI3BM;
  };
  if ((int64_t)blockIdx.x >= ntiles) return;
  if (a.skip_full) {  // every query of the tile predicted to overflow: nothing to do
    bool full = true;
    for (int q = tid; q < fBQ; q += kI3Threads)
      if (q0 + q < a.nq && a.count[(q0 + q) * kCountStride] <= (uint32_t)a.cap) full = false;
    if (__syncthreads_and(full)) return;
  }
  if constexpr (I8)
    i8_query_table<METRIC>(a, q0, sh->qtab, sh->qinf, tid, kI3Threads);
  else
    filter_query_table<METRIC>(a, q0, sh->qtab, sh->qab, tid, kI3Threads);
  for (int q = tid; q < fBQ; q += kI3Threads) sh->seg[q] = 0u;  // (ordered by the first barrier)
  // the ring starts zeroed (a slot whose DMA is dropped then holds finite values)
  for (int i = tid; i < kI3Slots * kI3QBytes / 16; i += kI3Threads)
    reinterpret_cast<i32x4*>(sh->qring)[i] = i32x4(0);
  __syncthreads();

  // the query tile, blocked by 32 components (FilterArgs::Qh); chunk c of
  // query q is 64 B at (c * qstride + q) * 64
  const __amdgpu_buffer_rsrc_t qr = [&] {
    const uint64_t qp = reinterpret_cast<uint64_t>(a.Qh + q0 * 32);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)qp);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(qp >> 32));
    const int nb = __builtin_amdgcn_readfirstlane(
        (int)(((int64_t)(a.dq / 32 - 1) * a.qstride + fBQ) * 64));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0,
                                             nb, 0x00020000);
  }();
  // this lane's piece of each of the wave's DMAs: query 16 j + lane / 4, slot
  // piece lane % 4 holding global piece (lane % 4) ^ ((q >> 2) & 3)
  uint32_t qv[kI3QDma];
#pragma unroll
  for (int i = 0; i < kI3QDma; ++i) {
    const int j = wid * kI3QDma + i;
    const int q = 16 * j + (lane >> 2);
    qv[i] = (uint32_t)(q * 64 + (((lane & 3) ^ ((q >> 2) & 3)) * 16));
  }
  // (chunks past the query tile's padding, when nch is padded to the
  // stages: an offset beyond the buffer, the DMA is dropped and the slot
  // keeps finite values of an earlier chunk, multiplied by zero image rows)
  const int qchunks = a.dq / CK;
  auto issue_q = [&](int c, int slot) {
    if (diag & 8) return;
    if (kI3QDmaAll < kI3Waves && wid >= kI3QDmaAll) return;  // (wave-uniform)
    unsigned char* st = sh->qring[slot];
#pragma unroll
    for (int i = 0; i < kI3QDma; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(qr, (i3_lds_ptr)(st + (wid * kI3QDma + i) * 1024), 16,
                                               c < qchunks ? qv[i] : 0x7fff0000u,
                                               (int)(c * a.qstride * 64), 0, 0);
  };
  // this wave's 32-row tile of the row tile at step iteration ti: its
  // k-steps, one KB each (a tile past the end: an empty descriptor, zeros)
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
  typedef f16x8 XA[kI2KS];
  auto load_x = [&](XA& xa, __amdgpu_buffer_rsrc_t xr, int c) {
    if (diag & 32) {
#pragma unroll
      for (int s = 0; s < kI2KS; ++s) xa[s] = f16x8((_Float16)0.f);
      return;
    }
#pragma unroll
    for (int s = 0; s < kI2KS; ++s) {
      const int ks = c * kI2KS + s;  // wave-uniform: past the row end reads zeros
      const uint32_t off = ks < ksteps ? xl : 0x7fff0000u;
      xa[s] = __builtin_bit_cast(
          f16x8, __builtin_amdgcn_raw_buffer_load_b128(xr, off, ks * 1024, 2 /* nt */));
    }
  };
  // B fragment of query tile u, k-step s of a slot: query Q = 32 u + l32,
  // global piece 2 s + h at its swizzled place
  uint32_t bq[kI2KS];
#pragma unroll
  for (int s = 0; s < kI2KS; ++s) {
    const int Q = (int)opaque((unsigned)l32);
    bq[s] = (uint32_t)(Q * 64 + (((2 * s + h) ^ ((Q >> 2) & 3)) * 16));
  }
  f32x16 acc[kI2QT];
  // a tile's first k-step takes its accumulator input from this constant
  // (int8: the bits of 1.5 * 2^23, see "int8 filter image"; fp16: zeros)
  // instead of 128 moves per tile into the accumulators
  const f32x16 acc0 = f32x16(I8 ? kI8Magic : 0.f);
  // FIRST: the tile's first chunk (its k-step 0 starts from acc0)
  auto compute = [&](const XA& xa, int slot, auto first) {
    constexpr bool FIRST = decltype(first)::value;
    if (diag & 4) {  // (diagnostics: no MFMA; the row loads stay live)
      if (xa[0][0] == (_Float16)1.2345f && xa[kI2KS - 1][7] == (_Float16)2.f) a.count[0] = 7;
      if (FIRST) {
#pragma unroll
        for (int u = 0; u < kI2QT; ++u) acc[u] = acc0;
      }
      return;
    }
    const unsigned char* st = sh->qring[slot];
    // B fragments of a k-step read into their own registers before its
    // MFMAs (FX_I3_BPF 1; 2: both k-steps' first): left to itself, hipcc
    // read each fragment into one register set right before its MFMA and
    // waited lgkmcnt(0) in between, so every MFMA paid a full LDS latency
    auto mfma = [&](int u, const f16x8& xv, const f16x8& bv, bool start) {
      const f32x16 cin = start ? acc0 : acc[u];
      if constexpr (I8) {
        typedef int i32x16 __attribute__((ext_vector_type(16)));
        acc[u] = __builtin_bit_cast(f32x16, __builtin_amdgcn_mfma_i32_32x32x32_i8(
            __builtin_bit_cast(i32x4, xv), __builtin_bit_cast(i32x4, bv),
            __builtin_bit_cast(i32x16, cin), 0, 0, 0));
      } else {
        acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xv, bv, cin, 0, 0, 0);
      }
    };
#if FX_I3_BPF != 0
    // (query tile u sits 32 x 64 B further: (Q + 32 u) has the same swizzle)
    auto read_b = [&](f16x8 (&bv)[kI2QT], int s) {
#pragma unroll
      for (int u = 0; u < kI2QT; ++u)
        bv[u] = *reinterpret_cast<const f16x8*>(st + bq[s] + u * 32 * 64);
    };
#endif
#if FX_I3_BPF == 0
    static_for<kI2KS>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
#pragma unroll
      for (int u = 0; u < kI2QT; ++u) {
        const f16x8 bv = *reinterpret_cast<const f16x8*>(st + bq[s] + u * 32 * 64);
        mfma(u, xa[s], bv, FIRST && s == 0);
      }
    });
#elif FX_I3_BPF == 1
    static_for<kI2KS>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      f16x8 bv[kI2QT];
      read_b(bv, s);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kI2QT; ++u) mfma(u, xa[s], bv[u], FIRST && s == 0);
      __builtin_amdgcn_sched_barrier(0);
    });
#else
    static_assert(kI2KS == 2, "FX_I3_BPF 2: two k-steps per chunk");
    f16x8 b0[kI2QT], b1[kI2QT];
    read_b(b0, 0);
    read_b(b1, 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kI2QT; ++u) mfma(u, xa[0], b0[u], FIRST);
#pragma unroll
    for (int u = 0; u < kI2QT; ++u) mfma(u, xa[1], b1[u], false);
    __builtin_amdgcn_sched_barrier(0);
#endif
  };

  // ---- prologue: query chunks 0 .. QA-1 and image chunks 0 .. XS-1 of the
  // first tile in flight
  int qc = 0, qslot = 0;  // next query chunk to issue and its slot
  static_assert(!FX_I3_PAIR || (kI3Slots == 4 && XS % 2 == 0), "FX_I3_PAIR: two pairs, even stages");
#pragma unroll
  for (int i = 0; i < (FX_I3_PAIR ? 2 : FX_I3_QA); ++i) {
    issue_q(qc, qslot);
    qc = qc + 1 == nch ? 0 : qc + 1;
    qslot = qslot + 1 == kI3Slots ? 0 : qslot + 1;
  }
  XA xa[XS];
  int64_t xt = blockIdx.x;  // tile (iteration index) of the next image chunk to load
  int xc = 0;
  __amdgpu_buffer_rsrc_t xr = x_rsrc(xt);
  static_for<XS>([&](auto sc) {
    load_x(xa[decltype(sc)::value], xr, xc);
    if (++xc == nch) {
      xc = 0;
      xt += gridDim.x;
      xr = x_rsrc(xt);
    }
  });
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (once: the prologue's order differs)
  int rslot = 0;  // slot of the query chunk the next step reads
  int par = 0;
  const int lr = tid & (kI3BM - 1);  // the row this thread notes (threads >= kI3BM: duplicates)
  for (int64_t ti = blockIdx.x; ti < ntiles; ti += gridDim.x, par ^= 1) {
    const int64_t r0 = tile_r0(ti);
    if (tid < kRowFlagWords) sh->rflags[par][tid] = 0u;  // (read two tiles back)
    std::conditional_t<I8, f32x4, float> rsum = {};
    uint32_t mword = 0u;
    // one K step: multiply chunk c + S, then (LOAD) refill its register
    // stage with the chunk XS steps ahead (the next tile's first chunks at
    // the end of a tile, FX_I3_XPF)
    auto step = [&](int c, auto sc, auto ld, auto first) {
      constexpr int S = decltype(sc)::value;
      // query chunk c + S landed (this wave's DMAs; vmcnt retires in issue
      // order, and the loads issued after it are QA - 1 steps' DMAs plus the
      // image chunks of the QA steps from its own: none in a group that loads
      // nothing, i.e. the tile's last group without FX_I3_XPF, where only the
      // steps before the group's start loaded; extra loads, e.g. the rows'
      // terms, only make the wait stronger), and every wave done with the
      // slot refilled next
      constexpr bool LD = decltype(ld)::value;
      if constexpr (FX_I3_PAIR) {
        // even steps only (nch is a multiple of XS, so the step parity is
        // S's): the pair (c + S, c + S + 1) was issued two steps back, and
        // after it only image chunks: the two steps' own (none in a tile's
        // last group), or at a tile's first group the post-epilogue stages
        if constexpr (S % 2 == 0) {
          constexpr int kN = S == 0 ? (decltype(first)::value && !FX_I3_XPF ? XS * kI2KS : 2 * kI2KS)
                                    : (LD ? 2 * kI2KS : 0);
          if (diag & 16)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          else
            i3_wait_barrier<kN>();
#pragma unroll
          for (int i = 0; i < 2; ++i) {  // into the pair every wave finished before the barrier
            issue_q(qc, qslot);
            qc = qc + 1 == nch ? 0 : qc + 1;
            qslot = qslot + 1 == kI3Slots ? 0 : qslot + 1;
          }
        }
      } else {
      constexpr int kXAfter = LD ? FX_I3_QA : (FX_I3_QA > S ? FX_I3_QA - S : 0);
      if (diag & 16)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      else
        i3_wait_barrier<(FX_I3_QA - 1) * kI3QDma + kXAfter * kI2KS>();
      issue_q(qc, qslot);
      qc = qc + 1 == nch ? 0 : qc + 1;
      qslot = qslot + 1 == kI3Slots ? 0 : qslot + 1;
      }
      if constexpr (decltype(first)::value && S == 0) {  // the rows' image sums and mask words of this tile
        const int64_t row = r0 + lr < a.n ? r0 + lr : a.n - 1;
        if constexpr (I8)
          rsum = *reinterpret_cast<const f32x4*>(a.rowinfo + row * kI8RowInfo);
        else
          rsum = a.rowinfo[row];
        // (int8 image: the mask bit of the corpus row the image row holds)
        int64_t mrow = row;
        if constexpr (I8) mrow = perm_row(a.perm_a, a.n, row);
        // (both kernel arguments: global loads; a pointer to a __device__
        // constant made a flat load, which counts in lgkmcnt too, and the
        // step's LDS waits then waited for it)
        const bool masked = a.mask != nullptr;
        const uint32_t* mp = masked ? a.mask + (mrow >> 5)
                                    : reinterpret_cast<const uint32_t*>(a.rowinfo) + row * (I8 ? kI8RowInfo : 1);
        mword = *mp | (masked ? 0u : ~0u);
        if constexpr (I8) mword = masked ? (mword >> (mrow & 31)) << (row & 31) : mword;
      }
      compute(xa[S], rslot, std::bool_constant<decltype(first)::value && S == 0>{});
      rslot = rslot + 1 == kI3Slots ? 0 : rslot + 1;
      if constexpr (decltype(ld)::value) {
        load_x(xa[S], xr, xc);
        if (++xc == nch) {
          xc = 0;
          xt += gridDim.x;
          xr = x_rsrc(xt);
        }
      }
    };
    using Load = std::true_type;
    using Xpf = std::integral_constant<bool, FX_I3_XPF>;
    using First = std::true_type;
    using Later = std::false_type;
    // the first chunk group peeled (its first k-step starts from acc0)
    if (nch > XS) {
      static_for<XS>([&](auto sc) { step(0, sc, Load{}, First{}); });
      int c = XS;
      for (; c + XS < nch; c += XS)
        static_for<XS>([&](auto sc) { step(c, sc, Load{}, Later{}); });
      static_for<XS>([&](auto sc) { step(c, sc, Xpf{}, Later{}); });
    } else {
      static_for<XS>([&](auto sc) { step(0, sc, Xpf{}, First{}); });
    }
    if (tid < kI3BM) {  // one thread per row: bound factor, flags
      // (the row index recomputed here from opaque(tid): hoisted out of the
      // tile loop, its flag bit was spilled and reloaded behind a vmcnt(0))
      const int lr = (int)opaque((unsigned)tid);
      const int64_t row = r0 + lr;
      bool ok = row < a.n && ((mword >> (row & 31)) & 1u);
      if constexpr (I8) {  // {omega, 1/s, N/s, n^2/s}
        const float y1 = METRIC == 1 ? rsum[1] : METRIC == 2 ? rsum[2] : rsum[3];
        i8_note_row(sh->rinfo, sh->rterm, sh->rext, sh->rflags[par], lr, rsum[0], y1, rsum[1], ok);
        sh->rrow[lr] = (uint32_t)a.row_base + (row < a.n ? perm_row(a.perm_a, a.n, row) : 0u);
      } else {
      const float s = ok ? rsum : 0.f;
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
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (diag & 2) {
      if (acc[0][0] == 1.2345f) a.count[0] = 7;
    } else {
      if constexpr (I8)
        i8_epilogue<METRIC>(acc, sh->rinfo, sh->rterm, sh->rext, sh->rrow, sh->rflags[par],
                            sh->qtab, sh->qinf, a, q0, wid, h, l32, sh->seg, diag);
      else
        i3_epilogue<METRIC>(acc, sh->rinfo, sh->rterm, sh->rflags[par], sh->qtab, sh->qab, a, q0,
                            r0, wid, h, l32, sh->seg, diag);
    }
    if constexpr (!FX_I3_XPF) {  // the next tile's first chunks, after the epilogue
      static_for<XS>([&](auto sc) {
        load_x(xa[decltype(sc)::value], xr, xc);
        if (++xc == nch) {
          xc = 0;
          xt += gridDim.x;
          xr = x_rsrc(xt);
        }
      });
    }
  }
  // the ring's and the stream's last loads (past the end) land before the
  // workgroup's LDS is released; then the segments go out
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  filter_flush_segments<SEG, kI3Threads>(sh->seg, sh->segbase, a, q0, tid);
}

static int launch_img3(const FilterArgs& a, int metric, hipStream_t stream) {
  const void* fn =
      a.img8 ? (metric == FX_METRIC_COS  ? (const void*)filter_img3_kernel<2, true>
                : metric == FX_METRIC_IP ? (const void*)filter_img3_kernel<1, true>
                                         : (const void*)filter_img3_kernel<0, true>)
             : (metric == FX_METRIC_COS  ? (const void*)filter_img3_kernel<2, false>
                : metric == FX_METRIC_IP ? (const void*)filter_img3_kernel<1, false>
                                         : (const void*)filter_img3_kernel<0, false>);
  if (int rc = allow_lds(fn)) return rc;
  int cus = 0;
  if (int rc = device_cus(&cus)) return rc;
  int64_t bx = (int64_t)cus * FX_I3_BPC;  // workgroups per CU
  if (bx > a.num_tiles * kI3Sub) bx = a.num_tiles * kI3Sub;
  return launch_query_tiles(fn, "filter_img3_kernel", a, kI3Threads, sizeof(Img3Shared), bx, fBQ,
                            a.img8 ? kI8QInfo : 4, stream);
}

