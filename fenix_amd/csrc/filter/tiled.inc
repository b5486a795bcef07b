// What the tiled-image kernels with an LDS-DMA ring or LDS append segments
// share (after filter/tile.inc, before img3.inc / img8.inc / img6.inc): the
// counted-wait barrier and the inline-asm LDS appends, and for int8 images
// the derivation of the pass test ("int8 filter image" below) with its query
// table, bounds and epilogue (filter_img3_kernel<., true>, filter_img6_kernel;
// filter_img8_kernel takes the table and the bounds).
#ifndef FX_I3_SEG
#define FX_I3_SEG 24  // LDS append entries per query (overflow: global slots);
                      // filter_img3_kernel's and filter_img6_kernel's segments
#endif
typedef __attribute__((address_space(3))) void* i3_lds_ptr;

template <int N>
__device__ __forceinline__ void i3_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// LDS appends through inline asm: the compiler cannot tell the append
// segments from an LDS-DMA ring, so in a kernel with one it put vmcnt(0)
// before a plain ds_add_rtn / ds_write -- waiting for the ring's chunks in
// flight, about 1-2 us per wave and tile with an append (filter_img8_kernel:
// configs[2]'s F2 ran 1.94 ms with its appends, 1.09 without them).  The
// segments are never DMA targets; the flush reads them behind a barrier.
__device__ __forceinline__ uint32_t lds_add_rtn_u32(uint32_t* p, uint32_t v) {
  const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(p);
  uint32_t r;
  asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(a), "v"(v) : "memory");
  return r;
}
__device__ __forceinline__ void lds_write1_u32(uint32_t* p, uint32_t x) {
  const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(p);
  asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(x) : "memory");
}
__device__ __forceinline__ void lds_write2_u32(uint2* p, uint32_t x, uint32_t y) {
  const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint2*)(p);
  asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(uint2{x, y}) : "memory");
}
__device__ __forceinline__ void lds_write3_u32(uint32_t* p, uint32_t x, uint32_t y, uint32_t z) {
  const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(p);
  asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %2 offset:4\n\tds_write_b32 %0, %3 offset:8"
               ::"v"(a), "v"(x), "v"(y), "v"(z) : "memory");
}

// ------------------------------------------------------ int8 filter image
//
// The int8 image (launch_image8) halves the image stream again and runs on
// v_mfma_i32_32x32x32_i8 (twice the fp16 rate): per row a scale s, x~ =
// rint(x / s) in [-127, 127], w = |x~|, e >= |x - s x~|, v = e / s; per query
// the same with s_q, w_q, e_q (launch_qprep8).  Both are scaled so that w,
// w_q <= 2048, so the exact integer product I = x~ . q~ has |I| <= 2^22.
// With D = x . q, exactly:  D - s s_q I = (x - s x~) . q + s x~ . (q - s_q q~),
//   |D - s s_q I| <= s s_q (v P + w R),  P = |q| / s_q,  R = e_q / s_q
// (IP also carries the scan's f32 summation error g |x||q|, g = (d + 2) 2^-24
// with 1 % slack, into P and R; cosine and L2 carry it in their constants).
// With kappa = kI8Kappa and R' = max(R, P / kappa) (kept by the query),
// v P + w R <= (w + kappa v) R' = omega R': omega is the row's one error
// value (launch_image8).  Per metric, with M = 12582912 + I (the accumulator
// starts at the bits of 1.5 * 2^23, so the i32 sum read as a float is exactly
// M for |I| <= 2^22: no conversion), a pair can reach the threshold T only if
//   IP   I + omega R' + (1/s) (T / s_q)                    >= 0
//   cos  I + omega R' - (N / s) (1 - 2T - 2c) N_q / s_q    >= 0   (N = max(|x|, 1e-12))
//   L2   I + omega R' - (n^2 / s) / (2 s_q) - (1/s) (n_q^2 - T^2 (1 + 2^-20) / (1 - g2)) / (2 s_q) >= 0
// c = 3 g + 16 u and g2 = 2 g + 8 u cover the scan's own roundings (u = 2^-24;
// fx_exact.h exact_distance16: dot and norms in f32, one division).  Each
// per-query coefficient carries a relative slack >= 16 u (the roundings of the
// products and sums of the test) and the test compares with 12582912 - 8.
// The appends' [lb, ub] (i8_bounds) are evaluated in f32 from the same terms,
// each widened outward by 16 u of the magnitudes it was computed from (every
// rounding on the way is relative to a term it is added to, at most ~8 u).
// A non-finite row or query, or one whose scaled norm would exceed 2048, is
// forced through (omega or R' not finite).
constexpr float kI8Magic = 12582912.f;   // 1.5 * 2^23: bits 0x4B400000
constexpr float kI8C0 = 12582912.f - 8.f;

// Per query {R', c1, c2, 0} of the int8 pass test
//   M + omega R' + y1 c1 + y2 c2 >= kI8C0
// with the row values y1 (IP 1/s, cosine N/s, L2 n^2/s) and y2 (L2 1/s).
// No threshold yet (T NaN) or a forced query: R' = +inf (everything passes).
template <int METRIC>
__device__ __forceinline__ void i8_query_table(const FilterArgs& a, int64_t q0, f32x4* qtab,
                                               f32x4* qinf, int tid, int nthreads) {
  const float u = 5.9604644775390625e-08f;
  const float g = (float)(a.d + 2) * u * 1.01f;
  for (int i = tid; i < fBQ; i += nthreads) {
    const int64_t gq = q0 + i;
    f32x4 c = f32x4(0.f), qi = f32x4(0.f);
    if (gq < a.nq) {
      qi = *reinterpret_cast<const f32x4*>(a.qinfo + gq * kI8QInfo);  // {s_q, R', n_q^2, |q|}
      float tf = key_float((uint32_t)(a.thr[gq] >> 32));
      // the upper-bound test (ub_test): -R' below, T widened by 2^-14
      // relative (the rows that set T pass again)
      if (a.ub_test) tf += fabsf(tf) * 6.103515625e-05f;
      const float sq = qi[0];
      c[0] = qi[1];
      if constexpr (METRIC == 1) {
        const float t = tf / sq;
        c[1] = t + 16.f * u * fabsf(t);
      } else if constexpr (METRIC == 2) {
        const float cc = 3.f * g + 16.f * u;
        const float K = (1.f - 2.f * tf - 2.f * cc) * (fmaxf(qi[3], 1e-12f) / sq);
        c[1] = -K + (g + 16.f * u) * fabsf(K);
      } else {
        const float g2 = 2.f * g + 8.f * u;
        const float L1 = 0.5f / sq;
        const float t2 = tf * tf * (1.f + 9.5367431640625e-07f) / (1.f - g2);
        const float L0 = (qi[2] * (1.f - 4.f * u) - t2) * L1;
        c[1] = -L1 * (1.f - g - 16.f * u);
        c[2] = -L0 + 16.f * u * fabsf(L0);
      }
      if (tf != tf || !(c[0] <= 3.4e38f))
        c = f32x4{__builtin_inff(), 0.f, 0.f, 0.f};
      else if (a.ub_test)
        c[0] = -c[0];
    }
    qtab[i] = c;
    qinf[i] = qi;
  }
}

// [lb, ub] of an appended (row, query) pair of the int8 filter from M, the
// row's {omega, y1, 1/s} (i8_note_row) and the query's launch_qprep8 record,
// in f32 with outward slack: every rounding below is relative to a term it
// is added to (at most ~8 u each), so each bound is widened by 16 u of the
// magnitudes it was computed from.
template <int METRIC>
__device__ __forceinline__ void i8_bounds(float m, float om, float y1, float is, f32x4 qi, int d,
                                          float& lb, float& ub) {
  if (om != om) {  // forced row: below / above every key
    lb = -__builtin_inff();
    ub = __builtin_nanf("");
    return;
  }
  const float u = 5.9604644775390625e-08f;
  const float g = (float)(d + 2) * u * 1.01f;
  const float I = m - kI8Magic;  // exact
  const float E = fmaf(om * qi[1], 8.f * u, om * qi[1]) + 4.f;
  const float s = 1.f / is;
  const float sig = s * qi[0];
  const float a1 = I + E, a2 = I - E;
  if constexpr (METRIC == 1) {
    const float lo = -sig * a1, hi = -sig * a2;
    lb = lo - 16.f * u * fabsf(lo);
    ub = hi + 16.f * u * fabsf(hi);
  } else if constexpr (METRIC == 2) {
    const float c = 3.f * g + 32.f * u;
    const float den = fmaxf(y1 * s, 1e-12f) * fmaxf(qi[3], 1e-12f);
    const float r1 = sig * a1 / den, r2 = sig * a2 / den;
    lb = 0.5f - 0.5f * r1 - c - 16.f * u * (1.f + fabsf(r1));
    ub = 0.5f - 0.5f * r2 + c + 16.f * u * (1.f + fabsf(r2));
  } else {
    const float g2 = 2.f * g + 8.f * u;
    const float n2 = y1 * s;
    const float alo = n2 * (1.f - g - 16.f * u) + qi[2] * (1.f - 4.f * u);
    const float ahi = n2 * (1.f + g + 16.f * u) + qi[2] * (1.f + 4.f * u);
    const float t1 = 2.f * sig * a1, t2 = 2.f * sig * a2;
    const float lo2 = (1.f - g2) * (alo - t1) - 16.f * u * (alo + fabsf(t1));
    const float hi2 = (1.f + g2) * (ahi - t2) + 16.f * u * (ahi + fabsf(t2));
    lb = sqrtf(fmaxf(lo2, 0.f)) * (1.f - 4.f * u);
    ub = sqrtf(fmaxf(hi2, 0.f)) * (1.f + 4.f * u);
  }
  if (lb != lb) lb = -__builtin_inff();  // (a non-finite query: R' = inf)
  if (ub != ub) ub = __builtin_nanf("");
}

// One row's values for the int8 epilogue: omega (NaN: forced), y1 and 1/s,
// and its flags (filter_note_row's words)
__device__ __forceinline__ void i8_note_row(float* rinfo, float* rterm, float* rext,
                                            uint32_t* flags, int lr, float om, float y1, float is,
                                            bool ok) {
  rinfo[lr] = om;
  rterm[lr] = y1;
  rext[lr] = is;
  int word, bit;
  filter_row_bit<1>(lr, word, bit);
  if (!ok) atomicOr(&flags[16 + word], 1u << bit);
  else if (om != om) atomicOr(&flags[word], 1u << bit);
}

// i3_epilogue for the int8 image: the packed pass test above (2 or 3
// v_pk_fma_f32 and one v_pk_add_f32 per two pairs), appends with i8_bounds
// all-pass phases of at most this many tiles reserve fixed slots even when
// the slice shares its segments (i8_epilogue)
// QMASK (filter_img6_kernel's per-query row masks): rqmask holds fBQ / 32
// words of query bits per row of the tile; bit l32 of word u of a row says
// whether query 32 u + l32 of the slice admits it.
constexpr int64_t kAllPassSlotTiles = 64;
template <int METRIC, bool QMASK = false>
__device__ __forceinline__ void i8_epilogue(const f32x16 (&acc)[kI2QT], const float* rinfo,
                                            const float* rterm, const float* rext,
                                            const uint32_t* rrow, const uint32_t* flags,
                                            const f32x4* qtab, const f32x4* qinf,
                                            const FilterArgs& a, int64_t q0, int wid, int h,
                                            int l32, uint32_t* seg, int diag,
                                            int segcap = FX_I3_SEG,
                                            const uint32_t* rqmask = nullptr) {
  const int lr0 = wid * 32 + 4 * h;
  const uint32_t fmask = flags[wid * 2 + h], smask = flags[16 + wid * 2 + h];
  // row groups g of 4 rows outside (their values read once from LDS), query
  // tiles inside; fail bit j = 4 g + i enters last-in at bit 0, so g and i
  // run down
  uint32_t fail[kI2QT];
#pragma unroll
  for (int u = 0; u < kI2QT; ++u) fail[u] = 0u;
  const f32x2 nc0 = {-kI8C0, -kI8C0};
#pragma unroll
  for (int g = 3; g >= 0; --g) {
    const f32x4 om = *reinterpret_cast<const f32x4*>(rinfo + lr0 + 8 * g);
    const f32x4 y1 = *reinterpret_cast<const f32x4*>(rterm + lr0 + 8 * g);
    f32x4 y2 = f32x4(0.f);
    if constexpr (METRIC == 0) y2 = *reinterpret_cast<const f32x4*>(rext + lr0 + 8 * g);
#pragma unroll
    for (int u = 0; u < kI2QT; ++u) {
      const f32x4 co = qtab[u * 32 + l32];
      const f32x2 ra = {co[0], co[0]}, c1 = {co[1], co[1]}, c2 = {co[2], co[2]};
#pragma unroll
      for (int hp = 1; hp >= 0; --hp) {  // rows 4 g + 2 hp, + 1
        const int i = 2 * g + hp;
        const f32x2 xp = {acc[u][2 * i], acc[u][2 * i + 1]};
        const f32x2 op = hp ? f32x2{om[2], om[3]} : f32x2{om[0], om[1]};
        const f32x2 p1 = hp ? f32x2{y1[2], y1[3]} : f32x2{y1[0], y1[1]};
        f32x2 t = __builtin_elementwise_fma(op, ra, xp);
        t = __builtin_elementwise_fma(p1, c1, t);
        if constexpr (METRIC == 0) {
          const f32x2 p2 = hp ? f32x2{y2[2], y2[3]} : f32x2{y2[0], y2[1]};
          t = __builtin_elementwise_fma(p2, c2, t);
        }
        const f32x2 dd = t + nc0;
        fail[u] = __builtin_amdgcn_alignbit(fail[u], __float_as_uint(dd[1]), 31);
        fail[u] = __builtin_amdgcn_alignbit(fail[u], __float_as_uint(dd[0]), 31);
      }
    }
  }
  uint32_t pm[kI2QT];
  // (all_pass: every live row, whatever the test says: with R' = inf a zero
  // row's 0 * inf is a NaN whose sign decides the bit)
  const uint32_t force = a.all_pass ? ~0u : fmask;
  // QMASK: bit j of qbits[u] is the admission bit of the lane's row j for its
  // query of tile u (every lane of a half reads the same words: a broadcast);
  // applied after force, so a forced row and an all-pass phase obey the mask
  uint32_t qbits[kI2QT];
#pragma unroll
  for (int u = 0; u < kI2QT; ++u) qbits[u] = 0xffffu;
  if constexpr (QMASK) {
    typedef uint32_t qw_t __attribute__((ext_vector_type(kI2QT)));
#pragma unroll
    for (int u = 0; u < kI2QT; ++u) qbits[u] = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const qw_t w = reinterpret_cast<const qw_t*>(rqmask)[lr0 + (j & 3) + 8 * (j >> 2)];
#pragma unroll
      for (int u = 0; u < kI2QT; ++u) qbits[u] |= ((w[u] >> l32) & 1u) << j;
    }
  }
#pragma unroll
  for (int u = 0; u < kI2QT; ++u) {
    pm[u] = (diag & 1) ? 0u : (~fail[u] | force) & ~smask & qbits[u] & 0xffffu;
    if (q0 + u * 32 + l32 >= a.nq) pm[u] = 0u;
  }
  if (a.all_pass && (segcap <= FX_I3_SEG || a.num_tiles <= kAllPassSlotTiles)) {
                     // no threshold yet (first phase): every live pair, slots reserved
                     // per lane and query, accumulators indexed statically (a slice
                     // of few live queries over a large first sample, k ~ 1 000,
                     // appends through its segments below instead: its whole sample
                     // otherwise meets in one global counter, ~3 K atomics; a small
                     // one, k = 100's 20 tiles, is faster through the slots)
    static_for<kI2QT>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const uint32_t bits = pm[u];
      if (__ballot(bits != 0u) == 0ull) return;
      const int qi = u * 32 + (int)opaque((unsigned)l32);
      const int64_t gq = q0 + qi;
      uint32_t p = bits != 0u ? atomicAdd(&a.count[gq * kCountStride], (uint32_t)__popc(bits)) : 0u;
      const f32x4 qrec = qinf[qi];
      static_for<16>([&](auto jc) {
        constexpr int jj = decltype(jc)::value;
        if (!((bits >> jj) & 1u)) return;
        // (opaque: 16 rows' LDS offsets hoisted to the kernel start were spilled)
        const int lr = (int)opaque((unsigned)lr0) + (jj & 3) + 8 * (jj >> 2);
        float lb, ub;
        i8_bounds<METRIC>(acc[u][jj], rinfo[lr], rterm[lr], rext[lr], qrec, a.d, lb, ub);
        if (p < (uint32_t)a.cap) {
          const uint32_t grow = rrow[lr];
          const size_t slot = (size_t)gq * a.cap + p;
          if (a.cand_ub != nullptr) {
            a.cand[slot] = make_comp(lb, grow);
            a.cand_ub[slot] = make_comp(ub, grow);
          } else {
            a.cand[slot] = make_comp(ub, grow);
          }
        }
        ++p;
      });
    });
    return;
  }
  uint32_t any = 0u;
#pragma unroll
  for (int u = 0; u < kI2QT; ++u) any |= pm[u];
  if (__ballot(any != 0u) == 0ull) return;
  static_for<kI2QT>([&](auto uc) {
    constexpr int u = decltype(uc)::value;
    if (__ballot(pm[u] != 0u) == 0ull) return;
    const int qi = u * 32 + (int)opaque((unsigned)l32);  // (not hoisted: spilled)
    const int64_t gq = q0 + qi;
    uint32_t bits = pm[u];
    uint32_t p = bits != 0u ? lds_add_rtn_u32(&seg[qi], (uint32_t)__popc(bits)) : 0u;
    const f32x4 qrec = qinf[qi];
    uint32_t gp = ~0u;
    while (bits != 0u) {
      const int j = __builtin_ctz(bits);
      const uint32_t rest = bits;
      bits &= bits - 1u;
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
      float lb, ub;
      i8_bounds<METRIC>(x, rinfo[lr], rterm[lr], rext[lr], qrec, a.d, lb, ub);
      const uint32_t grow = rrow[lr];
      if (p < (uint32_t)segcap) {
        lds_write3_u32(seg + fBQ + 3 * (qi * segcap + p), order_key(lb), order_key(ub), grow);
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

