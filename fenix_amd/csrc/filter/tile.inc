// The batched filter's shared part: the tile constants and the device helpers
// that more than one kernel family uses, and the host launch helper.
//
// Included first by every variant translation unit (knn_filter_q256.hip,
// _h256, _q128, _q64, _q64i), inside its namespace fx::<variant>, after it
// has defined FX_FILTER_BQ and FX_FILTER_BK (and FX_FILTER_WAVES, where it
// has that knob).  The family files (staged.inc, img2.inc, tiled.inc,
// img3.inc, img8.inc, img6.inc, ring.inc) follow it; the variant's header
// says which of them it holds.
#ifndef FX_FILTER_WAVES
#define FX_FILTER_WAVES 8   // waves per workgroup (two per SIMD)
#endif
constexpr int fBM = kFilterTileRows;            // corpus rows per tile
constexpr int fBQ = FX_FILTER_BQ;               // queries per block
constexpr int fBK = FX_FILTER_BK;               // K chunk (elements)
constexpr int fLds = fBK + 8;                   // padded LDS row (halves): 16 B pad
constexpr int fWaves = FX_FILTER_WAVES;
constexpr int fThreads = 64 * fWaves;           // waves: fRG row groups x fQG query groups
constexpr int fRG = fBM / 64;                   // 64-row groups (2 MFMA row tiles each)
constexpr int fQG = fWaves / fRG;               // query groups
constexpr int fQT = fBQ / fQG / 32;             // 32-query MFMA tiles per wave
constexpr int fQC = fBK / 8;                    // 16-B f16 pieces per query per chunk
// Q pieces per thread per chunk (a variant with no register-staged kernels,
// q64i, may have fewer pieces than threads)
constexpr int fQP = fBQ * fQC / fThreads > 0 ? fBQ * fQC / fThreads : 1;
static_assert(fQG >= 1 && fRG * fQG == fWaves && fQT >= 1, "wave grid");

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Per-tile row flags for the epilogue, by tile parity: [forced | skipped][8]
// 32-bit masks, one per (64-row group, lane half) in the bit order of the
// lane's accumulator rows (filter_row_bit); up to 16 (row group, lane half)
// words per kind: 32-row groups (the tiled-image kernel) or 64-row groups
constexpr int kRowFlagWords = 2 * 16;
static_assert(fBM <= 256, "row flag words: (64-row group, lane half) <= 8");
struct FilterPreQ {  // one K chunk of the (L2-resident) query tile
  i32x4 q[fQP];
};

// Buffer loads: a per-tile descriptor (its size clips rows past n to zero) and
// 32-bit per-lane offsets, the chunk offset in the scalar operand.
struct FilterAddr {
  __amdgpu_buffer_rsrc_t xr, qr;
  int d, dq;
  uint32_t xs, qs;  // byte strides between a thread's consecutive X / Q pieces
  uint32_t qb;      // byte stride between blocks of 32 query components
};

// A thread's offsets, derived once per tile from opaque(tid) (so they are not
// hoisted and kept live across the epilogue); a piece / K step / buffer then
// adds a wave-uniform or compile-time constant: no per-use address math in
// the K loop (v_mul_lo_u32 is quarter rate).
constexpr uint32_t kQB = sizeof(_Float16) * fBQ * fLds;  // one LDS Q buffer, bytes
struct FilterOff {
  uint32_t xg, qg;  // global byte offsets of piece 0 (X within the tile, Q within the query tile)
  uint32_t xw, qw;  // LDS byte addresses of the stores of piece 0 (buffer 0)
  uint32_t xr, qr;  // LDS byte addresses of this lane's fragment reads (buffer 0)
  int kc;           // element offset of this lane's piece within a K chunk
};

template <typename T>
__device__ __forceinline__ T& lds_at(unsigned char* smem, uint32_t off) {
  return *reinterpret_cast<T*>(smem + off);
}

__device__ __forceinline__ void filter_load_q(FilterPreQ& p, const FilterAddr& ad,
                                              const FilterOff& o, int c, int diag) {
#pragma unroll
  for (int i = 0; i < fQP; ++i) {
    if (diag & 8) {
      p.q[i] = i32x4(0);
      continue;
    }
    // chunks past the padded row: an offset beyond the buffer (zeros)
    const uint32_t off = c * fBK < ad.dq ? o.qg + i * ad.qs : 0x7fff0000u;
    p.q[i] = __builtin_bit_cast(
        i32x4, __builtin_amdgcn_raw_buffer_load_b128(ad.qr, off, c * (fBK / 32) * ad.qb, 0));
  }
}

// Hide a value from loop-invariant code motion: addresses derived from it are
// recomputed (a few VALU ops) where they are used instead of being hoisted out
// of the chunk loop and kept live (or spilled) across it.
__device__ __forceinline__ unsigned opaque(unsigned v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Calls f(integral_constant<int, I>) for I = 0 .. N-1 (indices stay static)
template <int N, typename F, int I = 0>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<N, F, I + 1>(static_cast<F&&>(f));
  }
}

// static_for when STATIC, else a plain unrolled loop (the compiler's choice)
template <bool STATIC, int N, typename F>
__device__ __forceinline__ void unroll_for(F&& f) {
  if constexpr (STATIC) {
    static_for<N>(static_cast<F&&>(f));
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) f(i);
  }
}

// Per-query constants of the pass test (once per block).  The test lb <= T
// is linear in the product x for a fixed row, so it is precomputed as
// x >= a * rv + b with rv the row's value (cosine: max(|x|, 1e-12); IP: |x|;
// L2: |x|^2):
//   cos  lb = x c1 / rv + 0.5 - A - B / rv,  c1 = -0.5 / (scale |q|) < 0
//        -> x >= ((T - 0.5 + A) rv + B) / c1
//   IP   lb = -x / scale - A rv - B           -> x >= (-T - B - A rv) scale
//   L2   lb^2 = s2 - 2 x / scale - A s2 - B,  s2 = rv + |q|^2, against
//        T^2 (1 + 2^-20) -> x >= ((1 - A) s2 - B - T^2) scale / 2
// The roundings of this rearrangement are far inside the bound's slack.
// T = NaN (no threshold yet) or a forced query: everything passes
// (a = 0, b = -inf); padding queries: nothing (b = +inf).  qtab keeps
// {c1, c0, A, B} for the exact bounds of appended pairs.
template <int METRIC>
__device__ __forceinline__ void filter_query_table(const FilterArgs& a, int64_t q0, f32x4* qtab,
                                                   float2* qab, int tid, int nthreads) {
  for (int i = tid; i < fBQ; i += nthreads) {
    const int64_t gq = q0 + i;
    f32x4 c = f32x4(0.f);
    float2 ab = {0.f, __builtin_inff()};
    if (gq < a.nq) {
      const f32x4 info = *reinterpret_cast<const f32x4*>(a.qinfo + gq * 4);
      float tf = key_float((uint32_t)(a.thr[gq] >> 32));
      const float qinv = info[0], qa = info[1], qA = info[2], qB = info[3];
      c[2] = qA;
      c[3] = qB;
      // the upper-bound test (ub_test): the same forms with the error terms
      // A, B negated, and T widened by 2^-14 relative (the rows that set T
      // pass again; extra passes only cost an append)
      const float sA = a.ub_test ? -qA : qA, sB = a.ub_test ? -qB : qB;
      if (a.ub_test) tf += fabsf(tf) * 6.103515625e-05f;
      if constexpr (METRIC == 0) {
        c[0] = -2.f * qinv;
        c[1] = qa;
        const float t2 = tf * tf * (1.f + 9.5367431640625e-07f);
        const float h = 0.5f / qinv;
        ab.x = (1.f - sA) * h;
        ab.y = ((1.f - sA) * qa - sB - t2) * h;
      } else if constexpr (METRIC == 1) {
        c[0] = -qinv;
        const float sc = 1.f / qinv;
        ab.x = -sA * sc;
        ab.y = (-tf - sB) * sc;
      } else {
        c[0] = -0.5f * qinv / qa;
        ab.x = (tf - 0.5f + sA) / c[0];
        ab.y = sB / c[0];
      }
      if (tf != tf || !(qA <= 3.4e38f)) ab = {0.f, -__builtin_inff()};
    }
    qtab[i] = c;
    qab[i] = ab;
  }
}

// Where local row lr of a 256-row tile sits in the epilogue's masks when a
// wave owns RT 32-row MFMA tiles: the word of its (32 RT-row group, lane
// half) and its bit there, j with lr = 32 RT rg + 4 h + roff(j)
// (filter_epilogue).
template <int RT>
__device__ __forceinline__ void filter_row_bit(int lr, int& word, int& bit) {
  const int w = lr % (32 * RT), w2 = lr & 31;
  word = (lr / (32 * RT)) * 2 + ((w2 >> 2) & 1);
  bit = (w >> 5) * 16 + (w2 >> 3) * 4 + (w2 & 3);
}

// Record one row's bound factor for the epilogue (rv NaN: forced through,
// ok false: skipped), the cosine term 1 / rv of its appends, and its flags
// (words zeroed at the tile start, ordered by the K loop's barriers).
template <int METRIC, int RT = 2>
__device__ __forceinline__ void filter_note_row(float* rinfo, float* rterm, uint32_t* flags,
                                                int lr, float rv, bool ok) {
  rinfo[lr] = ok ? rv : -1.f;
  if constexpr (METRIC == 2) rterm[lr] = 1.f / rv;
  int word, bit;
  filter_row_bit<RT>(lr, word, bit);
  if (!ok) atomicOr(&flags[16 + word], 1u << bit);
  else if (rv != rv) atomicOr(&flags[word], 1u << bit);
}

// Epilogue of one tile: pass test per (row, query) — an fma, a subtraction
// and a funnel shift that collects the sign of (product - threshold) (see
// filter_query_table; extra passes only cost a rescored candidate); the
// lane's passes over its 16 RT rows form a bit mask per query column, one
// atomic per (lane, column) reserves their slots.  Forced rows (flag words
// 0..15) always pass, skipped rows (16..31) never.
template <int METRIC, int QT, int RT = 2>
__device__ __forceinline__ void filter_epilogue(const f32x16 (&acc)[RT][QT], const float* rinfo,
                                                const float* rterm, const uint32_t* flags,
                                                const f32x4* qtab, const float2* qab,
                                                const FilterArgs& a, int64_t q0, int64_t r0,
                                                int rg, int qg, int h, int l32, int diag) {
    constexpr int NR = 16 * RT;  // rows per lane
    constexpr uint32_t kAll = NR == 32 ? ~0u : (1u << NR) - 1u;
    const int lr0 = rg * 32 * RT + 4 * h;
    const float* ri = rinfo + lr0;
    const uint32_t grow0 = (uint32_t)(a.row_base + r0 + lr0);
    // row j of the lane (acc register j & 15 of row tile j >> 4) sits at a
    // compile-time offset from ri: row values are re-read from LDS where used
    auto roff = [](int j) { return (j >> 4) * 32 + (j & 3) + 8 * ((j & 15) >> 2); };
    const uint32_t fmask = flags[rg * 2 + h], smask = flags[16 + rg * 2 + h];
    uint32_t pm[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
      const float2 ab = qab[qg * QT * 32 + u * 32 + l32];
      // fail bits: sign of RN(x - t) is set exactly when x < t (x, t finite;
      // RN never flips a sign, x == t gives +0); bit j enters last-in at
      // bit 0, so j runs down
      uint32_t fail = 0u;
#pragma unroll
      for (int j = NR - 1; j >= 0; --j) {
        const float t = fmaf(ab.x, ri[roff(j)], ab.y);
        fail = __builtin_amdgcn_alignbit(fail, __float_as_uint(acc[j >> 4][u][j & 15] - t), 31);
      }
      // (b = -inf: no threshold yet or a forced query, every row passes -- said
      // here, not left to the sign of acc - t: a non-finite query's products
      // are NaN of either sign)
      const uint32_t qall = ab.y == -__builtin_inff() ? ~0u : 0u;
      pm[u] = (diag & 1) ? 0u : ((~fail | fmask | qall) & ~smask & kAll);
      if (q0 + qg * QT * 32 + u * 32 + l32 >= a.nq) pm[u] = 0u;
    }
    uint32_t any = 0u;
#pragma unroll
    for (int u = 0; u < QT; ++u) any |= pm[u];
    if (__ballot(any != 0u) == 0ull) return;
    uint32_t pos[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
      pos[u] = 0u;
      const int64_t gq = q0 + qg * QT * 32 + u * 32 + l32;
      if (pm[u] != 0u) {
        if ((diag & 32) && a.cand_ub != nullptr)  // profiling only (final phase): no atomic
          pos[u] = (uint32_t)l32 * 64u;
        else
          pos[u] = atomicAdd(&a.count[gq * kCountStride], (uint32_t)__popc(pm[u]));
      }
    }
#pragma unroll
    for (int u = 0; u < QT; ++u) {
      if (__ballot(pm[u] != 0u) == 0ull) continue;
      const int qi = qg * QT * 32 + u * 32 + l32;
      const int64_t gq = q0 + qi;
      const f32x4 qc = qtab[qi];
      const float qc1 = qc[0], qc0 = qc[1], qA = qc[2], qB = qc[3];
      const bool fq = !(qA <= 3.4e38f);
      uint32_t p = pos[u];
      // rows in groups of 4: a group no lane of the wave appends from is
      // skipped with one wave-uniform branch (a few appends per wave and tile)
#pragma unroll
      for (int g = 0; g < NR / 4; ++g) {
        if (__ballot(((pm[u] >> (4 * g)) & 0xfu) != 0u) == 0ull) continue;
#pragma unroll
      for (int j = 4 * g; j < 4 * g + 4; ++j) {
        if (!((pm[u] >> j) & 1u)) continue;
        const float rv = ri[roff(j)];
        const float x = acc[j >> 4][u][j & 15];
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
          const float rt = rterm[lr0 + roff(j)];
          const float dist = fmaf(x * rt, qc1, 0.5f);
          const float e = fmaf(qB, rt, qA);
          lb = dist - e;
          ub = dist + e;
        }
        if (fq || rv != rv) {  // forced: below / above every key
          lb = -__builtin_inff();
          ub = __builtin_nanf("");
        }
        if (p < (uint32_t)a.cap && !((diag & 64) && a.cand_ub != nullptr)) {  // (64: profiling)
          const uint32_t grow = grow0 + (uint32_t)roff(j);
          const size_t slot = (size_t)gq * a.cap + p;
          if (a.cand_ub != nullptr) {
            a.cand[slot] = make_comp(lb, grow);
            a.cand_ub[slot] = make_comp(ub, grow);
          } else {
            a.cand[slot] = make_comp(ub, grow);
          }
        }
        ++p;
      }
      }
    }
}

// filter_epilogue with the appends staged in LDS: they go to a per-(workgroup, query) LDS segment of SEG
// entries {lb key, ub key, row} (slot from an LDS atomic: no global atomic
// and no global store on the tile boundary), flushed at the kernel's end
// (filter_flush_segments); entries past SEG take a global slot as before.
template <int METRIC, int QT, int RT, int SEG>
__device__ __forceinline__ void filter_epilogue_seg(const f32x16 (&acc)[RT][QT], const float* rinfo,
                                                const float* rterm, const uint32_t* flags,
                                                const f32x4* qtab, const float2* qab,
                                                const FilterArgs& a, int64_t q0, int64_t r0,
                                                int rg, int qg, int h, int l32, int diag,
                                                uint32_t* seg) {
    constexpr int NR = 16 * RT;  // rows per lane
    constexpr uint32_t kAll = NR == 32 ? ~0u : (1u << NR) - 1u;
    const int lr0 = rg * 32 * RT + 4 * h;
    const float* ri = rinfo + lr0;
    const uint32_t grow0 = (uint32_t)(a.row_base + r0 + lr0);
    // row j of the lane (acc register j & 15 of row tile j >> 4) sits at a
    // compile-time offset from ri: row values are re-read from LDS where used
    auto roff = [](int j) { return (j >> 4) * 32 + (j & 3) + 8 * ((j & 15) >> 2); };
    const uint32_t fmask = flags[rg * 2 + h], smask = flags[16 + rg * 2 + h];
    uint32_t pm[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
      const float2 ab = qab[qg * QT * 32 + u * 32 + l32];
      // fail bits: sign of RN(x - t) is set exactly when x < t (x, t finite;
      // RN never flips a sign, x == t gives +0); bit j enters last-in at
      // bit 0, so j runs down
      uint32_t fail = 0u;
#pragma unroll
      for (int j = NR - 1; j >= 0; --j) {
        const float t = fmaf(ab.x, ri[roff(j)], ab.y);
        fail = __builtin_amdgcn_alignbit(fail, __float_as_uint(acc[j >> 4][u][j & 15] - t), 31);
      }
      // (b = -inf: no threshold yet or a forced query, every row passes -- said
      // here, not left to the sign of acc - t: a non-finite query's products
      // are NaN of either sign)
      const uint32_t qall = ab.y == -__builtin_inff() ? ~0u : 0u;
      pm[u] = (diag & 1) ? 0u : ((~fail | fmask | qall) & ~smask & kAll);
      if (q0 + qg * QT * 32 + u * 32 + l32 >= a.nq) pm[u] = 0u;
    }
    uint32_t any = 0u;
#pragma unroll
    for (int u = 0; u < QT; ++u) any |= pm[u];
    if (__ballot(any != 0u) == 0ull) return;
    uint32_t pos[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
      pos[u] = 0u;
      const int64_t gq = q0 + qg * QT * 32 + u * 32 + l32;
      if (pm[u] != 0u) {
        if constexpr (SEG > 0)  // LDS counter of the query (seg[0 .. fBQ))
          pos[u] = atomicAdd(&seg[qg * QT * 32 + u * 32 + l32], (uint32_t)__popc(pm[u]));
        else if ((diag & 32) && a.cand_ub != nullptr)  // profiling only (final phase): no atomic
          pos[u] = (uint32_t)l32 * 64u;
        else
          pos[u] = atomicAdd(&a.count[gq * kCountStride], (uint32_t)__popc(pm[u]));
      }
    }
    unroll_for<(SEG > 0), QT>([&](auto uc) {
      const int u = uc;
      if (__ballot(pm[u] != 0u) == 0ull) return;
      const int qi = qg * QT * 32 + u * 32 + l32;
      const int64_t gq = q0 + qi;
      const f32x4 qc = qtab[qi];
      const float qc1 = qc[0], qc0 = qc[1], qA = qc[2], qB = qc[3];
      const bool fq = !(qA <= 3.4e38f);
      uint32_t p = pos[u];
      uint32_t gp = ~0u;
      // rows in groups of 4: a group no lane of the wave appends from is
      // skipped with one wave-uniform branch (a few appends per wave and tile)
      unroll_for<(SEG > 0), NR / 4>([&](auto gc) {
        const int g = gc;
        if (__ballot(((pm[u] >> (4 * g)) & 0xfu) != 0u) == 0ull) return;
      unroll_for<(SEG > 0), 4>([&](auto jc) {
        const int j = 4 * g + (int)jc;
        if (!((pm[u] >> j) & 1u)) return;
        const float rv = ri[roff(j)];
        const float x = acc[j >> 4][u][j & 15];
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
          const float rt = rterm[lr0 + roff(j)];
          const float dist = fmaf(x * rt, qc1, 0.5f);
          const float e = fmaf(qB, rt, qA);
          lb = dist - e;
          ub = dist + e;
        }
        if (fq || rv != rv) {  // forced: below / above every key
          lb = -__builtin_inff();
          ub = __builtin_nanf("");
        }
        if constexpr (SEG > 0) {
          const uint32_t grow = grow0 + (uint32_t)roff(j);
          if (p < (uint32_t)SEG) {
            uint32_t* e = seg + fBQ + 3 * (qi * SEG + p);
            e[0] = order_key(lb);
            e[1] = order_key(ub);
            e[2] = grow;
          } else {  // rare: past the segment, global slots for the lane's remaining passes
            if (gp == ~0u) gp = atomicAdd(&a.count[gq * kCountStride], (uint32_t)__popc(pm[u] >> j));
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
        } else
        if (p < (uint32_t)a.cap && !((diag & 64) && a.cand_ub != nullptr)) {  // (64: profiling)
          const uint32_t grow = grow0 + (uint32_t)roff(j);
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
    });
}

// Write a workgroup's LDS append segments (filter_epilogue_seg) to the
// candidate buffer: one global atomic per query reserves the slots.  seg =
// [fBQ counters][fBQ x SEG entries {lb key, ub key, row}]; called by every
// thread after the last tile (ends with the counters reused as bases).
// segcap: entries per query (SEG, or more when the slice has fewer live
// queries: i8_epilogue's segcap), fBQ * SEG entries in all.
template <int SEG, int NT = fThreads>
__device__ __forceinline__ void filter_flush_segments(uint32_t* seg, uint32_t* base,
                                                      const FilterArgs& a, int64_t q0, int tid,
                                                      int segcap = SEG) {
  __syncthreads();
  for (int q = tid; q < fBQ; q += NT) {
    const uint32_t n = seg[q] < (uint32_t)segcap ? seg[q] : (uint32_t)segcap;
    seg[q] = n;
    base[q] = n != 0u && q0 + q < a.nq ? atomicAdd(&a.count[(q0 + q) * kCountStride], n) : 0u;
  }
  __syncthreads();
  for (int i = tid; i < fBQ * SEG; i += NT) {
    const int q = i / segcap, j = i % segcap;
    if (q >= fBQ || (uint32_t)j >= seg[q]) continue;
    const uint32_t p = base[q] + (uint32_t)j;
    if (p >= (uint32_t)a.cap) continue;
    const uint32_t* e = seg + fBQ + 3 * i;
    const size_t slot = (size_t)(q0 + q) * a.cap + p;
    if (a.cand_ub != nullptr) {
      a.cand[slot] = ((uint64_t)e[0] << 32) | e[2];
      a.cand_ub[slot] = ((uint64_t)e[1] << 32) | e[2];
    } else {
      a.cand[slot] = ((uint64_t)e[1] << 32) | e[2];
    }
  }
}

// The tiled-image kernels (img2, img3, img6): every wave multiplies its rows
// against all the queries of the tile
constexpr int kI2QT = fBQ / 32;  // query tiles per wave (every query)
constexpr int kI2KS = fBK / 16;  // k-steps per chunk

// Launch kernel fn (name: for the error text) over every query tile of the
// batch: grids of bx x (at most 65 535 query tiles of bq queries) workgroups
// of `threads` threads with smem bytes of dynamic LDS, each grid with its own
// copy of the arguments advanced to its first query (qinfo: qinfo_stride
// floats per query, 4 or kI8QInfo).
static int launch_query_tiles(const void* fn, const char* name, const FilterArgs& a, int threads,
                              size_t smem, int64_t bx, int bq, int qinfo_stride,
                              hipStream_t stream) {
  const int64_t qtiles = (a.nq + bq - 1) / bq;
  for (int64_t y0 = 0; y0 < qtiles; y0 += 65535) {
    FilterArgs b = a;
    const int64_t yn = (qtiles - y0) < 65535 ? (qtiles - y0) : 65535;
    b.Qh = a.Qh + y0 * bq * 32;  // (64 B per query and chunk in both formats)
    b.qinfo = a.qinfo + y0 * bq * qinfo_stride;
    b.thr = a.thr + y0 * bq;
    b.count = a.count + y0 * bq * kCountStride;
    b.cand = a.cand + y0 * bq * (int64_t)a.cap;
    if (a.cand_ub) b.cand_ub = a.cand_ub + y0 * bq * (int64_t)a.cap;
    b.nq = a.nq - y0 * bq;
    if (a.qmask != nullptr) b.qmask = a.qmask + y0 * bq / 32;
    void* args[] = {(void*)&b};
    hipError_t e = hipLaunchKernel(fn, dim3((unsigned)bx, (unsigned)yn), dim3(threads), args, smem,
                                   stream);
    if (e != hipSuccess) {
      set_error("%s launch: %s", name, hipGetErrorString(e));
      return FX_EHIP;
    }
  }
  return check_launch(name);
}
