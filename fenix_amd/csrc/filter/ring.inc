// ring_kernel: the rejected LDS-DMA ring variant of filter_kernel (DESIGN.md
// §3.6), diagnostic builds only (FX_DIAG_BUILD; tools/ select it with
// FX_FILTER_RING=1).  After filter/tile.inc.
//
// The same filter with every operand staged by LDS-DMA (buffer_load ... lds):
// no prefetch registers, a 3-deep ring of K-chunk stages (X rows and the query
// tile, 48 KB per stage for f32 rows), one raw s_barrier per chunk behind a
// COUNTED vmcnt so two stages stay in flight across it (a __syncthreads()
// would drain them: cdna_hip_programming.md §5 "Pipelining across barriers").
// The stage sequence runs on across tiles, so the next tile's first chunks
// stream in while a tile's epilogue runs.  Rows are converted to fp16 at
// fragment-read time (f32 corpora) or read as they are (f16 corpora: exact).
// LDS images are XOR-swizzled by 16-B piece (the DMA writes lane L at
// base + 16 L; the swizzle is applied to the global address) so fragment
// reads are bank-conflict free.
namespace ring {
#ifndef FX_RING_WAVES
#define FX_RING_WAVES (FX_FILTER_BQ >= 256 ? 16 : 8)  // 64 or 32 accumulator registers per wave
#endif
constexpr int kBM = 256, kBQ = FX_FILTER_BQ, kBK = 32, kStages = 3, kWaves = FX_RING_WAVES;
constexpr int kThreads = kWaves * 64;
static_assert(kBM == kFilterTileRows, "one tile height for every filter kernel");
constexpr int kRG = 4;                  // 64-row groups
constexpr int kQG = kWaves / kRG;       // query groups
constexpr int kQT = kBQ / kQG / 32;     // 32-query tiles per wave
template <typename XT>
struct Lay {
  static constexpr int xrow = kBK * (int)sizeof(XT);  // bytes per row per stage
  static constexpr int xbytes = kBM * xrow;
  static constexpr int qbytes = kBQ * kBK * 2;
  static constexpr int stage = xbytes + qbytes;
  // 1 KB DMA instructions per wave and stage; every wave issues the same
  // number (the counted waits rely on it), surplus ones land in a dummy KB
  static constexpr int xblocks = xbytes / 1024, qblocks = qbytes / 1024;
  static constexpr int xdma = (xblocks + kWaves - 1) / kWaves;
  static constexpr int qdma = (qblocks + kWaves - 1) / kWaves;
  static constexpr int ndma = xdma + qdma;
  static constexpr int rinfo = kStages * stage;
  static constexpr int rterm = rinfo + kBM * 4;
  static constexpr int rflags = rterm + kBM * 4;  // [2][kRowFlagWords] by tile parity
  static constexpr int qtab = rflags + 2 * kRowFlagWords * 4;
  static constexpr int qab = qtab + kBQ * 16;
  static constexpr int dummy = qab + kBQ * 8;
  static constexpr int total = dummy + 1024;
};

typedef __attribute__((address_space(3))) void* lds_ptr;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, int64_t bytes) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  const int nb = __builtin_amdgcn_readfirstlane((int)bytes);
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0,
                                           nb, 0x00020000);
}

// Issue the DMA of K chunk c of the tile at row r0 (and of the query tile)
// into stage buffer sb.  Rows past n read as zeros (descriptor size), pieces
// past d through an offset beyond it; a tile index past the end gets an empty
// descriptor, so every wave always issues exactly Lay::ndma instructions.
template <typename XT>
__device__ __forceinline__ void ring_issue(unsigned char* smem, const FilterArgs& a, int64_t r0,
                                           bool valid, int c, int sb, int wid, int lane,
                                           __amdgpu_buffer_rsrc_t qr) {
  using L = Lay<XT>;
  const int64_t rows = valid ? (a.n - r0 < kBM ? a.n - r0 : kBM) : 0;
  const __amdgpu_buffer_rsrc_t xr =
      make_rsrc(reinterpret_cast<const XT*>(a.X) + (valid ? r0 : 0) * (int64_t)a.d,
                rows * a.d * (int64_t)sizeof(XT));
  const int k0 = c * kBK;
  unsigned char* st = smem + sb * L::stage;
#pragma unroll
  for (int i = 0; i < L::xdma; ++i) {
    const int j = wid * L::xdma + i;  // 1-KB block of the stage's X image
    if (j >= L::xblocks) {            // wave-uniform: a dummy keeps the count
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(smem + L::dummy), 16, 0x7fff0000u,
                                               0, 0, 0);
      continue;
    }
    uint32_t voff;
    if constexpr (sizeof(XT) == 4) {  // 8 rows x 8 pieces of 16 B per block
      const int row = 8 * j + (lane >> 3);
      const int p = (lane & 7) ^ ((row >> 1) & 7);
      voff = k0 + p * 4 < a.d ? (uint32_t)((row * a.d + p * 4) * 4) : 0x7fff0000u;
    } else {  // 16 rows x 4 pieces
      const int row = 16 * j + (lane >> 2);
      const int p = (lane & 3) ^ ((row >> 2) & 3);
      voff = k0 + p * 8 < a.d ? (uint32_t)((row * a.d + p * 8) * 2) : 0x7fff0000u;
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(st + j * 1024), 16, voff,
                                             k0 * (int)sizeof(XT), 0, 2 /* nt */);
  }
#pragma unroll
  for (int i = 0; i < L::qdma; ++i) {
    const int j = wid * L::qdma + i;  // 16 queries x 4 pieces per block
    if (j >= L::qblocks) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(qr, (lds_ptr)(smem + L::dummy), 16, 0x7fff0000u,
                                               0, 0, 0);
      continue;
    }
    const int q = 16 * j + (lane >> 2);
    const int p = (lane & 3) ^ ((q >> 2) & 3);
    const uint32_t voff = (uint32_t)(q * 64 + p * 16);  // blocked layout (FilterArgs::Qh)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(qr, (lds_ptr)(st + L::xbytes + j * 1024), 16, voff,
                                             (int)(c * a.qstride * 64), 0, 0);
  }
}

// MFMAs of one stage: 2 k-steps x (2 row tiles x 4 query tiles).  Waves of
// query group 0 also accumulate the rows' sums of squares and fp16-overflow
// flags from the values they read.
// kv = d - (first k of the chunk): elements at k >= d are zeroed (the DMA of a
// piece past the row end is dropped, leaving stale LDS there; the query tile
// is zero-padded, but the row sums must not see it).
template <typename XT, bool IMG>
__device__ __forceinline__ void ring_compute(f32x16 (&acc)[2][kQT], const unsigned char* st,
                                             int rg, int qg, int l32, int h, int kv,
                                             float (&sq)[2], uint32_t& ovf) {
  using L = Lay<XT>;
#pragma unroll
  for (int s = 0; s < kBK / 16; ++s) {
    f16x8 av[2], bv[kQT];
    const int kf = 16 * s + 8 * h;  // first k of this lane's fragment, relative to the chunk
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int R = rg * 64 + t * 32 + l32;
      if constexpr (sizeof(XT) == 4) {
        const int p0 = 4 * s + 2 * h, sw = (R >> 1) & 7;
        f32x4 a0 = *reinterpret_cast<const f32x4*>(st + R * L::xrow + ((p0 ^ sw) * 16));
        f32x4 a1 = *reinterpret_cast<const f32x4*>(st + R * L::xrow + (((p0 + 1) ^ sw) * 16));
        if (kf >= kv) a0 = f32x4(0.f);
        if (kf + 4 >= kv) a1 = f32x4(0.f);
        const f16x4 c0 = __builtin_convertvector(a0, f16x4);
        const f16x4 c1 = __builtin_convertvector(a1, f16x4);
        av[t] = __builtin_shufflevector(c0, c1, 0, 1, 2, 3, 4, 5, 6, 7);
        if (qg == 0) {
          float m = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            sq[t] = fmaf(a0[e], a0[e], sq[t]);
            sq[t] = fmaf(a1[e], a1[e], sq[t]);
            m = fmaxf(m, fmaxf(fabsf(a0[e]), fabsf(a1[e])));
          }
          ovf |= (uint32_t)(m >= 65520.f) << t;
        }
      } else {
        const int p = 2 * s + h;
        av[t] = *reinterpret_cast<const f16x8*>(st + R * L::xrow + ((p ^ ((R >> 2) & 3)) * 16));
        if (kf >= kv) av[t] = f16x8(0);
        if (!IMG && qg == 0) {
#pragma unroll
          for (int e = 0; e < 8; ++e) sq[t] = fmaf((float)av[t][e], (float)av[t][e], sq[t]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kQT; ++u) {
      const int Q = qg * kQT * 32 + u * 32 + l32;
      const int p = 2 * s + h;
      bv[u] = *reinterpret_cast<const f16x8*>(st + L::xbytes + Q * 64 + ((p ^ ((Q >> 2) & 3)) * 16));
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < kQT; ++u)
        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[t], bv[u], acc[t][u], 0, 0, 0);
  }
}

// Wait until this wave's DMAs of the stage to be read have landed (the last
// N issued stay in flight), then the workgroup barrier: every wave's DMAs of
// that stage are in, and every wave is done reading the stage being refilled.
template <int N>
__device__ __forceinline__ void ring_sync() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

__device__ __forceinline__ void lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
}  // namespace ring

// IMG: the rows are an f32 corpus's fp16 filter image (row sums from rowinfo)
template <typename XT, int METRIC, bool IMG>
__global__ void __launch_bounds__(ring::kThreads, ring::kWaves / 4) ring_kernel(FilterArgs a) {
  using namespace ring;
  using L = Lay<XT>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* rinfo = reinterpret_cast<float*>(smem + L::rinfo);
  float* rterm = reinterpret_cast<float*>(smem + L::rterm);
  uint32_t* rflags = reinterpret_cast<uint32_t*>(smem + L::rflags);
  f32x4* qtab = reinterpret_cast<f32x4*>(smem + L::qtab);
  float2* qab = reinterpret_cast<float2*>(smem + L::qab);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (SGPR)
  const int rg = wid % kRG, qg = wid / kRG;  // 64-row group, query group
  const int h = lane >> 5, l32 = lane & 31;
  const int64_t q0 = (int64_t)blockIdx.y * kBQ;
  const int nch = (a.d + kBK - 1) / kBK;
  const int diag = a.diag;
  filter_query_table<METRIC>(a, q0, qtab, qab, tid, kThreads);
  const __amdgpu_buffer_rsrc_t qr =
      make_rsrc(a.Qh + q0 * 32, ((int64_t)(a.dq / 32 - 1) * a.qstride + kBQ) * 64);

  // step sequence: (tile ti, chunk c) -> stage buffer (step % 3)
  auto tile_r0 = [&](int64_t ti) -> int64_t { return (a.tile_start + ti * a.tile_stride) * kBM; };
  int64_t ti = blockIdx.x;
  if (ti >= a.num_tiles) return;
  // prologue: steps 0 and 1
  int64_t it = ti;  // tile of the next step to issue
  int ic = 0;       // its chunk
  int isb = 0;      // its stage buffer
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    ring_issue<XT>(smem, a, tile_r0(it), it < a.num_tiles, ic, isb, wid, lane, qr);
    if (++ic == nch) {
      ic = 0;
      it += gridDim.x;
    }
    isb = isb == kStages - 1 ? 0 : isb + 1;
  }
  int sb = 0;  // stage buffer of the current step
  int par = 0;
  for (; ti < a.num_tiles; ti += gridDim.x, par ^= 1) {
    const int64_t r0 = tile_r0(ti);
    uint32_t* flags = rflags + par * kRowFlagWords;
    if (tid < kRowFlagWords) flags[tid] = 0u;  // (read two tiles back; barriers since)
    f32x16 acc[2][kQT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < kQT; ++u) acc[t][u] = f32x16(0.f);
    float sq[2] = {0.f, 0.f};
    uint32_t ovf = 0u;
    for (int c = 0; c < nch; ++c) {
      ring_sync<L::ndma>();
      ring_issue<XT>(smem, a, tile_r0(it), it < a.num_tiles, ic, isb, wid, (int)opaque(lane), qr);
      if (++ic == nch) {
        ic = 0;
        it += gridDim.x;
      }
      isb = isb == kStages - 1 ? 0 : isb + 1;
      if (!(diag & 4)) {
        const int ol = (int)opaque(lane);
        ring_compute<XT, IMG>(acc, smem + sb * L::stage, rg, qg, ol & 31, ol >> 5, a.d - c * kBK, sq,
                         ovf);
      }
      sb = sb == kStages - 1 ? 0 : sb + 1;
    }
    // row values: query-group-0 waves hold the rows' partial sums (lane halves)
    if (qg == 0) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sq[t] += __shfl_xor(sq[t], 32);
        const uint32_t of = (ovf | __shfl_xor(ovf, 32)) >> t & 1u;
        if (h == 0) {
          const int lr = rg * 64 + t * 32 + l32;
          const int64_t row = r0 + lr;
          bool ok = row < a.n;
          if constexpr (IMG) sq[t] = ok ? a.rowinfo[row] : 0.f;
          if (ok && a.mask != nullptr) ok = (a.mask[row >> 5] >> (row & 31)) & 1u;
          float rv;
          if constexpr (METRIC == 0) {
            rv = sq[t];
          } else if constexpr (METRIC == 1) {
            rv = sqrtf(sq[t]);
          } else {
            rv = fmaxf(sqrtf(sq[t]), 1e-12f);
          }
          if (!(sq[t] <= 3.4e38f) || of) rv = __builtin_nanf("");
          filter_note_row<METRIC>(rinfo, rterm, flags, lr, rv, ok);
        }
      }
    }
    lds_sync();
    if (!(diag & 2)) {
      const int ol = (int)opaque(lane);  // keep the epilogue's lane math out of the chunk loop
      filter_epilogue<METRIC, kQT>(acc, rinfo, rterm, flags, qtab, qab, a, q0, r0, rg, qg, ol >> 5,
                                   ol & 31, diag);
    }
  }
  // drain: the ring's last DMAs (empty descriptors past the end) must land
  // before the workgroup's LDS is released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <typename XT, bool IMG = false>
static int launch_ring(const FilterArgs& a, int metric, hipStream_t stream) {
  const void* fn = metric == FX_METRIC_COS ? (const void*)ring_kernel<XT, 2, IMG>
                   : metric == FX_METRIC_IP ? (const void*)ring_kernel<XT, 1, IMG>
                                            : (const void*)ring_kernel<XT, 0, IMG>;
  if (int rc = allow_lds(fn)) return rc;
  int cus = 0;
  if (int rc = device_cus(&cus)) return rc;
  int64_t bx = cus;
  if (bx > a.num_tiles) bx = a.num_tiles;
  return launch_query_tiles(fn, "ring_kernel", a, ring::kThreads, ring::Lay<XT>::total, bx,
                            ring::kBQ, 4, stream);
}

// FX_FILTER_RING=1 (filter_ring()): every row type, and row-major fp16 images
static int launch_ring_rows(const FilterArgs& a, int metric, hipStream_t stream) {
  const bool f16 = a.dtype == FX_DTYPE_F16;
  if (a.rowinfo != nullptr) {
    if (!f16) {
      set_error("filter: a filter image is fp16");
      return FX_EINVAL;
    }
    return launch_ring<_Float16, true>(a, metric, stream);
  }
  return f16 ? launch_ring<_Float16>(a, metric, stream) : launch_ring<float>(a, metric, stream);
}

