// Row predicates evaluated on the device into the search's row bitmap.
//
// The filter of index.py:161 (a pc.Expression over scalar columns of the
// source) arrives as a verified postfix program (fenix_amd/io/predicate.py):
// leaf compares of a column with a literal, set membership, null tests, and
// Kleene and / or / not above them.  pred_kernel runs it once per row:
//
//   * one lane per row, grid-stride over 256-row steps; a wave's 64 results
//     leave as two ballot words through ordinary vector stores, the kept-row
//     count as a popcount per block and one atomic add per block (mask_kernel's
//     shape, knn_code.hip);
//   * the program and the column table ride in the kernel-argument struct, so
//     instruction fetch and dispatch are scalar and wave-uniform;
//   * every stack entry is a (value, known) pair of booleans; each lane keeps
//     the two stacks as two 32-bit shift registers (push: shift left, pop:
//     shift right), so nothing is indexed dynamically and nothing goes to
//     scratch.  An unknown entry holds value 0, which makes the Kleene forms
//     plain bit operations (see kAnd / kOr below);
//   * values are loaded at the column's own width, coalesced over the wave,
//     integers widened to int64 and floats to double: the compares are the
//     ones Arrow makes (an int8 column against an int64 literal in int64, a
//     float32 column against a double literal in double);
//   * set membership is a binary search of the op's sorted slice of one int64
//     pool.
//
// The pool is the one input that is neither a kernel argument nor a caller's
// device buffer: fx_pred_eval checks it on the host (sorted slices) and copies
// it into one of a few device slots it keeps per device (under that device's
// own lock), each guarded by an event recorded behind the kernel that reads it.
#include <map>
#include <mutex>

#include "fx_internal.h"

namespace fx {
namespace {

constexpr int kPredThreads = 256;
constexpr int kPoolSlots = 4;

struct PredArgs {
  fx_pred_column cols[FX_PRED_MAX_COLUMNS];
  fx_pred_op ops[FX_PRED_MAX_OPS];
  int nops;
  const int64_t* pool;      // device copy of the set pool (null: no is_in)
  int64_t n, row0;
  const uint32_t* and_mask;
  uint32_t* out;
  int64_t words;
  unsigned long long* count;
};

__device__ __forceinline__ bool is_float(int dtype) { return dtype >= FX_PRED_F32; }

// the column's value at staged row i, integers as int64, floats as the bits of a double
__device__ __forceinline__ int64_t load_value(const void* p, int dtype, int64_t i) {
  switch (dtype) {
    case FX_PRED_I8: return static_cast<const int8_t*>(p)[i];
    case FX_PRED_I16: return static_cast<const int16_t*>(p)[i];
    case FX_PRED_I32: return static_cast<const int32_t*>(p)[i];
    case FX_PRED_I64: return static_cast<const int64_t*>(p)[i];
    case FX_PRED_U8: return static_cast<const uint8_t*>(p)[i];
    case FX_PRED_U16: return static_cast<const uint16_t*>(p)[i];
    case FX_PRED_U32: return static_cast<const uint32_t*>(p)[i];
    case FX_PRED_F32: return __double_as_longlong((double)static_cast<const float*>(p)[i]);
    default: return static_cast<const int64_t*>(p)[i];  // FX_PRED_F64: the bits
  }
}

template <typename T>
__device__ __forceinline__ bool compare(int op, T x, T y) {
  switch (op) {
    case FX_PRED_EQ: return x == y;
    case FX_PRED_NE: return x != y;
    case FX_PRED_LT: return x < y;
    case FX_PRED_LE: return x <= y;
    case FX_PRED_GT: return x > y;
    default: return x >= y;  // FX_PRED_GE
  }
}

__device__ __forceinline__ bool in_set(const int64_t* __restrict__ s, int len, int64_t x) {
  int lo = 0, hi = len;  // first entry >= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo < len && s[lo] == x;
}

__global__ void __launch_bounds__(kPredThreads) pred_kernel(const PredArgs a) {
  __shared__ unsigned int wsum[kPredThreads / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned int kept = 0;
  for (int64_t base = (int64_t)blockIdx.x * kPredThreads; base < a.n;
       base += (int64_t)gridDim.x * kPredThreads) {
    const int64_t r = base + threadIdx.x;
    bool bit = false;
    if (r < a.n) {
      const int64_t i = a.row0 + r;  // staged row
      uint32_t val = 0, known = 0;   // bit 0: top of the stack
      for (int pc = 0; pc < a.nops; ++pc) {
        const fx_pred_op& op = a.ops[pc];
        if (op.op <= FX_PRED_IS_VALID) {  // leaves push
          const fx_pred_column& c = a.cols[op.column];
          const bool valid = c.valid == nullptr || ((c.valid[i >> 5] >> (i & 31)) & 1u);
          bool v, k = true;
          if (op.op == FX_PRED_IS_VALID) {
            v = valid;
          } else if (op.op == FX_PRED_IS_NULL) {
            v = !valid;
            if (valid && op.imm != 0 && is_float(c.dtype)) {  // nan_is_null
              const double x = __longlong_as_double(load_value(c.values, c.dtype, i));
              v = x != x;
            }
          } else {
            v = false;
            if (valid) {
              const int64_t x = load_value(c.values, c.dtype, i);
              if (op.op == FX_PRED_IS_IN) {
                v = in_set(a.pool + op.set_offset, op.set_length, x);
              } else if (is_float(c.dtype)) {
                v = compare<double>(op.op, __longlong_as_double(x), __longlong_as_double(op.imm));
              } else {
                v = compare<int64_t>(op.op, x, op.imm);
              }
            }
            k = valid || op.op == FX_PRED_IS_IN;  // is_in of a null is false, a compare null
          }
          val = (val << 1) | (uint32_t)(v && k);
          known = (known << 1) | (uint32_t)k;
        } else if (op.op == FX_PRED_NOT) {
          val = (val & ~1u) | (~val & known & 1u);
        } else {
          const uint32_t va = val & 1u, vb = (val >> 1) & 1u;
          const uint32_t ka = known & 1u, kb = (known >> 1) & 1u;
          uint32_t v, k;
          if (op.op == FX_PRED_AND) {  // false and anything is false
            v = va & vb;
            k = (ka & kb) | (ka & ~va) | (kb & ~vb);
          } else {                     // kOr: true or anything is true
            v = va | vb;
            k = (ka & kb) | va | vb;
          }
          val = ((val >> 2) << 1) | v;
          known = ((known >> 2) << 1) | (k & 1u);
        }
      }
      bit = val & 1u;  // a null result drops the row
      if (a.and_mask != nullptr) bit = bit && ((a.and_mask[r >> 5] >> (r & 31)) & 1u);
    }
    const uint64_t b = __ballot(bit);
    const int64_t w0 = (r - lane) >> 5;
    if (lane == 0 && w0 < a.words) a.out[w0] = (uint32_t)b;
    if (lane == 32 && w0 + 1 < a.words) a.out[w0 + 1] = (uint32_t)(b >> 32);
    kept += (unsigned int)__popcll(b);
  }
  if (a.count == nullptr) return;
  if (lane == 0) wsum[wid] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int t = 0;
    for (int w = 0; w < kPredThreads / 64; ++w) t += wsum[w];
    if (t) atomicAdd(a.count, (unsigned long long)t);
  }
}

// Device copies of set pools: per device a ring of slots, each reused only
// once the kernel that read it last has run (its event).
struct PoolSlot {
  int64_t* dev = nullptr;
  hipEvent_t done = nullptr;
};
struct PoolRing {
  std::mutex mu;  // one enqueue at a time per device: slot choice, copy, launch, event
  PoolSlot slot[kPoolSlots];
  int next = 0;
};
std::mutex g_pools_mu;  // the map only
std::map<int, PoolRing> g_pools;

// the ring of the stream's device (the calling thread's current device, as
// every entry point; std::map keeps the reference valid)
int pool_ring(PoolRing** out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) {
    set_error("hipGetDevice: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  std::lock_guard<std::mutex> lk(g_pools_mu);
  *out = &g_pools[dev];
  return FX_OK;
}

// ring.mu held
int stage_pool(PoolRing& ring, const int64_t* host, int64_t len, hipStream_t stream,
               PoolSlot** out) {
  hipError_t e;
  PoolSlot& s = ring.slot[ring.next];
  ring.next = (ring.next + 1) % kPoolSlots;
  if (s.dev == nullptr) {
    e = hipMalloc(reinterpret_cast<void**>(&s.dev), (size_t)FX_PRED_MAX_POOL * 8);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
    if (e != hipSuccess) {
      if (s.dev != nullptr) (void)hipFree(s.dev);
      s.dev = nullptr;
      set_error("predicate set pool: %s", hipGetErrorString(e));
      return FX_EHIP;
    }
  } else {
    e = hipEventSynchronize(s.done);
    if (e != hipSuccess) {
      set_error("predicate set pool: %s", hipGetErrorString(e));
      return FX_EHIP;
    }
  }
  e = hipMemcpyAsync(s.dev, host, (size_t)len * 8, hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) {
    set_error("predicate set pool copy: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  *out = &s;
  return FX_OK;
}

int refuse(const char* what, int at) {
  set_error("fx_pred_eval: %s (instruction %d)", what, at);
  return FX_EINVAL;
}

// the program is well formed: *pool_len = entries of set_pool it reads
int validate(const fx_pred_column* cols, int ncols, const fx_pred_op* ops, int nops,
             const int64_t* set_pool, int64_t* pool_len) {
  for (int c = 0; c < ncols; ++c) {
    if (cols[c].dtype < FX_PRED_I8 || cols[c].dtype > FX_PRED_F64) return refuse("bad dtype", -1);
    if (cols[c].values == nullptr) return refuse("column without values", -1);
  }
  int depth = 0;
  int64_t used = 0;
  for (int i = 0; i < nops; ++i) {
    const fx_pred_op& op = ops[i];
    if (op.op < FX_PRED_EQ || op.op > FX_PRED_NOT) return refuse("unknown instruction", i);
    if (op.op <= FX_PRED_IS_VALID) {
      if (op.column < 0 || op.column >= ncols) return refuse("column index out of range", i);
      const bool flt = cols[op.column].dtype >= FX_PRED_F32;
      if (op.op == FX_PRED_IS_NULL && op.imm != 0 && op.imm != 1)
        return refuse("is_null flag", i);
      if (op.op == FX_PRED_IS_IN) {
        if (flt) return refuse("is_in on a float column", i);
        if (op.set_offset < 0 || op.set_length < 1 || op.set_length > FX_PRED_MAX_SET ||
            (int64_t)op.set_offset + op.set_length > FX_PRED_MAX_POOL || set_pool == nullptr)
          return refuse("set slice out of range", i);
        const int64_t* s = set_pool + op.set_offset;
        for (int j = 1; j < op.set_length; ++j)
          if (s[j - 1] >= s[j]) return refuse("set slice not sorted", i);
        if ((int64_t)op.set_offset + op.set_length > used)
          used = (int64_t)op.set_offset + op.set_length;
      }
      ++depth;
    } else {
      const int need = op.op == FX_PRED_NOT ? 1 : 2;
      if (depth < need) return refuse("stack underflow", i);
      depth -= need - 1;
    }
  }
  if (depth != 1) return refuse("final stack depth is not 1", nops);
  *pool_len = used;
  return FX_OK;
}

}  // namespace
}  // namespace fx

using namespace fx;

extern "C" {

int fx_pred_limits(int* max_columns, int* max_ops, int* max_set, int* max_pool) {
  if (max_columns != nullptr) *max_columns = FX_PRED_MAX_COLUMNS;
  if (max_ops != nullptr) *max_ops = FX_PRED_MAX_OPS;
  if (max_set != nullptr) *max_set = FX_PRED_MAX_SET;
  if (max_pool != nullptr) *max_pool = FX_PRED_MAX_POOL;
  return FX_OK;
}

int fx_pred_eval(const fx_pred_column* cols, int ncols, const fx_pred_op* ops, int nops,
                 const int64_t* set_pool, int64_t n, int64_t row0, const uint32_t* and_mask,
                 uint32_t* out_mask, uint64_t* out_count, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (n < 0 || row0 < 0 || ncols < 0 || ncols > FX_PRED_MAX_COLUMNS || nops < 1 ||
      nops > FX_PRED_MAX_OPS || ops == nullptr || (ncols > 0 && cols == nullptr) ||
      (n > 0 && out_mask == nullptr)) {
    set_error("fx_pred_eval: invalid arguments");
    return FX_EINVAL;
  }
  int64_t pool_len = 0;
  int rc = validate(cols, ncols, ops, nops, set_pool, &pool_len);
  if (rc) return rc;
  if (n == 0) {
    if (out_count != nullptr) {
      hipError_t e = hipMemsetAsync(out_count, 0, 8, stream);
      if (e != hipSuccess) {
        set_error("predicate memset: %s", hipGetErrorString(e));
        return FX_EHIP;
      }
    }
    return FX_OK;
  }
  PredArgs a = {};
  for (int c = 0; c < ncols; ++c) a.cols[c] = cols[c];
  for (int i = 0; i < nops; ++i) a.ops[i] = ops[i];
  a.nops = nops;
  a.n = n;
  a.row0 = row0;
  a.and_mask = and_mask;
  a.out = out_mask;
  a.words = (n + 31) / 32;
  a.count = reinterpret_cast<unsigned long long*>(out_count);
  int cus = 0;
  rc = device_cus(&cus);
  if (rc) return rc;
  int64_t blocks = (n + kPredThreads - 1) / kPredThreads;
  if (blocks > (int64_t)cus * 8) blocks = (int64_t)cus * 8;
  std::unique_lock<std::mutex> lk;
  PoolSlot* slot = nullptr;
  if (pool_len > 0) {
    PoolRing* ring = nullptr;
    rc = pool_ring(&ring);
    if (rc) return rc;
    lk = std::unique_lock<std::mutex>(ring->mu);
    rc = stage_pool(*ring, set_pool, pool_len, stream, &slot);
    if (rc) return rc;
    a.pool = slot->dev;
  }
  // the count is cleared last: every failure above leaves the output untouched
  if (out_count != nullptr) {
    hipError_t e = hipMemsetAsync(out_count, 0, 8, stream);
    if (e != hipSuccess) {
      set_error("predicate memset: %s", hipGetErrorString(e));
      return FX_EHIP;
    }
  }
  hipLaunchKernelGGL(pred_kernel, dim3((unsigned)blocks), dim3(kPredThreads), 0, stream, a);
  rc = check_launch("pred_kernel");
  if (slot != nullptr) {
    hipError_t e = hipEventRecord(slot->done, stream);
    if (rc == FX_OK && e != hipSuccess) {
      set_error("predicate set pool event: %s", hipGetErrorString(e));
      rc = FX_EHIP;
    }
  }
  return rc;
}

}  // extern "C"
