// Runtime helpers shared by every unit: the thread's last error, the
// process options, and per-device properties cached on first use.  No kernel.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <set>
#include <tuple>
#include <utility>

#include "fx_internal.h"

namespace fx {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

const char* last_error() { return g_err; }

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return FX_EHIP;
  }
  return FX_OK;
}

// ----------------------------------------------------------------- options --
#define FX_OPTION_NAME(id, name, dflt) name,
#define FX_OPTION_DEFAULT(id, name, dflt) {dflt},
static const char* const kOptNames[kOptCount] = {FX_OPTIONS(FX_OPTION_NAME)};
static std::atomic<int64_t> g_opts[kOptCount] = {FX_OPTIONS(FX_OPTION_DEFAULT)};
#undef FX_OPTION_NAME
#undef FX_OPTION_DEFAULT

int64_t option(Option o) { return g_opts[o].load(std::memory_order_relaxed); }

static int option_index(const char* name) {
  for (int i = 0; name != nullptr && i < kOptCount; ++i)
    if (strcmp(name, kOptNames[i]) == 0) return i;
  return -1;
}

static int unknown_option(const char* name) {
  set_error("unknown option %s", name ? name : "(null)");
  return FX_EINVAL;
}

int set_option(const char* name, int64_t value) {
  const int i = option_index(name);
  if (i < 0) return unknown_option(name);
  if (i == kOptI8MaxK && (value < 0 || value > kSelectMaxK)) {
    set_error("option i8_max_k=%lld outside [0, %d] (the select kernel's LDS bound)",
              (long long)value, kSelectMaxK);
    return FX_EINVAL;
  }
  g_opts[i].store(value, std::memory_order_relaxed);
  return FX_OK;
}

int get_option(const char* name, int64_t* out) {
  const int i = option_index(name);
  if (i < 0 || out == nullptr) return unknown_option(name);
  *out = option((Option)i);
  return FX_OK;
}

#ifdef FX_DIAG_BUILD
int diag_env(const char* name, int dflt) {
  const char* env = getenv(name);
  return env != nullptr ? atoi(env) : dflt;
}
#endif

// ------------------------------------------------------- device properties --
static std::mutex g_mu;

static int current_device(int* dev) {
  hipError_t e = hipGetDevice(dev);
  if (e != hipSuccess) {
    set_error("hipGetDevice: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  return FX_OK;
}

bool device_present() {
  static std::atomic<bool> seen{false};  // (a device does not go away; its absence is re-checked)
  if (seen.load(std::memory_order_relaxed)) return true;
  int count = 0;
  const bool ok = hipGetDeviceCount(&count) == hipSuccess && count > 0;
  if (ok) seen.store(true, std::memory_order_relaxed);
  return ok;
}

int device_cus(int* out) {
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  static std::map<int, int> cache;
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = cache.find(dev);
  if (it != cache.end()) {
    *out = it->second;
    return FX_OK;
  }
  int cus = 0;
  hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) {
    set_error("hipDeviceGetAttribute: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  cache[dev] = cus;
  *out = cus;
  return FX_OK;
}

// The dynamic-LDS limit above 64 KB is a per-device function attribute: set
// it once per (device, kernel), so a table sharded over several devices can
// launch the same kernel on each of them.
int allow_lds(const void* fn) {
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  static std::set<std::pair<int, const void*>> done;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!done.insert(std::make_pair(dev, fn)).second) return FX_OK;
  // the dynamic share of the 160 KB: whatever the kernel's static __shared__
  // variables leave
  hipFuncAttributes at = {};
  hipError_t e = hipFuncGetAttributes(&at, fn);
  if (e != hipSuccess) {
    done.erase(std::make_pair(dev, fn));
    set_error("hipFuncGetAttributes: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                          160 * 1024 - (int)at.sharedSizeBytes);
  if (e != hipSuccess) {
    done.erase(std::make_pair(dev, fn));
    set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  return FX_OK;
}

int kernel_occupancy(const void* fn, int block, size_t smem, int* out) {
  if (smem > 64 * 1024) {
    int rc = allow_lds(fn);
    if (rc) return rc;
  }
  int dev = 0;
  if (int rc = current_device(&dev)) return rc;
  static std::map<std::tuple<int, const void*, size_t>, int> cache;
  std::lock_guard<std::mutex> lk(g_mu);
  auto key = std::make_tuple(dev, fn, smem);
  auto it = cache.find(key);
  if (it != cache.end()) {
    *out = it->second;
    return FX_OK;
  }
  int nb = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, block, smem);
  if (e != hipSuccess) {
    set_error("hipOccupancyMaxActiveBlocksPerMultiprocessor: %s", hipGetErrorString(e));
    return FX_EHIP;
  }
  cache[key] = nb;
  *out = nb;
  return FX_OK;
}

}  // namespace fx
