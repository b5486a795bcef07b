// The batched filter with 64-query tiles and K chunks of 64, namespace
// fx::q64: batches of <= 64 queries (e.g. concurrent requests coalesced by the
// Flight server, fenix_amd/coalesce.py) re-read and multiply a quarter of the
// padding of a 256-query tile.  Holds
//   filter_kernel<float / _Float16, ., false>   both row types (filter/staged.inc)
//   filter_img2_kernel<.>                       tiled fp16 images (filter/img2.inc)
// and in diagnostic builds filter_kernel<_Float16, ., true> (row-major fp16
// images) and ring_kernel (filter/ring.inc).  launch_filter (knn_filter.hip)
// sends it every batch of <= 64 queries but int8 images (the q64i variant).
#include "fx_internal.h"

#include <type_traits>

#define FX_FILTER_BQ 64
#define FX_FILTER_BK 64

namespace fx {
namespace q64 {

#include "filter/tile.inc"
#include "filter/staged.inc"
#include "filter/img2.inc"
#ifdef FX_DIAG_BUILD
#include "filter/ring.inc"
#endif

int launch(const FilterArgs& a, int metric, hipStream_t stream) {
  if (a.num_tiles <= 0) return FX_OK;
  if (a.rowinfo != nullptr && image_tiled())  // the image in MFMA fragment order
    return launch_img2(a, metric, stream);
#ifdef FX_DIAG_BUILD
  if (filter_ring()) return launch_ring_rows(a, metric, stream);
#endif
  return launch_staged<kRowsF32 | kRowsF16>(a, metric, stream);
}

}  // namespace q64
}  // namespace fx
