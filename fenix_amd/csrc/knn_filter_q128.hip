// The batched filter with 128-query tiles and K chunks of 32 (one 16-B query
// piece per thread), namespace fx::q128: batches of 65..128 queries, which a
// 256-query tile would half pad.  Holds
//   filter_kernel<float / _Float16, ., false>   both row types (filter/staged.inc)
//   filter_img3_kernel<., false / true>         tiled fp16 / int8 images (filter/img3.inc)
//   filter_img6_kernel<., false / true>         int8 images, a resident slice (filter/img6.inc);
//                                               true: per-query row masks (FilterArgs::qmask)
// and in diagnostic builds filter_kernel<_Float16, ., true> (row-major fp16
// images) and ring_kernel (filter/ring.inc).  launch_filter (knn_filter.hip)
// sends launch() every batch of 65..128 queries, and launch_img6() the int8
// images of such a batch whose slice fits (img6_fits; with option img6 = 2
// those of larger batches too), and every batch of more than 64 queries with
// per-query row masks whose slice fits (img6_fits_qmask), as slices of 128.
#include "fx_internal.h"

#include <type_traits>

#define FX_FILTER_BQ 128
#define FX_FILTER_BK 32

namespace fx {
namespace q128 {

#include "filter/tile.inc"
#include "filter/staged.inc"
#include "filter/tiled.inc"
#include "filter/img3.inc"
#include "filter/img6.inc"  // launch_img6(), img6_fits()
#ifdef FX_DIAG_BUILD
#include "filter/ring.inc"
#endif

int launch(const FilterArgs& a, int metric, hipStream_t stream) {
  if (a.num_tiles <= 0) return FX_OK;
  if (a.rowinfo != nullptr && image_tiled())  // the image in MFMA fragment order
    return launch_img3(a, metric, stream);
#ifdef FX_DIAG_BUILD
  if (filter_ring()) return launch_ring_rows(a, metric, stream);
#endif
  return launch_staged<kRowsF32 | kRowsF16>(a, metric, stream);
}

}  // namespace q128
}  // namespace fx
