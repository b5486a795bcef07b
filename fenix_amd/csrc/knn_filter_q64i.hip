// The tiled-image kernels with 64-query tiles and K chunks of 32 (as the
// tiled images need), namespace fx::q64i: int8 filter images for batches of
// <= 64 queries, which a 256-query tile would multiply mostly as padding.
// Holds
//   filter_img3_kernel<., false / true>   tiled fp16 / int8 images (filter/img3.inc)
//   filter_img6_kernel<., false / true>   int8 images, a resident slice (filter/img6.inc);
//                                         true: per-query row masks (FilterArgs::qmask)
// and in diagnostic builds ring_kernel (filter/ring.inc); no register-staged
// kernel (fp16 and f32 rows of <= 64 queries take the q64 variant).
// launch_filter (knn_filter.hip) sends it the int8 images of batches of <= 64
// queries: launch_img6() when the slice fits (img6_fits), else launch(); with
// per-query row masks also larger batches, as slices of 64, where a 128-query
// slice does not fit the row length (filter_qmask_kind).
#include "fx_internal.h"

#include <type_traits>

#define FX_FILTER_BQ 64
#define FX_FILTER_BK 32

namespace fx {
namespace q64i {

#include "filter/tile.inc"
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
  set_error("filter: row type not compiled into this variant");
  return FX_EUNSUPPORTED;
}

}  // namespace q64i
}  // namespace fx
