// The batched filter with 256-query tiles and K chunks of 32, namespace
// fx::q256.  Holds
//   filter_kernel<float, ., false>        f32 rows (filter/staged.inc)
//   filter_img3_kernel<., false / true>   tiled fp16 / int8 images (filter/img3.inc)
//   filter_img8_kernel<., 1..6, .>        int8 images, d <= 768 (filter/img8.inc)
// and in diagnostic builds ring_kernel (filter/ring.inc).  launch_filter
// (knn_filter.hip) sends it batches of more than 128 queries: f32 rows, every
// tiled image, and (diagnostic builds, FX_FILTER_RING=1) every row type.
// FX_Q256_WAVES is a tuning knob of this compilation only.
#include "fx_internal.h"

#include <type_traits>

#define FX_FILTER_BQ 256
#define FX_FILTER_BK 32
#ifdef FX_Q256_WAVES
#define FX_FILTER_WAVES FX_Q256_WAVES
#endif

namespace fx {
namespace q256 {

#include "filter/tile.inc"
#include "filter/staged.inc"
#include "filter/tiled.inc"
#include "filter/img3.inc"
#include "filter/img8.inc"
#ifdef FX_DIAG_BUILD
#include "filter/ring.inc"
#endif

int launch(const FilterArgs& a, int metric, hipStream_t stream) {
  if (a.num_tiles <= 0) return FX_OK;
  if (a.rowinfo != nullptr && image_tiled())  // the image in MFMA fragment order
    return img8_serves(a) ? launch_img8(a, metric, stream) : launch_img3(a, metric, stream);
#ifdef FX_DIAG_BUILD
  if (filter_ring()) return launch_ring_rows(a, metric, stream);
#endif
  return launch_staged<kRowsF32>(a, metric, stream);
}

}  // namespace q256
}  // namespace fx
