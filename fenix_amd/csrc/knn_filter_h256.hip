// The batched filter for fp16 rows with 256-query tiles and 64-wide K chunks,
// namespace fx::h256: a row's K chunk is then 128 B, one whole cache line per
// row and load, where 32-wide chunks fetch every line twice.  Holds
//   filter_kernel<_Float16, ., false>     fp16 rows (filter/staged.inc)
// and in diagnostic builds filter_kernel<_Float16, ., true> (row-major fp16
// images) and ring_kernel (filter/ring.inc).  launch_filter (knn_filter.hip)
// sends it fp16 rows (and row-major images) of more than 128 queries; tiled
// images go to the q256 variant (this one measured 7 % slower on them).
// FX_H256_BK / FX_H256_WAVES are tuning knobs of this compilation only.
#include "fx_internal.h"

#include <type_traits>

#ifndef FX_H256_BK
#define FX_H256_BK 64
#endif
#define FX_FILTER_BQ 256
#define FX_FILTER_BK FX_H256_BK
#ifdef FX_H256_WAVES
#define FX_FILTER_WAVES FX_H256_WAVES
#endif

namespace fx {
namespace h256 {

#include "filter/tile.inc"
#include "filter/staged.inc"
#ifdef FX_DIAG_BUILD
#include "filter/ring.inc"
#endif

int launch(const FilterArgs& a, int metric, hipStream_t stream) {
  if (a.num_tiles <= 0) return FX_OK;
  if (a.rowinfo != nullptr && image_tiled()) {
    set_error("filter: the tiled image is not compiled into this variant");
    return FX_EUNSUPPORTED;
  }
#ifdef FX_DIAG_BUILD
  if (filter_ring()) return launch_ring_rows(a, metric, stream);
#endif
  return launch_staged<kRowsF16>(a, metric, stream);
}

}  // namespace h256
}  // namespace fx
