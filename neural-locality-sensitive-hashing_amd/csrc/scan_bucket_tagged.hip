// The tiled scan behind per-query tag filters (nlsh_scan_topk_cells_phase_tagged / _sq8_tagged): the instantiations of bscang_kernel
// (scan_bucket_tiled.h) for every storage, sq8 among them.  A translation unit of its own, and so a code object of its own, like
// scan_bucket_filtered.hip: the kernels of scan_bucket.hip, scan_bucket_typed.hip, scan_bucket_filtered.hip, scan_bucket_range.hip and
// scan_bucket_affine.hip are compiled from units that instantiate nothing tagged and stay the code they were before the tags existed
// (profiles/row_tags.txt).
// the phase trace (tools/scan_trace.py) is the float32 kernels': its buffer lives in scan_bucket.hip
#undef NLSH_SCAN_TRACE
#undef NLSH_SCAN_TRACE_CLOCK
#undef NLSH_SCAN_TRACE_EPILOGUE
#undef NLSH_SCAN_TRACE_HWID
#include "scan_bucket_args.h"
#include "scan_bucket_tiled.h"

namespace nlsh {

template <int STORE, bool WIDEK>
static const void *bscang_of(int metric) { return NLSH_TILED_KERNEL(bscang_kernel, metric, STORE, WIDEK); }
// storage: NLSH_STORE_F32 | F16 | U8, or NLSH_STORE_SQ8 for a call that carries a quantiser
const void *tagged_scan_kernel_of(int storage, int metric, bool wide) {
    if (storage == NLSH_STORE_SQ8) return wide ? bscang_of<NLSH_STORE_SQ8, true>(metric) : bscang_of<NLSH_STORE_SQ8, false>(metric);
    if (storage == NLSH_STORE_F16) return wide ? bscang_of<NLSH_STORE_F16, true>(metric) : bscang_of<NLSH_STORE_F16, false>(metric);
    if (storage == NLSH_STORE_U8) return wide ? bscang_of<NLSH_STORE_U8, true>(metric) : bscang_of<NLSH_STORE_U8, false>(metric);
    return wide ? bscang_of<NLSH_STORE_F32, true>(metric) : bscang_of<NLSH_STORE_F32, false>(metric);
}

}  // namespace nlsh
