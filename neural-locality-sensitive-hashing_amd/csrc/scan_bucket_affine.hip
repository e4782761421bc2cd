// The tiled scan over an sq8 corpus (nlsh_scan_topk_cells_phase_sq8): the instantiations of bscana_kernel (scan_bucket_tiled.h) -- uint8
// codes decoded per dimension, deq(c, j) = float(c) * step[j] + lo[j], where the tile is written.  A translation unit of its own, and so
// a code object of its own, like scan_bucket_typed.hip: the kernels of scan_bucket.hip, scan_bucket_typed.hip, scan_bucket_filtered.hip
// and scan_bucket_range.hip are compiled from units that instantiate nothing affine and stay the code they were before the affine
// form existed (profiles/sq8_storage.txt).
// the phase trace (tools/scan_trace.py) is the float32 kernels': its buffer lives in scan_bucket.hip
#undef NLSH_SCAN_TRACE
#undef NLSH_SCAN_TRACE_CLOCK
#undef NLSH_SCAN_TRACE_EPILOGUE
#undef NLSH_SCAN_TRACE_HWID
#include "scan_bucket_args.h"
#include "scan_bucket_tiled.h"

namespace nlsh {

const void *affine_scan_kernel_of(int metric, bool wide) {
    return wide ? NLSH_TILED_KERNEL(bscana_kernel, metric, true) : NLSH_TILED_KERNEL(bscana_kernel, metric, false);
}

}  // namespace nlsh
