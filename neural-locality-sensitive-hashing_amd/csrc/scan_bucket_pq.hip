// The tiled scan over a product-quantised corpus (nlsh_scan_topk_cells_phase_pq): the instantiations of bscanq_kernel
// (scan_bucket_tiled.h) -- M code bytes per row, a staged 16-byte chunk gathered from the codebook where the tile is written.  A
// translation unit of its own, and so a code object of its own, like scan_bucket_affine.hip: the kernels of the other scan units are
// compiled from units that instantiate nothing product-quantised and stay the code they were (profiles/pq_storage.txt).
// the phase trace (tools/scan_trace.py) is the float32 kernels': its buffer lives in scan_bucket.hip
#undef NLSH_SCAN_TRACE
#undef NLSH_SCAN_TRACE_CLOCK
#undef NLSH_SCAN_TRACE_EPILOGUE
#undef NLSH_SCAN_TRACE_HWID
#include "scan_bucket_args.h"
#include "scan_bucket_tiled.h"

namespace nlsh {

const void *pq_scan_kernel_of(int metric, bool wide) {
    return wide ? NLSH_TILED_KERNEL(bscanq_kernel, metric, true) : NLSH_TILED_KERNEL(bscanq_kernel, metric, false);
}

}  // namespace nlsh
