// The tiled scan behind a row filter (nlsh_scan_topk_cells_phase_filtered): the instantiations of bscanf_kernel (scan_bucket_tiled.h) for
// every storage.  A translation unit of its own, and so a code object of its own, like scan_bucket_typed.hip: the kernels of scan_bucket.hip
// and scan_bucket_typed.hip are compiled from units that instantiate nothing filtered and stay the code they were before the filter
// existed (profiles/row_filter.txt).
// the phase trace (tools/scan_trace.py) is the float32 kernels': its buffer lives in scan_bucket.hip
#undef NLSH_SCAN_TRACE
#undef NLSH_SCAN_TRACE_CLOCK
#undef NLSH_SCAN_TRACE_EPILOGUE
#undef NLSH_SCAN_TRACE_HWID
#include "scan_bucket_args.h"
#include "scan_bucket_tiled.h"

namespace nlsh {

template <int STORE, bool WIDEK>
static const void *bscanf_of(int metric) { return NLSH_TILED_KERNEL(bscanf_kernel, metric, STORE, WIDEK); }
const void *filtered_scan_kernel_of(int storage, int metric, bool wide) {
    if (storage == NLSH_STORE_F16) return wide ? bscanf_of<NLSH_STORE_F16, true>(metric) : bscanf_of<NLSH_STORE_F16, false>(metric);
    if (storage == NLSH_STORE_U8) return wide ? bscanf_of<NLSH_STORE_U8, true>(metric) : bscanf_of<NLSH_STORE_U8, false>(metric);
    return wide ? bscanf_of<NLSH_STORE_F32, true>(metric) : bscanf_of<NLSH_STORE_F32, false>(metric);
}

}  // namespace nlsh
