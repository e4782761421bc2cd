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

// 4 queries per wave, 4 waves, 4 row tiles: the shape tiled_task_body is written for (scan_bucket.hip: TILED_QB / 4, TILED_TPS)
template <int STORE, bool WIDEK>
static const void *bscanf_of(int metric) {
    if (metric == NLSH_METRIC_L2_EPS) return (const void *)bscanf_kernel<NLSH_METRIC_L2_EPS, 4, 4, 4, STORE, WIDEK>;
    if (metric == NLSH_METRIC_L2_EPS_FOLDED) return (const void *)bscanf_kernel<NLSH_METRIC_L2_EPS_FOLDED, 4, 4, 4, STORE, WIDEK>;
    return (const void *)bscanf_kernel<NLSH_METRIC_COSINE, 4, 4, 4, STORE, WIDEK>;
}
const void *filtered_scan_kernel_of(int storage, int metric, bool wide) {
    if (storage == NLSH_STORE_F16) return wide ? bscanf_of<NLSH_STORE_F16, true>(metric) : bscanf_of<NLSH_STORE_F16, false>(metric);
    if (storage == NLSH_STORE_U8) return wide ? bscanf_of<NLSH_STORE_U8, true>(metric) : bscanf_of<NLSH_STORE_U8, false>(metric);
    return wide ? bscanf_of<NLSH_STORE_F32, true>(metric) : bscanf_of<NLSH_STORE_F32, false>(metric);
}

}  // namespace nlsh
