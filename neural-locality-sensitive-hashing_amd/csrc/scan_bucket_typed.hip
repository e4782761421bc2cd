// The tiled scan over a float16 / uint8 corpus (NLSH_STORE_F16, NLSH_STORE_U8): the instantiations of bscant_kernel (scan_bucket_tiled.h).
// A translation unit of its own, and so a code object of its own: the float32 kernels of scan_bucket.hip are compiled from a unit that
// instantiates nothing typed and stay, byte for byte, the code they were before typed storage existed (profiles/corpus_storage.txt).
// the phase trace (tools/scan_trace.py) is the float32 kernels': its buffer lives in scan_bucket.hip
#undef NLSH_SCAN_TRACE
#undef NLSH_SCAN_TRACE_CLOCK
#undef NLSH_SCAN_TRACE_EPILOGUE
#undef NLSH_SCAN_TRACE_HWID
#include "scan_bucket_args.h"
#include "scan_bucket_tiled.h"

namespace nlsh {

template <int STORE, bool WIDEK>
static const void *bscant_of(int metric) { return NLSH_TILED_KERNEL(bscant_kernel, metric, STORE, WIDEK); }
const void *typed_scan_kernel_of(int storage, int metric, bool wide) {
    if (storage == NLSH_STORE_F16) return wide ? bscant_of<NLSH_STORE_F16, true>(metric) : bscant_of<NLSH_STORE_F16, false>(metric);
    return wide ? bscant_of<NLSH_STORE_U8, true>(metric) : bscant_of<NLSH_STORE_U8, false>(metric);
}

}  // namespace nlsh
