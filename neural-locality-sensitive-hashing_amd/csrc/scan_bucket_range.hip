// Radius (range) queries on the tiled scan (nlsh_range_count / nlsh_range_fill): the instantiations of bscanr_kernel (scan_bucket_tiled.h)
// for every metric and storage, the two small kernels around them and the two calls.  A translation unit of its own, and so a code
// object of its own, like scan_bucket_filtered.hip: the kernels of scan_bucket.hip, scan_bucket_typed.hip and scan_bucket_filtered.hip
// are compiled from units that instantiate nothing of this and stay the code they were (profiles/range_query.txt).
//
// Flow (two calls, one host read between them -- the length of the output is not known before the scan has run):
//   nlsh_range_count   PLAN phase of a k = 1 call (bplan, bscan, bscatter: scan_bucket.hip; a k = 1 partial area costs nothing and is never
//                      written), candidate counts from the plan's records, then bscanr_kernel in count mode: one atomic add per
//                      (task, slot) list with a hit
//   host               reads the counts, makes their exclusive prefix sum and allocates the outputs
//   nlsh_range_fill    bscanr_kernel in fill mode on the plan the count call left in the workspace (same distances, same hits: a list
//                      reserves its slots of the query's segment with one atomic add and stores its keys), rocPRIM's segmented radix
//                      sort of the 64-bit keys per query, and the unpack of the sorted keys into distances and ids
// Keys within a query are distinct (distinct ids, every (query, bucket) pair scanned once), so the sorted result does not depend on the
// order of the atomics.
// the phase trace (tools/scan_trace.py) is the float32 kernels': its buffer lives in scan_bucket.hip
#undef NLSH_SCAN_TRACE
#undef NLSH_SCAN_TRACE_CLOCK
#undef NLSH_SCAN_TRACE_EPILOGUE
#undef NLSH_SCAN_TRACE_HWID
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "scan_bucket_args.h"
#include "scan_bucket_tiled.h"

namespace nlsh {

template <int STORE>
static const void *bscanr_of(int metric) { return NLSH_TILED_KERNEL(bscanr_kernel, metric, STORE); }
static const void *range_scan_kernel_of(int storage, int metric) {
    if (storage == NLSH_STORE_F16) return bscanr_of<NLSH_STORE_F16>(metric);
    if (storage == NLSH_STORE_U8) return bscanr_of<NLSH_STORE_U8>(metric);
    return bscanr_of<NLSH_STORE_F32>(metric);
}

// n_candidates of every query = rows of its probed buckets, before the radius and before the filter: the sum merge_query takes over the
// records bscatter left per (query, probe) -- zeros for slots past the key count, repeated keys and keys without a bucket
__global__ __launch_bounds__(256) void range_ncand_kernel(const int4 *prec, long long Q, int P, int32_t *out_ncand) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    int c = 0;
    for (int p = 0; p < P; ++p) c += prec[q * P + p].z;
    out_ncand[q] = c;
}

// sorted keys -> distances and ids (the top-k merges' merge_finish, without padding: every key is a candidate's)
__global__ __launch_bounds__(256) void range_unpack_kernel(const uint64_t *keys, long long total, float *out_dist, int32_t *out_idx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint64_t key = keys[i];
    if (out_dist) out_dist[i] = float_from_mono((uint32_t)(key >> 32));
    out_idx[i] = (int32_t)(uint32_t)key;
}

struct RangeSortWs {
    size_t unsorted, sorted, tmp, tmp_bytes, total;
};
// Host arithmetic only, so that a caller can size the workspace without a device: the sort's own temporary storage is BOUNDED here --
// rocPRIM's segmented radix sort with separate input and output keeps one more copy of the keys (8 * total), two segment-index arrays
// and two counters (8 * Q + 8) and, in a union with the key copy, the storage of its three-way partition of the segment indices (a few
// look-back words per block of segments) -- and nlsh_range_fill holds rocPRIM's own figure against the bound before it launches anything.
static void range_sort_layout(long long Q, long long total, RangeSortWs *w) {
    size_t o = 0;
    w->unsorted = o; o += ws_align((size_t)total * 8);
    w->sorted = o;   o += ws_align((size_t)total * 8);
    w->tmp = o; w->tmp_bytes = ws_align((size_t)total * 8 + (size_t)Q * 17 + 65536); o += w->tmp_bytes;
    w->total = o;
}

// what both calls check before anything is launched: the one check of a scan call, on the descriptor of the k = 1 plan their kernel runs
// on, and the argument only a radius call has
static int range_check(const char *who, const BucketScanCall &c, const float *radius) {
    const int rc = scan_call_check(who, c, 0);   // no top-k outputs: each call checks its own
    if (rc != NLSH_OK) return rc;
    NLSH_REQUIRE(radius, NLSH_E_INVALID, "%s: radius is null", who);
    NLSH_REQUIRE(((uintptr_t)radius & 3) == 0, NLSH_E_INVALID, "%s: radius must be 4-byte aligned", who);
    return NLSH_OK;
}

// bscanr_kernel of a call, on the plan in its workspace
static int range_scan_launch(const BucketScanCall &c, const BArgs &a, const RangeArgs &r) {
    if (c.max_tasks <= 0) return NLSH_OK;
    if (c.ev_begin) NLSH_CHECK_HIP(hipEventRecord((hipEvent_t)c.ev_begin, c.stream));
    const void *fn = range_scan_kernel_of(c.storage, c.metric);
    BArgs a_ = a;
    RangeArgs r_ = r;
    void *argv[2] = {&a_, &r_};
    NLSH_CHECK_HIP(hipLaunchKernel(fn, tiled_grid(c.max_tasks), tiled_block(), argv, 0, c.stream));
    if (c.ev_end) NLSH_CHECK_HIP(hipEventRecord((hipEvent_t)c.ev_end, c.stream));
    return NLSH_OK;
}

}  // namespace nlsh

extern "C" size_t nlsh_range_workspace(int64_t Q, int P, int64_t max_tasks, int64_t n_buckets, int d) {
    if (Q < 0 || P < 1 || max_tasks < 0 || n_buckets < 0 || d < 1) {
        nlsh::set_error("range_workspace: bad sizes (Q=%lld, P=%d, max_tasks=%lld, n_buckets=%lld, d=%d)", (long long)Q, P, (long long)max_tasks,
                        (long long)n_buckets, d);
        return 0;
    }
    return nlsh::bucket_scan_workspace(Q, P, 1, max_tasks, n_buckets, d);
}

extern "C" size_t nlsh_range_sort_workspace(int64_t Q, int64_t total) {
    if (Q < 0 || total < 0 || total >= (1ll << 31)) {
        nlsh::set_error("range_sort_workspace: Q=%lld, total=%lld (total must be in [0, 2^31))", (long long)Q, (long long)total);
        return 0;
    }
    nlsh::RangeSortWs w;
    nlsh::range_sort_layout(Q, total, &w);
    return w.total;
}

extern "C" int nlsh_range_count(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid, const int32_t *uniq_keys,
                                const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets, const int32_t *cell_of,
                                const int32_t *cell_offsets, int32_t n_cells, const float *inv_norm, const float *queries, int64_t q_stride,
                                int64_t Q, const int32_t *qkeys, const int32_t *nkeys, int P, int metric, int algo, const uint32_t *row_filter,
                                const float *radius, int32_t *out_count, int32_t *out_ncand, int32_t *status, void *workspace,
                                size_t workspace_bytes, int64_t max_tasks, void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream) {
    using namespace nlsh;
    BucketScanCall c = {};
    NLSH_SCAN_CALL_COMMON(c);
    c.cell_of = cell_of; c.cell_offsets = cell_offsets; c.n_cells = n_cells; c.storage = storage; c.row_filter = row_filter;
    c.k = 1; c.seg = 512; c.phases = NLSH_PHASE_PLAN;   // the plan of a k = 1 call: a k = 1 partial area costs nothing and is never written
    const int rc = range_check("range_count", c, radius);
    if (rc != NLSH_OK) return rc;
    NLSH_REQUIRE(out_count, NLSH_E_INVALID, "range_count: out_count is null");
    NLSH_REQUIRE(((uintptr_t)out_count & 3) == 0 && ((uintptr_t)out_ncand & 3) == 0, NLSH_E_INVALID, "range_count: out_count / out_ncand must be 4-byte aligned");
    if (Q == 0) return NLSH_OK;
    NLSH_REQUIRE(out_ncand, NLSH_E_INVALID, "range_count: out_ncand is null");
    BucketScanPrep p;
    const int ra = bucket_scan_args(c, &p);   // holds the workspace against the k = 1 layout
    if (ra != NLSH_OK) return ra;
    NLSH_CHECK_HIP(hipMemsetAsync(out_count, 0, (size_t)Q * sizeof(int32_t), c.stream));
    const int rp = bucket_scan_run(c);         // PLAN: status words, task table, slot records, per-probe records
    if (rp != NLSH_OK) return rp;
    hipLaunchKernelGGL(range_ncand_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, c.stream, (const int4 *)p.a.prec, (long long)Q, P, out_ncand);
    RangeArgs r = {row_filter, radius, out_count, nullptr, nullptr, 0, NLSH_RANGE_COUNT};
    const int rs = range_scan_launch(c, p.a, r);
    if (rs != NLSH_OK) return rs;
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

extern "C" int nlsh_range_fill(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid, const int32_t *uniq_keys,
                               const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets, const int32_t *cell_of,
                               const int32_t *cell_offsets, int32_t n_cells, const float *inv_norm, const float *queries, int64_t q_stride,
                               int64_t Q, const int32_t *qkeys, const int32_t *nkeys, int P, int metric, int algo, const uint32_t *row_filter,
                               const float *radius, const int64_t *row_offsets, int64_t total, int32_t *cursor, uint64_t *out_keys,
                               float *out_dist, int32_t *out_idx, int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                               void *sort_workspace, size_t sort_workspace_bytes, void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream) {
    using namespace nlsh;
    BucketScanCall c = {};
    NLSH_SCAN_CALL_COMMON(c);
    c.cell_of = cell_of; c.cell_offsets = cell_offsets; c.n_cells = n_cells; c.storage = storage; c.row_filter = row_filter;
    c.k = 1; c.seg = 512; c.phases = NLSH_PHASE_PLAN;   // the plan of a k = 1 call: a k = 1 partial area costs nothing and is never written
    const int rc = range_check("range_fill", c, radius);
    if (rc != NLSH_OK) return rc;
    NLSH_REQUIRE(row_offsets, NLSH_E_INVALID, "range_fill: row_offsets is null");
    NLSH_REQUIRE(((uintptr_t)row_offsets & 7) == 0 && ((uintptr_t)out_keys & 7) == 0, NLSH_E_INVALID, "range_fill: row_offsets / out_keys must be 8-byte aligned");
    NLSH_REQUIRE(total >= 0 && total < (1ll << 31), NLSH_E_INVALID, "range_fill: total=%lld not in [0, 2^31)", (long long)total);
    if (Q == 0) return NLSH_OK;
    NLSH_REQUIRE(cursor && ((uintptr_t)cursor & 3) == 0, NLSH_E_INVALID, "range_fill: cursor is null or misaligned");
    NLSH_REQUIRE(total == 0 || out_idx, NLSH_E_INVALID, "range_fill: out_idx is null");
    RangeSortWs w;
    range_sort_layout(Q, total, &w);
    NLSH_REQUIRE(total == 0 || (sort_workspace && ((uintptr_t)sort_workspace & 15) == 0 && sort_workspace_bytes >= w.total), NLSH_E_WORKSPACE,
                 "range_fill: sort_workspace %zu < %zu (or null / not 16-byte aligned)", sort_workspace_bytes, w.total);
    BucketScanPrep p;
    const int ra = bucket_scan_args(c, &p);
    if (ra != NLSH_OK) return ra;
    if (total > 0) {   // the sort's own need against the bound nlsh_range_sort_workspace sized the workspace by
        size_t need = 0;
        uint64_t *nulk = nullptr;
        NLSH_CHECK_HIP(rocprim::segmented_radix_sort_keys(nullptr, need, nulk, nulk, (unsigned)total, (unsigned)Q, row_offsets, row_offsets + 1, 0, 64, c.stream));
        NLSH_REQUIRE(need <= w.tmp_bytes, NLSH_E_WORKSPACE, "range_fill: the segmented sort asks for %zu bytes, the sort_workspace layout holds %zu for it",
                     need, w.tmp_bytes);
    }
    NLSH_CHECK_HIP(hipMemsetAsync(cursor, 0, (size_t)Q * sizeof(int32_t), c.stream));
    if (total == 0) return NLSH_OK;   // nothing in range anywhere: nothing to scan for
    char *sb = (char *)sort_workspace;
    uint64_t *unsorted = (uint64_t *)(sb + w.unsorted), *sorted = out_keys ? out_keys : (uint64_t *)(sb + w.sorted);
    RangeArgs r = {row_filter, radius, cursor, row_offsets, unsorted, (long long)total, NLSH_RANGE_FILL};
    const int rs = range_scan_launch(c, p.a, r);
    if (rs != NLSH_OK) return rs;
    size_t tb = w.tmp_bytes;
    NLSH_CHECK_HIP(rocprim::segmented_radix_sort_keys(sb + w.tmp, tb, unsorted, sorted, (unsigned)total, (unsigned)Q, row_offsets, row_offsets + 1, 0, 64, c.stream));
    hipLaunchKernelGGL(range_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.stream, (const uint64_t *)sorted, (long long)total, out_dist, out_idx);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
