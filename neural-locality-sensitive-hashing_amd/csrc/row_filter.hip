// Row filter of the tiled scan (nlsh_scan_topk_cells_phase_filtered): a bitset over the bucket-sorted rows, built from row ids.
//
// The filter is in POSITION order -- bit p & 31 of word p >> 5 belongs to sorted row p, the row whose id is gid[p] -- because that is
// what the scan has in hand: a lane of the tiled kernel owns sorted row `prow` and reads word prow >> 5 beside gid[prow], coalesced
// and with no load that depends on the id.  Ids are any int32 (negative, sparse), so a bitset indexed by id is not an option; the
// translation from ids to positions is done once per filter, here, and a filter serves every call until the index is mutated.
#include "common.h"

namespace nlsh {

// One wavefront per 64 consecutive sorted rows, one row per lane.  Membership of gid[p]: a lower-bound search in the strictly ascending
// id list `ids` [n_ids], or a lookup in the dense array `dense` [n_dense] indexed by id - id_base (ids outside it are not members).
// allowed = member XOR invert.  The wave's ballot is its two filter words -- rows >= n_rows contribute zero bits, so the tail of the
// last word pair is zero -- stored by lane 0; the allowed rows are counted with one atomic per wave.
__global__ __launch_bounds__(256) void row_filter_build_kernel(const int32_t *gid, long long n_rows, const int32_t *ids, long long n_ids,
                                                                const uint8_t *dense, long long n_dense, int id_base, int invert,
                                                                uint32_t *row_filter, int32_t *n_allowed) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform: the wave's 64-row group
    if (w * 64 >= n_rows) return;
    const long long p = w * 64 + lane;
    bool allowed = false;
    if (p < n_rows) {
        const int32_t id = gid[p];
        bool member;
        if (ids) {
            long long lo = 0, hi = n_ids;   // lower_bound in the ascending ids
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (ids[mid] < id) lo = mid + 1; else hi = mid;
            }
            member = lo < n_ids && ids[lo] == id;
        } else {
            const long long off = (long long)id - (long long)id_base;
            member = off >= 0 && off < n_dense && dense[off] != 0;
        }
        allowed = member != (invert != 0);
    }
    const unsigned long long bits = __ballot(allowed);
    if (lane == 0) {
        row_filter[2 * w] = (uint32_t)bits;
        row_filter[2 * w + 1] = (uint32_t)(bits >> 32);
        const int n = __popcll(bits);
        if (n) atomicAdd(n_allowed, n);
    }
}

}  // namespace nlsh

using namespace nlsh;

extern "C" size_t nlsh_row_filter_words(int64_t n_rows) {
    if (n_rows < 0) { set_error("row_filter_words: n_rows=%lld", (long long)n_rows); return 0; }
    return 2 * (size_t)((n_rows + 63) / 64);
}

extern "C" int nlsh_row_filter_build(const int32_t *gid, int64_t n_rows, const int32_t *ids, int64_t n_ids, const uint8_t *dense,
                                     int64_t n_dense, int32_t id_base, int invert, uint32_t *row_filter, int32_t *n_allowed,
                                     nlsh_stream_t stream) {
    NLSH_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), NLSH_E_INVALID, "row_filter_build: n_rows=%lld not in [0, 2^31)", (long long)n_rows);
    NLSH_REQUIRE(!(ids && dense), NLSH_E_INVALID, "row_filter_build: both ids and dense given, exactly one is the source");
    NLSH_REQUIRE(ids || dense, NLSH_E_INVALID, "row_filter_build: neither ids nor dense given, exactly one is the source");
    NLSH_REQUIRE(!ids || n_ids >= 0, NLSH_E_INVALID, "row_filter_build: n_ids=%lld", (long long)n_ids);
    NLSH_REQUIRE(!dense || n_dense >= 0, NLSH_E_INVALID, "row_filter_build: n_dense=%lld", (long long)n_dense);
    NLSH_REQUIRE(invert == 0 || invert == 1, NLSH_E_INVALID, "row_filter_build: invert=%d", invert);
    NLSH_REQUIRE(n_allowed, NLSH_E_INVALID, "row_filter_build: n_allowed is null");
    NLSH_REQUIRE(n_rows == 0 || gid, NLSH_E_INVALID, "row_filter_build: gid is null");
    NLSH_REQUIRE(n_rows == 0 || row_filter, NLSH_E_INVALID, "row_filter_build: row_filter is null");
    NLSH_REQUIRE(((uintptr_t)row_filter & 3) == 0 && ((uintptr_t)n_allowed & 3) == 0, NLSH_E_INVALID,
                 "row_filter_build: row_filter and n_allowed must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    NLSH_CHECK_HIP(hipMemsetAsync(n_allowed, 0, sizeof(int32_t), s));
    if (n_rows == 0) return NLSH_OK;
    const long long waves = (n_rows + 63) / 64;
    hipLaunchKernelGGL(row_filter_build_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, gid, (long long)n_rows, ids, (long long)n_ids,
                       dense, (long long)n_dense, (int)id_base, invert, row_filter, n_allowed);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
