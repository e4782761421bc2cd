// The argument struct of the bucket-major scan kernels (scan_bucket.hip and the typed, filtered and range units), the tile shape they are
// all instantiated with, and a call's prepared launch: pointers into the caller's arrays and workspace.
#pragma once
#include "scan_common.h"
#include "scan_plan.h"

namespace nlsh {

// The shape tiled_task_body is written for, and every tiled kernel is instantiated with <METRIC, TILED_QW, TILED_NW, TILED_TPS, ...>:
constexpr int TILED_QW = 4;   // queries per wave (SGPR budget: two chunks x QW x 4 scalar values in flight)
constexpr int TILED_QB = 16;  // queries per task of the tiled schedule
constexpr int TILED_NW = TILED_QB / TILED_QW;   // waves per workgroup
constexpr int TILED_TPS = 4;  // 64-row tiles per task of the tiled schedule (segment = 64*TPS rows)
// a shared window (nlsh_build_cells: window_rows <= 256) must fit ONE segment: bscatter derives a window bucket's partial-list count from
// its own size and clamps its row range to the segment, so a window wider than a segment would silently lose rows
static_assert(64 * TILED_TPS >= 256, "the tiled schedule's segment must hold the widest row window nlsh_build_cells accepts (256 rows)");
static_assert(NLSH_MAX_K_TILED <= 64 * TILED_TPS, "a (task, query) list is selected from the 64 * TPS candidates the wave holds");
// The launch shape of every tiled kernel: one workgroup per task; the chunked XCD map works on 8 x 16 ids.  (Persistent workgroups and
// several tasks per workgroup were measured slower in r02 and r04: profiles/r04_tasks_per_workgroup_ab.txt, DESIGN.md appendix A.)
inline dim3 tiled_grid(long long max_tasks) { return dim3((unsigned)((max_tasks + 127) / 128 * 128)); }
inline dim3 tiled_block() { return dim3(64 * TILED_NW); }
// the instantiation K<METRIC, TILED_QW, TILED_NW, TILED_TPS, ...> of a tiled kernel template for a run-time metric
#define NLSH_TILED_KERNEL(K, metric, ...)                                                                                                  \
    ((metric) == NLSH_METRIC_L2_EPS          ? (const void *)K<NLSH_METRIC_L2_EPS, TILED_QW, TILED_NW, TILED_TPS, ##__VA_ARGS__>           \
     : (metric) == NLSH_METRIC_L2_EPS_FOLDED ? (const void *)K<NLSH_METRIC_L2_EPS_FOLDED, TILED_QW, TILED_NW, TILED_TPS, ##__VA_ARGS__>    \
                                             : (const void *)K<NLSH_METRIC_COSINE, TILED_QW, TILED_NW, TILED_TPS, ##__VA_ARGS__>)

struct BArgs {
    const float *corpus;
    long long row_stride;
    int d;
    const int32_t *gid;
    const int32_t *uniq;
    const int32_t *offsets;
    int nb;
    // Cells (nlsh_build_cells; tiled schedule): the unit the PLAN phase counts pairs and lays out tasks by.  A cell is a big bucket on
    // its own, or a run of consecutive small buckets of at most `window_rows` (<= 256) rows that share one row window -- the
    // queries probing ANY of them share the window's tasks, each with its own row range.  Without cells: cell == bucket.
    const int32_t *cell_of;    // [nb] bucket -> cell, or nullptr
    const int32_t *coffsets;   // [nc + 1] first sorted row of every cell (== offsets without cells)
    int nc;                    // cells (== nb without cells)
    const float *inv_norm;
    const float *queries;
    long long q_stride;
    long long Q;
    const int32_t *qkeys;
    const int32_t *nkeys;
    int P, k, seg, QB;
    float *out_dist;
    int32_t *out_idx;
    uint64_t *out_keys;
    int32_t *out_ncand;
    int32_t *status;
    int32_t *inv_q, *bcount;   // bcount: per CELL
    int4 *ppair;    // [Q*P] what the lookup left per (query, probe) pair (scan_plan.h): {cell, slot in the cell's list, bucket rows, first row inside the cell}
    int4 *cellrec;  // [nc] per cell, written by bscan: {first pair of its list, first task, query groups, 0}
    int4 *prec;  // [Q*P] per (query, probe): {first task of its query group, slot in the group, bucket rows, query groups}; .z = 0: no bucket
    int4 *task;
    int2 *task_qr;     // tiled schedule: [max_tasks][16] {query id, row range lo | hi << 16} of every (task, slot): the task's group's slice of
                       // inv_q, repeated per row segment, and the rows of the query's bucket inside the task's rows (a whole segment of a
                       // big bucket; the bucket's slice of a shared window).  ONE 8-byte record: one store in bscatter, one load in the scan
    uint64_t *partial;
    long long max_tasks;
    const int32_t *border;     // [nc] schedule order of the cells (largest first) or nullptr = CSR order
    unsigned long long *lookback;   // [blocks of bscan] per-block (pairs, tasks, negative counter seen) totals + ready bit, zeroed by the plan launch
    int32_t *hits;             // [blocks of the plan launch] (query, probe) pairs each block counted | PLAN_VIOL_* flags
    unsigned long long *tauq;  // [Q] running upper bound of each query's k-th best key (atomicMin), KEY_NONE-initialised
    const float *qpad;  // tiled variant: queries padded to d4p*4 floats (L2: pad = -eps; cosine: pre-normalised, pad = 0)
    float *qpad_w;      // same buffer, writable (prep_query); qpad aliases `queries` when no padding/normalisation is needed
    long long qpad_stride;
    int d4p;
};

// Second parameter of the radius-query kernels (bscanr_kernel, scan_bucket_range.hip; nlsh_range_count / nlsh_range_fill): what the range
// epilogue of tiled_task_body reads beside BArgs, which keeps its layout.
#define NLSH_RANGE_COUNT 0
#define NLSH_RANGE_FILL 1
struct RangeArgs {
    const uint32_t *row_filter;    // bitset over the sorted rows (nlsh_row_filter_build) or nullptr: every row allowed
    const float *radius;           // [Q] a candidate is a hit iff dist <= radius[q] (IEEE: a NaN distance never is)
    int32_t *counter;              // [Q] zeroed by the call; count mode: hits of the query; fill mode: its write cursor
    const int64_t *row_offsets;    // fill mode: [Q + 1] exclusive prefix sum of the counts
    uint64_t *keys;                // fill mode: [total] the hits' sort keys, a query's in no particular order
    long long total;               // fill mode: row_offsets[Q] as the host read it; no key is stored at or behind it
    int mode;                      // NLSH_RANGE_COUNT | NLSH_RANGE_FILL (wave-uniform)
};

// The corpus storage of the affine kernels (bscana_kernel, scan_bucket_affine.hip; nlsh_scan_topk_cells_phase_sq8): uint8 codes in the
// uint8 layout, decoded per dimension as the tile is written (Stored<NLSH_STORE_SQ8>).  Internal: the C ABI's storage codes end at
// NLSH_STORE_U8, an sq8 call is a uint8 call that carries a quantiser (BucketScanCall::affine).
#define NLSH_STORE_SQ8 3
// The side arguments of a tiled scan: everything a call can carry beside BArgs, which keeps its layout.  ONE struct, the second parameter
// of the filtered, affine and tagged kernels (bscanf_kernel, bscana_kernel, bscang_kernel) and what tiled_task_body reads its filter and
// its quantiser from in every form; a kernel reads the fields its compile-time flags (FILT, STORE, TAGS) name and no others.  Filled once
// per call from the BucketScanCall (scan_launch_of).  The field order decides how the compiler merges the argument loads: with this one
// every kernel keeps its resource figures and its arithmetic loops (profiles/scan_side_args.txt).
struct SideArgs {
    const uint64_t *tags;          // TAGS: [N] tag word of every SORTED row, read with the row position the lane already has
    const uint64_t *qmask;         // TAGS: [Q] mask of every query of the call
    int match;                     // TAGS: NLSH_TAG_ANY | NLSH_TAG_ALL | NLSH_TAG_EQ (wave-uniform)
    const uint32_t *row_filter;    // bitset over the sorted rows (nlsh_row_filter_build); FILT: never null, otherwise nullptr = every row allowed
    const float4 *lo4;             // NLSH_STORE_SQ8: [row_stride / 4] the quantiser's offsets, padded to the pitch with 0
    const float4 *step4;           // NLSH_STORE_SQ8: [row_stride / 4] its steps, padded with 1: a padded column (code 0) decodes to +0
};

// The corpus storage of the PQ kernels (bscanq_kernel, scan_bucket_pq.hip; nlsh_scan_topk_cells_phase_pq): M code bytes per row, a staged
// 16-byte slot gathered from the codebook as the tile is written (l2_task*, scan_bucket_tiled.h).  Internal, like NLSH_STORE_SQ8: a pq
// call is a uint8 call that carries a codebook (BucketScanCall::pq).
#define NLSH_STORE_PQ 4
// THIRD parameter of the PQ kernels, theirs alone: SideArgs and BArgs keep their layout and field order (see SideArgs above).
struct PqArgs {
    const float4 *cb4;             // the codebook [M, 256, dsub] float32 as float4s: entry (m, code) is cps consecutive ones
    long long pitch;               // bytes between the code rows (a multiple of 16, >= M)
    int cps;                       // 16-byte chunks per sub-vector: dsub / 4 = 1 | 2 | 4
};

// A call's prepared launch (scan_bucket.hip): the workspace held against the schedule's layout (NLSH_E_WORKSPACE), then what the scan kernels
// take (bucket_scan_run; the radius calls for their own kernel), what the lookup takes (step.hip, probe_ranked.hip: the launch that does it),
// the metric the schedule really computes and whether the tiled schedule needs its padded / pre-normalised query copy
struct BucketScanPrep { BArgs a; PlanArgs pa; int metric; bool prep; };
int bucket_scan_args(const BucketScanCall &c, BucketScanPrep *p);

}  // namespace nlsh
