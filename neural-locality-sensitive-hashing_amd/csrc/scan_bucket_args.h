// The argument struct of the bucket-major scan kernels (scan_bucket.hip, scan_bucket_typed.hip): pointers into the caller's arrays and workspace.
#pragma once
#include "scan_common.h"

namespace nlsh {

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

// BArgs of a call, as bucket_scan_run builds them (scan_bucket.hip): the radius query launches its own kernel on the plan the PLAN phase
// of a k = 1 call left in the workspace
int bucket_scan_bargs(const BucketScanCall &c, BArgs *a);

}  // namespace nlsh
