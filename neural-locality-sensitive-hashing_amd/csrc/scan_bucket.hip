// Bucket-major candidate scan (algos NLSH_SCAN_BUCKET_MAJOR and NLSH_SCAN_BUCKET_TILED of nlsh_scan_topk).
//
// Same contract as the query-major kernel (scan_topk.hip; reference nlsh/indexer.py:62-95), different
// schedule: when many queries of a batch probe the same buckets (SIFT1M-shaped run: 45k distinct
// (query, bucket) pairs over 5k buckets -> every corpus row is a candidate of ~24 queries) the
// query-major kernel re-reads each row once per query and sits on the HBM roofline.  Here the
// (query, probe) pairs are inverted into per-bucket query lists on the device and a row tile is scored
// against a GROUP of queries per fetch:
//   bscan2 (wave-level):  one wavefront = (bucket segment, <= 8 queries in VGPRs); lanes span a row,
//                         cross-lane DPP/permlane reduction per (row, query); same bits as query-major;
//   bscan3 (LDS-tiled):   one workgroup = (256-row segment, <= 16 queries); every lane owns a row of each
//                         tile, queries arrive as scalar loads, no cross-lane traffic, k-ordered fmaf chain
//                         (bit-identical to the oracle), selection by bisection instead of insertion.
//
// Per batch, all on the caller's stream, no host round trip (r06: five launches with the lookup fused into encode_hash, six without):
//   bplan    thread/(query,probe): binary search key -> bucket -> cell; the pair takes its slot in the cell's list (atomicAdd);
//            scan_plan.h -- in the epilogue of encode_hash_kernel when the keys come from there, bplan_kernel for caller-supplied keys
//            (tiled, cosine / folded L2 / d % 4 != 0 only: the padded / pre-normalised query copy is written by the same launch)
//   bscan    thread/cell: reads AND resets the cell's pair counter; block scan + decoupled look-back over the per-block totals ->
//            disjoint pair/task ranges; task = (group of <= QB pairs, segment of <= seg rows), segment-major ids
//   bscatter thread/(query,probe): the pair's record into its cell's query list and its tasks' slot records (no atomics)
//   bscan2 | bscan3: partial top-k per (task, query)
//   bmerge   wave/query: merge the partial lists of its (probe, segment) pairs -> final top-k
// Results do not depend on slot/task order: every list is merged with the (distance, id) comparator.
#include <new>

#include "step_nodes.h"

#include "scan_bucket_args.h"   // BArgs: what the scan kernels take

// The device code, one header per phase / schedule, in the order of the batch (each opens namespace nlsh itself and needs BArgs):
#include "scan_bucket_plan.h"    // bplan_kernel, bscan_kernel (block scan, look-back), bscatter_kernel
#include "scan_bucket_wave.h"    // bscan2_*: the wave-level schedule
#include "scan_bucket_tiled.h"   // k-block assembly, l2_task*, tiled_task_body, bscan3_kernel, bscanw_kernel (bscant_kernel: instantiated in scan_bucket_typed.hip)
#include "scan_bucket_merge.h"   // merge_query, merge_query_wide, bmerge_kernel, bmergew_kernel

namespace nlsh {

struct BWs {
    size_t ppair, prec, inv_q, bcount, cellrec, lookback, hits, task, task_qr, partial, qpad, tauq, total;
};
// blocks of the launch that does the lookup: bplan_kernel's 256 pairs per block, or encode_hash's workgroups (>= 16 rows each)
static inline long long plan_blocks_max(long long Q, int P) {
    const long long a = (Q * P + 255) / 256, b = (Q + 15) / 16;
    return (a > b ? a : b) + 1;
}
static void blayout(long long Q, int P, int k, long long max_tasks, long long nb, int d, bool tiled, BWs *w) {
    size_t o = 0;
    const size_t qp = (size_t)Q * P * 4, nb4 = (size_t)(nb > 0 ? nb : 1) * 4;
    w->bcount = o;   o += ws_align(nb4);   // first, at an offset that does not depend on the batch: ZERO between calls (workspace contract)
    w->ppair = o;    o += ws_align(qp * 4);
    w->prec = o;     o += ws_align(qp * 4);
    w->inv_q = o;    o += ws_align(qp);
    w->cellrec = o;  o += ws_align(nb4 * 4);
    w->lookback = o; o += ws_align((size_t)((nb + 255) / 256 + 1) * 8);
    w->hits = o;     o += ws_align((size_t)plan_blocks_max(Q, P) * 4);
    // everything above sits at offsets that do not depend on max_tasks: a lookup done for one table size (encode_hash's epilogue)
    // stays valid when the call is repeated with a larger table
    w->task = o;     o += ws_align((size_t)max_tasks * sizeof(int4));
    w->task_qr = o;  o += tiled ? ws_align((size_t)max_tasks * TILED_QB * 8) : 0;
    w->partial = o;  o += ws_align((size_t)max_tasks * (tiled ? TILED_QB : 8) * k * 8);
    w->qpad = o;     o += tiled ? ws_align((size_t)Q * ((d + 3) / 4) * 16) : 0;
    w->tauq = o;     o += ws_align((size_t)Q * 8);
    w->total = o;
}

size_t bucket_scan_workspace(long long Q, int P, int k, long long max_tasks, long long n_buckets, int d) {
    BWs w, wt;
    blayout(Q, P, k, max_tasks, n_buckets, d, false, &w);
    blayout(Q, P, k, max_tasks, n_buckets, d, true, &wt);
    return w.total > wt.total ? w.total : wt.total;
}

}  // namespace nlsh

extern "C" int nlsh_scan_workspace_layout(int64_t Q, int P, int k, int64_t max_tasks, int64_t n_buckets, int d, int algo,
                                          size_t *task_table_offset, size_t *task_queries_offset, size_t *task_ranges_offset) {
    NLSH_REQUIRE(algo == NLSH_SCAN_BUCKET_MAJOR || algo == NLSH_SCAN_BUCKET_TILED, NLSH_E_INVALID, "scan_workspace_layout: algo=%d has no task table of this form", algo);
    NLSH_REQUIRE(Q >= 0 && P >= 1 && k >= 1 && max_tasks >= 0 && n_buckets >= 0 && d >= 1, NLSH_E_INVALID, "scan_workspace_layout: bad sizes");
    nlsh::BWs w;
    nlsh::blayout(Q, P, k, max_tasks, n_buckets, d, algo == NLSH_SCAN_BUCKET_TILED, &w);
    if (task_table_offset) *task_table_offset = w.task;
    if (task_queries_offset) *task_queries_offset = w.task_qr;        // interleaved: {query id, range} pairs, 8 bytes per (task, slot)
    if (task_ranges_offset) *task_ranges_offset = w.task_qr + 4;
    return NLSH_OK;
}

namespace nlsh {

template <int METRIC>
static const void *bscan2_of(int d4) {
    if (d4 <= 16) return (const void *)bscan2_kernel<16, 1, METRIC, 8>;
    if (d4 <= 32) return (const void *)bscan2_kernel<32, 1, METRIC, 8>;
    if (d4 <= 64) return (const void *)bscan2_kernel<64, 1, METRIC, 8>;
    if (d4 <= 128) return (const void *)bscan2_kernel<64, 2, METRIC, 4>;
    return (const void *)bscan2_kernel<64, 4, METRIC, 2>;
}

// The SCAN phase's launch of a call -- kernel, grid, block and argument vector -- for bucket_scan_run and bucket_scan_node alike.
struct ScanLaunch {
    const void *fn;
    dim3 grid, block;
    void *argv[3];   // the kernel's BArgs and, read by the filtered, affine, tagged and PQ kernels alone, `side` as their second parameter;
                     // `pqa` is the PQ kernels' third
    SideArgs side;   // the call's filter, quantiser, tags, masks and mode: what it does not carry is null
    PqArgs pqa;      // the call's codebook, code pitch and chunks per sub-vector (a pq call's alone)
};
static int scan_launch_of(const BucketScanCall &c, int metric, const BArgs *a, ScanLaunch *l) {
    l->side = SideArgs{c.row_tags, c.query_masks, c.tag_match, c.row_filter, c.affine ? (const float4 *)c.quant_lo : nullptr,
                       c.affine ? (const float4 *)c.quant_step : nullptr};
    l->argv[0] = (void *)a;
    l->argv[1] = (void *)&l->side;
    l->pqa = PqArgs{(const float4 *)c.pq_codebook, c.pq_pitch, c.pq_dsub / 4};
    l->argv[2] = (void *)&l->pqa;
    const bool wide = c.k > NLSH_MAX_K;   // wide k: the same task body, its epilogue selecting up to 64 * TPS keys per list
    if (!c.tiled()) {
        NLSH_REQUIRE(!c.row_filter && c.storage == NLSH_STORE_F32 && !c.affine && !c.row_tags && !c.pq, NLSH_E_UNSUPPORTED,
                     "scan_topk(bucket-major): row_filter, row_tags and a float16 / uint8 corpus are read by the tiled schedule only");
        l->grid = dim3((unsigned)((c.max_tasks + 3) / 4));  // one wavefront per task
        l->block = dim3(256);
    } else {
        l->grid = tiled_grid(c.max_tasks);
        l->block = tiled_block();
    }
    // (the float32 tiled kernels are named before the wave-level ones: a code object keeps its kernels in the order the host code first
    // names them, and scan_bucket.hip's is compared byte for byte across changes of this file)
    if (c.tiled() && c.pq) l->fn = pq_scan_kernel_of(metric, wide);                                                    // scan_bucket_pq.hip
    else if (c.tiled() && c.row_tags) l->fn = tagged_scan_kernel_of(c.affine ? NLSH_STORE_SQ8 : c.storage, metric, wide);   // scan_bucket_tagged.hip
    else if (c.tiled() && c.affine) l->fn = affine_scan_kernel_of(metric, wide);                                      // scan_bucket_affine.hip
    else if (c.tiled() && c.row_filter) l->fn = filtered_scan_kernel_of(c.storage, metric, wide);                    // scan_bucket_filtered.hip
    else if (c.tiled() && c.storage != NLSH_STORE_F32) l->fn = typed_scan_kernel_of(c.storage, metric, wide);   // scan_bucket_typed.hip
    else if (c.tiled() && wide) l->fn = NLSH_TILED_KERNEL(bscanw_kernel, metric);
    else if (c.tiled()) l->fn = NLSH_TILED_KERNEL(bscan3_kernel, metric);
    else l->fn = metric == NLSH_METRIC_L2_EPS ? bscan2_of<NLSH_METRIC_L2_EPS>((c.d + 3) / 4) : bscan2_of<NLSH_METRIC_COSINE>((c.d + 3) / 4);
    return NLSH_OK;
}

// A call's prepared launch (scan_bucket_args.h): BArgs and PlanArgs pointing into the caller's workspace, the effective metric, `prep`.
int bucket_scan_args(const BucketScanCall &c, BucketScanPrep *p) {
    BArgs &a = p->a;
    PlanArgs &pa = p->pa;
    const bool tiled = c.tiled();
    BWs w;
    blayout(c.Q, c.P, c.k, c.max_tasks, c.nb, c.d, tiled, &w);
    NLSH_REQUIRE(c.workspace_bytes >= w.total, NLSH_E_WORKSPACE, "scan_topk(bucket-major): workspace %zu < %zu", c.workspace_bytes, w.total);
    const int d4 = (c.d + 3) / 4;
    a.corpus = c.corpus; a.row_stride = c.row_stride; a.d = c.d; a.gid = c.gid; a.uniq = c.uniq; a.offsets = c.offsets; a.nb = c.nb;
    // cells exist for the tiled schedule only (a window is one 256-row segment of its task shape); the wave-level schedule ignores them
    const bool cells = tiled && c.cell_of && c.cell_offsets && c.n_cells > 0;
    a.cell_of = cells ? c.cell_of : nullptr; a.coffsets = cells ? c.cell_offsets : c.offsets; a.nc = cells ? c.n_cells : c.nb;
    a.inv_norm = c.inv_norm; a.queries = c.queries; a.q_stride = c.q_stride; a.Q = c.Q; a.qkeys = c.qkeys; a.nkeys = c.nkeys;
    a.P = c.P; a.k = c.k; a.seg = tiled ? 64 * TILED_TPS : scan_seg_rows(c.seg); a.QB = tiled ? TILED_QB : (d4 <= 64 ? 8 : (d4 <= 128 ? 4 : 2));
    a.qpad_w = (float *)((char *)c.workspace + w.qpad); a.qpad = a.qpad_w; a.qpad_stride = (long long)d4 * 4; a.d4p = d4;
    // L2 with d % 4 == 0 needs neither padding nor normalisation: read the caller's queries directly
    // the folded L2 form exists in the tiled schedule only (it always needs the prepared query copy: q + eps); the other two
    // schedules answer NLSH_METRIC_L2_EPS_FOLDED with the exact form, which is inside the same tolerance
    const int metric = (!tiled && c.metric == NLSH_METRIC_L2_EPS_FOLDED) ? NLSH_METRIC_L2_EPS : c.metric;
    const bool prep = tiled && !(metric == NLSH_METRIC_L2_EPS && (c.d & 3) == 0 && (c.q_stride & 3) == 0 && ((uintptr_t)c.queries & 15) == 0);
    if (tiled && !prep) { a.qpad = c.queries; a.qpad_stride = c.q_stride; }
    a.out_dist = c.out_dist; a.out_idx = c.out_idx; a.out_keys = c.out_keys; a.out_ncand = c.out_ncand; a.status = c.status;
    char *base = (char *)c.workspace;
    a.ppair = (int4 *)(base + w.ppair); a.prec = (int4 *)(base + w.prec); a.inv_q = (int32_t *)(base + w.inv_q);
    a.bcount = (int32_t *)(base + w.bcount); a.cellrec = (int4 *)(base + w.cellrec); a.lookback = (unsigned long long *)(base + w.lookback);
    a.hits = (int32_t *)(base + w.hits); a.border = c.bucket_order; a.task = (int4 *)(base + w.task);
    a.task_qr = tiled ? (int2 *)(base + w.task_qr) : nullptr; a.partial = (uint64_t *)(base + w.partial);
    a.max_tasks = c.max_tasks;
    a.tauq = (unsigned long long *)(base + w.tauq);

    pa.uniq = a.uniq; pa.offsets = a.offsets; pa.cell_of = a.cell_of; pa.coffsets = a.coffsets; pa.nb = a.nb;
    pa.stride = 1; pa.nco = a.nb;   // the launcher of the lookup sizes the coarse table for the LDS it has (plan_coarse)
    pa.seg = a.seg; pa.P = a.P; pa.Q = a.Q; pa.qkeys = a.qkeys; pa.qnkeys = a.nkeys;
    pa.bcount = a.bcount; pa.ppair = a.ppair; pa.hits = a.hits; pa.status = a.status; pa.tauq = a.tauq;
    pa.lookback = a.lookback; pa.n_lookback = (a.nc + 255) / 256;
    pa.queries = c.queries; pa.q_stride = c.q_stride; pa.qpad = a.qpad_w; pa.qpad_stride = (long long)d4 * 4; pa.d = c.d; pa.d4p = d4;
    pa.prep_metric = prep ? metric : -1;
    pa.enabled = 1;
    p->metric = metric;
    p->prep = prep;
    return NLSH_OK;
}

int bucket_scan_node(const BucketScanCall &c, ScanNode *out) {
    static_assert(sizeof(BArgs) <= sizeof(out->args) && alignof(BArgs) <= 16, "ScanNode::args must hold the scan kernels' argument struct");
    NLSH_REQUIRE(c.max_tasks > 0, NLSH_E_INVALID, "scan node: empty task table");
    // a node carries ONE kernel parameter (ScanNode::argv): the filtered kernels take two
    NLSH_REQUIRE(c.row_filter == nullptr, NLSH_E_UNSUPPORTED, "scan node: a call with a row_filter cannot be replayed from a graph node");
    NLSH_REQUIRE(!c.affine, NLSH_E_UNSUPPORTED, "scan node: a call over an sq8 corpus cannot be replayed from a graph node");
    NLSH_REQUIRE(c.row_tags == nullptr, NLSH_E_UNSUPPORTED, "scan node: a call with row_tags cannot be replayed from a graph node");
    NLSH_REQUIRE(!c.pq, NLSH_E_UNSUPPORTED, "scan node: a call over a pq corpus cannot be replayed from a graph node");
    BucketScanPrep p;
    int rc = bucket_scan_args(c, &p);
    if (rc != NLSH_OK) return rc;
    BArgs *a = new (out->args) BArgs(p.a);
    ScanLaunch l;
    rc = scan_launch_of(c, p.metric, a, &l);
    if (rc != NLSH_OK) return rc;
    out->p = hipKernelNodeParams{};
    out->p.func = const_cast<void *>(l.fn);
    out->p.gridDim = l.grid; out->p.blockDim = l.block;
    out->argv[0] = l.argv[0];
    out->p.kernelParams = out->argv; out->p.sharedMemBytes = 0; out->p.extra = nullptr;
    return NLSH_OK;
}

int bucket_scan_run(const BucketScanCall &c) {
    BucketScanPrep p;
    int rc = bucket_scan_args(c, &p);
    if (rc != NLSH_OK) return rc;
    const BArgs &a = p.a;
    const bool scan = (c.phases & NLSH_PHASE_SCAN) && c.max_tasks > 0;
    ScanLaunch l;
    if (scan && (rc = scan_launch_of(c, p.metric, &a, &l)) != NLSH_OK) return rc;   // before anything is enqueued

    hipStream_t s = c.stream;
    const unsigned gp = (unsigned)((c.Q * c.P + 255) / 256);
    if (c.phases & NLSH_PHASE_PLAN) {
        // The lookup as a launch of its own (caller-supplied keys; keys made by encode_hash are looked up in ITS epilogue and the
        // caller passes NLSH_PHASE_PLAN_REST instead).  (One fused launch with grid barriers between the steps of this counting
        // sort was built and measured in r02: 127 us with agent-scope fences -- each writes back / invalidates an XCD's L2 --, 63 us
        // with device-coherent sc1 accesses instead, against 35 us for the separate launches: crossing XCDs inside a kernel costs as
        // much as a kernel boundary on this part.)  The per-cell pair counters need no clearing launch: bscan_kernel hands every
        // count back, so they are zero again after every call (workspace contract, nlsh_hip.h).
        PlanArgs pa = p.pa;
        plan_coarse(pa, 1024);
        const unsigned gprep = p.prep ? (unsigned)((c.Q + 3) / 4) : 0u;   // the query copy rides in the same launch
        hipLaunchKernelGGL(bplan_kernel, dim3(gp + gprep), dim3(256), 0, s, pa, gp);
    }
    if (c.phases & (NLSH_PHASE_PLAN | NLSH_PHASE_PLAN_REST)) {
        // (r03: bcount + bscan as ONE single-workgroup launch for indexes of <= 8192 buckets took 23 us against 16.4 us for the two
        // launches of r02-r05: one CU writes 12 k task descriptors slower than 23 workgroups do.  r06: one launch of all the
        // workgroups with a look-back over their totals, see bscan_kernel.)
        const int plan_blocks = (c.phases & NLSH_PHASE_PLAN) ? (int)gp : c.plan_blocks;
        if (a.nc > 0) hipLaunchKernelGGL(bscan_kernel, dim3((unsigned)((a.nc + 255) / 256)), dim3(256), 0, s, a, plan_blocks);
        hipLaunchKernelGGL(bscatter_kernel, dim3(gp), dim3(256), 0, s, a);
    }
    if (scan) {
        if (c.ev_begin) NLSH_CHECK_HIP(hipEventRecord((hipEvent_t)c.ev_begin, s));
        NLSH_CHECK_HIP(hipLaunchKernel(l.fn, l.grid, l.block, l.argv, 0, s));
        if (c.ev_end) NLSH_CHECK_HIP(hipEventRecord((hipEvent_t)c.ev_end, s));
    }
    if (c.phases & NLSH_PHASE_MERGE) {
        const dim3 gm((unsigned)((c.Q + 3) / 4));
        if (c.host_out) {
            NLSH_REQUIRE(c.k <= NLSH_MAX_K, NLSH_E_UNSUPPORTED, "scan_topk(bucket-major): the host-writing merge takes k <= %d", NLSH_MAX_K);
            hipLaunchKernelGGL(bmerge_host_kernel, gm, dim3(256), 0, s, a, c.host_out);
        } else if (c.k <= NLSH_MAX_K) hipLaunchKernelGGL(bmerge_kernel, gm, dim3(256), 0, s, a);
        else if (c.k <= 128) hipLaunchKernelGGL(bmergew_kernel<2>, gm, dim3(256), 0, s, a);
        else if (c.k <= 192) hipLaunchKernelGGL(bmergew_kernel<3>, gm, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(bmergew_kernel<4>, gm, dim3(256), 0, s, a);
    }
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

}  // namespace nlsh
