// One pipelined query batch per C-ABI call (nlsh_query_step_enqueue, ABI v3).
//
// A batch of the reference's `Indexer.query` (nlsh/indexer.py:56-96) is encode_hash + the PLAN, SCAN and MERGE phases of the scan:
// seven kernel launches.  Pipelined over HIP streams (front: encode + PLAN | mid: SCAN | tail: MERGE [+ the shard exchange]) it
// also needs eight to ten event records / waits, and through r04 the Python facade issued all of them one ctypes / torch call at a
// time: ~0.09 ms of host time per batch, which on small shards (8 GPUs: scan 0.055-0.068 ms) WAS the step.  Here the slot -- the
// validated encode launch, the scan call, the four streams and the slot's events -- is built once (nlsh_step_create) and a batch is
// ONE call that only swaps the batch pointer, its row stride and the Philox seed.  The library owns the events (it is linked against
// the HIP runtime the kernels use; ADVICE r04: the facade used to dlopen "libamdhip64.so" by name for them); the streams and every
// buffer stay the caller's.  Same kernels, same arguments, same results as the phase calls: only where the launches are issued from
// changes.
//
// r06 (ABI v4): the batch is FIVE launches -- the bucket lookup of the PLAN phase runs in encode_hash's epilogue (scan_plan.h) whenever
// the schedule is a bucket-major one, and the rest of the PLAN phase is two launches instead of three -- and the same batch exists
// as a one-stream call for callers that do not pipeline (nlsh_query_batch: what `Indexer.query_tensors` issues).
#include <cstdlib>
#include <new>

#include "step_nodes.h"

#include "scan_bucket_args.h"   // BucketScanPrep: the lookup's PlanArgs of a scan call

using namespace nlsh;

struct nlsh_step {
    EncPlan enc;
    nlsh_step_desc_t d;
    int dims[NLSH_MAX_LAYERS + 1];
    hipEvent_t ready, encoded, planned, scanned, done;
    bool done_pending;   // hold_done: the caller still has to release the batch (nlsh_step_release)
    // graph slots (nlsh_step_create_graph): the batch's five launches captured once, replayed on `lane`
    hipStream_t lane;
    hipGraph_t graph;
    hipGraphExec_t exec;
    hipGraphNode_t enc_node, scan_node;
    bool graph_failed;   // the capture or the instantiation did not work on this runtime: the slot launches its batches eagerly on its stream
};

// One batch's scan call: the descriptor's members by name, the batch pointer and the stream.  The caller names what else its call has
// (events, the workgroups of a fused lookup, a host block) on the descriptor it gets back.
static BucketScanCall step_scan_call(const nlsh_step_desc_t &d, const float *queries, int64_t q_stride, hipStream_t stream, int phases) {
    BucketScanCall c = {};
    c.corpus = d.corpus_sorted; c.row_stride = d.row_stride; c.d = d.d; c.gid = d.gid; c.uniq = d.uniq_keys; c.offsets = d.offsets;
    c.bucket_order = d.bucket_order; c.nb = d.n_buckets; c.cell_of = d.cell_of; c.cell_offsets = d.cell_offsets; c.n_cells = d.n_cells;
    c.inv_norm = d.inv_norm; c.queries = queries; c.q_stride = q_stride; c.Q = d.Q; c.qkeys = d.qkeys; c.nkeys = d.nkeys;
    c.P = d.n_probes; c.k = d.k; c.metric = d.metric; c.algo = d.algo; c.seg = d.seg_rows;
    c.out_dist = d.out_dist; c.out_idx = d.out_idx; c.out_keys = d.out_keys; c.out_ncand = d.out_ncand; c.status = d.status;
    c.workspace = d.workspace; c.workspace_bytes = d.workspace_bytes; c.max_tasks = d.max_tasks;
    c.stream = stream; c.phases = phases;
    return c;
}
constexpr int SCAN_AND_MERGE = NLSH_PHASE_SCAN | NLSH_PHASE_MERGE;   // what follows a batch's plan phase (NLSH_PHASE_PLAN, or _REST behind a fused lookup)
// the one check of a scan call, with the internal phase bit allowed
static int step_scan_check(const BucketScanCall &c) { return scan_call_check("scan_topk", c, SCAN_NEEDS_TOPK_OUT | SCAN_ALLOWS_PLAN_REST); }
// check, and the lookup's arguments for this call's workspace (bucket-major schedules)
static int step_scan_prepare(const BucketScanCall &c, BucketScanPrep *p) {
    const int rc = step_scan_check(c);
    return rc != NLSH_OK ? rc : bucket_scan_args(c, p);
}
static int step_scan_run(const BucketScanCall &c) {
    const int rc = step_scan_check(c);
    if (rc != NLSH_OK || c.Q == 0) return rc;
    return scan_call_run(c);
}

static bool fuses_lookup(const nlsh_step_desc_t &d) { return d.algo != NLSH_SCAN_QUERY_MAJOR && d.n_probes <= 64 && d.n_buckets > 0; }

// encode_hash with the bucket lookup in its epilogue when the schedule allows it; *plan_phase = what is left of the PLAN phase
static int launch_encode(EncPlan &enc, const nlsh_step_desc_t &d, const float *queries, int64_t q_stride, uint64_t seed, hipStream_t s, int *plan_phase,
                         int *plan_blocks) {
    *plan_phase = NLSH_PHASE_PLAN;
    *plan_blocks = 0;
    if (!fuses_lookup(d)) return encode_plan_launch(enc, queries, q_stride, seed, s);
    BucketScanPrep p;
    int rc = step_scan_prepare(step_scan_call(d, queries, q_stride, s, NLSH_PHASE_PLAN_REST), &p);
    if (rc == NLSH_OK) rc = encode_plan_fuse_lookup(enc, p.pa);   // idempotent: the first call of a slot sizes the coarse table's LDS
    if (rc != NLSH_OK) return rc;
    *plan_phase = NLSH_PHASE_PLAN_REST;
    *plan_blocks = (int)enc.grid;
    return encode_plan_launch(enc, queries, q_stride, seed, s, &p.pa);
}

static int make_event(hipEvent_t *e) {
    NLSH_CHECK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return NLSH_OK;
}

static int step_create(const nlsh_step_desc_t *desc, size_t desc_bytes, hipStream_t lane, nlsh_step_t **out) {
    NLSH_REQUIRE(desc && out, NLSH_E_INVALID, "step_create: null pointer");
    NLSH_REQUIRE(desc_bytes == sizeof(nlsh_step_desc_t), NLSH_E_INVALID, "step_create: descriptor of %zu bytes, this library's is %zu (ABI %d)",
                 desc_bytes, sizeof(nlsh_step_desc_t), NLSH_ABI_VERSION);
    if (lane == nullptr) {
        NLSH_REQUIRE(desc->front && desc->mid && desc->tail, NLSH_E_INVALID, "step_create: the front, mid and tail streams must be real streams (not the default stream)");
        NLSH_REQUIRE(desc->front != desc->mid && desc->mid != desc->tail && desc->front != desc->tail && desc->plan != desc->front && desc->plan != desc->mid &&
                         desc->plan != desc->tail,
                     NLSH_E_INVALID, "step_create: front, plan, mid and tail must be DIFFERENT streams (the stages overlap only across streams, and an event is recorded on one and waited for on the next)");
    }
    NLSH_REQUIRE(desc->n_layers >= 1 && desc->n_layers <= NLSH_MAX_LAYERS && desc->dims, NLSH_E_INVALID, "step_create: n_layers=%d", desc->n_layers);
    NLSH_REQUIRE(desc->n_probes >= 1 && desc->n_probes <= NLSH_MAX_PROBES, NLSH_E_UNSUPPORTED, "step_create: n_probes=%d not in [1,%d] (one scan call per batch)",
                 desc->n_probes, NLSH_MAX_PROBES);
    NLSH_REQUIRE(desc->Q >= 1 && desc->dims[0] == desc->d, NLSH_E_INVALID, "step_create: Q=%lld, encoder input %d vs corpus dimension %d", (long long)desc->Q,
                 desc->dims[0], desc->d);
    nlsh_step *s = new (std::nothrow) nlsh_step();
    NLSH_REQUIRE(s != nullptr, NLSH_E_INVALID, "step_create: out of host memory");
    s->d = *desc;
    for (int l = 0; l <= desc->n_layers; ++l) s->dims[l] = desc->dims[l];
    s->d.dims = s->dims;
    s->ready = s->encoded = s->planned = s->scanned = s->done = nullptr;
    s->done_pending = false;
    s->lane = lane; s->graph = nullptr; s->exec = nullptr; s->enc_node = s->scan_node = nullptr;
    s->graph_failed = getenv("NLSH_STEP_NO_GRAPH") != nullptr;    // diagnostic: a graph slot without its graph (what a failed capture leaves)
    const hipStream_t last = lane ? lane : (hipStream_t)desc->tail;    // the stream a batch ends on
    int rc = encode_plan_fill(s->enc, desc->Q, desc->n_layers, s->dims, desc->packed, desc->act, desc->key_mode, desc->n_probes, desc->n_multi_rows, 0,
                              nullptr, nullptr, nullptr, desc->qkeys, desc->nkeys);
    // the scan call's own argument checks (workspace alignment and size, strides, limits) run HERE, on a stand-in batch pointer, so
    // that a bad descriptor fails before anything is enqueued (they used to fail inside the first enqueue, behind its encode)
    if (rc == NLSH_OK) {
        const BucketScanCall c = step_scan_call(s->d, desc->corpus_sorted ? desc->corpus_sorted : (const float *)desc->workspace,
                                                desc->row_stride >= desc->d ? desc->row_stride : desc->d, last, NLSH_PHASE_SCAN);
        if (desc->algo == NLSH_SCAN_QUERY_MAJOR) {
            rc = step_scan_check(c);
            if (rc == NLSH_OK) rc = query_major_workspace(c);
        } else {
            BucketScanPrep p;
            rc = step_scan_prepare(c, &p);
            if (rc == NLSH_OK && fuses_lookup(s->d)) rc = encode_plan_fuse_lookup(s->enc, p.pa);
        }
    }
    if (rc == NLSH_OK && lane != nullptr && !(fuses_lookup(s->d) && desc->max_tasks > 0)) {
        set_error("step_create_graph: graph slots take the bucket-major schedules (algo 1, 2) on a non-empty index and task table");
        rc = NLSH_E_UNSUPPORTED;
    }
    if (rc == NLSH_OK) rc = encode_plan_prepare(s->enc);     // the dynamic-LDS permission of the encode's form: not inside a capture
    if (rc == NLSH_OK) rc = make_event(&s->ready);
    if (rc == NLSH_OK && !lane) rc = make_event(&s->encoded);
    if (rc == NLSH_OK && !lane) rc = make_event(&s->planned);
    if (rc == NLSH_OK && !lane) rc = make_event(&s->scanned);
    if (rc == NLSH_OK) rc = make_event(&s->done);
    if (rc == NLSH_OK && hipEventRecord(s->done, last) != hipSuccess) {   // the slot starts out free
        set_error("step_create: hipEventRecord failed");
        rc = NLSH_E_HIP;
    }
    if (rc != NLSH_OK) {
        nlsh_step_destroy(s);
        return rc;
    }
    *out = s;
    return NLSH_OK;
}

extern "C" int nlsh_step_create(const nlsh_step_desc_t *desc, size_t desc_bytes, nlsh_step_t **out) {
    return step_create(desc, desc_bytes, nullptr, out);
}

extern "C" int nlsh_step_create_graph(const nlsh_step_desc_t *desc, size_t desc_bytes, nlsh_stream_t lane, nlsh_step_t **out) {
    NLSH_REQUIRE(lane != nullptr, NLSH_E_INVALID, "step_create_graph: the slot's stream must be a real stream (not the default stream: it is captured)");
    return step_create(desc, desc_bytes, (hipStream_t)lane, out);
}

extern "C" int nlsh_step_destroy(nlsh_step_t *s) {
    if (!s) return NLSH_OK;
    for (hipEvent_t e : {s->ready, s->encoded, s->planned, s->scanned, s->done})
        if (e) (void)hipEventDestroy(e);
    if (s->exec) (void)hipGraphExecDestroy(s->exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    delete s;
    return NLSH_OK;
}

extern "C" int nlsh_step_set_weights(nlsh_step_t *s, const float *packed) {
    NLSH_REQUIRE(s && packed, NLSH_E_INVALID, "step_set_weights: null pointer");
    s->enc.a.packed = packed;
    s->d.packed = packed;
    return NLSH_OK;
}


// A graph slot's batch: the five launches replayed from the slot's captured graph on the slot's own stream.  Batches of different slots
// overlap because their streams do (the slot's previous batch precedes this one on the same stream: no event between them).  Per batch the
// host makes ONE graph launch, two node updates (the encode's batch pointer / stride / seed / lookup arguments, the scan's query
// pointer) and the `done` record -- r05's staged slots made seven launches and eight to ten event calls (~3.5 us each inside the runtime).
// With scan events requested the batch is launched eagerly on the same stream (an event record cannot be re-pointed in a graph).
static int graph_capture(nlsh_step *s, const float *queries, int64_t q_stride, uint64_t seed) {
    NLSH_CHECK_HIP(hipStreamBeginCapture(s->lane, hipStreamCaptureModeThreadLocal));
    int plan_phase, plan_blocks;
    int rc = launch_encode(s->enc, s->d, queries, q_stride, seed, s->lane, &plan_phase, &plan_blocks);
    BucketScanCall rest = step_scan_call(s->d, queries, q_stride, s->lane, plan_phase | SCAN_AND_MERGE);
    rest.plan_blocks = plan_blocks;
    if (rc == NLSH_OK) rc = step_scan_run(rest);
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(s->lane, &g);
    if (rc != NLSH_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    NLSH_CHECK_HIP(ce);
    s->graph = g;
    // the two nodes whose arguments change per batch, found by their kernels
    EncNode en;
    ScanNode sn;
    const BucketScanCall c = step_scan_call(s->d, queries, q_stride, s->lane, NLSH_PHASE_SCAN);
    rc = step_scan_check(c);
    if (rc == NLSH_OK) rc = bucket_scan_node(c, &sn);
    if (rc == NLSH_OK) rc = encode_plan_node(s->enc, queries, q_stride, seed, nullptr, &en);
    if (rc != NLSH_OK) return rc;
    size_t n = 0;
    NLSH_CHECK_HIP(hipGraphGetNodes(g, nullptr, &n));
    hipGraphNode_t nodes[16];
    NLSH_REQUIRE(n >= 2 && n <= 16, NLSH_E_HIP, "step graph: %zu nodes captured", n);
    NLSH_CHECK_HIP(hipGraphGetNodes(g, nodes, &n));
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType t;
        NLSH_CHECK_HIP(hipGraphNodeGetType(nodes[i], &t));
        if (t != hipGraphNodeTypeKernel) continue;
        hipKernelNodeParams kp;
        NLSH_CHECK_HIP(hipGraphKernelNodeGetParams(nodes[i], &kp));
        if (kp.func == en.p.func) s->enc_node = nodes[i];
        else if (kp.func == sn.p.func) s->scan_node = nodes[i];
    }
    NLSH_REQUIRE(s->enc_node && s->scan_node, NLSH_E_HIP, "step graph: the encode / scan nodes were not found among the %zu captured", n);
    NLSH_CHECK_HIP(hipGraphInstantiate(&s->exec, g, nullptr, nullptr, 0));
    return NLSH_OK;
}

static int graph_enqueue(nlsh_step *s, const float *queries, int64_t q_stride, uint64_t seed, nlsh_stream_t producer, void *ev0, void *ev1) {
    const hipStream_t lane = s->lane;
    if ((hipStream_t)producer != lane) {    // the batch may still be in flight on the stream that produced it (as for the staged slots)
        const hipError_t qe = hipStreamQuery((hipStream_t)producer);
        if (qe == hipErrorNotReady) {
            (void)hipGetLastError();
            NLSH_CHECK_HIP(hipEventRecord(s->ready, (hipStream_t)producer));
            NLSH_CHECK_HIP(hipStreamWaitEvent(lane, s->ready, 0));
        } else {
            NLSH_CHECK_HIP(qe);
        }
    }
    int rc;
    if (!s->exec && !s->graph_failed && !(ev0 || ev1)) {
        // Captured once.  A runtime that cannot capture or instantiate the batch (nothing has been launched by a failed capture) leaves the
        // slot what a graph slot is without its graph: the same five launches, eagerly, on the slot's own stream -- same results, same
        // overlap between slots, ~0.005 ms more host time per batch (profiles/r06_shard_step_profile_eager_on_lane_vs_staged.jsonl).
        if (graph_capture(s, queries, q_stride, seed) != NLSH_OK) {
            s->graph_failed = true;
            if (s->exec) { (void)hipGraphExecDestroy(s->exec); s->exec = nullptr; }
            if (s->graph) { (void)hipGraphDestroy(s->graph); s->graph = nullptr; }
            (void)hipGetLastError();
        }
    }
    if (ev0 || ev1 || !s->exec) {
        int plan_phase, plan_blocks;
        rc = launch_encode(s->enc, s->d, queries, q_stride, seed, lane, &plan_phase, &plan_blocks);
        BucketScanCall rest = step_scan_call(s->d, queries, q_stride, lane, plan_phase | SCAN_AND_MERGE);
        rest.plan_blocks = plan_blocks; rest.ev_begin = ev0; rest.ev_end = ev1;
        if (rc == NLSH_OK) rc = step_scan_run(rest);
        if (rc != NLSH_OK) return rc;
    } else {
        // this batch's arguments of the two nodes that carry them
        const BucketScanCall c = step_scan_call(s->d, queries, q_stride, lane, NLSH_PHASE_SCAN);
        BucketScanPrep p;
        EncNode en;
        ScanNode sn;
        rc = step_scan_prepare(c, &p);
        if (rc == NLSH_OK) rc = encode_plan_fuse_lookup(s->enc, p.pa);
        if (rc == NLSH_OK) rc = encode_plan_node(s->enc, queries, q_stride, seed, &p.pa, &en);
        if (rc == NLSH_OK) rc = bucket_scan_node(c, &sn);
        if (rc != NLSH_OK) return rc;
        NLSH_CHECK_HIP(hipGraphExecKernelNodeSetParams(s->exec, s->enc_node, &en.p));
        NLSH_CHECK_HIP(hipGraphExecKernelNodeSetParams(s->exec, s->scan_node, &sn.p));
        NLSH_CHECK_HIP(hipGraphLaunch(s->exec, lane));
    }
    if (s->d.hold_done) s->done_pending = true;     // the caller queues more work on the slot's stream (the shard exchange) first
    else NLSH_CHECK_HIP(hipEventRecord(s->done, lane));
    return NLSH_OK;
}

extern "C" int nlsh_query_step_enqueue(nlsh_step_t *s, const float *queries, int64_t q_stride, uint64_t seed, nlsh_stream_t producer,
                                       void *ev_scan_begin, void *ev_scan_end) {
    NLSH_REQUIRE(s && queries, NLSH_E_INVALID, "query_step_enqueue: null pointer");
    NLSH_REQUIRE(!s->done_pending, NLSH_E_INVALID, "query_step_enqueue: the slot's previous batch was not released (nlsh_step_release)");
    if (s->lane) return graph_enqueue(s, queries, q_stride, seed, producer, ev_scan_begin, ev_scan_end);
    const hipStream_t front = (hipStream_t)s->d.front, mid = (hipStream_t)s->d.mid, tail = (hipStream_t)s->d.tail;
    NLSH_CHECK_HIP(hipStreamWaitEvent(front, s->done, 0));            // the slot's previous batch has left the tail: its buffers are free
    // The batch may still be in flight on the stream that produced it.  NULL is a stream like any other here -- the default stream, where
    // torch produces a tensor unless told otherwise -- and the stage streams are non-blocking ones that do NOT order themselves behind it.
    // A producer stream with nothing in flight (one query, ~1 us: the steady state of a loop over batches made earlier) needs no event.
    bool wait_producer = (hipStream_t)producer != front;
    if (wait_producer) {
        const hipError_t qe = hipStreamQuery((hipStream_t)producer);
        if (qe == hipSuccess) wait_producer = false;
        else if (qe == hipErrorNotReady) (void)hipGetLastError();     // an answer, not a failure
        else NLSH_CHECK_HIP(qe);
    }
    if (wait_producer) {
        NLSH_CHECK_HIP(hipEventRecord(s->ready, (hipStream_t)producer));
        NLSH_CHECK_HIP(hipStreamWaitEvent(front, s->ready, 0));
    }
    int plan_phase, plan_blocks;
    int rc = launch_encode(s->enc, s->d, queries, q_stride, seed, front, &plan_phase, &plan_blocks);
    if (rc != NLSH_OK) return rc;
    hipStream_t hp = front;
    if (s->d.plan) {                                                  // four stages: the PLAN phase on a stream of its own behind the encode
        hp = (hipStream_t)s->d.plan;
        NLSH_CHECK_HIP(hipEventRecord(s->encoded, front));
        NLSH_CHECK_HIP(hipStreamWaitEvent(hp, s->encoded, 0));
    }
    BucketScanCall c = step_scan_call(s->d, queries, q_stride, hp, plan_phase);
    c.plan_blocks = plan_blocks;
    rc = step_scan_run(c);
    if (rc != NLSH_OK) return rc;
    NLSH_CHECK_HIP(hipEventRecord(s->planned, hp));
    NLSH_CHECK_HIP(hipStreamWaitEvent(mid, s->planned, 0));
    c = step_scan_call(s->d, queries, q_stride, mid, NLSH_PHASE_SCAN);
    c.ev_begin = ev_scan_begin; c.ev_end = ev_scan_end;
    rc = step_scan_run(c);
    if (rc != NLSH_OK) return rc;
    NLSH_CHECK_HIP(hipEventRecord(s->scanned, mid));
    NLSH_CHECK_HIP(hipStreamWaitEvent(tail, s->scanned, 0));
    rc = step_scan_run(step_scan_call(s->d, queries, q_stride, tail, NLSH_PHASE_MERGE));
    if (rc != NLSH_OK) return rc;
    if (s->d.hold_done) s->done_pending = true;                       // the caller queues more work on the tail stream (the shard exchange) first
    else NLSH_CHECK_HIP(hipEventRecord(s->done, tail));
    return NLSH_OK;
}

extern "C" int nlsh_step_release(nlsh_step_t *s) {
    NLSH_REQUIRE(s, NLSH_E_INVALID, "step_release: null pointer");
    NLSH_CHECK_HIP(hipEventRecord(s->done, s->lane ? s->lane : (hipStream_t)s->d.tail));
    s->done_pending = false;
    return NLSH_OK;
}

extern "C" int nlsh_step_busy(nlsh_step_t *s) {
    NLSH_REQUIRE(s, NLSH_E_INVALID, "step_busy: null pointer");
    if (s->done_pending) return 1;
    const hipError_t e = hipEventQuery(s->done);
    if (e == hipSuccess) return 0;
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();   // "not ready" is an answer, not a failure: do not leave it behind as the thread's last HIP error
        return 1;
    }
    set_error("hipEventQuery failed: %s", hipGetErrorString(e));
    return NLSH_E_HIP;
}

// The same batch on ONE stream, nothing kept between calls (the streams and hold_done of `desc` are ignored): encode_hash with the
// bucket lookup in its epilogue, then bscan, bscatter, the scan kernel and bmerge -- five launches.  `lookup_done` != 0 repeats the
// scan part only, on keys (and their lookup) an earlier call of the same batch left in `qkeys` / the workspace: the retry after a
// task-table overflow (status[1] = 1; the lookup's records sit at workspace offsets that do not depend on max_tasks), with the
// lookup redone by the stand-alone kernel.
extern "C" int nlsh_query_batch(const nlsh_step_desc_t *desc, size_t desc_bytes, const float *queries, int64_t q_stride, uint64_t seed, int64_t row0,
                                int lookup_done, void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream) {
    NLSH_REQUIRE(desc, NLSH_E_INVALID, "query_batch: null pointer");
    NLSH_REQUIRE(desc_bytes == sizeof(nlsh_step_desc_t), NLSH_E_INVALID, "query_batch: descriptor of %zu bytes, this library's is %zu (ABI %d)", desc_bytes,
                 sizeof(nlsh_step_desc_t), NLSH_ABI_VERSION);
    NLSH_REQUIRE(desc->Q >= 0, NLSH_E_INVALID, "query_batch: Q=%lld", (long long)desc->Q);
    if (desc->Q == 0) return NLSH_OK;
    NLSH_REQUIRE(queries, NLSH_E_INVALID, "query_batch: null pointer");
    NLSH_REQUIRE(desc->n_layers >= 1 && desc->n_layers <= NLSH_MAX_LAYERS && desc->dims && desc->dims[0] == desc->d, NLSH_E_INVALID,
                 "query_batch: n_layers=%d, encoder input vs corpus dimension %d", desc->n_layers, desc->d);
    NLSH_REQUIRE(desc->n_probes >= 1 && desc->n_probes <= NLSH_MAX_PROBES, NLSH_E_UNSUPPORTED, "query_batch: n_probes=%d not in [1,%d] (one scan call per batch)",
                 desc->n_probes, NLSH_MAX_PROBES);
    hipStream_t s = (hipStream_t)stream;
    int plan_phase = NLSH_PHASE_PLAN, plan_blocks = 0;
    if (!lookup_done) {
        EncPlan enc;
        int rc = encode_plan_fill(enc, desc->Q, desc->n_layers, desc->dims, desc->packed, desc->act, desc->key_mode, desc->n_probes, desc->n_multi_rows, row0, nullptr,
                                  nullptr, nullptr, desc->qkeys, desc->nkeys);
        if (rc == NLSH_OK) rc = launch_encode(enc, *desc, queries, q_stride, seed, s, &plan_phase, &plan_blocks);
        if (rc != NLSH_OK) return rc;
    }
    BucketScanCall rest = step_scan_call(*desc, queries, q_stride, s, plan_phase | SCAN_AND_MERGE);
    rest.plan_blocks = plan_blocks; rest.ev_begin = ev_scan_begin; rest.ev_end = ev_scan_end;
    return step_scan_run(rest);
}

// The merge's host-writing form stores through the DEVICE's address of the result block: it must be host memory the runtime has mapped
// for the device (hipHostMalloc / hipHostRegister, a pinned tensor), from its first word to its last.
static int host_block_mapped(const char *who, const int32_t *host_out, size_t need, int32_t **mapped) {
    *mapped = nullptr;
    for (const int32_t *p : {host_out, host_out + (need - 1)}) {
        hipPointerAttribute_t at;
        const hipError_t e = hipPointerGetAttributes(&at, p);
        if (e != hipSuccess) (void)hipGetLastError();     // memory the runtime does not know: an answer, not a failure to keep
        NLSH_REQUIRE(e == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer != nullptr, NLSH_E_INVALID,
                     "%s: host_out is not host memory mapped for the device (hipHostMalloc / hipHostRegister; a device pointer is refused)", who);
        if (!*mapped) *mapped = (int32_t *)at.devicePointer;
    }
    return NLSH_OK;
}

// nlsh_query_batch for a caller that wants the batch's results on the HOST (`Indexer.query`): the same five launches, the last one the
// host-writing form of the merge (scan_bucket_merge.h, bmerge_host_kernel), which stores ids, candidate counts, the status words and the
// key rows of the queries with fewer than k candidates straight into `host_out` -- no device->host copy command follows the kernels.
// Every argument is checked before anything is enqueued.
extern "C" int nlsh_query_batch_host(const nlsh_step_desc_t *desc, size_t desc_bytes, const float *queries, int64_t q_stride, uint64_t seed, int64_t row0,
                                     int lookup_done, int32_t *host_out, size_t host_words, nlsh_stream_t stream) {
    NLSH_REQUIRE(desc, NLSH_E_INVALID, "query_batch_host: null pointer");
    NLSH_REQUIRE(desc_bytes == sizeof(nlsh_step_desc_t), NLSH_E_INVALID, "query_batch_host: descriptor of %zu bytes, this library's is %zu (ABI %d)", desc_bytes,
                 sizeof(nlsh_step_desc_t), NLSH_ABI_VERSION);
    NLSH_REQUIRE(desc->Q >= 0 && desc->Q < (1ll << 31), NLSH_E_INVALID, "query_batch_host: Q=%lld", (long long)desc->Q);
    NLSH_REQUIRE(host_out, NLSH_E_INVALID, "query_batch_host: host_out is null");
    NLSH_REQUIRE(desc->k >= 1 && desc->k <= NLSH_MAX_K, NLSH_E_INVALID, "query_batch_host: k=%d not in [1,%d] (the host-writing merge; nlsh_query_batch takes wider k)",
                 desc->k, NLSH_MAX_K);
    NLSH_REQUIRE(desc->algo == NLSH_SCAN_BUCKET_MAJOR || desc->algo == NLSH_SCAN_BUCKET_TILED, NLSH_E_INVALID,
                 "query_batch_host: algo=%d: only the bucket-major schedules (1, 2) have a host-writing merge", desc->algo);
    NLSH_REQUIRE(desc->n_probes >= 1 && desc->n_probes <= NLSH_MAX_PROBES, NLSH_E_UNSUPPORTED, "query_batch_host: n_probes=%d not in [1,%d] (one scan call per batch)",
                 desc->n_probes, NLSH_MAX_PROBES);
    const size_t need = (size_t)desc->Q * (size_t)(desc->k + 1 + desc->n_probes + 1) + 2;   // ids | counts | status | key rows
    NLSH_REQUIRE(host_words >= need, NLSH_E_INVALID, "query_batch_host: host_out of %zu words, Q=%lld k=%d n_probes=%d need %zu", host_words, (long long)desc->Q,
                 desc->k, desc->n_probes, need);
    if (desc->Q == 0) return NLSH_OK;
    NLSH_REQUIRE(queries, NLSH_E_INVALID, "query_batch_host: null pointer");
    NLSH_REQUIRE(desc->n_layers >= 1 && desc->n_layers <= NLSH_MAX_LAYERS && desc->dims && desc->dims[0] == desc->d, NLSH_E_INVALID,
                 "query_batch_host: n_layers=%d, encoder input vs corpus dimension %d", desc->n_layers, desc->d);
    int32_t *mapped = nullptr;
    if (const int mrc = host_block_mapped("query_batch_host", host_out, need, &mapped)) return mrc;
    hipStream_t s = (hipStream_t)stream;
    // the scan call's own checks and its workspace size, on the host, before the encode is launched
    BucketScanCall c = step_scan_call(*desc, queries, q_stride, s, NLSH_PHASE_PLAN | SCAN_AND_MERGE);
    BucketScanPrep p;
    int rc = step_scan_prepare(c, &p);
    if (rc != NLSH_OK) return rc;
    int plan_phase = NLSH_PHASE_PLAN, plan_blocks = 0;
    if (!lookup_done) {
        EncPlan enc;
        rc = encode_plan_fill(enc, desc->Q, desc->n_layers, desc->dims, desc->packed, desc->act, desc->key_mode, desc->n_probes, desc->n_multi_rows, row0, nullptr,
                              nullptr, nullptr, desc->qkeys, desc->nkeys);
        if (rc == NLSH_OK) rc = launch_encode(enc, *desc, queries, q_stride, seed, s, &plan_phase, &plan_blocks);
        if (rc != NLSH_OK) return rc;
    }
    c.phases = plan_phase | SCAN_AND_MERGE;
    c.plan_blocks = plan_blocks;
    c.host_out = mapped;
    return bucket_scan_run(c);
}

// The ranked multi-probe mode (nlsh_probe_ranked, optionally with nlsh_probe_ranked_budget's per-row stop) as ONE call of five launches:
// encode_hash with one probe, handing out z and the hard code; probe_ranked_plan_kernel (probe_ranked.hip), which ranks a row's keys into
// desc->qkeys / desc->nkeys AND looks them up -- the third home of the lookup of scan_plan.h --; then bscan, bscatter, the scan kernel and
// the merge (NLSH_PHASE_PLAN_REST | SCAN | MERGE).  The two-step form it replaces made seven: the key table went out to memory and came
// back through the stand-alone bplan_kernel.  Ranked keys are a function of the row alone: no seed, no row0.
struct RankedScratch {
    size_t z, code, keys, nkeys, total;
};
static void ranked_scratch_layout(int64_t Q, int H, RankedScratch *w) {
    const size_t rows = (size_t)(Q > 0 ? Q : 1);
    size_t o = 0;
    w->z = o;     o += ws_align(rows * (size_t)H * 4);
    w->code = o;  o += ws_align(rows * 4);
    w->keys = o;  o += ws_align(rows * 4);    // the one-probe encode's own [Q, 1] key table and counts: required outputs of the launch,
    w->nkeys = o; o += ws_align(rows * 4);    // read by nobody (the ranked kernel re-derives slot 0 from the hard code)
    w->total = o;
}

extern "C" size_t nlsh_query_batch_ranked_scratch(int64_t Q, int H) {
    if (Q < 0 || Q >= (1ll << 31) || H < 1 || H > NLSH_MAX_HASH_BITS) return 0;
    RankedScratch w;
    ranked_scratch_layout(Q, H, &w);
    return w.total;
}

extern "C" int nlsh_query_batch_ranked(const nlsh_step_desc_t *desc, size_t desc_bytes, const float *queries, int64_t q_stride, int lookup_done,
                                       int32_t budget, void *scratch, size_t scratch_bytes, int32_t *host_out, size_t host_words,
                                       void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream) {
    NLSH_REQUIRE(desc, NLSH_E_INVALID, "query_batch_ranked: null pointer");
    NLSH_REQUIRE(desc_bytes == sizeof(nlsh_step_desc_t), NLSH_E_INVALID, "query_batch_ranked: descriptor of %zu bytes, this library's is %zu (ABI %d)",
                 desc_bytes, sizeof(nlsh_step_desc_t), NLSH_ABI_VERSION);
    NLSH_REQUIRE(desc->Q >= 0 && desc->Q < (1ll << 31), NLSH_E_INVALID, "query_batch_ranked: Q=%lld", (long long)desc->Q);
    NLSH_REQUIRE(desc->algo == NLSH_SCAN_BUCKET_MAJOR || desc->algo == NLSH_SCAN_BUCKET_TILED, NLSH_E_INVALID,
                 "query_batch_ranked: algo=%d: the lookup rides in the ranking launch for the bucket-major schedules (1, 2) only", desc->algo);
    NLSH_REQUIRE(desc->n_buckets > 0, NLSH_E_INVALID, "query_batch_ranked: n_buckets=%d (an empty index has nothing to look up)", (int)desc->n_buckets);
    NLSH_REQUIRE(desc->n_probes >= 1 && desc->n_probes <= NLSH_MAX_PROBES, NLSH_E_UNSUPPORTED, "query_batch_ranked: n_probes=%d not in [1,%d] (one scan call per batch)",
                 desc->n_probes, NLSH_MAX_PROBES);
    NLSH_REQUIRE(desc->n_layers >= 1 && desc->n_layers <= NLSH_MAX_LAYERS && desc->dims && desc->dims[0] == desc->d, NLSH_E_INVALID,
                 "query_batch_ranked: n_layers=%d, encoder input vs corpus dimension %d", desc->n_layers, desc->d);
    const int H = desc->dims[desc->n_layers];
    NLSH_REQUIRE(H >= 1 && H <= NLSH_MAX_HASH_BITS, NLSH_E_UNSUPPORTED, "query_batch_ranked: H=%d not in [1, NLSH_MAX_HASH_BITS=%d]", H, NLSH_MAX_HASH_BITS);
    NLSH_REQUIRE(budget >= 0, NLSH_E_INVALID, "query_batch_ranked: budget=%d < 0 (0 = no budget)", (int)budget);
    RankedScratch w;
    ranked_scratch_layout(desc->Q, H, &w);
    NLSH_REQUIRE(scratch, NLSH_E_INVALID, "query_batch_ranked: scratch is null");
    NLSH_REQUIRE(scratch_bytes >= w.total, NLSH_E_WORKSPACE, "query_batch_ranked: scratch of %zu bytes, Q=%lld H=%d need %zu (nlsh_query_batch_ranked_scratch)",
                 scratch_bytes, (long long)desc->Q, H, w.total);
    size_t need = 0;
    if (host_out) {     // the host-writing merge: nlsh_query_batch_host's form and checks
        NLSH_REQUIRE(desc->k >= 1 && desc->k <= NLSH_MAX_K, NLSH_E_INVALID, "query_batch_ranked: k=%d not in [1,%d] (the host-writing merge; pass host_out = NULL for wider k)",
                     desc->k, NLSH_MAX_K);
        need = (size_t)desc->Q * (size_t)(desc->k + 1 + desc->n_probes + 1) + 2;   // ids | counts | status | key rows
        NLSH_REQUIRE(host_words >= need, NLSH_E_INVALID, "query_batch_ranked: host_out of %zu words, Q=%lld k=%d n_probes=%d need %zu", host_words,
                     (long long)desc->Q, desc->k, desc->n_probes, need);
    }
    if (desc->Q == 0) return NLSH_OK;
    NLSH_REQUIRE(queries, NLSH_E_INVALID, "query_batch_ranked: null pointer");
    int32_t *mapped = nullptr;
    if (host_out)
        if (const int mrc = host_block_mapped("query_batch_ranked", host_out, need, &mapped)) return mrc;
    hipStream_t s = (hipStream_t)stream;
    // the scan call's own checks and its workspace size, on the host, before anything is launched
    BucketScanCall c = step_scan_call(*desc, queries, q_stride, s, NLSH_PHASE_PLAN | SCAN_AND_MERGE);
    c.ev_begin = ev_scan_begin; c.ev_end = ev_scan_end;
    BucketScanPrep p;
    int rc = step_scan_prepare(c, &p);
    if (rc != NLSH_OK) return rc;
    int plan_phase = NLSH_PHASE_PLAN, plan_blocks = 0;
    if (!lookup_done) {
        char *base = (char *)scratch;
        float *z = (float *)(base + w.z);
        uint32_t *code = (uint32_t *)(base + w.code);
        EncPlan enc;
        rc = encode_plan_fill(enc, desc->Q, desc->n_layers, desc->dims, desc->packed, desc->act, desc->key_mode, 1, desc->n_multi_rows, 0, z, nullptr, code,
                              (int32_t *)(base + w.keys), (int32_t *)(base + w.nkeys));
        if (rc == NLSH_OK) rc = encode_plan_launch(enc, queries, q_stride, 0, s);
        if (rc == NLSH_OK)
            rc = probe_ranked_plan_launch(z, H, code, H, desc->key_mode, desc->n_multi_rows, budget, p.pa, desc->qkeys, desc->nkeys, s, &plan_blocks);
        if (rc != NLSH_OK) return rc;
        plan_phase = NLSH_PHASE_PLAN_REST;
    }
    c.phases = plan_phase | SCAN_AND_MERGE;
    c.plan_blocks = plan_blocks;
    c.host_out = mapped;
    return bucket_scan_run(c);
}
