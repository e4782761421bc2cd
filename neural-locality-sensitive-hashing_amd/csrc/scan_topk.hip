// scan_topk: bucket lookup + candidate distance scan + top-k for a whole query batch.
//
// Replaces the host-driven per-query loop of Indexer.query (nlsh/indexer.py:62-95): dict lookup
// (:68), one index_select launch per (query, key) (:77-82), one distance launch per query
// (:84-87; nlsh/data.py:99-109, 191-201), cat (:88), topk + .tolist() with a device sync per
// query (:90-91).
//
// Three schedules, one contract (selected by `algo`; Indexer.choose_algo picks per batch):
//   0 QUERY-MAJOR (this file): one wavefront per (query, <= seg_rows candidates); every candidate row is
//     fetched once per query that probes it: the HBM-roofline design.  Best when buckets are small and few
//     queries share a bucket (balanced hash): a query's <= P buckets are walked by one wave.
//   1 BUCKET-MAJOR, wave level (scan_bucket.hip): one wavefront per (bucket segment, <= 8 queries held in
//     registers); same lane-partial + DPP tree arithmetic as 0, so 0 and 1 are bit-identical.
//   2 BUCKET-MAJOR, LDS-tiled (scan_bucket.hip): one workgroup per (256-row segment, <= 16 queries), lane
//     owns a row, k-ordered fmaf chain (bit-identical to the oracle), up to 16x less HBM traffic.
//
// gfx950 mapping of the query-major kernel (HBM-bound: 4*d bytes, 3*d flop per candidate)
//   * the corpus is bucket-contiguous (nlsh_gather_rows), so a query's candidate list is a
//     concatenation of <= P contiguous row ranges: streaming, not gathering;
//   * plan kernel: thread per query; binary search of each key in uniq_keys, prefix of bucket
//     sizes, candidates cut into segments of seg_rows -> one task per segment;
//   * scan kernel: ONE wavefront per task, one task per wave of the grid, so the hardware
//     workgroup dispatcher load-balances skewed buckets.  A wave walks its segment in tiles of
//     64 candidates.  LPR lanes cover one row with 16-byte loads (a wave-instruction fetches
//     64/LPR whole rows = 1 KiB, fully coalesced), U wave-loads are kept in flight, the
//     (q-c+eps)^2 / dot partials are reduced across the LPR lanes with DPP adds, and lane l ends
//     up owning exactly one candidate of the tile;
//   * per-wave top-k: the running best-64 (distance,id) keys live sorted across the 64 lanes;
//     a tile is filtered against the k-th key with one ballot and only survivors are inserted
//     (ballot + popcount + one lane shift), so the steady state costs ~3 instructions per tile;
//   * queries whose candidates span several tasks are combined by a small merge kernel with the
//     same comparator; nlsh_merge_topk does the same across corpus shards (multi-GPU).
#include "scan_common.h"

namespace nlsh {

struct ScanArgs {
    const float *corpus;
    long long row_stride;
    int d;
    const int32_t *gid;
    const int32_t *uniq;
    const int32_t *offsets;
    int nb;
    const float *inv_norm;
    const float *queries;
    long long q_stride;
    long long Q;
    const int32_t *qkeys;
    const int32_t *nkeys;
    int P, k, metric, seg;
    float *out_dist;
    int32_t *out_idx;
    uint64_t *out_keys;
    int32_t *out_ncand;
    int32_t *status;
    // workspace
    int32_t *pstart, *pcum, *nseg, *tbase, *task_q, *task_s;
    uint64_t *partial;
    long long max_tasks;
};

// ------------------------------------------------------------------------------------ plan
__global__ __launch_bounds__(256) void plan_kernel(ScanArgs a) {
    __shared__ int32_t wsum[4];
    __shared__ int32_t base_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long q = (long long)blockIdx.x * 256 + tid;
    int32_t C = 0, ns = 0;
    if (q < a.Q) {
        int nk = a.nkeys[q];
        nk = nk < 0 ? 0 : (nk > a.P ? a.P : nk);
        for (int p = 0; p < a.P; ++p) {
            int32_t st = 0, sz = 0;
            if (p < nk) {
                const int32_t key = a.qkeys[q * a.P + p];
                bool dup = false;       // a query's keys are a set (nlsh/utils.pyx:27-31): a repeated key probes its bucket once
                for (int pp = 0; pp < p; ++pp) dup |= a.qkeys[q * a.P + pp] == key;
                int lo = 0, hi = dup ? 0 : a.nb;  // lower_bound in the ascending bucket keys
                while (lo < hi) {
                    int mid = (lo + hi) >> 1;
                    if (a.uniq[mid] < key) lo = mid + 1; else hi = mid;
                }
                if (!dup && lo < a.nb && a.uniq[lo] == key) {  // unknown key = empty bucket (indexer.py:61,68)
                    st = a.offsets[lo];
                    sz = a.offsets[lo + 1] - st;
                }
            }
            a.pstart[q * a.P + p] = st;
            a.pcum[q * a.P + p] = C;
            C += sz;
        }
        ns = (C + a.seg - 1) / a.seg;
        a.out_ncand[q] = C;  // n_candidates, indexer.py:71,94
        if (C == 0)  // no task will touch this query: write the empty result here
            for (int i = 0; i < a.k; ++i) store_topk(a.out_dist, a.out_idx, a.out_keys, q, a.k, KEY_NONE, i);
    }
    // block-exclusive scan of ns, one atomic per block for the global task base
    int32_t incl = ns;
    for (int m = 1; m < 64; m <<= 1) {
        int32_t t = __shfl_up(incl, m);
        if (lane >= m) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int32_t woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    if (tid == 0) {
        int32_t tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        base_s = tot ? atomicAdd(&a.status[0], tot) : 0;
    }
    __syncthreads();
    if (q < a.Q) {
        const int32_t tb = base_s + woff + incl - ns;
        a.nseg[q] = ns;
        a.tbase[q] = tb;
        for (int s = 0; s < ns; ++s) {
            long long t = (long long)tb + s;
            if (t < a.max_tasks) { a.task_q[t] = (int32_t)q; a.task_s[t] = s; }
        }
    }
}

// ------------------------------------------------------------------------------------ scan
// LPR lanes cover one row, VPL 16-byte words per lane (d4 = ceil(d/4) <= LPR*VPL).
template <int LPR, int VPL, int METRIC>
__global__ __launch_bounds__(256) void scan_kernel(ScanArgs a) {
    constexpr int RPI = 64 / LPR;              // rows per wave-load
    constexpr int U = (VPL == 1) ? 8 : (VPL == 2 ? 4 : 2);  // wave-loads in flight
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    long long ntasks = a.status[0];
    if (ntasks > a.max_tasks) {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.status[1] = 1;  // incomplete: caller must retry
        ntasks = a.max_tasks;
    }
    if (t >= ntasks) return;

    const long long q = __builtin_amdgcn_readfirstlane(a.task_q[t]);
    const int s = __builtin_amdgcn_readfirstlane(a.task_s[t]);
    const int C = __builtin_amdgcn_readfirstlane(a.out_ncand[q]);
    const int nk = __builtin_amdgcn_readfirstlane(a.nkeys[q]);
    const int v0 = s * a.seg;
    const int v1 = min(C, v0 + a.seg);

    // probe table, one probe per lane
    int cum_l = 0x7FFFFFFF, st_l = 0;
    if (lane < a.P) { cum_l = a.pcum[q * a.P + lane]; st_l = a.pstart[q * a.P + lane]; }
    const int np = nk < a.P ? nk : a.P;

    const int li = lane % LPR, sub = lane / LPR;
    float4 qv[VPL];
    bool act[VPL];
    load_query<LPR, VPL, METRIC>(a.queries + q * a.q_stride, a.d, li, qv, act);

    const float4 *corpus4 = reinterpret_cast<const float4 *>(a.corpus);
    const long long stride4 = a.row_stride >> 2;
    uint64_t top = KEY_NONE, tau = KEY_NONE;

    for (int tile0 = v0; tile0 < v1; tile0 += 64) {
        const int ntile = min(64, v1 - tile0);            // wave-uniform
        const int myc = li * RPI + sub;                   // candidate of the tile this lane owns
        const bool valid = myc < ntile;
        const int myv = tile0 + myc;
        int pidx = -1;                                    // last probe whose first candidate <= myv
        for (int p = 0; p < np; ++p) pidx += (myv >= __builtin_amdgcn_readlane(cum_l, p)) ? 1 : 0;
        pidx = valid ? pidx : 0;
        const int stp = __shfl(st_l, pidx), cmp = __shfl(cum_l, pidx);
        const int prow = valid ? stp + (myv - cmp) : 0;   // row in the bucket-sorted corpus
        const int32_t mygid = valid ? a.gid[prow] : -1;
        float myinv = 0.0f;
        if (METRIC == NLSH_METRIC_COSINE) myinv = valid ? a.inv_norm[prow] : 0.0f;
        float mydist = __builtin_inff();

        for (int j0 = 0; j0 * RPI < ntile; j0 += U) {
            float4 cv[U][VPL];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u;
                const int row = __shfl(prow, sub * LPR + j);
                const bool ok = j * RPI + sub < ntile;
                const float4 *rp = corpus4 + (long long)row * stride4 + li;
#pragma unroll
                for (int v = 0; v < VPL; ++v)
                    cv[u][v] = (ok && act[v]) ? rp[v * LPR] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float tot = group_sum<LPR>(row_partial<VPL, METRIC>(qv, act, cv[u]));
                if (li == j0 + u) mydist = tot;
            }
        }
        const float dist = finish_distance<METRIC>(mydist, myinv);
        const uint64_t key = valid ? make_key(dist, mygid) : KEY_NONE;
        topk_offer(top, tau, key, a.k, lane);
    }

    const int ns = __builtin_amdgcn_readfirstlane(a.nseg[q]);
    if (ns == 1) store_topk(a.out_dist, a.out_idx, a.out_keys, q, a.k, top, lane);
    else if (lane < a.k) a.partial[t * a.k + lane] = top;
}

// ------------------------------------------------------------------------------------ merge
__global__ __launch_bounds__(256) void merge_segments_kernel(ScanArgs a) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.Q) return;
    const int ns = __builtin_amdgcn_readfirstlane(a.nseg[q]);
    if (ns <= 1) return;
    const long long tb = __builtin_amdgcn_readfirstlane(a.tbase[q]);
    uint64_t top = KEY_NONE, tau = KEY_NONE;
    for (int s = 0; s < ns; ++s) {
        const long long t = tb + s;
        if (t >= a.max_tasks) break;  // overflow: status[1] already set by scan_kernel
        const uint64_t key = lane < a.k ? a.partial[t * a.k + lane] : KEY_NONE;
        topk_offer(top, tau, key, a.k, lane);
    }
    store_topk(a.out_dist, a.out_idx, a.out_keys, q, a.k, top, lane);
}

__global__ __launch_bounds__(256) void merge_shards_kernel(const uint64_t *keys_in, long long row_stride, int G, long long Q, int k,
                                                            const int32_t *ncand_in, float *out_dist, int32_t *out_idx,
                                                            int32_t *out_ncand) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    // G shard lists of k keys: 3 x (64 / k) lists per round, the k best of them and of the best so far SELECTED
    // (merge_round), ranked and stored at the end -- no ordered insertion
    const int R = 64 / k, r = lane / k, e = lane - r * k;
    __shared__ uint64_t scratch[4][64];
    uint64_t *sc = scratch[threadIdx.x >> 6];
    uint64_t carry = KEY_NONE;
    for (int base = 0; base < G; base += 3 * R) {
        uint64_t key[4];
        key[0] = carry;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int g = base + s * R + r;
            key[s + 1] = (r < R && g < G) ? keys_in[((long long)g * Q + q) * row_stride + e] : KEY_NONE;
        }
        carry = merge_round<4>(key, k, lane, sc);
    }
    merge_finish(carry, k, lane, out_dist, out_idx, nullptr, q);
    if (out_ncand && (ncand_in || row_stride > k)) {
        int32_t nc = 0;
        for (int g = lane; g < G; g += 64) nc += ncand_in ? ncand_in[(long long)g * Q + q] : (int32_t)keys_in[((long long)g * Q + q) * row_stride + k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nc += __shfl_xor(nc, m);
        if (lane == 0) out_ncand[q] = nc;
    }
}

// merge_shards_kernel for k in 65..NLSH_MAX_K_TILED: KPL = ceil(k / 64) keys per lane, NL shard lists per round beside the carry
template <int KPL>
__global__ __launch_bounds__(256) void merge_shards_wide_kernel(const uint64_t *keys_in, long long row_stride, int G, long long Q, int k,
                                                                 const int32_t *ncand_in, float *out_dist, int32_t *out_idx,
                                                                 int32_t *out_ncand) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    constexpr int NL = KPL == 2 ? 3 : 1;
    __shared__ uint64_t scratch[4][NLSH_MAX_K_TILED];
    uint64_t *sc = scratch[threadIdx.x >> 6];
    uint64_t carry[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) carry[i] = KEY_NONE;
    for (int base = 0; base < G; base += NL) {
        uint64_t key[KPL * (1 + NL)];
#pragma unroll
        for (int i = 0; i < KPL; ++i) key[i] = carry[i];
#pragma unroll
        for (int s = 0; s < NL; ++s) {
            const int g = base + s;
#pragma unroll
            for (int i = 0; i < KPL; ++i)
                key[KPL * (1 + s) + i] = (g < G && i * 64 + lane < k) ? keys_in[((long long)g * Q + q) * row_stride + i * 64 + lane] : KEY_NONE;
        }
        merge_round_wide(key, carry, k, lane, sc);
    }
    merge_finish_wide(carry, sc, k, lane, out_dist, out_idx, nullptr, q);
    if (out_ncand && (ncand_in || row_stride > k)) {
        int32_t nc = 0;
        for (int g = lane; g < G; g += 64) nc += ncand_in ? ncand_in[(long long)g * Q + q] : (int32_t)keys_in[((long long)g * Q + q) * row_stride + k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nc += __shfl_xor(nc, m);
        if (lane == 0) out_ncand[q] = nc;
    }
}

struct ScanWs {
    size_t pstart, pcum, nseg, tbase, task_q, task_s, partial, total;
};
static void scan_layout(long long Q, int P, int k, long long max_tasks, ScanWs *w) {
    size_t o = 0;
    w->pstart = o; o += ws_align((size_t)Q * P * 4);
    w->pcum = o;   o += ws_align((size_t)Q * P * 4);
    w->nseg = o;   o += ws_align((size_t)Q * 4);
    w->tbase = o;  o += ws_align((size_t)Q * 4);
    w->task_q = o; o += ws_align((size_t)max_tasks * 4);
    w->task_s = o; o += ws_align((size_t)max_tasks * 4);
    w->partial = o; o += ws_align((size_t)max_tasks * k * 8);
    w->total = o;
}

template <int METRIC>
static void launch_scan(const ScanArgs &a, int d4, unsigned grid, hipStream_t s) {
    if (d4 <= 16) hipLaunchKernelGGL((scan_kernel<16, 1, METRIC>), dim3(grid), dim3(256), 0, s, a);
    else if (d4 <= 32) hipLaunchKernelGGL((scan_kernel<32, 1, METRIC>), dim3(grid), dim3(256), 0, s, a);
    else if (d4 <= 64) hipLaunchKernelGGL((scan_kernel<64, 1, METRIC>), dim3(grid), dim3(256), 0, s, a);
    else if (d4 <= 128) hipLaunchKernelGGL((scan_kernel<64, 2, METRIC>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((scan_kernel<64, 4, METRIC>), dim3(grid), dim3(256), 0, s, a);
}

// ScanArgs of a call: the query-major layout of its workspace, held against workspace_bytes
static int query_major_args(const BucketScanCall &c, ScanArgs *args) {
    ScanWs w;
    scan_layout(c.Q, c.P, c.k, c.max_tasks, &w);
    NLSH_REQUIRE(c.workspace_bytes >= w.total, NLSH_E_WORKSPACE, "scan_topk: workspace %zu < %zu", c.workspace_bytes, w.total);
    ScanArgs &a = *args;
    a.corpus = c.corpus; a.row_stride = c.row_stride; a.d = c.d; a.gid = c.gid; a.uniq = c.uniq; a.offsets = c.offsets;
    a.nb = c.nb; a.inv_norm = c.inv_norm; a.queries = c.queries; a.q_stride = c.q_stride; a.Q = c.Q; a.qkeys = c.qkeys;
    a.nkeys = c.nkeys; a.P = c.P; a.k = c.k; a.seg = scan_seg_rows(c.seg); a.out_dist = c.out_dist; a.out_idx = c.out_idx;
    a.out_keys = c.out_keys; a.out_ncand = c.out_ncand; a.status = c.status; a.max_tasks = c.max_tasks;
    // the folded form exists in the tiled schedule only; the exact form is inside its tolerance
    a.metric = c.metric == NLSH_METRIC_L2_EPS_FOLDED ? NLSH_METRIC_L2_EPS : c.metric;
    char *base = (char *)c.workspace;
    a.pstart = (int32_t *)(base + w.pstart); a.pcum = (int32_t *)(base + w.pcum); a.nseg = (int32_t *)(base + w.nseg);
    a.tbase = (int32_t *)(base + w.tbase); a.task_q = (int32_t *)(base + w.task_q); a.task_s = (int32_t *)(base + w.task_s);
    a.partial = (uint64_t *)(base + w.partial);
    return NLSH_OK;
}

int query_major_workspace(const BucketScanCall &c) {
    ScanArgs a;
    return query_major_args(c, &a);
}

// The query-major schedule of a checked call: plan, scan, merge (bucket_scan_run is the same for the two bucket-major schedules)
int query_major_run(const BucketScanCall &c) {
    ScanArgs a;
    const int rc = query_major_args(c, &a);
    if (rc != NLSH_OK) return rc;
    hipStream_t s = c.stream;
    if (c.phases & NLSH_PHASE_PLAN) {
        NLSH_CHECK_HIP(hipMemsetAsync(c.status, 0, 2 * sizeof(int32_t), s));
        hipLaunchKernelGGL(plan_kernel, dim3((unsigned)((c.Q + 255) / 256)), dim3(256), 0, s, a);
    }
    if ((c.phases & NLSH_PHASE_SCAN) && c.max_tasks > 0) {
        const unsigned grid = (unsigned)((c.max_tasks + 3) / 4);
        const int d4 = (c.d + 3) / 4;
        if (c.ev_begin) NLSH_CHECK_HIP(hipEventRecord((hipEvent_t)c.ev_begin, s));
        if (a.metric == NLSH_METRIC_L2_EPS) launch_scan<NLSH_METRIC_L2_EPS>(a, d4, grid, s);
        else launch_scan<NLSH_METRIC_COSINE>(a, d4, grid, s);
        if (c.ev_end) NLSH_CHECK_HIP(hipEventRecord((hipEvent_t)c.ev_end, s));
    }
    if ((c.phases & NLSH_PHASE_MERGE) && c.max_tasks > 0)
        hipLaunchKernelGGL(merge_segments_kernel, dim3((unsigned)((c.Q + 3) / 4)), dim3(256), 0, s, a);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

// the pitch of the corpus rows: a multiple of 16 bytes -- 4 float32 / 8 float16 / 16 uint8 elements -- from a 16-byte aligned base
static int corpus_pitch_check(const char *who, const BucketScanCall &c) {
    if (c.pq) {   // code rows: M bytes at a pitch of 16-byte units; row_stride is the decoded row's width and must say the same M
        const long long M = c.pq_dsub > 0 ? (c.d + c.pq_dsub - 1) / c.pq_dsub : 0;
        NLSH_REQUIRE(c.pq_pitch >= M && c.pq_pitch % 16 == 0, NLSH_E_INVALID, "%s: code_pitch=%lld must be >= M=%lld and a multiple of 16 bytes", who,
                     c.pq_pitch, M);
        NLSH_REQUIRE(c.row_stride == M * c.pq_dsub, NLSH_E_INVALID, "%s: row_stride=%lld is not M * dsub = %lld (the decoded row's width)", who,
                     c.row_stride, M * c.pq_dsub);
        NLSH_REQUIRE(((uintptr_t)c.corpus & 15) == 0, NLSH_E_INVALID, "%s: corpus_sorted must be 16-byte aligned", who);
        return NLSH_OK;
    }
    const int per16 = c.storage == NLSH_STORE_F32 ? 4 : (c.storage == NLSH_STORE_F16 ? 8 : 16);
    NLSH_REQUIRE(c.row_stride >= c.d && c.row_stride % per16 == 0, NLSH_E_INVALID, "%s: row_stride=%lld must be >= d=%d and a multiple of %d elements "
                 "(a pitch of 16-byte units) for storage=%d", who, c.row_stride, c.d, per16, c.storage);
    NLSH_REQUIRE(((uintptr_t)c.corpus & 15) == 0, NLSH_E_INVALID, "%s: corpus_sorted must be 16-byte aligned", who);
    return NLSH_OK;
}

int scan_call_check(const char *who, const BucketScanCall &c, unsigned needs) {
    const bool topk = (needs & SCAN_NEEDS_TOPK_OUT) != 0;
    int rc;
    const int phase_max = NLSH_PHASE_PLAN | NLSH_PHASE_SCAN | NLSH_PHASE_MERGE | ((needs & SCAN_ALLOWS_PLAN_REST) ? NLSH_PHASE_PLAN_REST : 0);
    const int both_plans = NLSH_PHASE_PLAN | NLSH_PHASE_PLAN_REST;
    NLSH_REQUIRE(c.storage >= NLSH_STORE_F32 && c.storage <= NLSH_STORE_U8, NLSH_E_INVALID, "%s: storage=%d is none of NLSH_STORE_F32 / F16 / U8", who, c.storage);
    NLSH_REQUIRE(c.phases >= 1 && c.phases <= phase_max && (c.phases & both_plans) != both_plans, NLSH_E_INVALID, "%s: phases=%d", who, c.phases);
    NLSH_REQUIRE(c.algo == NLSH_SCAN_QUERY_MAJOR || c.algo == NLSH_SCAN_BUCKET_MAJOR || c.tiled(), NLSH_E_INVALID, "%s: algo=%d", who, c.algo);
    NLSH_REQUIRE(!(c.phases & NLSH_PHASE_PLAN_REST) || c.algo != NLSH_SCAN_QUERY_MAJOR, NLSH_E_INVALID, "%s: the query-major schedule has no fused lookup", who);
    // what the tiled schedule alone can do
    const char *tiled_only = "the tiled schedule only (NLSH_SCAN_BUCKET_TILED)";
    NLSH_REQUIRE(topk || c.tiled(), NLSH_E_UNSUPPORTED, "%s: a radius query is scanned by %s, not by algo=%d", who, tiled_only, c.algo);
    NLSH_REQUIRE(!c.row_filter || c.tiled(), NLSH_E_UNSUPPORTED, "%s: row_filter is read by %s, not by algo=%d", who, tiled_only, c.algo);
    NLSH_REQUIRE(!(c.row_tags || c.query_masks) || c.tiled(), NLSH_E_UNSUPPORTED, "%s: row_tags and query_masks are read by %s, not by algo=%d", who, tiled_only, c.algo);
    NLSH_REQUIRE(!c.affine || c.tiled(), NLSH_E_UNSUPPORTED, "%s: an sq8 corpus is read by %s, not by algo=%d", who, tiled_only, c.algo);
    NLSH_REQUIRE(c.storage == NLSH_STORE_F32 || c.tiled(), NLSH_E_UNSUPPORTED, "%s: a %s corpus (storage=%d) is read by %s, not by algo=%d", who,
                 c.storage == NLSH_STORE_F16 ? "float16" : "uint8", c.storage, tiled_only, c.algo);
    NLSH_REQUIRE(!c.affine || c.storage == NLSH_STORE_U8, NLSH_E_INVALID, "%s: an sq8 corpus is held in the uint8 layout, not storage=%d", who, c.storage);
    // a product-quantised corpus: the tiled schedule's direct top-k calls alone, one of three sub-vector widths, no tags
    NLSH_REQUIRE(!c.pq || c.tiled(), NLSH_E_UNSUPPORTED, "%s: a pq corpus is read by %s, not by algo=%d", who, tiled_only, c.algo);
    NLSH_REQUIRE(!c.pq || (topk && !(needs & SCAN_ALLOWS_PLAN_REST) && !(c.phases & NLSH_PHASE_PLAN_REST)), NLSH_E_UNSUPPORTED,
                 "%s: a pq corpus is read by the direct top-k calls only, not by a radius call, a step or a graph slot", who);
    NLSH_REQUIRE(!c.pq || !(c.row_tags || c.query_masks), NLSH_E_UNSUPPORTED, "%s: a pq corpus takes no row_tags", who);
    NLSH_REQUIRE(!c.pq || (c.storage == NLSH_STORE_U8 && !c.affine), NLSH_E_INVALID, "%s: a pq corpus is code bytes, not storage=%d", who, c.storage);
    NLSH_REQUIRE(!c.pq || c.pq_dsub == 4 || c.pq_dsub == 8 || c.pq_dsub == 16, NLSH_E_INVALID, "%s: dsub=%d is none of 4, 8, 16", who, c.pq_dsub);
    NLSH_REQUIRE(!c.pq || (c.pq_codebook && ((uintptr_t)c.pq_codebook & 15) == 0), NLSH_E_INVALID, "%s: the codebook is null or not 16-byte aligned", who);
    NLSH_REQUIRE(((uintptr_t)c.row_filter & 3) == 0, NLSH_E_INVALID, "%s: row_filter must be 4-byte aligned", who);
    // per-query tag filters (the schedule is held above): both arrays or neither, read with 8-byte loads, by the top-k kernels of a direct call alone
    NLSH_REQUIRE(c.row_tags || !c.query_masks, NLSH_E_INVALID, "%s: query_masks without row_tags", who);
    NLSH_REQUIRE(!c.row_tags || c.query_masks, NLSH_E_INVALID, "%s: row_tags without query_masks", who);
    NLSH_REQUIRE(((uintptr_t)c.row_tags & 7) == 0, NLSH_E_INVALID, "%s: row_tags must be 8-byte aligned", who);
    NLSH_REQUIRE(((uintptr_t)c.query_masks & 7) == 0, NLSH_E_INVALID, "%s: query_masks must be 8-byte aligned", who);
    NLSH_REQUIRE(!c.row_tags || (c.tag_match >= NLSH_TAG_ANY && c.tag_match <= NLSH_TAG_EQ), NLSH_E_INVALID,
                 "%s: tag_match=%d is none of NLSH_TAG_ANY / ALL / EQ", who, c.tag_match);
    NLSH_REQUIRE(!c.row_tags || (topk && !(needs & SCAN_ALLOWS_PLAN_REST) && !(c.phases & NLSH_PHASE_PLAN_REST)), NLSH_E_UNSUPPORTED,
                 "%s: row_tags are read by the direct top-k calls only, not by a radius call, a step or a graph slot", who);
    // A compressed copy's pitch is held HERE for the top-k calls, ahead of the limits and of the empty batch, as the typed entry always
    // did; float32 rows and the radius calls have theirs held behind both, below: each entry keeps the code it had.
    const bool pitch_first = topk && c.storage != NLSH_STORE_F32;
    if (pitch_first && (rc = corpus_pitch_check(who, c)) != NLSH_OK) return rc;
    NLSH_REQUIRE(c.Q >= 0 && c.Q < (1ll << 31), NLSH_E_INVALID, "%s: Q=%lld", who, c.Q);
    NLSH_REQUIRE(c.d >= 1 && c.d <= NLSH_MAX_DIM, NLSH_E_UNSUPPORTED, "%s: d=%d not in [1,%d]", who, c.d, NLSH_MAX_DIM);
    // one key per lane is built into the running top-k of the query-major and the wave-level bucket-major schedules; the tiled schedule
    // selects a list from the 64 * TPS = 256 candidates a wave holds
    NLSH_REQUIRE(c.k >= 1 && c.k <= (c.tiled() ? NLSH_MAX_K_TILED : NLSH_MAX_K), NLSH_E_UNSUPPORTED,
                 "%s: k=%d not supported by algo=%d: every schedule takes k in [1,%d], only the tiled schedule (NLSH_SCAN_BUCKET_TILED, "
                 "algo=\"tiled\" in the Python facade) takes k in [1,%d]", who, c.k, c.algo, NLSH_MAX_K, NLSH_MAX_K_TILED);
    NLSH_REQUIRE(c.P >= 1 && c.P <= NLSH_MAX_PROBES, NLSH_E_UNSUPPORTED, "%s: P=%d not in [1,%d]", who, c.P, NLSH_MAX_PROBES);
    NLSH_REQUIRE(c.metric >= NLSH_METRIC_L2_EPS && c.metric <= NLSH_METRIC_L2_EPS_FOLDED, NLSH_E_INVALID, "%s: metric=%d", who, c.metric);
    NLSH_REQUIRE(c.nb >= 0 && c.max_tasks >= 0 && c.seg >= 0, NLSH_E_INVALID, "%s: negative size (n_buckets=%d, max_tasks=%lld, seg_rows=%d)", who, c.nb, c.max_tasks, c.seg);
    NLSH_REQUIRE(c.n_cells >= 0 && c.n_cells <= c.nb && (c.n_cells == 0 || (c.cell_of && c.cell_offsets)), NLSH_E_INVALID,
                 "%s: n_cells=%d needs cell_of and cell_offsets and cannot exceed n_buckets=%d", who, c.n_cells, c.nb);
    if (c.Q == 0) return NLSH_OK;
    NLSH_REQUIRE(c.queries && c.qkeys && c.nkeys && c.status && c.workspace, NLSH_E_INVALID, "%s: null pointer (queries, qkeys, nkeys, status or workspace)", who);
    NLSH_REQUIRE(!topk || (c.out_dist && c.out_idx && c.out_ncand), NLSH_E_INVALID, "%s: null pointer (out_dist, out_idx or out_ncand)", who);
    NLSH_REQUIRE(c.nb == 0 || (c.corpus && c.gid && c.uniq && c.offsets), NLSH_E_INVALID, "%s: null index pointer", who);
    NLSH_REQUIRE(c.metric != NLSH_METRIC_COSINE || c.nb == 0 || c.inv_norm, NLSH_E_INVALID, "%s: cosine needs inv_norm", who);
    // the quantiser of an sq8 corpus: two arrays of row_stride floats, read as the float4 of a chunk column
    NLSH_REQUIRE(!c.affine || (c.quant_lo && c.quant_step), NLSH_E_INVALID, "%s: null pointer (lo or step)", who);
    NLSH_REQUIRE(!c.affine || ((((uintptr_t)c.quant_lo | (uintptr_t)c.quant_step) & 15) == 0), NLSH_E_INVALID, "%s: lo and step must be 16-byte aligned", who);
    if (!pitch_first && (rc = corpus_pitch_check(who, c)) != NLSH_OK) return rc;
    NLSH_REQUIRE(c.q_stride >= c.d, NLSH_E_INVALID, "%s: q_stride=%lld < d=%d", who, c.q_stride, c.d);
    // the task table and the partial lists are read with 16- and 8-byte accesses at 256-byte offsets of the workspace
    NLSH_REQUIRE(((uintptr_t)c.workspace & 15) == 0 && ((uintptr_t)c.out_keys & 7) == 0, NLSH_E_INVALID,
                 "%s: the workspace must be 16-byte aligned and out_keys 8-byte aligned", who);
    return NLSH_OK;
}

}  // namespace nlsh

using namespace nlsh;

extern "C" size_t nlsh_scan_workspace(int64_t Q, int P, int k, int64_t max_tasks, int64_t n_buckets, int d) {
    if (Q < 0 || P < 1 || k < 1 || max_tasks < 0 || n_buckets < 0 || d < 1) { set_error("scan_workspace: bad sizes"); return 0; }
    ScanWs w;
    scan_layout(Q, P, k, max_tasks, &w);
    const size_t b = bucket_scan_workspace(Q, P, k, max_tasks, n_buckets, d);
    return w.total > b ? w.total : b;
}

// The top-k entry points: fill, check, run.  The descriptor with what they all have, under the header's parameter names:
#define NLSH_TOPK_CALL(c)                                                                                                          \
    BucketScanCall c = {};                                                                                                         \
    NLSH_SCAN_CALL_COMMON(c);                                                                                                      \
    c.k = k; c.seg = seg_rows; c.out_dist = out_dist; c.out_idx = out_idx; c.out_keys = out_keys; c.out_ncand = out_ncand
static int topk_call(const char *who, const BucketScanCall &c) {
    const int rc = scan_call_check(who, c, SCAN_NEEDS_TOPK_OUT);
    if (rc != NLSH_OK || c.Q == 0) return rc;
    return scan_call_run(c);
}

extern "C" int nlsh_scan_topk(const float *corpus_sorted, int64_t row_stride, int d, const int32_t *gid,
                              const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                              const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q, const int32_t *qkeys,
                              const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows, float *out_dist,
                              int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand, int32_t *status, void *workspace,
                              size_t workspace_bytes, int64_t max_tasks, void *ev_scan_begin, void *ev_scan_end,
                              nlsh_stream_t stream) {
    NLSH_TOPK_CALL(c);
    c.phases = NLSH_PHASE_PLAN | NLSH_PHASE_SCAN | NLSH_PHASE_MERGE;
    return topk_call("scan_topk", c);
}

extern "C" int nlsh_scan_topk_phase(const float *corpus_sorted, int64_t row_stride, int d, const int32_t *gid,
                              const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                              const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q, const int32_t *qkeys, const int32_t *nkeys,
                              int P, int k, int metric, int algo, int seg_rows, float *out_dist, int32_t *out_idx,
                              uint64_t *out_keys, int32_t *out_ncand, int32_t *status, void *workspace, size_t workspace_bytes,
                              int64_t max_tasks, void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases) {
    NLSH_TOPK_CALL(c);
    c.phases = phases;
    return topk_call("scan_topk_phase", c);
}

// The six entries with cells fill their descriptor in two places, one per family: the narrower entries of a family are its widest one
// without the trailing arguments, under a name of their own in the refusals (`who`).
#define NLSH_CELLS_PARAMS                                                                                                          \
    int64_t row_stride, int d, const int32_t *gid, const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order,   \
    int32_t n_buckets, const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells, const float *inv_norm,                 \
    const float *queries, int64_t q_stride, int64_t Q, const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric,        \
    int algo, int seg_rows, float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand, int32_t *status,             \
    void *workspace, size_t workspace_bytes, int64_t max_tasks, void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream,       \
    int phases
#define NLSH_CELLS_ARGS                                                                                                            \
    row_stride, d, gid, uniq_keys, offsets, bucket_order, n_buckets, cell_of, cell_offsets, n_cells, inv_norm, queries, q_stride, Q, \
    qkeys, nkeys, P, k, metric, algo, seg_rows, out_dist, out_idx, out_keys, out_ncand, status, workspace, workspace_bytes,         \
    max_tasks, ev_scan_begin, ev_scan_end, stream, phases
// the cells / typed / filtered / tagged family
static int cells_topk_call(const char *who, const void *corpus_sorted, int storage, NLSH_CELLS_PARAMS, const uint32_t *row_filter,
                           const uint64_t *row_tags, const uint64_t *query_masks, int tag_match) {
    NLSH_TOPK_CALL(c);
    c.cell_of = cell_of; c.cell_offsets = cell_offsets; c.n_cells = n_cells;
    c.phases = phases; c.storage = storage; c.row_filter = row_filter;
    c.row_tags = row_tags; c.query_masks = query_masks; c.tag_match = tag_match;
    return topk_call(who, c);
}
// the sq8 / sq8_tagged family: uint8 layout, the quantiser beside it
static int sq8_topk_call(const char *who, const uint8_t *corpus_sorted, const float *lo, const float *step, NLSH_CELLS_PARAMS,
                         const uint32_t *row_filter, const uint64_t *row_tags, const uint64_t *query_masks, int tag_match) {
    NLSH_TOPK_CALL(c);
    c.cell_of = cell_of; c.cell_offsets = cell_offsets; c.n_cells = n_cells;
    c.phases = phases; c.storage = NLSH_STORE_U8; c.row_filter = row_filter;
    c.affine = true; c.quant_lo = lo; c.quant_step = step;
    c.row_tags = row_tags; c.query_masks = query_masks; c.tag_match = tag_match;
    return topk_call(who, c);
}

extern "C" int nlsh_scan_topk_cells_phase(const float *corpus_sorted, NLSH_CELLS_PARAMS) {
    return cells_topk_call("scan_topk_cells_phase", corpus_sorted, NLSH_STORE_F32, NLSH_CELLS_ARGS, nullptr, nullptr, nullptr, 0);
}

extern "C" int nlsh_scan_topk_cells_phase_typed(const void *corpus_sorted, int storage, NLSH_CELLS_PARAMS) {
    return cells_topk_call("scan_topk_typed", corpus_sorted, storage, NLSH_CELLS_ARGS, nullptr, nullptr, nullptr, 0);
}

extern "C" int nlsh_scan_topk_cells_phase_filtered(const void *corpus_sorted, int storage, NLSH_CELLS_PARAMS, const uint32_t *row_filter) {
    // without a filter this IS the typed call (include/nlsh_hip.h), and says so in its refusals
    return cells_topk_call(row_filter ? "scan_topk_filtered" : "scan_topk_typed", corpus_sorted, storage, NLSH_CELLS_ARGS, row_filter, nullptr, nullptr, 0);
}

// The filtered call over an sq8 corpus: uint8 layout, the quantiser behind the filter.  Not a fourth storage code of the typed calls
// (they answer NLSH_E_INVALID to anything past NLSH_STORE_U8): an entry of its own.
extern "C" int nlsh_scan_topk_cells_phase_sq8(const uint8_t *corpus_sorted, const float *lo, const float *step, NLSH_CELLS_PARAMS,
                                              const uint32_t *row_filter) {
    return sq8_topk_call("scan_topk_sq8", corpus_sorted, lo, step, NLSH_CELLS_ARGS, row_filter, nullptr, nullptr, 0);
}

// The filtered call over a product-quantised corpus: code rows, the codebook, dsub and the code pitch where the sq8 call has lo / step.
// row_stride is the decoded row's width, M * dsub.
extern "C" int nlsh_scan_topk_cells_phase_pq(const uint8_t *corpus_sorted, const float *codebook, int dsub, int64_t code_pitch, NLSH_CELLS_PARAMS,
                                             const uint32_t *row_filter) {
    NLSH_TOPK_CALL(c);
    c.cell_of = cell_of; c.cell_offsets = cell_offsets; c.n_cells = n_cells;
    c.phases = phases; c.storage = NLSH_STORE_U8; c.row_filter = row_filter;
    c.pq = true; c.pq_codebook = codebook; c.pq_dsub = dsub; c.pq_pitch = code_pitch;
    return topk_call("scan_topk_pq", c);
}

// The filtered call behind per-query tag filters: without row_tags it IS the filtered call, and says so in its refusals.
extern "C" int nlsh_scan_topk_cells_phase_tagged(const void *corpus_sorted, int storage, NLSH_CELLS_PARAMS, const uint32_t *row_filter,
                                                 const uint64_t *row_tags, const uint64_t *query_masks, int tag_match) {
    return cells_topk_call((row_tags || query_masks) ? "scan_topk_tagged" : (row_filter ? "scan_topk_filtered" : "scan_topk_typed"), corpus_sorted,
                           storage, NLSH_CELLS_ARGS, row_filter, row_tags, query_masks, tag_match);
}

extern "C" int nlsh_scan_topk_cells_phase_sq8_tagged(const uint8_t *corpus_sorted, const float *lo, const float *step, NLSH_CELLS_PARAMS,
                                                     const uint32_t *row_filter, const uint64_t *row_tags, const uint64_t *query_masks,
                                                     int tag_match) {
    return sq8_topk_call((row_tags || query_masks) ? "scan_topk_sq8_tagged" : "scan_topk_sq8", corpus_sorted, lo, step, NLSH_CELLS_ARGS, row_filter,
                         row_tags, query_masks, tag_match);
}
#undef NLSH_CELLS_PARAMS
#undef NLSH_CELLS_ARGS

extern "C" int nlsh_merge_topk(const uint64_t *keys_in, int64_t row_stride, int G, int64_t Q, int k, const int32_t *ncand_in,
                               float *out_dist, int32_t *out_idx, int32_t *out_ncand, nlsh_stream_t stream) {
    NLSH_REQUIRE(G >= 1 && Q >= 0 && k >= 1 && k <= NLSH_MAX_K_TILED && row_stride >= k, NLSH_E_INVALID,
                 "merge_topk: G=%d Q=%lld k=%d (at most %d) row_stride=%lld", G, (long long)Q, k, NLSH_MAX_K_TILED, (long long)row_stride);
    if (Q == 0) return NLSH_OK;
    NLSH_REQUIRE(keys_in && out_dist && out_idx, NLSH_E_INVALID, "merge_topk: null pointer");
    const dim3 grid((unsigned)((Q + 3) / 4));
    const void *fn = (const void *)merge_shards_kernel;
    if (k > 192) fn = (const void *)merge_shards_wide_kernel<4>;
    else if (k > 128) fn = (const void *)merge_shards_wide_kernel<3>;
    else if (k > NLSH_MAX_K) fn = (const void *)merge_shards_wide_kernel<2>;
    long long rs = row_stride, q64 = Q;
    void *argv[] = {&keys_in, &rs, &G, &q64, &k, &ncand_in, &out_dist, &out_idx, &out_ncand};
    NLSH_CHECK_HIP(hipLaunchKernel(fn, grid, dim3(256), argv, 0, (hipStream_t)stream));
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
