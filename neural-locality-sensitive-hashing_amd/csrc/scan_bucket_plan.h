// Bucket-major scan, PLAN phase (part of the translation unit scan_bucket.hip, which defines BArgs in front of this file): the lookup of
// caller-supplied keys (bplan_kernel), the task layout (bscan_kernel: block scan + decoupled look-back) and the scatter of the pairs
// into their cells' query lists and their tasks' slot records (bscatter_kernel).
#pragma once

namespace nlsh {

// Bucket lookup of every (query, probe) of a CALLER-SUPPLIED key table (keys from encode_hash are looked up in its own epilogue):
// scan_plan.h.  The coarse table (every `stride`-th key, <= 1024 entries) is loaded once per workgroup.
// Workgroups past `plan_blocks` prepare the tiled schedule's query copy instead (prep_metric >= 0), four queries each.
__global__ __launch_bounds__(256) void bplan_kernel(PlanArgs a, unsigned plan_blocks) {
    __shared__ int32_t coarse[1024];
    __shared__ int whits[4], wviol[4];
    if (blockIdx.x >= plan_blocks) {   // uniform per workgroup: no barrier below is reached by these
        const long long q = (long long)(blockIdx.x - plan_blocks) * 4 + (threadIdx.x >> 6);
        if (q < a.Q) prep_query(a, q, threadIdx.x & 63);
        return;
    }
    for (int i = threadIdx.x; i < a.nco; i += 256) coarse[i] = a.uniq[(long long)i * a.stride];
    if (blockIdx.x == 0) plan_batch_init(a, threadIdx.x, 256);   // per-batch initialisation rides along (no separate launch)
    __syncthreads();
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    int viol = 0;
    if (idx < a.Q * a.P) {
        const long long q = idx / a.P;
        const int p = (int)(idx - q * a.P);
        if (p == 0) a.tauq[q] = KEY_NONE;        // running bound of the query
        int nk = a.qnkeys[q];
        nk = nk < 0 ? 0 : (nk > a.P ? a.P : nk);
        int32_t key = 0;
        bool live = p < nk;
        if (live) {
            key = a.qkeys[idx];
            // a query's keys are a SET (nlsh/utils.pyx:27-31): a repeated key probes its bucket once.  encode_hash never
            // emits one; a C caller's table might, and the selection-based merges assume distinct (distance, id) keys.
            for (int pp = 0; pp < p; ++pp) live &= a.qkeys[idx - p + pp] != key;
        }
        hit = plan_pair(a, coarse, idx, key, live, viol);
    }
    // pairs this block added to the counters: bscan_kernel holds the counters' sum against the sum of these, which is how
    // a workspace head that was not zero on entry (workspace contract, nlsh_hip.h) is caught instead of trusted
    const unsigned long long m = __ballot(hit);
    const unsigned long long v1 = __ballot(viol & PLAN_VIOL_COUNTER), v2 = __ballot(viol & PLAN_VIOL_CELLS);
    if ((threadIdx.x & 63) == 0) {
        whits[threadIdx.x >> 6] = __popcll(m);
        wviol[threadIdx.x >> 6] = (v1 ? PLAN_VIOL_COUNTER : 0) | (v2 ? PLAN_VIOL_CELLS : 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) a.hits[blockIdx.x] = (whits[0] + whits[1] + whits[2] + whits[3]) | wviol[0] | wviol[1] | wviol[2] | wviol[3];
}

// exclusive scan of a 64-bit value over the 256 threads of a block (two packed 32-bit sums scanned together: the low word must not
// carry into the high one, which the callers' ranges guarantee: low = pairs <= Q * P < 2^31)
__device__ __forceinline__ unsigned long long block_excl_scan64(unsigned long long v, unsigned long long *wsum, unsigned long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned lo = __shfl_up((unsigned)incl, m), hi = __shfl_up((unsigned)(incl >> 32), m);
        if (lane >= m) incl += ((unsigned long long)hi << 32) | lo;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned long long woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return woff + incl - v;
}

// Tasks are numbered in SCHEDULE order: cell `border[i]` (cells by descending size, fixed at index build)
// is handled by thread i, so the heavy (segment x query-group) tasks of the big buckets get the low ids and are
// dispatched first, the single small tasks of the small buckets last: the kernel no longer ends on a tail of
// 40-us tasks started in its last microseconds (measured: machine full until 370 us, drained until 440 us).
// Numbering is deterministic (no dependence on block timing): block j publishes its totals, block i sums the
// totals of the blocks before it.
//
// r06: ONE launch (r02-r05: bcount_kernel left the per-block totals, a second launch summed them: a dependent launch costs ~4.5 us
// on this part whatever it does).  Decoupled look-back without the chain: a block publishes its OWN totals -- they depend on nothing
// but its own 256 counters -- as one 64-bit word {tasks : 32 | pairs : 30 | negative counter seen : 1 | ready : 1} with a
// device-scope store, then thread t waits for the words of blocks t, t + 256, ... < blockIdx.x and the block adds them up.  Blocks
// are dispatched in index order and a block only ever waits for LOWER indices, which wait for nothing unfinished: the lowest
// unfinished block always runs, so the wait cannot deadlock whatever the grid size.  The slots are zeroed by the plan launch in
// front of this one (plan_batch_init).  Device-scope (sc1) accesses to the slots only: no fence, no L2 write-back (r02 measured an
// in-kernel grid barrier with agent-scope fences at 127 us -- each writes back an XCD's L2).
//
// The pair counters are READ AND RESET here (thread per cell): the slot of every pair was fixed when the lookup incremented the
// counter (scan_plan.h), so nobody needs the counts after this kernel, and the head of the workspace is zero again for the next
// batch (workspace contract) without the scatter step's atomicSub of r01-r05.
//
// status[1] = 2: the pair counters were not zero when the batch's lookup started (an uninitialised buffer, one lent to another
// schedule).  The LAST block knows every total: the counters must sum to the pairs the lookup counted this batch, none may be
// negative and no pair may have drawn a negative slot.  On a violation status[0] = 0 -- the scan launches no task -- and bscatter,
// which starts after this kernel, drops every pair: nothing is ever addressed through a stale count (negative counts are clamped
// to zero before they enter a prefix; descriptors are written inside the table only; the pair lists are only written by bscatter).
// The facade turns the flag into NLSH_E_WORKSPACE.  status[1] = 3: the lookup refused a pair of a foreign cell layout (scan_plan.h).
constexpr unsigned long long LB_READY = 1ull, LB_NEG = 2ull;
__device__ __forceinline__ void lookback_publish(unsigned long long *slot, unsigned long long v) {
    __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long lookback_wait(unsigned long long *slot) {
    unsigned long long v;
    do { v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (!(v & LB_READY));
    return v;
}

__global__ __launch_bounds__(256) void bscan_kernel(BArgs a, int plan_blocks) {
    __shared__ unsigned long long wsum[4];
    __shared__ unsigned long long base_s;
    __shared__ int neg_s, flags_s;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) { neg_s = 0; flags_s = 0; }
    const bool last_block = blockIdx.x == gridDim.x - 1;
    // the last block's verdict needs the lookup's per-block pair counts: requested NOW, with the first loads of the kernel, not behind the
    // look-back (the last block ends the kernel: a round trip on its path is a round trip of the launch)
    int hsum = 0, hflags = 0;
    if (last_block)
        for (int j = threadIdx.x; j < plan_blocks; j += 256) {
            const int h = a.hits[j];
            hsum += h & PLAN_HITS_MASK;
            hflags |= h & ~PLAN_HITS_MASK;
        }
    int b = 0, m = 0, s = 0, ns = 0, ng = 0;
    bool neg = false;
    if (i < a.nc) {
        b = a.border ? a.border[i] : i;   // a CELL (a bucket when the index has no cells)
        m = a.bcount[b];
        if (m != 0) a.bcount[b] = 0;      // handed back: zero again for the next batch
        neg = m < 0;
        m = neg ? 0 : m;                  // a stale negative count enters no prefix (the batch is refused below)
        s = a.coffsets[b + 1] - a.coffsets[b];
        ns = (s + a.seg - 1) / a.seg;
        ng = (m + a.QB - 1) / a.QB;
    }
    const int nt = ng * ns;
    unsigned long long tot;
    const unsigned long long ex = block_excl_scan64(((unsigned long long)(unsigned)nt << 32) | (unsigned)m, wsum, &tot);   // (barriers inside: neg_s is initialised)
    if (neg) neg_s = 1;
    __syncthreads();
    if (threadIdx.x == 0)
        lookback_publish(a.lookback + blockIdx.x, (tot & 0xFFFFFFFF00000000ull) | ((tot & 0x3FFFFFFFull) << 2) | (neg_s ? LB_NEG : 0ull) | LB_READY);
    // totals of the blocks before this one
    unsigned long long prev = 0;
    int pneg = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) {
        const unsigned long long v = lookback_wait(a.lookback + j);
        prev += (v & 0xFFFFFFFF00000000ull) | ((v >> 2) & 0x3FFFFFFFull);
        pneg |= (v & LB_NEG) ? 1 : 0;
    }
    {
        unsigned long long ptot;
        block_excl_scan64(prev, wsum, &ptot);
        if (threadIdx.x == 0) base_s = ptot;
        if (pneg) neg_s = 1;
    }
    if (last_block) {   // the verdict: every total is known here
        unsigned long long htot;
        __syncthreads();
        block_excl_scan64((unsigned long long)(unsigned)hsum, wsum, &htot);
        if (hflags) atomicOr(&flags_s, hflags);
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long all = base_s + tot;
            const bool bad = (all & 0xFFFFFFFFull) != htot || neg_s != 0 || (flags_s & PLAN_VIOL_COUNTER);
            a.status[0] = bad ? 0 : (int)(all >> 32);   // tasks needed (may exceed max_tasks: the caller retries)
            a.status[1] = bad ? 2 : ((flags_s & PLAN_VIOL_CELLS) ? 3 : 0);
        }
    }
    __syncthreads();
    // A cell's descriptors are written by its own thread (writing a block's tasks with all its threads, one task per thread and
    // round, measured 15.6 us against 9.5 us on the SIFT1M-shaped batch) -- unless it has more than HEAVY of them: a 180 k-row
    // bucket probed by thousands of queries (Deep100M-shaped: 707 segments x hundreds of query groups) is 10^5 descriptors, and one
    // thread writing them made this kernel 1.0 ms of a 37-ms step (r03).  Heavy cells are queued in LDS and written by the whole block.
    constexpr int HEAVY = 256, HEAVY_SLOTS = 256;
    __shared__ int heavy_n;
    __shared__ int heavy_b[HEAVY_SLOTS][6];   // po, to, ng, nt, m, cell (row0 and size are re-read)
    if (threadIdx.x == 0) heavy_n = 0;
    __syncthreads();
    if (i < a.nc) {
        const unsigned long long off = base_s + ex;
        const int po = (int)(off & 0xFFFFFFFFull), to = (int)(off >> 32);
        a.cellrec[b] = make_int4(po, to, ng, 0);
        if (nt > HEAVY) {
            const int slot = atomicAdd(&heavy_n, 1);   // <= 256 threads, so a slot always exists
            heavy_b[slot][0] = po; heavy_b[slot][1] = to; heavy_b[slot][2] = ng; heavy_b[slot][3] = nt; heavy_b[slot][4] = m; heavy_b[slot][5] = b;
        } else {
            const int row0 = a.coffsets[b];
            for (int t = 0; t < nt; ++t) {
                const long long tt = (long long)to + t;
                if (tt >= a.max_tasks) break;
                // segment-major: the query groups of one row segment get consecutive task ids, so they run
                // at about the same time (and, with the chunked XCD map of bscan3, on one XCD's L2)
                const int si = t / ng, gi = t - si * ng;
                a.task[tt] = make_int4(po + gi * a.QB, min(a.QB, m - gi * a.QB), row0 + si * a.seg, min(a.seg, s - si * a.seg));
            }
        }
    }
    __syncthreads();
    for (int h = 0; h < heavy_n; ++h) {
        const int po = heavy_b[h][0], to = heavy_b[h][1], hng = heavy_b[h][2], hnt = heavy_b[h][3], hm = heavy_b[h][4], hb = heavy_b[h][5];
        const int row0 = a.coffsets[hb], hs = a.coffsets[hb + 1] - row0;
        for (int t = threadIdx.x; t < hnt; t += 256) {
            const long long tt = (long long)to + t;
            if (tt >= a.max_tasks) break;
            const int si = t / hng, gi = t - si * hng;
            a.task[tt] = make_int4(po + gi * a.QB, min(a.QB, hm - gi * a.QB), row0 + si * a.seg, min(a.seg, hs - si * a.seg));
        }
    }
}

// Every counted pair into its cell's query list and its tasks' slot records.  r06: no atomics and one dependent load level -- the
// lookup left {cell, slot, bucket rows, first row inside the cell} per pair (scan_plan.h) and bscan one {first pair, first task,
// query groups} record per cell (r01-r05: atomicSub on the cell's counter for the slot, then five loads behind it).
__global__ __launch_bounds__(256) void bscatter_kernel(BArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.Q * a.P) return;
    const int4 pp = a.ppair[idx];
    if (pp.x < 0 || a.status[1] == 2) {   // no bucket, or a poisoned workspace (bscan_kernel): nothing is addressed through the counters
        a.prec[idx] = make_int4(0, 0, 0, 0);
        return;
    }
    const int rel = pp.y, size = pp.z, lo0 = pp.w;   // slot in the cell's pair list; rows of the BUCKET; its first row inside the cell (0 for a bucket that is its own cell)
    const int4 cr = a.cellrec[pp.x];
    a.inv_q[cr.x + rel] = (int32_t)(idx / a.P);
    // what bmerge needs to find this probe's partial lists, resolved here so that it has one load level less:
    // task of (segment si, group gi) = first task of the cell + si * ngroups + gi
    const int gi = rel / a.QB;
    // `size` = rows of the BUCKET: the query's candidate count, and (size + seg - 1) / seg = its partial lists -- one per row segment of
    // a big bucket, exactly one for a bucket inside a shared window (window_rows <= seg; the lookup refuses cells that break this)
    const int t0 = cr.y + gi, ng = cr.z;
    a.prec[idx] = make_int4(t0, rel - gi * a.QB, size, ng);
    if (a.task_qr) {
        // the tiled scan reads a task's query ids from the task's own record (address known from the task id alone: the
        // ids arrive with the descriptor instead of one dependent round trip later); one copy per row segment
        const int ns = (size + a.seg - 1) / a.seg;
        for (int si = 0; si < ns; ++si) {
            const long long tt = (long long)t0 + (long long)si * ng;
            if (tt >= a.max_tasks) break;
            const int lo = max(lo0 - si * a.seg, 0), hi = min(lo0 + size - si * a.seg, a.seg);   // the bucket's rows inside segment si
            a.task_qr[tt * a.QB + (rel - gi * a.QB)] = make_int2((int32_t)(idx / a.P), lo | (hi << 16));
        }
    }
}

}  // namespace nlsh
