// Bucket-major scan, MERGE phase (part of the translation unit scan_bucket.hip, which defines BArgs in front of this file): one
// wavefront merges the partial lists of a query's (probe, segment) pairs into its final top-k; bmerge_kernel for k <= 64,
// bmergew_kernel<KPL> for k up to NLSH_MAX_K_TILED.  bmerge_host_kernel is bmerge_kernel for a caller that wants the results on the
// HOST (nlsh_query_batch_host): same merge, the ids / counts / status words / key rows of the short queries stored into one
// host-visible block instead of the device outputs.
#pragma once

namespace nlsh {

// Merge of ONE query's partial lists into its final top-k (one wavefront; `sc` = 64 u64 of LDS scratch owned by the wave).
// HOST: nothing is stored to the device outputs -- the ordered ids go to `stage_ids` (k words of LDS, the workgroup stores its queries' rows
// as one run) and the candidate count is returned.
template <bool HOST = false>
__device__ __forceinline__ int merge_query(const BArgs &a, long long q, int lane, uint64_t *sc, int2 *ltab, int32_t *stage_ids = nullptr) {
    // lane p holds probe p's record (written by bscatter): where its partial lists are.  bscatter writes a record for EVERY slot of
    // the [Q, P] table -- zeros for slots past the query's key count, for repeated keys and for keys without a bucket -- so the key
    // count is not needed here (r04: its load sat in front of the record load, one dependent round trip per wave)
    int ns_l = 0, j_l = 0, ng_l = 0;
    long long t0_l = 0;
    int size_l = 0;
    if (lane < a.P) {
        const int4 rec = a.prec[q * a.P + lane];
        t0_l = rec.x; j_l = rec.y; size_l = rec.z; ng_l = rec.w;
        ns_l = (size_l + a.seg - 1) / a.seg;
    }
    // n_candidates of the query (indexer.py:71,94) = rows of its probed buckets
    const int c = __builtin_amdgcn_readlane(wave_incl_scan_i32(size_l), 63);
    if (!HOST && lane == 0) a.out_ncand[q] = c;
    // The query's partial lists (one per probe and row segment) are numbered 0..L-1 by an inclusive scan of the
    // per-probe segment counts.  A round fetches 3 x R lists (R = 64/k per load instruction: lane -> (list, entry)) and
    // SELECTS the k best of them and the best so far (merge_round); typical queries (<= 18 lists at k = 10) take one round.
    const int incl = wave_incl_scan_i32(ns_l);
    const int L = __builtin_amdgcn_readlane(incl, 63);
    const int R = 64 / a.k;
    const int r = lane / a.k, e = lane - r * a.k;
    // r06: where list `li` lives -- (task, slot) -- comes from a table in LDS that lane p fills for its probe's ns_l lists (task of
    // segment si = first task + si * query groups), instead of a 6-step shuffle search + 6 more shuffles per fetched list: the merge is
    // bound by its instruction count (10^4 waves x ~10 per SIMD), and a typical query has 5-18 lists of 1-2 segments per probe.  Queries
    // with a probe of more than LIST_TAB_MAX_SEG segments (a giant bucket) or more than LIST_TAB lists keep the search.
    constexpr int LIST_TAB = 128, LIST_TAB_MAX_SEG = 8;
    const bool tabbed = ltab != nullptr && L <= LIST_TAB && (int)wave_minmax_u32<true>((uint32_t)ns_l) <= LIST_TAB_MAX_SEG;   // wave-uniform
    if (tabbed) {
        const int first = incl - ns_l;
        for (int si = 0; si < LIST_TAB_MAX_SEG; ++si)
            if (si < ns_l) ltab[first + si] = make_int2((int)(t0_l + (long long)si * ng_l), j_l);
    }
    // keys of list slot `li` (one list per group of k lanes): which probe it belongs to, which segment of that probe's bucket
    auto fetch = [&](int li) -> uint64_t {
        long long t;
        int j;
        if (tabbed) {
            const int2 ent = ltab[(r < R && li < L) ? li : 0];   // same wave wrote it: LDS operations of a wave complete in order
            t = ent.x; j = ent.y;
        } else {
            int lo = 0, hi = 63;  // probe of list li = first lane whose inclusive count exceeds li
#pragma unroll
            for (int step = 0; step < 6; ++step) {
                const int mid = (lo + hi) >> 1;
                if (__shfl(incl, mid) > li) hi = mid; else lo = mid + 1;
            }
            const int p = lo > 63 ? 63 : lo;
            const int si = li - (__shfl(incl, p) - __shfl(ns_l, p));
            t = (long long)(((unsigned long long)(unsigned)__shfl((int)(t0_l >> 32), p) << 32) | (unsigned)__shfl((int)t0_l, p)) + (long long)si * __shfl(ng_l, p);
            j = __shfl(j_l, p);
        }
        // t >= max_tasks: table overflow, status[1] was set by the scan kernel and the caller repeats the call
        const bool live = r < R && li < L && t < a.max_tasks;
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(a.partial) + ((live ? t : 0) * a.QB + j) * a.k + e;
        return live ? (uint64_t)*src : KEY_NONE;
    };
    uint64_t carry = KEY_NONE;
    if (L <= R) {
        // r06: a query with at most R lists (GloVe-shaped: 6.5 probed buckets of a few rows each) selects from ONE key per lane -- a
        // quarter of the ballots per bisection step of the general round and one list lookup instead of three; <= 2R lists: two
        uint64_t key[1] = {fetch(r)};
        carry = merge_round<1>(key, a.k, lane, sc);
    } else if (L <= 2 * R) {
        uint64_t key[2] = {fetch(r), fetch(R + r)};
        carry = merge_round<2>(key, a.k, lane, sc);
    } else {
        for (int base = 0; base < L; base += 3 * R) {
            uint64_t key[4];
            key[0] = carry;
#pragma unroll
            for (int s = 0; s < 3; ++s) key[s + 1] = fetch(base + s * R + r);
            carry = merge_round<4>(key, a.k, lane, sc);
        }
    }
    if (HOST) merge_finish_ids(carry, a.k, lane, stage_ids);
    else merge_finish(carry, a.k, lane, a.out_dist, a.out_idx, a.out_keys, q);
    return c;
}

// merge_query for k in 65..NLSH_MAX_K_TILED (the tiled schedule only): the same records, the same list table and the same search for
// queries that leave it; a list is k keys fetched KPL = ceil(k / 64) per lane (entry e in register e / 64 of lane e % 64) instead of 64 / k
// lists per load, and a round takes NL lists beside the carry (merge_round_wide: (1 + NL) * KPL <= 8 keys per lane).  `sc` = NLSH_MAX_K_TILED
// u64 of LDS scratch owned by the wave.
template <int KPL>
__device__ __forceinline__ void merge_query_wide(const BArgs &a, long long q, int lane, uint64_t *sc, int2 *ltab) {
    int ns_l = 0, j_l = 0, ng_l = 0;
    long long t0_l = 0;
    int size_l = 0;
    if (lane < a.P) {
        const int4 rec = a.prec[q * a.P + lane];
        t0_l = rec.x; j_l = rec.y; size_l = rec.z; ng_l = rec.w;
        ns_l = (size_l + a.seg - 1) / a.seg;
    }
    {
        const int c = __builtin_amdgcn_readlane(wave_incl_scan_i32(size_l), 63);
        if (lane == 0) a.out_ncand[q] = c;
    }
    const int incl = wave_incl_scan_i32(ns_l);
    const int L = __builtin_amdgcn_readlane(incl, 63);
    constexpr int LIST_TAB = 128, LIST_TAB_MAX_SEG = 8;
    const bool tabbed = L <= LIST_TAB && (int)wave_minmax_u32<true>((uint32_t)ns_l) <= LIST_TAB_MAX_SEG;   // wave-uniform
    if (tabbed) {
        const int first = incl - ns_l;
        for (int si = 0; si < LIST_TAB_MAX_SEG; ++si)
            if (si < ns_l) ltab[first + si] = make_int2((int)(t0_l + (long long)si * ng_l), j_l);
    }
    // the KPL registers of list `li` (wave-uniform; li >= L: absent)
    auto fetch = [&](int li, uint64_t *dst) {
        long long t;
        int j;
        if (tabbed) {
            const int2 ent = ltab[li < L ? li : 0];   // same wave wrote it: LDS operations of a wave complete in order
            t = ent.x; j = ent.y;
        } else {
            int lo = 0, hi = 63;  // probe of list li = first lane whose inclusive count exceeds li
#pragma unroll
            for (int step = 0; step < 6; ++step) {
                const int mid = (lo + hi) >> 1;
                if (__shfl(incl, mid) > li) hi = mid; else lo = mid + 1;
            }
            const int p = lo > 63 ? 63 : lo;
            const int si = li - (__shfl(incl, p) - __shfl(ns_l, p));
            t = (long long)(((unsigned long long)(unsigned)__shfl((int)(t0_l >> 32), p) << 32) | (unsigned)__shfl((int)t0_l, p)) + (long long)si * __shfl(ng_l, p);
            j = __shfl(j_l, p);
        }
        // t >= max_tasks: table overflow, status[1] was set by the scan kernel and the caller repeats the call
        const bool live = li < L && t < a.max_tasks;
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(a.partial) + ((live ? t : 0) * a.QB + j) * a.k;
#pragma unroll
        for (int i = 0; i < KPL; ++i) dst[i] = (live && i * 64 + lane < a.k) ? (uint64_t)src[i * 64 + lane] : KEY_NONE;
    };
    constexpr int NL = KPL == 2 ? 3 : 1;
    uint64_t carry[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) carry[i] = KEY_NONE;
    for (int base = 0; base < L; base += NL) {
        uint64_t key[KPL * (1 + NL)];
#pragma unroll
        for (int i = 0; i < KPL; ++i) key[i] = carry[i];
#pragma unroll
        for (int s = 0; s < NL; ++s) fetch(base + s, key + KPL * (1 + s));
        merge_round_wide(key, carry, a.k, lane, sc);
    }
    merge_finish_wide(carry, sc, a.k, lane, a.out_dist, a.out_idx, a.out_keys, q);
}

// (r01-r05 re-checked here that every pair counter was back at zero; since r06 bscan_kernel resets the counters itself and its
// verdict covers every way a stale count can enter a batch -- positive ones through the sum, negative ones directly.)
__global__ __launch_bounds__(256) void bmerge_kernel(BArgs a) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    __shared__ uint64_t scratch[4][64];
    __shared__ int2 list_tab[4][128];    // merge_query's LIST_TAB entries per wave
    if (q < a.Q) merge_query(a, q, lane, scratch[threadIdx.x >> 6], list_tab[threadIdx.x >> 6]);
}

// The merge of nlsh_query_batch_host (k <= 64): `host` is a host-visible block of int32 words,
//     ids [Q * k] | counts [Q] | status [2] | key rows of the short queries [Q * (P + 1)]
// A workgroup's four queries are consecutive, so their id rows are ONE contiguous run of 4 * k words (160 bytes at k = 10) and their counts
// one of 4: the waves leave the ordered ids and the count in LDS and the workgroup stores each run with consecutive lanes, 16 bytes per
// lane where the run starts on a 16-byte boundary and is whole (always, but for the batch's last workgroup, when the block is 16-byte
// aligned and Q * k a multiple of 4) -- ten 16-byte stores of one instruction per workgroup towards the host link instead of forty
// scattered 4-byte ones of four (the block is uncached for the device: every store instruction leaves as the partial lines it covers).
// Only a query with fewer than k candidates (the caller's special case: the reference's F7 rule) also stores its key row, nkeys[q] and
// its P keys, at the query's own row of the last block; the rows of the other queries are not touched.  Nothing is stored to out_dist /
// out_idx / out_ncand; the status words stay on the device as well and the first workgroup copies them (the scan kernel, earlier on the
// stream, was the last to set them).  Plain vector stores; the end of the kernel makes them visible to the host.
__global__ __launch_bounds__(256) void bmerge_host_kernel(BArgs a, int32_t *host) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q0 = (long long)blockIdx.x * 4, q = q0 + wave;
    __shared__ uint64_t scratch[4][64];
    __shared__ int2 list_tab[4][128];
    __shared__ __attribute__((aligned(16))) int32_t ids[4 * 64];      // the workgroup's id rows, packed: query w's row at [w * k, (w + 1) * k)
    __shared__ __attribute__((aligned(16))) int32_t counts[4];
    if (q < a.Q) {
        const int c = merge_query<true>(a, q, lane, scratch[wave], list_tab[wave], ids + wave * a.k);
        if (lane == 0) counts[wave] = c;
        if (c < a.k) {       // wave-uniform
            int32_t *row = host + a.Q * a.k + a.Q + 2 + q * (a.P + 1);
            if (lane == 0) row[0] = a.nkeys[q];
            if (lane < a.P) row[1 + lane] = a.qkeys[q * a.P + lane];
        }
    }
    __syncthreads();
    const int nq = (int)(a.Q - q0 < 4 ? a.Q - q0 : 4);
    const int t = threadIdx.x, n_ids = nq * a.k;
    int32_t *ids_out = host + q0 * a.k, *counts_out = host + a.Q * a.k + q0;
    if ((((uintptr_t)ids_out & 15) | (n_ids & 3)) == 0) {      // workgroup-uniform
        if (t < n_ids / 4) reinterpret_cast<int4 *>(ids_out)[t] = reinterpret_cast<const int4 *>(ids)[t];
    } else if (t < n_ids) ids_out[t] = ids[t];
    if (nq == 4 && ((uintptr_t)counts_out & 15) == 0) {
        if (t == 0) *reinterpret_cast<int4 *>(counts_out) = *reinterpret_cast<const int4 *>(counts);
    } else if (t < nq) counts_out[t] = counts[t];
    if (blockIdx.x == 0 && t < 2) host[a.Q * a.k + a.Q + t] = a.status[t];
}

// Wide-k merge (k in 65..NLSH_MAX_K_TILED): KPL = ceil(k / 64) keys per lane, one list = KPL coalesced loads of the wave.
template <int KPL>
__global__ __launch_bounds__(256) void bmergew_kernel(BArgs a) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    __shared__ uint64_t scratch[4][NLSH_MAX_K_TILED];
    __shared__ int2 list_tab[4][128];
    if (q < a.Q) merge_query_wide<KPL>(a, q, lane, scratch[threadIdx.x >> 6], list_tab[threadIdx.x >> 6]);
}

}  // namespace nlsh
