// Wave-level building blocks shared by the query-major and bucket-major scan kernels.
#pragma once
#include "common.h"

// Diagnostic timing builds (`make VARIANT=diag EXTRA="-DNLSH_DIAG -DNLSH_ABLATE=n"`, tools/scan_bench.py): every switch below
// produces WRONG results by design (it removes a piece of the kernel to time the rest) and exists only under NLSH_DIAG, so that a
// stray -D on the shipped build cannot turn one on.  NLSH_ABLATE: 1 no distance math, 2 no global loads, 3 no top-k selection,
// 5 no epilogue, 6 neither math nor epilogue (staging skeleton), 7 tasks of <= 64 rows vanish,
// 8 tasks of <= 4 queries vanish, 9 every workgroup leaves after its descriptor loads, 11 no bisection in the
// selection, 12 = 2 + 5 (no global loads, no epilogue), 13 = 2 + 6 (barriers and LDS writes only).  NLSH_NO_STAGE_BARRIER=1: the stage barriers of the hand-scheduled task body are removed (the four waves of a
// workgroup race on the tile): what the barriers' straggler coupling costs (r03: 3-5 %).
// (Two r03 experiments lived here behind switches and were deleted in r04, measured slower and never shipped: LDS-DMA staging of the
// k-blocks, NLSH_TILED_GLDS, and the per-query merge inside the scan launch, NLSH_MERGE_IN_SCAN.  DESIGN.md appendix A and
// profiles/r03_glds_ab.txt / r03_merge_in_scan_ab.txt keep the findings; git history keeps the code.)
#ifdef NLSH_DIAG
#ifndef NLSH_ABLATE
#define NLSH_ABLATE 0
#endif
#ifndef NLSH_NO_STAGE_BARRIER
#define NLSH_NO_STAGE_BARRIER 0
#endif
#else
#if defined(NLSH_ABLATE) || defined(NLSH_NO_STAGE_BARRIER)
#error "NLSH_ABLATE / NLSH_NO_STAGE_BARRIER produce wrong results by design: diagnostic builds only (add -DNLSH_DIAG)"
#endif
#define NLSH_ABLATE 0
#define NLSH_NO_STAGE_BARRIER 0
#endif

namespace nlsh {

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}

// sum over aligned groups of LPR lanes; every lane of a group receives the same bits
template <int LPR>
__device__ __forceinline__ float group_sum(float x) {
    x += dpp_f<0xB1>(x);                    // quad_perm [1,0,3,2]
    x += dpp_f<0x4E>(x);                    // quad_perm [2,3,0,1]
    x += dpp_f<0x141>(x);                   // row_half_mirror
    x += dpp_f<0x140>(x);                   // row_mirror -> 16-lane sums
    // gfx950 v_permlane16_swap / v_permlane32_swap exchange 16-lane rows / 32-lane halves between
    // TWO registers (semantics probed on hardware: tools/probe_permlane.hip): with a = b = x,
    // a' = {x0,x0,x2,x2}, b' = {x1,x1,x3,x3}, so a' + b' is the cross-row sum in every lane with no
    // LDS round trip.  Written as asm: through the builtin hipcc (ROCm 7.2) folded the second result
    // into the first when both inputs carry the same value and emitted a' + a'.  The s_nop covers
    // the VALU-write -> permlane-read wait states (hipcc pads nothing inside asm).
    if (LPR >= 32) {
        float a = x, b = x;
        asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
        x = a + b;
    }
    if (LPR >= 64) {
        float a = x, b = x;
        asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
        x = a + b;
    }
    return x;
}

// 64-bit value of lane `src` (wave-uniform index) as a wave-uniform value: two v_readlane_b32,
// no LDS round trip (a generic __shfl compiles to ds_bpermute).
__device__ __forceinline__ uint64_t read_lane64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// value of lane-1 (lane 0 keeps its own): DPP wave_shr:1, two v_mov_b32_dpp
__device__ __forceinline__ uint64_t lane_shift_up64(uint64_t v) {
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t slo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xF, 0xF, false);
    const uint32_t shi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xF, 0xF, false);
    return ((uint64_t)shi << 32) | slo;
}

// best-64 list, sorted ascending across lanes; insert one wave-uniform key
__device__ __forceinline__ void topk_insert(uint64_t &top, uint64_t c, int lane) {
    const int posn = __popcll(__ballot(top < c));
    const uint64_t up = lane_shift_up64(top);
    top = lane < posn ? top : (lane == posn ? c : up);
}

// offer one key per lane; only keys below the current k-th best (tau) are inserted
__device__ __forceinline__ void topk_offer(uint64_t &top, uint64_t &tau, uint64_t key, int k, int lane) {
    unsigned long long m = __ballot(key < tau);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint64_t c = read_lane64(key, src);
        if (c < tau) {
            topk_insert(top, c, lane);
            const uint64_t kth = read_lane64(top, k - 1);
            tau = kth < tau ? kth : tau;  // never rises: tau may start from a bound published by another list
        }
    }
}

// Per-query running bound shared by all lists of a query (agent-scope relaxed atomics: sc1 load / atomic umin).
// tau semantics in topk_offer: a key is inserted iff key < tau, so the published bound is (k-th best key + 1).
__device__ __forceinline__ uint64_t global_tau_load(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void global_tau_publish(unsigned long long *p, uint64_t top, int k, int lane) {
    const uint64_t kth = read_lane64(top, k - 1);
    if (kth != KEY_NONE && lane == 0) atomicMin(p, (unsigned long long)kth + 1ull);
}

// wave-wide min / max of a u32 (every lane gets the result): DPP row operations, no LDS, no scalar ALU
template <bool MAX>
__device__ __forceinline__ uint32_t wave_minmax_u32(uint32_t x) {
    auto op = [](uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); };
    const uint32_t id = MAX ? 0u : 0xFFFFFFFFu;
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, (int)x, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, (int)x, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, (int)x, 0x141, 0xF, 0xF, false));  // row_half_mirror
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, (int)x, 0x140, 0xF, 0xF, false));  // row_mirror -> 16-lane result
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, (int)x, 0x142, 0xA, 0xF, false));  // row_bcast15 into rows 1 and 3
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, (int)x, 0x143, 0xC, 0xF, false));  // row_bcast31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// wave-wide inclusive prefix sum of an i32 (lane l gets x_0 + ... + x_l): four row_shr steps inside each 16-lane row (zero fill), then the
// row totals carried across with row_bcast15 / row_bcast31 -- six DPP adds, no LDS crossbar (`__shfl_up` is a ds_bpermute per step)
__device__ __forceinline__ int wave_incl_scan_i32(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);    // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);    // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);    // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);    // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);   // row_bcast15: lane 15 of rows 0 / 2 into rows 1 / 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);   // row_bcast31: lane 31 into rows 2 and 3
    return x;
}

// k smallest of the wave's NK*64 keys (NK per lane, KEY_NONE = absent), written UNSORTED to out[0..k)
// (KEY_NONE padded), without any ordered insertion.  A bisection on the distance word looks for ANY threshold that
// separates exactly k keys (ballots + scalar popcounts): it starts from the [min, max] bracket of the present
// distances (two DPP reductions) and stops as soon as a pivot has exactly k keys at or below it -- with 256 keys
// spread over the bracket that takes ~9 steps instead of the 32 a search for the exact k-th value needs.  This matters
// because a step is ~17 scalar-ALU instructions and a CU has ONE scalar unit for its four SIMDs (r02 ablation: with the
// 32-step form the selection was HALF of the tiled scan's time, 95 M of its SALU instructions per launch).  Exact
// distance ties at the k-th place (no pivot separates k keys) fall back to the exact search plus a second bisection
// on the id word.  Survivors are compacted with mbcnt prefix counts.  Returns an exclusive upper bound of this list's
// k-th best key to publish for the query (every key at or above it is beyond the list's k best) or KEY_NONE when the
// list holds fewer than k keys.
// CLAMP (the merges): keys that reach a merge are distinct when every (query, bucket) pair was scanned once -- the plan
// kernels de-duplicate a query's probe keys, corpus shards are disjoint -- but nlsh_merge_topk takes whatever lists a C
// caller hands it: with repeated keys the tie search can select more than k, so the compaction never writes past out[k).
// WIDE (k up to NLSH_MAX_K_TILED, compile time): the search and the compaction are generic in k; what assumes one output slot per lane is
// the KEY_NONE padding behind the survivors, which the wide form writes with a lane-strided loop.  The narrow form's code is unchanged.
__device__ __forceinline__ void select_pad_wide(uint64_t *out, int from, int k, int lane) {
    for (int i = lane; i < k; i += 64)
        if (i >= from) out[i] = KEY_NONE;
}

template <int NK, bool CLAMP = false, bool WIDE = false>
__device__ __forceinline__ uint64_t select_k_smallest(const uint64_t (&key)[NK], int k, int lane, uint64_t *out) {
    uint32_t hi[NK], lo[NK];
    int n = 0;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        hi[i] = (uint32_t)(key[i] >> 32);
        lo[i] = (uint32_t)key[i];
        n += __popcll(__ballot(key[i] != KEY_NONE));
    }
    // r05: the two short cases first.  18-36 % of the tiled scan's lists reach this point with NO key below the query's published bound and
    // 23-41 % with fewer than k (profiles/r05_epilogue_counters_and_ablations.txt): neither needs a cut, and the general compaction below
    // spends six compares per key slot re-deriving "present" from a cut that takes everything (r04's single path: same results, slower).
    if (n == 0) {
        if constexpr (WIDE) select_pad_wide(out, 0, k, lane);
        else if (lane < k) out[lane] = KEY_NONE;
        return KEY_NONE;
    }
    if (n < k) {
        int base0 = 0;
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const bool sel = key[i] != KEY_NONE;
            const unsigned long long m = __ballot(sel);
            if (m) {   // wave-uniform: an absent tile costs one scalar compare
                const int pos = base0 + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (sel) out[pos] = key[i];
                base0 += __popcll(m);
            }
        }
        if constexpr (WIDE) select_pad_wide(out, base0, k, lane);
        else if (lane >= base0 && lane < k) out[lane] = KEY_NONE;
        return KEY_NONE;
    }
    uint32_t dk = 0xFFFFFFFFu, idk = 0xFFFFFFFFu;  // take everything present (hi of a present key < 0xFFFFFFFF)
    if (n >= k) {
        uint32_t mn = hi[0], mx = hi[0] == 0xFFFFFFFFu ? 0u : hi[0];
#pragma unroll
        for (int i = 1; i < NK; ++i) {
            mn = hi[i] < mn ? hi[i] : mn;
            const uint32_t h = hi[i] == 0xFFFFFFFFu ? 0u : hi[i];
            mx = h > mx ? h : mx;
        }
        uint32_t a = wave_minmax_u32<false>(mn), b = wave_minmax_u32<true>(mx);
        // invariants: #{hi <= b} >= k (b = max: all n > k keys) and #{hi < a} < k (a = min: none)
        bool split = false;
        if (n == k) { a = b; split = true; }   // all present keys are taken: the cut is the largest of them
#if NLSH_ABLATE == 11   // diagnostic timing build (WRONG results): no bisection at all -- what the search for the cut costs
        a = b; split = true;
#endif
        while (a < b) {
            const uint32_t mid = a + ((b - a) >> 1);
            int cnt = 0;
#pragma unroll
            for (int i = 0; i < NK; ++i) cnt += __popcll(__ballot(hi[i] <= mid));
            if (cnt == k) { a = mid; split = true; break; }   // exactly k keys at or below the pivot: done
            if (cnt > k) b = mid; else a = mid + 1;
        }
        dk = a;
        if (!split) {   // a == b = the k-th distance, shared by keys on both sides of the cut (or n has exactly k at/below max)
            int c_less = 0, c_eq = 0;
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                c_less += __popcll(__ballot(hi[i] < dk));
                c_eq += __popcll(__ballot(hi[i] == dk));
            }
            const int need = k - c_less;  // >= 1 keys to take among those at distance d_k
            if (c_eq > need) {            // exact distance ties: smallest ids win
                a = 0; b = 0xFFFFFFFFu;
                while (a < b) {
                    const uint32_t mid = a + ((b - a) >> 1);
                    int cnt = 0;
#pragma unroll
                    for (int i = 0; i < NK; ++i) cnt += __popcll(__ballot(hi[i] == dk && lo[i] <= mid));
                    if (cnt >= need) b = mid; else a = mid + 1;
                }
                idk = a;
            }
        }
    }
    int base = 0;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        const bool sel = key[i] != KEY_NONE && (hi[i] < dk || (hi[i] == dk && lo[i] <= idk));
        const unsigned long long m = __ballot(sel);
        const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#if NLSH_ABLATE == 11
        if (sel && pos < k) {
#else
        if (sel && (!CLAMP || pos < k)) {
#endif
            out[pos] = key[i];
        }
        base += __popcll(m);
    }
    if constexpr (WIDE) select_pad_wide(out, base, k, lane);
    else if (lane >= base && lane < k) out[lane] = KEY_NONE;
    return n >= k ? ((uint64_t)dk + 1ull) << 32 : KEY_NONE;
}

// Merging many short lists by SELECTION instead of ordered insertion: a wave keeps its current best k keys unsorted in
// lanes 0..k-1 (`carry`), takes NK-1 new keys per lane and round, lets select_k_smallest pick the k best of all NK*64 and
// reads them back from a per-wave LDS scratch (k keys, compacted: real keys first, KEY_NONE after).  The ordered
// insertion it replaces (topk_offer) cost ~100 instructions per inserted key and the first list of every query inserts
// all of its k keys.  merge_finish ranks the k survivors (k uniform compare steps) and stores them in ascending order.
template <int NK>
__device__ __forceinline__ uint64_t merge_round(uint64_t (&key)[NK], int k, int lane, uint64_t *scratch) {
    select_k_smallest<NK, true>(key, k, lane, scratch);
    return lane < k ? scratch[lane] : KEY_NONE;   // same wave wrote it: LDS operations of a wave complete in order
}

__device__ __forceinline__ void merge_finish(uint64_t carry, int k, int lane, float *out_dist, int32_t *out_idx, uint64_t *out_keys, long long q) {
    int rank = 0;
    for (int j = 0; j < k; ++j) {   // keys are distinct ((distance, id) with distinct ids), KEY_NONE sits behind the real ones;
        const uint64_t kj = read_lane64(carry, j);   // equal keys (a C caller's repeated lists) are ordered by lane: every slot is written
        rank += (kj < carry || (kj == carry && j < lane)) ? 1 : 0;
    }
    if (lane < k) {
        const bool none = carry == KEY_NONE;
        const int pos = none ? lane : rank;
        out_dist[q * k + pos] = none ? __builtin_inff() : float_from_mono((uint32_t)(carry >> 32));
        out_idx[q * k + pos] = none ? -1 : (int32_t)(uint32_t)carry;
        if (out_keys) out_keys[q * k + pos] = carry;
    }
}

// merge_finish for a caller that wants only the ids, in a buffer of its own (k words, LDS): same order, -1 past a short list.
// (The ranking loop is merge_finish's, repeated: with the loop in a helper shared by both, bmerge_kernel and merge_shards_kernel no longer
// compile to the parent's instructions -- tools/isa_lint.py --compare classes them d -- and the narrow merge is bound by its instruction count.)
__device__ __forceinline__ void merge_finish_ids(uint64_t carry, int k, int lane, int32_t *ids) {
    int rank = 0;
    for (int j = 0; j < k; ++j) {
        const uint64_t kj = read_lane64(carry, j);
        rank += (kj < carry || (kj == carry && j < lane)) ? 1 : 0;
    }
    if (lane < k) {
        const bool none = carry == KEY_NONE;
        ids[none ? lane : rank] = none ? -1 : (int32_t)(uint32_t)carry;
    }
}

// Wide k (65..NLSH_MAX_K_TILED = 256): the same merge by selection with KPL = ceil(k / 64) keys per lane -- entry e of a k-key list sits in
// register e / 64 of lane e % 64.  A round selects the k best of the carry and of NL new lists (NK = KPL * (1 + NL) <= 8 keys per lane) into
// the wave's LDS scratch (k keys; NLSH_MAX_K_TILED of them per wave are reserved) and reads the carry back from it.
template <int NK, int KPL>
__device__ __forceinline__ void merge_round_wide(const uint64_t (&key)[NK], uint64_t (&carry)[KPL], int k, int lane, uint64_t *scratch) {
    select_k_smallest<NK, true, true>(key, k, lane, scratch);
#pragma unroll
    for (int i = 0; i < KPL; ++i) carry[i] = i * 64 + lane < k ? scratch[i * 64 + lane] : KEY_NONE;   // same wave wrote it (see merge_round)
}

// Final ordering of the wide carry: every lane ranks its KPL keys against the survivors in the scratch copy (one broadcast LDS read per
// survivor, KPL compares each).  `scratch` is what the LAST round left: real keys in [0, n_real), KEY_NONE behind -- with no round at all the
// carry is all KEY_NONE, n_real = 0 and the scratch is never read.  Same order and padding as merge_finish.
template <int KPL>
__device__ __forceinline__ void merge_finish_wide(const uint64_t (&carry)[KPL], const uint64_t *scratch, int k, int lane, float *out_dist,
                                                  int32_t *out_idx, uint64_t *out_keys, long long q) {
    int n_real = 0, rank[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        n_real += __popcll(__ballot(carry[i] != KEY_NONE));
        rank[i] = 0;
    }
    for (int j = 0; j < n_real; ++j) {   // equal keys (a C caller's repeated lists) are ordered by slot: every slot is written
        const uint64_t kj = scratch[j];
#pragma unroll
        for (int i = 0; i < KPL; ++i) rank[i] += (kj < carry[i] || (kj == carry[i] && j < i * 64 + lane)) ? 1 : 0;
    }
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const int slot = i * 64 + lane;
        if (slot < k) {
            const bool none = carry[i] == KEY_NONE;
            const int pos = none ? slot : rank[i];
            out_dist[q * k + pos] = none ? __builtin_inff() : float_from_mono((uint32_t)(carry[i] >> 32));
            out_idx[q * k + pos] = none ? -1 : (int32_t)(uint32_t)carry[i];
            if (out_keys) out_keys[q * k + pos] = carry[i];
        }
    }
}

__device__ __forceinline__ void store_topk(float *out_dist, int32_t *out_idx, uint64_t *out_keys, long long q, int k,
                                           uint64_t top, int lane) {
    if (lane < k) {
        const bool none = top == KEY_NONE;
        out_dist[q * k + lane] = none ? __builtin_inff() : float_from_mono((uint32_t)(top >> 32));
        out_idx[q * k + lane] = none ? -1 : (int32_t)(uint32_t)top;
        if (out_keys) out_keys[q * k + lane] = top;
    }
}

// Query fragment of one lane: columns 4*(li + v*LPR) .. +3, padded so that padding contributes 0
// (L2: (q - 0) + eps == 0 with q = -eps; cosine: 0).  Cosine fragments are pre-divided by
// max(||q||, 1e-8) like cosine_similarity does with x1.
template <int LPR, int VPL, int METRIC>
__device__ __forceinline__ void load_query(const float *qp, int d, int li, float4 (&qv)[VPL], bool (&act)[VPL]) {
    const float padv = METRIC == NLSH_METRIC_L2_EPS ? -1e-6f : 0.0f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
        const int c0 = 4 * (li + v * LPR);
        act[v] = c0 < d;
        qv[v].x = c0 + 0 < d ? qp[c0 + 0] : padv;
        qv[v].y = c0 + 1 < d ? qp[c0 + 1] : padv;
        qv[v].z = c0 + 2 < d ? qp[c0 + 2] : padv;
        qv[v].w = c0 + 3 < d ? qp[c0 + 3] : padv;
    }
    if (METRIC == NLSH_METRIC_COSINE) {
        float ss = 0.0f;
#pragma unroll
        for (int v = 0; v < VPL; ++v)
            if (act[v]) { ss = fmaf(qv[v].x, qv[v].x, ss); ss = fmaf(qv[v].y, qv[v].y, ss); ss = fmaf(qv[v].z, qv[v].z, ss); ss = fmaf(qv[v].w, qv[v].w, ss); }
        ss = group_sum<LPR>(ss);
        const float nrm = fmaxf(sqrtf(ss), 1e-8f);
#pragma unroll
        for (int v = 0; v < VPL; ++v) { qv[v].x /= nrm; qv[v].y /= nrm; qv[v].z /= nrm; qv[v].w /= nrm; }
    }
}

// lane-partial of one row against one query fragment
template <int VPL, int METRIC>
__device__ __forceinline__ float row_partial(const float4 (&qv)[VPL], const bool (&act)[VPL], const float4 (&cv)[VPL]) {
    float sacc = 0.0f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
        if (METRIC == NLSH_METRIC_L2_EPS) {
            // F.pairwise_distance: || (x1 - x2) + eps ||  (nlsh/data.py:201)
            float t0 = (qv[v].x - cv[v].x) + 1e-6f, t1 = (qv[v].y - cv[v].y) + 1e-6f;
            float t2 = (qv[v].z - cv[v].z) + 1e-6f, t3 = (qv[v].w - cv[v].w) + 1e-6f;
            float part = fmaf(t3, t3, fmaf(t2, t2, fmaf(t1, t1, t0 * t0)));
            sacc += act[v] ? part : 0.0f;
        } else {
            sacc += fmaf(qv[v].w, cv[v].w, fmaf(qv[v].z, cv[v].z, fmaf(qv[v].y, cv[v].y, qv[v].x * cv[v].x)));
        }
    }
    return sacc;
}

// Correctly rounded sqrtf for x >= 2^-96 (and for +0, +inf and NaN, which come out as sqrtf gives them): the core of the sequence hipcc
// emits for sqrtf -- v_sqrt_f32 (1 ulp), then the two one-ulp neighbours are tried against the residual x - s'*s computed by ONE fma each
// -- without the x * 2^32 / * 2^-16 range scaling it wraps around that core for arguments below 2^-96 and without the class test that
// passes zeros and infinities through (27 VALU per call as compiled, 11 here).  The tiled scan takes 16 square roots per lane and task;
// callers hold the wave's arguments against 2^-96 first and fall back to sqrtf when any lies below (never on real distances: the smallest
// is sqrt(d) * 1e-6 for a query that IS a corpus row).
__device__ __forceinline__ float sqrt_rn_unscaled(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) - 1u), sp = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) + 1u);
    const float rm = fmaf(-sm, s, x), rp = fmaf(-sp, s, x);
    float r = rm <= 0.0f ? sm : s;
    r = rp > 0.0f ? sp : r;
    return r;
}

template <int METRIC>
__device__ __forceinline__ float finish_distance(float acc, float inv_norm) {
    if (METRIC != NLSH_METRIC_COSINE) return sqrtf(acc);   // both L2 forms
    return 1.0f - acc * inv_norm;  // 1 - cos (nlsh/data.py:109)
}

static inline size_t ws_align(size_t x) { return (x + 255) & ~(size_t)255; }

// One scan call, for all three schedules: what every C entry point (scan_topk.hip, scan_bucket_range.hip) and every batch of a step
// descriptor (step.hip) fills by member name, scan_call_check checks and scan_call_run enqueues.  Start from `BucketScanCall c = {}`.
struct BucketScanCall {
    const float *corpus; long long row_stride; int d; const int32_t *gid; const int32_t *uniq; const int32_t *offsets; int nb;
    const float *inv_norm; const float *queries; long long q_stride; long long Q; const int32_t *qkeys; const int32_t *nkeys;
    int P, k, metric;
    int algo;                     // NLSH_SCAN_*: the schedule; set here and nowhere else (tiled() below is what the bucket-major code asks)
    int seg;                      // seg_rows as the caller gave them (0 = default): scan_seg_rows() is what the two non-tiled schedules cut by
    float *out_dist; int32_t *out_idx; uint64_t *out_keys; int32_t *out_ncand; int32_t *status;
    void *workspace; size_t workspace_bytes; long long max_tasks; void *ev_begin; void *ev_end; hipStream_t stream;
    const int32_t *bucket_order;  // nlsh_bucket_order output (nlsh_build_cells' cell_order when cells are given) or nullptr
    int phases;                   // NLSH_PHASE_PLAN | NLSH_PHASE_SCAN | NLSH_PHASE_MERGE (| NLSH_PHASE_PLAN_REST, step.hip only)
    const int32_t *cell_of;       // nlsh_build_cells outputs, or nullptr / 0: every bucket is its own cell
    const int32_t *cell_offsets;
    int n_cells;
    int plan_blocks;              // NLSH_PHASE_PLAN_REST: workgroups of the encode_hash launch that did the lookup (entries of `hits`)
    int32_t *host_out;            // nlsh_query_batch_host: the MERGE phase (k <= NLSH_MAX_K) stores its results into this host-visible block
                                  // (layout: bmerge_host_kernel) instead of out_dist / out_idx / out_ncand; nullptr everywhere else
    int storage;                  // NLSH_STORE_*: what `corpus` really points to (row_stride in elements); anything but F32 is the tiled
                                  // schedule's alone (0 = F32 for every entry without a storage argument)
    const uint32_t *row_filter;   // bitset over the sorted rows (nlsh_row_filter_build) or nullptr: the tiled schedule's alone; the SCAN phase
                                  // then launches a filtered kernel, which reads it from its second parameter (SideArgs; BArgs does not hold it)
    bool affine;                  // nlsh_scan_topk_cells_phase_sq8: `corpus` holds sq8 codes in the uint8 layout (storage = NLSH_STORE_U8) and the
                                  // SCAN phase launches an affine kernel, which reads the quantiser (and the filter) from its second parameter
    const float *quant_lo;        // affine: [row_stride] per-dimension offsets, padded to the pitch with 0 (device, 16-byte aligned)
    const float *quant_step;      // affine: [row_stride] per-dimension steps, padded with 1
    const uint64_t *row_tags;     // nlsh_scan_topk_cells_phase_tagged / _sq8_tagged: [N] tag word of every sorted row, or nullptr: no tags.  The
                                  // tiled schedule's alone; the SCAN phase then launches a tagged kernel, whose second parameter (SideArgs) holds
                                  // the tags, the masks, the mode, the filter and -- affine -- the quantiser
    const uint64_t *query_masks;  // [Q] mask of every query; given iff row_tags is
    int tag_match;                // NLSH_TAG_ANY | NLSH_TAG_ALL | NLSH_TAG_EQ; looked at only with row_tags
    bool pq;                      // nlsh_scan_topk_cells_phase_pq: `corpus` holds product-quantiser codes, M = ceil(d / pq_dsub) bytes per row
                                  // (storage = NLSH_STORE_U8, row_stride = M * pq_dsub: the decoded row's width), and the SCAN phase launches a
                                  // PQ kernel, which reads the three fields below from a third parameter of its own (PqArgs)
    const float *pq_codebook;     // pq: [M, 256, pq_dsub] float32 (device, 16-byte aligned), columns at or beyond d held as +0
    int pq_dsub;                  // pq: 4 | 8 | 16
    long long pq_pitch;           // pq: bytes between the code rows, a multiple of 16 and >= M
    bool tiled() const { return algo == NLSH_SCAN_BUCKET_TILED; }
};
// internal phase bit (not part of the C ABI's phase mask): the PLAN phase WITHOUT the bucket lookup, which the batch's encode_hash
// launch already did in its epilogue (scan_plan.h, encode_plan_fuse_lookup): bscan + bscatter only
#define NLSH_PHASE_PLAN_REST 8
inline int scan_seg_rows(int seg_rows) { return ((seg_rows ? seg_rows : 512) + 63) / 64 * 64; }

// The members every scan entry point of the C ABI has, under the parameter names the header gives them: the one place they are copied.
#define NLSH_SCAN_CALL_COMMON(c)                                                                                                         \
    (c).corpus = (const float *)corpus_sorted; (c).row_stride = row_stride; (c).d = d; (c).gid = gid; (c).uniq = uniq_keys;              \
    (c).offsets = offsets; (c).nb = n_buckets; (c).bucket_order = bucket_order; (c).inv_norm = inv_norm; (c).queries = queries;           \
    (c).q_stride = q_stride; (c).Q = Q; (c).qkeys = qkeys; (c).nkeys = nkeys; (c).P = P; (c).metric = metric; (c).algo = algo;            \
    (c).status = status; (c).workspace = workspace; (c).workspace_bytes = workspace_bytes; (c).max_tasks = max_tasks;                     \
    (c).ev_begin = ev_scan_begin; (c).ev_end = ev_scan_end; (c).stream = (hipStream_t)stream

// THE argument check of a scan call (scan_topk.hip): limits, schedule, storage, filter, null pointers, strides and alignments, for every
// entry.  Host arithmetic only, before anything is enqueued; `who` prefixes the message.  An empty batch (Q == 0) passes without its
// pointers being looked at: the caller returns NLSH_OK for it after its own checks.
enum : unsigned {
    SCAN_NEEDS_TOPK_OUT = 1,      // out_dist, out_idx and out_ncand are written (every top-k call; a radius call has outputs of its own)
    SCAN_ALLOWS_PLAN_REST = 2,    // the internal phase bit may be set (step.hip); the C ABI's phase mask ends at NLSH_PHASE_MERGE
};
int scan_call_check(const char *who, const BucketScanCall &c, unsigned needs);
size_t bucket_scan_workspace(long long Q, int P, int k, long long max_tasks, long long n_buckets, int d);
int query_major_workspace(const BucketScanCall &c);   // holds workspace_bytes against the query-major layout
int query_major_run(const BucketScanCall &c);         // scan_topk.hip
int bucket_scan_run(const BucketScanCall &c);         // scan_bucket.hip
inline int scan_call_run(const BucketScanCall &c) { return c.algo == NLSH_SCAN_QUERY_MAJOR ? query_major_run(c) : bucket_scan_run(c); }
// the tiled scan kernel over a float16 / uint8 corpus (scan_bucket_typed.hip): storage NLSH_STORE_F16 | NLSH_STORE_U8, wide = k > NLSH_MAX_K
const void *typed_scan_kernel_of(int storage, int metric, bool wide);
// the tiled scan kernel behind a row filter (scan_bucket_filtered.hip): any storage; its parameters are (BArgs, SideArgs: scan_bucket_args.h), like the next two
const void *filtered_scan_kernel_of(int storage, int metric, bool wide);
// the tiled scan kernel over an sq8 corpus (scan_bucket_affine.hip), the quantiser and the filter inside the second parameter
const void *affine_scan_kernel_of(int metric, bool wide);
// the tiled scan kernel behind per-query tag filters (scan_bucket_tagged.hip): any storage, NLSH_STORE_SQ8 (scan_bucket_args.h) for an
// affine call; tags, masks, mode, the filter and the quantiser inside the second parameter
const void *tagged_scan_kernel_of(int storage, int metric, bool wide);
// the tiled scan kernel over a product-quantised corpus (scan_bucket_pq.hip): its parameters are (BArgs, SideArgs, PqArgs)
const void *pq_scan_kernel_of(int metric, bool wide);

}  // namespace nlsh
