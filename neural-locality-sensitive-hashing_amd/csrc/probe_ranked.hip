// nlsh_probe_ranked: likelihood-ranked multi-probe keys (include/nlsh_hip.h).
//
// For independent bits the log-odds of hasher bit h is the output pre-activation z[h] (sigmoid; 2 z[h] for the tanh head: the same
// order), so flipping a bit away from the hard code costs c[h] = |z[h]| and the n most probable codes are the n subsets of bits with
// the smallest cost sums.  The kernel enumerates them best-first (the shift / expand search of Lv et al.'s multi-probe LSH) over the
// bits sorted by cost; the exact order, ties included, is the one the header defines, so a result is a pure function of the row.
//
// One wavefront per row, everything in registers:
//   - the <= 32 costs are sorted by counting rank across lanes (32 lane reads for the rank, 32 for the inverse permutation);
//     lane i then holds sorted position i: its cost cs[i] and the code bit bv[i] = 1 << (H-1-s[i]) a flip of it toggles;
//   - the frontier holds up to 128 entries, two per lane (slot t = lane t & 63, register set t >> 6); an entry is
//     (cost bits, mask, chain without its last term, code bits flipped so far), an empty one has the 64-bit key ~0;
//   - a pop is a wave-wide minimum of the 64-bit key cost << 32 | mask (keys are distinct: masks are); the winning lane overwrites
//     its entry with the shift child, the expand child goes to the next unused slot.  After m pops at most m + 1 slots are in use,
//     so 128 slots serve n_probes <= 128;
//   - the popped codes stay in registers (slot p = lane p & 63) until the row is de-duplicated and stored.
// Every register set is named, none is indexed at run time: the kernel has no private segment.  The loop makes a fixed
// n_probes - 1 pops and every slot index is bounded by a constant, whatever the bits of z are.
//
// nlsh_probe_ranked_budget is the same loop (`probe_row<true>`) with a per-row stop: each KEPT key's bucket size is looked up in the
// index's CSR arrays and the loop ends after the first key that brings the row's candidate count to `budget`.  What differs:
//   - the first-occurrence de-duplication happens at pop time (the popped key against the kept keys, which sit one per lane: a compare
//     and a ballot), so a duplicate takes no slot and adds no candidates, and kept slot c lives in lane c & 63;
//   - the lookup is a 64-way search over uniq_keys: lane l probes the l-th of 64 evenly spaced entries of the current range, a ballot
//     of `entry <= key` names the sub-range, the range shrinks 64-fold per round.  The first round's 64 entries depend on n_buckets
//     alone and are loaded once per row into a register; the last round (stride 1) loads the two offsets beside the key, so a lookup
//     is ceil(log64(n_buckets)) dependent global round trips, one fewer when n_buckets > 64 (65 k buckets: 2).
// The unbudgeted kernel is `probe_row<false>`: every budget branch is `if constexpr`, its code is what it was.
//
// probe_ranked_plan_kernel<BUDGET> (nlsh_query_batch_ranked, step.hip) is the same loop again (`probe_row<BUDGET, true>`) and the THIRD
// home of the bucket lookup of the scan's PLAN phase (scan_plan.h; after bplan_kernel and encode_hash's epilogue): the row's kept keys sit
// one per lane after the compaction, so each lane looks its key up (`plan_pair`) in the launch that ranked it and the scan call continues
// with NLSH_PHASE_PLAN_REST -- the key table still goes out (the merge's key rows, the retry after a task-table overflow), but no kernel
// reads it back for a per-key search.  16 rows (wavefronts) per workgroup instead of 4: the `hits` array of the workspace has an entry per
// 16 queries (plan_blocks_max, scan_bucket.hip), and the 4-KB coarse key table is loaded once per 16 rows.  Waves past the last row skip
// the row work and still reach both barriers.  The plan branches are `if constexpr` too: the two kernels above compile to what they were.
// (Persistent workgroups -- two per CU, every wave walking its own rows, the coarse table loaded once per workgroup and no wave waiting
// for its neighbours' rows -- do not fit: inside a row loop the compiler needs 90 VGPRs, or spills 36-120 bytes per lane to scratch when
// held to the 64 that two 16-wave workgroups per CU leave; profiles/ranked_one_call.txt.)
#include "common.h"
#include "scan_plan.h"
#include "probe_lookup.h"   // lane_read, bucket_size: shared with probe_categorical.hip

namespace nlsh {
namespace {

constexpr int PR_ROWS = 4;          // rows (wavefronts) per workgroup
constexpr int PRP_ROWS = 16;        // ... of the kernel that also does the bucket lookup: one entry of `hits` per 16 queries
constexpr uint32_t PR_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t add_bits(uint32_t a, uint32_t b) {   // one fp32 add on bit patterns
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b));
}
__device__ __forceinline__ int32_t key_of(uint32_t code, int key_mode) {
    return key_mode == NLSH_KEY_REF_INT16 ? (int32_t)(int16_t)(uint16_t)(code & 0xFFFFu) : (int32_t)code;
}

template <bool BUDGET, bool PLAN = false>
__device__ __forceinline__ void probe_row(const float *__restrict__ z, long long z_stride, const uint32_t *__restrict__ code, long long n,
                                          int H, int key_mode, int P, long long n_multi_rows, const int32_t *__restrict__ uniq,
                                          const int32_t *__restrict__ offsets, uint32_t nb, int32_t budget,
                                          int32_t *__restrict__ keys_out, int32_t *__restrict__ nkeys_out, float *__restrict__ cost_out,
                                          int32_t *__restrict__ ncand_out, [[maybe_unused]] const PlanArgs *pa = nullptr,
                                          [[maybe_unused]] const int32_t *coarse = nullptr, [[maybe_unused]] bool *hit_out = nullptr,
                                          [[maybe_unused]] int *viol_out = nullptr) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (PLAN ? PRP_ROWS : PR_ROWS) + (threadIdx.x >> 6);
    if (row >= n) return;   // wave-uniform (PLAN: back to the kernel, which goes on to its barrier)

    // ---- costs, sorted by (bit pattern, bit index): lanes past H hold a sentinel above every cleared-sign pattern
    uint32_t c = PR_NONE;
    if (lane < H) c = __builtin_bit_cast(uint32_t, z[row * z_stride + lane]) & 0x7FFFFFFFu;
    // budgeted: made wave-uniform for the compiler (one address per wave), so the popped keys and the lookups are scalar
    const uint32_t hard = BUDGET ? (uint32_t)__builtin_amdgcn_readfirstlane((int)code[row]) : code[row];
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)c, j);
        rank += (cj < c || (cj == c && j < lane)) ? 1 : 0;
    }
    uint32_t cs = PR_NONE;   // cost at sorted position `lane`
    int s = 0;               // its bit index
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int rj = __builtin_amdgcn_readlane(rank, j);
        const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)c, j);
        if (rj == lane) { cs = cj; s = j; }
    }
    const uint32_t bv = lane < H ? 1u << (H - 1 - s) : 0u;

    // ---- frontier: slots 0..63 in the a_ set, 64..127 in the b_ set; the root {0} in slot 0
    uint32_t a_cost = PR_NONE, a_mask = PR_NONE, a_tp = 0, a_flip = 0;
    uint32_t b_cost = PR_NONE, b_mask = PR_NONE, b_tp = 0, b_flip = 0;
    {
        const uint32_t c0 = lane_read(cs, 0), b0 = lane_read(bv, 0);
        if (lane == 0) { a_cost = add_bits(0u, c0); a_mask = 1u; a_tp = 0u; a_flip = b0; }
    }
    int count = 1;   // slots in use
    // popped subsets: slot p in lane p & 63; slot 0 is the empty set
    uint32_t o_code0 = hard, o_cost0 = 0u, o_code1 = hard, o_cost1 = 0u;
    int cnt = 1;
    int np = row < n_multi_rows ? P : 1;
    // budget: slot 0 is kept whatever its bucket holds; a row whose hard bucket meets the budget makes no pop
    [[maybe_unused]] int32_t top = 0, cum = 0;
    [[maybe_unused]] const bool collide = key_mode == NLSH_KEY_REF_INT16 && H > 16;
    if constexpr (BUDGET) {
        if (nb) {
            const uint32_t at = (uint32_t)lane * ((nb + 63u) >> 6);
            if (at < nb) top = uniq[at];
            cum = bucket_size(key_of(hard, key_mode), uniq, offsets, nb, top, lane);
        }
        if (cum >= budget) np = 1;
    }
    for (int p = 1; p < np; ++p) {
        const unsigned long long ka = (unsigned long long)a_cost << 32 | a_mask, kb = (unsigned long long)b_cost << 32 | b_mask;
        const bool use_b = kb < ka;
        const unsigned long long km = use_b ? kb : ka;
        unsigned long long g = km;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned long long o = __shfl_xor(g, m);
            g = o < g ? o : g;
        }
        if (g == KEY_NONE) break;   // wave-uniform: all 2^H subsets are taken
        const int wl = __ffsll((long long)__ballot(km == g)) - 1;
        const uint32_t t = (uint32_t)(g >> 32), mask = (uint32_t)g;
        const uint32_t tp = lane_read(use_b ? b_tp : a_tp, wl), flip = lane_read(use_b ? b_flip : a_flip, wl);
        [[maybe_unused]] bool stop = false;
        if constexpr (BUDGET) {
            // a key seen before adds no candidates and takes no slot (its children are still pushed: the enumeration is the same)
            const int32_t key = key_of(hard ^ flip, key_mode);
            bool dup = false;
            if (collide)
                dup = __ballot((lane < cnt && key_of(o_code0, key_mode) == key) || (lane + 64 < cnt && key_of(o_code1, key_mode) == key)) != 0ull;
            if (!dup) {
                if (cnt < 64) {
                    if (lane == cnt) { o_code0 = hard ^ flip; o_cost0 = t; }
                } else if (lane == cnt - 64) {
                    o_code1 = hard ^ flip; o_cost1 = t;
                }
                ++cnt;
                if (nb) cum += bucket_size(key, uniq, offsets, nb, top, lane);   // disjoint buckets: cum <= N < 2^31
                stop = cum >= budget;
            }
        } else {
            if (p < 64) {
                if (lane == p) { o_code0 = hard ^ flip; o_cost0 = t; }
            } else if (lane == p - 64) {
                o_code1 = hard ^ flip; o_cost1 = t;
            }
            cnt = p + 1;
        }
        if constexpr (BUDGET) {
            if (stop) break;   // wave-uniform; the frontier is not needed any more
        }
        // children: only the last term of the chain changes (shift) or is appended (expand)
        const int j = 31 - __clz((int)mask);
        uint32_t s_cost = PR_NONE, s_mask = PR_NONE, s_tp = 0, s_flip = 0;
        if (j + 1 < H) {
            const uint32_t cn = lane_read(cs, j + 1), bj = lane_read(bv, j), bn = lane_read(bv, j + 1);
            s_cost = add_bits(tp, cn); s_mask = mask ^ (3u << j); s_tp = tp; s_flip = flip ^ bj ^ bn;
            const uint32_t e_cost = add_bits(t, cn), e_mask = mask | (1u << (j + 1)), e_flip = flip ^ bn;
            if (count < 64) {
                if (lane == count) { a_cost = e_cost; a_mask = e_mask; a_tp = t; a_flip = e_flip; }
            } else if (count < 128 && lane == count - 64) {
                b_cost = e_cost; b_mask = e_mask; b_tp = t; b_flip = e_flip;
            }
            ++count;
        }
        if (lane == wl) {
            if (use_b) { b_cost = s_cost; b_mask = s_mask; b_tp = s_tp; b_flip = s_flip; }
            else       { a_cost = s_cost; a_mask = s_mask; a_tp = s_tp; a_flip = s_flip; }
        }
    }

    // ---- keys, first-occurrence de-duplication (only 16-bit keys of wider codes can collide), store
    const int32_t key0 = key_of(o_code0, key_mode), key1 = key_of(o_code1, key_mode);
    bool first0 = lane < cnt, first1 = lane + 64 < cnt;
    if (!BUDGET && key_mode == NLSH_KEY_REF_INT16 && H > 16) {   // (the budgeted loop kept distinct keys only)
        for (int u = 0; u < cnt; ++u) {
            const int32_t ku = (int32_t)(u < 64 ? lane_read((uint32_t)key0, u) : lane_read((uint32_t)key1, u - 64));
            if (u < lane && ku == key0) first0 = false;
            if (u < lane + 64 && ku == key1) first1 = false;
        }
    }
    const unsigned long long m0 = __ballot(first0), m1 = __ballot(first1), below = (1ull << lane) - 1ull;
    const int n0 = __popcll(m0), nk = n0 + __popcll(m1);
    const long long base = row * (long long)P;
    if (first0) {
        const int pos = __popcll(m0 & below);
        keys_out[base + pos] = key0;
        if (cost_out) cost_out[base + pos] = __builtin_bit_cast(float, o_cost0);
    }
    if (first1) {
        const int pos = n0 + __popcll(m1 & below);
        keys_out[base + pos] = key1;
        if (cost_out) cost_out[base + pos] = __builtin_bit_cast(float, o_cost1);
    }
    for (int t = lane; t < P; t += 64) {
        if (t >= nk) {
            keys_out[base + t] = 0;
            if (cost_out) cost_out[base + t] = __builtin_bit_cast(float, 0x7F800000u);
            if constexpr (PLAN) pa->ppair[base + t] = make_int4(-1, 0, 0, 0);   // a dead slot: bscatter_kernel reads all Q * P records
        }
    }
    if constexpr (PLAN) {
        // P <= 64 here, so every kept key is in the first register set, one per lane: the row's lookups are issued together
        if (first0) *hit_out = plan_pair(*pa, coarse, base + __popcll(m0 & below), key0, true, *viol_out);
    }
    if (lane == 0) nkeys_out[row] = nk;
    if constexpr (BUDGET) {
        if (lane == 0 && ncand_out) ncand_out[row] = cum;
    }
}

__global__ __launch_bounds__(PR_ROWS * 64) void probe_ranked_kernel(const float *__restrict__ z, long long z_stride,
                                                                    const uint32_t *__restrict__ code, long long n, int H, int key_mode,
                                                                    int P, long long n_multi_rows, int32_t *__restrict__ keys_out,
                                                                    int32_t *__restrict__ nkeys_out, float *__restrict__ cost_out) {
    probe_row<false>(z, z_stride, code, n, H, key_mode, P, n_multi_rows, nullptr, nullptr, 0u, 0, keys_out, nkeys_out, cost_out, nullptr);
}

__global__ __launch_bounds__(PR_ROWS * 64) void probe_ranked_budget_kernel(const float *__restrict__ z, long long z_stride,
                                                                           const uint32_t *__restrict__ code, long long n, int H,
                                                                           int key_mode, int P, long long n_multi_rows,
                                                                           const int32_t *__restrict__ uniq, const int32_t *__restrict__ offsets,
                                                                           uint32_t nb, int32_t budget, int32_t *__restrict__ keys_out,
                                                                           int32_t *__restrict__ nkeys_out, float *__restrict__ cost_out,
                                                                           int32_t *__restrict__ ncand_out) {
    probe_row<true>(z, z_stride, code, n, H, key_mode, P, n_multi_rows, uniq, offsets, nb, budget, keys_out, nkeys_out, cost_out, ncand_out);
}

// Ranked keys AND their bucket lookup (see the head of this file).  What the launch leaves is what bplan_kernel leaves for the same key
// table: a pair record per (row, slot), the cell counters incremented, tauq, the padded / pre-normalised query copy when the schedule
// reads one (by the wave that owns the query), status / look-back slots initialised by block 0, and the block's entry of `hits`.
template <bool BUDGET>
__global__ __launch_bounds__(PRP_ROWS * 64) void probe_ranked_plan_kernel(const float *__restrict__ z, long long z_stride,
                                                                          const uint32_t *__restrict__ code, int H, int key_mode,
                                                                          long long n_multi_rows, int32_t budget, PlanArgs a,
                                                                          int32_t *__restrict__ keys_out, int32_t *__restrict__ nkeys_out) {
    __shared__ int32_t coarse[1024];
    __shared__ int whits[PRP_ROWS], wviol[PRP_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < a.nco; i += PRP_ROWS * 64) coarse[i] = a.uniq[(long long)i * a.stride];
    if (blockIdx.x == 0) plan_batch_init(a, threadIdx.x, PRP_ROWS * 64);
    const long long row = (long long)blockIdx.x * PRP_ROWS + wave;
    if (row < a.Q) {   // wave-uniform
        if (lane == 0) a.tauq[row] = KEY_NONE;   // running bound of the query
        if (a.prep_metric >= 0) prep_query(a, row, lane);
    }
    __syncthreads();
    bool hit = false;
    int viol = 0;
    probe_row<BUDGET, true>(z, z_stride, code, a.Q, H, key_mode, a.P, n_multi_rows, a.uniq, a.offsets, (uint32_t)a.nb, budget, keys_out,
                            nkeys_out, nullptr, nullptr, &a, coarse, &hit, &viol);
    const unsigned long long m = __ballot(hit);
    const unsigned long long v1 = __ballot(viol & PLAN_VIOL_COUNTER), v2 = __ballot(viol & PLAN_VIOL_CELLS);
    if (lane == 0) {
        whits[wave] = __popcll(m);
        wviol[wave] = (v1 ? PLAN_VIOL_COUNTER : 0) | (v2 ? PLAN_VIOL_CELLS : 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int h = 0, v = 0;
        for (int w = 0; w < PRP_ROWS; ++w) { h += whits[w]; v |= wviol[w]; }
        a.hits[blockIdx.x] = h | v;
    }
}

}  // namespace

// the launch of nlsh_query_batch_ranked (step.hip): `pa` = the PlanArgs of the scan call the keys go to (bucket_scan_args: BucketScanPrep::pa); the coarse
// table is sized here.  *blocks_out = workgroups launched = entries of `hits` the scan call's NLSH_PHASE_PLAN_REST sums.
int probe_ranked_plan_launch(const float *z, long long z_stride, const uint32_t *code, int H, int key_mode, long long n_multi_rows, int32_t budget,
                             PlanArgs &pa, int32_t *keys_out, int32_t *nkeys_out, hipStream_t stream, int *blocks_out) {
    NLSH_REQUIRE(pa.Q > 0 && pa.nb > 0 && pa.P >= 1 && pa.P <= 64 && H >= 1 && H <= NLSH_MAX_HASH_BITS && budget >= 0 && z_stride >= H,
                 NLSH_E_INVALID, "probe_ranked + lookup: Q=%lld n_buckets=%d n_probes=%d H=%d budget=%d", pa.Q, pa.nb, pa.P, H, (int)budget);
    NLSH_REQUIRE(z && code && keys_out && nkeys_out, NLSH_E_INVALID, "probe_ranked + lookup: null pointer");
    const long long grid = (pa.Q + PRP_ROWS - 1) / PRP_ROWS;
    NLSH_REQUIRE(grid <= 0x7FFFFFFF, NLSH_E_UNSUPPORTED, "probe_ranked + lookup: Q=%lld rows need more than 2^31 workgroups", pa.Q);
    plan_coarse(pa, 1024);
    if (budget > 0)
        hipLaunchKernelGGL(probe_ranked_plan_kernel<true>, dim3((unsigned)grid), dim3(PRP_ROWS * 64), 0, stream, z, z_stride, code, H, key_mode,
                           n_multi_rows, budget, pa, keys_out, nkeys_out);
    else
        hipLaunchKernelGGL(probe_ranked_plan_kernel<false>, dim3((unsigned)grid), dim3(PRP_ROWS * 64), 0, stream, z, z_stride, code, H, key_mode,
                           n_multi_rows, budget, pa, keys_out, nkeys_out);
    NLSH_CHECK_HIP(hipGetLastError());
    *blocks_out = (int)grid;
    return NLSH_OK;
}

}  // namespace nlsh

using namespace nlsh;

// the refusals both entry points make, before anything touches the device
static int probe_ranked_check(const float *z, int64_t z_stride, const uint32_t *code, int64_t n, int H, int key_mode, int n_probes,
                              const int32_t *keys_out, const int32_t *nkeys_out) {
    NLSH_REQUIRE(n >= 0, NLSH_E_INVALID, "probe_ranked: n=%lld", (long long)n);
    NLSH_REQUIRE(key_mode == NLSH_KEY_REF_INT16 || key_mode == NLSH_KEY_FULL, NLSH_E_INVALID, "probe_ranked: key_mode=%d", key_mode);
    NLSH_REQUIRE(H >= 1 && H <= NLSH_MAX_HASH_BITS, NLSH_E_UNSUPPORTED, "probe_ranked: H=%d not in [1, NLSH_MAX_HASH_BITS=%d]", H,
                 NLSH_MAX_HASH_BITS);
    NLSH_REQUIRE(n_probes >= 1 && n_probes <= NLSH_MAX_ENCODE_PROBES, NLSH_E_UNSUPPORTED,
                 "probe_ranked: n_probes=%d not in [1, NLSH_MAX_ENCODE_PROBES=%d]", n_probes, NLSH_MAX_ENCODE_PROBES);
    NLSH_REQUIRE(z_stride >= H, NLSH_E_INVALID, "probe_ranked: z_stride=%lld < H=%d", (long long)z_stride, H);
    NLSH_REQUIRE(n == 0 || (z && code && keys_out && nkeys_out), NLSH_E_INVALID, "probe_ranked: null pointer (z, code, keys_out and nkeys_out are required)");
    const int64_t grid = (n + PR_ROWS - 1) / PR_ROWS;
    NLSH_REQUIRE(grid <= 0x7FFFFFFF, NLSH_E_UNSUPPORTED, "probe_ranked: n=%lld rows need more than 2^31 workgroups", (long long)n);
    return NLSH_OK;
}

extern "C" int nlsh_probe_ranked(const float *z, int64_t z_stride, const uint32_t *code, int64_t n, int H, int key_mode, int n_probes,
                                 int64_t n_multi_rows, int32_t *keys_out, int32_t *nkeys_out, float *cost_out, nlsh_stream_t stream) {
    if (const int rc = probe_ranked_check(z, z_stride, code, n, H, key_mode, n_probes, keys_out, nkeys_out)) return rc;
    if (n == 0) return NLSH_OK;
    const int64_t grid = (n + PR_ROWS - 1) / PR_ROWS;
    hipLaunchKernelGGL(probe_ranked_kernel, dim3((unsigned)grid), dim3(PR_ROWS * 64), 0, (hipStream_t)stream, z, (long long)z_stride, code,
                       (long long)n, H, key_mode, n_probes, (long long)n_multi_rows, keys_out, nkeys_out, cost_out);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

extern "C" int nlsh_probe_ranked_budget(const float *z, int64_t z_stride, const uint32_t *code, int64_t n, int H, int key_mode,
                                        int n_probes, int64_t n_multi_rows, const int32_t *uniq_keys, const int32_t *offsets,
                                        int32_t n_buckets, int32_t budget, int32_t *keys_out, int32_t *nkeys_out, float *cost_out,
                                        int32_t *ncand_out, nlsh_stream_t stream) {
    NLSH_REQUIRE(budget >= 1, NLSH_E_INVALID, "probe_ranked_budget: budget=%d < 1", (int)budget);
    NLSH_REQUIRE(n_buckets >= 0, NLSH_E_INVALID, "probe_ranked_budget: n_buckets=%d", (int)n_buckets);
    NLSH_REQUIRE(n_buckets == 0 || (uniq_keys && offsets), NLSH_E_INVALID,
                 "probe_ranked_budget: null pointer (uniq_keys and offsets are required when n_buckets=%d > 0)", (int)n_buckets);
    if (const int rc = probe_ranked_check(z, z_stride, code, n, H, key_mode, n_probes, keys_out, nkeys_out)) return rc;
    if (n == 0) return NLSH_OK;
    const int64_t grid = (n + PR_ROWS - 1) / PR_ROWS;
    hipLaunchKernelGGL(probe_ranked_budget_kernel, dim3((unsigned)grid), dim3(PR_ROWS * 64), 0, (hipStream_t)stream, z, (long long)z_stride,
                       code, (long long)n, H, key_mode, n_probes, (long long)n_multi_rows, uniq_keys, offsets, (uint32_t)n_buckets, budget,
                       keys_out, nkeys_out, cost_out, ncand_out);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
