// nlsh_merge_topk_unique: the top-k merge of a multi-table index.  G lists per query, one per hash table over the SAME corpus, so one
// row can sit in several of them -- with the same 64-bit sort key in each, because the tiled schedule's distance of a (query, row) pair
// is a function of the two vectors alone.  Equal keys of different lists are one candidate; the output is the k
// smallest DISTINCT keys.  nlsh_merge_topk (scan_topk.hip) is the merge of DISJOINT lists and keeps a repeated key twice.
//
// One wavefront per query, as in merge_shards_kernel, and the same merge by selection (merge_round / merge_round_wide, scan_common.h).
// What is new happens before a key reaches the selection:
//   1. the query's G x k keys are staged in the wave's own LDS (8 G k bytes), read from global memory once, coalesced;
//   2. a key of list g is DEAD when a lower-numbered list holds an equal key: one lower-bound search per (key, lower list) in the
//      staged copy -- the lists are ascending and ~0-padded, so that is ceil(log2 k) + 2 LDS reads -- and a dead key enters the
//      selection as KEY_NONE.  Of the copies of a key exactly one survives, the one in the lowest-numbered list.
// Marking BEFORE selecting is what keeps the list full: selecting first and dropping repeats afterwards would return fewer than k keys
// although k distinct ones exist.  The staged copy is never written after step 1 (the searches of later rounds need it sorted): the
// mark lives in the register that feeds the selection.
//
// LDS: per wave 8 (G k + S) bytes, S = 64 (k <= 64) or 256 keys of selection scratch, sized per launch (dynamic), so a launch pays for
// its own G and k only.  k <= 64 runs four waves per workgroup: at most 4 x 8.5 KB = 34 KB at G = 16, k = 64.  k > 64 runs ONE wave
// per workgroup: at G = 16, k = 256 a wave stages 32 KB + 2 KB of scratch, four such workgroups fit the CU's 160 KB -- one wave per
// SIMD -- and every smaller G x k fits proportionally more (G = 4, k = 100: 5.1 KB per wave, the register file is the limit again).
// No atomics, no global scratch, no barrier (a wave only ever reads what it staged itself), every global load is consumed before the
// wave ends.
#include "scan_common.h"

namespace nlsh {

// Does the ascending, ~0-padded list L[0, k) hold `key` (a real key)?  Branch-free lower bound: every key before `lo` is below `key`
// and the bound lies in [lo, lo + n]; the trip count depends on k alone, so a wave's lanes stay together.  The loop ends with the bound
// at lo or lo + 1; keys of a list are distinct, so L[lo + 1] == key implies L[lo] < key and both places can be compared outright.
__device__ __forceinline__ bool list_holds(const uint64_t *L, int k, uint64_t key) {
    int lo = 0, n = k;
    while (n > 1) {
        const int half = n >> 1;
        lo = L[lo + half] < key ? lo + half : lo;   // lo + half <= lo + n - 1 <= k - 1
        n -= half;
    }
    const int up = lo + 1 < k ? lo + 1 : lo;
    return L[lo] == key || L[up] == key;
}

// `key` of list g, or KEY_NONE when one of the lists 0 .. g - 1 holds it too.  g may differ between the lanes (k <= 64: several lists
// share a register); lanes without a key pass g = 0.
__device__ __forceinline__ uint64_t drop_repeated(const uint64_t *staged, int k, int g, uint64_t key) {
    bool dead = key == KEY_NONE;
    for (int h = 0; h < g; ++h)
        if (!dead) dead = list_holds(staged + h * k, k, key);
    return dead ? KEY_NONE : key;
}

// KPL = keys per lane of a k-key list (1: k <= 64; 2, 3, 4: k <= 128, 192, 256); WPB = waves (queries) per workgroup.
// Dynamic LDS: WPB x (G k + S) keys, S = 64 for KPL 1, NLSH_MAX_K_TILED otherwise.
template <int KPL, int WPB>
__global__ __launch_bounds__(64 * WPB) void merge_unique_kernel(const uint64_t *keys_in, long long row_stride, int G, long long Q, int k,
                                                                 const int32_t *ncand_in, float *out_dist, int32_t *out_idx,
                                                                 uint64_t *out_keys, int32_t *out_ncand) {
    extern __shared__ uint64_t merge_unique_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * WPB + w;
    if (q >= Q) return;
    constexpr int S = KPL == 1 ? 64 : NLSH_MAX_K_TILED;
    const int n = G * k;                                        // <= NLSH_MAX_TABLES * NLSH_MAX_K_TILED = 4096
    uint64_t *staged = merge_unique_lds + (size_t)w * (n + S), *sc = staged + n;

    // 1. stage: list g of query q is keys_in[(g Q + q) row_stride + 0 .. k), g < G, q < Q, k <= row_stride
    if constexpr (KPL == 1) {
        for (int i = lane; i < n; i += 64) {
            const int g = i / k, e = i - g * k;
            staged[i] = keys_in[((long long)g * Q + q) * row_stride + e];
        }
    } else {
        for (int g = 0; g < G; ++g) {
            const uint64_t *row = keys_in + ((long long)g * Q + q) * row_stride;
            for (int e = lane; e < k; e += 64) staged[g * k + e] = row[e];
        }
    }
    __builtin_amdgcn_wave_barrier();   // the wave's LDS writes precede its reads below (LDS operations of a wave complete in order)

    // 2. + selection: merge_shards_kernel's rounds, every key passed through drop_repeated on its way from the staged copy
    if constexpr (KPL == 1) {
        const int R = 64 / k, r = lane / k, e = lane - r * k;
        uint64_t carry = KEY_NONE;
        for (int base = 0; base < G; base += 3 * R) {
            uint64_t key[4];
            key[0] = carry;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int g = base + s * R + r;
                const bool have = r < R && g < G;
                key[s + 1] = drop_repeated(staged, k, have ? g : 0, have ? staged[g * k + e] : KEY_NONE);
            }
            carry = merge_round<4>(key, k, lane, sc);
        }
        merge_finish(carry, k, lane, out_dist, out_idx, out_keys, q);
    } else {
        constexpr int NL = KPL == 2 ? 3 : 1;
        uint64_t carry[KPL];
#pragma unroll
        for (int i = 0; i < KPL; ++i) carry[i] = KEY_NONE;
        for (int base = 0; base < G; base += NL) {
            uint64_t key[KPL * (1 + NL)];
#pragma unroll
            for (int i = 0; i < KPL; ++i) key[i] = carry[i];
#pragma unroll
            for (int s = 0; s < NL; ++s) {
                const int g = base + s;   // wave-uniform
#pragma unroll
                for (int i = 0; i < KPL; ++i) {
                    const bool have = g < G && i * 64 + lane < k;
                    key[KPL * (1 + s) + i] = drop_repeated(staged, k, have ? g : 0, have ? staged[g * k + i * 64 + lane] : KEY_NONE);
                }
            }
            merge_round_wide(key, carry, k, lane, sc);
        }
        merge_finish_wide(carry, sc, k, lane, out_dist, out_idx, out_keys, q);
    }

    // candidate counts: the SUM over the lists (scored pairs, a row found by two tables counts twice), nlsh_merge_topk's three forms
    if (out_ncand && (ncand_in || row_stride > k)) {
        int32_t nc = 0;
        for (int g = lane; g < G; g += 64) nc += ncand_in ? ncand_in[(long long)g * Q + q] : (int32_t)keys_in[((long long)g * Q + q) * row_stride + k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nc += __shfl_xor(nc, m);
        if (lane == 0) out_ncand[q] = nc;
    }
}

}  // namespace nlsh

using namespace nlsh;

extern "C" int nlsh_merge_topk_unique(const uint64_t *keys_in, int64_t row_stride, int G, int64_t Q, int k, const int32_t *ncand_in,
                                      float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand, nlsh_stream_t stream) {
    NLSH_REQUIRE(G >= 1, NLSH_E_INVALID, "merge_topk_unique: G=%d, at least one list per query", G);
    NLSH_REQUIRE(G <= NLSH_MAX_TABLES, NLSH_E_UNSUPPORTED, "merge_topk_unique: G=%d, at most NLSH_MAX_TABLES = %d lists per query", G,
                 NLSH_MAX_TABLES);
    NLSH_REQUIRE(k >= 1, NLSH_E_INVALID, "merge_topk_unique: k=%d", k);
    NLSH_REQUIRE(k <= NLSH_MAX_K_TILED, NLSH_E_UNSUPPORTED, "merge_topk_unique: k=%d, at most NLSH_MAX_K_TILED = %d", k, NLSH_MAX_K_TILED);
    NLSH_REQUIRE(row_stride >= k, NLSH_E_INVALID, "merge_topk_unique: row_stride=%lld is less than k=%d", (long long)row_stride, k);
    NLSH_REQUIRE(Q >= 0, NLSH_E_INVALID, "merge_topk_unique: Q=%lld", (long long)Q);
    if (Q == 0) return NLSH_OK;
    NLSH_REQUIRE(keys_in, NLSH_E_INVALID, "merge_topk_unique: keys_in is null");
    NLSH_REQUIRE(out_dist, NLSH_E_INVALID, "merge_topk_unique: out_dist is null");
    NLSH_REQUIRE(out_idx, NLSH_E_INVALID, "merge_topk_unique: out_idx is null");
    NLSH_REQUIRE(((uintptr_t)keys_in & 7) == 0 && ((uintptr_t)out_keys & 7) == 0, NLSH_E_INVALID,
                 "merge_topk_unique: keys_in and out_keys must be 8-byte aligned");
    const bool wide = k > NLSH_MAX_K;
    const int wpb = wide ? 1 : 4;
    const int64_t blocks = (Q + wpb - 1) / wpb;
    NLSH_REQUIRE(blocks <= 0x7FFFFFFFll, NLSH_E_UNSUPPORTED, "merge_topk_unique: Q=%lld needs %lld workgroups, at most 2^31 - 1 per call",
                 (long long)Q, (long long)blocks);
    const size_t lds = (size_t)wpb * ((size_t)G * k + (wide ? NLSH_MAX_K_TILED : 64)) * sizeof(uint64_t);   // <= 34816 bytes
    const void *fn = (const void *)merge_unique_kernel<1, 4>;
    if (k > 192) fn = (const void *)merge_unique_kernel<4, 1>;
    else if (k > 128) fn = (const void *)merge_unique_kernel<3, 1>;
    else if (wide) fn = (const void *)merge_unique_kernel<2, 1>;
    long long rs = row_stride, q64 = Q;
    void *argv[] = {&keys_in, &rs, &G, &q64, &k, &ncand_in, &out_dist, &out_idx, &out_keys, &out_ncand};
    NLSH_CHECK_HIP(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(64 * wpb), argv, lds, (hipStream_t)stream));
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
