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
#include "common.h"

namespace nlsh {
namespace {

constexpr int PR_ROWS = 4;          // rows (wavefronts) per workgroup
constexpr uint32_t PR_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t lane_read(uint32_t v, int l) {   // l is wave-uniform
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(l));
}
__device__ __forceinline__ uint32_t add_bits(uint32_t a, uint32_t b) {   // one fp32 add on bit patterns
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b));
}
__device__ __forceinline__ int32_t key_of(uint32_t code, int key_mode) {
    return key_mode == NLSH_KEY_REF_INT16 ? (int32_t)(int16_t)(uint16_t)(code & 0xFFFFu) : (int32_t)code;
}

__global__ __launch_bounds__(PR_ROWS * 64) void probe_ranked_kernel(const float *__restrict__ z, long long z_stride,
                                                                    const uint32_t *__restrict__ code, long long n, int H, int key_mode,
                                                                    int P, long long n_multi_rows, int32_t *__restrict__ keys_out,
                                                                    int32_t *__restrict__ nkeys_out, float *__restrict__ cost_out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * PR_ROWS + (threadIdx.x >> 6);
    if (row >= n) return;   // wave-uniform

    // ---- costs, sorted by (bit pattern, bit index): lanes past H hold a sentinel above every cleared-sign pattern
    uint32_t c = PR_NONE;
    if (lane < H) c = __builtin_bit_cast(uint32_t, z[row * z_stride + lane]) & 0x7FFFFFFFu;
    const uint32_t hard = code[row];
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
    const int np = row < n_multi_rows ? P : 1;
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
        if (p < 64) {
            if (lane == p) { o_code0 = hard ^ flip; o_cost0 = t; }
        } else if (lane == p - 64) {
            o_code1 = hard ^ flip; o_cost1 = t;
        }
        cnt = p + 1;
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
    if (key_mode == NLSH_KEY_REF_INT16 && H > 16) {
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
        }
    }
    if (lane == 0) nkeys_out[row] = nk;
}

}  // namespace
}  // namespace nlsh

using namespace nlsh;

extern "C" int nlsh_probe_ranked(const float *z, int64_t z_stride, const uint32_t *code, int64_t n, int H, int key_mode, int n_probes,
                                 int64_t n_multi_rows, int32_t *keys_out, int32_t *nkeys_out, float *cost_out, nlsh_stream_t stream) {
    NLSH_REQUIRE(n >= 0, NLSH_E_INVALID, "probe_ranked: n=%lld", (long long)n);
    NLSH_REQUIRE(key_mode == NLSH_KEY_REF_INT16 || key_mode == NLSH_KEY_FULL, NLSH_E_INVALID, "probe_ranked: key_mode=%d", key_mode);
    NLSH_REQUIRE(H >= 1 && H <= NLSH_MAX_HASH_BITS, NLSH_E_UNSUPPORTED, "probe_ranked: H=%d not in [1, NLSH_MAX_HASH_BITS=%d]", H,
                 NLSH_MAX_HASH_BITS);
    NLSH_REQUIRE(n_probes >= 1 && n_probes <= NLSH_MAX_ENCODE_PROBES, NLSH_E_UNSUPPORTED,
                 "probe_ranked: n_probes=%d not in [1, NLSH_MAX_ENCODE_PROBES=%d]", n_probes, NLSH_MAX_ENCODE_PROBES);
    NLSH_REQUIRE(z_stride >= H, NLSH_E_INVALID, "probe_ranked: z_stride=%lld < H=%d", (long long)z_stride, H);
    NLSH_REQUIRE(n == 0 || (z && code && keys_out && nkeys_out), NLSH_E_INVALID, "probe_ranked: null pointer (z, code, keys_out and nkeys_out are required)");
    if (n == 0) return NLSH_OK;
    const int64_t grid = (n + PR_ROWS - 1) / PR_ROWS;
    NLSH_REQUIRE(grid <= 0x7FFFFFFF, NLSH_E_UNSUPPORTED, "probe_ranked: n=%lld rows need more than 2^31 workgroups", (long long)n);
    hipLaunchKernelGGL(probe_ranked_kernel, dim3((unsigned)grid), dim3(PR_ROWS * 64), 0, (hipStream_t)stream, z, (long long)z_stride, code,
                       (long long)n, H, key_mode, n_probes, (long long)n_multi_rows, keys_out, nkeys_out, cost_out);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
