// nlsh_probe_bins: the n best bins of a row of M logits, best first (include/nlsh_hip.h).  The multi-probe of a
// Categorical (softmax-bin) hash: softmax is monotone, so the n most probable bins are the n largest logits.
//
// One wavefront per row, PB_ROWS rows per workgroup.  A bin's sort key is 64 bits, u(z) << 32 | ~b: larger = better logit, then
// smaller bin; keys of one row are distinct and never 0, so 0 stands for "none".
//   - the row is loaded coalesced (16 bytes per lane where base and stride allow) and kept in the wave's own LDS region as u(z),
//     TRANSPOSED: bin b = l + 64 j sits at word l * S + j, S = ceil(M / 64) | 1 (odd).  Lane l owns bins l, l + 64, ...: its column
//     is contiguous, and so is what the 64 lanes read when they scan one owner's column together (S odd: no bank conflicts either way);
//   - every lane keeps the best key of its column in a register; a round is one wave maximum (the winner), then the wave reads the
//     winning lane's column, one entry per lane, and a second wave maximum over the entries BELOW the winner gives that lane its next
//     best.  Nothing is marked in LDS: "below the last key taken" is the whole state, so the row image is written once and read only;
//   - the wave maximum is four DPP steps inside each row of 16 lanes and four lane reads across the rows: no LDS traffic;
//   - the kept keys stay in registers (slot p in lane p & 63, two named sets for p < 128) until the row is stored with plain vector
//     stores.  No register array is indexed at run time, there is no private segment and no atomic.
// The loop makes at most min(n_probes, M) rounds and every LDS index is bounded by 64 * S, whatever the bits of the logits are.
//
// nlsh_probe_bins_budget is the same loop (`bins_row<true>`) with probe_ranked.hip's per-row stop: each kept key's bucket size is looked
// up (`bucket_size`, probe_lookup.h) and the loop ends after the first key that brings the row's candidates to `budget`.
#include "common.h"
#include "probe_lookup.h"

namespace nlsh {
namespace {

constexpr int PB_ROWS = 4;   // rows (wavefronts) per workgroup

__host__ __device__ inline int pb_stride(int M) { return ((M + 63) >> 6) | 1; }   // words per lane column

// IEEE total order as unsigned: a negative pattern complemented, a non-negative one with its sign bit set
__device__ __forceinline__ uint32_t order_bits(uint32_t f) { return (f & 0x80000000u) ? ~f : f | 0x80000000u; }
__device__ __forceinline__ uint32_t float_bits(uint32_t u) { return (u & 0x80000000u) ? u ^ 0x80000000u : ~u; }

template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_max(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
    const unsigned long long o = (unsigned long long)hi << 32 | lo;
    return o > v ? o : v;
}
__device__ __forceinline__ unsigned long long read_lane64(unsigned long long v, int l) {   // l is a constant
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32 |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}
// maximum over the 64 lanes, the same value in every lane; every lane of the wave must be active
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    v = dpp_max<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    v = dpp_max<0x4E>(v);    // quad_perm [2, 3, 0, 1]: a quad agrees
    v = dpp_max<0x141>(v);   // row_half_mirror: 8 lanes agree
    v = dpp_max<0x140>(v);   // row_mirror: a row of 16 agrees
    const unsigned long long a = read_lane64(v, 0), b = read_lane64(v, 16), c = read_lane64(v, 32), d = read_lane64(v, 48);
    const unsigned long long ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

template <bool BUDGET>
__device__ __forceinline__ void bins_row(const float *__restrict__ logits, long long stride, long long n, int M, int P, long long n_multi_rows,
                                         const int32_t *__restrict__ uniq, const int32_t *__restrict__ offsets, uint32_t nb, int32_t budget,
                                         int32_t *__restrict__ keys_out, int32_t *__restrict__ nkeys_out, float *__restrict__ logit_out,
                                         int32_t *__restrict__ ncand_out) {
    extern __shared__ uint32_t pb_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * PB_ROWS + wave;
    if (row >= n) return;   // wave-uniform; the kernel has no workgroup barrier (a wave reads only the LDS words it wrote)
    const int S = pb_stride(M), nj = (M + 63) >> 6;
    uint32_t *col = pb_lds + wave * 64 * S;   // this wave's image: 64 columns of S words

    // ---- the row into LDS as order bits, bin b at (b & 63) * S + (b >> 6)
    const float *src = logits + row * stride;
    const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    const int M4 = vec ? M >> 2 : 0;
    for (int t = lane; t < M4; t += 64) {
        const float4 f = reinterpret_cast<const float4 *>(src)[t];
        const int b = 4 * t;   // b .. b + 3 share b >> 6 (b is a multiple of 4)
        uint32_t *dst = col + (b & 63) * S + (b >> 6);
        dst[0] = order_bits(__builtin_bit_cast(uint32_t, f.x));
        dst[S] = order_bits(__builtin_bit_cast(uint32_t, f.y));
        dst[2 * S] = order_bits(__builtin_bit_cast(uint32_t, f.z));
        dst[3 * S] = order_bits(__builtin_bit_cast(uint32_t, f.w));
    }
    for (int b = 4 * M4 + lane; b < M; b += 64) col[(b & 63) * S + (b >> 6)] = order_bits(__builtin_bit_cast(uint32_t, src[b]));
    // the wave's LDS operations complete in order; the fence keeps the compiler from moving the reads below above the writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- every lane's best key
    unsigned long long cur = 0ull;
    for (int j = 0; j < nj; ++j) {
        const int b = lane + 64 * j;
        if (b < M) {
            const unsigned long long k = (unsigned long long)col[lane * S + j] << 32 | (uint32_t)~b;
            cur = k > cur ? k : cur;
        }
    }

    int np = row < n_multi_rows ? (P < M ? P : M) : 1;
    unsigned long long o0 = 0ull, o1 = 0ull;   // kept keys: slot p in lane p & 63 of set p >> 6
    int cnt = 0;
    [[maybe_unused]] int32_t top = 0, cum = 0;
    if constexpr (BUDGET) {
        if (nb) {
            const uint32_t at = (uint32_t)lane * ((nb + 63u) >> 6);
            if (at < nb) top = uniq[at];
        }
    }
    for (int p = 0; p < np; ++p) {
        const unsigned long long g = wave_max(cur);
        if (g == 0ull) break;   // wave-uniform; cannot happen for p < M (the keys are distinct and non-zero)
        if (p < 64) {
            if (lane == p) o0 = g;
        } else if (lane == p - 64) {
            o1 = g;
        }
        cnt = p + 1;
        if constexpr (BUDGET) {
            if (nb) cum += bucket_size((int32_t)~(uint32_t)g, uniq, offsets, nb, top, lane);   // disjoint buckets: cum <= N < 2^31
            if (cum >= budget) break;   // wave-uniform: slot 0 is kept whatever its bucket holds
        }
        if (p + 1 == np) break;
        // the winner's next best: its column, one entry per lane, below g
        const int wl = __builtin_amdgcn_readfirstlane(__ffsll((long long)__ballot(cur == g)) - 1);
        const int b = wl + 64 * lane;
        unsigned long long k = 0ull;
        if (lane < nj && b < M) k = (unsigned long long)col[wl * S + lane] << 32 | (uint32_t)~b;
        if (k >= g) k = 0ull;
        const unsigned long long nxt = wave_max(k);
        if (lane == wl) cur = nxt;
    }

    // ---- store: kept slots, then zeros (-inf in logit_out)
    const long long base = row * (long long)P;
    for (int t = lane; t < P; t += 64) {
        const unsigned long long o = t < 64 ? o0 : o1;
        const bool kept = t < cnt;
        keys_out[base + t] = kept ? (int32_t)~(uint32_t)o : 0;
        if (logit_out) logit_out[base + t] = __builtin_bit_cast(float, kept ? float_bits((uint32_t)(o >> 32)) : 0xFF800000u);
    }
    if (lane == 0) {
        nkeys_out[row] = cnt;
        if constexpr (BUDGET) {
            if (ncand_out) ncand_out[row] = cum;
        }
    }
}

__global__ __launch_bounds__(PB_ROWS * 64) void probe_bins_kernel(const float *__restrict__ logits, long long stride, long long n, int M, int P,
                                                                  long long n_multi_rows, int32_t *__restrict__ keys_out,
                                                                  int32_t *__restrict__ nkeys_out, float *__restrict__ logit_out) {
    bins_row<false>(logits, stride, n, M, P, n_multi_rows, nullptr, nullptr, 0u, 0, keys_out, nkeys_out, logit_out, nullptr);
}

__global__ __launch_bounds__(PB_ROWS * 64) void probe_bins_budget_kernel(const float *__restrict__ logits, long long stride, long long n, int M,
                                                                         int P, long long n_multi_rows, const int32_t *__restrict__ uniq,
                                                                         const int32_t *__restrict__ offsets, uint32_t nb, int32_t budget,
                                                                         int32_t *__restrict__ keys_out, int32_t *__restrict__ nkeys_out,
                                                                         float *__restrict__ logit_out, int32_t *__restrict__ ncand_out) {
    bins_row<true>(logits, stride, n, M, P, n_multi_rows, uniq, offsets, nb, budget, keys_out, nkeys_out, logit_out, ncand_out);
}

}  // namespace
}  // namespace nlsh

using namespace nlsh;

// the refusals both entry points make, before anything touches the device
static int probe_bins_check(const float *logits, int64_t logits_stride, int64_t n, int M, int n_probes, const int32_t *keys_out,
                            const int32_t *nkeys_out) {
    NLSH_REQUIRE(n >= 0, NLSH_E_INVALID, "probe_bins: n=%lld", (long long)n);
    NLSH_REQUIRE(M >= 1 && M <= NLSH_MAX_BINS, NLSH_E_UNSUPPORTED, "probe_bins: M=%d not in [1, NLSH_MAX_BINS=%d]", M, NLSH_MAX_BINS);
    NLSH_REQUIRE(n_probes >= 1 && n_probes <= NLSH_MAX_ENCODE_PROBES, NLSH_E_UNSUPPORTED,
                 "probe_bins: n_probes=%d not in [1, NLSH_MAX_ENCODE_PROBES=%d]", n_probes, NLSH_MAX_ENCODE_PROBES);
    NLSH_REQUIRE(logits_stride >= M, NLSH_E_INVALID, "probe_bins: logits_stride=%lld < M=%d", (long long)logits_stride, M);
    NLSH_REQUIRE(n == 0 || (logits && keys_out && nkeys_out), NLSH_E_INVALID,
                 "probe_bins: null pointer (logits, keys_out and nkeys_out are required)");
    const int64_t grid = (n + PB_ROWS - 1) / PB_ROWS;
    NLSH_REQUIRE(grid <= 0x7FFFFFFF, NLSH_E_UNSUPPORTED, "probe_bins: n=%lld rows need more than 2^31 workgroups", (long long)n);
    return NLSH_OK;
}

// dynamic LDS of a workgroup: PB_ROWS images of 64 columns (at M = NLSH_MAX_BINS: 4 x 16,640 B, above the 64 KB a kernel may take unasked)
static int probe_bins_lds(const void *fn, int M, size_t *lds) {
    *lds = (size_t)PB_ROWS * 64 * pb_stride(M) * 4;
    if (*lds > 64 * 1024) NLSH_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds));
    return NLSH_OK;
}

extern "C" int nlsh_probe_bins(const float *logits, int64_t logits_stride, int64_t n, int M, int n_probes, int64_t n_multi_rows,
                               int32_t *keys_out, int32_t *nkeys_out, float *logit_out, nlsh_stream_t stream) {
    if (const int rc = probe_bins_check(logits, logits_stride, n, M, n_probes, keys_out, nkeys_out)) return rc;
    if (n == 0) return NLSH_OK;
    size_t lds;
    if (const int rc = probe_bins_lds(reinterpret_cast<const void *>(probe_bins_kernel), M, &lds)) return rc;
    const int64_t grid = (n + PB_ROWS - 1) / PB_ROWS;
    hipLaunchKernelGGL(probe_bins_kernel, dim3((unsigned)grid), dim3(PB_ROWS * 64), lds, (hipStream_t)stream, logits, (long long)logits_stride,
                       (long long)n, M, n_probes, (long long)n_multi_rows, keys_out, nkeys_out, logit_out);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

extern "C" int nlsh_probe_bins_budget(const float *logits, int64_t logits_stride, int64_t n, int M, int n_probes, int64_t n_multi_rows,
                                      const int32_t *uniq_keys, const int32_t *offsets, int32_t n_buckets, int32_t budget,
                                      int32_t *keys_out, int32_t *nkeys_out, float *logit_out, int32_t *ncand_out, nlsh_stream_t stream) {
    NLSH_REQUIRE(budget >= 1, NLSH_E_INVALID, "probe_bins_budget: budget=%d < 1", (int)budget);
    NLSH_REQUIRE(n_buckets >= 0, NLSH_E_INVALID, "probe_bins_budget: n_buckets=%d", (int)n_buckets);
    NLSH_REQUIRE(n_buckets == 0 || (uniq_keys && offsets), NLSH_E_INVALID,
                 "probe_bins_budget: null pointer (uniq_keys and offsets are required when n_buckets=%d > 0)", (int)n_buckets);
    if (const int rc = probe_bins_check(logits, logits_stride, n, M, n_probes, keys_out, nkeys_out)) return rc;
    if (n == 0) return NLSH_OK;
    size_t lds;
    if (const int rc = probe_bins_lds(reinterpret_cast<const void *>(probe_bins_budget_kernel), M, &lds)) return rc;
    const int64_t grid = (n + PB_ROWS - 1) / PB_ROWS;
    hipLaunchKernelGGL(probe_bins_budget_kernel, dim3((unsigned)grid), dim3(PB_ROWS * 64), lds, (hipStream_t)stream, logits,
                       (long long)logits_stride, (long long)n, M, n_probes, (long long)n_multi_rows, uniq_keys, offsets, (uint32_t)n_buckets,
                       budget, keys_out, nkeys_out, logit_out, ncand_out);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
