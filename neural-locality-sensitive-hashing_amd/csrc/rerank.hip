// nlsh_rerank_topk: the second stage of a two-stage query.  Stage one -- a scan over a compressed or folded index --
// over-fetches kc candidates per query; this kernel scores those kc rows on the ORIGINAL float32 rows of a refine store (id order: row
// id - id_base) and keeps the k best.  The distance of a (query, row) pair has the bits the tiled float32 scan gives the same pair: one
// k-ascending fmaf chain per pair, the exact L2 form, the scan's epilogue (sqrt_rn_unscaled behind its 2^-96 guard, finish_distance
// otherwise) and the scan's key -- prep_query, finish_distance, sqrt_rn_unscaled, make_key and the selection are the scan's own code.
//
// One wavefront per query, up to four queries per workgroup, no barrier between waves (a wave only reads LDS it wrote itself).
//   query       wave-uniform: prep_query writes the padded (L2: -eps) / pre-normalised (cosine) copy into the wave's LDS once; the chain
//               reads it as broadcast ds_read_b128, never as one VGPR copy per lane.
//   candidates  64 at a time, lane l owns candidate l.  Its row is NOT walked by the lane (64 lanes x 64 different rows = 64 lines per
//               load instruction): the wave loads whole rows cooperatively -- 8 consecutive lanes take 128 consecutive bytes of one row,
//               16 bytes each -- one stage of RR_KB chunks ahead of the arithmetic, and writes them into a per-wave tile in the tiled
//               scan's transposed layout (row pitch RR_RS = 9 float4 slots, odd: the lane-owns-row ds_read_b128 is conflict-free).
//   ids         checked BEFORE any address is formed: -1 is padding, an id outside [id_base, id_base + n_rows) is dropped, its row is
//               never read, and the smallest query that held one is left in first_bad (one unsigned atomic minimum per such wave).
//   selection   kc <= 256 keys are at most 4 per lane: merge_round / merge_round_wide pick the k best, merge_finish(_wide) orders them.
// No workspace, no scratch memory, no atomics but the first_bad minimum.  The store may be device memory or pinned host memory mapped for
// the device: the kernel is the same, the entry point checks the mapping (the range check nlsh_query_batch_host makes of its block).
#include "scan_common.h"
#include "scan_plan.h"

namespace nlsh {

constexpr int RR_KB = 8;    // 16-byte chunks of every row per stage
constexpr int RR_RS = 9;    // tile row pitch in float4 slots
constexpr int RR_TILE_BYTES = 64 * RR_RS * 16;

struct RerankArgs {
    const float *queries; long long q_stride; long long Q; int d, d4p;
    const float4 *store; long long stride4; long long n_rows; int id_base;
    const float *inv_norm;
    const int32_t *cand; long long cand_stride; int kc, k;
    float *out_dist; int32_t *out_idx; uint64_t *out_keys; int32_t *out_count; int32_t *first_bad;
    int wave_lds;   // bytes of LDS per wave: tile | query copy (16 d4p) | selection scratch
};

// one element of the chain, in the tiled scan's operation order
template <int METRIC>
__device__ __forceinline__ float chain_step(float acc, float qv, float cv) {
    if (METRIC == NLSH_METRIC_COSINE) return fmaf(qv, cv, acc);
    const float t = (qv - cv) + 1e-6f;   // F.pairwise_distance: (x1 - x2) + eps
    return fmaf(t, t, acc);
}

// finish_distance<NLSH_METRIC_COSINE> -- 1.0f - acc * inv_norm -- in the instruction form every tiled scan kernel executes it: the compiler
// pairs the scan's tiles and emits v_pk_mul_f32 with the NEGATE modifier on the accumulator, then v_pk_add_f32 of 1.0 (packed math has no
// subtract).  On every finite or infinite product that is finish_distance's value, bit for bit; the forms part only in the SIGN of a NaN
// result, which the modifier flips and a v_sub_f32 keeps -- and the sign of a NaN distance is the top bit of its sort key, so it decides
// whether a row with a NaN sorts in front of every real distance or behind them.  Compiled from finish_distance itself this kernel got
// v_mul_f32 + v_sub_f32 and ordered such rows at the other end from the scan (tests/test_gpu_refine.py holds the order to the twin's).
__device__ __forceinline__ float cosine_finish_as_scanned(float acc, float inv_norm) {
    float dist;
    asm("v_mul_f32_e64 %0, %1, -%2\n\tv_add_f32_e32 %0, 1.0, %0" : "=&v"(dist) : "v"(inv_norm), "v"(acc));
    return dist;
}

template <int METRIC, bool WIDE>
__global__ __launch_bounds__(256) void rerank_kernel(RerankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rerank_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * (blockDim.x >> 6) + w;
    if (q >= a.Q) return;
    constexpr int NG = WIDE ? 4 : 1;   // candidate groups of 64 = keys per lane
    unsigned char *base = rerank_lds + (size_t)w * a.wave_lds;
    float4 *tile = reinterpret_cast<float4 *>(base);
    float *qlds = reinterpret_cast<float *>(base + RR_TILE_BYTES);
    uint64_t *sc = reinterpret_cast<uint64_t *>(qlds + a.d4p * 4);

    PlanArgs pa = {};
    pa.queries = a.queries; pa.q_stride = a.q_stride; pa.qpad = qlds; pa.qpad_stride = 0;
    pa.d = a.d; pa.d4p = a.d4p; pa.prep_metric = METRIC;
    prep_query(pa, q, lane);
    __builtin_amdgcn_wave_barrier();   // the wave's LDS writes precede its reads below (LDS operations of a wave complete in order)

    const int d = a.d, d4p = a.d4p;
    const int ch = lane & 7, sub = lane >> 3;
    uint64_t key[NG];
    int n_valid = 0;
    bool bad = false;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        key[g] = KEY_NONE;
        if (g * 64 >= a.kc) continue;   // wave-uniform
        const int c = g * 64 + lane;
        const int32_t id = c < a.kc ? a.cand[q * a.cand_stride + c] : -1;
        const long long rel = (long long)id - a.id_base;
        const bool valid = id != -1 && rel >= 0 && rel < a.n_rows;
        bad = bad || (id != -1 && !valid);
        const unsigned long long vmask = __ballot(valid);
        if (vmask == 0ull) continue;    // wave-uniform: nothing to read
        n_valid += __popcll(vmask);
        const uint32_t rel32 = valid ? (uint32_t)rel : 0u;   // id and id_base are int32: a valid rel is below 2^32
        const float inv = (METRIC == NLSH_METRIC_COSINE && valid) ? a.inv_norm[rel] : 0.0f;
        // rows the lane helps to load: row i * 8 + sub, chunk ch of every stage
        const float4 *rp[RR_KB];
#pragma unroll
        for (int i = 0; i < RR_KB; ++i) {
            const int row = i * 8 + sub;
            const uint32_t r = (uint32_t)__shfl((int)rel32, row);
            rp[i] = ((vmask >> row) & 1ull) ? a.store + (long long)r * a.stride4 + ch : nullptr;   // an invalid id forms no address
        }
        float4 regs[RR_KB];
#pragma unroll
        for (int i = 0; i < RR_KB; ++i) regs[i] = (rp[i] && ch < d4p) ? rp[i][0] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float acc = 0.0f;
        for (int c0 = 0; c0 < d4p; c0 += RR_KB) {
#pragma unroll
            for (int i = 0; i < RR_KB; ++i) tile[(i * 8 + sub) * RR_RS + ch] = regs[i];
            __builtin_amdgcn_wave_barrier();
            const int cn = c0 + RR_KB;
            if (cn < d4p) {             // the next stage's rows, requested before this stage's arithmetic
#pragma unroll
                for (int i = 0; i < RR_KB; ++i) regs[i] = (rp[i] && cn + ch < d4p) ? rp[i][cn] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            const int nchunk = d4p - c0 < RR_KB ? d4p - c0 : RR_KB;
            for (int cc = 0; cc < nchunk; ++cc) {
                const float4 r = tile[lane * RR_RS + cc];
                const float4 qv = reinterpret_cast<const float4 *>(qlds)[c0 + cc];
                const int e0 = 4 * (c0 + cc);
                if (e0 + 4 <= d) {      // wave-uniform
                    acc = chain_step<METRIC>(acc, qv.x, r.x);
                    acc = chain_step<METRIC>(acc, qv.y, r.y);
                    acc = chain_step<METRIC>(acc, qv.z, r.z);
                    acc = chain_step<METRIC>(acc, qv.w, r.w);
                } else {                // the row's last chunk: the chain ends at d, whatever the pitch padding holds
                    acc = chain_step<METRIC>(acc, qv.x, r.x);
                    if (e0 + 1 < d) acc = chain_step<METRIC>(acc, qv.y, r.y);
                    if (e0 + 2 < d) acc = chain_step<METRIC>(acc, qv.z, r.z);
                }
            }
            __builtin_amdgcn_wave_barrier();   // the tile is rewritten by the next stage
        }
        // the tiled scan's epilogue: one wave-uniform guard per list, square roots without the range scaling behind it
        uint64_t kk;
        bool lean = METRIC != NLSH_METRIC_COSINE;
        if (lean) lean = __ballot(valid && !(acc >= 0x1p-96f)) == 0ull;   // a NaN fails the comparison
        if (lean) {
            const float dist = sqrt_rn_unscaled(acc);
            kk = ((uint64_t)(__builtin_bit_cast(uint32_t, dist) | 0x80000000u) << 32) | (uint32_t)id;   // == make_key for dist >= +0
        } else if (METRIC == NLSH_METRIC_COSINE) {
            kk = make_key(cosine_finish_as_scanned(acc, inv), id);
        } else {
            kk = make_key(finish_distance<METRIC>(acc, inv), id);
        }
        key[g] = valid ? kk : KEY_NONE;
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicMin(reinterpret_cast<unsigned int *>(a.first_bad), (unsigned int)q);
    if (a.out_count && lane == 0) a.out_count[q] = n_valid < a.k ? n_valid : a.k;
    if constexpr (WIDE) {
        uint64_t carry[NG];
        merge_round_wide<NG, NG>(key, carry, a.k, lane, sc);
        merge_finish_wide<NG>(carry, sc, a.k, lane, a.out_dist, a.out_idx, a.out_keys, q);
    } else {
        const uint64_t carry = merge_round<1>(key, a.k, lane, sc);
        merge_finish(carry, a.k, lane, a.out_dist, a.out_idx, a.out_keys, q);
    }
}

// `store` as the device sees it: host memory mapped for the device, first and last byte (nlsh_query_batch_host's check of its block)
static int store_mapped(const float *store, size_t n_floats, const float **mapped) {
    *mapped = nullptr;
    for (const float *p : {store, store + (n_floats - 1)}) {
        hipPointerAttribute_t at;
        const hipError_t e = hipPointerGetAttributes(&at, p);
        if (e != hipSuccess) (void)hipGetLastError();     // memory the runtime does not know: an answer, not a failure to keep
        NLSH_REQUIRE(e == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer != nullptr, NLSH_E_INVALID,
                     "rerank_topk: store_on_host=1 but store is not host memory mapped for the device (hipHostMalloc / hipHostRegister; a "
                     "device pointer is refused)");
        if (!*mapped) *mapped = (const float *)at.devicePointer;
    }
    return NLSH_OK;
}

}  // namespace nlsh

using namespace nlsh;

extern "C" int nlsh_rerank_topk(const float *queries, int64_t q_stride, int64_t Q, int d, const float *store, int64_t store_stride,
                                int64_t n_rows, int32_t id_base, int store_on_host, const float *store_inv_norm, const int32_t *cand,
                                int64_t cand_stride, int kc, int k, int metric, float *out_dist, int32_t *out_idx, uint64_t *out_keys,
                                int32_t *out_count, int32_t *first_bad, nlsh_stream_t stream) {
    NLSH_REQUIRE(k >= 1 && k <= kc && kc <= NLSH_MAX_K_TILED, NLSH_E_UNSUPPORTED,
                 "rerank_topk: k=%d, kc=%d, need 1 <= k <= kc <= NLSH_MAX_K_TILED = %d", k, kc, NLSH_MAX_K_TILED);
    NLSH_REQUIRE(d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_UNSUPPORTED, "rerank_topk: d=%d, need 1 <= d <= NLSH_MAX_DIM = %d", d, NLSH_MAX_DIM);
    NLSH_REQUIRE(metric != NLSH_METRIC_L2_EPS_FOLDED, NLSH_E_INVALID,
                 "rerank_topk: metric NLSH_METRIC_L2_EPS_FOLDED: the re-rank is the exact L2 form (pass NLSH_METRIC_L2_EPS)");
    NLSH_REQUIRE(metric == NLSH_METRIC_L2_EPS || metric == NLSH_METRIC_COSINE, NLSH_E_INVALID, "rerank_topk: metric=%d", metric);
    NLSH_REQUIRE(store_stride >= d && store_stride % 4 == 0, NLSH_E_INVALID,
                 "rerank_topk: store_stride=%lld must be a multiple of 4 floats and at least d=%d", (long long)store_stride, d);
    NLSH_REQUIRE(((uintptr_t)store & 15) == 0, NLSH_E_INVALID, "rerank_topk: store must be 16-byte aligned");
    NLSH_REQUIRE(cand_stride >= kc, NLSH_E_INVALID, "rerank_topk: cand_stride=%lld is less than kc=%d", (long long)cand_stride, kc);
    NLSH_REQUIRE(n_rows >= 0 && n_rows <= (1ll << 32), NLSH_E_INVALID, "rerank_topk: n_rows=%lld (row ids are int32)", (long long)n_rows);
    NLSH_REQUIRE(Q >= 0 && Q < (1ll << 31), NLSH_E_INVALID, "rerank_topk: Q=%lld", (long long)Q);
    NLSH_REQUIRE(store_on_host == 0 || store_on_host == 1, NLSH_E_INVALID, "rerank_topk: store_on_host=%d", store_on_host);
    NLSH_REQUIRE(metric != NLSH_METRIC_COSINE || store_inv_norm, NLSH_E_INVALID, "rerank_topk: cosine needs store_inv_norm");
    NLSH_REQUIRE(first_bad, NLSH_E_INVALID, "rerank_topk: first_bad is null");
    if (Q == 0) return NLSH_OK;
    NLSH_REQUIRE(queries, NLSH_E_INVALID, "rerank_topk: queries is null");
    NLSH_REQUIRE(q_stride >= d, NLSH_E_INVALID, "rerank_topk: q_stride=%lld is less than d=%d", (long long)q_stride, d);
    NLSH_REQUIRE(store || n_rows == 0, NLSH_E_INVALID, "rerank_topk: store is null");
    NLSH_REQUIRE(cand, NLSH_E_INVALID, "rerank_topk: cand is null");
    NLSH_REQUIRE(out_dist, NLSH_E_INVALID, "rerank_topk: out_dist is null");
    NLSH_REQUIRE(out_idx, NLSH_E_INVALID, "rerank_topk: out_idx is null");
    NLSH_REQUIRE(((uintptr_t)out_keys & 7) == 0, NLSH_E_INVALID, "rerank_topk: out_keys must be 8-byte aligned");
    if (store_on_host && n_rows > 0) {
        const float *mapped = nullptr;
        if (const int mrc = store_mapped(store, (size_t)n_rows * (size_t)store_stride, &mapped)) return mrc;
        store = mapped;
    }
    RerankArgs a = {};
    a.queries = queries; a.q_stride = q_stride; a.Q = Q; a.d = d; a.d4p = (d + 3) / 4;
    a.store = reinterpret_cast<const float4 *>(store); a.stride4 = store_stride / 4; a.n_rows = n_rows; a.id_base = id_base;
    a.inv_norm = store_inv_norm;
    a.cand = cand; a.cand_stride = cand_stride; a.kc = kc; a.k = k;
    a.out_dist = out_dist; a.out_idx = out_idx; a.out_keys = out_keys; a.out_count = out_count; a.first_bad = first_bad;
    const bool wide = kc > NLSH_MAX_K;
    a.wave_lds = RR_TILE_BYTES + a.d4p * 16 + (wide ? NLSH_MAX_K_TILED : 64) * (int)sizeof(uint64_t);   // <= 15360 bytes
    const int wpb = 4 * a.wave_lds <= 48 * 1024 ? 4 : 2;      // queries (waves) per workgroup
    const int64_t blocks = (Q + wpb - 1) / wpb;
    const void *fn;
    if (metric == NLSH_METRIC_COSINE) fn = wide ? (const void *)rerank_kernel<NLSH_METRIC_COSINE, true> : (const void *)rerank_kernel<NLSH_METRIC_COSINE, false>;
    else fn = wide ? (const void *)rerank_kernel<NLSH_METRIC_L2_EPS, true> : (const void *)rerank_kernel<NLSH_METRIC_L2_EPS, false>;
    hipStream_t s = (hipStream_t)stream;
    NLSH_CHECK_HIP(hipMemsetAsync(first_bad, 0xFF, sizeof(int32_t), s));   // -1 = no offending query; as unsigned, the minimum's identity
    void *argv[] = {&a};
    NLSH_CHECK_HIP(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(64 * wpb), argv, (size_t)wpb * a.wave_lds, s));
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
