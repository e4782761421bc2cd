// sq8 corpus storage, the row side (included by build_csr.hip behind its row helpers, which this is built from): the codec that
// build_csr.hip's row kernels encode and decode an sq8 index by, and training the per-dimension quantiser.
//
// THE RULE (include/nlsh_hip.h states it; tests hold the kernels to it bit for bit).  A quantiser is lo[d], step[d], float32, step > 0.
//   decode  deq(c, j) = float(c) * step[j] + lo[j]                       two roundings, never a fused multiply-add
//   encode  t = (x - lo[j]) / step[j]; code = clamp(rint(t), 0, 255)     IEEE subtract, correctly rounded divide, ties to even; a finite
//           value out of range saturates (the row is counted), a NaN or an infinity refuses the row (first_bad)
//   train   lo = min + 0.0f, hi = max + 0.0f (either zero becomes +0), step = (hi - lo) / 255.0f, or 1.0f where hi == lo
// Columns >= d of the pitch are code 0, and the quantiser arrays the kernels read are padded to the pitch with lo = 0, step = 1.
// The library is built with -ffp-contract=off: every expression below is the separate IEEE operations it spells.
#pragma once

namespace nlsh {

__device__ __forceinline__ float4 sq8_decode4(uint32_t w, const float4 lo, const float4 st) {
    const float4 c = unpack_chunk<NLSH_STORE_U8>(w);
    return make_float4(c.x * st.x + lo.x, c.y * st.y + lo.y, c.z * st.z + lo.z, c.w * st.w + lo.w);
}

__device__ __forceinline__ uint32_t sq8_code(float x, float lo, float st, bool live, bool &bad, bool &clamped) {
    const float r = rintf((x - lo) / st);             // the default rounding mode: half to even
    bad = bad || (live && !__builtin_isfinite(x));
    clamped = clamped || (live && (r < 0.0f || r > 255.0f));
    return live ? (uint32_t)fminf(fmaxf(r, 0.0f), 255.0f) : 0u;     // a NaN (refused above) comes out as 0
}

// The sq8 destination codec (the policy of build_csr.hip's row kernels): codes in the uint8 layout, encoded and decoded by lo4 / st4, the
// pitch-padded quantiser as the float4 of a chunk column.  A uint8 source IS codes: copied.
struct Sq8Codec {
    const float4 *lo4, *st4;
    typedef uint32_t word;
    static constexpr bool counts_clamped = true;
    template <int SRC> __device__ __forceinline__ HeldChunk<word> encode(const void *row, int c, int d, bool vec, bool &bad, bool &clamped) const {
        const float4 v = load_chunk_as_f32<SRC>(row, c, d, vec);        // columns >= d: zero
        const float4 lo = lo4[c], st = st4[c];
        const word w = SRC == NLSH_STORE_U8 ? pack_chunk<NLSH_STORE_U8>(v)
                     : sq8_code(v.x, lo.x, st.x, c * 4 + 0 < d, bad, clamped) | (sq8_code(v.y, lo.y, st.y, c * 4 + 1 < d, bad, clamped) << 8) |
                       (sq8_code(v.z, lo.z, st.z, c * 4 + 2 < d, bad, clamped) << 16) | (sq8_code(v.w, lo.w, st.w, c * 4 + 3 < d, bad, clamped) << 24);
        return {w, sq8_decode4(w, lo, st)};
    }
    __device__ __forceinline__ float4 decode(word w, int c) const { return sq8_decode4(w, lo4[c], st4[c]); }
};

// The inv_norm pass of an sq8 update, instantiated here: it takes the place in the code object that update_inv_norm_sq8_kernel had, so the
// kernels behind it keep the function ordinal their branch labels spell (profiles/row_codec.txt).
template __global__ void update_inv_norm_of_kernel<Sq8Codec>(const void *, long long, const float *, long long, const int32_t *, long long, float *,
                                                             const Sq8Codec);

// ---- training: per-column minimum and maximum of [n, d] rows (float32 / float16, any row stride), one read of the corpus.
// A workgroup is W x (256 / W) threads: W (a power of two >= ceil(d / 4), <= 256) chunk columns by 256 / W rows; a thread walks rows
// ry, ry + RY * gridDim.x, ... of its chunk column (one 16- / 8-byte load per row where the source allows, element loads otherwise), the
// workgroup's rows are folded through LDS and its partial goes to part[block][2][W] -- then sq8_train_final_kernel folds the partials
// and writes lo and step.  Minimum and maximum are order-free: no float atomics, and the result is bit-defined.
constexpr int SQ8_TRAIN_MAX_BLOCKS = 2048;
template <int SRC>
__global__ __launch_bounds__(256) void sq8_train_partial_kernel(const void *rows, long long stride, int d, long long n, int lgw, float4 *part,
                                                                 int32_t *first_bad, int vec) {
    typedef typename StoreElem<SRC>::elem src_t;
    __shared__ float4 smin[256], smax[256];
    const int W = 1 << lgw, RY = 256 >> lgw;
    const int cx = threadIdx.x & (W - 1), ry = threadIdx.x >> lgw;
    const int d4 = (d + 3) >> 2;
    const float inf = __builtin_inff();
    float4 mn = make_float4(inf, inf, inf, inf), mx = make_float4(-inf, -inf, -inf, -inf);
    if (cx < d4) {
        for (long long i = (long long)blockIdx.x * RY + ry; i < n; i += (long long)gridDim.x * RY) {
            const float4 v = load_chunk_as_f32<SRC>(static_cast<const src_t *>(rows) + i * stride, cx, d, vec != 0);   // columns >= d: zero
            const bool bad = !(__builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z) && __builtin_isfinite(v.w));
            report_bad_row(first_bad, bad, i);
            mn = make_float4(fminf(mn.x, v.x), fminf(mn.y, v.y), fminf(mn.z, v.z), fminf(mn.w, v.w));
            mx = make_float4(fmaxf(mx.x, v.x), fmaxf(mx.y, v.y), fmaxf(mx.z, v.z), fmaxf(mx.w, v.w));
        }
    }
    smin[threadIdx.x] = mn; smax[threadIdx.x] = mx;
    __syncthreads();
    if (ry == 0) {
        for (int r = 1; r < RY; ++r) {
            const float4 a = smin[r * W + cx], b = smax[r * W + cx];
            mn = make_float4(fminf(mn.x, a.x), fminf(mn.y, a.y), fminf(mn.z, a.z), fminf(mn.w, a.w));
            mx = make_float4(fmaxf(mx.x, b.x), fmaxf(mx.y, b.y), fmaxf(mx.z, b.z), fmaxf(mx.w, b.w));
        }
        part[((long long)blockIdx.x * 2 + 0) * W + cx] = mn;
        part[((long long)blockIdx.x * 2 + 1) * W + cx] = mx;
    }
}

// A workgroup of 16 x 16 threads per 16 entries of the padded quantiser: thread (c, s) folds the partials s, s + 16, ... of column
// j = 16 * block + c (64-byte reads across c), the 16 slices meet in LDS, and slice 0 writes lo and step; j >= d is the padding
// (lo = 0, step = 1).  (One thread per column walking all the partials took 0.5 ms of a 0.64-ms training call: 2048 dependent steps.)
__global__ __launch_bounds__(256) void sq8_train_final_kernel(const float *part, int blocks, int lgw, int d, long long n, float *lo, float *step,
                                                               long long quant_stride) {
    __shared__ float smn[16][17], smx[16][17];
    const int c = threadIdx.x & 15, s = threadIdx.x >> 4;
    const long long j = (long long)blockIdx.x * 16 + c;
    const bool live = j < d && n > 0;
    const int W4 = 4 << lgw;     // floats per partial row
    float mn = __builtin_inff(), mx = -__builtin_inff();
    if (live) {
        for (int b = s; b < blocks; b += 16) {
            mn = fminf(mn, part[((long long)b * 2 + 0) * W4 + j]);
            mx = fmaxf(mx, part[((long long)b * 2 + 1) * W4 + j]);
        }
    }
    smn[s][c] = mn; smx[s][c] = mx;
    __syncthreads();
    if (s != 0 || j >= quant_stride) return;
    if (!live) { lo[j] = 0.0f; step[j] = 1.0f; return; }
    for (int r = 1; r < 16; ++r) { mn = fminf(mn, smn[r][c]); mx = fmaxf(mx, smx[r][c]); }
    const float l = mn + 0.0f, h = mx + 0.0f;         // a zero of either sign becomes +0
    lo[j] = l;
    step[j] = h == l ? 1.0f : (h - l) / 255.0f;       // an overflowing range gives +inf: the caller refuses the column
}

static int sq8_train_shape(long long n, int d, int *lgw, int *blocks) {
    const int d4 = (d + 3) / 4;
    int lg = 0;
    while ((1 << lg) < d4) ++lg;
    const int RY = 256 >> lg;
    long long b = (n + RY - 1) / RY;
    // enough rows per workgroup that the partials stay a small fraction of the corpus
    if (b > SQ8_TRAIN_MAX_BLOCKS) b = SQ8_TRAIN_MAX_BLOCKS;
    if (b < 1) b = 1;
    *lgw = lg; *blocks = (int)b;
    return NLSH_OK;
}

}  // namespace nlsh
