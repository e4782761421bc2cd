// sq8 corpus storage, the row side (included by build_csr.hip behind its row helpers, which these kernels are built from): training the
// per-dimension quantiser, the encoding gather, and the row and inv_norm passes of nlsh_csr_update_sq8.
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

// chunk c of a source row as its four codes.  A uint8 source IS codes: copied.
template <int SRC>
__device__ __forceinline__ uint32_t sq8_encode_chunk(const void *row, int c, int d, bool vec, const float4 *lo4, const float4 *st4, bool &bad, bool &clamped) {
    const float4 v = load_chunk_as_f32<SRC>(row, c, d, vec);        // columns >= d: zero
    if (SRC == NLSH_STORE_U8) return pack_chunk<NLSH_STORE_U8>(v);
    const float4 lo = lo4[c], st = st4[c];
    return sq8_code(v.x, lo.x, st.x, c * 4 + 0 < d, bad, clamped) | (sq8_code(v.y, lo.y, st.y, c * 4 + 1 < d, bad, clamped) << 8) |
           (sq8_code(v.z, lo.z, st.z, c * 4 + 2 < d, bad, clamped) << 16) | (sq8_code(v.w, lo.w, st.w, c * 4 + 3 < d, bad, clamped) << 24);
}

// gather_rows_typed_kernel with the encoding destination: one wavefront per destination row, chunk c of the row on lane c % 64.  The sum
// of squares runs over the DECODED values in that lane assignment and chain, so inv_norm has the bits nlsh_gather_rows gives on deq(codes).
template <int SRC>
__global__ __launch_bounds__(256) void gather_rows_sq8_kernel(const void *corpus, long long src_stride, int d, const int32_t *perm, long long n,
                                                               uint32_t *sorted, long long dst_stride, const float4 *lo4, const float4 *st4,
                                                               float *inv_norm, int32_t *gid, int32_t id_base, int32_t *first_bad,
                                                               int32_t *clamped_rows, int vec) {
    typedef typename StoreElem<SRC>::elem src_t;
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const int d4 = (int)(dst_stride >> 2);
    for (long long i = wave; i < n; i += nwaves) {
        const long long src = perm[i];
        const src_t *s = static_cast<const src_t *>(corpus) + src * src_stride;
        uint32_t *dst = sorted + i * (long long)d4;
        float ss = 0.0f;
        bool bad = false, clamped = false;
        for (int c = lane; c < d4; c += 64) {
            const uint32_t w = sq8_encode_chunk<SRC>(s, c, d, vec != 0, lo4, st4, bad, clamped);
            dst[c] = w;
            ss = sumsq_chain(sq8_decode4(w, lo4[c], st4[c]), ss);
        }
        if (inv_norm) {
            ss = sumsq_lanes(ss, 64);
            if (lane == 0) inv_norm[i] = inv_norm_of(ss);
        }
        if (gid && lane == 0) gid[i] = (int32_t)src + id_base;
        report_bad_row(first_bad, bad, src);
        const bool row_clamped = __any(clamped && !bad);             // wave-uniform: the row is the wave's
        if (clamped_rows && row_clamped && lane == 0) atomicAdd(clamped_rows, 1);
    }
}

// update_rows_typed_kernel for an sq8 index: 16-byte units of 16 codes, kept rows moved as bytes, new rows encoded on the way in (a uint8
// new row is codes: copied).  inv_norm is update_inv_norm_sq8_kernel's, for the reason given at update_rows_typed_kernel.
template <int NEW>
__global__ __launch_bounds__(256) void update_rows_sq8_kernel(const uint4 *sorted_old, long long units_old, long long n_old,
                                                               const void *rows_new, long long stride_new, long long m_new, int d,
                                                               const int32_t *src, long long n_out, uint4 *sorted_out, long long units_out,
                                                               int lg, const float4 *lo4, const float4 *st4, int32_t *first_bad,
                                                               int32_t *clamped_rows, int vec) {
    typedef typename StoreElem<NEW>::elem new_t;
    const int lane = threadIdx.x & 63;
    const int lanes = 1 << lg, g = lane & (lanes - 1), rows_per_inst = 64 >> lg;
    const unsigned long long group = lanes == 64 ? ~0ull : (((1ull << lanes) - 1) << (lane - g));   // the lanes of this lane's row
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long step = (long long)rows_per_inst * ROWS_IN_FLIGHT;
    for (long long base = wave * step; base < n_out; base += nwaves * step) {     // wave-uniform
        const uint4 *so[ROWS_IN_FLIGHT];
        const new_t *sn[ROWS_IN_FLIGHT];
        long long p[ROWS_IN_FLIGHT];
        int32_t from[ROWS_IN_FLIGHT];
        bool bad[ROWS_IN_FLIGHT], clamped[ROWS_IN_FLIGHT];
#pragma unroll
        for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
            p[r] = base + (long long)r * rows_per_inst + (lane >> lg);
            from[r] = p[r] < n_out ? src[p[r]] : 0;
            const bool is_old = from[r] >= 0;
            const long long j = is_old ? (long long)from[r] : (long long)~from[r];
            const bool ok = p[r] < n_out && j < (is_old ? n_old : m_new);
            so[r] = (ok && is_old) ? sorted_old + j * units_old : nullptr;
            sn[r] = (ok && !is_old) ? static_cast<const new_t *>(rows_new) + j * stride_new : nullptr;
            bad[r] = clamped[r] = false;
        }
        for (int u = g; u < units_out; u += 64) {
            uint4 w[ROWS_IN_FLIGHT];
#pragma unroll
            for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
                if (so[r]) w[r] = u < units_old ? so[r][u] : make_uint4(0u, 0u, 0u, 0u);
                else if (sn[r]) {
                    uint32_t q[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) q[j] = sq8_encode_chunk<NEW>(sn[r], 4 * u + j, d, vec != 0, lo4, st4, bad[r], clamped[r]);
                    w[r] = make_uint4(q[0], q[1], q[2], q[3]);
                } else w[r] = make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int r = 0; r < ROWS_IN_FLIGHT; ++r)
                if (p[r] < n_out) sorted_out[p[r] * units_out + u] = w[r];
        }
#pragma unroll
        for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
            report_bad_row(first_bad, bad[r], (long long)~from[r]);
            const unsigned long long cm = __ballot(clamped[r] && !bad[r]), bm = __ballot(bad[r]);
            if (clamped_rows && g == 0 && (cm & group) && !(bm & group)) atomicAdd(clamped_rows, 1);    // one add per saturated row
        }
    }
}

// update_inv_norm_typed_kernel over decoded codes.
__global__ __launch_bounds__(256) void update_inv_norm_sq8_kernel(const uint32_t *sorted_out, long long stride_out, const float4 *lo4, const float4 *st4,
                                                                   const float *inv_old, long long n_old, const int32_t *src, long long n_out,
                                                                   float *inv_out) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const int d4 = (int)(stride_out >> 2);
    for (long long p0 = wave * 64; p0 < n_out; p0 += nwaves * 64) {     // wave-uniform
        const long long p = p0 + lane;
        const int32_t from = p < n_out ? src[p] : 0;
        if (p < n_out && from >= 0) inv_out[p] = from < n_old ? inv_old[from] : inv_norm_of(0.0f);
        unsigned long long todo = __ballot(p < n_out && from < 0);
        while (todo) {                                                   // wave-uniform: every lane reaches the butterfly
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t *row = sorted_out + (p0 + l) * (long long)d4;
            float ss = 0.0f;
            for (int c = lane; c < d4; c += 64) ss = sumsq_chain(sq8_decode4(row[c], lo4[c], st4[c]), ss);
            ss = sumsq_lanes(ss, 64);
            if (lane == 0) inv_out[p0 + l] = inv_norm_of(ss);
        }
    }
}

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
