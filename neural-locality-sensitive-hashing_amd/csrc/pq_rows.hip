// storage="pq" (include/nlsh_hip.h): the row side of product-quantised storage.  A codebook C is float32 [M, 256, dsub],
// dsub in {4, 8, 16}, M = ceil(d / dsub); a row is M bytes, byte m the index of one of the 256 centroids of sub-vector m.
//   nlsh_pq_encode       rows (float32 / float16, any row stride) -> codes: per sub-vector the centroid of the smallest squared distance,
//                        summed in ascending column order with separate subtract, multiply and add (the library is built with
//                        -ffp-contract=off), ties to the lowest index; a row holding a NaN or an infinity is refused by number.
//   nlsh_pq_decode_rows  codes -> float32 rows: element j is C[j / dsub][code[j / dsub]][j % dsub], a copy.
//   nlsh_pq_inv_norm     inv_norm of code rows, by the float32 path's rule on the decoded row (build_csr.hip, update_inv_norm_of_kernel):
//                        chunk c of the row on lane c % 64, an fmaf chain x, y, z, w per chunk in ascending c, the 64-lane xor butterfly
//                        from 32 down, 1 / max(sqrt(ss), 1e-8).
// The sorted copy of a pq index is a uint8 row store of width M: nlsh_gather_rows_typed and nlsh_csr_update_typed move it as bytes.
#include "common.h"

namespace nlsh {

template <int SRC> struct PqSrc;
template <> struct PqSrc<NLSH_STORE_F32> { typedef float elem; };
template <> struct PqSrc<NLSH_STORE_F16> { typedef _Float16 elem; };

// One workgroup per 256 rows, a lane owns a row.  Per sub-vector the 256 x DSUB slab of the codebook goes to LDS once; the lane holds
// its row's sub-vector in registers and walks the centroids, which all lanes read at the same LDS address (a broadcast).  Columns at or
// beyond d are left out of the sum (`ncols`, workgroup-uniform).  The first centroid starts the minimum and a strict `<` replaces it, so
// equal sums -- +inf among them, where a difference overflows -- keep the lowest index.  A sum is never a NaN: x and C are finite, so a
// difference is finite or an infinity and its square is not negative.
template <int SRC, int DSUB>
__global__ __launch_bounds__(256) void pq_encode_kernel(const void *rows, long long row_stride, int d, long long n, const float *codebook, int M,
                                                        uint8_t *codes, long long code_pitch, int32_t *first_bad) {
    typedef typename PqSrc<SRC>::elem src_t;
    __shared__ float4 slab[256 * DSUB / 4];
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = row < n;
    const src_t *x = static_cast<const src_t *>(rows) + (live ? row : 0) * row_stride;
    bool bad = false;
    for (int m = 0; m < M; ++m) {
        const float4 *src4 = reinterpret_cast<const float4 *>(codebook + (long long)m * 256 * DSUB);
        __syncthreads();   // everyone has finished with the previous slab
        for (int i = threadIdx.x; i < 256 * DSUB / 4; i += 256) slab[i] = src4[i];
        __syncthreads();
        const int col0 = m * DSUB, ncols = min(DSUB, d - col0);
        float v[DSUB];
#pragma unroll
        for (int j = 0; j < DSUB; ++j) {
            v[j] = (live && j < ncols) ? (float)x[col0 + j] : 0.0f;
            bad = bad || !(fabsf(v[j]) <= 3.4028234663852886e38f);   // a NaN fails the comparison
        }
        float best = 0.0f;
        int best_c = 0;
        for (int c = 0; c < 256; ++c) {
            float cv[DSUB];
#pragma unroll
            for (int j4 = 0; j4 < DSUB / 4; ++j4) {
                const float4 w = slab[c * (DSUB / 4) + j4];
                cv[4 * j4] = w.x; cv[4 * j4 + 1] = w.y; cv[4 * j4 + 2] = w.z; cv[4 * j4 + 3] = w.w;
            }
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < DSUB; ++j)
                if (j < ncols) {
                    const float t = v[j] - cv[j];
                    acc = acc + t * t;
                }
            const bool take = c == 0 || acc < best;
            best = take ? acc : best;
            best_c = take ? c : best_c;
        }
        if (live) codes[row * code_pitch + m] = (uint8_t)best_c;
    }
    if (live && bad) atomicMin(reinterpret_cast<unsigned int *>(first_bad), (unsigned int)row);   // first_bad starts at -1: unsigned minimum
}

// one thread per (row, sub-vector): DSUB floats of one codebook entry, the columns below d
__global__ __launch_bounds__(256) void pq_decode_kernel(const uint8_t *codes, long long code_pitch, long long n, const float *codebook, int dsub,
                                                        int M, int d, float *out, long long out_stride) {
    const long long total = n * M;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / M;
        const int m = (int)(i - row * M);
        const float *e = codebook + ((long long)m * 256 + codes[row * code_pitch + m]) * dsub;
        float *o = out + row * out_stride + (long long)m * dsub;
        const int ncols = min(dsub, d - m * dsub);
        for (int j = 0; j < ncols; ++j) o[j] = e[j];
    }
}

// One wavefront per row: the chain and the butterfly of gather_rows_kernel over the decoded row's M * cps chunks (columns at or beyond d
// are +0 in the codebook and add nothing: a sum of squares is never -0).
__global__ __launch_bounds__(256) void pq_inv_norm_kernel(const uint8_t *codes, long long code_pitch, long long n, const float4 *cb4, int cps,
                                                          int M, float *inv_norm) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const int d4 = M * cps, sh = cps >> 1;   // cps 1 / 2 / 4 -> shift 0 / 1 / 2
    for (long long i = wave; i < n; i += nwaves) {
        const uint8_t *row = codes + i * code_pitch;
        float ss = 0.0f;
        for (int c = lane; c < d4; c += 64) {
            const int m = c >> sh;
            const float4 v = cb4[(((long long)m * 256 + row[m]) << sh) + (c & (cps - 1))];
            ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
        }
        for (int mm = 32; mm >= 1; mm >>= 1) ss += __shfl_xor(ss, mm);
        if (lane == 0) inv_norm[i] = 1.0f / fmaxf(sqrtf(ss), 1e-8f);
    }
}

static bool pq_dsub_ok(int dsub) { return dsub == 4 || dsub == 8 || dsub == 16; }

// what the three calls share: sizes, the codebook, the codes
static int pq_common_check(const char *who, int d, int64_t n, const float *codebook, int dsub, const uint8_t *codes, int64_t code_pitch) {
    NLSH_REQUIRE(pq_dsub_ok(dsub), NLSH_E_INVALID, "%s: dsub=%d is none of 4, 8, 16", who, dsub);
    NLSH_REQUIRE(n >= 0 && n < (1ll << 31) && d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_INVALID, "%s: n=%lld d=%d", who, (long long)n, d);
    NLSH_REQUIRE(codebook && ((uintptr_t)codebook & 15) == 0, NLSH_E_INVALID, "%s: the codebook is null or not 16-byte aligned", who);
    if (n) {
        NLSH_REQUIRE(codes, NLSH_E_INVALID, "%s: codes is null", who);
        NLSH_REQUIRE(code_pitch >= (d + dsub - 1) / dsub, NLSH_E_INVALID, "%s: code_pitch=%lld < M=%d", who, (long long)code_pitch, (d + dsub - 1) / dsub);
    }
    return NLSH_OK;
}

}  // namespace nlsh

using namespace nlsh;

extern "C" int nlsh_pq_encode(const void *rows, int storage, int64_t row_stride, int d, int64_t n, const float *codebook, int dsub,
                              uint8_t *codes, int64_t code_pitch, int32_t *first_bad, nlsh_stream_t stream) {
    NLSH_REQUIRE(storage == NLSH_STORE_F32 || storage == NLSH_STORE_F16, NLSH_E_INVALID, "pq_encode: storage=%d is neither NLSH_STORE_F32 nor NLSH_STORE_F16", storage);
    int rc = pq_common_check("pq_encode", d, n, codebook, dsub, codes, code_pitch);
    if (rc != NLSH_OK) return rc;
    NLSH_REQUIRE(first_bad, NLSH_E_INVALID, "pq_encode: first_bad is null");
    if (n) {
        NLSH_REQUIRE(rows, NLSH_E_INVALID, "pq_encode: rows is null");
        NLSH_REQUIRE(row_stride >= d, NLSH_E_INVALID, "pq_encode: row_stride=%lld < d=%d", (long long)row_stride, d);
        NLSH_REQUIRE(((uintptr_t)rows & (storage == NLSH_STORE_F32 ? 3 : 1)) == 0, NLSH_E_INVALID, "pq_encode: rows is not aligned to its element size");
    }
    hipStream_t s = (hipStream_t)stream;
    NLSH_CHECK_HIP(hipMemsetAsync(first_bad, 0xFF, sizeof(int32_t), s));   // -1: every row is finite
    if (n == 0) return NLSH_OK;
    const bool f32 = storage == NLSH_STORE_F32;
    const void *fn = dsub == 4 ? (f32 ? (const void *)pq_encode_kernel<NLSH_STORE_F32, 4> : (const void *)pq_encode_kernel<NLSH_STORE_F16, 4>)
                   : dsub == 8 ? (f32 ? (const void *)pq_encode_kernel<NLSH_STORE_F32, 8> : (const void *)pq_encode_kernel<NLSH_STORE_F16, 8>)
                               : (f32 ? (const void *)pq_encode_kernel<NLSH_STORE_F32, 16> : (const void *)pq_encode_kernel<NLSH_STORE_F16, 16>);
    long long rs = row_stride, nn = n, cp = code_pitch;
    int M = (d + dsub - 1) / dsub;
    void *argv[] = {&rows, &rs, &d, &nn, &codebook, &M, &codes, &cp, &first_bad};
    NLSH_CHECK_HIP(hipLaunchKernel(fn, dim3((unsigned)((n + 255) / 256)), dim3(256), argv, 0, s));
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

extern "C" int nlsh_pq_decode_rows(const uint8_t *codes, int64_t code_pitch, int64_t n, const float *codebook, int dsub, int d, float *out,
                                   int64_t out_stride, nlsh_stream_t stream) {
    int rc = pq_common_check("pq_decode_rows", d, n, codebook, dsub, codes, code_pitch);
    if (rc != NLSH_OK) return rc;
    if (n == 0) return NLSH_OK;
    NLSH_REQUIRE(out && ((uintptr_t)out & 3) == 0, NLSH_E_INVALID, "pq_decode_rows: out is null or not 4-byte aligned");
    NLSH_REQUIRE(out_stride >= d, NLSH_E_INVALID, "pq_decode_rows: out_stride=%lld < d=%d", (long long)out_stride, d);
    const int M = (d + dsub - 1) / dsub;
    long long blocks = (n * M + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(pq_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, codes, (long long)code_pitch, (long long)n, codebook,
                       dsub, M, d, out, (long long)out_stride);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

extern "C" int nlsh_pq_inv_norm(const uint8_t *codes, int64_t code_pitch, int64_t n, const float *codebook, int dsub, int d, float *inv_norm,
                                nlsh_stream_t stream) {
    int rc = pq_common_check("pq_inv_norm", d, n, codebook, dsub, codes, code_pitch);
    if (rc != NLSH_OK) return rc;
    if (n == 0) return NLSH_OK;
    NLSH_REQUIRE(inv_norm, NLSH_E_INVALID, "pq_inv_norm: inv_norm is null");
    const int M = (d + dsub - 1) / dsub;
    long long blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(pq_inv_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, codes, (long long)code_pitch, (long long)n,
                       (const float4 *)codebook, dsub / 4, M, inv_norm);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
