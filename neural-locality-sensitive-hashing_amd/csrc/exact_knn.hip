// Exact brute-force k-NN (nlsh_exact_topk): fp32-MFMA distance GEMM with the top-k selection fused behind it.  Replaces, for callers that
// want it, the reference's mm + topk precompute (precompute.py:22-67): ground truth of a query set and the self-kNN of a training set.  The
// [Q, N] distance matrix never exists: a workgroup forms a 128 x 128 block of it in its accumulators, compares it with the queries' running
// k-th best and throws it away.
//
// Distances (precompute.py:22-54; NOT the scan's pairwise_distance form -- no square root, no epsilon):
//   NLSH_EXACT_L2      (||c||^2 - 2 (q.c)) + ||q||^2
//   NLSH_EXACT_COSINE  1 - ((q.c) * inv||q||) * inv||c||,  inv||x|| = 1 / max(||x||, 1e-12)   (the clamp of data.brute_force_topk)
// Numerical contract: q.c, ||q||^2 and ||c||^2 are each ONE fp32 chain over the dimension, ascending from 0 -- the accumulator chain of
// v_mfma_f32_32x32x2_f32 for q.c (bit for bit an fmaf chain; zero padding of the dimension adds fma(0, 0, acc) = acc), an fmaf chain for the
// norms.  No split-K, no partial sums across workgroups: the distance of a (query, row) pair is a function of the two vectors alone, whatever
// tile, column split or launch shape the pair falls in.
// Order: the project's total order, ascending 64-bit key monotone(dist) << 32 | row id.  Inputs are finite (precondition, not checked).
//
// Launches: exact_norms_kernel (corpus, queries) -> exact_knn_kernel -> nlsh_merge_topk's kernel with G = column splits.
//   * a workgroup (4 waves, 2 x 2, each 2 x 2 tiles of 32 x 32) owns 128 queries x one column split of the corpus and walks the split in
//     tiles of 128 rows; rows are the MFMA's A operand and queries its B operand, so a lane holds 16 rows of ONE query per accumulator tile
//     and the query's threshold and norm live in that lane's registers;
//   * both operands go through LDS in slabs of 32 dimensions in the de-interleaved layout of the streamed encoder (one ds_read_b128 = the
//     operands of four k-steps); the next slab's global loads are in flight under the current slab's MFMAs;
//   * epilogue: two or three VALU operations form the distance, one compare holds it against the query's threshold; a survivor takes a slot of
//     the query's candidate buffer (LDS counter, keys in the workspace: 128 queries x 256..512 keys do not fit 160 KiB of LDS beside two
//     workgroups' tiles, and after the first tiles almost nothing survives);
//   * between two tiles a wave compacts every buffer that the next tile could overflow to its k smallest keys (select_k_smallest, the
//     selection the merges use) and tightens the threshold to the k-th distance.  The threshold is STRICT: a later row at exactly the k-th
//     distance has a larger id than the k keys kept (a workgroup walks rows in ascending order), so it lies beyond them in the total order;
//   * the split's final k keys stay at the head of the query's buffer row; merge_topk reads them with row_stride = the buffer's capacity.
#include "scan_common.h"

namespace nlsh {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int XK_BM = 128;         // corpus rows per tile
constexpr int XK_BQ = 128;         // queries per workgroup
constexpr int XK_KS = 32;          // dimensions per LDS slab
constexpr int XK_S = XK_KS + 4;    // LDS row stride: S / 4 odd -> conflict-free ds_read_b128
constexpr int XK_MAX_SPLITS = 1024;
constexpr int XK_AUTO_SLOTS = 512;   // workgroups the chip holds at two per CU
constexpr int XK_AUTO_MAX_SPLITS = 64;

// candidate-buffer capacity of a k class: a tile adds at most XK_BM keys per query, a buffer is compacted to k keys when it holds more than
// CAP - XK_BM, so CAP - XK_BM >= k
static inline int exact_cap(int k) { return k <= 64 ? 256 : 512; }

struct XArgs {
    const float *corpus; long long row_stride; long long N; int d;
    const float *queries; long long q_stride; long long Q; int k;
    long long self_row0; int S; int nqt;
    const float *cnorm, *qnorm;
    uint64_t *cand;
};

// one thread per row: the chain is sequential by contract.  L2: ||x||^2; cosine: 1 / max(||x||, 1e-12)
__global__ __launch_bounds__(256) void exact_norms_kernel(const float *__restrict__ x, long long stride, long long n, int d, int metric,
                                                          float *__restrict__ out) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const float *p = x + r * stride;
    float ss = 0.0f;
    if ((((long long)d | stride) & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        for (int c = 0; c < d; c += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(p + c);
            ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
        }
    } else {
        for (int c = 0; c < d; ++c) ss = fmaf(p[c], p[c], ss);
    }
    out[r] = metric == NLSH_EXACT_COSINE ? 1.0f / fmaxf(sqrtf(ss), 1e-12f) : ss;
}

// the k smallest of the n keys of one query's buffer, written back to its head (KEY_NONE padded to k); one wave
template <int NK>
__device__ __forceinline__ uint64_t exact_compact(uint64_t *buf, int n, int k, int lane) {
    uint64_t key[NK];
#pragma unroll
    for (int i = 0; i < NK; ++i) key[i] = i * 64 + lane < n ? buf[i * 64 + lane] : KEY_NONE;
    // every lane's loads are consumed by the selection's first ballots before any lane stores: in place is safe within one wave
    return select_k_smallest<NK, false, true>(key, k, lane, buf);
}

template <int NK, int METRIC>
__global__ __launch_bounds__(256, 2) void exact_knn_kernel(XArgs a) {
    constexpr int CAP = NK * 64, NV = XK_BM * (XK_KS / 4) / 256;
    static_assert(XK_BM == XK_BQ, "one staging loop serves both operands");
    __shared__ float4 As4[XK_BM * XK_S / 4], Bs4[XK_BQ * XK_S / 4], cns4[XK_BM / 4];
    __shared__ float thr[XK_BQ];
    __shared__ int cnt[XK_BQ];
    float *As = reinterpret_cast<float *>(As4), *Bs = reinterpret_cast<float *>(Bs4), *cns = reinterpret_cast<float *>(cns4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int wr = wave & 1, wc = wave >> 1;
    const int s = (int)(blockIdx.x / (unsigned)a.nqt);
    const long long q0 = (long long)(blockIdx.x - (unsigned)s * (unsigned)a.nqt) * XK_BQ;
    const long long T = (a.N + XK_BM - 1) / XK_BM, t_begin = s * T / a.S, t_end = (s + 1) * T / a.S;
    const int d = a.d, nslab = (d + XK_KS - 1) / XK_KS;
    uint64_t *cbase = a.cand + ((long long)s * a.Q + q0) * CAP;   // rows of queries past Q are never touched

    if (tid < XK_BQ) {
        thr[tid] = q0 + tid < a.Q ? __builtin_inff() : -__builtin_inff();   // a padding query takes nothing
        cnt[tid] = 0;
    }
    float qnv[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const long long qg = q0 + (wc * 2 + ct) * 32 + lr;
        qnv[ct] = qg < a.Q ? a.qnorm[qg] : 0.0f;
    }
    const bool vec_a = (((long long)d | a.row_stride) & 3) == 0 && (reinterpret_cast<uintptr_t>(a.corpus) & 15) == 0;
    const bool vec_b = (((long long)d | a.q_stride) & 3) == 0 && (reinterpret_cast<uintptr_t>(a.queries) & 15) == 0;

    float4 va[NV], vb[NV];
    auto load_rows = [&](float4 (&v)[NV], const float *base, long long stride, long long row0, long long nrows, bool vec, int k0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = i * 256 + tid, r = e >> 3, k = k0 + 4 * (e & 7);
            const long long grow = row0 + r;
            const bool live = grow < nrows;
            const float *src = base + grow * stride + k;
            if (vec) {
                v[i] = (live && k < d) ? *reinterpret_cast<const float4 *>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                v[i].x = live && k < d ? src[0] : 0.0f;
                v[i].y = live && k + 1 < d ? src[1] : 0.0f;
                v[i].z = live && k + 2 < d ? src[2] : 0.0f;
                v[i].w = live && k + 3 < d ? src[3] : 0.0f;
            }
        }
    };
    auto stage = [&](float *dst0, const float4 (&v)[NV]) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = i * 256 + tid, r = e >> 3, q = e & 7;
            float *dst = dst0 + r * XK_S + ((4 * q) & ~7) + ((q & 1) << 1);   // pos(4q + j) = base + {0, 4, 1, 5}
            dst[0] = v[i].x; dst[4] = v[i].y; dst[1] = v[i].z; dst[5] = v[i].w;
        }
    };
    const float *arow = As + (wr * 64 + lr) * XK_S + 4 * lh;
    const float *brow = Bs + (wc * 64 + lr) * XK_S + 4 * lh;

    for (long long t = t_begin; t < t_end; ++t) {
        const long long c0 = t * XK_BM;
        f32x16 acc[2][2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[rt][ct][i] = 0.0f;
        load_rows(va, a.corpus, a.row_stride, c0, a.N, vec_a, 0);
        load_rows(vb, a.queries, a.q_stride, q0, a.Q, vec_b, 0);
        const float cn_mine = (tid < XK_BM && c0 + tid < a.N) ? a.cnorm[c0 + tid] : 0.0f;
        for (int sl = 0; sl < nslab; ++sl) {
            __syncthreads();   // every wave has finished with the previous slab (and with the previous tile's norms)
            stage(As, va);
            stage(Bs, vb);
            if (sl == 0 && tid < XK_BM) cns[tid] = cn_mine;
            __syncthreads();
            if (sl + 1 < nslab) {
                load_rows(va, a.corpus, a.row_stride, c0, a.N, vec_a, (sl + 1) * XK_KS);
                load_rows(vb, a.queries, a.q_stride, q0, a.Q, vec_b, (sl + 1) * XK_KS);
            }
#pragma unroll
            for (int j = 0; j < XK_KS / 8; ++j) {
                if (sl * XK_KS + j * 8 < d) {   // whole groups of 8 past d hold zeros only
                    float4 av[2], bv[2];
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) av[rt] = *reinterpret_cast<const float4 *>(arow + rt * 32 * XK_S + j * 8);
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) bv[ct] = *reinterpret_cast<const float4 *>(brow + ct * 32 * XK_S + j * 8);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                            for (int ct = 0; ct < 2; ++ct) {
                                const float aa = i == 0 ? av[rt].x : i == 1 ? av[rt].y : i == 2 ? av[rt].z : av[rt].w;
                                const float bb = i == 0 ? bv[ct].x : i == 1 ? bv[ct].y : i == 2 ? bv[ct].z : bv[ct].w;
                                acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa, bb, acc[rt][ct], 0, 0, 0);
                            }
                }
            }
        }

        // C/D map: col (query) = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int qi = (wc * 2 + ct) * 32 + lr;
            const float th = thr[qi], qn = qnv[ct];
            const long long self_row = a.self_row0 >= 0 ? a.self_row0 + q0 + qi : -1;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const int rbase = (wr * 2 + rt) * 32 + 4 * lh;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 cn4 = *reinterpret_cast<const float4 *>(cns + rbase + 8 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float dot = acc[rt][ct][4 * g + e];
                        const float cn = e == 0 ? cn4.x : e == 1 ? cn4.y : e == 2 ? cn4.z : cn4.w;
                        float dist;
                        if (METRIC == NLSH_EXACT_L2) dist = (cn - 2.0f * dot) + qn;
                        else dist = 1.0f - (dot * qn) * cn;
                        if (dist < th) {
                            const long long row = c0 + rbase + 8 * g + e;
                            if (row < a.N && row != self_row) {
                                const int pos = atomicAdd(&cnt[qi], 1);   // < CAP: the buffer held <= CAP - XK_BM keys before this tile
                                cbase[(long long)qi * CAP + pos] = make_key(dist, (int32_t)row);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();   // the tile's candidates are in the buffers, its counters final
        for (int qi = wave; qi < XK_BQ; qi += 4) {
            const int n = __builtin_amdgcn_readfirstlane(cnt[qi]);
            if (n > CAP - XK_BM) {
                const uint64_t bound = exact_compact<NK>(cbase + (long long)qi * CAP, n, a.k, lane);
                if (lane == 0) {
                    cnt[qi] = a.k;   // n > CAP - XK_BM >= k
                    thr[qi] = float_from_mono((uint32_t)(bound >> 32) - 1u);   // bound = (k-th distance word + 1) << 32
                }
            }
        }
    }

    __syncthreads();   // a split without tiles (N = 0) comes here straight from the initialisation
    for (int qi = wave; qi < XK_BQ; qi += 4) {
        if (q0 + qi >= a.Q) break;
        const int n = __builtin_amdgcn_readfirstlane(cnt[qi]);
        exact_compact<NK>(cbase + (long long)qi * CAP, n, a.k, lane);
    }
}

struct ExactWs {
    size_t cnorm, qnorm, cand, total;
    int S, cap;
};

// splits = 0: as many column splits as fill the chip's workgroup slots beside the query tiles, a function of Q alone (so that the
// workspace depends on N through the norm array only); the launch clamps it to the number of corpus tiles
static bool exact_layout(long long Q, long long N, int k, int splits, ExactWs *w) {
    if (k < 1 || k > NLSH_MAX_K_TILED || Q < 0 || N < 0 || N >= (1ll << 31) || splits < 0 || splits > XK_MAX_SPLITS) return false;
    const long long nqt = (Q + XK_BQ - 1) / XK_BQ;
    long long S = splits;
    if (S == 0) {
        S = nqt > 0 ? XK_AUTO_SLOTS / nqt : 1;
        S = S < 1 ? 1 : S > XK_AUTO_MAX_SPLITS ? XK_AUTO_MAX_SPLITS : S;
    }
    if (nqt * S >= (1ll << 31)) return false;
    w->S = (int)S;
    w->cap = exact_cap(k);
    size_t o = 256;   // never 0 for valid arguments
    w->cnorm = o; o += ws_align((size_t)N * 4);
    w->qnorm = o; o += ws_align((size_t)Q * 4);
    w->cand = o;  o += ws_align((size_t)S * (size_t)Q * (size_t)w->cap * 8);
    w->total = o;
    return true;
}

}  // namespace nlsh

using namespace nlsh;

extern "C" size_t nlsh_exact_workspace(int64_t Q, int64_t N, int k, int splits) {
    ExactWs w;
    return exact_layout(Q, N, k, splits, &w) ? w.total : 0;
}

extern "C" int nlsh_exact_topk(const float *corpus, int64_t row_stride, int64_t N, int d, const float *queries, int64_t q_stride, int64_t Q,
                               int k, int metric, int64_t self_row0, int splits, float *out_dist, int32_t *out_idx, void *workspace,
                               size_t workspace_bytes, nlsh_stream_t stream) {
    NLSH_REQUIRE(d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_UNSUPPORTED, "exact_topk: d=%d outside 1..%d (NLSH_MAX_DIM)", d, NLSH_MAX_DIM);
    NLSH_REQUIRE(k >= 1 && k <= NLSH_MAX_K_TILED, NLSH_E_UNSUPPORTED, "exact_topk: k=%d outside 1..%d (NLSH_MAX_K_TILED)", k, NLSH_MAX_K_TILED);
    NLSH_REQUIRE(metric == NLSH_EXACT_L2 || metric == NLSH_EXACT_COSINE, NLSH_E_INVALID,
                 "exact_topk: metric=%d is neither NLSH_EXACT_L2 nor NLSH_EXACT_COSINE", metric);
    NLSH_REQUIRE(Q >= 0 && N >= 0, NLSH_E_INVALID, "exact_topk: Q=%lld N=%lld", (long long)Q, (long long)N);
    NLSH_REQUIRE(N < (1ll << 31), NLSH_E_UNSUPPORTED, "exact_topk: N=%lld, row ids are int32 (N < 2^31)", (long long)N);
    NLSH_REQUIRE(row_stride >= d && q_stride >= d, NLSH_E_INVALID, "exact_topk: row_stride=%lld q_stride=%lld below d=%d", (long long)row_stride,
                 (long long)q_stride, d);
    NLSH_REQUIRE(self_row0 >= -1, NLSH_E_INVALID, "exact_topk: self_row0=%lld (-1 = none)", (long long)self_row0);
    NLSH_REQUIRE(splits >= 0 && splits <= XK_MAX_SPLITS, NLSH_E_INVALID, "exact_topk: splits=%d outside 0..%d (0 = automatic)", splits, XK_MAX_SPLITS);
    ExactWs w;
    NLSH_REQUIRE(exact_layout(Q, N, k, splits, &w), NLSH_E_UNSUPPORTED, "exact_topk: Q=%lld with %d splits exceeds the launch grid", (long long)Q,
                 splits);
    if (Q == 0) return NLSH_OK;
    NLSH_REQUIRE(workspace_bytes >= w.total, NLSH_E_WORKSPACE, "exact_topk: workspace %zu < %zu bytes (nlsh_exact_workspace)", workspace_bytes,
                 w.total);
    NLSH_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, NLSH_E_INVALID,
                 "exact_topk: workspace is null or not 16-byte aligned");
    NLSH_REQUIRE(queries && out_dist && out_idx && (corpus || N == 0), NLSH_E_INVALID, "exact_topk: null pointer");

    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    float *cnorm = reinterpret_cast<float *>(ws + w.cnorm), *qnorm = reinterpret_cast<float *>(ws + w.qnorm);
    if (N > 0)
        hipLaunchKernelGGL(exact_norms_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, corpus, (long long)row_stride, (long long)N, d,
                           metric, cnorm);
    hipLaunchKernelGGL(exact_norms_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, queries, (long long)q_stride, (long long)Q, d,
                       metric, qnorm);
    NLSH_CHECK_HIP(hipGetLastError());

    XArgs a;
    a.corpus = corpus; a.row_stride = row_stride; a.N = N; a.d = d;
    a.queries = queries; a.q_stride = q_stride; a.Q = Q; a.k = k;
    a.self_row0 = self_row0;
    const long long T = (N + XK_BM - 1) / XK_BM;
    a.S = (int)(T < 1 ? 1 : T < w.S ? T : w.S);
    a.nqt = (int)((Q + XK_BQ - 1) / XK_BQ);
    a.cnorm = cnorm; a.qnorm = qnorm;
    a.cand = reinterpret_cast<uint64_t *>(ws + w.cand);
    const dim3 grid((unsigned)((long long)a.nqt * a.S));
    if (w.cap == 256) {
        if (metric == NLSH_EXACT_L2) hipLaunchKernelGGL((exact_knn_kernel<4, NLSH_EXACT_L2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((exact_knn_kernel<4, NLSH_EXACT_COSINE>), grid, dim3(256), 0, st, a);
    } else {
        if (metric == NLSH_EXACT_L2) hipLaunchKernelGGL((exact_knn_kernel<8, NLSH_EXACT_L2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((exact_knn_kernel<8, NLSH_EXACT_COSINE>), grid, dim3(256), 0, st, a);
    }
    NLSH_CHECK_HIP(hipGetLastError());
    return nlsh_merge_topk(a.cand, w.cap, a.S, Q, k, nullptr, out_dist, out_idx, nullptr, stream);
}
