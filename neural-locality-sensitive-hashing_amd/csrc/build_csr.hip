// Index build: keys[n] -> CSR (perm, uniq_keys, offsets) and the bucket-contiguous corpus copy.
//
// Replaces build_index (nlsh/indexer.py:6-24: Python dict of row lists + one tiny H2D per
// bucket) and, once per index instead of once per (query, key), the index_select gather of
// nlsh/indexer.py:77-82.  The stable LSD radix sort of (key, row) pairs is rocPRIM's (a native
// ROCm primitive; this step is SURVEY.md §8(f) row N1, outside the graded scan/encode kernels);
// bucket heads, offsets and the row permutation/gather are hand-written.
// Index update (nlsh_csr_update, no reference counterpart): new rows merged into and removed rows dropped from a built index in one
// out-of-place pass, with the build's own bucket-table kernels and row helpers.
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "common.h"

namespace nlsh {

__global__ void iota_kernel(int32_t *v, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        v[i] = (int32_t)i;
}

__global__ void head_flags_kernel(const int32_t *sk, long long n, int32_t *flags) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        flags[i] = (i == 0 || sk[i] != sk[i - 1]) ? 1 : 0;
}

// rank[i] = inclusive prefix sum of flags -> bucket index + 1 of row i (sorted order).
__global__ void emit_buckets_kernel(const int32_t *sk, const int32_t *flags, const int32_t *rank, long long n,
                                    int32_t *uniq, int32_t *offsets, int32_t *n_buckets) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (flags[i]) {
            int b = rank[i] - 1;
            uniq[b] = sk[i];
            offsets[b] = (int32_t)i;
        }
        if (i == n - 1) {
            int nb = rank[i];
            offsets[nb] = (int32_t)n;
            *n_buckets = nb;
        }
    }
}

// float4 number c of a d-float row at `s`, columns >= d read as zero.  VEC: `s` is 16-byte aligned (one 16-byte load where the whole
// float4 lies inside the row).
template <bool VEC>
__device__ __forceinline__ float4 load_row_chunk(const float *s, int c, int d) {
    float4 v;
    if (VEC) {
        v = (c * 4 + 3 < d) ? *reinterpret_cast<const float4 *>(s + c * 4) : make_float4(0, 0, 0, 0);
        if (!(c * 4 + 3 < d)) {
            v.x = c * 4 + 0 < d ? s[c * 4 + 0] : 0.0f;
            v.y = c * 4 + 1 < d ? s[c * 4 + 1] : 0.0f;
            v.z = c * 4 + 2 < d ? s[c * 4 + 2] : 0.0f;
            v.w = 0.0f;
        }
    } else {
        v.x = c * 4 + 0 < d ? s[c * 4 + 0] : 0.0f;
        v.y = c * 4 + 1 < d ? s[c * 4 + 1] : 0.0f;
        v.z = c * 4 + 2 < d ? s[c * 4 + 2] : 0.0f;
        v.w = c * 4 + 3 < d ? s[c * 4 + 3] : 0.0f;
    }
    return v;
}

// A row's sum of squares, the part of one lane: lane l of the row's lane group chains the float4s l, l + 64, l + 128, ... in that order.
__device__ __forceinline__ float sumsq_chain(float4 v, float ss) {
    ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
    return ss;
}

// ... and the sum over the row's `lanes` lanes (a power of two, an aligned group of the wavefront): the xor butterfly from lanes / 2
// down.  A row of at most `lanes` float4s summed over 64 lanes gives the same bits: the lanes past the row hold +0, a sum of squares
// is never -0, so every butterfly step of 64 lanes above lanes / 2 adds +0 to it.  EVERY lane of the wavefront must call this.
__device__ __forceinline__ float sumsq_lanes(float ss, int lanes) {
    for (int m = 32; m >= 1; m >>= 1) {
        const float other = __shfl_xor(ss, m);
        ss += m < lanes ? other : 0.0f;
    }
    return ss;
}

__device__ __forceinline__ float inv_norm_of(float ss) { return 1.0f / fmaxf(sqrtf(ss), 1e-8f); }  // cosine_similarity eps (nlsh/data.py:109)

// One wavefront per destination row; 16-byte loads when the source allows it.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *corpus, long long src_stride, int d, const int32_t *perm,
                                                           long long n, float *sorted, long long dst_stride, float *inv_norm,
                                                           int32_t *gid, int32_t id_base) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const int d4 = (int)(dst_stride >> 2);
    for (long long i = wave; i < n; i += nwaves) {
        const long long src = perm[i];
        const float *s = corpus + src * src_stride;
        float4 *dst = reinterpret_cast<float4 *>(sorted + i * dst_stride);
        float ss = 0.0f;
        for (int c = lane; c < d4; c += 64) {
            const float4 v = load_row_chunk<VEC>(s, c, d);
            dst[c] = v;
            ss = sumsq_chain(v, ss);
        }
        if (inv_norm) {
            ss = sumsq_lanes(ss, 64);
            if (lane == 0) inv_norm[i] = inv_norm_of(ss);
        }
        if (gid && lane == 0) gid[i] = (int32_t)src + id_base;
    }
}

// bucket sizes as sort keys + identity values for the size-descending schedule order
__global__ void bucket_sizes_kernel(const int32_t *offsets, long long nb, uint32_t *sizes, int32_t *idx) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (long long)gridDim.x * blockDim.x) {
        sizes[i] = (uint32_t)(offsets[i + 1] - offsets[i]);
        idx[i] = (int32_t)i;
    }
}


// ---- cells: runs of consecutive small buckets that share one row window of the tiled scan ------------------------------------
// Greedy packing in CSR order: a bucket of more than `W` rows is a cell of its own; consecutive buckets of <= W rows are packed
// into one cell while the cell's rows stay <= W.  One WAVEFRONT packs CELL_SPAN consecutive buckets (the packing restarts at every
// span boundary, so the result is a pure function of (offsets, W) and the spans are independent): it holds 64 buckets at a time,
// one per lane, and takes one ballot per CELL, not per bucket -- the lanes past the open cell's last fitting bucket vote, the
// first of them starts the next cell.
constexpr int CELL_SPAN = 1024;

__global__ __launch_bounds__(256) void cell_flags_kernel(const int32_t *offsets, long long nb, int W, int32_t *flags) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long b0 = wave * CELL_SPAN;
    if (b0 >= nb) return;
    int cur = -1;   // first row of the open cell; -1: none (span start, or the previous bucket was a big one)
    for (int ch = 0; ch < CELL_SPAN / 64; ++ch) {
        const long long cb = b0 + (long long)ch * 64;
        if (cb >= nb) break;
        const long long b = cb + lane;
        const int nvalid = (int)min((long long)64, nb - cb);
        const int s = b < nb ? offsets[b] : 0, e = b < nb ? offsets[b + 1] : 0;
        const bool small = (e - s) <= W;
        unsigned long long starts = 0;
        int pos = 0;
        while (pos < nvalid) {
            const int s_p = __builtin_amdgcn_readlane(s, pos), e_p = __builtin_amdgcn_readlane(e, pos);
            if (e_p - s_p > W) {          // big bucket: a cell of its own, and nothing is open behind it
                starts |= 1ull << pos;
                cur = -1;
                ++pos;
                continue;
            }
            if (cur < 0 || e_p - cur > W) {   // does not fit the open cell: it opens the next one
                starts |= 1ull << pos;
                cur = s_p;
            }
            const unsigned long long stop = __ballot(lane > pos && lane < nvalid && (!small || e - cur > W));
            pos = stop ? __ffsll((long long)stop) - 1 : nvalid;
        }
        if (b < nb) flags[b] = (int32_t)((starts >> lane) & 1ull);
    }
}

// rank = inclusive prefix sum of the flags: cell of bucket b = rank[b] - 1.  cell_offsets is written for ALL nb + 1 slots (slots past
// the last cell hold N: zero-row cells), so the size sort below can run on nb entries without the host knowing the cell count.
__global__ void emit_cells_kernel(const int32_t *offsets, const int32_t *flags, const int32_t *rank, long long nb, int32_t *cell_of,
                                  int32_t *cell_offsets, int32_t *n_cells) {
    const int32_t nc = rank[nb - 1], n_rows = offsets[nb];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i <= nb; i += (long long)gridDim.x * blockDim.x) {
        if (i < nb) {
            cell_of[i] = rank[i] - 1;
            if (flags[i]) cell_offsets[rank[i] - 1] = offsets[i];
        }
        if (i >= nc) cell_offsets[i] = n_rows;
        if (i == 0) *n_cells = nc;
    }
}

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct OrderWs {
    size_t sizes, sorted_sizes, idx, tmp, tmp_bytes, total;
};

static int order_layout(long long nb, OrderWs *w, hipStream_t s) {
    const size_t n4 = align_up((size_t)(nb > 0 ? nb : 1) * 4);
    size_t t_sort = 0;
    uint32_t *nulk = nullptr;
    int32_t *nulv = nullptr;
    hipError_t e = rocprim::radix_sort_pairs_desc(nullptr, t_sort, nulk, nulk, nulv, nulv, (size_t)nb, 0, 32, s);
    if (e != hipSuccess) { set_error("rocprim::radix_sort_pairs_desc size query: %s", hipGetErrorString(e)); return NLSH_E_HIP; }
    w->sizes = 0;
    w->sorted_sizes = n4;
    w->idx = 2 * n4;
    w->tmp = 3 * n4;
    w->tmp_bytes = align_up(t_sort);
    w->total = w->tmp + w->tmp_bytes;
    return NLSH_OK;
}

struct CsrWs {
    size_t sk, iota, flags, rank, tmp, tmp_bytes, total;
};

static int csr_layout(long long n, CsrWs *w, hipStream_t s) {
    size_t n4 = align_up((size_t)(n > 0 ? n : 1) * 4);
    size_t t_sort = 0, t_scan = 0;
    int32_t *nul = nullptr;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, t_sort, nul, nul, nul, nul, (size_t)n, 0, 32, s);
    if (e != hipSuccess) { set_error("rocprim::radix_sort_pairs size query: %s", hipGetErrorString(e)); return NLSH_E_HIP; }
    e = rocprim::inclusive_scan(nullptr, t_scan, nul, nul, (size_t)n, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) { set_error("rocprim::inclusive_scan size query: %s", hipGetErrorString(e)); return NLSH_E_HIP; }
    w->sk = 0;
    w->iota = w->sk + n4;
    w->flags = w->iota + n4;
    w->rank = w->flags + n4;
    w->tmp = w->rank + n4;
    w->tmp_bytes = align_up(t_sort > t_scan ? t_sort : t_scan);
    w->total = w->tmp + w->tmp_bytes;
    return NLSH_OK;
}

// keys[n] (n >= 1) -> perm, uniq_keys, offsets, n_buckets with caller-placed scratch: sk, iota, flags, rank int32 [n] each, tmp for rocPRIM.
static int build_csr_on(const int32_t *keys, long long n, int32_t *perm, int32_t *uniq_keys, int32_t *offsets, int32_t *n_buckets,
                        int32_t *sk, int32_t *iota, int32_t *flags, int32_t *rank, void *tmp, size_t tmp_bytes, hipStream_t s) {
    int grid = (int)((n + 255) / 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(iota_kernel, dim3(grid), dim3(256), 0, s, iota, n);
    size_t tb = tmp_bytes;
    // stable: equal keys keep ascending row order (the insertion order of indexer.py:8-13)
    NLSH_CHECK_HIP(rocprim::radix_sort_pairs(tmp, tb, keys, sk, iota, perm, (size_t)n, 0, 32, s));
    hipLaunchKernelGGL(head_flags_kernel, dim3(grid), dim3(256), 0, s, sk, n, flags);
    tb = tmp_bytes;
    NLSH_CHECK_HIP(rocprim::inclusive_scan(tmp, tb, flags, rank, (size_t)n, rocprim::plus<int32_t>(), s));
    hipLaunchKernelGGL(emit_buckets_kernel, dim3(grid), dim3(256), 0, s, sk, flags, rank, n, uniq_keys, offsets, n_buckets);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

// ---- index update: merge a sorted batch of new rows into the CSR index, drop removed rows (include/nlsh_hip.h, nlsh_csr_update) -------
// Positions are int32 throughout (n_old, n_out < 2^31).  `kex` = exclusive prefix sum of `keep` with kex[n_old] = rows kept; NULL = every
// old row is kept (kex[i] = i).

__device__ __forceinline__ int kept_before(const int32_t *kex, int i) { return kex ? kex[i] : i; }

// first index in [0, n) with a[index] >= v (lower) / > v (upper), signed order
__device__ __forceinline__ int lower_bound_i32(const int32_t *a, int n, int32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int upper_bound_i32(const int32_t *a, int n, int32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Once per bucket of either side, the distance its rows move:
//   shift_old[b] = new rows with a key below uniq_old[b]            (a kept old row i of bucket b lands at kex[i] + shift_old[b])
//   shift_new[c] = kept old rows with a key up to uniq_new[c]       (the new row at new-sorted position t of bucket c lands at t + shift_new[c])
__global__ void update_shifts_kernel(const int32_t *uniq_old, const int32_t *offs_old, int nb_old, int n_old, const int32_t *kex,
                                     const int32_t *uniq_new, const int32_t *offs_new, const int32_t *nb_new_p, int m_new,
                                     int32_t *shift_old, int32_t *shift_new) {
    const int nb_new = m_new ? *nb_new_p : 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)nb_old + nb_new; i += (long long)gridDim.x * blockDim.x) {
        if (i < nb_old) {
            const int b = (int)i;
            shift_old[b] = m_new ? offs_new[lower_bound_i32(uniq_new, nb_new, uniq_old[b])] : 0;
        } else {
            const int c = (int)(i - nb_old);
            const int rows = n_old ? offs_old[upper_bound_i32(uniq_old, nb_old, uniq_new[c])] : 0;
            shift_new[c] = kept_before(kex, rows);
        }
    }
}

// Index pass: one thread per old row and per new row -> src, gid and key at its destination.  A destination outside [0, n_out) (only a
// caller whose n_kept is not the number of set `keep` bytes produces one) is not written.
__global__ void update_index_kernel(const int32_t *gid_old, const int32_t *uniq_old, const int32_t *offs_old, int nb_old, int n_old,
                                    const uint8_t *keep, const int32_t *kex, const int32_t *shift_old,
                                    const int32_t *perm_new, const int32_t *uniq_new, const int32_t *offs_new, const int32_t *nb_new_p,
                                    const int32_t *ids_new, const int32_t *shift_new, int m_new, long long n_out,
                                    int32_t *src_out, int32_t *gid_out, int32_t *key_out) {
    const int nb_new = m_new ? *nb_new_p : 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)n_old + m_new; i += (long long)gridDim.x * blockDim.x) {
        long long dst;
        int32_t src, id, key;
        if (i < n_old) {
            if (keep && !keep[i]) continue;
            const int b = min(max(upper_bound_i32(offs_old, nb_old + 1, (int32_t)i) - 1, 0), nb_old - 1);     // offs_old[b] <= i < offs_old[b + 1]
            dst = (long long)kept_before(kex, (int)i) + shift_old[b];
            src = (int32_t)i;
            id = gid_old[i];
            key = uniq_old[b];
        } else {
            const int t = (int)(i - n_old);
            const int c = min(max(upper_bound_i32(offs_new, nb_new + 1, t) - 1, 0), nb_new - 1);
            const int j = perm_new[t];
            dst = (long long)t + shift_new[c];
            src = ~j;
            id = ids_new[j];
            key = uniq_new[c];
        }
        if (dst >= 0 && dst < n_out) {
            src_out[dst] = src;
            gid_out[dst] = id;
            key_out[dst] = key;
        }
    }
}

// Row pass, output-driven: destination row p takes old sorted row src[p] (its inv_norm copied) or new row ~src[p] (zero-padded, its
// inv_norm computed as gather_rows_kernel computes it).  A row has 2^lg lanes, the smallest power of two that covers its float4s (64
// and the lane loop from 65 float4s on), so one wave-instruction moves 64 >> lg whole rows with 16 bytes per lane, and ROWS_IN_FLIGHT
// instructions' loads are issued before the first store.  Destination rows of one instruction are consecutive: the stores are one
// contiguous run, the old sources runs of a bucket's kept rows.
constexpr int ROWS_IN_FLIGHT = 4;

template <bool VEC>
__global__ __launch_bounds__(256) void update_rows_kernel(const float *sorted_old, long long stride_old, const float *inv_old, long long n_old,
                                                           const float *rows_new, long long stride_new, long long m_new, int d,
                                                           const int32_t *src, long long n_out, float *sorted_out, long long stride_out,
                                                           float *inv_out, int lg) {
    const int lane = threadIdx.x & 63;
    const int lanes = 1 << lg, g = lane & (lanes - 1), rows_per_inst = 64 >> lg;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const int d4 = (int)(stride_out >> 2);
    const long long step = (long long)rows_per_inst * ROWS_IN_FLIGHT;
    for (long long base = wave * step; base < n_out; base += nwaves * step) {      // wave-uniform: every lane reaches the butterfly
        const float *s[ROWS_IN_FLIGHT];
        long long p[ROWS_IN_FLIGHT];
        int32_t from[ROWS_IN_FLIGHT];
        float ss[ROWS_IN_FLIGHT];
#pragma unroll
        for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
            p[r] = base + (long long)r * rows_per_inst + (lane >> lg);
            from[r] = p[r] < n_out ? src[p[r]] : 0;
            // a source outside either side (a slot the index pass never wrote: see there) reads as an all-zero row
            const bool is_old = from[r] >= 0;
            const long long j = is_old ? (long long)from[r] : (long long)~from[r];
            const bool ok = p[r] < n_out && j < (is_old ? n_old : m_new);
            s[r] = !ok ? nullptr : is_old ? sorted_old + j * stride_old : rows_new + j * stride_new;
            ss[r] = 0.0f;
        }
        for (int c = g; c < d4; c += 64) {
            float4 v[ROWS_IN_FLIGHT];
#pragma unroll
            for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
                if (!s[r]) v[r] = make_float4(0, 0, 0, 0);
                else if (from[r] >= 0) v[r] = load_row_chunk<true>(s[r], c, d);
                else v[r] = load_row_chunk<VEC>(s[r], c, d);
            }
#pragma unroll
            for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
                if (p[r] < n_out) reinterpret_cast<float4 *>(sorted_out + p[r] * stride_out)[c] = v[r];
                ss[r] = sumsq_chain(v[r], ss[r]);
            }
        }
        if (inv_out) {
#pragma unroll
            for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
                const float total = sumsq_lanes(ss[r], lanes);
                if (g == 0 && p[r] < n_out) inv_out[p[r]] = (from[r] >= 0 && s[r]) ? inv_old[from[r]] : inv_norm_of(total);
            }
        }
    }
}

// ---- stored rows (NLSH_STORE_* and sq8): rows of float32 / float16 / uint8 elements in, rows of any storage out -----------------------
// The unit is the 4-element chunk of the float32 kernels above -- one float4 of the dequantised row, 16 / 8 / 4 bytes stored -- dealt to
// the lanes as there (chunk c to lane c % 64, or to lane c of the row's lane group), so a row's sum of squares is the same fmaf chain and
// the same butterfly over the same values: inv_norm has the bits the float32 kernels give on the dequantised rows.  A wider pitch only
// appends chunks of zeros to a lane's chain (fmaf(0, 0, ss) == ss: a sum of squares is never -0).
template <int STORE> struct StoreElem;
template <> struct StoreElem<NLSH_STORE_F32> { typedef float elem; typedef float4 word; };
template <> struct StoreElem<NLSH_STORE_F16> { typedef _Float16 elem; typedef uint2 word; };
template <> struct StoreElem<NLSH_STORE_U8> { typedef uint8_t elem; typedef uint32_t word; };

static int store_per16(int storage) { return storage == NLSH_STORE_F32 ? 4 : storage == NLSH_STORE_F16 ? 8 : 16; }   // elements per 16 bytes
// rows of `storage` elements at `base` with this stride: does every row start on a 4-element chunk boundary (16 / 8 / 4 bytes)?
static int store_vec_ok(const void *base, int storage, long long stride) {
    const uintptr_t chunk = storage == NLSH_STORE_F32 ? 16 : storage == NLSH_STORE_F16 ? 8 : 4;
    return ((stride & 3) == 0 && ((uintptr_t)base & (chunk - 1)) == 0) ? 1 : 0;
}
static bool store_ok(int storage) { return storage == NLSH_STORE_F32 || storage == NLSH_STORE_F16 || storage == NLSH_STORE_U8; }

// a stored chunk, dequantised (exact)
template <int DST> __device__ __forceinline__ float4 unpack_chunk(typename StoreElem<DST>::word w);
template <> __device__ __forceinline__ float4 unpack_chunk<NLSH_STORE_F32>(float4 w) { return w; }
template <> __device__ __forceinline__ float4 unpack_chunk<NLSH_STORE_F16>(uint2 w) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 lo = __builtin_bit_cast(h2, w.x), hi = __builtin_bit_cast(h2, w.y);
    return make_float4((float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y);
}
template <> __device__ __forceinline__ float4 unpack_chunk<NLSH_STORE_U8>(uint32_t w) {
    return make_float4((float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24));
}

// chunk c of a d-element row at `s` as float32 (exact), columns >= d zero.  `vec` (wave-uniform, decided on the host): the row starts on
// a chunk boundary of its own storage (16 / 8 / 4 bytes) and its stride is whole chunks, so a chunk that lies inside the row is ONE load
// of its stored word -- what gather_rows_kernel<true> does for float32; otherwise element loads, any alignment of the source.
template <int SRC>
__device__ __forceinline__ float4 load_chunk_as_f32(const void *row, int c, int d, bool vec) {
    const typename StoreElem<SRC>::elem *s = static_cast<const typename StoreElem<SRC>::elem *>(row);
    if (vec && c * 4 + 3 < d) return unpack_chunk<SRC>(*reinterpret_cast<const typename StoreElem<SRC>::word *>(s + c * 4));
    float4 v;
    v.x = c * 4 + 0 < d ? (float)s[c * 4 + 0] : 0.0f;
    v.y = c * 4 + 1 < d ? (float)s[c * 4 + 1] : 0.0f;
    v.z = c * 4 + 2 < d ? (float)s[c * 4 + 2] : 0.0f;
    v.w = c * 4 + 3 < d ? (float)s[c * 4 + 3] : 0.0f;
    return v;
}

// One value as storage DST holds it, dequantised again; `bad` is set when the value does not survive: float16 -- round to nearest even,
// a FINITE value that becomes an infinity is refused (infinities and NaNs pass as themselves); uint8 -- integers in [0, 255] only.
template <int DST>
__device__ __forceinline__ float requantise(float x, bool &bad) {
    if (DST == NLSH_STORE_F16) {
        const float y = (float)(_Float16)x;
        bad = bad || (__builtin_isinf(y) && !__builtin_isinf(x));
        return y;
    }
    if (DST == NLSH_STORE_U8) {
        const bool ok = x >= 0.0f && x <= 255.0f && x == truncf(x);   // a NaN fails the comparisons
        bad = bad || !ok;
        return ok ? fabsf(x) : 0.0f;                                  // -0 is stored as 0
    }
    return x;
}
template <int DST>
__device__ __forceinline__ float4 requantise4(float4 v, bool &bad) {
    return make_float4(requantise<DST>(v.x, bad), requantise<DST>(v.y, bad), requantise<DST>(v.z, bad), requantise<DST>(v.w, bad));
}

// a chunk of representable values as its stored word
template <int DST> __device__ __forceinline__ typename StoreElem<DST>::word pack_chunk(float4 v);
template <> __device__ __forceinline__ float4 pack_chunk<NLSH_STORE_F32>(float4 v) { return v; }
template <> __device__ __forceinline__ uint2 pack_chunk<NLSH_STORE_F16>(float4 v) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 lo, hi;
    lo.x = (_Float16)v.x; lo.y = (_Float16)v.y; hi.x = (_Float16)v.z; hi.y = (_Float16)v.w;
    return make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
}
template <> __device__ __forceinline__ uint32_t pack_chunk<NLSH_STORE_U8>(float4 v) {
    return (uint32_t)v.x | ((uint32_t)v.y << 8) | ((uint32_t)v.z << 16) | ((uint32_t)v.w << 24);
}

// the smallest row that held a value the destination storage cannot take (first_bad starts at -1 = 0xFFFFFFFF: unsigned minimum)
__device__ __forceinline__ void report_bad_row(int32_t *first_bad, bool bad, long long row) {
    if (first_bad && bad) atomicMin(reinterpret_cast<unsigned int *>(first_bad), (unsigned int)row);
}

// ---- the destination codec: how a row is held.  A codec gives the stored `word` of a chunk, `encode<SRC>` (chunk c of a d-element source
// row of storage SRC -> its word, with the float4 that word stands for beside it: the encoder has it in hand, and decode(pack(v)) of a
// uint8 word costs the gather four conversions the compiler cannot fold; sets `bad` when the row must be refused and `clamped` when a
// value saturated), `decode` (the word of chunk c -> that float4, for a pass that has only the stored row) and `counts_clamped` (are
// saturated rows counted?).  StoreCodec<DST> is the stateless one of NLSH_STORE_F32 / F16 / U8; Sq8Codec (sq8_rows.h) carries its
// quantiser.  The three row kernels below are written once on it.
template <class W> struct HeldChunk { W word; float4 values; };
template <int DST> struct StoreCodec {
    typedef typename StoreElem<DST>::word word;
    static constexpr bool counts_clamped = false;
    template <int SRC> __device__ __forceinline__ HeldChunk<word> encode(const void *row, int c, int d, bool vec, bool &bad, bool &) const {
        const float4 v = requantise4<DST>(load_chunk_as_f32<SRC>(row, c, d, vec), bad);
        return {pack_chunk<DST>(v), v};
    }
    __device__ __forceinline__ float4 decode(word w, int) const { return unpack_chunk<DST>(w); }
};

// One 16-byte unit of a row as the codec holds it: 1, 2 or 4 chunks, encoded from SRC elements.
template <int SRC, class Codec>
__device__ __forceinline__ uint4 encode_unit(const Codec &codec, const void *row, int u, int d, bool vec, bool &bad, bool &clamped) {
    constexpr int CHUNKS = 16 / (int)sizeof(typename Codec::word);
    struct { typename Codec::word w[CHUNKS]; } unit;
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) unit.w[j] = codec.template encode<SRC>(row, CHUNKS * u + j, d, vec, bad, clamped).word;
    return __builtin_bit_cast(uint4, unit);
}

// gather_rows_kernel between storages: one wavefront per destination row, chunk c of the row on lane c % 64.  The sum of squares runs over
// the values the stored words stand for, in that lane assignment and chain, so inv_norm has the bits nlsh_gather_rows gives on the
// dequantised rows.
template <int SRC, class Codec>
__global__ __launch_bounds__(256) void gather_rows_to_kernel(const void *corpus, long long src_stride, int d, const int32_t *perm, long long n,
                                                              void *sorted, long long dst_stride, float *inv_norm, int32_t *gid, int32_t id_base,
                                                              int32_t *first_bad, int vec, int32_t *clamped_rows, const Codec codec) {
    typedef typename StoreElem<SRC>::elem src_t;
    typedef typename Codec::word word_t;
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const int d4 = (int)(dst_stride >> 2);
    for (long long i = wave; i < n; i += nwaves) {
        const long long src = perm[i];
        const src_t *s = static_cast<const src_t *>(corpus) + src * src_stride;
        word_t *dst = static_cast<word_t *>(sorted) + i * (long long)d4;
        float ss = 0.0f;
        bool bad = false, clamped = false;
        for (int c = lane; c < d4; c += 64) {
            const HeldChunk<word_t> h = codec.template encode<SRC>(s, c, d, vec != 0, bad, clamped);
            dst[c] = h.word;
            ss = sumsq_chain(h.values, ss);
        }
        if (inv_norm) {
            ss = sumsq_lanes(ss, 64);
            if (lane == 0) inv_norm[i] = inv_norm_of(ss);
        }
        if (gid && lane == 0) gid[i] = (int32_t)src + id_base;
        report_bad_row(first_bad, bad, src);
        if (Codec::counts_clamped) {
            const bool row_clamped = __any(clamped) && !__any(bad);      // wave-uniform: the row is the wave's; a refused row is not counted
            if (clamped_rows && row_clamped && lane == 0) atomicAdd(clamped_rows, 1);
        }
    }
}

// update_rows_kernel on a stored index, generalised from "d floats" to "row bytes": the unit is 16 bytes of the stored row (strides in
// 16-byte units), a row has 2^lg lanes covering its units.  Kept rows are moved as bytes; new rows (NEW elements, any alignment) are
// encoded on the way in (columns >= d zero), the smallest new row that does not survive is reported and the saturated ones are counted.
// inv_norm is not this kernel's: a lane holds one, two or four chunks of a new row here, which is not the lane assignment the sum of
// squares is defined on -- update_inv_norm_of_kernel computes it from the rows this kernel wrote.
template <int NEW, class Codec>
__global__ __launch_bounds__(256) void update_rows_to_kernel(const uint4 *sorted_old, long long units_old, long long n_old,
                                                              const void *rows_new, long long stride_new, long long m_new, int d,
                                                              const int32_t *src, long long n_out, uint4 *sorted_out, long long units_out,
                                                              int lg, int32_t *first_bad, int vec, int32_t *clamped_rows, const Codec codec) {
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
            // a source outside either side (a slot the index pass never wrote: see there) reads as an all-zero row
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
                else if (sn[r]) w[r] = encode_unit<NEW>(codec, sn[r], u, d, vec != 0, bad[r], clamped[r]);
                else w[r] = make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int r = 0; r < ROWS_IN_FLIGHT; ++r)
                if (p[r] < n_out) sorted_out[p[r] * units_out + u] = w[r];
        }
#pragma unroll
        for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
            report_bad_row(first_bad, bad[r], (long long)~from[r]);
            if (Codec::counts_clamped) {
                const unsigned long long cm = __ballot(clamped[r] && !bad[r]), bm = __ballot(bad[r]);
                if (clamped_rows && g == 0 && (cm & group) && !(bm & group)) atomicAdd(clamped_rows, 1);    // one add per saturated row
            }
        }
    }
}

// inv_norm of the updated stored index: a kept row's value is copied (one lane per row, 64 consecutive rows per wave), a new row's is
// computed from the row update_rows_to_kernel stored -- by the whole wave, chunk c on lane c % 64, the 64-lane butterfly: the chain
// and the bits of gather_rows_to_kernel (and of the float32 kernels on the dequantised row).
template <class Codec>
__global__ __launch_bounds__(256) void update_inv_norm_of_kernel(const void *sorted_out, long long stride_out, const float *inv_old, long long n_old,
                                                                  const int32_t *src, long long n_out, float *inv_out, const Codec codec) {
    typedef typename Codec::word word_t;
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
            const word_t *row = static_cast<const word_t *>(sorted_out) + (p0 + l) * (long long)d4;
            float ss = 0.0f;
            for (int c = lane; c < d4; c += 64) ss = sumsq_chain(codec.decode(row[c], c), ss);
            ss = sumsq_lanes(ss, 64);
            if (lane == 0) inv_out[p0 + l] = inv_norm_of(ss);
        }
    }
}

__global__ void keep_flags_kernel(const uint8_t *keep, long long n, int32_t *flags) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        flags[i] = keep[i] ? 1 : 0;
}

// The scratch rocPRIM asks for is only known on a device (its size queries read the device's properties); the workspace size must be
// a pure function of the row counts (callers size buffers without one), so the region is BOUNDED here and nlsh_csr_update checks
// the real queries against the bound before it launches anything.  Radix sort of n (key, value) pairs: a second copy of both arrays,
// digit histograms and one look-back word per digit and block; scans: one look-back word per block.
static size_t sort_tmp_bound(size_t n) { return align_up(24 * n + (256u << 10)); }
static size_t scan_tmp_bound(size_t n) { return align_up(n / 4 + (64u << 10)); }

struct UpdateWs {
    size_t kex, shift_old, key_out, flags, rank;                             // old side and output: n_old + 1, nb_old, 3 x n_out
    size_t perm_n, uniq_n, offs_n, nb_n, shift_new, sk, iota, flags_n, rank_n;   // new side: the CSR of the m_new keys and its scratch
    size_t tmp, tmp_bytes, total;
};

static bool update_args_ok(long long n_old, long long nb_old, long long m_new) {
    return n_old >= 0 && n_old < (1ll << 31) && m_new >= 0 && m_new < (1ll << 31) && nb_old >= 0 && nb_old <= n_old;
}

static void update_layout(long long n_old, long long nb_old, long long m_new, UpdateWs *w) {
    long long n_out = n_old + m_new;         // rows written when nothing is removed
    if (n_out > 0x7FFFFFFFll) n_out = 0x7FFFFFFFll;
    const size_t a_old = align_up((size_t)(n_old + 1) * 4), a_nb = align_up((size_t)(nb_old + 1) * 4);
    const size_t a_out = align_up((size_t)(n_out + 1) * 4), a_new = align_up((size_t)(m_new + 1) * 4);
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += bytes; return here; };
    w->kex = take(a_old);
    w->shift_old = take(a_nb);
    w->key_out = take(a_out);
    w->flags = take(a_out);
    w->rank = take(a_out);
    w->perm_n = take(a_new);
    w->uniq_n = take(a_new);
    w->offs_n = take(a_new);
    w->nb_n = take(256);
    w->shift_new = take(a_new);
    w->sk = take(a_new);
    w->iota = take(a_new);
    w->flags_n = take(a_new);
    w->rank_n = take(a_new);
    const size_t t_sort = sort_tmp_bound((size_t)m_new), t_scan = scan_tmp_bound((size_t)(n_out > n_old ? n_out : n_old));
    w->tmp = at;
    w->tmp_bytes = t_sort > t_scan ? t_sort : t_scan;
    w->total = w->tmp + w->tmp_bytes;
}

}  // namespace nlsh

#include "sq8_rows.h"   // storage="sq8": its codec and training, built from the row helpers above

using namespace nlsh;

extern "C" size_t nlsh_build_csr_workspace(int64_t n) {
    if (n < 0) { set_error("build_csr_workspace: n=%lld", (long long)n); return 0; }
    CsrWs w;
    if (csr_layout(n, &w, nullptr) != NLSH_OK) return 0;
    return w.total;
}

extern "C" int nlsh_build_csr(const int32_t *keys, int64_t n, int32_t *perm, int32_t *uniq_keys, int32_t *offsets,
                              int32_t *n_buckets, void *workspace, size_t workspace_bytes, nlsh_stream_t stream) {
    NLSH_REQUIRE(n >= 0 && n < (1ll << 31), NLSH_E_INVALID, "build_csr: n=%lld", (long long)n);
    NLSH_REQUIRE(offsets && n_buckets, NLSH_E_INVALID, "build_csr: null output");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        NLSH_CHECK_HIP(hipMemsetAsync(offsets, 0, sizeof(int32_t), s));
        NLSH_CHECK_HIP(hipMemsetAsync(n_buckets, 0, sizeof(int32_t), s));
        return NLSH_OK;
    }
    NLSH_REQUIRE(keys && perm && uniq_keys && workspace, NLSH_E_INVALID, "build_csr: null pointer");
    CsrWs w;
    int rc = csr_layout(n, &w, s);
    if (rc != NLSH_OK) return rc;
    NLSH_REQUIRE(workspace_bytes >= w.total, NLSH_E_WORKSPACE, "build_csr: workspace %zu < %zu", workspace_bytes, w.total);
    NLSH_REQUIRE(((uintptr_t)workspace & 15) == 0, NLSH_E_INVALID, "build_csr: the workspace must be 16-byte aligned");
    char *base = (char *)workspace;
    int32_t *sk = (int32_t *)(base + w.sk), *iota = (int32_t *)(base + w.iota);
    int32_t *flags = (int32_t *)(base + w.flags), *rank = (int32_t *)(base + w.rank);
    return build_csr_on(keys, (long long)n, perm, uniq_keys, offsets, n_buckets, sk, iota, flags, rank, base + w.tmp, w.tmp_bytes, s);
}

extern "C" size_t nlsh_bucket_order_workspace(int64_t n_buckets) {
    if (n_buckets < 0) { set_error("bucket_order_workspace: n_buckets=%lld", (long long)n_buckets); return 0; }
    OrderWs w;
    if (order_layout(n_buckets, &w, nullptr) != NLSH_OK) return 0;
    return w.total;
}

extern "C" int nlsh_bucket_order(const int32_t *offsets, int64_t n_buckets, int32_t *order_out, void *workspace,
                                 size_t workspace_bytes, nlsh_stream_t stream) {
    NLSH_REQUIRE(n_buckets >= 0 && n_buckets < (1ll << 31), NLSH_E_INVALID, "bucket_order: n_buckets=%lld", (long long)n_buckets);
    if (n_buckets == 0) return NLSH_OK;
    NLSH_REQUIRE(offsets && order_out && workspace, NLSH_E_INVALID, "bucket_order: null pointer");
    hipStream_t s = (hipStream_t)stream;
    OrderWs w;
    int rc = order_layout(n_buckets, &w, s);
    if (rc != NLSH_OK) return rc;
    NLSH_REQUIRE(workspace_bytes >= w.total, NLSH_E_WORKSPACE, "bucket_order: workspace %zu < %zu", workspace_bytes, w.total);
    NLSH_REQUIRE(((uintptr_t)workspace & 15) == 0, NLSH_E_INVALID, "bucket_order: the workspace must be 16-byte aligned");
    char *base = (char *)workspace;
    uint32_t *sizes = (uint32_t *)(base + w.sizes), *sorted_sizes = (uint32_t *)(base + w.sorted_sizes);
    int32_t *idx = (int32_t *)(base + w.idx);
    int grid = (int)((n_buckets + 255) / 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(bucket_sizes_kernel, dim3(grid), dim3(256), 0, s, offsets, (long long)n_buckets, sizes, idx);
    size_t tb = w.tmp_bytes;
    // stable: buckets of equal size keep ascending key order -> the order is a pure function of the index
    NLSH_CHECK_HIP(rocprim::radix_sort_pairs_desc(base + w.tmp, tb, sizes, sorted_sizes, idx, order_out, (size_t)n_buckets, 0, 32, s));
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

struct CellWs {
    size_t flags, rank, tmp, tmp_bytes, order, total;
};
static int cell_layout(long long nb, CellWs *w, hipStream_t s) {
    const size_t n4 = align_up((size_t)(nb > 0 ? nb : 1) * 4);
    size_t t_scan = 0;
    int32_t *nul = nullptr;
    hipError_t e = rocprim::inclusive_scan(nullptr, t_scan, nul, nul, (size_t)nb, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) { set_error("rocprim::inclusive_scan size query: %s", hipGetErrorString(e)); return NLSH_E_HIP; }
    OrderWs ow;
    int rc = order_layout(nb, &ow, s);
    if (rc != NLSH_OK) return rc;
    w->flags = 0;
    w->rank = n4;
    w->tmp = 2 * n4;
    w->tmp_bytes = align_up(t_scan);
    w->order = w->tmp + w->tmp_bytes;
    w->total = w->order + ow.total;
    return NLSH_OK;
}

extern "C" size_t nlsh_build_cells_workspace(int64_t n_buckets) {
    if (n_buckets < 0) { set_error("build_cells_workspace: n_buckets=%lld", (long long)n_buckets); return 0; }
    CellWs w;
    if (cell_layout(n_buckets, &w, nullptr) != NLSH_OK) return 0;
    return w.total;
}

extern "C" int nlsh_build_cells(const int32_t *offsets, int64_t n_buckets, int window_rows, int32_t *cell_of, int32_t *cell_offsets,
                                int32_t *cell_order, int32_t *n_cells, void *workspace, size_t workspace_bytes, nlsh_stream_t stream) {
    NLSH_REQUIRE(n_buckets >= 0 && n_buckets < (1ll << 31), NLSH_E_INVALID, "build_cells: n_buckets=%lld", (long long)n_buckets);
    NLSH_REQUIRE(window_rows >= 1 && window_rows <= 256, NLSH_E_UNSUPPORTED, "build_cells: window_rows=%d not in [1,256] (one segment of the tiled scan)", window_rows);
    NLSH_REQUIRE(n_cells, NLSH_E_INVALID, "build_cells: null output");
    hipStream_t s = (hipStream_t)stream;
    if (n_buckets == 0) {
        NLSH_CHECK_HIP(hipMemsetAsync(n_cells, 0, sizeof(int32_t), s));
        return NLSH_OK;
    }
    NLSH_REQUIRE(offsets && cell_of && cell_offsets && cell_order && workspace, NLSH_E_INVALID, "build_cells: null pointer");
    CellWs w;
    int rc = cell_layout(n_buckets, &w, s);
    if (rc != NLSH_OK) return rc;
    NLSH_REQUIRE(workspace_bytes >= w.total, NLSH_E_WORKSPACE, "build_cells: workspace %zu < %zu", workspace_bytes, w.total);
    NLSH_REQUIRE(((uintptr_t)workspace & 15) == 0, NLSH_E_INVALID, "build_cells: the workspace must be 16-byte aligned");
    char *base = (char *)workspace;
    int32_t *flags = (int32_t *)(base + w.flags), *rank = (int32_t *)(base + w.rank);
    const long long spans = (n_buckets + CELL_SPAN - 1) / CELL_SPAN;
    hipLaunchKernelGGL(cell_flags_kernel, dim3((unsigned)((spans + 3) / 4)), dim3(256), 0, s, offsets, (long long)n_buckets, window_rows, flags);
    size_t tb = w.tmp_bytes;
    NLSH_CHECK_HIP(rocprim::inclusive_scan(base + w.tmp, tb, flags, rank, (size_t)n_buckets, rocprim::plus<int32_t>(), s));
    int grid = (int)((n_buckets + 256) / 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(emit_cells_kernel, dim3(grid), dim3(256), 0, s, offsets, flags, rank, (long long)n_buckets, cell_of, cell_offsets, n_cells);
    NLSH_CHECK_HIP(hipGetLastError());
    // schedule order of the cells: by descending rows over all n_buckets slots (the zero-row slots past the last cell sort behind
    // every real cell, so the first *n_cells entries are the order of the cells)
    return nlsh_bucket_order(cell_offsets, n_buckets, cell_order, base + w.order, workspace_bytes - w.order, stream);
}

extern "C" size_t nlsh_csr_update_workspace(int64_t n_old, int64_t n_buckets_old, int64_t m_new) {
    if (!update_args_ok(n_old, n_buckets_old, m_new)) {
        set_error("csr_update_workspace: n_old=%lld n_buckets_old=%lld m_new=%lld", (long long)n_old, (long long)n_buckets_old, (long long)m_new);
        return 0;
    }
    UpdateWs w;
    update_layout(n_old, n_buckets_old, m_new, &w);
    return w.total;
}

// ---- the row calls: nlsh_gather_rows / _typed / _sq8 and nlsh_csr_update / _typed / _sq8 are fill, check, run on one description ---------
// Start from `RowCall c = {}`.
struct RowCall {
    int d;
    // the rows that arrive: the corpus of a gather (n_src = n, picked by perm), the new rows of an update (n_src = m_new)
    const void *src; int src_storage; long long src_stride, n_src;
    // the rows that are written: `sorted` of a gather, `sorted_out` of an update (n_kept + m_new rows), with inv_norm and gid beside them
    void *dst; int dst_storage; long long dst_stride;
    float *inv_norm; int32_t *gid;
    // how they are held: the stateless codec of dst_storage, or (sq8; dst_storage is NLSH_STORE_U8 then) the codec of this quantiser
    bool sq8; const float *lo, *step;
    int32_t *first_bad, *clamped_rows;      // the optional flags of a conversion
    hipStream_t stream;
    // a gather only
    const int32_t *perm; int32_t id_base;
    // an update only: the index that is read, the new rows' keys and ids, the tables of the result, the workspace
    const void *old_rows; long long old_stride, n_old, nb_old, n_kept;
    const int32_t *gid_old; const float *inv_old; const int32_t *uniq_old, *offs_old; const uint8_t *keep;
    const int32_t *keys_new, *ids_new;
    int32_t *src_out, *uniq_out, *offsets_out, *n_buckets_out; void *workspace; size_t workspace_bytes;
};

// what an entry needs of the check
enum : unsigned {
    ROW_UPDATE = 1u,                // an update: the counts, the old index, the tables of the result and the workspace are held too
    ROW_SRC_ELEMENT_ALIGNED = 2u,   // the arriving rows are read with element loads: their pointer is held to its element size
};

// The one argument check of the six entries.  Nothing behind it runs, and no pointer is read, unless all of it passes.
static int row_call_check(const char *who, const RowCall &c, unsigned needs) {
    const bool upd = (needs & ROW_UPDATE) != 0;
    // the arguments under the names the entry's header gives them
    const char *src_storage = upd ? "new_storage" : "src_storage", *dst_storage = upd ? "storage" : "dst_storage";
    const char *src_rows = upd ? "rows_new / keys_new / ids_new" : "corpus / perm", *dst_rows = upd ? "sorted_out" : "sorted";
    const char *src_stride = upd ? "new_stride" : "src_stride", *dst_stride = upd ? "stride_out" : "dst_stride";
    const int d = c.d;
    NLSH_REQUIRE(store_ok(c.src_storage) && store_ok(c.dst_storage), NLSH_E_INVALID, "%s: %s=%d / %s=%d is none of NLSH_STORE_F32 / F16 / U8", who,
                 src_storage, c.src_storage, dst_storage, c.dst_storage);
    const int per16 = store_per16(c.dst_storage);
    // the quantiser: an update holds it whatever the counts, a gather of no rows looks at no pointer
    const bool quant = c.sq8 && (upd || c.n_src);
    NLSH_REQUIRE(!quant || (c.lo && c.step), NLSH_E_INVALID, "%s: lo / step is null", who);
    NLSH_REQUIRE(!quant || ((((uintptr_t)c.lo | (uintptr_t)c.step) & 15) == 0), NLSH_E_INVALID, "%s: lo and step must be 16-byte aligned", who);
    NLSH_REQUIRE(d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_INVALID, "%s: d=%d not in [1, NLSH_MAX_DIM = %d]", who, d, NLSH_MAX_DIM);
    long long n_dst = c.n_src;
    if (!upd) {
        NLSH_REQUIRE(c.n_src >= 0, NLSH_E_INVALID, "%s: n=%lld", who, c.n_src);
    } else {
        NLSH_REQUIRE(c.n_old >= 0 && c.n_old < (1ll << 31), NLSH_E_INVALID, "%s: n_old=%lld not in [0, 2^31)", who, c.n_old);
        NLSH_REQUIRE(c.nb_old >= 0 && c.nb_old <= c.n_old, NLSH_E_INVALID, "%s: n_buckets_old=%lld not in [0, n_old=%lld]", who, c.nb_old, c.n_old);
        NLSH_REQUIRE(c.n_src >= 0 && c.n_src < (1ll << 31), NLSH_E_INVALID, "%s: m_new=%lld not in [0, 2^31)", who, c.n_src);
        NLSH_REQUIRE(c.n_kept >= 0 && c.n_kept <= c.n_old, NLSH_E_INVALID, "%s: n_kept=%lld not in [0, n_old=%lld]", who, c.n_kept, c.n_old);
        NLSH_REQUIRE(c.keep || c.n_kept == c.n_old, NLSH_E_INVALID, "%s: keep is null (every row kept) but n_kept=%lld != n_old=%lld", who, c.n_kept, c.n_old);
        n_dst = c.n_kept + c.n_src;
        NLSH_REQUIRE(n_dst <= 0x7FFFFFFFll, NLSH_E_INVALID, "%s: n_kept + m_new = %lld rows > 2^31 - 1 (int32 row positions)", who, n_dst);
        NLSH_REQUIRE(c.offsets_out && c.n_buckets_out, NLSH_E_INVALID, "%s: offsets_out / n_buckets_out is null", who);
        if (c.n_old) {
            NLSH_REQUIRE(c.old_stride >= d && c.old_stride % per16 == 0, NLSH_E_INVALID, "%s: row_stride=%lld must be >= d=%d and a multiple of %d", who,
                         c.old_stride, d, per16);
            NLSH_REQUIRE(c.old_rows && c.gid_old && c.uniq_old && c.offs_old, NLSH_E_INVALID, "%s: corpus_sorted / gid / uniq_keys / offsets is null with n_old=%lld",
                         who, c.n_old);
            NLSH_REQUIRE(((uintptr_t)c.old_rows & 15) == 0, NLSH_E_INVALID, "%s: corpus_sorted must be 16-byte aligned", who);
            NLSH_REQUIRE(c.nb_old >= 1, NLSH_E_INVALID, "%s: n_buckets_old=0 with n_old=%lld rows", who, c.n_old);
        }
    }
    // a conversion must be able to report (a gather says so even for no rows)
    NLSH_REQUIRE(c.first_bad || c.src_storage == c.dst_storage || (upd && c.n_src == 0), NLSH_E_INVALID,
                 "%s: first_bad is null but the rows are converted (%s=%d, %s=%d)", who, src_storage, c.src_storage, dst_storage, c.dst_storage);
    if (c.n_src) {
        NLSH_REQUIRE(c.src && (upd ? c.keys_new && c.ids_new : c.perm != nullptr), NLSH_E_INVALID, "%s: %s is null", who, src_rows);
        NLSH_REQUIRE(c.src_stride >= d, NLSH_E_INVALID, "%s: %s=%lld < d=%d", who, src_stride, c.src_stride, d);
        NLSH_REQUIRE(!(needs & ROW_SRC_ELEMENT_ALIGNED) || ((uintptr_t)c.src & (c.src_storage == NLSH_STORE_F32 ? 3 : c.src_storage == NLSH_STORE_F16 ? 1 : 0)) == 0,
                     NLSH_E_INVALID, "%s: %s is not aligned to its element size", who, upd ? "rows_new" : "corpus");
    }
    if (n_dst) {
        NLSH_REQUIRE(c.dst && (!upd || (c.gid && c.src_out && c.uniq_out)), NLSH_E_INVALID, "%s: %s is null", who, upd ? "sorted_out / gid_out / src_out / uniq_out" : dst_rows);
        NLSH_REQUIRE(c.dst_stride >= d && c.dst_stride % per16 == 0, NLSH_E_INVALID, "%s: %s=%lld must be >= d=%d and a multiple of %d elements (a pitch of 16-byte units)",
                     who, dst_stride, c.dst_stride, d, per16);
        NLSH_REQUIRE(((uintptr_t)c.dst & 15) == 0, NLSH_E_INVALID, "%s: %s must be 16-byte aligned", who, dst_rows);
    }
    if (upd && n_dst) {
        NLSH_REQUIRE(!c.inv_norm || c.inv_old || c.n_kept == 0, NLSH_E_INVALID, "%s: inv_norm_out is wanted but inv_norm (the kept rows') is null", who);
        NLSH_REQUIRE(c.workspace, NLSH_E_INVALID, "%s: workspace is null", who);
        NLSH_REQUIRE(((uintptr_t)c.workspace & 15) == 0, NLSH_E_INVALID, "%s: the workspace must be 16-byte aligned", who);
        UpdateWs w;
        update_layout(c.n_old, c.nb_old, c.n_src, &w);
        NLSH_REQUIRE(c.workspace_bytes >= w.total, NLSH_E_INVALID, "%s: workspace_bytes=%zu < nlsh_csr_update_workspace = %zu", who, c.workspace_bytes, w.total);
    }
    return NLSH_OK;
}

struct RowKernels { const void *gather, *update, *inv_norm; };
static RowKernels row_kernels(const RowCall &c);      // defined behind the two calls: the float32 kernels keep their place in the code object

// -1: every row survived its conversion; 0 saturated rows
static int row_flags_clear(const RowCall &c) {
    if (c.first_bad) NLSH_CHECK_HIP(hipMemsetAsync(c.first_bad, 0xFF, sizeof(int32_t), c.stream));
    if (c.clamped_rows) NLSH_CHECK_HIP(hipMemsetAsync(c.clamped_rows, 0, sizeof(int32_t), c.stream));
    return NLSH_OK;
}

static int gather_call(const char *who, RowCall c, unsigned needs) {
    int rc = row_call_check(who, c, needs);
    if (rc != NLSH_OK || (rc = row_flags_clear(c)) != NLSH_OK || c.n_src == 0) return rc;
    hipStream_t s = c.stream;
    long long blocks = (c.n_src + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    int vec = store_vec_ok(c.src, c.src_storage, c.src_stride);      // rows on chunk boundaries of their storage: one load per chunk
    const RowKernels k = row_kernels(c);
    if (!k.gather) {
        const float *corpus = (const float *)c.src;
        float *sorted = (float *)c.dst;
        if (vec)
            hipLaunchKernelGGL(gather_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, corpus, c.src_stride, c.d, c.perm, c.n_src, sorted,
                               c.dst_stride, c.inv_norm, c.gid, c.id_base);
        else
            hipLaunchKernelGGL(gather_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, corpus, c.src_stride, c.d, c.perm, c.n_src, sorted,
                               c.dst_stride, c.inv_norm, c.gid, c.id_base);
    } else {
        Sq8Codec codec = {(const float4 *)c.lo, (const float4 *)c.step};     // a stateless codec is an empty argument: nothing of this is read
        void *argv[] = {&c.src, &c.src_stride, &c.d, &c.perm, &c.n_src, &c.dst, &c.dst_stride, &c.inv_norm, &c.gid, &c.id_base, &c.first_bad, &vec,
                        &c.clamped_rows, &codec};
        NLSH_CHECK_HIP(hipLaunchKernel(k.gather, dim3((unsigned)blocks), dim3(256), argv, 0, s));
    }
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

static int update_call(const char *who, RowCall c) {
    int rc = row_call_check(who, c, ROW_UPDATE);
    if (rc != NLSH_OK || (rc = row_flags_clear(c)) != NLSH_OK) return rc;
    hipStream_t s = c.stream;
    long long n_old = c.n_old, m_new = c.n_src, n_out = c.n_kept + c.n_src;
    if (n_out == 0) {
        NLSH_CHECK_HIP(hipMemsetAsync(c.offsets_out, 0, sizeof(int32_t), s));
        NLSH_CHECK_HIP(hipMemsetAsync(c.n_buckets_out, 0, sizeof(int32_t), s));
        return NLSH_OK;
    }
    UpdateWs w;
    update_layout(n_old, c.nb_old, m_new, &w);
    char *base = (char *)c.workspace;
    int32_t *kex = c.keep ? (int32_t *)(base + w.kex) : nullptr, *shift_old = (int32_t *)(base + w.shift_old);
    int32_t *key_out = (int32_t *)(base + w.key_out), *flags = (int32_t *)(base + w.flags), *rank = (int32_t *)(base + w.rank);
    int32_t *perm_n = (int32_t *)(base + w.perm_n), *uniq_n = (int32_t *)(base + w.uniq_n), *offs_n = (int32_t *)(base + w.offs_n);
    int32_t *nb_n = (int32_t *)(base + w.nb_n), *shift_new = (int32_t *)(base + w.shift_new);
    void *tmp = base + w.tmp;
    int32_t *nul = nullptr;
    const size_t n_scan = (size_t)(n_out > n_old ? n_out : n_old);
    size_t t_sort = 0, t_scan = 0;      // what rocPRIM really asks for on this device, against the bound the workspace was sized by
    if (m_new) NLSH_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t_sort, nul, nul, nul, nul, (size_t)m_new, 0, 32, s));
    NLSH_CHECK_HIP(rocprim::inclusive_scan(nullptr, t_scan, nul, nul, n_scan, rocprim::plus<int32_t>(), s));
    NLSH_REQUIRE(t_sort <= w.tmp_bytes && t_scan <= w.tmp_bytes, NLSH_E_WORKSPACE, "%s: rocPRIM scratch (sort %zu, scan %zu bytes) exceeds the %zu bytes "
                 "the workspace formula reserves for it", who, t_sort, t_scan, w.tmp_bytes);
    auto grid_of = [](long long n) { long long g = (n + 255) / 256; return dim3((unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g)); };
    if (m_new) {
        rc = build_csr_on(c.keys_new, m_new, perm_n, uniq_n, offs_n, nb_n, (int32_t *)(base + w.sk), (int32_t *)(base + w.iota),
                          (int32_t *)(base + w.flags_n), (int32_t *)(base + w.rank_n), tmp, w.tmp_bytes, s);
        if (rc != NLSH_OK) return rc;
    }
    if (c.keep) {         // kex[0] = 0, kex[i + 1] = keep[0] + ... + keep[i]
        hipLaunchKernelGGL(keep_flags_kernel, grid_of(n_old), dim3(256), 0, s, c.keep, n_old, flags);
        NLSH_CHECK_HIP(hipMemsetAsync(kex, 0, sizeof(int32_t), s));
        size_t tb = w.tmp_bytes;
        NLSH_CHECK_HIP(rocprim::inclusive_scan(tmp, tb, flags, kex + 1, (size_t)n_old, rocprim::plus<int32_t>(), s));
    }
    hipLaunchKernelGGL(update_shifts_kernel, grid_of(c.nb_old + m_new), dim3(256), 0, s, c.uniq_old, c.offs_old, (int)c.nb_old, (int)n_old, kex,
                       uniq_n, offs_n, nb_n, (int)m_new, shift_old, shift_new);
    hipLaunchKernelGGL(update_index_kernel, grid_of(n_old + m_new), dim3(256), 0, s, c.gid_old, c.uniq_old, c.offs_old, (int)c.nb_old, (int)n_old, c.keep, kex,
                       shift_old, perm_n, uniq_n, offs_n, nb_n, c.ids_new, shift_new, (int)m_new, n_out, c.src_out, c.gid, key_out);
    // the bucket table of the result: the run-length encoding of the keys at their destinations (emptied buckets vanish, new ones appear)
    hipLaunchKernelGGL(head_flags_kernel, grid_of(n_out), dim3(256), 0, s, key_out, n_out, flags);
    size_t tb = w.tmp_bytes;
    NLSH_CHECK_HIP(rocprim::inclusive_scan(tmp, tb, flags, rank, (size_t)n_out, rocprim::plus<int32_t>(), s));
    hipLaunchKernelGGL(emit_buckets_kernel, grid_of(n_out), dim3(256), 0, s, key_out, flags, rank, n_out, c.uniq_out, c.offsets_out, c.n_buckets_out);
    // the rows: 2^lg lanes per row of `units` 16-byte units (float32 rows into a float32 index: of float4s), ROWS_IN_FLIGHT rows per lane group
    const RowKernels k = row_kernels(c);
    const int per16 = store_per16(c.dst_storage);
    long long units_old = c.old_stride / per16, units_out = k.update ? c.dst_stride / per16 : c.dst_stride >> 2;
    int lg = 0;
    while ((1 << lg) < units_out && lg < 6) ++lg;
    const long long rows_per_wave = (long long)(64 >> lg) * ROWS_IN_FLIGHT;
    long long blocks = ((n_out + rows_per_wave - 1) / rows_per_wave + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;
    int vec = store_vec_ok(c.src, c.src_storage, c.src_stride);      // new rows on chunk boundaries of their storage: one load per chunk
    if (!k.update) {      // one pass, inv_norm fused
        const float *old_f = (const float *)c.old_rows, *new_f = (const float *)c.src;
        float *out_f = (float *)c.dst;
        if (vec)
            hipLaunchKernelGGL(update_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, old_f, c.old_stride, c.inv_old, n_old, new_f, c.src_stride,
                               m_new, c.d, c.src_out, n_out, out_f, c.dst_stride, c.inv_norm, lg);
        else
            hipLaunchKernelGGL(update_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, old_f, c.old_stride, c.inv_old, n_old, new_f, c.src_stride,
                               m_new, c.d, c.src_out, n_out, out_f, c.dst_stride, c.inv_norm, lg);
    } else {              // the row pass in 16-byte units, then the inv_norm pass over what it wrote
        Sq8Codec codec = {(const float4 *)c.lo, (const float4 *)c.step};     // a stateless codec is an empty argument: nothing of this is read
        void *argv[] = {&c.old_rows, &units_old, &n_old, &c.src, &c.src_stride, &m_new, &c.d, &c.src_out, &n_out, &c.dst, &units_out, &lg, &c.first_bad, &vec,
                        &c.clamped_rows, &codec};
        NLSH_CHECK_HIP(hipLaunchKernel(k.update, dim3((unsigned)blocks), dim3(256), argv, 0, s));
        if (c.inv_norm) {
            long long iblocks = ((n_out + 63) / 64 + 3) / 4;
            if (iblocks > 256 * 8) iblocks = 256 * 8;
            void *argi[] = {&c.dst, &c.dst_stride, &c.inv_old, &n_old, &c.src_out, &n_out, &c.inv_norm, &codec};
            NLSH_CHECK_HIP(hipLaunchKernel(k.inv_norm, dim3((unsigned)iblocks), dim3(256), argi, 0, s));
        }
    }
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

// The one place a (source storage, destination codec) pair becomes kernels.  Float32 rows into a float32 index have none here: they
// are gather_rows_kernel's and update_rows_kernel's.
template <int SRC, class Codec> static RowKernels row_kernels_of() {
    return {(const void *)gather_rows_to_kernel<SRC, Codec>, (const void *)update_rows_to_kernel<SRC, Codec>, (const void *)update_inv_norm_of_kernel<Codec>};
}
template <> RowKernels row_kernels_of<NLSH_STORE_F32, StoreCodec<NLSH_STORE_F32>>() { return {nullptr, nullptr, nullptr}; }
template <class Codec> static RowKernels row_kernels_to(int src_storage) {
    return src_storage == NLSH_STORE_F32 ? row_kernels_of<NLSH_STORE_F32, Codec>()
         : src_storage == NLSH_STORE_F16 ? row_kernels_of<NLSH_STORE_F16, Codec>() : row_kernels_of<NLSH_STORE_U8, Codec>();
}
static RowKernels row_kernels(const RowCall &c) {
    if (c.sq8) return row_kernels_to<Sq8Codec>(c.src_storage);
    return c.dst_storage == NLSH_STORE_F32 ? row_kernels_to<StoreCodec<NLSH_STORE_F32>>(c.src_storage)
         : c.dst_storage == NLSH_STORE_F16 ? row_kernels_to<StoreCodec<NLSH_STORE_F16>>(c.src_storage) : row_kernels_to<StoreCodec<NLSH_STORE_U8>>(c.src_storage);
}

// The descriptor of a gather / of an update with what their three entries all have, under the header's parameter names.
#define NLSH_GATHER_CALL(c)                                                                                                          \
    RowCall c = {};                                                                                                                  \
    c.d = d; c.src = corpus; c.src_stride = src_stride; c.n_src = n; c.perm = perm; c.dst = sorted; c.dst_stride = dst_stride;      \
    c.inv_norm = inv_norm; c.gid = gid; c.id_base = id_base; c.stream = (hipStream_t)stream
#define NLSH_UPDATE_CALL(c)                                                                                                          \
    RowCall c = {};                                                                                                                  \
    c.d = d; c.src = rows_new; c.src_stride = new_stride; c.n_src = m_new; c.keys_new = keys_new; c.ids_new = ids_new;              \
    c.old_rows = corpus_sorted; c.old_stride = row_stride; c.n_old = n_old; c.nb_old = n_buckets_old; c.n_kept = n_kept; c.keep = keep; \
    c.gid_old = gid; c.inv_old = inv_norm; c.uniq_old = uniq_keys; c.offs_old = offsets;                                             \
    c.dst = sorted_out; c.dst_stride = stride_out; c.gid = gid_out; c.inv_norm = inv_norm_out; c.src_out = src_out; c.uniq_out = uniq_out; \
    c.offsets_out = offsets_out; c.n_buckets_out = n_buckets_out; c.workspace = workspace; c.workspace_bytes = workspace_bytes;     \
    c.stream = (hipStream_t)stream

extern "C" int nlsh_gather_rows(const float *corpus, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                                float *sorted, int64_t dst_stride, float *inv_norm, int32_t *gid, int32_t id_base,
                                nlsh_stream_t stream) {
    NLSH_GATHER_CALL(c);
    c.src_storage = c.dst_storage = NLSH_STORE_F32;
    return gather_call("gather_rows", c, 0);      // any alignment of `corpus`, as ever
}

extern "C" int nlsh_gather_rows_typed(const void *corpus, int src_storage, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                                      void *sorted, int dst_storage, int64_t dst_stride, float *inv_norm, int32_t *gid, int32_t id_base,
                                      int32_t *first_bad, nlsh_stream_t stream) {
    NLSH_GATHER_CALL(c);
    c.src_storage = src_storage; c.dst_storage = dst_storage; c.first_bad = first_bad;
    return gather_call("gather_rows_typed", c, ROW_SRC_ELEMENT_ALIGNED);
}

extern "C" int nlsh_gather_rows_sq8(const void *corpus, int src_storage, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                                    uint8_t *sorted, int64_t dst_stride, const float *lo, const float *step, float *inv_norm, int32_t *gid,
                                    int32_t id_base, int32_t *first_bad, int32_t *clamped_rows, nlsh_stream_t stream) {
    NLSH_GATHER_CALL(c);
    c.src_storage = src_storage; c.dst_storage = NLSH_STORE_U8; c.first_bad = first_bad;
    c.sq8 = true; c.lo = lo; c.step = step; c.clamped_rows = clamped_rows;
    return gather_call("gather_rows_sq8", c, ROW_SRC_ELEMENT_ALIGNED);
}

extern "C" int nlsh_csr_update(const float *corpus_sorted, int64_t row_stride, int d, const int32_t *gid, const float *inv_norm,
                               const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                               const uint8_t *keep, int64_t n_kept,
                               const float *rows_new, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new, int64_t m_new,
                               float *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                               int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out,
                               void *workspace, size_t workspace_bytes, nlsh_stream_t stream) {
    NLSH_UPDATE_CALL(c);
    c.src_storage = c.dst_storage = NLSH_STORE_F32;
    return update_call("csr_update", c);
}

// `storage` = elements of corpus_sorted and sorted_out (strides in elements), `new_storage` = elements of rows_new
extern "C" int nlsh_csr_update_typed(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid, const float *inv_norm,
                                     const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                                     const uint8_t *keep, int64_t n_kept,
                                     const void *rows_new, int new_storage, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new,
                                     int64_t m_new,
                                     void *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                                     int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out, int32_t *first_bad,
                                     void *workspace, size_t workspace_bytes, nlsh_stream_t stream) {
    NLSH_UPDATE_CALL(c);
    c.src_storage = new_storage; c.dst_storage = storage; c.first_bad = first_bad;
    return update_call("csr_update", c);
}

extern "C" int nlsh_csr_update_sq8(const uint8_t *corpus_sorted, const float *lo, const float *step, int64_t row_stride, int d, const int32_t *gid,
                                   const float *inv_norm, const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                                   const uint8_t *keep, int64_t n_kept,
                                   const void *rows_new, int new_storage, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new,
                                   int64_t m_new,
                                   uint8_t *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                                   int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out, int32_t *first_bad, int32_t *clamped_rows,
                                   void *workspace, size_t workspace_bytes, nlsh_stream_t stream) {
    // one quantiser serves both sides: its arrays cover the wider of the two pitches only if the caller made them so
    NLSH_REQUIRE(n_old == 0 || m_new == 0 || n_kept + m_new == 0 || row_stride == stride_out, NLSH_E_INVALID,
                 "csr_update_sq8: row_stride=%lld != stride_out=%lld (lo and step are padded to ONE pitch)", (long long)row_stride, (long long)stride_out);
    NLSH_UPDATE_CALL(c);
    c.src_storage = new_storage; c.dst_storage = NLSH_STORE_U8; c.first_bad = first_bad;
    c.sq8 = true; c.lo = lo; c.step = step; c.clamped_rows = clamped_rows;
    return update_call("csr_update", c);
}

// ---- storage="sq8" (sq8_rows.h): training the quantiser
static bool sq8_source_ok(int storage) { return storage == NLSH_STORE_F32 || storage == NLSH_STORE_F16; }

extern "C" size_t nlsh_sq8_train_workspace(int64_t n, int d) {
    if (n < 0 || d < 1 || d > NLSH_MAX_DIM) { set_error("sq8_train_workspace: n=%lld d=%d", (long long)n, d); return 0; }
    int lgw, blocks;
    sq8_train_shape(n, d, &lgw, &blocks);
    return align_up((size_t)blocks * 2 * ((size_t)16 << lgw));
}

extern "C" int nlsh_sq8_train(const void *rows, int storage, int64_t row_stride, int d, int64_t n, float *lo, float *step, int64_t quant_stride,
                              int32_t *first_bad, void *workspace, size_t workspace_bytes, nlsh_stream_t stream) {
    NLSH_REQUIRE(sq8_source_ok(storage), NLSH_E_INVALID, "sq8_train: storage=%d is neither NLSH_STORE_F32 nor NLSH_STORE_F16", storage);
    NLSH_REQUIRE(n >= 0 && d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_INVALID, "sq8_train: n=%lld d=%d", (long long)n, d);
    NLSH_REQUIRE(quant_stride >= d, NLSH_E_INVALID, "sq8_train: quant_stride=%lld < d=%d", (long long)quant_stride, d);
    NLSH_REQUIRE(lo && step && first_bad, NLSH_E_INVALID, "sq8_train: lo / step / first_bad is null");
    int lgw, blocks;
    sq8_train_shape(n, d, &lgw, &blocks);
    if (n) {
        NLSH_REQUIRE(rows && workspace, NLSH_E_INVALID, "sq8_train: rows / workspace is null");
        NLSH_REQUIRE(row_stride >= d, NLSH_E_INVALID, "sq8_train: row_stride=%lld < d=%d", (long long)row_stride, d);
        NLSH_REQUIRE(((uintptr_t)rows & (storage == NLSH_STORE_F32 ? 3 : 1)) == 0, NLSH_E_INVALID, "sq8_train: rows is not aligned to its element size");
        NLSH_REQUIRE(((uintptr_t)workspace & 15) == 0, NLSH_E_INVALID, "sq8_train: the workspace must be 16-byte aligned");
        NLSH_REQUIRE(workspace_bytes >= nlsh_sq8_train_workspace(n, d), NLSH_E_WORKSPACE, "sq8_train: workspace %zu < %zu", workspace_bytes,
                     nlsh_sq8_train_workspace(n, d));
    }
    hipStream_t s = (hipStream_t)stream;
    NLSH_CHECK_HIP(hipMemsetAsync(first_bad, 0xFF, sizeof(int32_t), s));   // -1: every row is finite
    long long rs = row_stride, nn = n, qs = quant_stride;
    if (n) {
        int vec = store_vec_ok(rows, storage, row_stride);
        const void *fn = storage == NLSH_STORE_F32 ? (const void *)sq8_train_partial_kernel<NLSH_STORE_F32> : (const void *)sq8_train_partial_kernel<NLSH_STORE_F16>;
        void *argv[] = {&rows, &rs, &d, &nn, &lgw, &workspace, &first_bad, &vec};
        NLSH_CHECK_HIP(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), argv, 0, s));
    }
    const float *part = (const float *)workspace;
    hipLaunchKernelGGL(sq8_train_final_kernel, dim3((unsigned)((quant_stride + 15) / 16)), dim3(256), 0, s, part, blocks, lgw, d, nn, lo, step, qs);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}
