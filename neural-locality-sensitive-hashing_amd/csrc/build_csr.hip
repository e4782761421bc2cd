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

// ---- typed storage (NLSH_STORE_*): rows of float32 / float16 / uint8 elements in, rows of any of the three out -------------------------
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

// gather_rows_kernel between storages: one wavefront per destination row, chunk c of the row on lane c % 64.
template <int SRC, int DST>
__global__ __launch_bounds__(256) void gather_rows_typed_kernel(const void *corpus, long long src_stride, int d, const int32_t *perm, long long n,
                                                                 void *sorted, long long dst_stride, float *inv_norm, int32_t *gid, int32_t id_base,
                                                                 int32_t *first_bad, int vec) {
    typedef typename StoreElem<SRC>::elem src_t;
    typedef typename StoreElem<DST>::word word_t;
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const int d4 = (int)(dst_stride >> 2);
    for (long long i = wave; i < n; i += nwaves) {
        const long long src = perm[i];
        const src_t *s = static_cast<const src_t *>(corpus) + src * src_stride;
        word_t *dst = static_cast<word_t *>(sorted) + i * (long long)d4;
        float ss = 0.0f;
        bool bad = false;
        for (int c = lane; c < d4; c += 64) {
            const float4 v = requantise4<DST>(load_chunk_as_f32<SRC>(s, c, d, vec != 0), bad);
            dst[c] = pack_chunk<DST>(v);
            ss = sumsq_chain(v, ss);
        }
        if (inv_norm) {
            ss = sumsq_lanes(ss, 64);
            if (lane == 0) inv_norm[i] = inv_norm_of(ss);
        }
        if (gid && lane == 0) gid[i] = (int32_t)src + id_base;
        report_bad_row(first_bad, bad, src);
    }
}

// One 16-byte unit of a new row (E = 4 / 8 / 16 elements of storage DST = E / 4 chunks), converted from NEW elements.
template <int NEW, int DST>
__device__ __forceinline__ uint4 convert_unit(const void *row, int u, int d, bool vec, bool &bad) {
    if (DST == NLSH_STORE_F32) {
        const float4 v = requantise4<NLSH_STORE_F32>(load_chunk_as_f32<NEW>(row, u, d, vec), bad);
        return __builtin_bit_cast(uint4, v);
    } else if (DST == NLSH_STORE_F16) {
        const uint2 a = pack_chunk<NLSH_STORE_F16>(requantise4<NLSH_STORE_F16>(load_chunk_as_f32<NEW>(row, 2 * u, d, vec), bad));
        const uint2 b = pack_chunk<NLSH_STORE_F16>(requantise4<NLSH_STORE_F16>(load_chunk_as_f32<NEW>(row, 2 * u + 1, d, vec), bad));
        return make_uint4(a.x, a.y, b.x, b.y);
    } else {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = pack_chunk<NLSH_STORE_U8>(requantise4<NLSH_STORE_U8>(load_chunk_as_f32<NEW>(row, 4 * u + j, d, vec), bad));
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// update_rows_kernel on a typed index, generalised from "d floats" to "row bytes": the unit is 16 bytes of the stored row (strides in
// 16-byte units), a row has 2^lg lanes covering its units.  Kept rows are moved as bytes; new rows (NEW elements, any alignment) are
// converted on the way in (columns >= d zero) and the smallest new row that does not survive is reported.  inv_norm is not this
// kernel's: a lane holds one, two or four chunks of a new row here, which is not the lane assignment the sum of squares is defined
// on -- update_inv_norm_typed_kernel computes it from the rows this kernel wrote.
template <int NEW, int DST>
__global__ __launch_bounds__(256) void update_rows_typed_kernel(const uint4 *sorted_old, long long units_old, long long n_old,
                                                                 const void *rows_new, long long stride_new, long long m_new, int d,
                                                                 const int32_t *src, long long n_out, uint4 *sorted_out, long long units_out,
                                                                 int lg, int32_t *first_bad, int vec) {
    typedef typename StoreElem<NEW>::elem new_t;
    const int lane = threadIdx.x & 63;
    const int lanes = 1 << lg, g = lane & (lanes - 1), rows_per_inst = 64 >> lg;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long step = (long long)rows_per_inst * ROWS_IN_FLIGHT;
    for (long long base = wave * step; base < n_out; base += nwaves * step) {
        const uint4 *so[ROWS_IN_FLIGHT];
        const new_t *sn[ROWS_IN_FLIGHT];
        long long p[ROWS_IN_FLIGHT];
        int32_t from[ROWS_IN_FLIGHT];
        bool bad[ROWS_IN_FLIGHT];
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
            bad[r] = false;
        }
        for (int u = g; u < units_out; u += 64) {
            uint4 w[ROWS_IN_FLIGHT];
#pragma unroll
            for (int r = 0; r < ROWS_IN_FLIGHT; ++r) {
                if (so[r]) w[r] = u < units_old ? so[r][u] : make_uint4(0u, 0u, 0u, 0u);
                else if (sn[r]) w[r] = convert_unit<NEW, DST>(sn[r], u, d, vec != 0, bad[r]);
                else w[r] = make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int r = 0; r < ROWS_IN_FLIGHT; ++r)
                if (p[r] < n_out) sorted_out[p[r] * units_out + u] = w[r];
        }
#pragma unroll
        for (int r = 0; r < ROWS_IN_FLIGHT; ++r) report_bad_row(first_bad, bad[r], (long long)~from[r]);
    }
}

// inv_norm of the updated typed index: a kept row's value is copied (one lane per row, 64 consecutive rows per wave), a new row's is
// computed from the row update_rows_typed_kernel stored -- by the whole wave, chunk c on lane c % 64, the 64-lane butterfly: the chain
// and the bits of gather_rows_typed_kernel (and of the float32 kernels on the dequantised row).
template <int DST>
__global__ __launch_bounds__(256) void update_inv_norm_typed_kernel(const void *sorted_out, long long stride_out, const float *inv_old, long long n_old,
                                                                     const int32_t *src, long long n_out, float *inv_out) {
    typedef typename StoreElem<DST>::word word_t;
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
            for (int c = lane; c < d4; c += 64) ss = sumsq_chain(unpack_chunk<DST>(row[c]), ss);
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

#include "sq8_rows.h"   // storage="sq8": training, the encoding gather and the update passes, built from the row helpers above

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

extern "C" int nlsh_gather_rows(const float *corpus, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                                float *sorted, int64_t dst_stride, float *inv_norm, int32_t *gid, int32_t id_base,
                                nlsh_stream_t stream) {
    NLSH_REQUIRE(n >= 0 && d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_INVALID, "gather_rows: n=%lld d=%d", (long long)n, d);
    if (n == 0) return NLSH_OK;
    NLSH_REQUIRE(corpus && perm && sorted, NLSH_E_INVALID, "gather_rows: null pointer");
    NLSH_REQUIRE(dst_stride >= d && (dst_stride & 3) == 0 && ((uintptr_t)sorted & 15) == 0, NLSH_E_INVALID,
                 "gather_rows: dst_stride=%lld must be >= d, a multiple of 4, and `sorted` 16-byte aligned", (long long)dst_stride);
    NLSH_REQUIRE(src_stride >= d, NLSH_E_INVALID, "gather_rows: src_stride < d");
    hipStream_t s = (hipStream_t)stream;
    long long blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    bool vec = ((src_stride & 3) == 0) && (((uintptr_t)corpus & 15) == 0);
    if (vec)
        hipLaunchKernelGGL(gather_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, corpus, (long long)src_stride, d, perm,
                           (long long)n, sorted, (long long)dst_stride, inv_norm, gid, id_base);
    else
        hipLaunchKernelGGL(gather_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, corpus, (long long)src_stride, d, perm,
                           (long long)n, sorted, (long long)dst_stride, inv_norm, gid, id_base);
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
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

// nlsh_csr_update and nlsh_csr_update_typed: `storage` = elements of corpus_sorted and sorted_out (strides in elements), `new_storage` =
// elements of rows_new; float32 on both sides is the float32 row kernel, untouched.
static int csr_update_impl(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid, const float *inv_norm,
                           const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                           const uint8_t *keep, int64_t n_kept,
                           const void *rows_new, int new_storage, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new, int64_t m_new,
                           void *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                           int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out, int32_t *first_bad,
                           void *workspace, size_t workspace_bytes, nlsh_stream_t stream,
                           bool sq8 = false, const float *lo = nullptr, const float *step = nullptr, int32_t *clamped_rows = nullptr) {
    // ---- host checks: nothing below them runs, and no pointer is read, unless all of them pass
    NLSH_REQUIRE(store_ok(storage) && store_ok(new_storage), NLSH_E_INVALID, "csr_update: storage=%d / new_storage=%d is none of NLSH_STORE_F32 / F16 / U8",
                 storage, new_storage);
    // nlsh_csr_update_sq8: the uint8 layout (storage is NLSH_STORE_U8) with the quantiser the new rows are encoded and the norms decoded by
    NLSH_REQUIRE(!sq8 || (lo && step), NLSH_E_INVALID, "csr_update: lo / step is null");
    NLSH_REQUIRE(!sq8 || ((((uintptr_t)lo | (uintptr_t)step) & 15) == 0), NLSH_E_INVALID, "csr_update: lo and step must be 16-byte aligned");
    const int per16 = store_per16(storage);
    NLSH_REQUIRE(d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_INVALID, "csr_update: d=%d not in [1, NLSH_MAX_DIM = %d]", d, NLSH_MAX_DIM);
    NLSH_REQUIRE(n_old >= 0 && n_old < (1ll << 31), NLSH_E_INVALID, "csr_update: n_old=%lld not in [0, 2^31)", (long long)n_old);
    NLSH_REQUIRE(n_buckets_old >= 0 && n_buckets_old <= n_old, NLSH_E_INVALID, "csr_update: n_buckets_old=%lld not in [0, n_old=%lld]",
                 (long long)n_buckets_old, (long long)n_old);
    NLSH_REQUIRE(m_new >= 0 && m_new < (1ll << 31), NLSH_E_INVALID, "csr_update: m_new=%lld not in [0, 2^31)", (long long)m_new);
    NLSH_REQUIRE(n_kept >= 0 && n_kept <= n_old, NLSH_E_INVALID, "csr_update: n_kept=%lld not in [0, n_old=%lld]", (long long)n_kept, (long long)n_old);
    NLSH_REQUIRE(keep || n_kept == n_old, NLSH_E_INVALID, "csr_update: keep is null (every row kept) but n_kept=%lld != n_old=%lld",
                 (long long)n_kept, (long long)n_old);
    const long long n_out = (long long)n_kept + (long long)m_new;
    NLSH_REQUIRE(n_out <= 0x7FFFFFFFll, NLSH_E_INVALID, "csr_update: n_kept + m_new = %lld rows > 2^31 - 1 (int32 row positions)", n_out);
    NLSH_REQUIRE(offsets_out && n_buckets_out, NLSH_E_INVALID, "csr_update: offsets_out / n_buckets_out is null");
    if (n_old) {
        NLSH_REQUIRE(row_stride >= d && row_stride % per16 == 0, NLSH_E_INVALID, "csr_update: row_stride=%lld must be >= d=%d and a multiple of %d",
                     (long long)row_stride, d, per16);
        NLSH_REQUIRE(corpus_sorted && gid && uniq_keys && offsets, NLSH_E_INVALID, "csr_update: corpus_sorted / gid / uniq_keys / offsets is null with n_old=%lld",
                     (long long)n_old);
        NLSH_REQUIRE(((uintptr_t)corpus_sorted & 15) == 0, NLSH_E_INVALID, "csr_update: corpus_sorted must be 16-byte aligned");
        NLSH_REQUIRE(n_buckets_old >= 1, NLSH_E_INVALID, "csr_update: n_buckets_old=0 with n_old=%lld rows", (long long)n_old);
    }
    if (m_new) {
        NLSH_REQUIRE(new_stride >= d, NLSH_E_INVALID, "csr_update: new_stride=%lld < d=%d", (long long)new_stride, d);
        NLSH_REQUIRE(rows_new && keys_new && ids_new, NLSH_E_INVALID, "csr_update: rows_new / keys_new / ids_new is null with m_new=%lld", (long long)m_new);
        NLSH_REQUIRE(first_bad || new_storage == storage, NLSH_E_INVALID, "csr_update: first_bad is null but the new rows (new_storage=%d) are converted to storage=%d",
                     new_storage, storage);
    }
    UpdateWs w;
    update_layout(n_old, n_buckets_old, m_new, &w);
    if (n_out) {
        NLSH_REQUIRE(stride_out >= d && stride_out % per16 == 0, NLSH_E_INVALID, "csr_update: stride_out=%lld must be >= d=%d and a multiple of %d",
                     (long long)stride_out, d, per16);
        NLSH_REQUIRE(sorted_out && gid_out && src_out && uniq_out, NLSH_E_INVALID, "csr_update: sorted_out / gid_out / src_out / uniq_out is null");
        NLSH_REQUIRE(((uintptr_t)sorted_out & 15) == 0, NLSH_E_INVALID, "csr_update: sorted_out must be 16-byte aligned");
        NLSH_REQUIRE(!inv_norm_out || inv_norm || n_kept == 0, NLSH_E_INVALID, "csr_update: inv_norm_out is wanted but inv_norm (the kept rows') is null");
        NLSH_REQUIRE(workspace, NLSH_E_INVALID, "csr_update: workspace is null");
        NLSH_REQUIRE(((uintptr_t)workspace & 15) == 0, NLSH_E_INVALID, "csr_update: the workspace must be 16-byte aligned");
        NLSH_REQUIRE(workspace_bytes >= w.total, NLSH_E_INVALID, "csr_update: workspace_bytes=%zu < nlsh_csr_update_workspace = %zu", workspace_bytes, w.total);
    }
    // ---- device work
    hipStream_t s = (hipStream_t)stream;
    if (first_bad) NLSH_CHECK_HIP(hipMemsetAsync(first_bad, 0xFF, sizeof(int32_t), s));   // -1: every new row survived its conversion
    if (clamped_rows) NLSH_CHECK_HIP(hipMemsetAsync(clamped_rows, 0, sizeof(int32_t), s));
    if (n_out == 0) {
        NLSH_CHECK_HIP(hipMemsetAsync(offsets_out, 0, sizeof(int32_t), s));
        NLSH_CHECK_HIP(hipMemsetAsync(n_buckets_out, 0, sizeof(int32_t), s));
        return NLSH_OK;
    }
    char *base = (char *)workspace;
    int32_t *kex = keep ? (int32_t *)(base + w.kex) : nullptr, *shift_old = (int32_t *)(base + w.shift_old);
    int32_t *key_out = (int32_t *)(base + w.key_out), *flags = (int32_t *)(base + w.flags), *rank = (int32_t *)(base + w.rank);
    int32_t *perm_n = (int32_t *)(base + w.perm_n), *uniq_n = (int32_t *)(base + w.uniq_n), *offs_n = (int32_t *)(base + w.offs_n);
    int32_t *nb_n = (int32_t *)(base + w.nb_n), *shift_new = (int32_t *)(base + w.shift_new);
    void *tmp = base + w.tmp;
    int32_t *nul = nullptr;
    const size_t n_scan = (size_t)(n_out > n_old ? n_out : n_old);
    size_t t_sort = 0, t_scan = 0;      // what rocPRIM really asks for on this device, against the bound the workspace was sized by
    if (m_new) NLSH_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t_sort, nul, nul, nul, nul, (size_t)m_new, 0, 32, s));
    NLSH_CHECK_HIP(rocprim::inclusive_scan(nullptr, t_scan, nul, nul, n_scan, rocprim::plus<int32_t>(), s));
    NLSH_REQUIRE(t_sort <= w.tmp_bytes && t_scan <= w.tmp_bytes, NLSH_E_WORKSPACE, "csr_update: rocPRIM scratch (sort %zu, scan %zu bytes) exceeds the %zu bytes "
                 "the workspace formula reserves for it", t_sort, t_scan, w.tmp_bytes);
    auto grid_of = [](long long n) { long long g = (n + 255) / 256; return dim3((unsigned)(g < 1 ? 1 : g > 2048 ? 2048 : g)); };
    if (m_new) {
        int rc = build_csr_on(keys_new, (long long)m_new, perm_n, uniq_n, offs_n, nb_n, (int32_t *)(base + w.sk), (int32_t *)(base + w.iota),
                              (int32_t *)(base + w.flags_n), (int32_t *)(base + w.rank_n), tmp, w.tmp_bytes, s);
        if (rc != NLSH_OK) return rc;
    }
    if (keep) {         // kex[0] = 0, kex[i + 1] = keep[0] + ... + keep[i]
        hipLaunchKernelGGL(keep_flags_kernel, grid_of(n_old), dim3(256), 0, s, keep, (long long)n_old, flags);
        NLSH_CHECK_HIP(hipMemsetAsync(kex, 0, sizeof(int32_t), s));
        size_t tb = w.tmp_bytes;
        NLSH_CHECK_HIP(rocprim::inclusive_scan(tmp, tb, flags, kex + 1, (size_t)n_old, rocprim::plus<int32_t>(), s));
    }
    hipLaunchKernelGGL(update_shifts_kernel, grid_of(n_buckets_old + m_new), dim3(256), 0, s, uniq_keys, offsets, (int)n_buckets_old, (int)n_old, kex,
                       uniq_n, offs_n, nb_n, (int)m_new, shift_old, shift_new);
    hipLaunchKernelGGL(update_index_kernel, grid_of(n_old + m_new), dim3(256), 0, s, gid, uniq_keys, offsets, (int)n_buckets_old, (int)n_old, keep, kex,
                       shift_old, perm_n, uniq_n, offs_n, nb_n, ids_new, shift_new, (int)m_new, n_out, src_out, gid_out, key_out);
    // the bucket table of the result: the run-length encoding of the keys at their destinations (emptied buckets vanish, new ones appear)
    hipLaunchKernelGGL(head_flags_kernel, grid_of(n_out), dim3(256), 0, s, key_out, n_out, flags);
    size_t tb = w.tmp_bytes;
    NLSH_CHECK_HIP(rocprim::inclusive_scan(tmp, tb, flags, rank, (size_t)n_out, rocprim::plus<int32_t>(), s));
    hipLaunchKernelGGL(emit_buckets_kernel, grid_of(n_out), dim3(256), 0, s, key_out, flags, rank, n_out, uniq_out, offsets_out, n_buckets_out);
    // the rows
    const int d4 = (int)(stride_out >> 2);
    int lg = 0;
    while ((1 << lg) < d4 && lg < 6) ++lg;
    const long long rows_per_wave = (long long)(64 >> lg) * ROWS_IN_FLIGHT;
    long long blocks = ((n_out + rows_per_wave - 1) / rows_per_wave + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (storage == NLSH_STORE_F32 && new_storage == NLSH_STORE_F32) {
        const float *old_f = (const float *)corpus_sorted, *new_f = (const float *)rows_new;
        float *out_f = (float *)sorted_out;
        const bool vec = ((new_stride & 3) == 0) && (((uintptr_t)rows_new & 15) == 0);
        if (vec)
            hipLaunchKernelGGL(update_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, old_f, (long long)row_stride, inv_norm, (long long)n_old,
                               new_f, (long long)new_stride, (long long)m_new, d, src_out, n_out, out_f, (long long)stride_out, inv_norm_out, lg);
        else
            hipLaunchKernelGGL(update_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, old_f, (long long)row_stride, inv_norm, (long long)n_old,
                               new_f, (long long)new_stride, (long long)m_new, d, src_out, n_out, out_f, (long long)stride_out, inv_norm_out, lg);
    } else {
        // typed storage: the row pass in 16-byte units, then the inv_norm pass over what it wrote
        const long long units_old = row_stride / per16, units_out = stride_out / per16;
        int lgu = 0;
        while ((1 << lgu) < units_out && lgu < 6) ++lgu;
        const long long rows_per_wave_u = (long long)(64 >> lgu) * ROWS_IN_FLIGHT;
        long long ublocks = ((n_out + rows_per_wave_u - 1) / rows_per_wave_u + 3) / 4;
        if (ublocks > 256 * 8) ublocks = 256 * 8;
        const void *fn = nullptr;
#define NLSH_UPD(N, D) if (new_storage == N && storage == D) fn = (const void *)update_rows_typed_kernel<N, D>;
        NLSH_UPD(NLSH_STORE_F16, NLSH_STORE_F32) NLSH_UPD(NLSH_STORE_U8, NLSH_STORE_F32)
        NLSH_UPD(NLSH_STORE_F32, NLSH_STORE_F16) NLSH_UPD(NLSH_STORE_F16, NLSH_STORE_F16) NLSH_UPD(NLSH_STORE_U8, NLSH_STORE_F16)
        NLSH_UPD(NLSH_STORE_F32, NLSH_STORE_U8) NLSH_UPD(NLSH_STORE_F16, NLSH_STORE_U8) NLSH_UPD(NLSH_STORE_U8, NLSH_STORE_U8)
#undef NLSH_UPD
        long long uo = units_old, nold = n_old, sn = new_stride, mn = m_new, no = n_out, ut = units_out, sto = stride_out;
        int vecn = store_vec_ok(rows_new, new_storage, new_stride);      // new rows on chunk boundaries of their storage: one load per chunk
        void *argv[] = {&corpus_sorted, &uo, &nold, &rows_new, &sn, &mn, &d, &src_out, &no, &sorted_out, &ut, &lgu, &first_bad, &vecn};
        if (sq8) {      // the same two passes with the quantiser: new rows encoded (uint8 ones are codes), norms over decoded values
            const void *fs = new_storage == NLSH_STORE_F32 ? (const void *)update_rows_sq8_kernel<NLSH_STORE_F32>
                           : new_storage == NLSH_STORE_F16 ? (const void *)update_rows_sq8_kernel<NLSH_STORE_F16>
                                                           : (const void *)update_rows_sq8_kernel<NLSH_STORE_U8>;
            void *args[] = {&corpus_sorted, &uo, &nold, &rows_new, &sn, &mn, &d, &src_out, &no, &sorted_out, &ut, &lgu, &lo, &step, &first_bad,
                            &clamped_rows, &vecn};
            NLSH_CHECK_HIP(hipLaunchKernel(fs, dim3((unsigned)ublocks), dim3(256), args, 0, s));
            if (inv_norm_out) {
                long long iblocks = ((n_out + 63) / 64 + 3) / 4;
                if (iblocks > 256 * 8) iblocks = 256 * 8;
                void *argi[] = {&sorted_out, &sto, &lo, &step, &inv_norm, &nold, &src_out, &no, &inv_norm_out};
                NLSH_CHECK_HIP(hipLaunchKernel((const void *)update_inv_norm_sq8_kernel, dim3((unsigned)iblocks), dim3(256), argi, 0, s));
            }
            NLSH_CHECK_HIP(hipGetLastError());
            return NLSH_OK;
        }
        NLSH_CHECK_HIP(hipLaunchKernel(fn, dim3((unsigned)ublocks), dim3(256), argv, 0, s));
        if (inv_norm_out) {
            const void *fi = storage == NLSH_STORE_F32 ? (const void *)update_inv_norm_typed_kernel<NLSH_STORE_F32>
                           : storage == NLSH_STORE_F16 ? (const void *)update_inv_norm_typed_kernel<NLSH_STORE_F16>
                                                       : (const void *)update_inv_norm_typed_kernel<NLSH_STORE_U8>;
            long long iblocks = ((n_out + 63) / 64 + 3) / 4;
            if (iblocks > 256 * 8) iblocks = 256 * 8;
            void *argi[] = {&sorted_out, &sto, &inv_norm, &nold, &src_out, &no, &inv_norm_out};
            NLSH_CHECK_HIP(hipLaunchKernel(fi, dim3((unsigned)iblocks), dim3(256), argi, 0, s));
        }
    }
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

extern "C" int nlsh_csr_update(const float *corpus_sorted, int64_t row_stride, int d, const int32_t *gid, const float *inv_norm,
                               const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                               const uint8_t *keep, int64_t n_kept,
                               const float *rows_new, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new, int64_t m_new,
                               float *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                               int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out,
                               void *workspace, size_t workspace_bytes, nlsh_stream_t stream) {
    return csr_update_impl(corpus_sorted, NLSH_STORE_F32, row_stride, d, gid, inv_norm, uniq_keys, offsets, n_old, n_buckets_old, keep, n_kept,
                           rows_new, NLSH_STORE_F32, new_stride, keys_new, ids_new, m_new, sorted_out, stride_out, gid_out, inv_norm_out, src_out,
                           uniq_out, offsets_out, n_buckets_out, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int nlsh_csr_update_typed(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid, const float *inv_norm,
                                     const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                                     const uint8_t *keep, int64_t n_kept,
                                     const void *rows_new, int new_storage, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new,
                                     int64_t m_new,
                                     void *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                                     int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out, int32_t *first_bad,
                                     void *workspace, size_t workspace_bytes, nlsh_stream_t stream) {
    return csr_update_impl(corpus_sorted, storage, row_stride, d, gid, inv_norm, uniq_keys, offsets, n_old, n_buckets_old, keep, n_kept,
                           rows_new, new_storage, new_stride, keys_new, ids_new, m_new, sorted_out, stride_out, gid_out, inv_norm_out, src_out,
                           uniq_out, offsets_out, n_buckets_out, first_bad, workspace, workspace_bytes, stream);
}

extern "C" int nlsh_gather_rows_typed(const void *corpus, int src_storage, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                                      void *sorted, int dst_storage, int64_t dst_stride, float *inv_norm, int32_t *gid, int32_t id_base,
                                      int32_t *first_bad, nlsh_stream_t stream) {
    NLSH_REQUIRE(store_ok(src_storage) && store_ok(dst_storage), NLSH_E_INVALID,
                 "gather_rows_typed: src_storage=%d / dst_storage=%d is none of NLSH_STORE_F32 / F16 / U8", src_storage, dst_storage);
    NLSH_REQUIRE(n >= 0 && d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_INVALID, "gather_rows_typed: n=%lld d=%d", (long long)n, d);
    NLSH_REQUIRE(first_bad || src_storage == dst_storage, NLSH_E_INVALID,
                 "gather_rows_typed: first_bad is null but the rows are converted (src_storage=%d, dst_storage=%d)", src_storage, dst_storage);
    if (n) {
        NLSH_REQUIRE(corpus && perm && sorted, NLSH_E_INVALID, "gather_rows_typed: corpus / perm / sorted is null");
        NLSH_REQUIRE(dst_stride >= d && dst_stride % store_per16(dst_storage) == 0, NLSH_E_INVALID,
                     "gather_rows_typed: dst_stride=%lld must be >= d=%d and a multiple of %d elements (a pitch of 16-byte units) for dst_storage=%d",
                     (long long)dst_stride, d, store_per16(dst_storage), dst_storage);
        NLSH_REQUIRE(((uintptr_t)sorted & 15) == 0, NLSH_E_INVALID, "gather_rows_typed: sorted must be 16-byte aligned");
        NLSH_REQUIRE(src_stride >= d, NLSH_E_INVALID, "gather_rows_typed: src_stride=%lld < d=%d", (long long)src_stride, d);
        // an element pointer is read with element loads: it must be aligned to its element
        NLSH_REQUIRE(((uintptr_t)corpus & (src_storage == NLSH_STORE_F32 ? 3 : src_storage == NLSH_STORE_F16 ? 1 : 0)) == 0, NLSH_E_INVALID,
                     "gather_rows_typed: corpus is not aligned to its element size");
    }
    hipStream_t s = (hipStream_t)stream;
    if (first_bad) NLSH_CHECK_HIP(hipMemsetAsync(first_bad, 0xFF, sizeof(int32_t), s));   // -1: every row survived its conversion
    if (n == 0) return NLSH_OK;
    if (src_storage == NLSH_STORE_F32 && dst_storage == NLSH_STORE_F32)
        return nlsh_gather_rows((const float *)corpus, src_stride, d, perm, n, (float *)sorted, dst_stride, inv_norm, gid, id_base, stream);
    long long blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const void *fn = nullptr;
#define NLSH_GAT(S, D) if (src_storage == S && dst_storage == D) fn = (const void *)gather_rows_typed_kernel<S, D>;
    NLSH_GAT(NLSH_STORE_F16, NLSH_STORE_F32) NLSH_GAT(NLSH_STORE_U8, NLSH_STORE_F32)
    NLSH_GAT(NLSH_STORE_F32, NLSH_STORE_F16) NLSH_GAT(NLSH_STORE_F16, NLSH_STORE_F16) NLSH_GAT(NLSH_STORE_U8, NLSH_STORE_F16)
    NLSH_GAT(NLSH_STORE_F32, NLSH_STORE_U8) NLSH_GAT(NLSH_STORE_F16, NLSH_STORE_U8) NLSH_GAT(NLSH_STORE_U8, NLSH_STORE_U8)
#undef NLSH_GAT
    long long ss = src_stride, nn = n, ds = dst_stride;
    int vec = store_vec_ok(corpus, src_storage, src_stride);             // rows on chunk boundaries of their storage: one load per chunk
    void *argv[] = {&corpus, &ss, &d, &perm, &nn, &sorted, &ds, &inv_norm, &gid, &id_base, &first_bad, &vec};
    NLSH_CHECK_HIP(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), argv, 0, s));
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
}

// ---- storage="sq8" (sq8_rows.h): entry points of their own beside the typed ones, which refuse every storage code past NLSH_STORE_U8
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

extern "C" int nlsh_gather_rows_sq8(const void *corpus, int src_storage, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                                    uint8_t *sorted, int64_t dst_stride, const float *lo, const float *step, float *inv_norm, int32_t *gid,
                                    int32_t id_base, int32_t *first_bad, int32_t *clamped_rows, nlsh_stream_t stream) {
    NLSH_REQUIRE(store_ok(src_storage), NLSH_E_INVALID, "gather_rows_sq8: src_storage=%d is none of NLSH_STORE_F32 / F16 / U8", src_storage);
    NLSH_REQUIRE(n >= 0 && d >= 1 && d <= NLSH_MAX_DIM, NLSH_E_INVALID, "gather_rows_sq8: n=%lld d=%d", (long long)n, d);
    NLSH_REQUIRE(first_bad || src_storage == NLSH_STORE_U8, NLSH_E_INVALID, "gather_rows_sq8: first_bad is null but the rows are encoded (src_storage=%d)", src_storage);
    if (n) {
        NLSH_REQUIRE(corpus && perm && sorted, NLSH_E_INVALID, "gather_rows_sq8: corpus / perm / sorted is null");
        NLSH_REQUIRE(lo && step, NLSH_E_INVALID, "gather_rows_sq8: lo / step is null");
        NLSH_REQUIRE(dst_stride >= d && dst_stride % 16 == 0, NLSH_E_INVALID,
                     "gather_rows_sq8: dst_stride=%lld must be >= d=%d and a multiple of 16 elements (a pitch of 16-byte units)", (long long)dst_stride, d);
        NLSH_REQUIRE(((uintptr_t)sorted & 15) == 0, NLSH_E_INVALID, "gather_rows_sq8: sorted must be 16-byte aligned");
        NLSH_REQUIRE((((uintptr_t)lo | (uintptr_t)step) & 15) == 0, NLSH_E_INVALID, "gather_rows_sq8: lo and step must be 16-byte aligned");
        NLSH_REQUIRE(src_stride >= d, NLSH_E_INVALID, "gather_rows_sq8: src_stride=%lld < d=%d", (long long)src_stride, d);
        NLSH_REQUIRE(((uintptr_t)corpus & (src_storage == NLSH_STORE_F32 ? 3 : src_storage == NLSH_STORE_F16 ? 1 : 0)) == 0, NLSH_E_INVALID,
                     "gather_rows_sq8: corpus is not aligned to its element size");
    }
    hipStream_t s = (hipStream_t)stream;
    if (first_bad) NLSH_CHECK_HIP(hipMemsetAsync(first_bad, 0xFF, sizeof(int32_t), s));   // -1: every row is finite
    if (clamped_rows) NLSH_CHECK_HIP(hipMemsetAsync(clamped_rows, 0, sizeof(int32_t), s));
    if (n == 0) return NLSH_OK;
    long long blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const void *fn = src_storage == NLSH_STORE_F32 ? (const void *)gather_rows_sq8_kernel<NLSH_STORE_F32>
                   : src_storage == NLSH_STORE_F16 ? (const void *)gather_rows_sq8_kernel<NLSH_STORE_F16>
                                                   : (const void *)gather_rows_sq8_kernel<NLSH_STORE_U8>;
    long long ss = src_stride, nn = n, ds = dst_stride;
    int vec = store_vec_ok(corpus, src_storage, src_stride);
    void *argv[] = {&corpus, &ss, &d, &perm, &nn, &sorted, &ds, &lo, &step, &inv_norm, &gid, &id_base, &first_bad, &clamped_rows, &vec};
    NLSH_CHECK_HIP(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), argv, 0, s));
    NLSH_CHECK_HIP(hipGetLastError());
    return NLSH_OK;
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
    return csr_update_impl(corpus_sorted, NLSH_STORE_U8, row_stride, d, gid, inv_norm, uniq_keys, offsets, n_old, n_buckets_old, keep, n_kept,
                           rows_new, new_storage, new_stride, keys_new, ids_new, m_new, sorted_out, stride_out, gid_out, inv_norm_out, src_out,
                           uniq_out, offsets_out, n_buckets_out, first_bad, workspace, workspace_bytes, stream, true, lo, step, clamped_rows);
}
