// Bucket-major scan, LDS-tiled schedule (included by two translation units behind scan_bucket_args.h, which defines BArgs: scan_bucket.hip
// instantiates the float32 kernels, scan_bucket_typed.hip the float16 / uint8 ones):
// the hand-scheduled k-blocks, the task bodies built from them (l2_task*), one task start to finish (tiled_task_body) and the kernels
// bscan3_kernel (k <= 64) and bscanw_kernel (k up to NLSH_MAX_K_TILED) over a float32 corpus, bscant_kernel over a float16 / uint8 one,
// bscanf_kernel behind a row filter (scan_bucket_filtered.hip instantiates it), bscanr_kernel for radius queries (scan_bucket_range.hip),
// bscana_kernel over an sq8 corpus (scan_bucket_affine.hip), bscang_kernel behind per-query tag filters (scan_bucket_tagged.hip),
// bscanq_kernel over a product-quantised corpus (scan_bucket_pq.hip).
#pragma once

// Diagnostic build only (make EXTRA=-DNLSH_SCAN_TRACE, tools/scan_trace.py): wave 0 of every bscan3 workgroup
// leaves its phase durations (100 MHz wall_clock64 ticks) in g_scan_trace; the shipped library has neither.
#ifdef NLSH_SCAN_TRACE
#define NLSH_TRACE_SLOTS (1 << 16)
__device__ float g_scan_trace[NLSH_TRACE_SLOTS * 8];
extern "C" int nlsh_debug_scan_trace(float *host, int n_floats) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_scan_trace), (size_t)n_floats * 4);
}
#define SCAN_NOW() wall_clock64()
#else
#define SCAN_NOW() 0ull
#endif

// 16-byte chunks per k-block of the tiled schedule.  4 (64 bytes of every row per stage): 20 KB of LDS and 64 VGPRs
// per workgroup -> 6-7 workgroups per CU; 8 measured 0.404 ms against 0.350 ms at 4 waves/SIMD, 2 the same as 4.
#ifndef NLSH_TILED_KB
#define NLSH_TILED_KB 4
#endif

// (NLSH_ABLATE / NLSH_NO_STAGE_BARRIER: diagnostic switches, defined in scan_common.h, live only under -DNLSH_DIAG)
#define NLSH_STAGE_SYNC() do { if (!NLSH_NO_STAGE_BARRIER) __syncthreads(); } while (0)

// Settled A/B experiments of the tiled schedule whose switches were removed; what shipped is the plain code below, the measurements
// are in DESIGN.md appendix A and git history keeps the losing forms:
//   - a task's queries are dealt round-robin over the 4 waves (NLSH_SLOT), not in blocks of 4 (r02: equal or slower);
//   - no s_setprio inside / outside the distance loop (r02: equal or slower);
//   - min waves per SIMD hint of the tiled kernels stays 1 (8 = 64 VGPRs / 80 SGPRs: measured equal, 43 SGPR spills);
//   - eps of the hand-scheduled L2 block is the 32-bit literal (8-byte v_add), not a VGPR (4-byte; r02: equal or slower);
//   - the cosine block reads the query chunk straight from SGPRs (68 VGPRs, 7 waves per SIMD, every v_fmac at the SGPR-operand rate: 0.195 ms
//     on the skewed cosine run), not from VGPR copies made once per chunk (84 VGPRs, 5 waves: 0.207 ms);
//   - every task, cosine included, runs the hand-scheduled k-blocks; the compiler-scheduled loop they replaced is gone (r02);
//   - short segments take fat stages, tasks that fit one stage the single-stage body, the query lines are warmed a stage ahead and the
//     L2 epilogue is the lean one (r05: square roots without the range scaling, one wave-uniform guard per list, sign-free key build).

// slot of query jq of a wave in its task's 16 slot records: the queries of a task are dealt round-robin over its NW waves
#define NLSH_SLOT(wave, jq) ((wave) + NW * (jq))

namespace nlsh {

// ------------------------------------------------------------------------------------ tiled variant
// NLSH_SCAN_BUCKET_TILED: one WORKGROUP per task = (256-row bucket segment, group of <= 16 queries).
// The segment goes through LDS one k-block (KB 16-byte chunks of every row) at a time (coalesced 16-byte
// global loads -> ds_write_b128, odd row stride = conflict-free column reads) and every lane OWNS ONE ROW of
// each 64-row tile: it walks the row in k order and updates QW query accumulators per tile, the query values
// arriving as wave-uniform scalar loads (s_load from the queries, or from a padded / pre-normalised copy when
// the prepared query copy is needed).  No cross-lane reduction at all: 3 VALU per element and query for L2 ((q-c), +eps, fma),
// 1 for cosine; the distance of lane l's row is a k-ascending fmaf chain, bit-identical to the oracle's scalar
// loop.  Four waves share the tile, so a row is fetched from HBM/L2 once per 16 queries.  The next k-block's
// global loads are issued before the current one is computed (load early, ds_write late).
//
// What bounds it (r01 traces, tools/scan_trace.py, tools/probe_l2_loop.hip): the inner loop's instruction mix
// sustains 1 VALU / 2.5-2.9 cycles per SIMD in isolation; the kernel reaches ~60 % of that because a wave spends
// ~35 % of a task outside the distance loop (stage barriers, top-k selection) and only resident waves of OTHER
// workgroups fill those gaps -- occupancy is the lever that paid (KB 8 -> 4: 4 -> 6-7 workgroups per CU, 0.40 ->
// 0.34 ms).  Measured and dropped: branch-free loop bodies specialised on (queries, tiles) per wave, with and
// without hand-placed LDS/SMEM double buffering (the scheduler keeps the scalar query chunks in VGPRs: 110-150
// VGPRs, 3-4 waves/SIMD, 0.43-0.49 ms); reading the next step's row chunk one step ahead (+3 %); reading all
// tiles' chunks of a step up front (+-0); a second copy of the loop without the per-query guards for waves that
// hold all QW queries (79 VGPRs -> 6 waves/SIMD: 0.363 vs 0.344 ms); requesting a k-block's first query chunk before
// the stage barriers (0.346 vs 0.337 ms: the barrier's lgkmcnt(0) then also waits for the scalar loads); touching the
// next 64-byte query line with a dummy scalar load one line ahead (SGPR spills 28 -> 50: 0.355 vs 0.331 ms); one
// s_load_dwordx16 per query line instead of four x4 (64 VGPRs kept, +-0: the scalar loads are not what waves wait for).
typedef const __attribute__((address_space(4))) float *const_f32p;

// ---- hand-scheduled k-block of a FULL L2 task (4 queries per wave x 4 row tiles x 4 chunks) ------------------------------
// r02 finding (ISA + SQ counters of the compiler-scheduled loop): every (tile, query) block sat behind two or three
// uniform branches and an `s_waitcnt lgkmcnt(0)` placed directly after its `ds_read_b128` -- the LDS round trip was exposed
// 16 times per chunk step and the scalar loads of the next chunk (same counter) were waited for as soon as they were
// issued; waves spent as many cycles stalled at issue as executing.  Full tasks are 29 % of the tasks and most of the
// arithmetic, so their k-blocks run this straight-line form instead: VALU in inline asm (the compiler cannot re-order or
// re-guard it), the row chunk of tile t+1 and the query chunk c+1 requested one block (48 VALU) ahead, no branches.
// The arithmetic is the oracle's, in its order: F.pairwise_distance is || (x1 - x2) + eps || summed in k order (nlsh/data.py:201), so
// an accumulator takes (q - c) + eps, squared, as an fmaf chain in ascending k -> bit-identical results.
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct QSet { f32x4 v[4]; };   // one 16-byte chunk of each of the wave's (up to) 4 queries: 16 SGPRs

// NQ s_load_dwordx4 (query pointer + byte offset in an SGPR) that the compiler can neither merge into wider loads (x8
// pairs need 64 SGPRs for a double buffer and spilled) nor move; the caller waits for them with s_waitcnt lgkmcnt(0)
// before the first VALU block that reads them.
// `after`: a VGPR the loads pretend to read -- the row chunk the NEXT VALU block consumes.  LDS and scalar loads share
// one counter and scalar loads return out of order, so any wait for LDS data also waits for scalar loads in flight: the
// compiler's wait for that row chunk is thereby placed BEFORE these loads are issued, and they get a whole VALU block
// of cover before the next wait.
template <int NQ>
__device__ __forceinline__ void load_qset(QSet &q, const const_f32p (&qk)[4], int byte_off, float after) {
    if (NQ == 4)
        asm volatile("s_load_dwordx4 %0, %4, %8\n\ts_load_dwordx4 %1, %5, %8\n\ts_load_dwordx4 %2, %6, %8\n\ts_load_dwordx4 %3, %7, %8"
                     : "=&s"(q.v[0]), "=&s"(q.v[1]), "=&s"(q.v[2]), "=&s"(q.v[3])
                     : "s"(qk[0]), "s"(qk[1]), "s"(qk[2]), "s"(qk[3]), "s"(byte_off), "v"(after));
    else if (NQ == 3)
        asm volatile("s_load_dwordx4 %0, %3, %6\n\ts_load_dwordx4 %1, %4, %6\n\ts_load_dwordx4 %2, %5, %6"
                     : "=&s"(q.v[0]), "=&s"(q.v[1]), "=&s"(q.v[2])
                     : "s"(qk[0]), "s"(qk[1]), "s"(qk[2]), "s"(byte_off), "v"(after));
    else if (NQ == 2)
        asm volatile("s_load_dwordx4 %0, %2, %4\n\ts_load_dwordx4 %1, %3, %4"
                     : "=&s"(q.v[0]), "=&s"(q.v[1])
                     : "s"(qk[0]), "s"(qk[1]), "s"(byte_off), "v"(after));
    else
        asm volatile("s_load_dwordx4 %0, %1, %2" : "=&s"(q.v[0]) : "s"(qk[0]), "s"(byte_off), "v"(after));
}

// One (tile, chunk) block = NQ query blocks in ONE asm statement: the compiler pads every inline-asm statement with an
// s_nop (it cannot see the hazards inside), and per-query statements left 25 of them per chunk pair in the hot loop.
// eps is the 32-bit LITERAL, not an SGPR: tools/probe_l2_block.hip measured 2.2 cycles per VALU for this block with the
// literal against 2.9-3.4 with eps in an SGPR (a VALU instruction that reads an SGPR issues slower on gfx950: sub/add
// with SGPR operands only, 4.1 cycles) -- only the v_sub reads one (the query value).
#define NLSH_QBLK(J)                                                                                               \
    "v_sub_f32 %[t0], %[q" #J "0], %[r0]\n\tv_sub_f32 %[t1], %[q" #J "1], %[r1]\n\t"                                 \
    "v_sub_f32 %[t2], %[q" #J "2], %[r2]\n\tv_sub_f32 %[t3], %[q" #J "3], %[r3]\n\t"                                 \
    "v_add_f32 %[t0], 0x358637bd, %[t0]\n\tv_add_f32 %[t1], 0x358637bd, %[t1]\n\t"                                   \
    "v_add_f32 %[t2], 0x358637bd, %[t2]\n\tv_add_f32 %[t3], 0x358637bd, %[t3]\n\t"                                   \
    "v_fmac_f32 %[a" #J "], %[t0], %[t0]\n\tv_fmac_f32 %[a" #J "], %[t1], %[t1]\n\t"                                 \
    "v_fmac_f32 %[a" #J "], %[t2], %[t2]\n\tv_fmac_f32 %[a" #J "], %[t3], %[t3]\n\t"
// The 2-op form (NLSH_METRIC_L2_EPS_FOLDED): eps is folded into the query copy prep_query writes, a block is v_sub + v_fmac -- 8
// instead of 12 VALU per chunk and query.  (q + eps) - c rounds differently from (q - c) + eps, so it is NOT the oracle's bits:
// an opt-in within the north_star's 1e-4 tolerance, never the default.
#define NLSH_QBLK2(J)                                                                                              \
    "v_sub_f32 %[t0], %[q" #J "0], %[r0]\n\tv_sub_f32 %[t1], %[q" #J "1], %[r1]\n\t"                                 \
    "v_sub_f32 %[t2], %[q" #J "2], %[r2]\n\tv_sub_f32 %[t3], %[q" #J "3], %[r3]\n\t"                                 \
    "v_fmac_f32 %[a" #J "], %[t0], %[t0]\n\tv_fmac_f32 %[a" #J "], %[t1], %[t1]\n\t"                                 \
    "v_fmac_f32 %[a" #J "], %[t2], %[t2]\n\tv_fmac_f32 %[a" #J "], %[t3], %[t3]\n\t"
#define NLSH_QIN(J) [q##J##0] "s"(q.v[J].x), [q##J##1] "s"(q.v[J].y), [q##J##2] "s"(q.v[J].z), [q##J##3] "s"(q.v[J].w)
#define NLSH_TMP [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3)
#define NLSH_RIN [r0] "v"(r.x), [r1] "v"(r.y), [r2] "v"(r.z), [r3] "v"(r.w)
template <int NQ>
__device__ __forceinline__ void l2f_tile_block(float (&acc)[4], const float4 r, const QSet &q) {
    float t0, t1, t2, t3;
    if (NQ == 4)
        asm volatile(NLSH_QBLK2(0) NLSH_QBLK2(1) NLSH_QBLK2(2) NLSH_QBLK2(3)
                     : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), NLSH_TMP
                     : NLSH_RIN, NLSH_QIN(0), NLSH_QIN(1), NLSH_QIN(2), NLSH_QIN(3));
    else if (NQ == 3)
        asm volatile(NLSH_QBLK2(0) NLSH_QBLK2(1) NLSH_QBLK2(2)
                     : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), NLSH_TMP
                     : NLSH_RIN, NLSH_QIN(0), NLSH_QIN(1), NLSH_QIN(2));
    else if (NQ == 2)
        asm volatile(NLSH_QBLK2(0) NLSH_QBLK2(1) : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), NLSH_TMP : NLSH_RIN, NLSH_QIN(0), NLSH_QIN(1));
    else
        asm volatile(NLSH_QBLK2(0) : [a0] "+v"(acc[0]), NLSH_TMP : NLSH_RIN, NLSH_QIN(0));
}
template <int NQ>
__device__ __forceinline__ void l2_tile_block(float (&acc)[4], const float4 r, const QSet &q) {
    float t0, t1, t2, t3;
    if (NQ == 4)
        asm volatile(NLSH_QBLK(0) NLSH_QBLK(1) NLSH_QBLK(2) NLSH_QBLK(3)
                     : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), NLSH_TMP
                     : NLSH_RIN, NLSH_QIN(0), NLSH_QIN(1), NLSH_QIN(2), NLSH_QIN(3));
    else if (NQ == 3)
        asm volatile(NLSH_QBLK(0) NLSH_QBLK(1) NLSH_QBLK(2)
                     : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), NLSH_TMP
                     : NLSH_RIN, NLSH_QIN(0), NLSH_QIN(1), NLSH_QIN(2));
    else if (NQ == 2)
        asm volatile(NLSH_QBLK(0) NLSH_QBLK(1) : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), NLSH_TMP : NLSH_RIN, NLSH_QIN(0), NLSH_QIN(1));
    else
        asm volatile(NLSH_QBLK(0) : [a0] "+v"(acc[0]), NLSH_TMP : NLSH_RIN, NLSH_QIN(0));
}
#undef NLSH_QBLK
#undef NLSH_QBLK2
#undef NLSH_QIN
#undef NLSH_TMP

// Cosine form of the block: acc += q_k * c_k, an fmaf chain in ascending k, one VALU per element, the query chunk read straight from
// its SGPRs.  (A v_fmac that reads its multiplier from an SGPR issues at about half the rate of one that reads a VGPR
// (tools/probe_l2_block.hip), and here EVERY instruction reads one; VGPR copies made once per chunk cost 16 registers and two waves per
// SIMD and measured slower: see the list at the top of the file.)
#define NLSH_CBLK(J)                                                                                              \
    "v_fmac_f32 %[a" #J "], %[q" #J "0], %[r0]\n\tv_fmac_f32 %[a" #J "], %[q" #J "1], %[r1]\n\t"                     \
    "v_fmac_f32 %[a" #J "], %[q" #J "2], %[r2]\n\tv_fmac_f32 %[a" #J "], %[q" #J "3], %[r3]\n\t"
#define NLSH_CIN(J) [q##J##0] "s"(q.v[J].x), [q##J##1] "s"(q.v[J].y), [q##J##2] "s"(q.v[J].z), [q##J##3] "s"(q.v[J].w)
template <int NQ>
__device__ __forceinline__ void cos_tile_block(float (&acc)[4], const float4 r, const QSet &q) {
    if (NQ == 4)
        asm volatile(NLSH_CBLK(0) NLSH_CBLK(1) NLSH_CBLK(2) NLSH_CBLK(3)
                     : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3])
                     : NLSH_RIN, NLSH_CIN(0), NLSH_CIN(1), NLSH_CIN(2), NLSH_CIN(3));
    else if (NQ == 3)
        asm volatile(NLSH_CBLK(0) NLSH_CBLK(1) NLSH_CBLK(2)
                     : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2])
                     : NLSH_RIN, NLSH_CIN(0), NLSH_CIN(1), NLSH_CIN(2));
    else if (NQ == 2)
        asm volatile(NLSH_CBLK(0) NLSH_CBLK(1) : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]) : NLSH_RIN, NLSH_CIN(0), NLSH_CIN(1));
    else
        asm volatile(NLSH_CBLK(0) : [a0] "+v"(acc[0]) : NLSH_RIN, NLSH_CIN(0));
}
#undef NLSH_CBLK
#undef NLSH_CIN
#undef NLSH_RIN

// One k-block (nchunk 16-byte chunks of every row, LDS row stride RSt slots) for a wave that holds NQ queries, on NT
// 64-row tiles.  Blocks = (chunk, tile) pairs in chunk-major order; two chunks are unrolled so that the row-chunk
// registers (rr[0], rr[1]) and the query sets (qa, qb) alternate statically: block j reads rr[j & 1] while the row
// chunk of block j + 1 is on its way into rr[(j + 1) & 1], and the query chunk c + 1 is requested during the first block
// of chunk c.  The main loop has NO branch but its back edge: prefetches past the end of the k-block are clamped to its
// last chunk (valid addresses, values unused) instead of being guarded -- guarded, the loop carried 8 branches, 22
// scalar-ALU instructions and 25 s_nops per 384 VALU, and on this machine instruction issue is what the kernel is
// bound by (r02: kernel time tracks VALU x 2.3 + scalar x 2..4 cycles per SIMD across every variant measured).
template <int NQ, int NT, int METRIC = NLSH_METRIC_L2_EPS>
__device__ __forceinline__ void l2_kblock(const float4 *col, int RSt, int nchunk, const const_f32p (&qk)[4], float (&acc)[4][4]) {
    constexpr bool COS = METRIC == NLSH_METRIC_COSINE;
    QSet qa, qb;
    float4 rr[2];
    const int TS = 64 * RSt;   // tile stride in float4 slots
    const int last = nchunk - 1;
    rr[0] = col[0];
    load_qset<NQ>(qa, qk, 0, 0.0f);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    int c = 0;
    for (; c + 1 < nchunk; c += 2) {
        const int c2 = min(c + 2, last);   // first chunk of the next pair (clamped on the last pair)
#pragma unroll
        for (int j = 0; j < 2 * NT; ++j) {
            const int tl = j % NT, cc = j / NT;             // compile-time after unrolling
            const int jn = j + 1, tn = jn % NT, cn = jn / NT;
            rr[jn & 1] = col[tn * TS + (cn == 2 ? c2 : c + cn)];
            if (tl == 0) {
                if (cc == 0) load_qset<NQ>(qb, qk, 16 * (c + 1), rr[j & 1].x);
                else load_qset<NQ>(qa, qk, 16 * c2, rr[j & 1].x);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (COS) {
                cos_tile_block<NQ>(acc[tl], rr[j & 1], cc ? qb : qa);
            } else if (METRIC == NLSH_METRIC_L2_EPS_FOLDED) {
                l2f_tile_block<NQ>(acc[tl], rr[j & 1], cc ? qb : qa);
            } else {
                l2_tile_block<NQ>(acc[tl], rr[j & 1], cc ? qb : qa);
            }
            if (tl == NT - 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the next chunk's queries (and first row chunk)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (c < nchunk) {   // odd chunk count (d / 4 not a multiple of the stage width): one more chunk, queries in qa, tile 0 in rr[0]
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (j + 1 < NT) rr[(j + 1) & 1] = col[(j + 1) * TS + c];
            __builtin_amdgcn_sched_barrier(0);
            if (COS) {
                cos_tile_block<NQ>(acc[j], rr[j & 1], qa);
            } else if (METRIC == NLSH_METRIC_L2_EPS_FOLDED) {
                l2f_tile_block<NQ>(acc[j], rr[j & 1], qa);
            } else {
                l2_tile_block<NQ>(acc[j], rr[j & 1], qa);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// Scalar-cache warm-up of the query lines a k-block will read.  Every 64-byte line of a query is read by exactly one wave exactly once
// per task, so its first `s_load` always misses the scalar cache (SQC_DCACHE: 5.2 M requests, 1.08 M misses per launch = one per line) and
// the k-block's first wait -- directly behind the load -- sat through an L2 round trip eight times per task.  A throw-away one-dword load
// of each line, issued a stage earlier (the result register is never read), moves that round trip under the barriers and the LDS
// write of the stage in between.  gfx950 has no scalar prefetch instruction.
// `sink` is the destination of every throw-away load and MUST stay allocated until a `s_waitcnt lgkmcnt(0)` behind them (the loads
// complete asynchronously: a destination the compiler has already handed to another value is overwritten when they land -- the first
// version of this did exactly that and faulted).  It is threaded through the statements as a read-write operand and released by
// `warm_query_lines_done` after the wait.
template <int NQ>
__device__ __forceinline__ void warm_query_lines(const const_f32p (&qs)[4], int byte_off, int byte_end, float &sink) {
    for (int off = byte_off; off < byte_end; off += 64) {
#pragma unroll
        for (int jq = 0; jq < NQ; ++jq) asm volatile("s_load_dword %0, %1, %2" : "+s"(sink) : "s"(qs[jq]), "s"(off));
    }
}
__device__ __forceinline__ void warm_query_lines_done(float &sink) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(sink)::"memory");
}

// ---- corpus storage (NLSH_STORE_*, nlsh_scan_topk_cells_phase_typed) ------------------------------------------------------------
// A 16-byte LDS slot -- one float4 chunk of a row -- is 16 / 8 / 4 bytes of a float32 / float16 / uint8 corpus in memory.  The staging
// code loads the chunk's `word`, keeps it narrow in the staging registers while the load is in flight and converts it to float4 when the
// tile is written (`widen`: exact conversions, plain C++ -- v_cvt_f32_f16 / v_cvt_f32_ubyte0..3 as compiled).  Everything behind the
// tile -- the k-blocks, the query side, the epilogues -- is the same code on the same float32 values: a typed index answers with the
// bits of the float32 index over the dequantised rows, and the conversion is paid per (task, row element), never per query.
// The float32 form is the identity on float4: the float32 kernels are the instantiations they were.
template <int STORE> struct Stored;
template <> struct Stored<NLSH_STORE_F32> {
    typedef float4 word;
    static __device__ __forceinline__ float4 widen(float4 w) { return w; }
    static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <> struct Stored<NLSH_STORE_F16> {
    typedef uint2 word;     // four halves
    static __device__ __forceinline__ float4 widen(uint2 w) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 lo = __builtin_bit_cast(h2, w.x), hi = __builtin_bit_cast(h2, w.y);
        return make_float4((float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y);
    }
    static __device__ __forceinline__ uint2 zero() { return make_uint2(0u, 0u); }
};
template <> struct Stored<NLSH_STORE_U8> {
    typedef uint32_t word;  // four bytes
    static __device__ __forceinline__ float4 widen(uint32_t w) {
        return make_float4((float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24));
    }
    static __device__ __forceinline__ uint32_t zero() { return 0u; }
};
// The affine form (storage="sq8"; bscana_kernel): the word is uint8 storage's, and `widen` takes the chunk's four offsets and steps --
// deq(c, j) = float(c) * step[j] + lo[j], a multiply and an add with a rounding each (the library is built with -ffp-contract=off: no
// fused multiply-add), which is `codes.float() * step + lo` in torch.  The staging code requests lo4 / step4 of its chunk column beside
// the row words (the padded arrays are <= 8 KB and stay in the cache); behind the tile the values are float32 like every other storage's.
template <> struct Stored<NLSH_STORE_SQ8> {
    typedef uint32_t word;
    static __device__ __forceinline__ float4 widen(uint32_t w, const float4 lo, const float4 st) {
        const float4 c = Stored<NLSH_STORE_U8>::widen(w);
        return make_float4(c.x * st.x + lo.x, c.y * st.y + lo.y, c.z * st.z + lo.z, c.w * st.w + lo.w);
    }
    static __device__ __forceinline__ uint32_t zero() { return 0u; }
};
// The product-quantised form (storage="pq"; bscanq_kernel): a row is M code bytes, and what is staged is the DECODED chunk -- the float4 of
// the codebook entry its code byte names, a copy without arithmetic.  The staging registers hold float4s like the
// float32 form's, `widen` is the identity, and the staging code of l2_task / l2_task_single does the two dependent loads.
template <> struct Stored<NLSH_STORE_PQ> {
    typedef float4 word;
    static __device__ __forceinline__ float4 widen(float4 w) { return w; }
    static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};

// All k-blocks of one L2 task for a wave that holds NQ (0..4) of its queries, NTL = tiles of the task (1..4): staging
// (global -> registers -> LDS, next k-block's loads in flight during the current one) + the hand-scheduled k-blocks.
// The (NQ, NTL) pair is chosen ONCE per task, outside the k-block loop: chosen per k-block, the 16 accumulators crossed
// a 16-way switch every k-block and the register allocator copied all of them in and out each time (466 v_mov in the
// kernel, +67 % instructions on small shapes).  NTL also fixes the fat-stage geometry at compile time.
// (WIDEK changes nothing in here: it gives the wide-k kernels instantiations of their own.  The stage_load lambda below is an ordinary
// function that the compiler inlines by its own judgement, and with a second kernel calling the SAME instantiation it judged differently:
// the k <= 64 kernels' staging code changed and took three more VGPRs.)
// (STORE: the corpus storage, see Stored above; a typed kernel's task bodies are instantiations of their own for the same reason.)
template <int NW, int NQ, int NTL, int METRIC = NLSH_METRIC_L2_EPS, bool WIDEK = false, int STORE = NLSH_STORE_F32>
__device__ __forceinline__ void l2_task(float4 *tile, const typename Stored<STORE>::word *corpus4, long long stride4, int d4, int row0, int nrows,
                                        const const_f32p (&qs)[4], int tid, int lane, float (&acc)[4][4],
                                        [[maybe_unused]] unsigned long long (&tr)[3],
                                        [[maybe_unused]] const float4 *qlo = nullptr, [[maybe_unused]] const float4 *qstep = nullptr,
                                        [[maybe_unused]] const PqArgs *pq = nullptr) {
    constexpr int NTH = 64 * NW, KB = NLSH_TILED_KB;
    // A task costs ~15 us before it does any work (r01 trace: 16 us for 1 query x <= 64 rows, 55 us for 16 x 256): one
    // exposed global-load round trip + two barriers per k-block.  Short segments therefore take FATTER k-blocks --
    // the LDS tile holds 256 rows x KB chunks = 64 rows x 4*KB chunks: 1 tile -> 4*KB chunks per stage, 2 tiles ->
    // 2*KB -- and go through a quarter / half of the stages (a third of the tasks of the headline run are <= 128 rows).
    constexpr int kshift = NTL <= 1 ? 2 : (NTL == 2 ? 1 : 0);
    constexpr int KBt = KB << kshift, RSt = KBt + 1, RPPt = (NTH / KB) >> kshift, SPT = 256 * KB / NTH;
    const int nkb = (d4 + KBt - 1) / KBt;
    const int sc = tid & (KBt - 1), sr = tid / KBt;   // staging map: KBt threads cover 16*KBt contiguous bytes of a row
    typename Stored<STORE>::word stg[SPT];
    // (NLSH_STORE_SQ8: every staged word of a thread lies in ONE chunk column per stage, so its offsets and steps are one pair of
    // 16-byte loads per stage, in flight with the row words)
    [[maybe_unused]] float4 lo_c, step_c;
    // Rows past the end of the segment and chunks past the end of a row are CLAMPED, not zero-filled: the clamped loads read valid
    // memory, rows >= nrows are masked at the epilogue (`valid`) and a k-block only evaluates its `nchunk` real chunks.  Guarded,
    // every staged word sat behind its own exec mask + branch + zero fill: ~22 VALU, 12 SALU and 4 branches per stage and wave.
    // (r04: a SECOND register set -- two k-blocks of a wave's rows in flight, for the waves that hold <= 0 / 1 / 2 / 4 of the task's
    // queries -- measured equal on all three workloads at 76 / 80 VGPRs and 3-6 % slower at 88: DESIGN.md appendix A.)
    const typename Stored<STORE>::word *rowp[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) rowp[i] = corpus4 + (long long)(row0 + min(sr + RPPt * i, nrows - 1)) * stride4;
    // (NLSH_STORE_PQ: a staged slot is two DEPENDENT loads -- the code byte of (row, gc / cps), then the float4 that byte names in the
    // codebook.  The code bytes run ONE STAGE AHEAD of the gathers: stage_load(kb) gathers with the bytes it holds and requests those of
    // stage kb + 1 behind them, so a gather's address is a whole k-block old when it is needed and only the task's first byte load is
    // an exposed round trip.  Four registers per thread; a thread's bytes of the whole task would be M per row, up to 256.  A clamped
    // slot (row nrows - 1, chunk d4 - 1) names a real code byte, and any byte a real entry: (d4 - 1) / cps < M.)
    [[maybe_unused]] const uint8_t *crow[SPT];
    [[maybe_unused]] uint32_t pcode[SPT];
    [[maybe_unused]] const float4 *pcb = nullptr;
    [[maybe_unused]] int psh = 0, pmask = 0;
    if constexpr (STORE == NLSH_STORE_PQ) {
        pcb = pq->cb4; psh = pq->cps >> 1; pmask = pq->cps - 1;   // cps 1 / 2 / 4 -> shift 0 / 1 / 2
#pragma unroll
        for (int i = 0; i < SPT; ++i)
            crow[i] = reinterpret_cast<const uint8_t *>(corpus4) + (long long)(row0 + min(sr + RPPt * i, nrows - 1)) * pq->pitch;
    }
    [[maybe_unused]] auto code_load = [&](int kb) {
        const int m = min(kb * KBt + sc, d4 - 1) >> psh;
#pragma unroll
        for (int i = 0; i < SPT; ++i) pcode[i] = crow[i][m];
    };
    auto stage_load = [&](int kb) {
        const int gc = min(kb * KBt + sc, d4 - 1);
        if constexpr (STORE == NLSH_STORE_PQ) {
            const float4 *e = pcb + (((gc >> psh) * 256) << psh) + (gc & pmask);
#pragma unroll
            for (int i = 0; i < SPT; ++i) stg[i] = e[pcode[i] << psh];
            if (kb + 1 < nkb) code_load(kb + 1);
        } else {
#pragma unroll
            for (int i = 0; i < SPT; ++i) stg[i] = (NLSH_ABLATE != 2 && NLSH_ABLATE != 12 && NLSH_ABLATE != 13) ? rowp[i][gc] : Stored<STORE>::zero();
            if constexpr (STORE == NLSH_STORE_SQ8) { lo_c = qlo[gc]; step_c = qstep[gc]; }
        }
    };
    if constexpr (STORE == NLSH_STORE_PQ) code_load(0);
    stage_load(0);
    float qsink = 0.0f;
    asm volatile("" : "+s"(qsink));
    if (NQ > 0) warm_query_lines<(NQ > 0 ? NQ : 1)>(qs, 0, min(KBt, d4) * 16, qsink);
    for (int kb = 0; kb < nkb; ++kb) {
        [[maybe_unused]] const unsigned long long ta = SCAN_NOW();
        NLSH_STAGE_SYNC();  // everyone has finished reading the previous k-block
        [[maybe_unused]] const unsigned long long tb = SCAN_NOW();
#pragma unroll
        for (int i = 0; i < SPT; ++i) {
            if constexpr (STORE == NLSH_STORE_SQ8) tile[(sr + RPPt * i) * RSt + sc] = Stored<STORE>::widen(stg[i], lo_c, step_c);
            else tile[(sr + RPPt * i) * RSt + sc] = Stored<STORE>::widen(stg[i]);
        }
        NLSH_STAGE_SYNC();
        if (kb + 1 < nkb) stage_load(kb + 1);  // in flight while this k-block is computed
        // (r05: the queries' published bounds requested HERE in front of the last k-block, whose staging registers are free, instead of
        // behind it: the eight registers stay live across the 20 task bodies' joins -- 80 VGPRs, 6 waves per SIMD)
        [[maybe_unused]] const unsigned long long tc = SCAN_NOW();
        tr[0] += tb - ta;   // first barrier: the slowest wave's previous k-block
        tr[1] += tc - tb;   // own stage data (vmcnt) + LDS write + second barrier
        if (NQ > 0) warm_query_lines_done(qsink);   // behind the two barriers: the lines of this k-block are in the scalar cache
        if (NQ > 0 && NLSH_ABLATE != 1 && NLSH_ABLATE != 6 && NLSH_ABLATE != 13) {
            const int nchunk = min(KBt, d4 - kb * KBt);
            const_f32p qk[4];
#pragma unroll
            for (int jq = 0; jq < 4; ++jq) qk[jq] = qs[jq] + kb * KBt * 4;
            l2_kblock<(NQ > 0 ? NQ : 1), NTL, METRIC>(tile + lane * RSt, RSt, nchunk, qk, acc);
            if (kb + 1 < nkb) warm_query_lines<(NQ > 0 ? NQ : 1)>(qs, (kb + 1) * KBt * 16, min((kb + 2) * KBt, d4) * 16, qsink);
#ifdef NLSH_SCAN_TRACE
            asm volatile("" : "+v"(acc[0][0]));
            tr[2] += SCAN_NOW() - tc;
#endif
        }
    }
    // No warm-up load is in flight here (the last k-block issues none: its range is empty), but only the loop bounds say so.
    // One wait makes it a property of the control-flow graph, which is what tools/isa_lint.py checks: the sink register is
    // released on EVERY path into the epilogue, whatever a future compiler makes of the loop.
    if (NQ > 0) warm_query_lines_done(qsink);
}

// Single-stage task (r05): a task whose rows x 16-byte chunks fit the workgroup's LDS stage at once (rows * d4 <= 1024 slots: <= 40 rows
// of a 100-d corpus, <= 32 of a 128-d one) is staged in ONE pass -- four loads per thread over the rows' contiguous bytes, one barrier --
// and scored by ONE k-block call over all d4 chunks.  The fat two-stage form it replaces for such tasks cut every row at byte 256: rows
// of 400 bytes are not aligned to the 128-byte lines of the L2, so nearly every line held bytes of both stages and was requested twice,
// a whole stage apart -- on the balanced workloads, whose scan is bound by the memory system (the load skeleton alone is 0.10 of GloVe's
// 0.12 ms), the counters saw 1.33x the bytes the task table accounts for (profiles/r05_traffic_tally.txt).  Here every line of the task
// is requested once, and the task has one exposed round trip less.  Same k-ascending fmaf chain per (row, query): same bits.
constexpr int SINGLE_STAGE_SLOTS = 1024;   // float4 slots one pass of the 256 threads stages (4 each)
template <int NW, int NQ, int METRIC = NLSH_METRIC_L2_EPS, int STORE = NLSH_STORE_F32>
__device__ __forceinline__ void l2_task_single(float4 *tile, const typename Stored<STORE>::word *corpus4, long long stride4, int d4, int row0, int nrows,
                                               const const_f32p (&qs)[4], int tid, int lane, float (&acc)[4][4],
                                               [[maybe_unused]] const float4 *qlo = nullptr, [[maybe_unused]] const float4 *qstep = nullptr,
                                               [[maybe_unused]] const PqArgs *pq = nullptr) {
    constexpr int NTH = 64 * NW, SPT = SINGLE_STAGE_SLOTS / NTH;
    const int RS = d4 | 1;                   // odd LDS row stride (16-byte slots): conflict-free column reads
    const int total = nrows * d4;
    const float inv = 1.0f / (float)d4;
    // (r05: the pass started at the 128-byte line below the task's first byte, so that every wave-load covered whole lines of the L2: the
    // counters did not move -- 289.6 against 289.5 K FETCH_SIZE units per GloVe launch -- and the shift was removed; DESIGN.md appendix A.)
    typename Stored<STORE>::word stg[SPT];
    int dst[SPT];
    [[maybe_unused]] int col[SPT];   // NLSH_STORE_SQ8: the slot's chunk column, whose offsets and steps are read where the tile is written
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int idx = min(tid + NTH * i, total - 1);   // slots past the task's last chunk re-read it (valid address, value never written)
        int r = (int)((float)idx * inv);                  // idx / d4 without an integer division: off by at most one, put right below
        r -= (r * d4 > idx) ? 1 : 0;
        r += ((r + 1) * d4 <= idx) ? 1 : 0;
        const int c = idx - r * d4;
        if constexpr (STORE == NLSH_STORE_PQ) {   // the slot's code byte, then the float4 it names: both loads exposed, once per task
            const int psh = pq->cps >> 1, m = c >> psh;
            const uint32_t code = reinterpret_cast<const uint8_t *>(corpus4)[(long long)(row0 + r) * pq->pitch + m];
            stg[i] = pq->cb4[((m * 256 + (int)code) << psh) + (c & (pq->cps - 1))];
        } else
        stg[i] = (NLSH_ABLATE != 2 && NLSH_ABLATE != 12 && NLSH_ABLATE != 13) ? corpus4[(long long)(row0 + r) * stride4 + c] : Stored<STORE>::zero();
        dst[i] = r * RS + c;
        if constexpr (STORE == NLSH_STORE_SQ8) col[i] = c;
    }
    float qsink = 0.0f;
    asm volatile("" : "+s"(qsink));
    if (NQ > 0) warm_query_lines<(NQ > 0 ? NQ : 1)>(qs, 0, d4 * 16, qsink);
    // one task per workgroup: nobody has read the tile before, so the writes need no barrier in front of them
#pragma unroll
    for (int i = 0; i < SPT; ++i)
        if (tid + NTH * i < total) {
            if constexpr (STORE == NLSH_STORE_SQ8) tile[dst[i]] = Stored<STORE>::widen(stg[i], qlo[col[i]], qstep[col[i]]);
            else tile[dst[i]] = Stored<STORE>::widen(stg[i]);
        }
    NLSH_STAGE_SYNC();
    if (NQ > 0) {
        warm_query_lines_done(qsink);
        if (NLSH_ABLATE != 1 && NLSH_ABLATE != 6 && NLSH_ABLATE != 13) {
            const_f32p qk[4];
#pragma unroll
            for (int jq = 0; jq < 4; ++jq) qk[jq] = qs[jq];
            // lanes past the task's last row walk its last row (staged data; their results are masked at the epilogue)
            l2_kblock<(NQ > 0 ? NQ : 1), 1, METRIC>(tile + min(lane, nrows - 1) * RS, RS, d4, qk, acc);
        }
    }
}

template <int NW, int NQ, int METRIC = NLSH_METRIC_L2_EPS, bool WIDEK = false, int STORE = NLSH_STORE_F32>
__device__ __forceinline__ void l2_task_nt(int ntile, float4 *tile, const typename Stored<STORE>::word *corpus4, long long stride4, int d4, int row0, int nrows,
                                           const const_f32p (&qs)[4], int tid, int lane, float (&acc)[4][4], unsigned long long (&tr)[3],
                                           [[maybe_unused]] const float4 *qlo = nullptr, [[maybe_unused]] const float4 *qstep = nullptr,
                                           [[maybe_unused]] const PqArgs *pq = nullptr) {
    if constexpr (STORE == NLSH_STORE_SQ8 || STORE == NLSH_STORE_PQ) {   // the same switch, the quantiser / the codebook handed on
        switch (ntile) {
            case 0: l2_task_single<NW, NQ, METRIC, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, qlo, qstep, pq); break;
            case 1: l2_task<NW, NQ, 1, METRIC, WIDEK, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, tr, qlo, qstep, pq); break;
            case 2: l2_task<NW, NQ, 2, METRIC, WIDEK, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, tr, qlo, qstep, pq); break;
            case 3: l2_task<NW, NQ, 3, METRIC, WIDEK, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, tr, qlo, qstep, pq); break;
            default: l2_task<NW, NQ, 4, METRIC, WIDEK, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, tr, qlo, qstep, pq); break;
        }
        return;
    }
    switch (ntile) {
        case 0: l2_task_single<NW, NQ, METRIC, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc); break;   // "0 tiles": the single-stage body
        case 1: l2_task<NW, NQ, 1, METRIC, WIDEK, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, tr); break;
        case 2: l2_task<NW, NQ, 2, METRIC, WIDEK, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, tr); break;
        case 3: l2_task<NW, NQ, 3, METRIC, WIDEK, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, tr); break;
        default: l2_task<NW, NQ, 4, METRIC, WIDEK, STORE>(tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, tr); break;
    }
}

// QW queries per wave, NW waves per workgroup (QW*NW queries per task), TPS 64-row tiles per task.
// k-blocks of KB chunks are the OUTER loop: one stage holds the KB-chunk slice of ALL 64*TPS rows of
// the segment in LDS, so every scalar-loaded query chunk is applied to TPS row tiles (TPS x fewer
// scalar loads and SALU per VALU than a tile-outer loop) and the accumulators of all tiles live in
// registers until the last k-block.  Chunks go through two scalar register sets: the s_loads of
// chunk c+1 are issued before chunk c is evaluated.
// One task of the tiled schedule, start to finish (operands of the task already requested by the caller: descriptor and
// the wave's query ids).  `tile` = the workgroup's LDS stage.
// WIDEK (compile time): k in 65..NLSH_MAX_K_TILED -- the epilogue's selection pads its k-key list with a lane-strided loop; everything in
// front of the epilogue is the same code, so every distance keeps its bits.
// FILT (compile time; nlsh_scan_topk_cells_phase_filtered): `side->row_filter` is a bitset over the sorted rows (bit p & 31 of word p >> 5:
// row p may be returned).  The lane's word of every tile is requested beside its row id at the top of the task and its bit enters `mine` in
// the epilogue: a denied row is dropped in front of the selection and changes nothing in staging, in the k-blocks or in a distance.
// Off (the default), neither the parameter nor the words exist in the code.
// RANGE (compile time; nlsh_range_count / nlsh_range_fill, bscanr_kernel): the RANGE EPILOGUE in place of the selection.  Everything up to
// the epilogue is the same code, so every distance keeps its bits; per (task, slot) list a candidate is a hit iff it is `mine` and
// dist <= range->radius[q] (IEEE float32: a NaN distance never is, +inf only at radius +inf), the hits are counted with ballots over the
// TPS tiles and lane 0 adds the count to range->counter[q] -- the whole answer in count mode; in fill mode the add's result is the
// list's first slot of the query's segment and every hit lane stores its key at row_offsets[q] + slot (mbcnt ranks, as in
// select_k_smallest's compaction).  tauq and partial are not touched.  side->row_filter (nullable) is the filter, a run-time operand
// here: a null pointer gives every lane an all-ones word.  Off (the default), neither the parameter nor the code exists.
// TAGS (compile time; nlsh_scan_topk_cells_phase_tagged / _sq8_tagged, bscang_kernel): per-query tag filters.  Every sorted row carries a
// 64-bit tag word (side->tags, read with the row position the lane already has: 8 bytes per lane and tile, coalesced), every query a 64-bit
// mask (side->qmask[q], wave-uniform: a scalar load per query of the wave, of the slot's own query -- qid[jq] is the id of slot
// NLSH_SLOT(wave, jq), clamped as everywhere) and the call one match mode.  Tags, masks and the optional bitset bit (side->row_filter) are
// folded into ONE register of 16 pass bits (bit tl * QW + jq) in front of the task bodies, so that neither the tag words nor the filter
// words are live during the arithmetic; bit (tl, jq) enters `mine` in the epilogue.  A denied row changes nothing in staging, in the
// k-blocks or in a distance.  With STORE == NLSH_STORE_SQ8 the quantiser is side->lo4 / step4, as in the affine kernels.  Off (the
// default), none of it exists.
template <int METRIC, int QW, int NW, int TPS, bool WIDEK = false, int STORE = NLSH_STORE_F32, bool FILT = false, bool RANGE = false,
          bool TAGS = false>
__device__ __forceinline__ void tiled_task_body(const BArgs &a, float4 *tile, long long t, const int4 desc, const int2 qr_all, int tid, int lane,
                                                int wave, [[maybe_unused]] unsigned long long ts_entry,
                                                [[maybe_unused]] const SideArgs *side = nullptr,
                                                [[maybe_unused]] const RangeArgs *range = nullptr,
                                                [[maybe_unused]] const PqArgs *pq = nullptr) {
    static_assert(!(RANGE && (FILT || WIDEK)), "the range epilogue takes its filter as a nullable run-time operand and selects nothing");
    static_assert(!(TAGS && (FILT || RANGE)), "the tagged kernels take their filter as a nullable run-time operand and have no range epilogue");
    // AFFINE (STORE == NLSH_STORE_SQ8; nlsh_scan_topk_cells_phase_sq8, bscana_kernel): the staging code decodes with side->lo4 / step4,
    // and the filter is a nullable run-time operand as in the range kernels.  Off, none of it exists in the code.
    constexpr bool AFFINE = STORE == NLSH_STORE_SQ8;
    static_assert(!(AFFINE && (FILT || RANGE)), "the affine kernels take their filter as a nullable run-time operand and have no range epilogue");
    // SIDE: the forms that read `side` at all; in the others neither the parameter nor the filter words exist in the code
    // PQ (STORE == NLSH_STORE_PQ; nlsh_scan_topk_cells_phase_pq, bscanq_kernel): the staging code gathers from pq->cb4 by the rows' code
    // bytes, and the filter is a nullable run-time operand as in the affine kernels.  Off, none of it exists in the code.
    constexpr bool PQ = STORE == NLSH_STORE_PQ;
    static_assert(!(PQ && (FILT || RANGE || TAGS)), "the PQ kernels take their filter as a nullable run-time operand and have neither tags nor a range epilogue");
    constexpr bool SIDE = FILT || RANGE || AFFINE || TAGS || PQ;
    static_assert(QW == 4 && TPS == 4 && NW == 4, "the hand-scheduled task bodies (l2_task_nt) are written for 4 waves x 4 queries x 4 row tiles");
#ifdef NLSH_SCAN_TRACE_CLOCK
    const unsigned long long ts0 = SCAN_NOW();
    const unsigned long long core0 = __builtin_amdgcn_s_memtime();   // shader-clock counter beside the 100 MHz stamps: the clock held
#endif
    const int nq = __builtin_amdgcn_readfirstlane(desc.y);       // desc.x (first pair of the group) is the wave-level schedule's: the tiled tasks carry their query ids
    // The task's rows, narrowed to the hull of the rows its queries own: a 64-row window shared by several small buckets is staged and
    // scored from the first row of its first PROBED bucket to the last row of its last one (GloVe-1.2M: 1.27x -> 1.10x the rows of the
    // probed buckets, profiles/r05_traffic_tally.txt; the balanced workloads' scan is bound by the bytes it moves).  The hull is the
    // min / max over the task's <= 16 slot ranges (two wave-wide DPP reductions per task; a segment of a big bucket gives itself).
    // Same rows per query, same chains: same bits.
    const bool slot_live = (lane & (QW * NW - 1)) < nq;
    const int h_lo = (int)wave_minmax_u32<false>(slot_live ? (uint32_t)(qr_all.y & 0xFFFF) : 0xFFFFu);
    const int h_hi = (int)wave_minmax_u32<true>(slot_live ? (uint32_t)(qr_all.y >> 16) : 0u);
    const int row0 = __builtin_amdgcn_readfirstlane(desc.z) + h_lo;
    const int nrows = min(h_hi, __builtin_amdgcn_readfirstlane(desc.w)) - h_lo;  // <= 64 * TPS rows (the host fixes seg = 64 * TPS)
    if (nrows <= 0) return;   // wave-uniform, in front of every barrier: slot records a stale counter invented (workspace contract; bmerge flags it)
    // queries are dealt round-robin over the waves (slot = wave + NW*jq): a group of 5 queries costs the
    // workgroup 2 query-times per stage (2,1,1,1) instead of 4 (4,1,0,0); the stage barrier waits for the slowest wave
    int nqw = (nq - wave + NW - 1) / NW;
    nqw = __builtin_amdgcn_readfirstlane(nqw < 0 ? 0 : (nqw > QW ? QW : nqw));

    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const_f32p qs[QW];
    int qid[QW];
#pragma unroll
    for (int jq = 0; jq < QW; ++jq) {
        // ids clamped into [0, Q) so that a slot a stale counter invented (bmerge flags it) addresses nothing outside the queries
        qid[jq] = min(max(__builtin_amdgcn_readlane(qr_all.x, NLSH_SLOT(wave_u, jq)), 0), (int)a.Q - 1);
        qs[jq] = (const_f32p)(a.qpad + (long long)qid[jq] * a.qpad_stride);
    }

    const typename Stored<STORE>::word *corpus4 = reinterpret_cast<const typename Stored<STORE>::word *>(a.corpus);
    const long long stride4 = a.row_stride >> 2;   // row pitch in 4-element chunks, whatever the storage
    const int d4 = a.d4p;
    const int ntile = (nrows + 63) >> 6;
    float acc[TPS][QW];
#pragma unroll
    for (int tl = 0; tl < TPS; ++tl)
#pragma unroll
        for (int jq = 0; jq < QW; ++jq) acc[tl][jq] = 0.0f;

    // global row ids (and cosine norms) of the rows this lane owns: requested up front, consumed by the epilogue --
    // issued there, the load was an exposed round trip at the end of every task (r02 trace: ~2 us of a 28-us task)
    int32_t mygid[TPS];
    float myinv[TPS];
    bool valid[TPS];
    [[maybe_unused]] uint32_t myfw[TPS];   // FILT: the filter word that holds the row's bit (lanes past the task's last row: the word of row0, in range)
#pragma unroll
    for (int tl = 0; tl < TPS; ++tl) {
        valid[tl] = tl * 64 + lane < nrows;
        const int prow = row0 + (valid[tl] ? tl * 64 + lane : 0);
        mygid[tl] = valid[tl] ? a.gid[prow] : -1;
        myinv[tl] = (METRIC == NLSH_METRIC_COSINE && valid[tl]) ? a.inv_norm[prow] : 0.0f;
        // the filter word, read HERE for every form: FILT reads it without a test, the other forms take a null pointer as all ones
        if constexpr (SIDE) myfw[tl] = (FILT || side->row_filter) ? side->row_filter[prow >> 5] : 0xFFFFFFFFu;
    }
    // the quantiser, read HERE for every form
    [[maybe_unused]] const float4 *qlo = nullptr, *qstep = nullptr;
    if constexpr (AFFINE) { qlo = side->lo4; qstep = side->step4; }
    // TAGS: the 16 pass bits of the lane's (tile, query) pairs.  The masks of the wave's LIVE slots only (jq < nqw: what the epilogue
    // reads the bounds of); lanes past the task's last row hold the words of row0 and are never `valid`.  The empty asm pins the fold in
    // front of the task bodies: behind them, the eight tag registers and the filter words would live through the arithmetic.
    [[maybe_unused]] uint32_t pass = 0u;
    if constexpr (TAGS) {
        uint64_t mytag[TPS], qm[QW];
#pragma unroll
        for (int tl = 0; tl < TPS; ++tl) mytag[tl] = side->tags[row0 + (valid[tl] ? tl * 64 + lane : 0)];
#pragma unroll
        for (int jq = 0; jq < QW; ++jq) qm[jq] = jq < nqw ? side->qmask[qid[jq]] : 0ull;
        const int match = side->match;
#pragma unroll
        for (int tl = 0; tl < TPS; ++tl) {
            const bool fbit = (myfw[tl] >> ((row0 + tl * 64 + lane) & 31)) & 1u;   // valid lanes: the bit of prow
#pragma unroll
            for (int jq = 0; jq < QW; ++jq) {
                const uint64_t both = mytag[tl] & qm[jq];
                const bool ok = match == NLSH_TAG_ANY ? both != 0ull : (match == NLSH_TAG_ALL ? both == qm[jq] : mytag[tl] == qm[jq]);
                pass |= (ok && fbit && jq < nqw) ? 1u << (tl * QW + jq) : 0u;
            }
        }
        asm volatile("" : "+v"(pass));
    }
    [[maybe_unused]] unsigned long long trl[3] = {0, 0, 0};
    [[maybe_unused]] const unsigned long long ts_in = SCAN_NOW();
    // a task whose rows x chunks fit one stage takes the single-stage body (l2_task_single): selected as "0 tiles" of the same switch
    const int nt_sel = (nrows * d4 <= SINGLE_STAGE_SLOTS && nrows <= 64) ? 0 : ntile;   // wave-uniform (task shape)
    // the hand-scheduled form, specialised per (queries of this wave, tiles of the task); same barrier count on every path
    switch (nqw) {
        case 0: l2_task_nt<NW, 0, METRIC, WIDEK, STORE>(nt_sel, tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, trl, qlo, qstep, pq); break;
        case 1: l2_task_nt<NW, 1, METRIC, WIDEK, STORE>(nt_sel, tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, trl, qlo, qstep, pq); break;
        case 2: l2_task_nt<NW, 2, METRIC, WIDEK, STORE>(nt_sel, tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, trl, qlo, qstep, pq); break;
        case 3: l2_task_nt<NW, 3, METRIC, WIDEK, STORE>(nt_sel, tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, trl, qlo, qstep, pq); break;
        default: l2_task_nt<NW, 4, METRIC, WIDEK, STORE>(nt_sel, tile, corpus4, stride4, d4, row0, nrows, qs, tid, lane, acc, trl, qlo, qstep, pq); break;
    }
    if (nqw == 0) return;
    if (NLSH_ABLATE == 5 || NLSH_ABLATE == 6 || NLSH_ABLATE == 12 || NLSH_ABLATE == 13) {   // diagnostic: no epilogue at all (the accumulators are kept alive)
#pragma unroll
        for (int tl = 0; tl < TPS; ++tl)
#pragma unroll
            for (int jq = 0; jq < QW; ++jq) asm volatile("" ::"v"(acc[tl][jq]));
        return;
    }
    // lane = row of each tile -> one candidate per lane, tile and query
    // Lists of the same query in other tasks publish their k-th best key to tauq[q] (atomicMin): no
    // candidate above it can reach the final top-k, so it pre-filters this list (fewer insertions).
    // Which partial entries survive depends on timing; the merged result does not.
    // All <= 64*TPS candidates of a list exist at once here (TPS keys per lane), so the k best are
    // SELECTED (bisection + compaction, select_k_smallest) instead of inserted one by one.
    [[maybe_unused]] const unsigned long long ts3 = SCAN_NOW();
    // the running bounds of the wave's queries are requested together (one exposed round trip, not one per query)
    uint64_t tau_w[QW];
    [[maybe_unused]] float rad_w[QW];   // RANGE: the queries' radii, requested together where the bounds are (the bounds are not read)
#pragma unroll
    for (int jq = 0; jq < QW; ++jq) {
        if (RANGE) { tau_w[jq] = KEY_NONE; rad_w[jq] = jq < nqw ? range->radius[qid[jq]] : 0.0f; }
        else tau_w[jq] = jq < nqw ? global_tau_load(a.tauq + qid[jq]) : KEY_NONE;
    }
    constexpr bool LEAN = METRIC != NLSH_METRIC_COSINE;   // r05: square roots without the range scaling, sign-free key build (L2 only)
#pragma unroll
    for (int jq = 0; jq < QW; ++jq) {
        if (jq < nqw) {
            const uint64_t tau_g = tau_w[jq];
            // rows of the task that belong to THIS query's bucket: all of them for a segment of a big bucket, the bucket's slice of a
            // window shared by several small buckets (the other rows were scored for nothing: the arithmetic of a shared window is what
            // a task of its own would have cost each of those buckets in fixed latency)
            const int rng = __builtin_amdgcn_readlane(qr_all.y, NLSH_SLOT(wave_u, jq));
            const unsigned r_lo = (unsigned)((rng & 0xFFFF) - h_lo), r_n = (unsigned)(rng >> 16) - (unsigned)(rng & 0xFFFF);   // relative to the first row staged
            uint64_t key[TPS];
            [[maybe_unused]] bool hit[TPS];   // RANGE: in range (the key is then the candidate's, never KEY_NONE)
            // LEAN: every accumulator of the list at or above 2^-96 (wave-uniform test; NaN compares false and takes the general path)
            // -> square roots without the range scaling, and a non-negative distance's order-preserving word is its bits with the sign set
            bool lean = LEAN;
            // (FILT: the test stays over the task's rows, denied ones included, as it already covers the rows of a shared window's other
            // buckets: it only picks between two correctly rounded square roots, sqrt_rn_unscaled and finish_distance's sqrtf -- same bits)
            if (LEAN) {   // tiles the task does not have hold zeros and lanes past its last row another row's (or nobody's) sums: neither is asked
                bool ok = true;
#pragma unroll
                for (int tl = 0; tl < TPS; ++tl) ok = ok && (tl >= ntile || !valid[tl] || acc[tl][jq] >= 0x1p-96f);   // a NaN fails the comparison
                lean = __ballot(!ok) == 0ull;
            }
#pragma unroll
            for (int tl = 0; tl < TPS; ++tl) {
                bool mine = valid[tl] && (unsigned)(tl * 64 + lane) - r_lo < r_n;
                if (TAGS) mine = mine && ((pass >> (tl * QW + jq)) & 1u);   // tag, mask and filter bit of (tile, query), folded at the top
                else if (SIDE) mine = mine && ((myfw[tl] >> ((row0 + tl * 64 + lane) & 31)) & 1u);   // valid lanes: the bit of prow
                uint64_t kk;
                [[maybe_unused]] float dist_r;   // RANGE: the distance the key is built from, held against the radius
                if (lean) {
                    const float dist = sqrt_rn_unscaled(acc[tl][jq]);
                    kk = ((uint64_t)(__builtin_bit_cast(uint32_t, dist) | 0x80000000u) << 32) | (uint32_t)mygid[tl];   // == make_key for dist >= +0
                    dist_r = dist;
                } else {
                    const float dist = finish_distance<METRIC>(acc[tl][jq], myinv[tl]);
                    kk = make_key(dist, mygid[tl]);
                    dist_r = dist;
                }
                if (RANGE) hit[tl] = mine && dist_r <= rad_w[jq];   // a NaN distance compares false, whatever the radius
                kk = mine ? kk : KEY_NONE;
                key[tl] = kk < tau_g ? kk : KEY_NONE;  // beyond another list's k-th best: cannot reach the final top-k
            }
            if (RANGE) {
                // hits of the list: one ballot per tile; a hit lane's rank is the hits of the tiles in front of its own plus the hit
                // lanes below it (mbcnt).  One atomic per list and mode, by lane 0, and none for a list without a hit.
                unsigned long long hm[TPS];
                int n_hits = 0;
#pragma unroll
                for (int tl = 0; tl < TPS; ++tl) { hm[tl] = __ballot(hit[tl]); n_hits += __popcll(hm[tl]); }
                if (n_hits == 0) continue;   // wave-uniform
                int32_t *ctr = range->counter + qid[jq];
                if (range->mode == NLSH_RANGE_COUNT) {
                    if (lane == 0) atomicAdd(ctr, n_hits);
                    continue;
                }
                int base = 0;
                if (lane == 0) base = atomicAdd(ctr, n_hits);
                base = __builtin_amdgcn_readfirstlane(base);
                // the query's segment: a slot past its end (offsets that are not the prefix sum of THIS plan's counts) is not written,
                // and the cursor the call leaves then exceeds the segment's length
                const long long seg0 = range->row_offsets[qid[jq]], seg_n = range->row_offsets[qid[jq] + 1] - seg0;
#pragma unroll
                for (int tl = 0; tl < TPS; ++tl) {
                    const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(hm[tl] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm[tl], 0u));
                    if (hit[tl] && pos >= 0 && pos < seg_n && seg0 >= 0 && seg0 + pos < range->total) range->keys[seg0 + pos] = key[tl];
                    base += __popcll(hm[tl]);
                }
                continue;
            }
            uint64_t *out = a.partial + ((long long)t * (QW * NW) + NLSH_SLOT(wave, jq)) * a.k;
#ifdef NLSH_SCAN_TRACE_EPILOGUE
            {   // diagnostic: how many (task, query) lists reach the selection with a published bound, and with how many survivors
                int n_all = 0, n_live = 0;
#pragma unroll
                for (int tl = 0; tl < TPS; ++tl) { n_all += __popcll(__ballot(valid[tl])); n_live += __popcll(__ballot(key[tl] != KEY_NONE)); }
                if (lane == 0) {
                    float *c = g_scan_trace + (NLSH_TRACE_SLOTS - 1) * 8;
                    atomicAdd(c + 0, 1.0f);
                    if (tau_g != KEY_NONE) atomicAdd(c + 1, 1.0f);
                    if (n_live == 0) atomicAdd(c + 2, 1.0f);
                    else if (n_live < a.k) atomicAdd(c + 3, 1.0f);
                    atomicAdd(c + 4, (float)n_all);
                    atomicAdd(c + 5, (float)n_live);
                }
            }
#endif
            if (NLSH_ABLATE != 3) {
                // (r04: one-tile tasks selecting from ONE key per lane instead of TPS with three absent -- a quarter of the ballots per
                // bisection step -- measured equal on all three workloads, profiles/r04_select_nk1_ab.txt; not kept)
                const uint64_t bound = select_k_smallest<TPS, false, WIDEK>(key, a.k, lane, out);
                if (bound != KEY_NONE && lane == 0) atomicMin(a.tauq + qid[jq], (unsigned long long)bound);
            } else if (lane < a.k) out[lane] = key[0];
        }
    }
#ifdef NLSH_SCAN_TRACE
    if (tid == 0 && t < NLSH_TRACE_SLOTS) {
        const unsigned long long ts4 = SCAN_NOW();
        float *o = g_scan_trace + t * 8;
        o[0] = (float)(ts4 - ts_entry); o[1] = (float)(ts_in - ts_entry); o[2] = (float)trl[0]; o[3] = (float)trl[2];
        o[4] = (float)trl[1]; o[5] = (float)(ts4 - ts3); o[6] = (float)(nq * 1000 + nrows); o[7] = (float)(ts_entry & 0xFFFFFFull);
#ifdef NLSH_SCAN_TRACE_HWID   // (r05's placement analysis: overwrites the barrier-1 and compute columns)
        // where it ran: HW_ID (wave/simd/cu/sh/se) and XCC_ID, as exact small integers
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        o[2] = (float)(((xcc & 0xF) << 12) | (((hw >> 13) & 0x7) << 9) | (((hw >> 12) & 0x1) << 8) | (((hw >> 8) & 0xF) << 4) | (((hw >> 4) & 0x3) << 2));
        o[3] = (float)(hw & 0xF);
#endif
#ifdef NLSH_SCAN_TRACE_CLOCK
        o[4] = (float)(__builtin_amdgcn_s_memtime() - core0); o[1] = (float)(ts4 - ts0);   // core cycles and 100 MHz ticks of the same interval
#endif
    }
#endif
}


// The task pick of every tiled kernel: after it `t` (task id), `desc` (its descriptor) and `qr_all` (its slot records) are in scope, and a
// workgroup past the task count has returned.  Needs `a` (BArgs), `lane`, QW and NW.  A MACRO, not a function: as a __forceinline__ function
// that returns the three through references the compiler merges the two slot-record dwords into one load and re-orders the hot loops of
// bscan3_kernel and bscanw_kernel (profiles/scan_side_args.txt); expanded in each __global__ it is the text every kernel carried, and the
// kernels are the code they were.
//   - status: a task count above the table is clamped and flagged incomplete -- the caller must retry (a refusal of the PLAN phase, 2 or
//     3, stays).
//   - Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an L2).  Task ids are dealt to the XCDs in CHUNKS of 16
//     consecutive ids: the query groups of one row segment (consecutive ids) mostly land on one XCD and re-read its rows from that L2
//     instead of HBM, while every XCD still walks the size-ordered task list front to back (a contiguous 1/8 range per XCD would hand all
//     the heavy tasks to XCD 0).  Placement only changes speed, never results.
//   - The descriptor is requested BEFORE the task count is known (index clamped into the table): one dependent round trip less in front
//     of every task.
//   - All 16 {query id, row range} records of the task come in ONE load, one record per lane (& 15) -- address known from the task id
//     alone, requested with the descriptor.  A wave picks its own slots out of it with v_readlane (r04: four 8-byte loads per wave), and
//     the hull of the rows the task's queries own at all is taken over all sixteen (r05).  Slots >= nq hold garbage, never used.
//   - (r06: cross-task prefetch into the XCD's L2 -- a finished workgroup touching the rows of the task 1792-3072 ids ahead on its XCD
//     with loads nobody waits for -- was built and is NOT here: every run of it ended in a GPU exception.  Cause not established: only
//     queue dumps were kept, and the form that did not fault differed in distance, task class and the wait.  With the wait in front of
//     s_endpgm the workgroup's slot is held for exactly the HBM miss the prefetch was meant to hide.  DESIGN.md appendix A.)
#define NLSH_TILED_PICK(a)                                                                   \
    long long ntasks = (a).status[0];                                                        \
    if (ntasks > (a).max_tasks) {                                                            \
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&(a).status[1], 1);               \
        ntasks = (a).max_tasks;                                                              \
    }                                                                                        \
    constexpr int XC = 16;                                                                   \
    const long long j = blockIdx.x >> 3;                                                     \
    const long long t = ((j / XC) * 8 + (blockIdx.x & 7)) * XC + (j % XC);                   \
    const long long tc = t < (a).max_tasks ? t : (a).max_tasks - 1;                          \
    const int4 desc = (a).task[tc];                                                          \
    const int2 qr_all = (a).task_qr[tc * (QW * NW) + (lane & (QW * NW - 1))];                \
    if (t >= ntasks) return

// The eight kernels below are shells: the LDS stage, the pick, one call of tiled_task_body.  The stage is declared in each __global__:
// handed to a shared function, or declared in one, its address stops being a compile-time constant of the staging code and the float32
// kernels' instructions change.  Each is a kernel of its own name with task bodies of its own instantiation, in a translation unit of
// its own where it says so, so that the kernels in front of it keep their code and their register / occupancy budget; BArgs keeps its
// layout, and what a form needs beside it rides in a second parameter (SideArgs, RangeArgs: scan_bucket_args.h).

// The tiled scan over a float32 corpus, k <= 64: what every default call runs.
template <int METRIC, int QW, int NW, int TPS>
__global__ __launch_bounds__(64 * NW, 1) void bscan3_kernel(BArgs a) {
    constexpr int KB = NLSH_TILED_KB;        // 16-byte chunks per k-block
    constexpr int RS = KB + 1;               // odd LDS row stride (16-byte slots) -> conflict-free column reads
    constexpr int ROWS = 64 * TPS;
    __shared__ float4 tile[ROWS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] const unsigned long long ts_entry = SCAN_NOW();
    NLSH_TILED_PICK(a);
    if (NLSH_ABLATE == 9) return;   // diagnostic: every workgroup leaves after its descriptor loads (what dispatching the grid costs)
    if (NLSH_ABLATE == 8 && desc.y <= 4) return;   // diagnostic: tasks with few queries vanish (what the low-density tasks cost)
    if (NLSH_ABLATE == 7 && desc.w <= 64) return;   // diagnostic: tasks of <= 64 rows vanish (what a kernel without the tail of tiny tasks would take)
    tiled_task_body<METRIC, QW, NW, TPS>(a, tile, t, desc, qr_all, tid, lane, wave, ts_entry);
}

// k in 65..NLSH_MAX_K_TILED: bscan3_kernel with the wide epilogue.
template <int METRIC, int QW, int NW, int TPS>
__global__ __launch_bounds__(64 * NW, 1) void bscanw_kernel(BArgs a) {
    constexpr int RS = NLSH_TILED_KB + 1;
    __shared__ float4 tile[64 * TPS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] const unsigned long long ts_entry = SCAN_NOW();
    NLSH_TILED_PICK(a);
    tiled_task_body<METRIC, QW, NW, TPS, true>(a, tile, t, desc, qr_all, tid, lane, wave, ts_entry);
}

// A float16 / uint8 corpus (STORE: NLSH_STORE_F16 | NLSH_STORE_U8; nlsh_scan_topk_cells_phase_typed), k <= 64 (WIDEK false) and k in
// 65..NLSH_MAX_K_TILED (true).  Instantiated in scan_bucket_typed.hip (profiles/corpus_storage.txt).
template <int METRIC, int QW, int NW, int TPS, int STORE, bool WIDEK>
__global__ __launch_bounds__(64 * NW, 1) void bscant_kernel(BArgs a) {
    static_assert(STORE == NLSH_STORE_F16 || STORE == NLSH_STORE_U8, "the float32 corpus has bscan3_kernel / bscanw_kernel");
    constexpr int RS = NLSH_TILED_KB + 1;
    __shared__ float4 tile[64 * TPS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] const unsigned long long ts_entry = SCAN_NOW();
    NLSH_TILED_PICK(a);
    tiled_task_body<METRIC, QW, NW, TPS, WIDEK, STORE>(a, tile, t, desc, qr_all, tid, lane, wave, ts_entry);
}

// Behind a row filter (FILT of tiled_task_body; nlsh_scan_topk_cells_phase_filtered), every storage, both k classes: s.row_filter is never
// null.  Instantiated in scan_bucket_filtered.hip (profiles/row_filter.txt).
template <int METRIC, int QW, int NW, int TPS, int STORE, bool WIDEK>
__global__ __launch_bounds__(64 * NW, 1) void bscanf_kernel(BArgs a, SideArgs s) {
    constexpr int RS = NLSH_TILED_KB + 1;
    __shared__ float4 tile[64 * TPS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] const unsigned long long ts_entry = SCAN_NOW();
    NLSH_TILED_PICK(a);
    tiled_task_body<METRIC, QW, NW, TPS, WIDEK, STORE, true>(a, tile, t, desc, qr_all, tid, lane, wave, ts_entry, &s);
}

// The radius query's scan (RANGE of tiled_task_body; nlsh_range_count / nlsh_range_fill), every storage: the range epilogue.  One kernel
// per (metric, storage) serves both modes and both filter states -- r.mode and r.row_filter are wave-uniform run-time operands.  The
// kernel's parameters stay (BArgs, RangeArgs); the filter reaches the task body in a SideArgs built here, like every other form's.
// Instantiated in scan_bucket_range.hip (profiles/range_query.txt).
template <int METRIC, int QW, int NW, int TPS, int STORE>
__global__ __launch_bounds__(64 * NW, 1) void bscanr_kernel(BArgs a, RangeArgs r) {
    constexpr int RS = NLSH_TILED_KB + 1;
    __shared__ float4 tile[64 * TPS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] const unsigned long long ts_entry = SCAN_NOW();
    NLSH_TILED_PICK(a);
    const SideArgs s = {nullptr, nullptr, 0, r.row_filter, nullptr, nullptr};
    tiled_task_body<METRIC, QW, NW, TPS, false, STORE, false, true>(a, tile, t, desc, qr_all, tid, lane, wave, ts_entry, &s, &r);
}

// An sq8 corpus (STORE == NLSH_STORE_SQ8; nlsh_scan_topk_cells_phase_sq8): uint8 codes decoded per dimension with s.lo4 / s.step4 as the
// tile is written, both k classes.  One kernel per (metric, k class) serves both filter states -- s.row_filter is a wave-uniform run-time
// operand, as in the range kernels.  Instantiated in scan_bucket_affine.hip (profiles/sq8_storage.txt).
template <int METRIC, int QW, int NW, int TPS, bool WIDEK>
__global__ __launch_bounds__(64 * NW, 1) void bscana_kernel(BArgs a, SideArgs s) {
    constexpr int RS = NLSH_TILED_KB + 1;
    __shared__ float4 tile[64 * TPS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] const unsigned long long ts_entry = SCAN_NOW();
    NLSH_TILED_PICK(a);
    tiled_task_body<METRIC, QW, NW, TPS, WIDEK, NLSH_STORE_SQ8>(a, tile, t, desc, qr_all, tid, lane, wave, ts_entry, &s);
}

// A product-quantised corpus (STORE == NLSH_STORE_PQ; nlsh_scan_topk_cells_phase_pq): M code bytes per row, the staged chunk gathered from
// the codebook as the tile is written, both k classes.  One kernel per (metric, k class) serves both filter states -- s.row_filter is a
// wave-uniform run-time operand.  The codebook, the code pitch and cps are a THIRD parameter of these kernels alone (PqArgs).
// Instantiated in scan_bucket_pq.hip (profiles/pq_storage.txt).
template <int METRIC, int QW, int NW, int TPS, bool WIDEK>
__global__ __launch_bounds__(64 * NW, 1) void bscanq_kernel(BArgs a, SideArgs s, PqArgs p) {
    constexpr int RS = NLSH_TILED_KB + 1;
    __shared__ float4 tile[64 * TPS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] const unsigned long long ts_entry = SCAN_NOW();
    NLSH_TILED_PICK(a);
    tiled_task_body<METRIC, QW, NW, TPS, WIDEK, NLSH_STORE_PQ>(a, tile, t, desc, qr_all, tid, lane, wave, ts_entry, &s, nullptr, &p);
}

// Behind per-query tag filters (TAGS of tiled_task_body; nlsh_scan_topk_cells_phase_tagged / _sq8_tagged), every storage -- NLSH_STORE_SQ8
// among them --, both k classes.  One kernel per (metric, storage, k class) serves the three match modes and both filter states: s.match
// and s.row_filter are wave-uniform run-time operands.  Instantiated in scan_bucket_tagged.hip (profiles/row_tags.txt).
template <int METRIC, int QW, int NW, int TPS, int STORE, bool WIDEK>
__global__ __launch_bounds__(64 * NW, 1) void bscang_kernel(BArgs a, SideArgs s) {
    constexpr int RS = NLSH_TILED_KB + 1;
    __shared__ float4 tile[64 * TPS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] const unsigned long long ts_entry = SCAN_NOW();
    NLSH_TILED_PICK(a);
    tiled_task_body<METRIC, QW, NW, TPS, WIDEK, STORE, false, false, true>(a, tile, t, desc, qr_all, tid, lane, wave, ts_entry, &s);
}

}  // namespace nlsh
