// Bucket-major scan, wave-level schedule (part of the translation unit scan_bucket.hip, which defines BArgs in front of this file):
// bscan2 -- one wavefront = (bucket segment, <= 8 queries in VGPRs).
#pragma once

namespace nlsh {

// One task: stream `nrows` rows starting at row0 once, score them against the nq <= QB queries of
// the group.  FULL (nq == QB, the common case in hot buckets) compiles without per-query branches.
template <int LPR, int VPL, int METRIC, int QB, bool FULL>
__device__ __forceinline__ void bscan2_task(const BArgs &a, long long t, int pair0, int nq, int row0, int nrows, int lane) {
    constexpr int RPI = 64 / LPR;
    constexpr int U = (VPL == 1) ? 4 : (VPL == 2 ? 2 : 1);  // wave-loads per pipeline stage (two stages in flight)
    const int li = lane % LPR, sub = lane / LPR;
    float4 qv[QB][VPL];
    bool act[VPL];
    uint64_t top[QB], tau[QB];
#pragma unroll
    for (int jq = 0; jq < QB; ++jq) {
        top[jq] = KEY_NONE;
        tau[jq] = KEY_NONE;
        // clamped into [0, Q): a slot that a stale counter invented (workspace contract violated; bmerge flags it) holds whatever
        // the buffer held, and nothing may be addressed through it
        const int qi = min(max(__builtin_amdgcn_readfirstlane(a.inv_q[pair0 + ((FULL || jq < nq) ? jq : 0)]), 0), (int)a.Q - 1);
        load_query<LPR, VPL, METRIC>(a.queries + (long long)qi * a.q_stride, a.d, li, qv[jq], act);
    }

    // The segment is walked in groups of U wave-loads (U*RPI rows); groups are software-pipelined
    // through two register sets so the next group's HBM/L2 latency hides under the current group's
    // QB*U distance evaluations.  LPR/U groups make one 64-row tile (one candidate per lane).
    constexpr int GPT = LPR / U;
    const float4 *seg4 = reinterpret_cast<const float4 *>(a.corpus) + (long long)row0 * (a.row_stride >> 2) + li;
    const long long stride4 = a.row_stride >> 2;
    const int G = (nrows + U * RPI - 1) / (U * RPI);
    const int myc = li * RPI + sub;  // candidate of a tile this lane owns
    float mydist[QB];
    int32_t mygid = -1;
    float myinv = 0.0f;
    bool valid = false;

    auto load_group = [&](float4 (&cv)[U][VPL], int g) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = (g * U + u) * RPI + sub;  // row of the segment this lane group covers
            const bool ok = r < nrows;
            const float4 *rp = seg4 + (long long)r * stride4;
#pragma unroll
            for (int v = 0; v < VPL; ++v)
                cv[u][v] = (ok && act[v]) ? rp[v * LPR] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto compute_group = [&](const float4 (&cv)[U][VPL], int g) {
        const int gi = g % GPT;
        if (gi == 0) {  // tile begin
            const int tile0 = (g / GPT) * 64;
            valid = tile0 + myc < nrows;
            const int prow = row0 + tile0 + (valid ? myc : 0);
            mygid = valid ? a.gid[prow] : -1;
            if (METRIC == NLSH_METRIC_COSINE) myinv = valid ? a.inv_norm[prow] : 0.0f;
#pragma unroll
            for (int jq = 0; jq < QB; ++jq) mydist[jq] = __builtin_inff();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool mine = li == gi * U + u;
#pragma unroll
            for (int jq = 0; jq < QB; ++jq) {
                if (FULL || jq < nq) {
                    const float tot = group_sum<LPR>(row_partial<VPL, METRIC>(qv[jq], act, cv[u]));
                    mydist[jq] = mine ? tot : mydist[jq];
                }
            }
        }
        if (gi == GPT - 1 || g == G - 1) {  // tile end: offer this lane's candidate to every query's list
#pragma unroll
            for (int jq = 0; jq < QB; ++jq) {
                if (FULL || jq < nq) {
                    const float dist = finish_distance<METRIC>(mydist[jq], myinv);
                    const uint64_t key = valid ? make_key(dist, mygid) : KEY_NONE;
                    topk_offer(top[jq], tau[jq], key, a.k, lane);
                }
            }
        }
    };

    float4 cvA[U][VPL], cvB[U][VPL];
    if (G > 0) load_group(cvA, 0);
    for (int g = 0; g < G; g += 2) {
        if (g + 1 < G) load_group(cvB, g + 1);
        compute_group(cvA, g);
        if (g + 1 >= G) break;
        if (g + 2 < G) load_group(cvA, g + 2);
        compute_group(cvB, g + 1);
    }
#pragma unroll
    for (int jq = 0; jq < QB; ++jq)
        if ((FULL || jq < nq) && lane < a.k) a.partial[((long long)t * QB + jq) * a.k + lane] = top[jq];
}

template <int LPR, int VPL, int METRIC, int QB>
__global__ __launch_bounds__(256) void bscan2_kernel(BArgs a) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    long long ntasks = a.status[0];
    if (ntasks > a.max_tasks) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&a.status[1], 1);  // incomplete: caller must retry (a refusal of the PLAN phase -- 2, 3 -- stays)
        ntasks = a.max_tasks;
    }
    if (t >= ntasks) return;
    const int4 desc = a.task[t];
    const int pair0 = __builtin_amdgcn_readfirstlane(desc.x);
    const int nq = __builtin_amdgcn_readfirstlane(desc.y);
    const int row0 = __builtin_amdgcn_readfirstlane(desc.z);
    const int nrows = __builtin_amdgcn_readfirstlane(desc.w);
    if (nq == QB) bscan2_task<LPR, VPL, METRIC, QB, true>(a, t, pair0, nq, row0, nrows, lane);
    else bscan2_task<LPR, VPL, METRIC, QB, false>(a, t, pair0, nq, row0, nrows, lane);
}

}  // namespace nlsh
