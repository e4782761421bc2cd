// The per-wave bucket-size lookup of the budgeted probe kernels (probe_ranked.hip, probe_categorical.hip): one definition, so both
// count candidates by the same rule.
#pragma once
#include "common.h"

namespace nlsh {
namespace {

__device__ __forceinline__ uint32_t lane_read(uint32_t v, int l) {   // l is wave-uniform
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(l));
}

// 64-way search of `key` in uniq_keys [nb] (ascending as signed int32) -> its bucket's size, 0 when absent.  Everything but `lane` is
// wave-uniform.  `top` = uniq_keys[lane * ceil(nb / 64)] where that index is < nb (the first round's probes, loaded once per row).
__device__ __forceinline__ int32_t bucket_size(int32_t key, const int32_t *__restrict__ uniq, const int32_t *__restrict__ offsets,
                                               uint32_t nb, int32_t top, int lane) {
    uint32_t lo = 0, len = nb;   // the range [lo, lo + len) holds the key if anything does; len >= 1
    bool first = true;
    while (true) {
        const uint32_t step = (len + 63u) >> 6;
        const uint32_t off = (uint32_t)lane * step;          // < len + 63: no wrap for len < 2^31
        const bool valid = off < len;
        const uint32_t idx = lo + off;                          // < lo + len <= nb when valid
        int32_t v = top;
        if (!first) v = valid ? uniq[idx] : 0;
        if (step == 1u) {
            int32_t sz = 0;
            if (valid) sz = offsets[idx + 1] - offsets[idx];  // issued beside the key's load: no extra round trip
            const unsigned long long eq = __ballot(valid && v == key);
            if (eq == 0ull) return 0;
            return (int32_t)lane_read((uint32_t)sz, __ffsll((long long)eq) - 1);
        }
        const unsigned long long le = __ballot(valid && v <= key);   // ascending keys: a prefix of the valid lanes
        if (le == 0ull) return 0;                                   // below the range's first key
        const uint32_t c = (uint32_t)__popcll(le) - 1u;
        const uint32_t rest = len - c * step;                       // entries from the chosen probe to the range's end
        lo += c * step;
        len = rest < step ? rest : step;
        first = false;
    }
}

}  // namespace
}  // namespace nlsh
