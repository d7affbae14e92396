// hz_cast_plan.h -- how many rays one chunk of Terrain.cast takes (DESIGN.md section 4 clause 21, section 5).
//
// The rays of a call go in chunks.  What a chunk needs on the device besides the caller's own device arrays, per ray:
//     12 bytes for `origins` given as host memory, 12 for `directions` / `targets` given as host memory,
//     1 / 4 / 12 bytes for an `occluded` / `dist` / `point` given as host memory,
//     16 bytes for order = "sorted": keys and ray numbers, in and out, of the radix sort (its histograms come on top and are
//     not part of the budget: about 2 bytes per ray, a function of the chunk alone).
// The chunk is
//     clamp(budget / bytes per ray, rounded down to a multiple of 64, 64, min(num_rays rounded up to 64, HZ_CAST_MAX_CHUNK))
// (nothing staged and nothing sorted: the upper limit).  It is a multiple of 64 and at least 64 -- one wave of
// k_cast_closest -- and depends on num_rays only through the upper limit, so the scratch of a call that needs more than one
// chunk does not grow with num_rays.
//
// It includes nothing and names no device type, so a host program can compile it as it stands (tests/cast_plan_host.cpp runs
// it at its edges under ASan + UBSan).
#pragma once

namespace hz {

#define HZ_CAST_BUDGET (256ull << 20)            // bytes per chunk ("cast_budget" of hz_debug_set)
#define HZ_CAST_MAX_RAYS 2147483584ll            // 2^31 - 64: rays of one call
#define HZ_CAST_MAX_CHUNK (1 << 24)              // rays of one launch

struct CastPlan {
    int chunk;                          // rays per launch: a multiple of 64, >= 64
    unsigned long long per_ray;         // staged and sort bytes per ray (0: the chunk needs no memory)
    unsigned long long stage_bytes;     // chunk * per_ray
};

// false: num_rays below 1 or above HZ_CAST_MAX_RAYS, or no budget (the caller's HZ_ERR_ARG)
inline bool cast_plan(long long num_rays, bool stage_origins, bool stage_ends, bool stage_occluded, bool stage_dist,
                      bool stage_point, bool sorted, unsigned long long budget, CastPlan *plan) {
    if (num_rays < 1 || num_rays > HZ_CAST_MAX_RAYS || budget < 1) return false;
    const unsigned long long per_ray = (stage_origins ? 12ull : 0ull) + (stage_ends ? 12ull : 0ull) + (stage_occluded ? 1ull : 0ull) +
                                       (stage_dist ? 4ull : 0ull) + (stage_point ? 12ull : 0ull) + (sorted ? 16ull : 0ull);
    const unsigned long long waves = ((unsigned long long)num_rays + 63ull) / 64ull;          // at most 2^25 - 1
    unsigned long long k = waves * 64ull;
    if (k > (unsigned long long)HZ_CAST_MAX_CHUNK) k = (unsigned long long)HZ_CAST_MAX_CHUNK;
    if (per_ray) {
        const unsigned long long fit = budget / per_ray / 64ull * 64ull;
        if (fit < k) k = fit;
        if (k < 64ull) k = 64ull;
    }
    plan->chunk = (int)k;
    plan->per_ray = per_ray;
    plan->stage_bytes = k * per_ray;              // at most 2^24 * 57
    return true;
}

}  // namespace hz
