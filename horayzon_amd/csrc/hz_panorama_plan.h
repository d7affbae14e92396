// hz_panorama_plan.h -- how many observers one launch of Terrain.panorama takes (DESIGN.md section 4 clause 20, section 5).
//
// An image of one observer is elev_num x azim_num pixels, cut into tiles of 8 x 8 (one wave each).  Outputs given as host
// memory are staged on the device one chunk of observers at a time: 4 bytes per pixel for `dist`, 12 for `point`.  The chunk is
//     clamp(budget / (pixels * staged bytes per pixel), 1, min(num_obs, HZ_PANORAMA_MAX_OBS))
// (nothing staged: the upper limit), cut further so that tiles per observer * chunk stays below 2^31: (observer, tile)
// flattens into blockIdx.x.
//
// It includes nothing and names no device type, so a host program can compile it as it stands
// (tests/panorama_plan_host.cpp runs it at its edges under ASan + UBSan).
#pragma once

namespace hz {

#define HZ_PANORAMA_BUDGET (256ull << 20)        // bytes of staged output per chunk ("panorama_budget" of hz_debug_set)
#define HZ_PANORAMA_MAX_OBS 32768                // observers of one launch
#define HZ_PANORAMA_MAX_PIXELS (1ull << 30)      // elev_num * azim_num of one image
#define HZ_PANORAMA_MAX_BLOCKS (1ull << 31)      // tiles * chunk stays BELOW this

struct PanoramaPlan {
    int chunk;                          // observers per launch, >= 1
    int tiles_a, tiles_e;               // tiles of an image along the azimuth and the elevation axis
    unsigned long long tiles;           // tiles_a * tiles_e: workgroups per observer
    unsigned long long pixels;          // elev_num * azim_num
    unsigned long long stage_bytes;     // device memory of the staged outputs of one chunk (0: nothing is staged)
};

// false: a count below 1, more than HZ_PANORAMA_MAX_PIXELS pixels, or no budget (the caller's HZ_ERR_ARG)
inline bool panorama_plan(int num_obs, int azim_num, int elev_num, bool stage_dist, bool stage_point,
                          unsigned long long budget, PanoramaPlan *plan) {
    if (num_obs < 1 || azim_num < 1 || elev_num < 1 || budget < 1) return false;
    const unsigned long long pixels = (unsigned long long)azim_num * (unsigned long long)elev_num;
    if (pixels > HZ_PANORAMA_MAX_PIXELS) return false;
    plan->pixels = pixels;
    plan->tiles_a = (int)(((unsigned)azim_num + 7u) / 8u);
    plan->tiles_e = (int)(((unsigned)elev_num + 7u) / 8u);
    plan->tiles = (unsigned long long)plan->tiles_a * (unsigned long long)plan->tiles_e;
    const unsigned long long per_pixel = (stage_dist ? 4ull : 0ull) + (stage_point ? 12ull : 0ull);
    unsigned long long k = num_obs < HZ_PANORAMA_MAX_OBS ? (unsigned long long)num_obs : (unsigned long long)HZ_PANORAMA_MAX_OBS;
    if (per_pixel) {
        const unsigned long long fit = budget / (pixels * per_pixel);       // (at most 2^30 * 16: no overflow)
        if (fit < k) k = fit;
        if (k < 1) k = 1;
    }
    const unsigned long long blocks = (HZ_PANORAMA_MAX_BLOCKS - 1) / plan->tiles;     // tiles <= 2^27: at least 15
    if (blocks < k) k = blocks;
    plan->chunk = (int)k;
    plan->stage_bytes = k * pixels * per_pixel;
    return true;
}

}  // namespace hz
