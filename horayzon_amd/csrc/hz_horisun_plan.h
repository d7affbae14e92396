// hz_horisun_plan.h -- launch plan of hz_horizon_terrain_run (hz_horisun.hip): plain C++, no HIP, so that the chunk
// arithmetic can be compiled into a stand-alone host program and run under a sanitizer (scripts/horisun_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace hz {

// Sun positions per launch of k_horisun.  A lane walks its positions in the inner loop, so a launch lasts as long as
// its chunk: 48 positions of the 3601^2 tile are ~0.6 G (cell, position) pairs.  Consecutive positions of a day stay
// in the same or the next 128-byte line of a lane's horizon row; a chunk boundary costs each lane one line again.
#define HZ_HORISUN_CHUNK 48
#define HZ_HORISUN_TPB 256

struct HorisunPlan {
    size_t cells = 0;        // dim_in_0 * dim_in_1
    int chunk = 0;           // positions per launch
    int num_chunks = 0;
    unsigned blocks = 0;     // grid.x: one lane per cell
};

// 0: ok; 1: a dimension, the position count or a product is out of range (nothing is launched then).  `knob` > 0 replaces
// the default chunk (hz_debug_set("horisun_chunk", n): tests).  num_outputs = per-position maps wanted (bytes per cell
// and position, 0 ... 5): their size must fit a size_t.
inline int horisun_plan(int dim_in_0, int dim_in_1, int azim_num, int num_sun, int knob, int bytes_per_pair, HorisunPlan *p) {
    if (dim_in_0 <= 0 || dim_in_1 <= 0 || azim_num <= 0 || num_sun <= 0 || bytes_per_pair < 0) return 1;
    const uint64_t cells = (uint64_t)dim_in_0 * (uint64_t)dim_in_1;             // < 2^62
    if (cells > (uint64_t)SIZE_MAX / ((uint64_t)azim_num * sizeof(float))) return 1;   // bytes of hori
    if (bytes_per_pair > 0 && cells > (uint64_t)SIZE_MAX / ((uint64_t)num_sun * (uint64_t)bytes_per_pair)) return 1;
    const uint64_t blocks = (cells + HZ_HORISUN_TPB - 1) / HZ_HORISUN_TPB;
    if (blocks > 0x7fffffffull) return 1;                                      // grid.x
    p->cells = (size_t)cells;
    p->chunk = knob > 0 ? knob : HZ_HORISUN_CHUNK;
    if (p->chunk > num_sun) p->chunk = num_sun;
    p->num_chunks = (num_sun - 1) / p->chunk + 1;
    p->blocks = (unsigned)blocks;
    return 0;
}

// chunk c of the plan: positions [*s0, *s0 + *count)
inline void horisun_chunk(const HorisunPlan &p, int num_sun, int c, int *s0, int *count) {
    *s0 = (int)((int64_t)c * p.chunk);
    const int left = num_sun - *s0;
    *count = left < p.chunk ? left : p.chunk;
}

}  // namespace hz
