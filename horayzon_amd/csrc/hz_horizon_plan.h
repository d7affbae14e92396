// hz_horizon_plan.h -- sizes of a gridded horizon call (horizon_run, hz_api_horizon.hip): rows per launch, the regions of the
// leftover records, the certificate scratch.  Plain C++, no HIP, so that the arithmetic can be compiled into a stand-alone
// host program and run under a sanitizer (scripts/horizon_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace hz {

#define HZ_LEFT_LEVELS 4                 // leftover regions (hand-over levels)
#define HZ_LEFT_WORDS 16                 // 32-bit words per leftover record
// default hand-over thresholds: byte l = level l (hz_opts.left_min)
#define HZ_LEFT_DEFAULT 0x00000024u

// Rows per launch when the horizon of a chunk of rows lives in a bounded device buffer of about `target` bytes.
// fixed_rows > 0 (hz_opts.chunk_rows): that many.  Otherwise equal chunks (whole 16-row tile rows) instead of full ones and a
// small rest: a slab of 1800 rows is 3 x 608 rows, not 830 + 830 + 140 -- every launch ends with a tail, and a short launch is
// mostly tail.  Never fewer than 16 rows (one tile row), whatever the target; never more than rows_all.
inline int horizon_chunk_rows(int rows_all, size_t row_bytes, size_t target, int fixed_rows) {
    int chunk_rows = rows_all;
    if (fixed_rows > 0) chunk_rows = std::min(chunk_rows, fixed_rows);
    else {
        chunk_rows = (int)std::max<size_t>(16, std::min<size_t>((size_t)chunk_rows, target / row_bytes));
        const int n_ch = (rows_all + chunk_rows - 1) / chunk_rows;
        chunk_rows = std::min(chunk_rows, std::max(16, ((rows_all + n_ch - 1) / n_ch + 15) / 16 * 16));
    }
    return std::min(chunk_rows, rows_all);
}

// Bytes of the near-field certificates of `cells` cells (hz_near.hip): near_idx u16[cells][azim_num], rounded up to 256 B,
// then near_r f32[cells]
inline size_t near_idx_bytes(size_t cells, int azim_num) { return (cells * (size_t)azim_num * 2 + 255) & ~(size_t)255; }
inline size_t near_scratch_bytes(size_t cells, int azim_num) { return near_idx_bytes(cells, azim_num) + cells * 4; }

// hz_opts.left_min -> hand-over thresholds per level (0: HZ_LEFT_DEFAULT, < 0: off; a byte is at most 56; a level that does
// not hand over is the last one).  Returns the number of follow-up launches.
inline int left_thresholds(int pack, int left_t[HZ_LEFT_LEVELS]) {
    int n = 0;
    for (int l = 0; l < HZ_LEFT_LEVELS; l++) left_t[l] = 0;
    const unsigned upack = pack == 0 ? HZ_LEFT_DEFAULT : (pack < 0 ? 0u : (unsigned)pack);
    for (int l = 0; l < HZ_LEFT_LEVELS; l++) {
        left_t[l] = (int)std::min((upack >> (8 * l)) & 0xffu, 56u);
        if (left_t[l] == 0) break;
        n = l + 1;
    }
    return n;
}

// The leftover buffer of a launch: one 64 B record per hand-over, region l sized from what the level above can hand over at
// most (level 0: per_xcd tiles x 8 XCDs x 4 blocks of 8 x 8 cells, left_t[0] records each; then groups of 64 records), every
// capacity a multiple of 64 records; behind the records the sort scratch (4 arrays of cap_max words, the sort's temporary
// words, 64 spare).  left_cap_test > 0 (tests) caps every region.
struct LeftPlan {
    bool on = false;                     // false: no hand-over (record numbers are 32 bit)
    unsigned left_base[HZ_LEFT_LEVELS] = {0, 0, 0, 0}, left_cap[HZ_LEFT_LEVELS] = {0, 0, 0, 0};
    unsigned cap_max = 0;
    size_t rec_bytes = 0, total_bytes = 0;      // the sort scratch starts at rec_bytes
};
inline LeftPlan left_plan(const int left_t[HZ_LEFT_LEVELS], int n_levels, int per_xcd, int left_cap_test,
                          size_t (*sort_temp_elems)(size_t)) {
    LeftPlan p;
    unsigned long long units = (unsigned long long)per_xcd * 8ull * 4ull;
    unsigned long long total = 0, cap_max = 0;
    for (int l = 0; l < n_levels; l++) {
        unsigned long long cap = ((units * (unsigned long long)left_t[l] + 63ull) & ~63ull) + 64ull;
        if (left_cap_test > 0) cap = std::min<unsigned long long>(cap, ((unsigned long long)left_cap_test + 63ull) & ~63ull);
        p.left_base[l] = (unsigned)total; p.left_cap[l] = (unsigned)cap;
        total += cap; cap_max = std::max(cap_max, cap);
        units = cap / 64ull;
    }
    if (n_levels <= 0 || total >= (1ull << 31)) return p;
    p.on = true;
    p.cap_max = (unsigned)cap_max;
    p.rec_bytes = (size_t)total * HZ_LEFT_WORDS * sizeof(unsigned);
    p.total_bytes = p.rec_bytes + (4 * (size_t)cap_max + sort_temp_elems((size_t)cap_max) + 64) * sizeof(uint32_t);
    return p;
}

}  // namespace hz
