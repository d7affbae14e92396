// Stand-alone host program over the sizes of a gridded horizon call (horayzon_amd/csrc/hz_horizon_plan.h: plain C++, no HIP):
// walks the rows-per-launch rule and the regions of the leftover records over small and large shapes and checks that the
// chunks tile the rows in order, that a chunk stays inside its byte target, that the regions do not overlap and that a plan
// that is on fits the 32-bit record numbers.  Meant to be built with a sanitizer and run on the host:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/horizon_plan_check.cpp -o /tmp/horizon_plan_check && /tmp/horizon_plan_check
#include "../horayzon_amd/csrc/hz_horizon_plan.h"
#include <cstdio>
#include <cstdlib>

static long fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED %s (line %d)\n", #c, __LINE__); fails++; } } while (0)

// hz_sort.hip: sort_temp_elems / scan_temp_elems (tiles of 1024 keys, scan tiles of 2048 words)
static size_t scan_temp(size_t n) {
    size_t total = 0;
    while (n > 2048) { n = (n + 2047) / 2048; total += n; }
    return total + 1;
}
static size_t sort_temp(size_t n) {
    const size_t tiles = (n + 1023) / 1024;
    return 2 * 256 * tiles + scan_temp(256 * tiles);
}

static void walk_rows(int rows, size_t row_bytes, size_t target, int fixed) {
    const int cr = hz::horizon_chunk_rows(rows, row_bytes, target, fixed);
    CHECK(cr >= 1 && cr <= rows);
    if (fixed > 0) CHECK(cr == (fixed < rows ? fixed : rows));
    else CHECK((size_t)cr * row_bytes <= target || cr <= 16);             // (the floor of one tile row)
    int next = 0, n = 0;
    for (int rb = 0; rb < rows; rb += cr, n++) {                          // horizon_run's loop
        const int re = rb + cr < rows ? rb + cr : rows;
        CHECK(rb == next && re > rb);
        CHECK(re - rb == cr || re == rows);                               // every chunk but the last is full
        next = re;
    }
    CHECK(next == rows && n == (rows + cr - 1) / cr);
}

static void walk_left(int pack, int per_xcd, int cap_test) {
    int t[HZ_LEFT_LEVELS];
    const int n = hz::left_thresholds(pack, t);
    CHECK(n >= 0 && n <= HZ_LEFT_LEVELS);
    for (int l = 0; l < HZ_LEFT_LEVELS; l++) CHECK(l < n ? (t[l] >= 1 && t[l] <= 56) : t[l] == 0);
    if (pack == 0) CHECK(n == 1 && t[0] == 36);
    if (pack < 0) CHECK(n == 0);
    const hz::LeftPlan p = hz::left_plan(t, n, per_xcd, cap_test, sort_temp);
    if (n == 0) { CHECK(!p.on); return; }
    if (!p.on) return;                                                   // off: nothing reads the regions
    unsigned long long end = 0, cap_max = 0;
    for (int l = 0; l < n; l++) {
        CHECK(p.left_base[l] == (unsigned)end);                          // regions follow each other: no overlap, no gap
        CHECK(p.left_cap[l] >= 64 && p.left_cap[l] % 64 == 0);
        if (cap_test > 0) CHECK(p.left_cap[l] <= (((unsigned)cap_test + 63u) & ~63u));
        else {                                                           // room for everything the level above can hand over
            const unsigned long long units = l == 0 ? (unsigned long long)per_xcd * 32ull : p.left_cap[l - 1] / 64ull;
            CHECK((unsigned long long)p.left_cap[l] >= units * (unsigned long long)t[l]);
        }
        end += p.left_cap[l];
        cap_max = cap_max > p.left_cap[l] ? cap_max : p.left_cap[l];
    }
    CHECK(end < (1ull << 31));
    CHECK(p.cap_max == cap_max);
    CHECK(p.rec_bytes == (size_t)end * HZ_LEFT_WORDS * 4);               // left_sort starts at rec_bytes
    CHECK(p.total_bytes == p.rec_bytes + (4 * (size_t)cap_max + sort_temp((size_t)cap_max) + 64) * 4);
}

int main() {
    // rows per launch
    const int azims[] = {1, 24, 360};
    const int big_rows[] = {3601, 14401};
    for (int azim : azims)
        for (int gib = 1; gib <= 16; gib *= 2)
            for (int fixed = 0; fixed <= (gib == 1 ? 40 : 0); fixed++) {      // (a fixed count ignores the target)
                const size_t target = (size_t)gib << 30;
                for (int w = 1; w <= 70; w++) {
                    const size_t row_bytes = (size_t)w * (size_t)azim * 4;
                    for (int rows = 1; rows <= 400; rows++) walk_rows(rows, row_bytes, target, fixed);
                }
                for (int rows : big_rows) {                               // the 3601^2 tile and the 14401^2 mosaic, full rows
                    walk_rows(rows, (size_t)rows * (size_t)azim * 4, target, fixed);
                    walk_rows(rows, (size_t)70 * (size_t)azim * 4, target, fixed);
                }
            }
    CHECK(hz::horizon_chunk_rows(1800, (size_t)3601 * 360 * 4, (size_t)4 << 30, 0) == 608);       // 3 x 608, not 830 + 830 + 140
    // a row that alone exceeds the target: the floor of 16 rows holds
    CHECK(hz::horizon_chunk_rows(100, (size_t)1 << 30, (size_t)1 << 30, 0) == 16);
    // the certificate scratch
    CHECK(hz::near_idx_bytes(1, 1) == 256 && hz::near_scratch_bytes(1, 1) == 260);
    CHECK(hz::near_scratch_bytes(43 * 63, 24) == ((43 * 63 * 24 * 2 + 255) / 256) * 256 + 43 * 63 * 4);
    CHECK(hz::near_idx_bytes(128, 1) == 256 && hz::near_idx_bytes(129, 1) == 512);
    // leftover regions: every threshold byte one level takes, several levels, test caps, small and large tile maps
    const int per_xcds[] = {1, 3, 12, 28 * 224, 112 * 900, 1 << 22, 1 << 26};
    const int caps[] = {0, 1, 64, 65, 4096};
    for (int per_xcd : per_xcds)
        for (int cap : caps) {
            for (int b = -1; b <= 255; b++) walk_left(b, per_xcd, cap);                                      // one level
            for (int b0 = 1; b0 <= 255; b0 += 7)
                for (int b1 = 0; b1 <= 255; b1 += 5) {
                    walk_left(b0 | (b1 << 8), per_xcd, cap);                                                 // two
                    walk_left(b0 | (b1 << 8) | (0x18 << 16), per_xcd, cap);                                  // three
                    walk_left(b0 | (b1 << 8) | (0x38 << 16) | (0x7f << 24), per_xcd, cap);                   // four
                }
            walk_left(0x1818, per_xcd, cap);
            walk_left((int)0x80000000u, per_xcd, cap);                                                       // negative: off
        }
    {   // a launch too large for 32-bit record numbers runs without the hand-over
        int t[HZ_LEFT_LEVELS];
        const int n = hz::left_thresholds(56, t);
        CHECK(n == 1 && !hz::left_plan(t, n, 1 << 26, 0, sort_temp).on && hz::left_plan(t, n, 1 << 20, 0, sort_temp).on);
    }
    std::printf(fails ? "%ld checks failed\n" : "horizon plan: all checks passed\n", fails);
    return fails ? 1 : 0;
}
