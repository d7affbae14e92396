// Stand-alone host program over the launch plan of k_horisun_coarse (horayzon_amd/csrc/hz_horisun_coarse_plan.h: plain C++, no
// HIP).  For every shape the tests use, a sweep of dims, blocks, tiles and chunks, and the 3569^2 tile, it walks the plan the
// way the kernel does -- workgroup (coarse row, strip, position group), tiles, passes, the writing threads and the adding
// lanes -- and checks that every cell of every block is added once and in row-major order, that every LDS index stays inside
// the allocation and the allocation inside the cap, that the positions of a chunk are each taken by one workgroup, and that
// the grid fits a launch.  Meant to be built with a sanitizer and run on the host:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/horisun_coarse_plan_check.cpp -o /tmp/horisun_coarse_plan_check && /tmp/horisun_coarse_plan_check
#include "../horayzon_amd/csrc/hz_horisun_coarse_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
static long plans = 0, fallbacks = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 50) std::printf("FAILED %s (line %d)\n", #c, __LINE__); fails++; } } while (0)

static const size_t LDS_CAP = 65536;

// rows_limit > 0: only that many coarse rows at each end of the domain are walked (the big tile)
static void walk(int d0, int d1, int p0, int p1, int chunk, int knob, bool codes, bool vals, int expect_fallback, int rows_limit = 0) {
    hz::HorisunCoarsePlan p;
    if (hz::horisun_coarse_plan(d0, d1, p0, p1, chunk, knob, codes, vals, &p)) {
        std::printf("refused %d x %d P %d x %d chunk %d\n", d0, d1, p0, p1, chunk); fails++; return;
    }
    plans++;
    const int cap = knob > 0 && knob < HZ_HSC_TILE ? knob : HZ_HSC_TILE;
    CHECK(p.fallback == (p1 > cap ? 1 : 0));
    if (expect_fallback >= 0) CHECK(p.fallback == expect_fallback);
    if (p.fallback) { fallbacks++; return; }
    CHECK(p.gy == d0 / p0 && p.gx == d1 / p1);
    CHECK(p.nb >= 1 && p.nb <= HZ_HSC_TPB && p.nstrips >= 1);
    CHECK((long long)p.nb * p.nstrips >= p.gx && (long long)p.nb * (p.nstrips - 1) < p.gx);
    CHECK(p.rows >= 1 && p.rows <= p0 && p.ntiles == (p0 + p.rows - 1) / p.rows);
    CHECK(p.pitch == p.rows * p.nb * p1 && p.pitch <= cap);
    CHECK(p1 > HZ_HSC_PREF_CELLS || p.pitch <= HZ_HSC_PREF_CELLS);
    CHECK(p.q >= 1 && p.q <= HZ_HSC_QMAX && p.q * p.nb <= HZ_HSC_TPB && p.q <= chunk);
    CHECK((unsigned long long)p.grid_x == (unsigned long long)p.gy * p.nstrips && p.grid_x <= 0x7fffffffu);
    CHECK(hz::horisun_coarse_groups(p, chunk) >= 1 && hz::horisun_coarse_groups(p, chunk) <= 65535u);
    // LDS layout: the values at 0, then the flags
    const size_t maps = (size_t)p.q * p.pitch;
    CHECK(p.off_flags == (vals ? maps * 4 : 0));
    CHECK(p.lds_bytes == p.off_flags + (codes ? maps : 0) && p.lds_bytes <= LDS_CAP);
    CHECK(maps * ((vals ? 4 : 0) + (codes ? 1 : 0)) <= HZ_HSC_LDS_MAPS);
    // positions: the groups of a chunk of k positions tile [0, k) in passes of at most q
    for (int k : {chunk, 1, (chunk + 1) / 2}) {
        const int groups = (int)hz::horisun_coarse_groups(p, k);
        int next = 0;
        for (int g = 0; g < groups; g++) {
            const int s_begin = g * p.q, s_end = std::min(k, s_begin + p.q);
            CHECK(s_begin == next && s_begin < s_end);
            next = s_end;
        }
        CHECK(next == k);
    }
    // cells: per workgroup (I, strip), the writers fill every LDS cell of the tile once; the adding lanes take every cell of
    // their block once, in row-major order, from the LDS cell its writer filled
    std::vector<long long> owner((size_t)p.pitch);                  // domain cell held by an LDS cell of the tile
    const int Wm = p.nb * p1;
    for (int I = 0; I < p.gy; I++) {
        if (rows_limit > 0 && I >= rows_limit && I < p.gy - rows_limit) continue;
        for (int strip = 0; strip < p.nstrips; strip++) {
            const int J0 = strip * p.nb, nbc = std::min(p.nb, p.gx - J0);
            CHECK(nbc >= 1);
            const int W = nbc * p1;
            std::vector<long long> last_cell((size_t)nbc, -1), count((size_t)nbc, 0);
            for (int r0 = 0; r0 < p0; r0 += p.rows) {
                const int rc = std::min(p.rows, p0 - r0), cells_t = rc * W;
                std::fill(owner.begin(), owner.end(), -1);
                const long long cell00 = (long long)(I * p0 + r0) * d1 + (long long)J0 * p1;
                // the pairs x = q * cells_t + e of a full pass, thread t takes x = t, t + TPB, ...: here q = 0 and q = p.q - 1
                for (int qq = 0; qq < p.q; qq += (p.q > 1 ? p.q - 1 : 1))
                    for (int e = 0; e < cells_t; e++) {
                        const long long x = (long long)qq * cells_t + e;
                        const int q2 = (int)(x / cells_t), e2 = (int)(x - (long long)q2 * cells_t);
                        CHECK(q2 == qq && e2 == e);
                        const int r = e / W, c = e - r * W, at = r * Wm + c;
                        CHECK(at >= 0 && at < p.pitch && (size_t)qq * p.pitch + at < maps);
                        if (at < 0 || at >= p.pitch) continue;
                        if (qq == 0) CHECK(owner[(size_t)at] == -1);
                        const long long cell = cell00 + (long long)r * d1 + c;
                        CHECK(cell >= 0 && cell < (long long)d0 * d1);
                        if (qq == 0) owner[(size_t)at] = cell; else CHECK(owner[(size_t)at] == cell);
                    }
                for (int ab = 0; ab < nbc; ab++)
                    for (int r = 0; r < rc; r++)
                        for (int dj = 0; dj < p1; dj++) {
                            const int at = r * Wm + ab * p1 + dj;
                            CHECK(at < p.pitch && (size_t)(p.q - 1) * p.pitch + at < maps);
                            const long long want = (long long)(I * p0 + r0 + r) * d1 + (long long)(J0 + ab) * p1 + dj;
                            CHECK(owner[(size_t)at] == want);
                            CHECK(want > last_cell[(size_t)ab]);
                            last_cell[(size_t)ab] = want;
                            count[(size_t)ab]++;
                        }
            }
            for (int ab = 0; ab < nbc; ab++) {
                CHECK(count[(size_t)ab] == (long long)p0 * p1);
                CHECK(last_cell[(size_t)ab] == (long long)((I + 1) * p0 - 1) * d1 + (long long)(J0 + ab + 1) * p1 - 1);
            }
        }
    }
}

static void walk_outputs(int d0, int d1, int p0, int p1, int chunk, int knob, int expect_fallback = -1, int rows_limit = 0) {
    walk(d0, d1, p0, p1, chunk, knob, true, true, expect_fallback, rows_limit);
    walk(d0, d1, p0, p1, chunk, knob, true, false, expect_fallback, rows_limit);
    walk(d0, d1, p0, p1, chunk, knob, false, true, expect_fallback, rows_limit);
}

int main() {
    const int knobs[] = {0, -1, 4096, 5000, 1024, 513, 512, 256, 64, 7, 1};
    const int chunks[] = {1, 2, 3, 7, 8, 9, 48, 144, 4096};
    // the shapes of the tests
    const int p_4860[][2] = {{4, 4}, {6, 20}, {48, 1}, {1, 60}, {48, 60}, {1, 1}, {3, 5}};
    const int p_812[][2] = {{2, 3}, {8, 12}, {1, 1}, {4, 1}};
    for (int k : knobs) for (int c : chunks) {
        for (auto &P : p_4860) walk_outputs(48, 60, P[0], P[1], c, k);
        for (auto &P : p_812) walk_outputs(8, 12, P[0], P[1], c, k);
        walk_outputs(1, 1, 1, 1, c, k);
        walk_outputs(1, 130, 1, 13, c, k);
        walk_outputs(1, 130, 1, 130, c, k);
    }
    // a sweep: every divisor pair of a few domains
    const int dims[][2] = {{37, 53}, {90, 90}, {12, 600}, {300, 12}, {7, 1024}, {2, 4098}, {1, 8194}};
    for (auto &d : dims)
        for (int p0 = 1; p0 <= d[0]; p0++) if (d[0] % p0 == 0)
            for (int p1 = 1; p1 <= d[1]; p1++) if (d[1] % p1 == 0)
                for (int k : {0, 64}) for (int c : {5, 48}) walk_outputs(d[0], d[1], p0, p1, c, k);
    // the blocks of the widest fused shape and the first that falls back
    walk_outputs(3, 8192, 3, 4096, 48, 0, 0);
    walk_outputs(3, 8194, 3, 4097, 48, 0, 1);
    walk_outputs(3, 8192, 1, 4096, 48, 4095, 1);
    // the 3601^2 tile's inner domain with 43 x 43 blocks (the coarse rows at both ends), and a domain at the dimension limit
    walk_outputs(3569, 3569, 43, 43, 48, 0, 0, 2);
    walk_outputs(3569, 3569, 1, 1, 48, 0, 0, 2);
    walk_outputs(3569, 3569, 43, 3569, 48, 0, 0, 1);
    walk_outputs(32767, 32767, 1, 1, 4096, 0, 0, 1);
    // refusals
    hz::HorisunCoarsePlan p;
    CHECK(hz::horisun_coarse_plan(0, 5, 1, 1, 1, 0, true, true, &p) == 1);
    CHECK(hz::horisun_coarse_plan(6, 8, 4, 2, 1, 0, true, true, &p) == 1);
    CHECK(hz::horisun_coarse_plan(6, 8, 0, 2, 1, 0, true, true, &p) == 1);
    CHECK(hz::horisun_coarse_plan(6, 8, 2, 16, 1, 0, true, true, &p) == 1);
    CHECK(hz::horisun_coarse_plan(6, 8, 2, 2, 0, 0, true, true, &p) == 1);
    CHECK(hz::horisun_coarse_plan(6, 8, 2, 2, HZ_HSC_CHUNK_MAX + 1, 0, true, true, &p) == 1);
    CHECK(hz::horisun_coarse_plan(6, 8, 2, 2, 1, 0, false, false, &p) == 1);
    CHECK(hz::horisun_coarse_plan(2147483647, 2147483647, 1, 1, 1, 0, true, true, &p) == 1);      // grid.x
    std::printf("%ld plans walked, %ld of them two-pass\n", plans, fallbacks);
    std::printf(fails ? "%d checks failed\n" : "horisun coarse plan: all checks passed\n", fails);
    return fails ? 1 : 0;
}
