// Stand-alone host program over the launch plan of hz_horizon_terrain_run (horayzon_amd/csrc/hz_horisun_plan.h: plain C++, no
// HIP): walks the chunks of every shape the tests use and of the extremes, and checks that they tile [0, num_sun) in ascending
// order and that every refused plan is one whose sizes do not fit.  Meant to be built with a sanitizer and run on the host:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/horisun_plan_check.cpp -o /tmp/horisun_plan_check && /tmp/horisun_plan_check
#include "../horayzon_amd/csrc/hz_horisun_plan.h"
#include <cstdio>
#include <cstdlib>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); fails++; } } while (0)

static void walk(int d0, int d1, int azim, int num_sun, int knob, int bytes) {
    hz::HorisunPlan p;
    if (hz::horisun_plan(d0, d1, azim, num_sun, knob, bytes, &p)) { std::printf("refused %d x %d A %d S %d\n", d0, d1, azim, num_sun); fails++; return; }
    CHECK(p.cells == (size_t)d0 * (size_t)d1);
    CHECK(p.chunk >= 1 && p.chunk <= num_sun && (knob <= 0 || p.chunk == (knob < num_sun ? knob : num_sun)));
    CHECK((unsigned long long)p.blocks * HZ_HORISUN_TPB >= p.cells && ((unsigned long long)p.blocks - 1) * HZ_HORISUN_TPB < p.cells);
    int next = 0;
    for (int c = 0; c < p.num_chunks; c++) {
        int s0 = -1, kc = -1;
        hz::horisun_chunk(p, num_sun, c, &s0, &kc);
        CHECK(s0 == next && kc >= 1 && kc <= p.chunk);
        next = s0 + kc;
    }
    CHECK(next == num_sun);
}

int main() {
    const int dims[][2] = {{37, 53}, {1, 1}, {1, 130}, {34, 34}, {3569, 3569}, {32767, 32767}};
    const int azims[] = {1, 2, 7, 16, 360};
    const int suns[] = {1, 5, 12, 47, 48, 49, 50, 144, 400, 32768, 40000, 2147483647};
    const int knobs[] = {0, -1, 1, 2, 3, 4, 5, 7, 2147483647};
    for (auto &d : dims) for (int a : azims) for (int s : suns) for (int k : knobs) {
        walk(d[0], d[1], a, s, k, 0);
        if ((double)d[0] * d[1] * (double)s * 5.0 < 1.0e18) walk(d[0], d[1], a, s, k, 5);
    }
    hz::HorisunPlan p;
    CHECK(hz::horisun_plan(0, 5, 1, 1, 0, 0, &p) == 1);
    CHECK(hz::horisun_plan(5, -1, 1, 1, 0, 0, &p) == 1);
    CHECK(hz::horisun_plan(5, 5, 0, 1, 0, 0, &p) == 1);
    CHECK(hz::horisun_plan(5, 5, 1, 0, 0, 0, &p) == 1);
    CHECK(hz::horisun_plan(2147483647, 2147483647, 2147483647, 1, 0, 0, &p) == 1);       // bytes of hori
    CHECK(hz::horisun_plan(2147483647, 2147483647, 1, 2147483647, 0, 5, &p) == 1);       // bytes of the per-position maps
    CHECK(hz::horisun_plan(2147483647, 2147483647, 1, 1, 0, 0, &p) == 1);                // grid.x
    std::printf(fails ? "%d checks failed\n" : "horisun plan: all checks passed\n", fails);
    return fails ? 1 : 0;
}
