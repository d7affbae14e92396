// Host program for horayzon_amd/csrc/hz_panorama_plan.h (tests/test_panorama_plan_host.py builds it with ASan + UBSan and runs
// it on the CPU): the header compiles without a device compiler, and the observers per launch of Terrain.panorama follow
// DESIGN.md section 4 clause 20 / section 5 at the edges -- a budget below one observer's images, one observer, more observers
// than a launch takes, the largest image, and the cap that keeps (observer, tile) below 2^31.  The formula is restated
// here in 128-bit integers, so an overflow in the header's 64-bit arithmetic shows as a difference (or as a UBSan finding).
#include <cstdio>
#include <initializer_list>

#include "../horayzon_amd/csrc/hz_panorama_plan.h"

using namespace hz;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { if (failures++ < 20) std::printf("line %d: %s failed\n", __LINE__, #c); } } while (0)

typedef unsigned __int128 u128;

// the clause as it reads
static int clause(int S, int A, int E, bool sd, bool sp, unsigned long long budget) {
    const u128 pixels = (u128)A * (u128)E;
    const u128 per = (u128)(sd ? 4 : 0) + (u128)(sp ? 12 : 0);
    u128 k = S < 32768 ? S : 32768;
    if (per != 0) {
        u128 fit = (u128)budget / (pixels * per);
        if (fit < 1) fit = 1;
        if (fit < k) k = fit;
    }
    const u128 tiles = (u128)((A + 7) / 8) * (u128)((E + 7) / 8);
    const u128 room = (((u128)1 << 31) - 1) / tiles;          // the largest k with tiles * k < 2^31
    if (room < k) k = room;
    return (int)k;
}

static void check(int S, int A, int E, bool sd, bool sp, unsigned long long budget) {
    PanoramaPlan p;
    const bool ok = panorama_plan(S, A, E, sd, sp, budget, &p);
    EXPECT(ok);
    if (!ok) return;
    const int want = clause(S, A, E, sd, sp, budget);
    if (p.chunk != want) std::printf("S %d A %d E %d stage %d %d budget %llu: chunk %d, clause %d\n", S, A, E, (int)sd, (int)sp, budget, p.chunk, want);
    EXPECT(p.chunk == want);
    EXPECT(p.chunk >= 1 && p.chunk <= S && p.chunk <= HZ_PANORAMA_MAX_OBS);
    EXPECT(p.pixels == (unsigned long long)A * (unsigned long long)E);
    EXPECT(p.tiles_a == (A + 7) / 8 && p.tiles_e == (E + 7) / 8);
    EXPECT(p.tiles == (unsigned long long)p.tiles_a * (unsigned long long)p.tiles_e);
    EXPECT(p.tiles * (unsigned long long)p.chunk < HZ_PANORAMA_MAX_BLOCKS);
    const unsigned long long per = (sd ? 4ull : 0ull) + (sp ? 12ull : 0ull);
    EXPECT(p.stage_bytes == (unsigned long long)p.chunk * p.pixels * per);
    // the staging is within the budget unless one observer alone exceeds it
    if (per) EXPECT(p.stage_bytes <= budget || p.chunk == 1);
}

int main() {
    PanoramaPlan p;
    // refused
    EXPECT(!panorama_plan(0, 8, 8, true, true, HZ_PANORAMA_BUDGET, &p));
    EXPECT(!panorama_plan(-1, 8, 8, true, true, HZ_PANORAMA_BUDGET, &p));
    EXPECT(!panorama_plan(1, 0, 8, true, true, HZ_PANORAMA_BUDGET, &p));
    EXPECT(!panorama_plan(1, 8, 0, true, true, HZ_PANORAMA_BUDGET, &p));
    EXPECT(!panorama_plan(1, 8, -3, true, true, HZ_PANORAMA_BUDGET, &p));
    EXPECT(!panorama_plan(1, 8, 8, true, true, 0, &p));
    EXPECT(!panorama_plan(1, (1 << 30) + 1, 1, true, true, HZ_PANORAMA_BUDGET, &p));
    EXPECT(!panorama_plan(1, 1 << 15, (1 << 15) + 1, false, false, HZ_PANORAMA_BUDGET, &p));
    EXPECT(!panorama_plan(1, 2147483647, 2147483647, true, true, HZ_PANORAMA_BUDGET, &p));

    // a budget smaller than one observer: chunks of one
    EXPECT(panorama_plan(6, 45, 21, true, true, 1, &p) && p.chunk == 1);
    EXPECT(panorama_plan(6, 45, 21, true, false, 45 * 21 * 4 - 1, &p) && p.chunk == 1);
    EXPECT(panorama_plan(6, 45, 21, true, false, 45 * 21 * 4, &p) && p.chunk == 1);
    EXPECT(panorama_plan(6, 45, 21, true, false, 2 * 45 * 21 * 4 - 1, &p) && p.chunk == 1);
    EXPECT(panorama_plan(6, 45, 21, true, false, 2 * 45 * 21 * 4, &p) && p.chunk == 2);
    EXPECT(panorama_plan(6, 45, 21, true, true, 2 * 45 * 21 * 16, &p) && p.chunk == 2 && p.stage_bytes == 2ull * 45 * 21 * 16);
    EXPECT(panorama_plan(6, 45, 21, false, true, 5 * 45 * 21 * 12, &p) && p.chunk == 5);
    EXPECT(panorama_plan(6, 45, 21, false, true, 1000 * 45 * 21 * 12, &p) && p.chunk == 6);
    // S = 1
    EXPECT(panorama_plan(1, 3600, 900, true, true, HZ_PANORAMA_BUDGET, &p) && p.chunk == 1 && p.stage_bytes == 3600ull * 900 * 16);
    EXPECT(panorama_plan(1, 1, 1, false, false, HZ_PANORAMA_BUDGET, &p) && p.chunk == 1 && p.stage_bytes == 0 && p.tiles == 1);
    // S > 32768: nothing staged takes the launch's limit, staged images the budget's
    EXPECT(panorama_plan(100000, 13, 5, false, false, HZ_PANORAMA_BUDGET, &p) && p.chunk == 32768 && p.stage_bytes == 0);
    EXPECT(panorama_plan(100000, 13, 5, true, true, HZ_PANORAMA_BUDGET, &p) && p.chunk == 32768);
    EXPECT(panorama_plan(2147483647, 1, 1, true, true, HZ_PANORAMA_BUDGET, &p) && p.chunk == 32768);
    EXPECT(panorama_plan(100000, 3600, 900, true, false, HZ_PANORAMA_BUDGET, &p) && p.chunk == 20);       // 268435456 / 12960000
    // E * A = 2^30 in its three extreme shapes: 2^27, 2^27 and 2^24 tiles
    EXPECT(panorama_plan(40, 1 << 30, 1, false, false, HZ_PANORAMA_BUDGET, &p) && p.tiles == (1ull << 27) && p.chunk == 15);
    EXPECT(panorama_plan(40, 1, 1 << 30, false, false, HZ_PANORAMA_BUDGET, &p) && p.tiles == (1ull << 27) && p.chunk == 15);
    EXPECT(panorama_plan(1000, 1 << 15, 1 << 15, false, false, HZ_PANORAMA_BUDGET, &p) && p.tiles == (1ull << 24) && p.chunk == 127);
    EXPECT(panorama_plan(40, 1 << 30, 1, true, true, HZ_PANORAMA_BUDGET, &p) && p.chunk == 1 && p.stage_bytes == (16ull << 30));
    // the 2^31 cap: 2^16 tiles per observer leave room for 32767 observers, not 32768
    EXPECT(panorama_plan(40000, 1 << 12, 1 << 10, false, false, HZ_PANORAMA_BUDGET, &p) && p.tiles == (1ull << 16) && p.chunk == 32767);
    EXPECT(panorama_plan(40000, (1 << 12) - 8, 1 << 10, false, false, HZ_PANORAMA_BUDGET, &p) && p.chunk == 32768);
    EXPECT(panorama_plan(40000, (1 << 12) + 1, 1 << 10, false, false, HZ_PANORAMA_BUDGET, &p) && p.tiles == 513ull * 128 && p.chunk == 32704);

    // sweep against the clause
    const int sizes[] = {1, 2, 7, 8, 9, 13, 45, 64, 65, 900, 3600, 4095, 4096, 4097, 32767, 32768, 1 << 20, 1 << 27, 1 << 30};
    const unsigned long long budgets[] = {1, 4, 16, 1000, 45 * 21 * 4, 1 << 20, HZ_PANORAMA_BUDGET, 1ull << 31, 1ull << 40, ~0ull};
    long cases = 0;
    for (int S : {1, 2, 6, 100, 32767, 32768, 32769, 100000, 2147483647})
        for (int A : sizes)
            for (int E : sizes) {
                if ((unsigned long long)A * (unsigned long long)E > HZ_PANORAMA_MAX_PIXELS) continue;
                for (unsigned long long b : budgets)
                    for (int st = 0; st < 4; st++) { check(S, A, E, st & 1, st & 2, b); cases++; }
            }
    std::printf("%ld cases\n", cases);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("panorama plan ok\n");
    return 0;
}
