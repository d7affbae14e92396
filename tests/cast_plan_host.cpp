// Host program for horayzon_amd/csrc/hz_cast_plan.h (tests/test_cast_plan_host.py builds it with ASan + UBSan and runs it on
// the CPU): the header compiles without a device compiler, and the rays per chunk of Terrain.cast follow DESIGN.md section 4
// clause 21 / section 5 at the edges -- one ray, one wave, one ray more, the largest call, every combination of staged
// arrays with and without the sort, budgets down to one wave and below.  The formula is restated here in 128-bit integers,
// so an overflow in the header's 64-bit arithmetic shows as a difference (or as a UBSan finding).
#include <cstdio>
#include <initializer_list>

#include "../horayzon_amd/csrc/hz_cast_plan.h"

using namespace hz;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { if (failures++ < 20) std::printf("line %d: %s failed\n", __LINE__, #c); } } while (0)

typedef unsigned __int128 u128;

static unsigned long long bytes_per_ray(int stage, bool sorted) {
    return ((stage & 1) ? 12ull : 0ull) + ((stage & 2) ? 12ull : 0ull) + ((stage & 4) ? 1ull : 0ull) + ((stage & 8) ? 4ull : 0ull) +
           ((stage & 16) ? 12ull : 0ull) + (sorted ? 16ull : 0ull);
}

// the clause as it reads
static long long clause(long long n, int stage, bool sorted, unsigned long long budget) {
    u128 k = ((u128)n + 63) / 64 * 64;
    if (k > ((u128)1 << 24)) k = (u128)1 << 24;
    const u128 per = bytes_per_ray(stage, sorted);
    if (per != 0) {
        u128 fit = (u128)budget / per / 64 * 64;
        if (fit < k) k = fit;
        if (k < 64) k = 64;
    }
    return (long long)k;
}

static bool plan(long long n, int stage, bool sorted, unsigned long long budget, CastPlan *p) {
    return cast_plan(n, stage & 1, stage & 2, stage & 4, stage & 8, stage & 16, sorted, budget, p);
}

static void check(long long n, int stage, bool sorted, unsigned long long budget) {
    CastPlan p;
    const bool ok = plan(n, stage, sorted, budget, &p);
    EXPECT(ok);
    if (!ok) return;
    const long long want = clause(n, stage, sorted, budget);
    if (p.chunk != want) std::printf("n %lld stage %d sorted %d budget %llu: chunk %d, clause %lld\n", n, stage, (int)sorted, budget, p.chunk, want);
    EXPECT(p.chunk == want);
    EXPECT(p.chunk >= 64 && p.chunk % 64 == 0 && p.chunk <= HZ_CAST_MAX_CHUNK);
    EXPECT((long long)p.chunk < n + 64);                         // never more than the call's rays, rounded up to a wave
    const unsigned long long per = bytes_per_ray(stage, sorted);
    EXPECT(p.per_ray == per);
    EXPECT(p.stage_bytes == (unsigned long long)p.chunk * per);
    // the memory is within the budget unless one wave alone exceeds it
    if (per) EXPECT(p.stage_bytes <= budget || p.chunk == 64);
    // the chunk of a call that needs several does not depend on its number of rays
    if (n > p.chunk) {
        CastPlan q;
        EXPECT(plan(2 * n <= HZ_CAST_MAX_RAYS ? 2 * n : HZ_CAST_MAX_RAYS, stage, sorted, budget, &q) && q.chunk == p.chunk && q.stage_bytes == p.stage_bytes);
    }
}

int main() {
    CastPlan p;
    // refused
    EXPECT(!plan(0, 31, true, HZ_CAST_BUDGET, &p));
    EXPECT(!plan(-1, 31, true, HZ_CAST_BUDGET, &p));
    EXPECT(!plan(HZ_CAST_MAX_RAYS + 1, 0, false, HZ_CAST_BUDGET, &p));
    EXPECT(!plan(1ll << 40, 0, false, HZ_CAST_BUDGET, &p));
    EXPECT(!plan(1, 31, true, 0, &p));

    // N = 1, 64, 65: one wave, one wave, two
    EXPECT(plan(1, 0, false, HZ_CAST_BUDGET, &p) && p.chunk == 64 && p.stage_bytes == 0 && p.per_ray == 0);
    EXPECT(plan(1, 31, true, HZ_CAST_BUDGET, &p) && p.chunk == 64 && p.per_ray == 57 && p.stage_bytes == 64 * 57);
    EXPECT(plan(64, 31, false, HZ_CAST_BUDGET, &p) && p.chunk == 64 && p.per_ray == 41);
    EXPECT(plan(65, 31, false, HZ_CAST_BUDGET, &p) && p.chunk == 128);
    EXPECT(plan(65, 4, false, 127, &p) && p.chunk == 64);
    EXPECT(plan(65, 4, false, 128, &p) && p.chunk == 128);
    // the largest call: nothing staged takes the launch's limit, everything staged the budget's
    EXPECT(plan(HZ_CAST_MAX_RAYS, 0, false, HZ_CAST_BUDGET, &p) && p.chunk == HZ_CAST_MAX_CHUNK && p.stage_bytes == 0);
    EXPECT(plan(HZ_CAST_MAX_RAYS, 31, true, HZ_CAST_BUDGET, &p) && p.chunk == 4709376 && p.stage_bytes <= HZ_CAST_BUDGET);     // 268435456 / 57 = 4709393 -> 73584 waves
    EXPECT(plan(HZ_CAST_MAX_RAYS, 0, true, HZ_CAST_BUDGET, &p) && p.chunk == HZ_CAST_MAX_CHUNK && p.stage_bytes == (256ull << 20));
    EXPECT(plan(HZ_CAST_MAX_RAYS, 31, true, ~0ull, &p) && p.chunk == HZ_CAST_MAX_CHUNK);
    // budgets down to one wave and below
    EXPECT(plan(4099, 28, false, 17 * 1024, &p) && p.chunk == 1024);       // occluded + dist + point: 17 bytes per ray
    EXPECT(plan(4099, 28, false, 17 * 1024 - 1, &p) && p.chunk == 960);
    EXPECT(plan(4099, 28, false, 17 * 64, &p) && p.chunk == 64);
    EXPECT(plan(4099, 28, false, 1, &p) && p.chunk == 64 && p.stage_bytes == 17 * 64);
    EXPECT(plan(4099, 0, false, 1, &p) && p.chunk == 4160);                // nothing staged: the budget plays no part
    EXPECT(plan(8198, 28, false, 17 * 1024, &p) && p.chunk == 1024);

    // sweep against the clause: every staging combination, with and without the sort
    const long long counts[] = {1, 2, 63, 64, 65, 127, 128, 129, 257, 4099, 8198, (1 << 24) - 64, (1 << 24) - 63, 1 << 24, (1 << 24) + 1,
                                1ll << 30, HZ_CAST_MAX_RAYS - 1, HZ_CAST_MAX_RAYS};
    const unsigned long long budgets[] = {1, 16, 57, 63, 64, 64 * 57 - 1, 64 * 57, 64 * 57 + 1, 17 * 1024, 1 << 20, HZ_CAST_BUDGET, 1ull << 31, 1ull << 40, ~0ull};
    long cases = 0;
    for (long long n : counts)
        for (unsigned long long b : budgets)
            for (int stage = 0; stage < 32; stage++)
                for (int sorted = 0; sorted < 2; sorted++) { check(n, stage, sorted != 0, b); cases++; }
    std::printf("%ld cases\n", cases);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("cast plan ok\n");
    return 0;
}
