// Host program for horayzon_amd/csrc/hz_sight_search.h (tests/test_sight_search_host.py builds it with ASan + UBSan and runs it
// on the CPU): the header compiles without a device compiler, and the per-lane search of Terrain.sight_height, driven one lane
// at a time, follows DESIGN.md section 4 clause 19 -- the order top, bottom, bisection; the result; the ray count -- for every
// table length up to a bound and for the packing limit, for monotone visibility with every first visible index and for random
// answers.  Every index the search asks for is read from a table of exactly n entries, so an index out of range is a
// sanitizer finding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../horayzon_amd/csrc/hz_sight_search.h"

using namespace hz;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { if (failures++ < 20) std::printf("line %d: %s failed\n", __LINE__, #c); } } while (0)

struct Outcome { int result; int rays; };          // result: a table index, or -1 for +inf

// the clause, written down as it reads; `vis` answers visible(k) and counts
template <typename V>
static Outcome clause(int n, V vis) {
    int rays = 0;
    auto ask = [&](int k) { rays++; return vis(k); };
    if (!ask(n - 1)) return {-1, rays};
    if (n == 1 || ask(0)) return {0, rays};
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ask(mid)) hi = mid; else lo = mid;
    }
    return {hi, rays};
}

// the state machine, one lane; `order` takes the indices in the order they were asked for
template <typename V>
static Outcome machine(int n, const std::vector<float> &table, V vis, std::vector<int> *order) {
    int phase = SIGHT_IDLE; unsigned lohi = 0;
    int k = sight_begin(phase, lohi, n);
    int rays = 0;
    volatile float sink = 0.0f;
    for (int guard = 0; guard < 64; guard++) {
        EXPECT(sight_is_index(k) && k < n);
        EXPECT(phase == SIGHT_TOP || phase == SIGHT_BOTTOM || phase == SIGHT_BISECT);
        sink = table.at((size_t)k);                // the kernel's one table load per ray
        if (order) order->push_back(k);
        rays++;
        k = sight_advance(phase, lohi, n, vis(k));
        if (!sight_is_index(k)) {
            EXPECT(phase == SIGHT_IDLE);
            EXPECT(k != SIGHT_DONE);
            if (k == SIGHT_UNREACHED) return {-1, rays};
            const int idx = sight_result_index(k);
            EXPECT(idx >= 0 && idx < n);
            sink = table.at((size_t)idx);
            return {idx, rays};
        }
    }
    (void)sink;
    EXPECT(!"the search did not end");
    return {-2, rays};
}

static int ceil_log2(int x) { int b = 0; while ((1 << b) < x) b++; return b; }

static void monotone(int n, int first) {           // visible(k) <=> k >= first; first == n: never
    std::vector<float> table((size_t)n, 1.0f);
    auto vis = [&](int k) { return k >= first; };
    std::vector<int> order;
    const Outcome a = clause(n, vis), b = machine(n, table, vis, &order);
    EXPECT(a.result == b.result && a.rays == b.rays);
    EXPECT(b.result == (first == n ? -1 : first));
    EXPECT(order[0] == n - 1);
    if (order.size() > 1) EXPECT(order[1] == 0);
    if (first == n) EXPECT(b.rays == 1);
    else if (first == 0) EXPECT(b.rays == (n == 1 ? 1 : 2));
    else EXPECT(b.rays >= 2 && b.rays <= 2 + ceil_log2(n - 1));
}

int main() {
    // packing
    for (int lo : {0, 1, 255, 65533}) for (int hi : {0, 1, 256, 65534}) {
        const unsigned w = sight_pack(lo, hi);
        EXPECT(sight_lo(w) == lo && sight_hi(w) == hi);
    }
    for (int idx : {0, 1, 65534}) EXPECT(sight_result_index(sight_result_index(idx)) == idx && !sight_is_index(sight_result_index(idx)));
    // every table length up to 300 and around the packing limit, every first visible index (a stride for the long tables)
    for (int n = 1; n <= 300; n++)
        for (int first = 0; first <= n; first++) monotone(n, first);
    for (int n : {1023, 1024, 1025, 4097, 32768, 32769, 65534, 65535}) {
        for (int first = 0; first <= n; first += 1 + n / 997) monotone(n, first);
        for (int first : {0, 1, 2, n / 2, n - 2, n - 1, n}) monotone(n, first);
    }
    // random answers (visibility that is not monotone): the machine is the clause, whatever the answers
    uint64_t seed = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    for (int trial = 0; trial < 20000; trial++) {
        const int n = (trial % 7 == 0) ? 65535 - (int)(rnd() % 3) : 1 + (int)(rnd() % 2000);
        const uint64_t salt = rnd();
        const unsigned bias = (unsigned)(rnd() % 5);
        auto vis = [&](int k) {
            uint64_t x = salt ^ ((uint64_t)k * 0xff51afd7ed558ccdull);
            x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 29;
            return (x % 5) >= bias;
        };
        std::vector<float> table((size_t)n, 1.0f);
        const Outcome a = clause(n, vis), b = machine(n, table, vis, nullptr);
        EXPECT(a.result == b.result && a.rays == b.rays);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("sight search ok\n");
    return 0;
}
