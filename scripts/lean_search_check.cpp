// lean_search_check.cpp -- host check of the lean search state of the flat guess_constant refill (hz_search.h: SearchLean,
// advance_az0_lean, advance_guess_flat) against the state machine it stands for, advance<ALG_GUESS>.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I<rocm>/include
//       scripts/lean_search_check.cpp -o lean_search_check && ./lean_search_check
//
// A plain host compiler sees hz_search.h with __device__ defined away (the HIP headers do that for it).  Both forms are driven cell by
// cell with the same hit / miss answers; after every call the states, the return values, the guard tallies, what the flat form told
// its two callbacks and every emitted value must be equal.  At random points both cells are handed over through a 16-word record
// as k_horizon writes it (hz_horizon.hip, hz_left_write) -- CROSSWISE: the lean form goes on from the record the Search form wrote and
// the other way round, so a record written by either form is restored by either form.  Also: hz_n_leave_packed == hz_n_leave.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace hz {
using std::max;
using std::min;
}
static inline unsigned long long __ballot(int pred) { return pred ? 1ull : 0ull; }      // a wave of one lane
static inline float __int_as_float(int v) { float f; memcpy(&f, &v, 4); return f; }
static inline int __float_as_int(float f) { int v; memcpy(&v, &f, 4); return v; }
#define HZ_BOX_START_PADS 16.0f      // (hz_common.h defines it for the device compiler only; hz_internal.h names it; nothing here reads it)
#include "../horayzon_amd/csrc/hz_search.h"

using namespace hz;

struct HostTables {
    std::vector<float> azim_sin, azim_cos, elev_ang, elev_sin, elev_cos;
    std::vector<int> mid_idx;
    Tables t;
};

// the expressions of build_tables (hz_api_horizon.hip)
static void build(int azim_num, float acc_deg, float low_deg, HostTables &h) {
    const float d2r = (float)(M_PI / 180.0);
    Tables &t = h.t;
    t.hori_acc = acc_deg * d2r; t.low = low_deg * d2r; t.up = 89.98f * d2r;
    t.step = (double)t.hori_acc / 5.0;
    t.azim_num = azim_num;
    h.azim_sin.assign((size_t)azim_num, 0.0f); h.azim_cos.assign((size_t)azim_num, 1.0f);
    t.elev_num = (int)ceil((double)(t.up - t.low) / t.step) + 1;
    const size_t n = (size_t)t.elev_num;
    h.elev_ang.resize(n); h.elev_sin.resize(n); h.elev_cos.resize(n);
    for (int i = 0; i < t.elev_num; i++) {
        const float ang = (float)((double)t.up - t.step * (double)i);
        h.elev_ang[n - 1 - (size_t)i] = ang; h.elev_sin[n - 1 - (size_t)i] = sinf(ang); h.elev_cos[n - 1 - (size_t)i] = cosf(ang);
    }
    h.mid_idx.assign(2 * n, 0);
    for (int i = 0; i + 10 < t.elev_num; i++) {
        const float es = (float)((double)(h.elev_ang[(size_t)i] + h.elev_ang[(size_t)i + 10]) / 2.0);
        const int mid = (int)roundf((float)((double)(es - t.low) / t.step));
        h.mid_idx[2 * (size_t)i] = mid;
        const float ev = h.elev_ang[(size_t)std::min(std::max(mid, 0), t.elev_num - 1)];
        memcpy(&h.mid_idx[2 * (size_t)i + 1], &ev, 4);
    }
    t.azim_sin = h.azim_sin.data(); t.azim_cos = h.azim_cos.data();
    t.elev_ang = h.elev_ang.data(); t.elev_sin = h.elev_sin.data(); t.elev_cos = h.elev_cos.data(); t.mid_idx = h.mid_idx.data();
}

static long long g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the record words of the search state (hz_horizon.hip): 1 k, 2 phase, 3 ind, 4 prev, 5 pazim, 6 count, 7 - 10 four floats
static void write_full(uint32_t *w, const Search &s) {
    w[1] = (uint32_t)s.k; w[2] = (uint32_t)s.phase; w[3] = (uint32_t)s.ind; w[4] = (uint32_t)s.prev; w[5] = (uint32_t)s.pazim; w[6] = (uint32_t)s.count;
    memcpy(&w[7], &s.lim_up, 4); memcpy(&w[8], &s.lim_low, 4); memcpy(&w[9], &s.elev_samp, 4); memcpy(&w[10], &s.ev, 4);
}
static void write_lean(uint32_t *w, const SearchLean &s, const float *lim, int stride) {
    w[1] = (uint32_t)s.k; w[2] = (uint32_t)s.phase; w[3] = (uint32_t)s.ind; w[4] = (uint32_t)s.prev; w[5] = (uint32_t)s.pazim; w[6] = (uint32_t)s.count;
    w[7] = w[8] = w[9] = w[10] = 0u;
    if (s.phase == PH_BIN) { memcpy(&w[7], &lim[0], 4); memcpy(&w[8], &lim[stride], 4); }
}
static void read_full(const uint32_t *w, Search &s) {
    s.k = (int)w[1]; s.phase = (int)w[2]; s.ind = (int)w[3]; s.prev = (int)w[4]; s.pazim = (int)w[5]; s.count = (int)w[6];
    memcpy(&s.lim_up, &w[7], 4); memcpy(&s.lim_low, &w[8], 4); memcpy(&s.elev_samp, &w[9], 4); memcpy(&s.ev, &w[10], 4);
}
static void read_lean(const uint32_t *w, SearchLean &s, float *lim, int stride) {
    s.k = (int)w[1]; s.phase = (int)w[2]; s.ind = (int)w[3]; s.prev = (int)w[4]; s.pazim = (int)w[5]; s.count = (int)w[6];
    if (s.phase == PH_BIN) { memcpy(&lim[0], &w[7], 4); memcpy(&lim[stride], &w[8], 4); }
}

struct Tally { long long calls = 0, bin_calls = 0, records = 0, bin_records = 0, guards = 0, end_low = 0, end_top = 0, emitted = 0, clamped_mid = 0; };

// mode 0: a horizon that wanders from azimuth to azimuth; 1: below the table (every ray free: azimuth 0 ends at index 0, DOWN runs
// into index 0); 2: above it (every ray blocked: the top index, UP guards); 3: answers at random
template <bool STAGE>
static void run_cells(const HostTables &h, int cells, int mode, uint32_t seed, Tally &ty) {
    const Tables &t = h.t;
    const int A = t.azim_num, top = t.elev_num - 1, stride = 3;      // (a stride that is not 1: lim[stride] and stage[j * stride] are not neighbours)
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    for (int c = 0; c < cells; c++) {
        // output rows and staging words of the two forms (exact sizes: the sanitizer sees every access outside them)
        std::vector<float> hr_v((size_t)A + 4, -9.0f), hl_v((size_t)A + 4, -9.0f);
        float *hr = hr_v.data(), *hl = hl_v.data();
        while ((reinterpret_cast<uintptr_t>(hr) & 15u) != 0) hr++;
        while ((reinterpret_cast<uintptr_t>(hl) & 15u) != 0) hl++;
        std::vector<float> lds_r(4 * (size_t)stride, NAN), lds_l(4 * (size_t)stride, NAN);      // rows 0 ... 3 of one lane
        Sink out_r, out_l;
        out_r.hori = hr; out_r.dist = nullptr; out_r.dist_hit = 0; out_r.stage = lds_r.data(); out_r.stride = stride;
        out_l.hori = hl; out_l.dist = nullptr; out_l.dist_hit = 0; out_l.stage = lds_l.data(); out_l.stride = stride;
        float *lim = lds_l.data() + (STAGE ? 2 : 0) * stride;      // rows 2 and 3 with staging, the two padding rows without (k_horizon)
        Search sr; sr.k = 0; sr.phase = PH_NEWAZ; sr.ind = sr.prev = sr.pazim = sr.count = 0; sr.lim_up = sr.lim_low = sr.elev_samp = sr.ev = 0;
        SearchLean sl; sl.k = 0; sl.phase = PH_NEWAZ; sl.ind = sl.prev = sl.pazim = sl.count = 0;
        unsigned gr = 0, gl = 0;
        float horizon = t.low + uni(rng) * (t.up - t.low);
        bool hit = false;
        int last_k = 0;
        for (;;) {
            int cb_k = -1, cb_ind = -1;
            const bool was_bin = sl.phase == PH_BIN || (sl.phase == PH_NEWAZ && sl.k == 0);
            const bool go_r = advance<ALG_GUESS, STAGE>(sr, hit, t, out_r, gr);
            const bool go_l = advance_guess_flat<STAGE>(sl, hit, t, out_l, gl, lim, stride, [&](int k) { cb_k = k; }, [&](int i) { cb_ind = i; });
            ty.calls++; ty.bin_calls += was_bin ? 1 : 0;
            CHECK(go_r == go_l, "cell %d", c);
            CHECK(gr == gl, "cell %d guards %u %u", c, gr, gl);
            if (!go_r || !go_l) { CHECK(sr.k == A && sl.k == A, "k %d %d", sr.k, sl.k); break; }
            CHECK(sr.k == sl.k && sr.phase == sl.phase && sr.ind == sl.ind && sr.prev == sl.prev && sr.pazim == sl.pazim && sr.count == sl.count,
                  "cell %d: k %d %d phase %d %d ind %d %d prev %d %d pazim %d %d count %d %d", c, sr.k, sl.k, sr.phase, sl.phase, sr.ind, sl.ind,
                  sr.prev, sl.prev, sr.pazim, sl.pazim, sr.count, sl.count);
            CHECK(cb_k == std::min(sl.k, A - 1) && cb_ind == sl.ind, "callbacks %d %d for k %d ind %d", cb_k, cb_ind, sl.k, sl.ind);
            CHECK(sl.ind >= 0 && sl.ind <= top && sl.k >= 0 && sl.k < A, "range");
            if (sl.phase == PH_BIN)
                CHECK(memcmp(&lim[0], &sr.lim_up, 4) == 0 && memcmp(&lim[stride], &sr.lim_low, 4) == 0, "lim %g %g against %g %g", lim[0], lim[stride], sr.lim_up, sr.lim_low);
            CHECK(memcmp(hr, hl, sizeof(float) * (size_t)A) == 0, "cell %d: emitted values differ at k %d", c, sl.k);
            if (STAGE) for (int j = 0; j < (sl.k & 3); j++)
                CHECK(memcmp(&lds_r[(size_t)j * stride], &lds_l[(size_t)j * stride], 4) == 0, "staged value %d of azimuth %d", j, sl.k);
            if (sl.k != last_k) { last_k = sl.k; ty.emitted++; if (mode == 0) horizon = std::min(std::max(horizon + (uni(rng) - 0.5f) * 0.2f, t.low - 0.1f), t.up + 0.1f); }
            if (sl.ind == 0) ty.end_low++;
            if (sl.ind == top) ty.end_top++;
            if (std::abs(sl.ind - sl.prev) != 10 && sl.phase >= PH_UP) ty.clamped_mid++;
            // hand over through a record, crosswise (more often in azimuth 0, where words 7 and 8 carry the two LDS values)
            if (uni(rng) < (sl.phase == PH_BIN ? 0.25f : 0.01f)) {
                uint32_t wr[16] = {0}, wl[16] = {0};
                float st_r[3], st_l[3];
                for (int j = 0; j < 3; j++) { st_r[j] = lds_r[(size_t)j * stride]; st_l[j] = lds_l[(size_t)j * stride]; }
                write_full(wr, sr); write_lean(wl, sl, lim, stride);
                CHECK(sl.phase != PH_BIN || (wl[7] == wr[7] && wl[8] == wr[8]), "record words 7 / 8");
                CHECK(sl.phase == PH_BIN || (wl[7] | wl[8]) == 0u, "words 7 / 8 outside PH_BIN");
                CHECK((wl[9] | wl[10]) == 0u, "words 9 / 10");
                std::fill(lds_r.begin(), lds_r.end(), NAN); std::fill(lds_l.begin(), lds_l.end(), NAN);     // another wave's LDS
                Search nr; SearchLean nl;
                read_full(wl, nr);                      // the Search form restores the lean form's record
                if (STAGE) for (int j = 0; j < 3; j++) { lds_r[(size_t)j * stride] = st_l[j]; lds_l[(size_t)j * stride] = st_r[j]; }
                read_lean(wr, nl, lim, stride);         // ... and the lean form the other's (behind the staged values, as in k_horizon)
                sr = nr; sl = nl;
                ty.records++; ty.bin_records += sl.phase == PH_BIN ? 1 : 0;
            }
            const float e = t.elev_ang[sl.ind];
            hit = mode == 1 ? false : mode == 2 ? true : mode == 3 ? (uni(rng) < 0.5f) : (e < horizon);
        }
        ty.guards += gl;
        CHECK(memcmp(hr, hl, sizeof(float) * (size_t)A) == 0, "cell %d: rows differ", c);
        for (int k = 0; k < A; k++) CHECK(hl[k] != -9.0f, "azimuth %d was never emitted", k);
    }
}

int main() {
    Tally ty;
    const struct { int azim; float acc, low; } cfg[] = {{8, 0.25f, -15.0f}, {6, 0.25f, -60.0f}, {1, 0.25f, -15.0f}, {90, 0.25f, 5.0f},
                                                         {360, 1.0f, -15.0f}, {4, 3.0f, 80.0f}, {5, 0.25f, 89.0f}};
    uint32_t seed = 1;
    for (const auto &c : cfg) {
        HostTables h;
        build(c.azim, c.acc, c.low, h);
        for (int mode = 0; mode < 4; mode++) {
            const int cells = std::max(40, 60000 / c.azim);
            if ((c.azim & 3) == 0) run_cells<true>(h, cells, mode, seed++, ty);
            run_cells<false>(h, cells, mode, seed++, ty);
        }
    }
    // the packed form of the compaction threshold (hz_common.h)
    for (int regroup = 1; regroup <= 64; regroup++)
        for (int rule = 0; rule < 2; rule++)
            for (int round = 0; round < 64; round++)
                for (int n = 1; n <= 64; n++)
                    CHECK(hz_n_leave_packed(hz_n_leave_pack(regroup, rule, round), n) == hz_n_leave(regroup, n, rule, round), "n_leave %d %d %d %d", regroup, rule, round, n);
    printf("transitions %lld (azimuth 0: %lld)  records %lld (in PH_BIN: %lld)  guards %lld  samples at index 0 / top: %lld / %lld  "
           "clamped steps %lld  azimuths %lld\n", ty.calls, ty.bin_calls, ty.records, ty.bin_records, ty.guards, ty.end_low, ty.end_top, ty.clamped_mid, ty.emitted);
    if (ty.calls < 1000000 || ty.bin_records < 1000 || ty.guards == 0 || ty.end_low == 0 || ty.end_top == 0 || ty.clamped_mid == 0) {
        printf("the run did not cover what it is for\n");
        return 1;
    }
    if (g_fail) { printf("lean search: %lld checks FAILED\n", g_fail); return 1; }
    printf("lean search: all checks passed\n");
    return 0;
}
