// hz_internal.h -- host-side internals of libhorayzon_hip (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include "../../include/horayzon_hip.h"
#include "hz_common.h"
#include "hz_horizon_plan.h"
#include <atomic>
#include <mutex>

#define HZ_MAX_TOP_NODES 2047   // upper bound of BFS-ordered top nodes (LDS staging)
#define HZ_MAX_STACK 40         // tree levels (= LDS stack entries per lane) the traversal kernels accept
// hit cache: levels between a leaf and its cached ancestor.  Measured 1..9 on the 3601^2 tile in round 1 (5-6 best) and again in
// round 5 after a cache walk that finds nothing stopped costing a trip through the caller (hz_horizon.hip: the root waits below the
// cached subtree): 3 and 4 tie, 0.7 % ahead of 5, 6 loses 1.6 %; discrete_sampling +7 % with 4 (profiles/r05/sweep_regroup_anc_after_cache_fix.log)
#ifndef HZ_ANC_LEVELS
#define HZ_ANC_LEVELS 4
#endif

namespace hz {

int set_error(int code, const char *fmt, ...);

#define HZ_SHADOW_FAST_CAP_DEFAULT 19   // entries of k_shadow_refill's fast stack (hz_shadow.hip)
// test knobs (hz_debug_set, include/horayzon_hip.h): process wide, read at every launch; results never depend on them
extern std::atomic<int> g_shadow_fast_cap;   // entries of k_shadow_refill's fast stack (default HZ_SHADOW_FAST_CAP_DEFAULT; 0: level stack only)
extern std::atomic<int> g_leaf_lend;         // 1 (default): k_horizon's fast stack lends idle lanes to the partner lane's second queued leaf (hz_trace, LEND)
extern std::atomic<int> g_flat_refill;       // 1 (default): guess_constant's fast-stack instantiations refill through advance_guess_flat (hz_search.h, FLAT)
extern std::atomic<int> g_regroup_rule;      // 1 (default): k_horizon's compaction threshold scales with the lanes that enter hz_trace (hz_n_leave, rule 1); 0: absolute
// (rounding of the relative threshold: 8 / 16 / 24 / 32 / 48 / 63 all run 1.158 - 1.166 s where the absolute rule runs 1.182 - 1.186 s,
//  profiles/r09/ab_regroup_rule.log call 5 -- time does not tell them apart; 48 had the narrowest range, 1.158 - 1.159 s)
#define HZ_REGROUP_ROUND 48
extern std::atomic<int> g_regroup_round;     // rule 1: the rounding addend of hz_n_leave, 0 ... 63 (default HZ_REGROUP_ROUND)
// (bit 16 of hz_opts.regroup forces rule 0 for one call: the A/B inside one library and process)
inline int regroup_rule_of(int opts_regroup) {
    return (g_regroup_rule.load(std::memory_order_relaxed) != 0 && !(opts_regroup > 0 && (opts_regroup & 0x10000))) ? 1 : 0;
}
extern std::atomic<int> g_topo_wide;         // 1: the reductions over the azimuth axis use the fallback kernel k_topo_wide
extern std::atomic<int> g_accum_chunk;       // > 0: sun positions per chunk of hz_terrain_accumulate (default 0: from the memory budget)
extern std::atomic<int> g_coarse_tile;       // > 0: cells of k_coarse_reduce's LDS tile, at most the default (hz_subgrid.hip; default 0)
extern std::atomic<int> g_horisun_chunk;     // > 0: sun positions per launch of hz_horizon_terrain_run (default 0: HZ_HORISUN_CHUNK)
extern std::atomic<int> g_horisun_coarse_tile;    // > 0: cells of k_horisun_coarse's LDS tile, at most the default (hz_horisun_coarse.hip; default 0)
extern std::atomic<int> g_horisun_coarse_route;   // hz_horizon_terrain_sw_dir_cor_coarse: 0 the fused kernel, 1 the two-pass route, -1 the layout's default

#define HZ_HIP(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return ::hz::set_error(HZ_ERR_HIP, "%s failed: %s (%s:%d)", #expr,            \
                                   hipGetErrorString(e_), __FILE__, __LINE__);            \
    } while (0)

struct Timer {
    std::chrono::high_resolution_clock::time_point t0;
    void start() { t0 = std::chrono::high_resolution_clock::now(); }
    double stop() const {
        return std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    }
};

struct Scene {
    int device = 0;
    hipStream_t stream = nullptr;
    void *blob = nullptr;
    size_t blob_bytes = 0;
    bool owns_blob = false;
    // 1 once a launch with the fast stack discipline overflowed: later launches use the one-entry-per-level kernel
    mutable std::atomic<int> level_stack{0};
    // Calls that launch on the scene's stream (horizon, locations, terrain set-up and shadow) hold `run_mu` from their
    // first enqueue to their last synchronisation: concurrent calls on one scene are allowed through the C ABI
    // (`const hz_scene *`, ctypes releases the GIL) and simply run one after the other -- they share the stream, so
    // the GPU would serialise them anyway.  This is what makes the scene-owned scratch below safe.
    mutable std::mutex run_mu;
    // scratch of the near-field certificates, grown on demand and kept with the scene (hz_api_horizon.hip; guarded by run_mu)
    mutable void *near_buf = nullptr;
    mutable size_t near_bytes = 0;
    // records of the cells a production launch of k_horizon left unfinished (hz_horizon.hip: leftover cells; guarded by run_mu)
    mutable void *left_buf = nullptr;
    mutable size_t left_bytes = 0;
    // grows one of the two scratch buffers to `need` bytes (the old contents are dropped); false: hipMalloc failed, the buffer is empty
    static bool grow_scratch(void *&buf, size_t &bytes, size_t need) {
        if (bytes >= need) return true;
        if (buf) (void)hipFree(buf);
        buf = nullptr; bytes = 0;
        if (hipMalloc(&buf, need) != hipSuccess) { (void)hipGetLastError(); buf = nullptr; return false; }
        bytes = need;
        return true;
    }
    BlobHeader hdr;
    const float *verts() const { return (const float *)((const char *)blob + hdr.off_verts); }
    const Node *nodes() const { return (const Node *)((const char *)blob + hdr.off_nodes); }
    const Prim *prims() const { return (const Prim *)((const char *)blob + hdr.off_prims); }
    const int *anc() const { return (const int *)((const char *)blob + hdr.off_anc); }
};

// hz_scene.hip
int scene_build(Scene *sc, const float *vert_grid, int d0, int d1, const float *vert_simp, int nvs,
                const int32_t *tri_simp, int nts, hz_stats *stats);

// device-side view handed to the traversal kernels
struct SceneView {
    const float *verts;
    const Node *nodes;
    const Prim *prims;
    const int *anc;  // hit-cache ancestors, one per leaf
    int d1;          // DEM row length (vertices)
    int n_top;       // BFS-ordered top nodes available for LDS staging
    float cx, cy, cz;
    float tau;       // box tests start at -tau and end at tfar + tau (hz_common.h: HZ_BOX_START_PADS)
};

inline SceneView scene_view(const Scene *sc) {
    SceneView v;
    v.verts = sc->verts(); v.nodes = sc->nodes(); v.prims = sc->prims(); v.anc = sc->anc();
    v.d1 = sc->hdr.d1; v.n_top = sc->hdr.n_top;
    v.cx = sc->hdr.center[0]; v.cy = sc->hdr.center[1]; v.cz = sc->hdr.center[2];
    v.tau = HZ_BOX_START_PADS * sc->hdr.pad;
    return v;
}

inline TileMap make_tile_map(int tiles_i, int tiles_j, int gw = 8) {
    TileMap m;
    m.tiles_i = tiles_i; m.tiles_j = tiles_j; m.gw = gw;
    m.rj = std::max(1, (tiles_j + 7) / 8);
    // patch rows: near-square patches, but at least 16 rows when the grid is high enough and at most 64.  Measured on
    // the 3601^2 tile (224 x 224 tiles; kernel ms per tile): 1 row 2016 (= one region per XCD, rounds 1-2: 2009 - 2014),
    // 2: 1957, 4: 1980, 8: 1945, 16: 1932, 32: 1931, 56: 1930, 112: 1928, 224: 1934; shadow kernel on its 224 x 7 grid of
    // super tiles (ms per sun position): 1: 1.455, 8: 1.265, 32: 1.317, 56: 1.260, 112: 1.417
    int pi = (tiles_i + m.rj - 1) / m.rj;
    pi = std::min(std::max(pi, std::min(16, tiles_i / 4)), 64);
    pi = std::max(1, std::min(pi, tiles_i));
    m.pi = pi;
    m.ri = (tiles_i + pi - 1) / pi;
    m.pi = (tiles_i + m.ri - 1) / m.ri;                  // drop patch rows that would be empty
    m.per_xcd = m.pi * m.ri * m.rj;
    return m;
}

// true if p points to device memory (HBM); false for host memory
bool is_device_ptr(const void *p);

// device view of an input array that may live on the host
template <typename T>
struct DevIn {
    const T *dev = nullptr;
    void *owned = nullptr;
    ~DevIn() { if (owned) (void)hipFree(owned); }
    int bind(const T *src, size_t count, hipStream_t st) {
        if (!src || count == 0) { dev = nullptr; return HZ_OK; }
        if (is_device_ptr(src)) { dev = src; return HZ_OK; }
        HZ_HIP(hipMalloc(&owned, count * sizeof(T)));
        HZ_HIP(hipMemcpyAsync(owned, src, count * sizeof(T), hipMemcpyHostToDevice, st));
        dev = static_cast<const T *>(owned);
        return HZ_OK;
    }
};

// device buffer for an output array that may live on the host
template <typename T>
struct DevOut {
    T *dev = nullptr;
    T *host = nullptr;
    void *owned = nullptr;
    size_t count = 0;
    ~DevOut() { if (owned) (void)hipFree(owned); }
    int bind(T *dst, size_t n) {
        count = n;
        if (!dst || n == 0) { dev = nullptr; return HZ_OK; }
        if (is_device_ptr(dst)) { dev = dst; return HZ_OK; }
        HZ_HIP(hipMalloc(&owned, n * sizeof(T)));
        dev = static_cast<T *>(owned); host = dst;
        return HZ_OK;
    }
    int finish(hipStream_t st) {
        if (host && count) HZ_HIP(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, st));
        return HZ_OK;
    }
};

// device memory that is freed with its scope
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};

// a timing event, created when it is first recorded
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    int record(hipStream_t st) {
        if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; return set_error(HZ_ERR_HIP, "hipEventCreate failed"); }
        (void)hipEventRecord(e, st);
        return HZ_OK;
    }
    // milliseconds from this event to `end`; 0 when one of them was never recorded
    float ms_until(const Event &end) const {
        float ms = 0.0f;
        if (e && end.e) (void)hipEventElapsedTime(&ms, e, end.e);
        return ms;
    }
};

// hz_api.hip: hipSetDevice after a range check; what hz_scene_destroy does (the sun-position drivers own scenes too)
int select_device(int device);
void scene_free(Scene *sc);

// streams come from a per-device pool and go back to it: the library never calls hipStreamDestroy (hz_api.hip)
int stream_acquire(int device, hipStream_t *st);
void stream_release(int device, hipStream_t st);

// horizon_comp.cpp:37-39
inline float deg2rad_f(float ang) { return (float)(((double)ang / 180.0) * M_PI); }

// hz_horizon.hip
struct HorizonArgs {
    const float *vec_norm, *vec_north;   // device
    const uint8_t *mask;                 // device
    float *hori;                         // device, may be null (skip_hori)
    int offset_0, offset_1, dim_in_0, dim_in_1;
    int row_begin, row_end;
    int azim_num, elev_num, alg;
    float hori_acc, low, up, dist;       // radians / metres
    float hori_fill, ray_org_elev;
    const float *azim_sin, *azim_cos, *elev_ang, *elev_sin, *elev_cos;  // device tables
    const int *mid_idx;
    int top_nodes, regroup, count_work, hit_cache;
    int level_stack;                     // 1: one-entry-per-level traversal stack (cannot overflow); 0: fast discipline
    const int *tile_list;                // null: every tile of the rows; else the n_list 8 x 8 blocks (workgroup number of
    int n_list;                          //   the full launch * 4 + wave) to compute: the blocks whose fast stack overflowed
    const unsigned short *near_idx;      // near-field certificates of rows [row_begin, row_end) (hz_near.hip) or null
    const float *near_r;
    int verify_near;                     // counting instantiation: N >= 1 re-traces one of every N shortened rays from parameter 0 (1: all)
    float *scratch_row;                  // counting instantiation only: null, or a device row of azim_num floats that takes EVERY store of the launch instead of
                                         // `hori` (the certificate monitor runs next to the production launch and must not write its rows)
    // Leftover cells (hz_horizon.hip): a block ends when at most left_min of its cells are unfinished and appends them to region
    // `left_mode` of left_rec; a launch with left_mode = l >= 1 finishes the records of region l - 1, in the order left_sort(l - 1) left
    // in left_sort (and hands over again when its left_min > 0 and a region l exists).  Region r: left_cap[r] records from record left_base[r].
    int left_min = 0;
    unsigned *left_rec = nullptr;        // HZ_LEFT_WORDS words per record; null: off
    int left_mode = 0;
    unsigned left_base[HZ_LEFT_LEVELS] = {0, 0, 0, 0}, left_cap[HZ_LEFT_LEVELS] = {0, 0, 0, 0};
    int left_regroup = 0, left_key_shift = 0;      // follow-up launches: compaction threshold (0: as `regroup`), log2 of the class width of the sort key
    uint32_t *left_sort = nullptr;       // sort scratch: 4 arrays of left_cap_max words (keys / values, in / out) + sort_temp_elems(left_cap_max)
    unsigned left_cap_max = 0;
    int no_persist = 0;                  // 1: one tile per workgroup instead of persistent waves (same-box A/Bs, tests)
    int persist_grid = 0;                // > 0 (tests): that many workgroups in a persistent launch, so that small grids run the block loop
    unsigned long long *counters;        // device u64[HZ_CNT_N] (the words: HZ_CNT_* below) + 2 x int[HZ_REDO_CAP] (blocks / groups to redo)
};
// the u64 words of HorizonArgs::counters (k_horizon adds to them; horizon_run zeroes them per chunk and reads them back)
enum {
    HZ_CNT_RAYS = 0, HZ_CNT_GUARDS = 1, HZ_CNT_NODES = 2, HZ_CNT_TRIS = 3, HZ_CNT_CELLS = 4,
    HZ_CNT_WAVE_NODE = 5, HZ_CNT_WAVE_LEAF = 6, HZ_CNT_WAVE_REFILL = 7,     // wave-level node / leaf / refill iterations
    HZ_CNT_OVERFLOW = 8,                 // 8 x 8 blocks whose fast-discipline stack overflowed (they are in the first redo list)
    HZ_CNT_SHORTENED = 9,                // rays shortened by a certificate
    HZ_CNT_VIOLATIONS = 10,              // certificate violations (verify)
    HZ_CNT_GUARD_CELLS = 11,             // cells with a guard event
    HZ_CNT_XCD_END = 12,                 // [12..19] counting instantiation: when the last wave of XCD x finished ...
    HZ_CNT_START = 20,                   // ... and ~(the earliest start)
    HZ_CNT_VERIFIED = 21,                // shortened rays that were re-traced (verify)
    HZ_CNT_LENT = 22, HZ_CNT_UNHELPED = 23,    // leaf lending, counting instantiation: leaf tests done by a partner lane, leaf-step lanes with a second leaf and no helper
    HZ_CNT_QUEUES = 24,                  // [24..27] = unsigned[8]: the per-XCD block queues of a persistent launch (zeroed by horizon_launch)
    HZ_CNT_LEFT_CELLS = 28, HZ_CNT_LEFT_AGAIN = 29,    // cells handed over by the production launch / again by a follow-up launch
    HZ_CNT_LEFT_OVERFLOW = 30            // groups of the follow-up launch whose fast stack overflowed (the second redo list)
};
// follow-up launches (hz_opts.left_tune; swept in round 6, profiles/r06/ab_leftover_tune.log: 73 ms against 76 with classes of one
// azimuth and the production launch's threshold of 36; classes of 32 azimuths: 95 ms)
#define HZ_LEFT_KEY_SHIFT 3              // log2 of the width of the azimuths-left classes of the sort key: 8 azimuths
#define HZ_LEFT_REGROUP 24               // compaction threshold in lanes under rule 0 of hz_n_leave (the absolute threshold) ...
#define HZ_LEFT_REGROUP_REL 32           // ... and under rule 1 (profiles/r09/ab_regroup_rule.log: follow-up launch 73.0 -> 71.1 ms, 40 and 48 tie, 56 loses)
#define HZ_CNT_LEFT 32                   // [32..63] = unsigned[HZ_LEFT_LEVELS][16], the control words of the leftover regions: [r][0] = slots
                                         // allocated in region r, [r][1] = valid records (k_left_keys), [r][8 + x] = groups of 64 handed to XCD x
#define HZ_CNT_REFILL 64                 // counting instantiation: [64..71] refills by lanes served (8 buckets of 8), [72..79] by lanes entering hz_trace behind them
#define HZ_CNT_N 80                      // u64 words in front of the redo list
#define HZ_REDO_CAP 16384                // 8 x 8 blocks of one launch that can be repeated one by one after a stack overflow
int horizon_launch(const Scene *sc, const HorizonArgs &a, hipStream_t st, int *used_level_stack = nullptr);
int left_sort(const HorizonArgs &a, int region, hipStream_t st);
int horizon_num_blocks(const HorizonArgs &a);

// hz_topo.hip: any subset of the three reductions over the azimuth axis from one pass over `hori`: the outputs that are
// not NULL are written (at least one; vec_tilt is read when svf or vsf is)
int topo_launch(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1, int len_2,
                float *svf, float *vsf, float *openness, hipStream_t st);
// the same on cell-major 16-bit codes, and straight from an azimuth-major horizon of either element type (q16: codes):
// `planes` points at azimuth 0 of the first of `ncell` cells, azimuth k lies k * stride elements on, vec_tilt and the maps
// start at that cell.  Every map is the words topo_launch gives on the decoded, cell-major horizon.
int topo_launch_q16(const float *azim, const uint16_t *hori, const float *vec_tilt, int len_0, int len_1, int len_2,
                    float *svf, float *vsf, float *openness, hipStream_t st);
int topo_launch_planes_direct(const float *azim, const void *planes, bool q16, size_t stride, const float *vec_tilt, size_t ncell,
                              int A, float *svf, float *vsf, float *openness, hipStream_t st);

// hz_near.hip: near-field certificates (pre-pass of the horizon kernel)
struct NearArgs {
    const float *vec_norm, *vec_north;   // device
    const uint8_t *mask;
    const float *azim_sin, *azim_cos;    // device tables
    int offset_0, offset_1, dim_in_1, row_begin, row_end, azim_num, elev_num;
    float ray_org_elev, hori_acc, low, up;   // radians / metres
    unsigned short *near_idx;            // out [rows * dim_in_1][azim_num]
    float *near_r;                       // out [rows * dim_in_1]
    unsigned *reasons = nullptr;         // debug: device u32[20] histogram of refusals (hz_near.hip), or null
    int ignore_bad_map = 0;              // tests only (opts.no_near_skip < 0): certificates without the scene's per-cell guard
};
int near_launch(const Scene *sc, const NearArgs &a, hipStream_t st);
int near_max_azim();

// hz_locations.hip
struct LocationsArgs {
    const float *coords, *vec_norm, *vec_north, *ray_org_elev;   // device
    float *hori, *dist;                                           // device; dist may be null
    int num_loc, azim_num, elev_num, alg, hori_dist_out;
    float hori_acc, low, up, dist_m;
    const float *azim_sin, *azim_cos, *elev_ang, *elev_sin, *elev_cos;
    const int *mid_idx;
    unsigned long long *counters;
};
int locations_launch(const Scene *sc, const LocationsArgs &a, hipStream_t st);

// hz_shadow.hip
struct ShadowArgs {
    const float *vec_tilt, *vec_norm, *surf_enl_fac, *elevation;   // device
    const uint8_t *mask;
    int offset_0, offset_1, dim_in_0, dim_in_1;
    const float *suns;                   // device f32[num_sun][3]
    int num_sun;                         // positions computed by ONE launch (grid.y); outputs [num_sun][dim_in_0][dim_in_1]
    float sw_dir_cor_fill, dot_prod_min;
    int refrac_cor;
    const double *refrac_fac;            // refrac_cor: device f64[cells], shadow_refrac_factor()
    int which;                           // 0 shadow (u8), 1 sw_dir_cor (f32)
    uint8_t *out_u8; float *out_f32;
    int top_nodes;
    int count_work;                      // 1: the counting instantiation
    unsigned long long *counters;        // device u64[HZ_SHADOW_CNT_N] (the words: HZ_SHADOW_CNT_* below)
};
// the u64 words of ShadowArgs::counters (the shadow kernels add to them; a Terrain call zeroes them and reads them back)
enum {
    HZ_SHADOW_CNT_RAYS = 0,
    HZ_SHADOW_CNT_NODES = 1, HZ_SHADOW_CNT_TRIS = 2,               // count_work: node visits, triangle tests,
    HZ_SHADOW_CNT_WAVE_NODE = 3, HZ_SHADOW_CNT_WAVE_LEAF = 4,      //   wave-level node / leaf steps
    HZ_SHADOW_CNT_TWICE = 8,                                       // count_work: rays traced twice (the fast stack overflowed)
    HZ_SHADOW_CNT_N = 16
};
int shadow_launch(const Scene *sc, const ShadowArgs &a, hipStream_t st);
int shadow_refrac_factor(const float *elevation, size_t n, double *out, hipStream_t st);
// hz_terrain_accumulate (hz_shadow.hip): one chunk of a.num_sun positions traced into scratch [num_sun][cells] (a.which = 0:
// shadow codes to a.out_u8 and, want_sw, the correction of the lit cells to a.out_f32; 1: the correction to a.out_f32), the
// chunk added to float64 accumulators in ascending order (w: device f32[k] or null = ones), the accumulators rounded once
int accum_trace_launch(const Scene *sc, const ShadowArgs &a, int want_sw, hipStream_t st);
int accum_add_launch(const uint8_t *codes, const float *vals, size_t n, int k, const float *w, double *acc_sw, double *acc_lit,
                     hipStream_t st);
int accum_final_launch(const uint8_t *mask, size_t n, float fill, const double *acc_sw, const double *acc_lit, float *out_sw,
                       float *out_lit, hipStream_t st);

// hz_viewshed.hip (hz_terrain_viewshed; device pointers; DESIGN.md section 4, clause 18): one launch of k_viewshed_refill over
// the a.num_sun observers a.suns of a chunk.  Of `a` the inputs, suns, num_sun, out_u8 (the codes u8[num_sun][cells], or null),
// count_work and counters are read.  seen_count i32[cells] (null: not wanted) takes +1 per observer that sees the cell,
// cells_seen i64[num_sun] (null: not wanted) + the cells each observer sees: the caller zeroes both, and sets the masked
// cells of seen_count to -1 after the last launch (viewshed_masked_launch).
struct ViewshedArgs {
    float target_elev, max_dist;
    int has_max, facing;                 // has_max = 0: no distance limit (max_dist is not read)
    int32_t *seen_count;
    int64_t *cells_seen;
};
int viewshed_launch(const Scene *sc, const ShadowArgs &a, const ViewshedArgs &v, hipStream_t st);
int viewshed_masked_launch(const uint8_t *mask, size_t n, int32_t *seen_count, hipStream_t st);

// hz_sight.hip (hz_terrain_sight_height; device pointers; DESIGN.md section 4, clause 19): one launch of k_sight_refill over
// the a.num_sun observers a.suns of a chunk.  Of `a` the inputs, suns, num_sun, out_f32 (the heights f32[num_sun][cells], or
// null), count_work and counters are read.  lowest f32[cells] (null: not wanted) takes the minimum of the finite results over
// the observers: the caller fills it with +inf before the first launch (sight_lowest_init_launch) and sets its masked cells
// to NaN after the last (sight_masked_launch).  cells_reached i64[num_sun] (null: not wanted) += the cells with a finite
// result per observer: the caller zeroes it.  heights: the checked table (hz_terrain_sight_height), device f32[num_heights].
struct SightArgs {
    const float *heights;
    int num_heights;
    float max_dist;
    int has_max;                         // 0: no distance limit (max_dist is not read)
    float *lowest;
    int64_t *cells_reached;
};
int sight_launch(const Scene *sc, const ShadowArgs &a, const SightArgs &v, hipStream_t st);
int sight_lowest_init_launch(size_t n, float *lowest, hipStream_t st);
int sight_masked_launch(const uint8_t *mask, size_t n, float *lowest, hipStream_t st);

// hz_subgrid.hip (hz_terrain_sw_dir_cor_coarse; device pointers): n u32[dim_0 / p0][dim_1 / p1] = unmasked cells per coarse
// cell; one chunk of k positions of accumulate's scratch (codes and / or vals, [k][cells]) reduced to block means
// f_cor / lit f32[k][gy][gx] (null: not wanted; f_cor needs vals, lit needs codes), coarse cells without a cell = fill
int coarse_count_launch(const uint8_t *mask, int dim_0, int dim_1, int p0, int p1, unsigned *n, hipStream_t st);
int coarse_reduce_launch(const uint8_t *codes, const float *vals, const uint8_t *mask, const unsigned *n, int dim_0, int dim_1,
                         int p0, int p1, int k, float fill, float *f_cor, float *lit, hipStream_t st);

// hz_horisun.hip (hz_horizon_terrain_run; device pointers): one launch of k_horisun over num_sun positions, one lane per cell.
// Per-position maps out_u8 / out_f32 [num_sun][cells] (null: not wanted).  Sums (sum_sw / sum_lit f32[cells], null: not
// wanted): the lane's float64 sums start at 0 (first) or at acc_sw / acc_lit f64[cells], take w[s] * value in ascending s and
// go back to acc_* or, in the last launch of a call, rounded once to sum_* (masked cells: fill)
struct HorisunArgs {
    const float *hori;                   // f32[cells][azim_num]; the q16 launches read it as u16[cells][azim_num]
    const float *vert;                   // f32[cells][3]: the vertices of the inner domain
    const float *vec_tilt, *vec_norm, *vec_north, *surf_enl_fac;
    const uint8_t *mask;
    size_t cells;
    int azim_num;
    const float *suns, *weights;         // f32[num_sun][3], f32[num_sun] or null = ones
    int num_sun;
    float fill, dot_prod_min;
    uint8_t *out_u8; float *out_f32;
    double *acc_sw, *acc_lit;
    float *sum_sw, *sum_lit;
    int first, last;
    const double *refrac_fac;            // null: no refraction; else f64[cells], shadow_refrac_factor() (clause 13)
};
// q16: a.hori addresses 16-bit codes u16[cells][azim_num] (hz_q16.h, clause 15) instead of float32
int horisun_launch(const HorisunArgs &a, unsigned blocks, hipStream_t st, bool q16 = false);

// hz_planes.hip: the azimuth-major horizon layout planes[k][cell] (clause 11; device pointers).
// Both transpositions move the `cells` x azim_num matrix `hori` (cell-major, contiguous) as 32-bit words; on the plane
// side cell c of `hori` is element k * plane_stride + cell0 + c, so a chunk of rows goes to its place in every plane of
// a larger domain (cell0 + cells <= plane_stride).
int hori_to_planes_launch(const float *hori, size_t cells, int azim_num, float *planes, size_t plane_stride, size_t cell0,
                          hipStream_t st);
int planes_to_hori_launch(const float *planes, size_t plane_stride, size_t cell0, size_t cells, int azim_num, float *hori,
                          hipStream_t st);
// horisun_launch for a horizon stored as planes: a.hori = planes f32[azim_num][plane_stride] (k_horisun_planes)
// (q16: planes of 16-bit codes u16[azim_num][plane_stride])
int horisun_planes_launch(const HorisunArgs &a, size_t plane_stride, unsigned blocks, hipStream_t st, bool q16 = false);

// hz_q16.hip: the 16-bit horizon code (clause 15; device pointers).  dst[i] = encode(src[i]) /
// decode(src[i]) for n elements; src and dst need the alignment of their element type only.  hori_quantise_planes_launch is
// hori_to_planes_launch with encode applied on the way out: planes_q[k * plane_stride + cell0 + c] = encode(hori[c][k]).
int hori_quantise_launch(const float *src, size_t n, uint16_t *dst, hipStream_t st);
int hori_dequantise_launch(const uint16_t *src, size_t n, float *dst, hipStream_t st);
int hori_quantise_planes_launch(const float *hori, size_t cells, int azim_num, uint16_t *planes_q, size_t plane_stride,
                                size_t cell0, hipStream_t st);

// hz_horidist.hip: the distance to the horizon of a gridded horizon (clause 16; device pointers).  One
// launch over the rows [row_begin, row_end) of the inner domain.  vec_norm, vec_north and mask are indexed by the cell of the
// inner domain, the scene's vertices by offset_0 / offset_1.  Cell c (0 = the first cell of row_begin) and azimuth k of the
// horizon is element c * azim_num + k of `hori`, or (planes) element k * hori_stride + hori_cell0 + c; `dist` likewise with
// its own stride and first cell.  q16: `hori` holds 16-bit codes (hz_q16.h) instead of float32.  block_w: cells of a wave's
// block in a row (8: the 8 x 8 block of k_horizon; 16, 32, 64: flatter blocks).  counters: device u64[2], [0] += distance
// rays, [1] += cells with mask == 1.
struct HoridistArgs {
    const float *vec_norm, *vec_north;
    const uint8_t *mask;
    const void *hori;
    float *dist;
    int q16, planes;
    size_t hori_stride, hori_cell0, dist_stride, dist_cell0;
    int offset_0, offset_1, dim_in_1, row_begin, row_end;
    int azim_num, elev_num;
    float hori_acc, up, dist_m, ray_org_elev;      // radians / metres
    const float *azim_sin, *azim_cos, *elev_ang, *elev_sin, *elev_cos;   // device tables
    int block_w;
    unsigned long long *counters;
};
int horidist_launch(const Scene *sc, const HoridistArgs &a, hipStream_t st);
extern std::atomic<int> g_horidist_traversal;   // "horidist_traversal" (hz_debug_set): 0 hz_closest's slot order, 1 (default, also < 0) the children of a node front to back
extern std::atomic<int> g_horidist_block_w;  // "horidist_block_w" (hz_debug_set): cells per row of a wave's block in the planes launches (default 8)

// hz_panorama.hip (hz_terrain_panorama; device pointers; DESIGN.md section 4, clause 20): one launch of k_panorama over the
// num_obs observers of a chunk, one wave per 8 x 8 tile of an observer's elev_num x azim_num image (tiles * num_obs < 2^31:
// hz_panorama_plan.h).  vec_north / vec_norm f32[num_obs][3], or both null = the planar frame.  The outputs start at the
// chunk's first observer: dist f32[num_obs][elev_num][azim_num], point f32[num_obs][elev_num][azim_num][3], hits
// i64[num_obs] += the pixels with a hit (the caller zeroes it); null: not wanted.
struct PanoramaArgs {
    const float *observers, *vec_north, *vec_norm;
    int num_obs;
    const float *azim_sin, *azim_cos, *elev_sin, *elev_cos;      // device tables
    int azim_num, elev_num;
    float max_dist;
    float *dist, *point;
    int64_t *hits;
};
int panorama_launch(const Scene *sc, const PanoramaArgs &a, hipStream_t st);
extern std::atomic<int> g_panorama_traversal;   // "panorama_traversal" (hz_debug_set): 0 hz_closest's slot order, 1 (default, also < 0) the children of a node front to back
extern std::atomic<int> g_panorama_budget;      // "panorama_budget" (hz_debug_set): > 0 bytes of staged output per chunk of hz_terrain_panorama (default 0: HZ_PANORAMA_BUDGET)

// hz_cast.hip (hz_terrain_cast; device pointers; DESIGN.md section 4, clause 21): one launch over the num_rays rays of a chunk
// (at most HZ_CAST_MAX_CHUNK, hz_cast_plan.h).  origins f32[num_rays][3]; ends f32[num_rays][3]: unit directions of length
// max_dist, or (segments) the targets the rays end at.  perm u32[num_rays] or null: the launch traces the rays in the order
// perm[0], perm[1], ... (a permutation of 0 ... num_rays - 1).  The outputs start at the chunk's first ray: occluded
// u8[num_rays], dist f32[num_rays], point f32[num_rays][3]; null: not wanted.  dist or point: k_cast_closest; occluded alone:
// k_cast_any (count_work: its counting instantiation).  counters[HZ_SHADOW_CNT_RAYS] += the rays traced.
struct CastArgs {
    const float *origins, *ends;
    const uint32_t *perm;
    unsigned num_rays;
    int segments;
    float max_dist;
    uint8_t *occluded;
    float *dist, *point;
    unsigned long long *counters;
    int count_work;
};
int cast_launch(const Scene *sc, const CastArgs &a, hipStream_t st);
// keys[i] = the sort key of ray i of the chunk (origin's Morton code over the scene's box, direction code), vals[i] = i
int cast_keys_launch(const Scene *sc, const float *origins, const float *ends, int segments, unsigned num_rays, uint32_t *keys,
                     uint32_t *vals, hipStream_t st);
#define HZ_CAST_FAST_CAP_DEFAULT 19             // entries of k_cast_any's fast stack (k_shadow_refill's value)
extern std::atomic<int> g_cast_budget;          // "cast_budget" (hz_debug_set): > 0 bytes of staging and sort memory per chunk of hz_terrain_cast (default 0: HZ_CAST_BUDGET)
extern std::atomic<int> g_cast_sort_only;       // "cast_sort_only" (hz_debug_set): 1 = hz_terrain_cast stops after the keys and the sort of every chunk and writes no output (scripts/cast_perf.py times them alone)
extern std::atomic<int> g_cast_fast_cap;        // "cast_fast_cap" (hz_debug_set): entries of k_cast_any's fast stack (default HZ_CAST_FAST_CAP_DEFAULT; 0: level stack only)

// hz_horisun_coarse.hip (hz_horizon_terrain_sw_dir_cor_coarse; device pointers): the plan of the fused kernel for chunks of
// up to `chunk` positions (hz_horisun_coarse_plan.h; plan->fallback = 1: the shape, the "horisun_coarse_route" knob or the layout's default asks
// for the two-pass route), and one launch of k_horisun_coarse over the a.num_sun <= chunk positions of a chunk: block means
// f_cor / lit f32[a.num_sun][gy][gx] (null: not wanted; as the plan was made) from a.hori (planes: f32[azim_num][plane_stride]),
// n = coarse_count_launch's counts.  Of `a` the inputs, cells, azim_num, suns, num_sun, fill and dot_prod_min are read.
struct HorisunCoarsePlan;
int horisun_coarse_plan_for(int dim_0, int dim_1, int p0, int p1, int chunk, bool planes, bool codes, bool vals,
                            HorisunCoarsePlan *plan);
int horisun_coarse_launch(const HorisunArgs &a, bool planes, size_t plane_stride, const HorisunCoarsePlan &plan,
                          const unsigned *n, int dim_1, int p0, int p1, float *f_cor, float *lit, hipStream_t st);

// hz_suntimes.hip (hz_horizon_terrain_sun_times; device pointers; DESIGN.md section 4, clause 14): one launch of k_suntimes over
// num_sun positions of a sun track, one lane per cell.  times f64[num_sun] = the times of those positions, t_before = the time of
// the position before the launch's first (not read in the first launch).  The per-cell state starts empty (first) or comes
// from state f64[5][cells] (rise, set, dur, open, g_prev) and state_n i32[cells] (2 * n + lit_prev), and goes back there or,
// in the last launch of a call, to the maps sunrise / sunset / duration f32[cells] and intervals i32[cells] (null: not wanted;
// masked cells: fill, -1).  A call of one launch (first and last) needs no state.  planes: hori = f32[azim_num][stride]
struct SuntimesArgs {
    const float *hori;                   // f32[cells][azim_num], or planes; the q16 launch reads 16-bit codes there
    size_t stride;                       // planes: words from one azimuth's plane to the next
    const float *vert;                   // f32[cells][3]: the vertices of the inner domain
    const float *vec_tilt, *vec_norm, *vec_north;
    const uint8_t *mask;
    size_t cells;
    int azim_num;
    const float *suns;                   // f32[num_sun][3]
    const double *times;                 // f64[num_sun]
    double t_before;
    int num_sun;
    float fill;
    int first, last;
    const double *refrac_fac;            // null: no refraction; else f64[cells] (clause 13)
    double *state; int32_t *state_n;
    float *sunrise, *sunset, *duration; int32_t *intervals;
};
size_t suntimes_state_bytes(size_t cells);
// q16: a.hori addresses 16-bit codes (clause 15) in the layout `planes` names
int suntimes_launch(const SuntimesArgs &a, bool planes, unsigned blocks, hipStream_t st, bool q16 = false);

// hz_sort.hip: hand-written stable LSD radix sort (pairs) and exclusive scan, uint32
size_t sort_temp_elems(size_t n);
size_t scan_temp_elems(size_t n);
int radix_sort_pairs_u32(uint32_t *keys_a, uint32_t *vals_a, uint32_t *keys_b, uint32_t *vals_b, size_t n,
                         uint32_t *temp, hipStream_t st, int passes = 4);
int exclusive_scan_u32(const uint32_t *in, uint32_t *out, size_t n, uint32_t *temp, hipStream_t st);

// hz_coast.hip: nearest coastline vertex of every water cell (float64)
#define HZ_COAST_LEAF 8                  // sorted vertices per leaf
#define HZ_COAST_CNT_N 2                 // u64 counters: [0] water cells queried, [1] lanes that hit the iteration bound
struct CoastIndex {
    uint32_t n_pts = 0, n_leaf = 0, n_leaf_pad = 1;
    size_t off_counters = 0, off_sorted = 0, off_nodes = 0, off_bbox = 0, off_sort = 0;   // layout of the scratch block
    unsigned long long *counters = nullptr;
    const double *sorted = nullptr;      // f64[n_leaf * HZ_COAST_LEAF][3], Morton order
    const void *nodes = nullptr;         // heap-ordered boxes, 2 * n_leaf_pad of 48 bytes
};
// bytes of device scratch the index of num_pts vertices needs (fills the sizes and offsets of *ix)
size_t coast_scratch_bytes(size_t num_pts, CoastIndex *ix);
int coast_index_build(const double *pts, void *scratch, CoastIndex *ix, hipStream_t st);
// any_hit = 0: dist f64[len_0][len_1]; 1: mask_buffer u8[len_0][len_1] = (distance > thr), thr2 = the largest double whose
// correctly rounded square root is <= thr.  All pointers device memory.
int coast_query_launch(const CoastIndex &ix, const double *x, const double *y, const double *z, const uint8_t *mask_land,
                       int len_0, int len_1, int any_hit, double thr, double thr2, double *dist, uint8_t *mask_buffer,
                       hipStream_t st);

// hz_bench.hip: machine calibration kernels (current device)
int bench_valu_peak(int packed, int waves_per_simd, double *winst_per_s_per_simd, double *clock_ghz, int *simds);
int bench_copy_peak(size_t bytes, double *gbs);
int bench_inst_rate(int op, double *cycles_per_inst);

// hz_prep.hip (device pointers)
int prep_slope(int which, const float *x, const float *y, const float *z, int len_0, int len_1,
               const float *rot_mat, int output_rot, float *vec_tilt, hipStream_t st);
int prep_lonlat2ecef(int ellps, const double *lon, const double *lat, const float *h, size_t n, double *X,
                     double *Y, double *Z, hipStream_t st);
int prep_ecef2enu(int ellps, double lon_or, double lat_or, const double *X, const double *Y, const double *Z,
                  size_t n, float *xe, float *ye, float *ze, hipStream_t st);
int prep_ecef2enu_vector(int ellps, double lon_or, double lat_or, const float *v, size_t n, float *o, hipStream_t st);
int prep_surf_norm(const double *lon, const double *lat, size_t n, float *o, hipStream_t st);
int prep_wgs2swiss(const double *lon, const double *lat, const float *h_wgs, size_t n, double *e, double *no, float *h_ch,
                   hipStream_t st);
int prep_swiss2wgs(const double *e, const double *no, const float *h_ch, size_t n, double *lon, double *lat, float *h_wgs,
                   hipStream_t st);
int prep_pack_vertices(const float *x, const float *y, const float *z, size_t n, size_t n_total, float *out,
                       hipStream_t st);
int prep_north_dir(int ellps, const double *X, const double *Y, const double *Z, const float *vn, size_t n,
                   float *o, hipStream_t st);

}  // namespace hz
