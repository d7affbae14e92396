// hz_api_sun.hip -- the drivers behind the C ABI (include/horayzon_hip.h) that answer for lists of sun positions:
// Terrain (hz_terrain_*: rays against the scene, restating CppTerrain, shadow_comp.cpp:304-605) and HorizonTerrain
// (hz_horizon_terrain_*: look-ups in a stored horizon).
//
// Ten calls walk their positions in chunks: terrain_run, hz_terrain_accumulate, hz_terrain_sw_dir_cor_coarse,
// hz_terrain_viewshed, hz_terrain_sight_height, hz_terrain_panorama, hz_terrain_cast, hz_horizon_terrain_run, hz_horizon_terrain_sw_dir_cor_coarse and hz_horizon_terrain_sun_times.  Each reads as checks, plan,
// allocations, one chunk loop with the launches, finish; what they share -- device, lock, stream, timers, the scratch tally,
// staged inputs, staged outputs -- is SunCall, ChunkFeed (an input that goes up chunk by chunk) and ChunkOut (an output that
// comes down chunk by chunk) below; the seven Terrain calls also share their end, terrain_finish.
#include "hz_internal.h"
#include "hz_horisun_plan.h"
#include "hz_horisun_coarse_plan.h"
#include "hz_panorama_plan.h"
#include "hz_cast_plan.h"
#include <cmath>
#include <vector>
#include <mutex>

namespace hz {

struct Terrain {
    int device = 0;
    Scene *scene = nullptr;
    bool owns_scene = false;
    int offset_0 = 0, offset_1 = 0, dim_in_0 = 0, dim_in_1 = 0;
    void *tilt = nullptr, *norm = nullptr, *enl = nullptr, *elev = nullptr, *mask = nullptr;
    double *refrac_fac = nullptr;             // refrac_cor: per cell the pressure / temperature factor of the refraction formula (hz_shadow.hip)
    bool own_tilt = false, own_norm = false, own_enl = false, own_elev = false, own_mask = false;
    float fill = 0, ang_max = 89.0f;
    int refrac = 0;
    int count_work = 0;                       // hz_terrain_count_work
    unsigned long long *counters = nullptr;   // device u64[HZ_SHADOW_CNT_N]
    float *sun_dev = nullptr;                 // staging memory of host sun positions, kept with the handle (grown on demand: the
    size_t sun_cap = 0;                       //   drop-in API is called once per time step -- no hipMalloc / hipFree per call)
    hipStream_t stream = nullptr;
    bool initialised = false;
};

static void terrain_release_arrays(Terrain *t) {
    (void)hipSetDevice(t->device);
    if (t->own_tilt && t->tilt) (void)hipFree(t->tilt);
    if (t->own_norm && t->norm) (void)hipFree(t->norm);
    if (t->own_enl && t->enl) (void)hipFree(t->enl);
    if (t->own_elev && t->elev) (void)hipFree(t->elev);
    if (t->own_mask && t->mask) (void)hipFree(t->mask);
    if (t->refrac_fac) { (void)hipFree(t->refrac_fac); t->refrac_fac = nullptr; }
    t->tilt = t->norm = t->enl = t->elev = t->mask = nullptr;
    t->own_tilt = t->own_norm = t->own_enl = t->own_elev = t->own_mask = false;
    // the counters live on the terrain's current GPU; a re-initialisation may move the terrain to another one
    if (t->counters) { (void)hipFree(t->counters); t->counters = nullptr; }
    if (t->sun_dev) { (void)hipFree(t->sun_dev); t->sun_dev = nullptr; t->sun_cap = 0; }
    if (t->owns_scene && t->scene) scene_free(t->scene);
    t->scene = nullptr; t->owns_scene = false; t->initialised = false;
}

// persistent device copy (Terrain keeps its inputs in HBM instead of raw host pointers,
// shadow_comp.cpp:332-346)
static int persist(const void *src, size_t bytes, hipStream_t st, void **dst, bool *own) {
    if (is_device_ptr(src)) { *dst = const_cast<void *>(src); *own = false; return HZ_OK; }
    HZ_HIP(hipMalloc(dst, bytes ? bytes : 16));
    *own = true;
    HZ_HIP(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st));
    return HZ_OK;
}

struct HorizonTerrain {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex run_mu;                        // calls on one handle run one after the other (they share the stream)
    const float *hori = nullptr;              // device; borrowed when the caller gave a device pointer
    bool own_hori = false;
    bool planes = false;                      // hori is f32[azim_num][cells] (hz_horizon_terrain_initialise_planes)
    bool q16 = false;                         // hori addresses 16-bit codes in that layout (hz_horizon_terrain_initialise_q16)
    int azim_num = 0, dim_in_0 = 0, dim_in_1 = 0;
    void *vert = nullptr, *tilt = nullptr, *norm = nullptr, *north = nullptr, *enl = nullptr, *mask = nullptr;   // owned copies
    float fill = 0, ang_max = 89.0f;
    double *refrac_fac = nullptr;             // hz_horizon_terrain_refraction: per cell the factor of the refraction formula (k_refrac_factor), or null = off
    bool initialised = false;
};

static void horisun_release(HorizonTerrain *t) {
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->own_hori && t->hori) (void)hipFree(const_cast<float *>(t->hori));
    for (void **q : {&t->vert, &t->tilt, &t->norm, &t->north, &t->enl, &t->mask}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    if (t->refrac_fac) { (void)hipFree(t->refrac_fac); t->refrac_fac = nullptr; }
    t->hori = nullptr; t->own_hori = false; t->initialised = false;
}

// device copy of `bytes` bytes of host or device memory (the object keeps no pointer of the caller's besides a device `hori`)
static int horisun_copy(const void *src, size_t bytes, hipStream_t st, void **dst) {
    HZ_HIP(hipMalloc(dst, bytes ? bytes : 16));
    HZ_HIP(hipMemcpyAsync(*dst, src, bytes, is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    return HZ_OK;
}

// ---------------------------------------------------------------------------------------
// the scaffold of a call that walks a list of sun positions in chunks
// ---------------------------------------------------------------------------------------
#define HZ_SHADOW_MAX_POS 32768     // positions of one launch of the shadow kernels: grid.y

// One input of such a call: `per` elements of T per position (positions: 3 floats, weights: 1 float, times: 1 double) in host
// or device memory, or none (null).  at() gives the device address of a chunk: the caller's own memory, or the feed's slice of
// the staging memory after the chunk went up into it (stream order keeps a slice intact until the launches before it are done).
template <typename T>
struct ChunkFeed {
    const T *src;
    size_t per;
    bool on_dev;
    T *stage = nullptr;                       // device memory for one chunk (SunCall::stage, or the caller's own)
    ChunkFeed(const T *src_, size_t per_) : src(src_), per(per_), on_dev(src_ && is_device_ptr(src_)) {}
    bool staged() const { return src && !on_dev; }
    size_t position_bytes() const { return per * sizeof(T); }
    int at(int s0, int kc, hipStream_t st, const T **dev) const {
        *dev = src ? src + per * (size_t)s0 : nullptr;
        if (!staged()) return HZ_OK;
        HZ_HIP(hipMemcpyAsync(stage, *dev, (size_t)kc * position_bytes(), hipMemcpyHostToDevice, st));
        *dev = stage;
        return HZ_OK;
    }
};

// One output of such a call that goes out chunk by chunk, ChunkFeed's mirror image: `per` elements of T per position in host
// or device memory, or none (null).  at() gives the device address a chunk is written to: the caller's own memory, or the one
// chunk of device memory a host output is staged in (SunCall::bind), which out() copies to the host after the chunk's
// launches (stream order keeps it intact until then, and the next chunk's launches wait for the copy).
template <typename T>
struct ChunkOut {
    T *dst;
    size_t per;
    bool on_dev;
    DevBuf chunk;                             // device memory for one chunk of a host output (SunCall::bind)
    ChunkOut(T *dst_, size_t per_) : dst(dst_), per(per_), on_dev(dst_ && is_device_ptr(dst_)) {}
    bool staged() const { return dst && !on_dev; }
    T *at(size_t s0) const { return staged() ? static_cast<T *>(chunk.p) : dst ? dst + per * s0 : nullptr; }
    int out(size_t s0, int kc, hipStream_t st) const {
        if (!staged()) return HZ_OK;
        HZ_HIP(hipMemcpyAsync(dst + per * s0, chunk.p, (size_t)kc * per * sizeof(T), hipMemcpyDeviceToHost, st));
        return HZ_OK;
    }
};

// The common start and end of such a call.  `scratch` adds up the device memory the call allocates besides the caller's
// buffers: what the calls that report hz_stats.scratch_bytes report.
struct SunCall {
    std::unique_lock<std::mutex> lock;        // held to the end of the call
    hipStream_t st = nullptr;
    Timer t_total;
    size_t scratch = 0;
    DevBuf staging;
    Event launches_begin, launches_end;
    float ms = 0.0f;                          // GPU time between the two

    // `mu`: the scene's run_mu for a Terrain (its launches share the scene's stream), the handle's own for a HorizonTerrain
    int start(int device, std::mutex &mu, hipStream_t stream) {
        HZ_HIP(hipSetDevice(device));
        lock = std::unique_lock<std::mutex>(mu);
        st = stream;
        t_total.start();
        return HZ_OK;
    }
    int alloc(DevBuf &b, size_t bytes) {
        HZ_HIP(b.alloc(bytes));
        scratch += bytes;
        return HZ_OK;
    }
    // an output of n elements (null: not wanted); a host output is staged on the device, which counts as scratch where the call says so
    template <typename T>
    int bind(DevOut<T> &o, T *dst, size_t n, bool counts_as_scratch) {
        const int rc = o.bind(dst, dst ? n : 0);
        if (!rc && o.owned && counts_as_scratch) scratch += n * sizeof(T);
        return rc;
    }
    // an output that goes out in chunks of up to k positions: a host output gets one chunk of device memory, which counts as scratch
    template <typename T>
    int bind(ChunkOut<T> &o, int k) {
        return o.staged() ? alloc(o.chunk, (size_t)k * o.per * sizeof(T)) : HZ_OK;
    }
    // staging memory for k positions of every feed, in the order given -- allocated only if one of them reads host memory
    template <typename... F>
    int stage(int k, F &...feeds) {
        if (!(feeds.staged() || ...)) return HZ_OK;
        const int rc = alloc(staging, (size_t)k * (feeds.position_bytes() + ...));
        if (rc) return rc;
        char *p = static_cast<char *>(staging.p);
        ((feeds.stage = reinterpret_cast<decltype(feeds.stage)>(p), p += (size_t)k * feeds.position_bytes()), ...);
        return HZ_OK;
    }
    int begin() { return launches_begin.record(st); }
    int end() {                               // waits for the launches
        const int rc = launches_end.record(st);
        if (rc) return rc;
        HZ_HIP(hipEventSynchronize(launches_end.e));
        ms = launches_begin.ms_until(launches_end);
        return HZ_OK;
    }
    // the staged outputs go to the host; the times of the call are added to `stats`
    template <typename... O>
    int finish(hz_stats *stats, O &...outs) {
        Timer t_d2h; t_d2h.start();
        int rc = HZ_OK;
        if (((rc = outs.finish(st)) || ...)) return rc;
        HZ_HIP(hipStreamSynchronize(st));
        if (stats) {
            stats->t_kernel_s += (double)ms * 1e-3;
            stats->t_d2h_s += t_d2h.stop();
            stats->t_total_s += t_total.stop();
        }
        return HZ_OK;
    }
};

static int check_distinct_outputs(const void *const *outs, int n) {
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (outs[i] && outs[i] == outs[j]) return set_error(HZ_ERR_ARG, "the outputs must be different arrays");
    return HZ_OK;
}

static int check_pixel_per_gc(int p0, int p1, int dim_0, int dim_1) {
    if (p0 < 1 || p1 < 1 || p0 > dim_0 || p1 > dim_1 || dim_0 % p0 || dim_1 % p1)
        return set_error(HZ_ERR_ARG, "'pixel_per_gc' (%d, %d) must be positive and divide the inner domain (%d, %d)", p0, p1, dim_0, dim_1);
    return HZ_OK;
}

// The scratch maps one chunk of k positions is traced into before it is reduced: 1 B shadow code and / or 4 B correction per
// cell and position.
struct ChunkMaps {
    DevBuf codes, vals;
    int alloc(SunCall &call, int k, size_t nc, bool want_lit, bool want_sw) {
        int rc = HZ_OK;
        if (want_lit && (rc = call.alloc(codes, (size_t)k * nc))) return rc;
        if (want_sw && (rc = call.alloc(vals, (size_t)k * nc * 4))) return rc;
        return HZ_OK;
    }
    uint8_t *u8() const { return static_cast<uint8_t *>(codes.p); }
    float *f32() const { return static_cast<float *>(vals.p); }
};

// The float64 sums of accumulate between the launches of a call: one map per wanted sum, in one allocation.
struct SumMaps {
    DevBuf buf;
    size_t bytes = 0;
    double *sw = nullptr, *lit = nullptr;
    int alloc(SunCall &call, size_t nc, bool want_sw, bool want_lit) {
        bytes = ((want_sw ? 1 : 0) + (want_lit ? 1 : 0)) * nc * sizeof(double);
        if (!bytes) return HZ_OK;
        const int rc = call.alloc(buf, bytes);
        if (rc) return rc;
        sw = want_sw ? static_cast<double *>(buf.p) : nullptr;
        lit = want_lit ? static_cast<double *>(buf.p) + (want_sw ? nc : 0) : nullptr;
        return HZ_OK;
    }
};

// what HorisunArgs and SuntimesArgs share: the handle's arrays
template <typename Args>
static void horisun_inputs(const HorizonTerrain *t, Args &a) {
    a.hori = t->hori; a.vert = (const float *)t->vert;
    a.vec_tilt = (const float *)t->tilt; a.vec_norm = (const float *)t->norm; a.vec_north = (const float *)t->north;
    a.mask = (const uint8_t *)t->mask;
    a.cells = (size_t)t->dim_in_0 * (size_t)t->dim_in_1; a.azim_num = t->azim_num;
    a.fill = t->fill;
    a.refrac_fac = t->refrac_fac;
}

// The end of every Terrain call: the launches are waited for and the counters read back, the outputs staged whole (`outs`) go
// to the host, and `stats` gets the times and what every Terrain call reports besides them -- with `report_scratch`, also
// the call's tally as scratch_bytes.
template <typename... O>
static int terrain_finish(const Terrain *t, SunCall &call, hz_stats *stats, bool report_scratch, O &...outs) {
    unsigned long long cnt[HZ_SHADOW_CNT_N];
    int rc;
    if ((rc = call.end())) return rc;
    HZ_HIP(hipMemcpyAsync(cnt, t->counters, HZ_SHADOW_CNT_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, call.st));
    HZ_HIP(hipStreamSynchronize(call.st));
    if ((rc = call.finish(stats, outs...)) || !stats) return rc;
    stats->num_rays += cnt[HZ_SHADOW_CNT_RAYS];
    stats->nodes_visited += cnt[HZ_SHADOW_CNT_NODES]; stats->tris_tested += cnt[HZ_SHADOW_CNT_TRIS];
    stats->wave_node_iters += cnt[HZ_SHADOW_CNT_WAVE_NODE]; stats->wave_leaf_iters += cnt[HZ_SHADOW_CNT_WAVE_LEAF];
    stats->bvh_height = t->scene->hdr.height; stats->scene_bytes = t->scene->hdr.total_bytes;
    if (report_scratch) stats->scratch_bytes = call.scratch;
    return HZ_OK;
}

// 'max_dist' of the line-of-sight calls (ViewshedArgs, SightArgs): anything but a finite distance above 0 is "no limit"
template <typename A>
static void set_max_dist(A &v, float max_dist) {
    v.has_max = (max_dist > 0.0f && std::isfinite(max_dist)) ? 1 : 0;
    v.max_dist = v.has_max ? max_dist : 0.0f;
}

}  // namespace hz

using namespace hz;

extern "C" {

// ---------------------------------------------------------------------------------------
// Terrain (shadow_comp.h:4-39)
// ---------------------------------------------------------------------------------------

int hz_terrain_create(int device, hz_terrain **terrain) {
    if (!terrain) return set_error(HZ_ERR_ARG, "terrain is NULL");
    int rc = select_device(device);
    if (rc) return rc;
    Terrain *t = new Terrain();
    t->device = device;
    *terrain = reinterpret_cast<hz_terrain *>(t);
    return HZ_OK;
}

static int terrain_init_common(Terrain *t, int offset_0, int offset_1, const float *vec_tilt,
                               const float *vec_norm, int dim_in_0, int dim_in_1, const float *surf_enl_fac,
                               const float *elevation, const uint8_t *mask, float sw_dir_cor_fill,
                               float ang_max, int refrac_cor) {
    const Scene *sc = t->scene;
    if (!vec_tilt || !vec_norm || !surf_enl_fac || !elevation || !mask) return set_error(HZ_ERR_ARG, "NULL input array");
    if (dim_in_0 <= 0 || dim_in_1 <= 0 || offset_0 < 0 || offset_1 < 0 ||
        offset_0 + dim_in_0 > sc->hdr.d0 || offset_1 + dim_in_1 > sc->hdr.d1)
        return set_error(HZ_ERR_ARG, "inconsistency between input arguments 'dem_dim_0', 'dem_dim_1', 'offset_0', 'offset_1' and 'vec_norm'");
    if (ang_max < 85.0f || ang_max > 89.99f) return set_error(HZ_ERR_ARG, "'ang_max' must be in the range [85.0, 89.99]");
    std::lock_guard<std::mutex> run_lock(sc->run_mu);
    hipStream_t st = sc->stream;
    const size_t nc = (size_t)dim_in_0 * dim_in_1;
    int rc;
    if ((rc = persist(vec_tilt, nc * 12, st, &t->tilt, &t->own_tilt))) return rc;
    if ((rc = persist(vec_norm, nc * 12, st, &t->norm, &t->own_norm))) return rc;
    if ((rc = persist(surf_enl_fac, nc * 4, st, &t->enl, &t->own_enl))) return rc;
    if ((rc = persist(elevation, nc * 4, st, &t->elev, &t->own_elev))) return rc;
    if ((rc = persist(mask, nc, st, &t->mask, &t->own_mask))) return rc;
    if (!t->counters) HZ_HIP(hipMalloc((void **)&t->counters, HZ_SHADOW_CNT_N * sizeof(unsigned long long)));
    if (refrac_cor) {
        // what the refraction formula needs from the cell's elevation alone -- temperature, pressure (a powf), two float64
        // divisions -- is the same for every sun position: formed once here (shadow_comp.cpp:438-441, :151-157)
        HZ_HIP(hipMalloc((void **)&t->refrac_fac, nc * sizeof(double)));
        if ((rc = shadow_refrac_factor((const float *)t->elev, nc, t->refrac_fac, st))) return rc;
    }
    HZ_HIP(hipStreamSynchronize(st));
    t->offset_0 = offset_0; t->offset_1 = offset_1; t->dim_in_0 = dim_in_0; t->dim_in_1 = dim_in_1;
    t->fill = sw_dir_cor_fill; t->ang_max = ang_max; t->refrac = refrac_cor ? 1 : 0;
    t->stream = st;
    t->initialised = true;
    return HZ_OK;
}

int hz_terrain_initialise(hz_terrain *terrain, const float *vert_grid, int dem_dim_0, int dem_dim_1,
                          int offset_0, int offset_1, const float *vec_tilt, const float *vec_norm,
                          int dim_in_0, int dim_in_1, const float *surf_enl_fac, const float *elevation,
                          const uint8_t *mask, const char *geom_type, float sw_dir_cor_fill, float ang_max,
                          int refrac_cor, hz_stats *stats) {
    if (!terrain) return set_error(HZ_ERR_ARG, "terrain is NULL");
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    terrain_release_arrays(t);
    HZ_HIP(hipSetDevice(t->device));
    hz_scene *scene = nullptr;
    // no simplified outer TIN in the shadow scene: shadow_comp.cpp:198-298
    int rc = hz_scene_create(vert_grid, dem_dim_0, dem_dim_1, geom_type, nullptr, 0, nullptr, 0, t->device,
                             &scene, stats);
    if (rc) return rc;
    t->scene = reinterpret_cast<Scene *>(scene);
    t->owns_scene = true;
    rc = terrain_init_common(t, offset_0, offset_1, vec_tilt, vec_norm, dim_in_0, dim_in_1, surf_enl_fac,
                             elevation, mask, sw_dir_cor_fill, ang_max, refrac_cor);
    if (rc) terrain_release_arrays(t);
    return rc;
}

int hz_terrain_initialise_scene(hz_terrain *terrain, const hz_scene *scene, int offset_0, int offset_1,
                                const float *vec_tilt, const float *vec_norm, int dim_in_0, int dim_in_1,
                                const float *surf_enl_fac, const float *elevation, const uint8_t *mask,
                                float sw_dir_cor_fill, float ang_max, int refrac_cor) {
    if (!terrain || !scene) return set_error(HZ_ERR_ARG, "terrain / scene is NULL");
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    terrain_release_arrays(t);
    t->scene = const_cast<Scene *>(reinterpret_cast<const Scene *>(scene));
    t->owns_scene = false;
    // the terrain lives on the scene's GPU: its per-cell arrays are allocated there and its kernels run on the
    // scene's stream (a Terrain created for another ordinal follows the scene)
    t->device = t->scene->device;
    HZ_HIP(hipSetDevice(t->device));
    int rc = terrain_init_common(t, offset_0, offset_1, vec_tilt, vec_norm, dim_in_0, dim_in_1, surf_enl_fac,
                                 elevation, mask, sw_dir_cor_fill, ang_max, refrac_cor);
    if (rc) terrain_release_arrays(t);
    return rc;
}

// the launch arguments every shadow / sw_dir_cor / accumulate launch of the terrain shares
static ShadowArgs terrain_args(const Terrain *t, int which) {
    ShadowArgs a;
    a.vec_tilt = (const float *)t->tilt; a.vec_norm = (const float *)t->norm;
    a.surf_enl_fac = (const float *)t->enl; a.elevation = (const float *)t->elev; a.mask = (const uint8_t *)t->mask;
    a.offset_0 = t->offset_0; a.offset_1 = t->offset_1; a.dim_in_0 = t->dim_in_0; a.dim_in_1 = t->dim_in_1;
    a.sw_dir_cor_fill = t->fill;
    a.dot_prod_min = cosf(deg2rad_f(t->ang_max));            // shadow_comp.cpp:498
    a.refrac_cor = t->refrac; a.refrac_fac = t->refrac_fac; a.which = which; a.top_nodes = -1; a.counters = t->counters;
    a.count_work = t->count_work;
    return a;
}

// a Terrain call's timed interval: opened with the kernels' counters zeroed, closed by terrain_finish (above) with the counters read back
static int terrain_begin(const Terrain *t, SunCall &call) {
    HZ_HIP(hipMemsetAsync(t->counters, 0, HZ_SHADOW_CNT_N * sizeof(unsigned long long), call.st));
    return call.begin();
}

// host positions (chunks of k) go up through the handle's own buffer: no allocation per call
static int terrain_stage_positions(Terrain *t, ChunkFeed<float> &suns, int k) {
    if (!suns.staged()) return HZ_OK;
    if (t->sun_cap < 3 * (size_t)k) {
        if (t->sun_dev) (void)hipFree(t->sun_dev);
        t->sun_dev = nullptr; t->sun_cap = 0;
        const size_t cap = std::max<size_t>(3 * (size_t)k, 3 * 256);
        HZ_HIP(hipMalloc((void **)&t->sun_dev, cap * sizeof(float)));
        t->sun_cap = cap;
    }
    suns.stage = t->sun_dev;
    return HZ_OK;
}

static int terrain_run(Terrain *t, const float *sun_positions, int num_sun, int which, uint8_t *out_u8,
                       float *out_f32, hz_stats *stats) {
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_position' has incorrect shape");
    if ((which == 0 && !out_u8) || (which == 1 && !out_f32)) return set_error(HZ_ERR_ARG, "output buffer is NULL");
    SunCall call;
    int rc;
    if ((rc = call.start(t->device, t->scene->run_mu, t->stream))) return rc;
    const size_t nc = (size_t)t->dim_in_0 * t->dim_in_1;
    const int k = std::min(num_sun, HZ_SHADOW_MAX_POS);
    ChunkFeed<float> suns(sun_positions, 3);
    if ((rc = terrain_stage_positions(t, suns, k))) return rc;
    DevOut<uint8_t> d_u8; DevOut<float> d_f32;
    if ((rc = call.bind(d_u8, out_u8, nc * (size_t)num_sun, false))) return rc;
    if ((rc = call.bind(d_f32, out_f32, nc * (size_t)num_sun, false))) return rc;
    ShadowArgs a = terrain_args(t, which);
    if ((rc = terrain_begin(t, call))) return rc;
    for (int s0 = 0; s0 < num_sun; s0 += k) {
        a.num_sun = std::min(k, num_sun - s0);
        if ((rc = suns.at(s0, a.num_sun, call.st, &a.suns))) return rc;
        a.out_u8 = d_u8.dev ? d_u8.dev + nc * (size_t)s0 : nullptr;
        a.out_f32 = d_f32.dev ? d_f32.dev + nc * (size_t)s0 : nullptr;
        if ((rc = shadow_launch(t->scene, a, call.st))) return rc;
    }
    return terrain_finish(t, call, stats, false, d_u8, d_f32);      // no scratch_bytes: these calls never reported it
}

int hz_terrain_count_work(hz_terrain *terrain, int on) {
    if (!terrain) return set_error(HZ_ERR_ARG, "terrain is NULL");
    reinterpret_cast<Terrain *>(terrain)->count_work = on ? 1 : 0;
    return HZ_OK;
}

int hz_terrain_shadow(hz_terrain *terrain, const float *sun_position, uint8_t *shadow_buffer, hz_stats *stats) {
    return terrain_run(reinterpret_cast<Terrain *>(terrain), sun_position, 1, 0, shadow_buffer, nullptr, stats);
}
int hz_terrain_sw_dir_cor(hz_terrain *terrain, const float *sun_position, float *sw_dir_cor_buffer, hz_stats *stats) {
    return terrain_run(reinterpret_cast<Terrain *>(terrain), sun_position, 1, 1, nullptr, sw_dir_cor_buffer, stats);
}
int hz_terrain_shadow_batch(hz_terrain *terrain, const float *sun_positions, int num_sun,
                            uint8_t *shadow_buffers, hz_stats *stats) {
    return terrain_run(reinterpret_cast<Terrain *>(terrain), sun_positions, num_sun, 0, shadow_buffers, nullptr, stats);
}
int hz_terrain_sw_dir_cor_batch(hz_terrain *terrain, const float *sun_positions, int num_sun,
                                float *sw_dir_cor_buffers, hz_stats *stats) {
    return terrain_run(reinterpret_cast<Terrain *>(terrain), sun_positions, num_sun, 1, nullptr, sw_dir_cor_buffers, stats);
}

// Terrain.accumulate (hz_shadow.hip: k_accum_refill, k_accum_add, k_accum_final).  Positions go in chunks of k: the scratch of
// one chunk (1 B shadow code and / or 4 B correction per cell and position) is held to HZ_ACCUM_BUDGET (and to a quarter of the
// free HBM), so the device memory of a call -- scratch, two float64 accumulators, staged outputs, positions and weights -- does
// not depend on num_sun.  Every chunk is a launch of its own with a tail of its own: on the 3601^2 tile, 144 positions in
// chunks of 33 (a 2 GiB budget) traced in 130 ms against 120 ms for the single launch of shadow_batch.
#ifndef HZ_ACCUM_BUDGET
#define HZ_ACCUM_BUDGET (8ull << 30)
#endif
#define HZ_ACCUM_CHUNK_MAX 256      // small grids: 256 positions per chunk are already one large launch

// positions per chunk of accumulate and of Terrain's coarse call.  Not capped at the number of positions of the call: the
// scratch of a call (hz_stats.scratch_bytes) does not depend on how many there are
static int accum_chunk_positions(size_t nc, bool want_lit, bool want_sw, int *chunk) {
    int k = g_accum_chunk.load(std::memory_order_relaxed);       // (hz_debug_set("accum_chunk", k): tests)
    if (k <= 0) {
        size_t free_b = 0, total_b = 0;
        HZ_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t budget = std::min<size_t>(HZ_ACCUM_BUDGET, free_b / 4);
        const size_t per_pos = nc * ((want_lit ? 1 : 0) + (want_sw ? 4 : 0));
        k = (int)std::max<size_t>(1, std::min<size_t>(HZ_ACCUM_CHUNK_MAX, budget / per_pos));
    }
    *chunk = std::min(k, HZ_SHADOW_MAX_POS);
    return HZ_OK;
}

int hz_terrain_accumulate(hz_terrain *terrain, const float *sun_positions, const float *weights, int num_sun,
                          float *sw_dir_cor_sum, float *sunlit_sum, hz_stats *stats) {
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_positions' has incorrect shape");
    if (!sw_dir_cor_sum && !sunlit_sum) return set_error(HZ_ERR_ARG, "no output buffer (sw_dir_cor_sum and sunlit_sum are NULL)");
    SunCall call;
    int rc, k;
    if ((rc = call.start(t->device, t->scene->run_mu, t->stream))) return rc;
    const size_t nc = (size_t)t->dim_in_0 * t->dim_in_1;
    const bool want_sw = sw_dir_cor_sum != nullptr, want_lit = sunlit_sum != nullptr;
    // the sunlit sum needs the shadow code (which = 0: the shadow ray set); the correction alone traces its own, smaller set
    ShadowArgs a = terrain_args(t, want_lit ? 0 : 1);
    if ((rc = accum_chunk_positions(nc, want_lit, want_sw, &k))) return rc;
    ChunkFeed<float> suns(sun_positions, 3), w(weights, 1);
    ChunkMaps maps;
    SumMaps acc;
    if ((rc = maps.alloc(call, k, nc, want_lit, want_sw)) || (rc = acc.alloc(call, nc, want_sw, want_lit))) return rc;
    if ((rc = call.stage(k, suns, w))) return rc;
    DevOut<float> d_sw, d_lit;
    if ((rc = call.bind(d_sw, sw_dir_cor_sum, nc, true)) || (rc = call.bind(d_lit, sunlit_sum, nc, true))) return rc;
    HZ_HIP(hipMemsetAsync(acc.buf.p, 0, acc.bytes, call.st));
    if ((rc = terrain_begin(t, call))) return rc;
    a.out_u8 = maps.u8();
    a.out_f32 = maps.f32();
    for (int s0 = 0; s0 < num_sun; s0 += k) {
        const float *w_dev = nullptr;
        a.num_sun = std::min(k, num_sun - s0);
        if ((rc = suns.at(s0, a.num_sun, call.st, &a.suns)) || (rc = w.at(s0, a.num_sun, call.st, &w_dev))) return rc;
        if ((rc = accum_trace_launch(t->scene, a, want_sw && want_lit, call.st))) return rc;
        if ((rc = accum_add_launch(a.out_u8, a.out_f32, nc, a.num_sun, w_dev, acc.sw, acc.lit, call.st))) return rc;
    }
    if ((rc = accum_final_launch(a.mask, nc, t->fill, acc.sw, acc.lit, d_sw.dev, d_lit.dev, call.st))) return rc;
    return terrain_finish(t, call, stats, true, d_sw, d_lit);
}

// Terrain.sw_dir_cor_coarse (hz_subgrid.hip: k_coarse_count, k_coarse_reduce).  accumulate's chunks and scratch; instead of
// per-cell accumulators every chunk is reduced over blocks of pixel_per_gc_0 x pixel_per_gc_1 cells straight into the
// outputs at its first position.  Device memory besides the outputs -- scratch, the cell counts of the coarse cells, staged
// positions -- does not depend on num_sun (outputs given as host pointers are staged on the device: num_sun * gy * gx floats).
int hz_terrain_sw_dir_cor_coarse(hz_terrain *terrain, const float *sun_positions, int num_sun, int pixel_per_gc_0,
                                 int pixel_per_gc_1, float *f_cor, float *sunlit_frac, hz_stats *stats) {
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_positions' has incorrect shape");
    if (!f_cor && !sunlit_frac) return set_error(HZ_ERR_ARG, "no output buffer (f_cor and sunlit_frac are NULL)");
    if (f_cor == sunlit_frac) return set_error(HZ_ERR_ARG, "'f_cor' and 'sunlit_frac' must be different arrays");
    const int p0 = pixel_per_gc_0, p1 = pixel_per_gc_1;
    int rc, k;
    if ((rc = check_pixel_per_gc(p0, p1, t->dim_in_0, t->dim_in_1))) return rc;
    SunCall call;
    if ((rc = call.start(t->device, t->scene->run_mu, t->stream))) return rc;
    const size_t nc = (size_t)t->dim_in_0 * t->dim_in_1;
    const size_t ng = (size_t)(t->dim_in_0 / p0) * (size_t)(t->dim_in_1 / p1);
    const bool want_sw = f_cor != nullptr, want_lit = sunlit_frac != nullptr;
    // the sunlit fraction needs the shadow code (which = 0: the shadow ray set); the correction alone traces its own, smaller set
    ShadowArgs a = terrain_args(t, want_lit ? 0 : 1);
    if ((rc = accum_chunk_positions(nc, want_lit, want_sw, &k))) return rc;
    ChunkFeed<float> suns(sun_positions, 3);
    ChunkMaps maps;
    DevBuf count;
    if ((rc = maps.alloc(call, k, nc, want_lit, want_sw)) || (rc = call.alloc(count, ng * sizeof(unsigned)))) return rc;
    if ((rc = call.stage(k, suns))) return rc;
    DevOut<float> d_sw, d_lit;
    if ((rc = call.bind(d_sw, f_cor, ng * (size_t)num_sun, false)) || (rc = call.bind(d_lit, sunlit_frac, ng * (size_t)num_sun, false))) return rc;
    if ((rc = terrain_begin(t, call))) return rc;
    if ((rc = coarse_count_launch(a.mask, t->dim_in_0, t->dim_in_1, p0, p1, static_cast<unsigned *>(count.p), call.st))) return rc;
    a.out_u8 = maps.u8();
    a.out_f32 = maps.f32();
    for (int s0 = 0; s0 < num_sun; s0 += k) {
        a.num_sun = std::min(k, num_sun - s0);
        if ((rc = suns.at(s0, a.num_sun, call.st, &a.suns))) return rc;
        if ((rc = accum_trace_launch(t->scene, a, want_sw && want_lit, call.st))) return rc;
        if ((rc = coarse_reduce_launch(a.out_u8, a.out_f32, a.mask, static_cast<const unsigned *>(count.p), t->dim_in_0,
                                       t->dim_in_1, p0, p1, a.num_sun, t->fill, d_sw.dev ? d_sw.dev + ng * (size_t)s0 : nullptr,
                                       d_lit.dev ? d_lit.dev + ng * (size_t)s0 : nullptr, call.st)))
            return rc;
    }
    return terrain_finish(t, call, stats, true, d_sw, d_lit);
}

// Terrain.viewshed (hz_viewshed.hip: k_viewshed_refill; DESIGN.md section 4 clause 18).  Observers go in launches of up to
// HZ_SHADOW_MAX_POS (grid.y), as the positions of terrain_run do.  The kernel writes the codes and adds to the two counts
// itself: no scratch per chunk, and device memory besides the outputs -- the handle's staging buffer for host observers,
// outputs given as host pointers staged on the device -- does not depend on num_obs but for those staged outputs.
int hz_terrain_viewshed(hz_terrain *terrain, const float *observers, int num_obs, float target_elev, float max_dist, int facing,
                        uint8_t *visible, int32_t *seen_count, int64_t *cells_seen, hz_stats *stats) {
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!observers || num_obs <= 0) return set_error(HZ_ERR_ARG, "array 'observers' has incorrect shape");
    if (!visible && !seen_count && !cells_seen) return set_error(HZ_ERR_ARG, "no output buffer (visible, seen_count and cells_seen are NULL)");
    const void *outs[3] = {visible, seen_count, cells_seen};
    int rc;
    if ((rc = check_distinct_outputs(outs, 3))) return rc;
    if (!(target_elev >= 0.005f) || !std::isfinite(target_elev)) return set_error(HZ_ERR_ARG, "'target_elev' must be at least 0.005 m");
    SunCall call;
    if ((rc = call.start(t->device, t->scene->run_mu, t->stream))) return rc;
    const size_t nc = (size_t)t->dim_in_0 * t->dim_in_1;
    const int k = std::min(num_obs, HZ_SHADOW_MAX_POS);
    ChunkFeed<float> obs(observers, 3);
    if ((rc = terrain_stage_positions(t, obs, k))) return rc;
    DevOut<uint8_t> d_vis; DevOut<int32_t> d_seen; DevOut<int64_t> d_cells;
    if ((rc = call.bind(d_vis, visible, nc * (size_t)num_obs, false)) || (rc = call.bind(d_seen, seen_count, nc, true)) ||
        (rc = call.bind(d_cells, cells_seen, (size_t)num_obs, false)))
        return rc;
    ShadowArgs a = terrain_args(t, 0);
    a.refrac_cor = 0; a.refrac_fac = nullptr;     // a line of sight is not bent
    ViewshedArgs v;
    v.target_elev = target_elev; v.facing = facing ? 1 : 0;
    set_max_dist(v, max_dist);
    v.seen_count = d_seen.dev;
    if (d_seen.dev) HZ_HIP(hipMemsetAsync(d_seen.dev, 0, nc * sizeof(int32_t), call.st));
    if (d_cells.dev) HZ_HIP(hipMemsetAsync(d_cells.dev, 0, (size_t)num_obs * sizeof(int64_t), call.st));
    if ((rc = terrain_begin(t, call))) return rc;
    a.out_f32 = nullptr;
    for (int s0 = 0; s0 < num_obs; s0 += k) {
        a.num_sun = std::min(k, num_obs - s0);
        if ((rc = obs.at(s0, a.num_sun, call.st, &a.suns))) return rc;
        a.out_u8 = d_vis.dev ? d_vis.dev + nc * (size_t)s0 : nullptr;
        v.cells_seen = d_cells.dev ? d_cells.dev + s0 : nullptr;
        if ((rc = viewshed_launch(t->scene, a, v, call.st))) return rc;
    }
    if ((rc = viewshed_masked_launch(a.mask, nc, d_seen.dev, call.st))) return rc;
    return terrain_finish(t, call, stats, true, d_vis, d_seen, d_cells);
}

// the rules of sight_height's table (DESIGN.md section 4 clause 19): the kernel indexes it and does no arithmetic on it
static int check_sight_heights(const float *h, int n) {
    if (!(h[0] >= 0.005f)) return set_error(HZ_ERR_ARG, "'heights' must start at 0.005 m or above");
    for (int i = 0; i < n; i++)
        if (!std::isfinite(h[i])) return set_error(HZ_ERR_ARG, "'heights' has non-finite entries");
    for (int i = 1; i < n; i++)
        if (!(h[i] > h[i - 1])) return set_error(HZ_ERR_ARG, "'heights' must be strictly increasing");
    return HZ_OK;
}

// Terrain.sight_height (hz_sight.hip: k_sight_refill; DESIGN.md section 4 clause 19).  Observers go in launches of up to
// HZ_SHADOW_MAX_POS (grid.y), as in hz_terrain_viewshed.  The kernel writes the heights, takes the minimum over observers and
// adds to the count itself: no scratch per chunk.  Device memory besides the outputs: the table if it came from the host
// (4 bytes per entry, counted), a host `lowest` staged on the device (counted), the handle's staging buffer for host
// observers and the staging of a host `height` / `cells_reached` (not counted, as in hz_terrain_viewshed).
int hz_terrain_sight_height(hz_terrain *terrain, const float *observers, int num_obs, const float *heights, int num_heights,
                            float max_dist, float *height, float *lowest, int64_t *cells_reached, hz_stats *stats) {
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!observers || num_obs <= 0) return set_error(HZ_ERR_ARG, "array 'observers' has incorrect shape");
    if (!heights || num_heights < 1 || num_heights > 65535)
        return set_error(HZ_ERR_ARG, "array 'heights' must have 1 to 65535 entries");
    if (!height && !lowest && !cells_reached) return set_error(HZ_ERR_ARG, "no output buffer (height, lowest and cells_reached are NULL)");
    const void *outs[3] = {height, lowest, cells_reached};
    int rc;
    if ((rc = check_distinct_outputs(outs, 3))) return rc;
    ChunkFeed<float> table(heights, 1);
    if (table.staged() && (rc = check_sight_heights(heights, num_heights))) return rc;
    SunCall call;
    if ((rc = call.start(t->device, t->scene->run_mu, t->stream))) return rc;
    if (!table.staged()) {                        // a table in device memory is read back for its checks
        std::vector<float> h((size_t)num_heights);
        HZ_HIP(hipMemcpy(h.data(), heights, h.size() * sizeof(float), hipMemcpyDeviceToHost));
        if ((rc = check_sight_heights(h.data(), num_heights))) return rc;
    }
    const size_t nc = (size_t)t->dim_in_0 * t->dim_in_1;
    const int k = std::min(num_obs, HZ_SHADOW_MAX_POS);
    ChunkFeed<float> obs(observers, 3);
    if ((rc = terrain_stage_positions(t, obs, k))) return rc;
    SightArgs v;
    if ((rc = call.stage(num_heights, table)) || (rc = table.at(0, num_heights, call.st, &v.heights))) return rc;   // staged once
    DevOut<float> d_height, d_lowest; DevOut<int64_t> d_cells;
    if ((rc = call.bind(d_height, height, nc * (size_t)num_obs, false)) || (rc = call.bind(d_lowest, lowest, nc, true)) ||
        (rc = call.bind(d_cells, cells_reached, (size_t)num_obs, false)))
        return rc;
    ShadowArgs a = terrain_args(t, 1);
    a.refrac_cor = 0; a.refrac_fac = nullptr;     // a line of sight is not bent
    v.num_heights = num_heights;
    set_max_dist(v, max_dist);
    v.lowest = d_lowest.dev;
    if ((rc = sight_lowest_init_launch(nc, d_lowest.dev, call.st))) return rc;
    if (d_cells.dev) HZ_HIP(hipMemsetAsync(d_cells.dev, 0, (size_t)num_obs * sizeof(int64_t), call.st));
    if ((rc = terrain_begin(t, call))) return rc;
    a.out_u8 = nullptr;
    for (int s0 = 0; s0 < num_obs; s0 += k) {
        a.num_sun = std::min(k, num_obs - s0);
        if ((rc = obs.at(s0, a.num_sun, call.st, &a.suns))) return rc;
        a.out_f32 = d_height.dev ? d_height.dev + nc * (size_t)s0 : nullptr;
        v.cells_reached = d_cells.dev ? d_cells.dev + s0 : nullptr;
        if ((rc = sight_launch(t->scene, a, v, call.st))) return rc;
    }
    if ((rc = sight_masked_launch(a.mask, nc, d_lowest.dev, call.st))) return rc;
    return terrain_finish(t, call, stats, true, d_height, d_lowest, d_cells);
}

// Terrain.panorama (hz_panorama.hip: k_panorama; DESIGN.md section 4 clause 20).  Observers go in chunks (hz_panorama_plan.h):
// a `dist` / `point` given as host memory is staged on the device one chunk at a time and copied out inside the loop, so the
// staging -- what hz_stats.scratch_bytes reports, with the four tables if they came from the host and the chunk's observers
// and frames if those did -- is held to the budget and does not grow with num_obs.  Device outputs are written in place.  A
// host `hits` is staged whole (8 bytes per observer, not counted, as cells_seen of hz_terrain_viewshed).
int hz_terrain_panorama(hz_terrain *terrain, const float *observers, int num_obs, const float *azim_sin, const float *azim_cos,
                        int azim_num, const float *elev_sin, const float *elev_cos, int elev_num, const float *vec_north,
                        const float *vec_norm, float max_dist, float *dist, float *point, int64_t *hits, hz_stats *stats) {
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!observers || num_obs < 1) return set_error(HZ_ERR_ARG, "array 'observers' has incorrect shape");
    if (!azim_sin || !azim_cos || azim_num < 1) return set_error(HZ_ERR_ARG, "the azimuth tables must have at least one entry");
    if (!elev_sin || !elev_cos || elev_num < 1) return set_error(HZ_ERR_ARG, "the elevation tables must have at least one entry");
    if ((unsigned long long)azim_num * (unsigned long long)elev_num > HZ_PANORAMA_MAX_PIXELS)
        return set_error(HZ_ERR_ARG, "an image of %d x %d pixels exceeds 2^30", elev_num, azim_num);
    if (!std::isfinite(max_dist) || !(max_dist > 0.0f)) return set_error(HZ_ERR_ARG, "'max_dist' must be finite and greater than 0");
    if (!dist && !point && !hits) return set_error(HZ_ERR_ARG, "no output buffer (dist, point and hits are NULL)");
    if ((vec_north == nullptr) != (vec_norm == nullptr)) return set_error(HZ_ERR_ARG, "'vec_north' and 'vec_norm' must be given together");
    const void *outs[3] = {dist, point, hits};
    int rc;
    if ((rc = check_distinct_outputs(outs, 3))) return rc;
    const size_t pixels = (size_t)azim_num * (size_t)elev_num;
    SunCall call;                                 // (before the outputs: their chunks are freed while the call holds its lock)
    ChunkOut<float> o_dist(dist, pixels), o_point(point, 3 * pixels);
    const int knob = g_panorama_budget.load(std::memory_order_relaxed);       // (hz_debug_set("panorama_budget", bytes): tests)
    PanoramaPlan plan;
    if (!panorama_plan(num_obs, azim_num, elev_num, o_dist.staged(), o_point.staged(), knob > 0 ? (unsigned long long)knob : HZ_PANORAMA_BUDGET, &plan))
        return set_error(HZ_ERR_ARG, "panorama: no plan for %d observers of %d x %d pixels", num_obs, elev_num, azim_num);
    if ((rc = call.start(t->device, t->scene->run_mu, t->stream))) return rc;
    const int k = plan.chunk;
    ChunkFeed<float> obs(observers, 3), north(vec_north, 3), norm(vec_norm, 3);
    if ((rc = vec_north ? call.stage(k, obs, north, norm) : call.stage(k, obs))) return rc;
    PanoramaArgs a;
    DevIn<float> d_as, d_ac, d_es, d_ec;
    if ((rc = d_as.bind(azim_sin, (size_t)azim_num, call.st)) || (rc = d_ac.bind(azim_cos, (size_t)azim_num, call.st)) ||
        (rc = d_es.bind(elev_sin, (size_t)elev_num, call.st)) || (rc = d_ec.bind(elev_cos, (size_t)elev_num, call.st)))
        return rc;
    call.scratch += ((d_as.owned ? 1 : 0) + (d_ac.owned ? 1 : 0)) * (size_t)azim_num * sizeof(float) +
                    ((d_es.owned ? 1 : 0) + (d_ec.owned ? 1 : 0)) * (size_t)elev_num * sizeof(float);
    a.azim_sin = d_as.dev; a.azim_cos = d_ac.dev; a.elev_sin = d_es.dev; a.elev_cos = d_ec.dev;
    a.azim_num = azim_num; a.elev_num = elev_num; a.max_dist = max_dist;
    DevOut<int64_t> d_hits;
    if ((rc = call.bind(o_dist, k)) || (rc = call.bind(o_point, k)) || (rc = call.bind(d_hits, hits, (size_t)num_obs, false))) return rc;
    if (d_hits.dev) HZ_HIP(hipMemsetAsync(d_hits.dev, 0, (size_t)num_obs * sizeof(int64_t), call.st));
    if ((rc = terrain_begin(t, call))) return rc;
    for (int s0 = 0; s0 < num_obs; s0 += k) {
        a.num_obs = std::min(k, num_obs - s0);
        if ((rc = obs.at(s0, a.num_obs, call.st, &a.observers)) || (rc = north.at(s0, a.num_obs, call.st, &a.vec_north)) ||
            (rc = norm.at(s0, a.num_obs, call.st, &a.vec_norm)))
            return rc;
        a.dist = o_dist.at(s0); a.point = o_point.at(s0);
        a.hits = d_hits.dev ? d_hits.dev + s0 : nullptr;
        if ((rc = panorama_launch(t->scene, a, call.st))) return rc;
        // the chunk's staged images go out before the next chunk is traced into the same memory (stream order)
        if ((rc = o_dist.out(s0, a.num_obs, call.st)) || (rc = o_point.out(s0, a.num_obs, call.st))) return rc;
    }
    if ((rc = terrain_finish(t, call, stats, true, d_hits))) return rc;
    if (stats) stats->num_rays += (unsigned long long)num_obs * plan.pixels;      // every pixel is one ray
    return HZ_OK;
}

// Terrain.cast (hz_cast.hip: k_cast_closest, k_cast_any, k_cast_keys; DESIGN.md section 4 clause 21).  The rays go in chunks
// (hz_cast_plan.h): origins and directions / targets given as host memory go up one chunk at a time, outputs given as host
// memory are staged one chunk at a time and copied out inside the loop, and order = 1 sorts the chunk's (key, ray number)
// pairs on the device; all of that -- what hz_stats.scratch_bytes reports -- is held to the budget and does not grow with
// num_rays.  Device arrays are read and written in place.  The copies are not overlapped with the tracing.
int hz_terrain_cast(hz_terrain *terrain, const float *origins, const float *directions, const float *targets, int num_rays,
                    float max_dist, int order, uint8_t *occluded, float *dist, float *point, hz_stats *stats) {
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!origins || num_rays < 1 || (long long)num_rays > HZ_CAST_MAX_RAYS) return set_error(HZ_ERR_ARG, "array 'origins' has incorrect shape");
    if ((directions == nullptr) == (targets == nullptr)) return set_error(HZ_ERR_ARG, "exactly one of 'directions' and 'targets' must be given");
    if (directions && (!std::isfinite(max_dist) || !(max_dist > 0.0f))) return set_error(HZ_ERR_ARG, "'max_dist' must be finite and greater than 0");
    if (order != 0 && order != 1) return set_error(HZ_ERR_ARG, "'order' is 0 (given) or 1 (sorted)");
    if (!occluded && !dist && !point) return set_error(HZ_ERR_ARG, "no output buffer (occluded, dist and point are NULL)");
    const void *outs[3] = {occluded, dist, point};
    int rc;
    if ((rc = check_distinct_outputs(outs, 3))) return rc;
    const float *ends_src = directions ? directions : targets;
    SunCall call;                                 // (before the outputs: their chunks are freed while the call holds its lock)
    ChunkFeed<float> org(origins, 3), ends(ends_src, 3);
    ChunkOut<uint8_t> o_occ(occluded, 1);
    ChunkOut<float> o_dist(dist, 1), o_point(point, 3);
    const int knob = g_cast_budget.load(std::memory_order_relaxed);           // (hz_debug_set("cast_budget", bytes): tests)
    CastPlan plan;
    if (!cast_plan(num_rays, org.staged(), ends.staged(), o_occ.staged(), o_dist.staged(), o_point.staged(), order == 1,
                   knob > 0 ? (unsigned long long)knob : HZ_CAST_BUDGET, &plan))
        return set_error(HZ_ERR_ARG, "cast: no plan for %d rays", num_rays);
    if ((rc = call.start(t->device, t->scene->run_mu, t->stream))) return rc;
    const int k = plan.chunk;
    if ((rc = org.staged() && ends.staged() ? call.stage(k, org, ends) : org.staged() ? call.stage(k, org) : call.stage(k, ends))) return rc;
    if ((rc = call.bind(o_occ, k)) || (rc = call.bind(o_dist, k)) || (rc = call.bind(o_point, k))) return rc;
    // order = 1: keys and ray numbers, in and out, and the sort's histograms
    DevBuf sort_buf;
    uint32_t *keys_a = nullptr, *vals_a = nullptr, *keys_b = nullptr, *vals_b = nullptr, *sort_tmp = nullptr;
    if (order == 1) {
        if ((rc = call.alloc(sort_buf, (4 * (size_t)k + sort_temp_elems((size_t)k)) * sizeof(uint32_t)))) return rc;
        keys_a = static_cast<uint32_t *>(sort_buf.p); vals_a = keys_a + k; keys_b = vals_a + k; vals_b = keys_b + k; sort_tmp = vals_b + k;
    }
    CastArgs a;
    a.segments = targets ? 1 : 0; a.max_dist = max_dist; a.perm = nullptr;
    a.counters = t->counters; a.count_work = t->count_work;
    const bool trace = g_cast_sort_only.load(std::memory_order_relaxed) == 0;
    if ((rc = terrain_begin(t, call))) return rc;
    for (long long s0 = 0; s0 < (long long)num_rays; s0 += k) {
        const int kc = (int)std::min<long long>(k, (long long)num_rays - s0);
        if ((rc = org.at((int)s0, kc, call.st, &a.origins)) || (rc = ends.at((int)s0, kc, call.st, &a.ends))) return rc;
        a.num_rays = (unsigned)kc;
        if (order == 1) {
            if ((rc = cast_keys_launch(t->scene, a.origins, a.ends, a.segments, a.num_rays, keys_a, vals_a, call.st)) ||
                (rc = radix_sort_pairs_u32(keys_a, vals_a, keys_b, vals_b, (size_t)kc, sort_tmp, call.st, 4)))      // 4 passes: sorted in vals_a
                return rc;
            a.perm = vals_a;
        }
        if (!trace) continue;
        a.occluded = o_occ.at(s0); a.dist = o_dist.at(s0); a.point = o_point.at(s0);
        if ((rc = cast_launch(t->scene, a, call.st))) return rc;
        // the chunk's staged results go out before the next chunk is traced into the same memory (stream order)
        if ((rc = o_occ.out(s0, kc, call.st)) || (rc = o_dist.out(s0, kc, call.st)) || (rc = o_point.out(s0, kc, call.st))) return rc;
    }
    return terrain_finish(t, call, stats, true);    // num_rays: the rays the kernels traced
}

int hz_terrain_destroy(hz_terrain *terrain) {
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    if (!t) return HZ_OK;
    (void)hipSetDevice(t->device);
    terrain_release_arrays(t);
    if (t->counters) (void)hipFree(t->counters);
    delete t;
    return HZ_OK;
}

// ---------------------------------------------------------------------------------------
// HorizonTerrain (hz_horisun.hip): Terrain's answers from a stored horizon, DESIGN.md section 4 clause 10
// ---------------------------------------------------------------------------------------

int hz_horizon_terrain_create(int device, hz_horizon_terrain **terrain) {
    if (!terrain) return set_error(HZ_ERR_ARG, "terrain is NULL");
    int rc = select_device(device);
    if (rc) return rc;
    HorizonTerrain *t = new HorizonTerrain();
    t->device = device;
    if ((rc = stream_acquire(device, &t->stream))) { delete t; return rc; }
    *terrain = reinterpret_cast<hz_horizon_terrain *>(t);
    return HZ_OK;
}

static int horisun_initialise(hz_horizon_terrain *terrain, bool planes, bool q16, const void *hori, int azim_num, const float *vert_grid,
                              int dem_dim_0, int dem_dim_1, int offset_0, int offset_1, const float *vec_tilt,
                              const float *vec_norm, const float *vec_north, int dim_in_0, int dim_in_1,
                              const float *surf_enl_fac, const uint8_t *mask, float sw_dir_cor_fill, float ang_max,
                              hz_stats *stats) {
    HorizonTerrain *t = reinterpret_cast<HorizonTerrain *>(terrain);
    if (!t) return set_error(HZ_ERR_ARG, "terrain is NULL");
    if (!hori || !vert_grid || !vec_tilt || !vec_norm || !vec_north || !surf_enl_fac || !mask)
        return set_error(HZ_ERR_ARG, "NULL input array");
    if (azim_num < 1) return set_error(HZ_ERR_ARG, "'azim_num' must be at least 1");
    if (dim_in_0 <= 0 || dim_in_1 <= 0 || offset_0 < 0 || offset_1 < 0 || dem_dim_0 <= 0 || dem_dim_1 <= 0 ||
        (long long)offset_0 + dim_in_0 > dem_dim_0 || (long long)offset_1 + dim_in_1 > dem_dim_1)
        return set_error(HZ_ERR_ARG, "inconsistency between input arguments 'dem_dim_0', 'dem_dim_1', 'offset_0', 'offset_1' and 'vec_norm'");
    if (!(ang_max >= 85.0f && ang_max <= 89.99f)) return set_error(HZ_ERR_ARG, "'ang_max' must be in the range [85.0, 89.99]");
    HorisunPlan plan;
    if (horisun_plan(dim_in_0, dim_in_1, azim_num, 1, 0, 0, &plan)) return set_error(HZ_ERR_ARG, "the inner domain or 'hori' is too large");
    std::lock_guard<std::mutex> run_lock(t->run_mu);
    horisun_release(t);
    HZ_HIP(hipSetDevice(t->device));
    hipStream_t st = t->stream;
    Timer t_total; t_total.start();
    const size_t nc = plan.cells;
    int rc = HZ_OK;
    if (is_device_ptr(hori)) { t->hori = static_cast<const float *>(hori); t->own_hori = false; }
    else {
        void *h = nullptr;
        rc = horisun_copy(hori, nc * (size_t)azim_num * (q16 ? sizeof(uint16_t) : sizeof(float)), st, &h);
        t->hori = static_cast<const float *>(h); t->own_hori = true;
    }
    if (!rc) rc = horisun_copy(vec_tilt, nc * 12, st, &t->tilt);
    if (!rc) rc = horisun_copy(vec_norm, nc * 12, st, &t->norm);
    if (!rc) rc = horisun_copy(vec_north, nc * 12, st, &t->north);
    if (!rc) rc = horisun_copy(surf_enl_fac, nc * 4, st, &t->enl);
    if (!rc) rc = horisun_copy(mask, nc, st, &t->mask);
    // the vertices of the inner domain only: rows of dim_in_1 vertices out of DEM rows of dem_dim_1
    if (!rc) {
        const hipError_t e = hipMalloc(&t->vert, nc * 12);
        if (e != hipSuccess) rc = set_error(HZ_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    if (!rc) {
        const float *src = vert_grid + 3 * ((size_t)offset_0 * (size_t)dem_dim_1 + (size_t)offset_1);
        const hipError_t e = hipMemcpy2DAsync(t->vert, (size_t)dim_in_1 * 12, src, (size_t)dem_dim_1 * 12, (size_t)dim_in_1 * 12,
                                              (size_t)dim_in_0, is_device_ptr(vert_grid) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
        if (e != hipSuccess) rc = set_error(HZ_ERR_HIP, "hipMemcpy2DAsync failed: %s", hipGetErrorString(e));
    }
    if (!rc) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(HZ_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    if (rc) { horisun_release(t); return rc; }
    t->azim_num = azim_num; t->dim_in_0 = dim_in_0; t->dim_in_1 = dim_in_1; t->planes = planes; t->q16 = q16;
    t->fill = sw_dir_cor_fill; t->ang_max = ang_max;
    t->initialised = true;
    if (stats) {
        const double dt = t_total.stop();
        stats->t_h2d_s += dt; stats->t_total_s += dt;
        stats->num_cells = nc;
    }
    return HZ_OK;
}

int hz_horizon_terrain_initialise(hz_horizon_terrain *terrain, const float *hori, int azim_num, const float *vert_grid,
                                  int dem_dim_0, int dem_dim_1, int offset_0, int offset_1, const float *vec_tilt,
                                  const float *vec_norm, const float *vec_north, int dim_in_0, int dim_in_1,
                                  const float *surf_enl_fac, const uint8_t *mask, float sw_dir_cor_fill, float ang_max,
                                  hz_stats *stats) {
    return horisun_initialise(terrain, false, false, hori, azim_num, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_tilt,
                              vec_norm, vec_north, dim_in_0, dim_in_1, surf_enl_fac, mask, sw_dir_cor_fill, ang_max, stats);
}

int hz_horizon_terrain_initialise_planes(hz_horizon_terrain *terrain, const float *planes, int azim_num, const float *vert_grid,
                                         int dem_dim_0, int dem_dim_1, int offset_0, int offset_1, const float *vec_tilt,
                                         const float *vec_norm, const float *vec_north, int dim_in_0, int dim_in_1,
                                         const float *surf_enl_fac, const uint8_t *mask, float sw_dir_cor_fill, float ang_max,
                                         hz_stats *stats) {
    return horisun_initialise(terrain, true, false, planes, azim_num, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_tilt,
                              vec_norm, vec_north, dim_in_0, dim_in_1, surf_enl_fac, mask, sw_dir_cor_fill, ang_max, stats);
}

int hz_horizon_terrain_initialise_q16(hz_horizon_terrain *terrain, const uint16_t *hori_q, int azim_num, int planes,
                                      const float *vert_grid, int dem_dim_0, int dem_dim_1, int offset_0, int offset_1,
                                      const float *vec_tilt, const float *vec_norm, const float *vec_north, int dim_in_0,
                                      int dim_in_1, const float *surf_enl_fac, const uint8_t *mask, float sw_dir_cor_fill,
                                      float ang_max, hz_stats *stats) {
    if (planes != 0 && planes != 1) return set_error(HZ_ERR_ARG, "planes must be 0 or 1");
    if (reinterpret_cast<uintptr_t>(hori_q) & 1) return set_error(HZ_ERR_ARG, "hori_q is not aligned to 2 bytes");
    return horisun_initialise(terrain, planes != 0, true, hori_q, azim_num, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                              vec_tilt, vec_norm, vec_north, dim_in_0, dim_in_1, surf_enl_fac, mask, sw_dir_cor_fill, ang_max,
                              stats);
}

// Refraction on (elevation f32[cells], host or device: copied, as surf_enl_fac is) or off (NULL): the per-cell float64 factor of
// Terrain's refrac_cor, 8 bytes per cell, which every later call hands to its kernels (clause 13)
int hz_horizon_terrain_refraction(hz_horizon_terrain *terrain, const float *elevation, hz_stats *stats) {
    HorizonTerrain *t = reinterpret_cast<HorizonTerrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "HorizonTerrain is not initialised");
    std::lock_guard<std::mutex> run_lock(t->run_mu);
    HZ_HIP(hipSetDevice(t->device));
    hipStream_t st = t->stream;
    Timer t_total; t_total.start();
    HZ_HIP(hipStreamSynchronize(st));
    if (t->refrac_fac) { (void)hipFree(t->refrac_fac); t->refrac_fac = nullptr; }
    const size_t nc = (size_t)t->dim_in_0 * (size_t)t->dim_in_1;
    if (elevation) {
        DevBuf elev, fac;
        int rc;
        if ((rc = horisun_copy(elevation, nc * sizeof(float), st, &elev.p))) return rc;
        HZ_HIP(fac.alloc(nc * sizeof(double)));
        if ((rc = shadow_refrac_factor(static_cast<const float *>(elev.p), nc, static_cast<double *>(fac.p), st))) return rc;
        HZ_HIP(hipStreamSynchronize(st));
        t->refrac_fac = static_cast<double *>(fac.p);
        fac.p = nullptr;
    }
    if (stats) {
        const double dt = t_total.stop();
        stats->t_h2d_s += dt; stats->t_total_s += dt;
        stats->num_cells = nc;
    }
    return HZ_OK;
}

// the launch arguments every k_horisun launch of the handle shares: no weights, no sums, no map per position, one launch
static HorisunArgs horisun_args(const HorizonTerrain *t) {
    HorisunArgs a{};
    horisun_inputs(t, a);
    a.surf_enl_fac = (const float *)t->enl;
    a.dot_prod_min = cosf(deg2rad_f(t->ang_max));            // shadow_comp.cpp:498
    a.first = a.last = 1;
    return a;
}

// one launch of k_horisun over a chunk; planes: the same launch plan, the horizon read as planes[k * cells + c] (k_horisun_planes, hz_planes.hip)
static int horisun_trace(const HorizonTerrain *t, const HorisunArgs &a, const HorisunPlan &plan, hipStream_t st) {
    return t->planes ? horisun_planes_launch(a, a.cells, plan.blocks, st, t->q16) : horisun_launch(a, plan.blocks, st, t->q16);
}

// what every HorizonTerrain call reports besides its times
static void horisun_stats(const SunCall &call, size_t nc, hz_stats *stats) {
    if (!stats) return;
    stats->num_cells = nc;
    stats->scratch_bytes = call.scratch;
}

int hz_horizon_terrain_run(hz_horizon_terrain *terrain, const float *sun_positions, const float *weights, int num_sun,
                           const hz_horisun_out *out, hz_stats *stats) {
    HorizonTerrain *t = reinterpret_cast<HorizonTerrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "HorizonTerrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_positions' has incorrect shape");
    if (!out || out->size != (int32_t)sizeof(hz_horisun_out))
        return set_error(HZ_ERR_ARG, "hz_horisun_out.size is %d, expected %d", out ? (int)out->size : 0, (int)sizeof(hz_horisun_out));
    const void *outs[4] = {out->shadow, out->sw_dir_cor, out->sw_dir_cor_sum, out->sunlit_sum};
    if (!outs[0] && !outs[1] && !outs[2] && !outs[3]) return set_error(HZ_ERR_ARG, "no output buffer (every pointer of hz_horisun_out is NULL)");
    int rc;
    if ((rc = check_distinct_outputs(outs, 4))) return rc;
    const bool want_sums = out->sw_dir_cor_sum || out->sunlit_sum;
    HorisunPlan plan;
    if (horisun_plan(t->dim_in_0, t->dim_in_1, t->azim_num, num_sun, g_horisun_chunk.load(std::memory_order_relaxed),
                     (out->shadow ? 1 : 0) + (out->sw_dir_cor ? 4 : 0), &plan))
        return set_error(HZ_ERR_ARG, "too many sun positions for the per-position outputs");
    SunCall call;
    if ((rc = call.start(t->device, t->run_mu, t->stream))) return rc;
    const size_t nc = plan.cells;
    ChunkFeed<float> suns(sun_positions, 3), w(want_sums ? weights : nullptr, 1);
    // the sums live in registers during a launch and in two float64 maps between the launches of a call
    SumMaps acc;
    if ((rc = acc.alloc(call, nc, out->sw_dir_cor_sum != nullptr, out->sunlit_sum != nullptr))) return rc;
    if ((rc = call.stage(plan.chunk, suns, w))) return rc;
    DevOut<uint8_t> d_u8; DevOut<float> d_f32, d_sw, d_lit;
    if ((rc = call.bind(d_u8, out->shadow, nc * (size_t)num_sun, false))) return rc;
    if ((rc = call.bind(d_f32, out->sw_dir_cor, nc * (size_t)num_sun, false))) return rc;
    if ((rc = call.bind(d_sw, out->sw_dir_cor_sum, nc, true)) || (rc = call.bind(d_lit, out->sunlit_sum, nc, true))) return rc;
    HorisunArgs a = horisun_args(t);
    a.acc_sw = acc.sw; a.acc_lit = acc.lit;
    a.sum_sw = d_sw.dev; a.sum_lit = d_lit.dev;
    if ((rc = call.begin())) return rc;
    for (int c = 0; c < plan.num_chunks; c++) {
        int s0 = 0;
        horisun_chunk(plan, num_sun, c, &s0, &a.num_sun);
        if ((rc = suns.at(s0, a.num_sun, call.st, &a.suns)) || (rc = w.at(s0, a.num_sun, call.st, &a.weights))) return rc;
        a.out_u8 = d_u8.dev ? d_u8.dev + nc * (size_t)s0 : nullptr;
        a.out_f32 = d_f32.dev ? d_f32.dev + nc * (size_t)s0 : nullptr;
        a.first = c == 0; a.last = c == plan.num_chunks - 1;
        if ((rc = horisun_trace(t, a, plan, call.st))) return rc;
    }
    if ((rc = call.end())) return rc;
    if ((rc = call.finish(stats, d_u8, d_f32, d_sw, d_lit))) return rc;
    horisun_stats(call, nc, stats);
    return HZ_OK;
}

// HorizonTerrain.sw_dir_cor_coarse (DESIGN.md section 4 clause 12).  Fused route: k_horisun_coarse (hz_horisun_coarse.hip) per
// chunk, no map per position.  Two-pass route (the measured default of both layouts, "horisun_coarse_route" = 1, and blocks
// wider than the fused kernel's LDS tile): the chunk goes through k_horisun / k_horisun_planes into scratch u8[k][cells] / f32[k][cells], which k_coarse_reduce
// (hz_subgrid.hip) reduces.  Device memory besides the outputs -- the scratch of the two-pass route, the cell counts of the
// coarse cells, staged positions -- does not depend on num_sun.
int hz_horizon_terrain_sw_dir_cor_coarse(hz_horizon_terrain *terrain, const float *sun_positions, int num_sun, int pixel_per_gc_0,
                                         int pixel_per_gc_1, float *f_cor, float *sunlit_frac, hz_stats *stats) {
    HorizonTerrain *t = reinterpret_cast<HorizonTerrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "HorizonTerrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_positions' has incorrect shape");
    if (!f_cor && !sunlit_frac) return set_error(HZ_ERR_ARG, "no output buffer (f_cor and sunlit_frac are NULL)");
    if (f_cor == sunlit_frac) return set_error(HZ_ERR_ARG, "'f_cor' and 'sunlit_frac' must be different arrays");
    const int p0 = pixel_per_gc_0, p1 = pixel_per_gc_1;
    int rc;
    if ((rc = check_pixel_per_gc(p0, p1, t->dim_in_0, t->dim_in_1))) return rc;
    const bool want_sw = f_cor != nullptr, want_lit = sunlit_frac != nullptr;
    HorisunPlan plan;
    if (horisun_plan(t->dim_in_0, t->dim_in_1, t->azim_num, num_sun, g_horisun_chunk.load(std::memory_order_relaxed), 0, &plan))
        return set_error(HZ_ERR_ARG, "too many sun positions");
    const int k = std::min(plan.chunk, HZ_HSC_CHUNK_MAX);        // grid.y of either route
    HorisunCoarsePlan cp;
    if ((rc = horisun_coarse_plan_for(t->dim_in_0, t->dim_in_1, p0, p1, k, t->planes, want_lit, want_sw, &cp))) return rc;
    if (t->q16) cp.fallback = 1;      // codes: always the two-pass route, whatever "horisun_coarse_route" says (no fused kernel reads them)
    const size_t nc = plan.cells;
    const size_t ng = (size_t)(t->dim_in_0 / p0) * (size_t)(t->dim_in_1 / p1);
    if (ng > (size_t)SIZE_MAX / sizeof(float) / (size_t)num_sun) return set_error(HZ_ERR_ARG, "too many sun positions");
    SunCall call;
    if ((rc = call.start(t->device, t->run_mu, t->stream))) return rc;
    ChunkFeed<float> suns(sun_positions, 3);
    ChunkMaps maps;
    DevBuf count;
    if (cp.fallback && (rc = maps.alloc(call, k, nc, want_lit, want_sw))) return rc;
    if ((rc = call.alloc(count, ng * sizeof(unsigned))) || (rc = call.stage(k, suns))) return rc;
    DevOut<float> d_sw, d_lit;
    if ((rc = call.bind(d_sw, f_cor, ng * (size_t)num_sun, false)) || (rc = call.bind(d_lit, sunlit_frac, ng * (size_t)num_sun, false))) return rc;
    HorisunArgs a = horisun_args(t);
    a.out_u8 = maps.u8();
    a.out_f32 = maps.f32();
    if ((rc = call.begin())) return rc;
    const unsigned *n = static_cast<const unsigned *>(count.p);
    if ((rc = coarse_count_launch(a.mask, t->dim_in_0, t->dim_in_1, p0, p1, static_cast<unsigned *>(count.p), call.st))) return rc;
    for (int s0 = 0; s0 < num_sun; s0 += k) {
        a.num_sun = std::min(k, num_sun - s0);
        if ((rc = suns.at(s0, a.num_sun, call.st, &a.suns))) return rc;
        float *o_sw = d_sw.dev ? d_sw.dev + ng * (size_t)s0 : nullptr, *o_lit = d_lit.dev ? d_lit.dev + ng * (size_t)s0 : nullptr;
        if (cp.fallback) {
            if ((rc = horisun_trace(t, a, plan, call.st))) return rc;
            if ((rc = coarse_reduce_launch(a.out_u8, a.out_f32, a.mask, n, t->dim_in_0, t->dim_in_1, p0, p1, a.num_sun, t->fill,
                                           o_sw, o_lit, call.st)))
                return rc;
        } else if ((rc = horisun_coarse_launch(a, t->planes, nc, cp, n, t->dim_in_1, p0, p1, o_sw, o_lit, call.st))) return rc;
    }
    if ((rc = call.end())) return rc;
    if ((rc = call.finish(stats, d_sw, d_lit))) return rc;
    horisun_stats(call, nc, stats);
    return HZ_OK;
}

// HorizonTerrain.sun_times (DESIGN.md section 4 clause 14; k_suntimes, hz_suntimes.hip): the position chunks of
// hz_horizon_terrain_run, each lane's running state in registers during a launch and in 44 B per cell between the launches of a
// call.  times[s0 - 1] of a chunk travels as a kernel argument; host positions and times go up one chunk at a time.
int hz_horizon_terrain_sun_times(hz_horizon_terrain *terrain, const float *sun_positions, const double *times, int num_sun,
                                 const hz_suntimes_out *out, hz_stats *stats) {
    HorizonTerrain *t = reinterpret_cast<HorizonTerrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "HorizonTerrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_positions' has incorrect shape");
    if (!times) return set_error(HZ_ERR_ARG, "array 'times' has incorrect shape");
    if (!out || out->size != (int32_t)sizeof(hz_suntimes_out))
        return set_error(HZ_ERR_ARG, "hz_suntimes_out.size is %d, expected %d", out ? (int)out->size : 0, (int)sizeof(hz_suntimes_out));
    const void *outs[4] = {out->sunrise, out->sunset, out->duration, out->intervals};
    if (!outs[0] && !outs[1] && !outs[2] && !outs[3]) return set_error(HZ_ERR_ARG, "no output buffer (every pointer of hz_suntimes_out is NULL)");
    int rc;
    if ((rc = check_distinct_outputs(outs, 4))) return rc;
    HorisunPlan plan;
    if (horisun_plan(t->dim_in_0, t->dim_in_1, t->azim_num, num_sun, g_horisun_chunk.load(std::memory_order_relaxed), 0, &plan))
        return set_error(HZ_ERR_ARG, "too many sun positions");
    SunCall call;
    if ((rc = call.start(t->device, t->run_mu, t->stream))) return rc;
    ChunkFeed<float> suns(sun_positions, 3);
    ChunkFeed<double> tm(times, 1);
    // the times on the host: they are checked here, and the one before each chunk is a kernel argument
    std::vector<double> times_down;
    const double *times_host = times;
    if (tm.on_dev) {
        times_down.resize((size_t)num_sun);
        HZ_HIP(hipMemcpy(times_down.data(), times, (size_t)num_sun * sizeof(double), hipMemcpyDeviceToHost));
        times_host = times_down.data();
    }
    for (int s = 0; s < num_sun; s++)
        if (!std::isfinite(times_host[s]) || (s > 0 && !(times_host[s] > times_host[s - 1])))
            return set_error(HZ_ERR_ARG, "'times' must be finite and strictly increasing (times[%d])", s);
    const size_t nc = plan.cells;
    DevBuf state;
    if (plan.num_chunks > 1 && (rc = call.alloc(state, suntimes_state_bytes(nc)))) return rc;
    if ((rc = call.stage(plan.chunk, tm, suns))) return rc;      // (the doubles first: alignment)
    DevOut<float> d_rise, d_set, d_dur; DevOut<int32_t> d_n;
    if ((rc = call.bind(d_rise, out->sunrise, nc, true)) || (rc = call.bind(d_set, out->sunset, nc, true)) ||
        (rc = call.bind(d_dur, out->duration, nc, true)) || (rc = call.bind(d_n, out->intervals, nc, true)))
        return rc;
    SuntimesArgs a{};
    horisun_inputs(t, a);
    a.stride = nc;
    a.state = static_cast<double *>(state.p);
    a.state_n = state.p ? reinterpret_cast<int32_t *>(a.state + 5 * nc) : nullptr;
    a.sunrise = d_rise.dev; a.sunset = d_set.dev; a.duration = d_dur.dev; a.intervals = d_n.dev;
    if ((rc = call.begin())) return rc;
    for (int c = 0; c < plan.num_chunks; c++) {
        int s0 = 0;
        horisun_chunk(plan, num_sun, c, &s0, &a.num_sun);
        if ((rc = suns.at(s0, a.num_sun, call.st, &a.suns)) || (rc = tm.at(s0, a.num_sun, call.st, &a.times))) return rc;
        a.t_before = s0 > 0 ? times_host[s0 - 1] : times_host[0];
        a.first = c == 0; a.last = c == plan.num_chunks - 1;
        if ((rc = suntimes_launch(a, t->planes, plan.blocks, call.st, t->q16))) return rc;
    }
    if ((rc = call.end())) return rc;
    if ((rc = call.finish(stats, d_rise, d_set, d_dur, d_n))) return rc;
    horisun_stats(call, nc, stats);
    return HZ_OK;
}

int hz_horizon_terrain_destroy(hz_horizon_terrain *terrain) {
    HorizonTerrain *t = reinterpret_cast<HorizonTerrain *>(terrain);
    if (!t) return HZ_OK;
    horisun_release(t);
    stream_release(t->device, t->stream);
    delete t;
    return HZ_OK;
}

}  // extern "C"
