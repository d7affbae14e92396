// hz_api.hip -- C-ABI entry points of libhorayzon_hip.so (see include/horayzon_hip.h).
//
// Scenes, the stream pool, the stand-alone reductions and conversions, and the Terrain / HorizonTerrain drivers restating
// CppTerrain (shadow_comp.cpp:304-605); the horizon drivers are in hz_api_horizon.hip.
#include "hz_internal.h"
#include "hz_horisun_plan.h"
#include "hz_horisun_coarse_plan.h"
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include <limits>
#include <mutex>
#include <utility>
#include <atomic>

namespace hz {

static thread_local std::string g_error;

int set_error(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}


static int select_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return set_error(HZ_ERR_NODEV, "no HIP device available (libhorayzon_hip needs an MI355X / gfx950 GPU)");
    }
    if (device < 0 || device >= n) return set_error(HZ_ERR_ARG, "device %d out of range (%d devices)", device, n);
    HZ_HIP(hipSetDevice(device));
    return HZ_OK;
}

static int check_geom(const char *s) {
    // all three describe the same surface (horizon_comp.cpp:139-183); the explicit
    // "triangle" split is what the LBVH leaves hold
    if (s && (strcmp(s, "triangle") == 0 || strcmp(s, "quad") == 0 || strcmp(s, "grid") == 0)) return HZ_OK;
    return set_error(HZ_ERR_ARG, "invalid input argument for geom_type");
}

// ---- stream pool --------------------------------------------------------------------------------
// Streams are taken from a per-device pool and go back to it; the library NEVER calls hipStreamDestroy.
// Reason (root cause of the "stray element" of round 1, DESIGN_HISTORY.md section 2): with the HIP runtime of
// ROCm 7.0 (libamdhip64 as bundled with PyTorch 2.10+rocm7.0) hipStreamDestroy() frees the ~920-byte stream
// object while a completion callback of that stream can still be pending on the ROCr async-events thread;
// the callback then decrements a counter at offset 152 and stores a 32-bit zero at offset 888 of the FREED
// block -- i.e. into whatever the application allocated there next (a 912-byte NumPy array shares the malloc
// size class: one float of a result array turned 0.0 after the call had returned).  Caught with the heap
// tripwire scripts/stray/hzq_preload.c: writer = libhsa-runtime64 AsyncEventsLoop -> libamdhip64 callback,
// block allocated in hipStreamCreateWithFlags, freed in hipStreamDestroy.  A pooled stream is synchronised
// before it is reused, so no work ever outlives its owner.
static std::mutex g_stream_mu;
static std::vector<std::pair<int, hipStream_t>> g_stream_pool;    // (device, idle stream)

int stream_acquire(int device, hipStream_t *st) {
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        for (size_t i = 0; i < g_stream_pool.size(); i++)
            if (g_stream_pool[i].first == device) {
                *st = g_stream_pool[i].second;
                g_stream_pool.erase(g_stream_pool.begin() + (long)i);
                return HZ_OK;
            }
    }
    const hipError_t e = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    if (e != hipSuccess) return set_error(HZ_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    return HZ_OK;
}

void stream_release(int device, hipStream_t st) {
    if (!st) return;
    (void)hipStreamSynchronize(st);
    std::lock_guard<std::mutex> lk(g_stream_mu);
    g_stream_pool.emplace_back(device, st);
}

static int scene_new(int device, Scene **out) {
    int rc = select_device(device);
    if (rc) return rc;
    Scene *sc = new Scene();
    sc->device = device;
    if ((rc = stream_acquire(device, &sc->stream))) { delete sc; return rc; }
    *out = sc;
    return HZ_OK;
}

static void scene_free(Scene *sc) {
    if (!sc) return;
    (void)hipSetDevice(sc->device);
    stream_release(sc->device, sc->stream);
    if (sc->near_buf) (void)hipFree(sc->near_buf);
    if (sc->left_buf) (void)hipFree(sc->left_buf);
    if (sc->owns_blob && sc->blob) (void)hipFree(sc->blob);
    delete sc;
}

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
    unsigned long long *counters = nullptr;   // device u64[16]
    float *sun_dev = nullptr;                 // persistent device copy of the sun positions of a call (grown on demand: the
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

}  // namespace hz

using namespace hz;

extern "C" {

const char *hz_last_error(void) { return g_error.c_str(); }

int hz_abi_version(void) { return 6; }

int hz_abi_struct_sizes(int *opts_bytes, int *stats_bytes) {
    if (opts_bytes) *opts_bytes = (int)sizeof(hz_opts);
    if (stats_bytes) *stats_bytes = (int)sizeof(hz_stats);
    return HZ_OK;
}

int hz_device_count(int *count) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    if (count) *count = n;
    return HZ_OK;
}

int hz_device_info(int device, char *name, int cap, int *cu, uint64_t *hbm_bytes) {
    int rc = select_device(device);
    if (rc) return rc;
    hipDeviceProp_t prop;
    HZ_HIP(hipGetDeviceProperties(&prop, device));
    if (name && cap > 0) { strncpy(name, prop.gcnArchName, (size_t)cap - 1); name[cap - 1] = 0; }
    if (cu) *cu = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)prop.totalGlobalMem;
    return HZ_OK;
}

int hz_scene_create(const float *vert_grid, int dem_dim_0, int dem_dim_1, const char *geom_type,
                    const float *vert_simp, int num_vert_simp, const int32_t *tri_ind_simp,
                    int num_tri_simp, int device, hz_scene **scene, hz_stats *stats) {
    if (!scene || !vert_grid) return set_error(HZ_ERR_ARG, "scene / vert_grid is NULL");
    int rc = check_geom(geom_type);
    if (rc) return rc;
    Scene *sc = nullptr;
    if ((rc = scene_new(device, &sc))) return rc;
    rc = scene_build(sc, vert_grid, dem_dim_0, dem_dim_1, vert_simp, num_vert_simp, tri_ind_simp,
                     num_tri_simp, stats);
    if (rc) { scene_free(sc); return rc; }
    *scene = reinterpret_cast<hz_scene *>(sc);
    return HZ_OK;
}

int hz_scene_blob(const hz_scene *scene, void **device_ptr, size_t *nbytes) {
    if (!scene) return set_error(HZ_ERR_ARG, "scene is NULL");
    const Scene *sc = reinterpret_cast<const Scene *>(scene);
    if (device_ptr) *device_ptr = sc->blob;
    if (nbytes) *nbytes = sc->blob_bytes;
    return HZ_OK;
}

int hz_scene_vertices(const hz_scene *scene, const float **device_ptr, int *dem_dim_0, int *dem_dim_1, int *height_field) {
    if (!scene) return set_error(HZ_ERR_ARG, "scene is NULL");
    const Scene *sc = reinterpret_cast<const Scene *>(scene);
    if (device_ptr) *device_ptr = sc->verts();
    if (dem_dim_0) *dem_dim_0 = sc->hdr.d0;
    if (dem_dim_1) *dem_dim_1 = sc->hdr.d1;
    if (height_field) *height_field = (sc->hdr.flags & HZ_BLOB_HEIGHT_FIELD) ? 1 : 0;
    return HZ_OK;
}

int hz_scene_adopt(void *device_ptr, size_t nbytes, int device, hz_scene **scene) {
    if (!device_ptr || !scene || nbytes < sizeof(BlobHeader)) return set_error(HZ_ERR_ARG, "invalid blob");
    Scene *sc = nullptr;
    int rc = scene_new(device, &sc);
    if (rc) return rc;
    BlobHeader h;
    const hipError_t e = hipMemcpy(&h, device_ptr, sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { scene_free(sc); return set_error(HZ_ERR_HIP, "reading blob header failed: %s", hipGetErrorString(e)); }
    if (h.magic != HZ_BLOB_MAGIC || h.version != HZ_BLOB_VERSION || h.total_bytes > nbytes) {
        scene_free(sc);
        return set_error(HZ_ERR_ARG, "not a horayzon scene blob (magic/version/size mismatch)");
    }
    sc->blob = device_ptr; sc->blob_bytes = nbytes; sc->owns_blob = false; sc->hdr = h;
    *scene = reinterpret_cast<hz_scene *>(sc);
    return HZ_OK;
}

int hz_scene_destroy(hz_scene *scene) {
    scene_free(reinterpret_cast<Scene *>(scene));
    return HZ_OK;
}

static int topo_api(int kind, const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1,
                    int len_2, float *out, int device) {
    if (!azim || !hori || !out || (kind != 2 && !vec_tilt)) return set_error(HZ_ERR_ARG, "NULL argument");
    // (the openness reads no azim[1] - azim[0]: one azimuth is enough, as in hz_topo_params and the reference)
    if (len_0 <= 0 || len_1 <= 0 || len_2 < (kind == 2 ? 1 : 2)) return set_error(HZ_ERR_ARG, "Inconsistent/incorrect shapes of input arrays");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    const size_t ncell = (size_t)len_0 * len_1;
    DevIn<float> d_azim, d_hori, d_tilt;
    DevOut<float> d_out;
    if ((rc = d_azim.bind(azim, (size_t)len_2, st))) return rc;
    if ((rc = d_hori.bind(hori, ncell * (size_t)len_2, st))) return rc;
    if (kind != 2) if ((rc = d_tilt.bind(vec_tilt, ncell * 3, st))) return rc;
    if ((rc = d_out.bind(out, ncell))) return rc;
    if ((rc = topo_launch(kind, d_azim.dev, d_hori.dev, d_tilt.dev, len_0, len_1, len_2, d_out.dev, st))) return rc;
    if ((rc = d_out.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

int hz_sky_view_factor(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1,
                       int len_2, float *svf, int device) {
    return topo_api(0, azim, hori, vec_tilt, len_0, len_1, len_2, svf, device);
}
int hz_visible_sky_fraction(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1,
                            int len_2, float *vsf, int device) {
    return topo_api(1, azim, hori, vec_tilt, len_0, len_1, len_2, vsf, device);
}
int hz_topographic_openness(const float *azim, const float *hori, int len_0, int len_1, int len_2, float *top,
                            int device) {
    return topo_api(2, azim, hori, nullptr, len_0, len_1, len_2, top, device);
}

int hz_topo_params(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1, int len_2,
                   float *svf, float *vsf, float *openness, int device) {
    const bool tilt = svf || vsf;
    if (!svf && !vsf && !openness) return set_error(HZ_ERR_ARG, "no output requested (svf, vsf and openness are NULL)");
    if (!azim || !hori || (tilt && !vec_tilt)) return set_error(HZ_ERR_ARG, "NULL argument");
    if (len_0 <= 0 || len_1 <= 0 || len_2 < (tilt ? 2 : 1)) return set_error(HZ_ERR_ARG, "Inconsistent/incorrect shapes of input arrays");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    const size_t ncell = (size_t)len_0 * len_1;
    DevIn<float> d_azim, d_hori, d_tilt;
    DevOut<float> d_svf, d_vsf, d_open;
    if ((rc = d_azim.bind(azim, (size_t)len_2, st))) return rc;
    if ((rc = d_hori.bind(hori, ncell * (size_t)len_2, st))) return rc;
    if (tilt) if ((rc = d_tilt.bind(vec_tilt, ncell * 3, st))) return rc;
    if ((rc = d_svf.bind(svf, svf ? ncell : 0))) return rc;
    if ((rc = d_vsf.bind(vsf, vsf ? ncell : 0))) return rc;
    if ((rc = d_open.bind(openness, openness ? ncell : 0))) return rc;
    if ((rc = topo_multi_launch(d_azim.dev, d_hori.dev, d_tilt.dev, len_0, len_1, len_2, d_svf.dev, d_vsf.dev, d_open.dev, st)))
        return rc;
    if ((rc = d_svf.finish(st)) || (rc = d_vsf.finish(st)) || (rc = d_open.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

// ---------------------------------------------------------------------------------------
// the azimuth-major layout (hz_planes.hip): planes[k][y][x] and hori[y][x][k] hold the same 32-bit word
// ---------------------------------------------------------------------------------------
// Cells per staging chunk of the entry points below when a side is host memory (and rows of hz_topo_params_planes'
// cell-major buffer): 256 MiB of horizon, so the device never holds a second full copy.  hz_debug_set("planes_chunk", n).
static std::atomic<int> g_planes_chunk{0};
static size_t planes_chunk_cells(size_t cells, int azim_num) {
    const int knob = g_planes_chunk.load(std::memory_order_relaxed);
    size_t n = knob > 0 ? (size_t)knob : std::max<size_t>(64, (((size_t)256 << 20) / ((size_t)azim_num * sizeof(float))) & ~(size_t)63);
    return std::min(n, cells);
}

static int planes_check_shape(const void *a, const void *b, int len_0, int len_1, int len_2) {
    if (!a || !b) return set_error(HZ_ERR_ARG, "NULL argument");
    if (len_0 <= 0 || len_1 <= 0 || len_2 <= 0) return set_error(HZ_ERR_ARG, "Inconsistent/incorrect shapes of input arrays");
    if ((uint64_t)len_0 * (uint64_t)len_1 > (uint64_t)SIZE_MAX / ((uint64_t)len_2 * sizeof(float)))
        return set_error(HZ_ERR_ARG, "the horizon is too large");
    return HZ_OK;
}

struct DevScratch {
    void *p = nullptr;
    ~DevScratch() { if (p) (void)hipFree(p); }
};

// to_planes: hori -> planes, else planes -> hori; each side host or device memory, a host side goes through chunk buffers
static int planes_convert(bool to_planes, const float *src, float *dst, int len_0, int len_1, int len_2, int device) {
    int rc = planes_check_shape(src, dst, len_0, len_1, len_2);
    if (rc) return rc;
    if ((rc = select_device(device))) return rc;
    hipStream_t st = nullptr;
    const size_t cells = (size_t)len_0 * len_1, A = (size_t)len_2;
    const float *hori_c = to_planes ? src : nullptr, *planes_c = to_planes ? nullptr : src;
    float *hori = to_planes ? nullptr : dst, *planes = to_planes ? dst : nullptr;
    const bool hori_dev = is_device_ptr(to_planes ? (const void *)hori_c : (const void *)hori);
    const bool planes_dev = is_device_ptr(to_planes ? (const void *)planes : (const void *)planes_c);
    const size_t chunk = (hori_dev && planes_dev) ? cells : planes_chunk_cells(cells, len_2);
    DevScratch d_h, d_p;
    if (!hori_dev) HZ_HIP(hipMalloc(&d_h.p, chunk * A * sizeof(float)));
    if (!planes_dev) HZ_HIP(hipMalloc(&d_p.p, chunk * A * sizeof(float)));
    for (size_t c0 = 0; c0 < cells; c0 += chunk) {
        const size_t n = std::min(chunk, cells - c0);
        if (to_planes) {
            const float *h = hori_c + c0 * A;
            if (!hori_dev) { HZ_HIP(hipMemcpyAsync(d_h.p, h, n * A * sizeof(float), hipMemcpyHostToDevice, st)); h = (const float *)d_h.p; }
            if (planes_dev) rc = hori_to_planes_launch(h, n, len_2, planes, cells, c0, st);
            else {
                rc = hori_to_planes_launch(h, n, len_2, (float *)d_p.p, n, 0, st);
                if (!rc) HZ_HIP(hipMemcpy2DAsync(planes + c0, cells * sizeof(float), d_p.p, n * sizeof(float), n * sizeof(float), A,
                                                 hipMemcpyDeviceToHost, st));
            }
        } else {
            float *h = hori_dev ? hori + c0 * A : (float *)d_h.p;
            if (planes_dev) rc = planes_to_hori_launch(planes_c, cells, c0, n, len_2, h, st);
            else {
                HZ_HIP(hipMemcpy2DAsync(d_p.p, n * sizeof(float), planes_c + c0, cells * sizeof(float), n * sizeof(float), A,
                                        hipMemcpyHostToDevice, st));
                rc = planes_to_hori_launch((const float *)d_p.p, n, 0, n, len_2, h, st);
            }
            if (!rc && !hori_dev) HZ_HIP(hipMemcpyAsync(hori + c0 * A, h, n * A * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        HZ_HIP(hipStreamSynchronize(st));           // the chunk buffers are used again
    }
    return HZ_OK;
}

int hz_hori_to_planes(const float *hori, int len_0, int len_1, int len_2, float *planes, int device) {
    return planes_convert(true, hori, planes, len_0, len_1, len_2, device);
}

int hz_hori_from_planes(const float *planes, int len_0, int len_1, int len_2, float *hori, int device) {
    return planes_convert(false, planes, hori, len_0, len_1, len_2, device);
}

// ---------------------------------------------------------------------------------------
// the 16-bit horizon code (hz_q16.hip; DESIGN.md section 4, clause 15)
// ---------------------------------------------------------------------------------------
// Elements per staging chunk of hz_hori_quantise / hz_hori_dequantise when a side is host memory: 64 Mi elements (256 MiB of
// float32, 128 MiB of codes).  hz_debug_set("q16_chunk", n).
static std::atomic<int> g_q16_chunk{0};

// encode: src f32 -> dst u16, else src u16 -> dst f32; each side host or device memory, a host side goes through a chunk buffer
static int q16_convert(bool encode, const void *src, size_t n, void *dst, int device) {
    if (n == 0) return HZ_OK;
    if (!src || !dst) return set_error(HZ_ERR_ARG, "NULL argument");
    const size_t src_size = encode ? sizeof(float) : sizeof(uint16_t), dst_size = encode ? sizeof(uint16_t) : sizeof(float);
    if ((reinterpret_cast<uintptr_t>(src) & (src_size - 1)) || (reinterpret_cast<uintptr_t>(dst) & (dst_size - 1)))
        return set_error(HZ_ERR_ARG, "an array is not aligned to its element type");
    if (n > (size_t)SIZE_MAX / sizeof(float)) return set_error(HZ_ERR_ARG, "the horizon is too large");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    const bool src_dev = is_device_ptr(src), dst_dev = is_device_ptr(dst);
    const int knob = g_q16_chunk.load(std::memory_order_relaxed);
    const size_t chunk = (src_dev && dst_dev) ? n : std::min(n, knob > 0 ? (size_t)knob : (size_t)64 << 20);
    DevScratch d_src, d_dst;
    if (!src_dev) HZ_HIP(hipMalloc(&d_src.p, chunk * src_size));
    if (!dst_dev) HZ_HIP(hipMalloc(&d_dst.p, chunk * dst_size));
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        const char *in = static_cast<const char *>(src) + i0 * src_size;
        char *out = static_cast<char *>(dst) + i0 * dst_size;
        if (!src_dev) { HZ_HIP(hipMemcpyAsync(d_src.p, in, m * src_size, hipMemcpyHostToDevice, st)); in = static_cast<const char *>(d_src.p); }
        void *o = dst_dev ? (void *)out : d_dst.p;
        rc = encode ? hori_quantise_launch(reinterpret_cast<const float *>(in), m, static_cast<uint16_t *>(o), st)
                    : hori_dequantise_launch(reinterpret_cast<const uint16_t *>(in), m, static_cast<float *>(o), st);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        if (!dst_dev) HZ_HIP(hipMemcpyAsync(out, o, m * dst_size, hipMemcpyDeviceToHost, st));
        HZ_HIP(hipStreamSynchronize(st));           // the chunk buffers are used again
    }
    return HZ_OK;
}

int hz_hori_quantise(const float *src, size_t n, uint16_t *dst, int device) { return q16_convert(true, src, n, dst, device); }

int hz_hori_dequantise(const uint16_t *src, size_t n, float *dst, int device) { return q16_convert(false, src, n, dst, device); }

// hz_topo_params on planes: rows [rb, re) of every plane back into a bounded cell-major buffer (k_planes_to_hori), then the
// reduction launch hz_topo_params makes on it -- no numerics are written again, so every map is the same words
int hz_topo_params_planes(const float *azim, const float *planes, const float *vec_tilt, int len_0, int len_1, int len_2,
                          float *svf, float *vsf, float *openness, int device) {
    const bool tilt = svf || vsf;
    if (!svf && !vsf && !openness) return set_error(HZ_ERR_ARG, "no output requested (svf, vsf and openness are NULL)");
    if (!azim || !planes || (tilt && !vec_tilt)) return set_error(HZ_ERR_ARG, "NULL argument");
    if (len_0 <= 0 || len_1 <= 0 || len_2 < (tilt ? 2 : 1)) return set_error(HZ_ERR_ARG, "Inconsistent/incorrect shapes of input arrays");
    int rc = planes_check_shape(azim, planes, len_0, len_1, len_2);
    if (rc) return rc;
    if ((rc = select_device(device))) return rc;
    hipStream_t st = nullptr;
    const size_t ncell = (size_t)len_0 * len_1, A = (size_t)len_2;
    DevIn<float> d_azim, d_tilt;
    DevOut<float> d_svf, d_vsf, d_open;
    if ((rc = d_azim.bind(azim, A, st))) return rc;
    if (tilt) if ((rc = d_tilt.bind(vec_tilt, ncell * 3, st))) return rc;
    if ((rc = d_svf.bind(svf, svf ? ncell : 0))) return rc;
    if ((rc = d_vsf.bind(vsf, vsf ? ncell : 0))) return rc;
    if ((rc = d_open.bind(openness, openness ? ncell : 0))) return rc;
    const bool planes_dev = is_device_ptr(planes);
    const int rows = (int)std::max<size_t>(1, planes_chunk_cells(ncell, len_2) / (size_t)len_1);
    const size_t chunk = (size_t)rows * len_1;
    DevScratch d_h, d_p;
    HZ_HIP(hipMalloc(&d_h.p, chunk * A * sizeof(float)));
    if (!planes_dev) HZ_HIP(hipMalloc(&d_p.p, chunk * A * sizeof(float)));
    for (int rb = 0; rb < len_0; rb += rows) {
        const int re = std::min(rb + rows, len_0);
        const size_t c0 = (size_t)rb * len_1, n = (size_t)(re - rb) * len_1;
        if (planes_dev) rc = planes_to_hori_launch(planes, ncell, c0, n, len_2, (float *)d_h.p, st);
        else {
            HZ_HIP(hipMemcpy2DAsync(d_p.p, n * sizeof(float), planes + c0, ncell * sizeof(float), n * sizeof(float), A,
                                    hipMemcpyHostToDevice, st));
            rc = planes_to_hori_launch((const float *)d_p.p, n, 0, n, len_2, (float *)d_h.p, st);
        }
        if (!rc) rc = topo_multi_launch(d_azim.dev, (const float *)d_h.p, d_tilt.dev ? d_tilt.dev + 3 * c0 : nullptr, re - rb, len_1,
                                        len_2, d_svf.dev ? d_svf.dev + c0 : nullptr, d_vsf.dev ? d_vsf.dev + c0 : nullptr,
                                        d_open.dev ? d_open.dev + c0 : nullptr, st);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        HZ_HIP(hipStreamSynchronize(st));           // the chunk buffers are used again
    }
    if ((rc = d_svf.finish(st)) || (rc = d_vsf.finish(st)) || (rc = d_open.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

// ---------------------------------------------------------------------------------------
// test hooks for the build primitives (hz_sort.hip)
// ---------------------------------------------------------------------------------------
int hz_debug_sort_pairs(uint32_t *keys, uint32_t *vals, size_t n, int device) {
    if (!keys || !vals) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    void *dk = nullptr, *dv = nullptr, *dk2 = nullptr, *dv2 = nullptr, *tmp = nullptr;
    const size_t bytes = (n ? n : 1) * 4;
    HZ_HIP(hipMalloc(&dk, bytes)); HZ_HIP(hipMalloc(&dv, bytes)); HZ_HIP(hipMalloc(&dk2, bytes)); HZ_HIP(hipMalloc(&dv2, bytes));
    HZ_HIP(hipMalloc(&tmp, sort_temp_elems(n) * 4 + 16));
    HZ_HIP(hipMemcpy(dk, keys, n * 4, hipMemcpyHostToDevice));
    HZ_HIP(hipMemcpy(dv, vals, n * 4, hipMemcpyHostToDevice));
    rc = radix_sort_pairs_u32((uint32_t *)dk, (uint32_t *)dv, (uint32_t *)dk2, (uint32_t *)dv2, n, (uint32_t *)tmp, st);
    if (!rc) {
        HZ_HIP(hipStreamSynchronize(st));
        HZ_HIP(hipMemcpy(keys, dk, n * 4, hipMemcpyDeviceToHost));
        HZ_HIP(hipMemcpy(vals, dv, n * 4, hipMemcpyDeviceToHost));
    }
    (void)hipFree(dk); (void)hipFree(dv); (void)hipFree(dk2); (void)hipFree(dv2); (void)hipFree(tmp);
    return rc;
}

int hz_debug_exclusive_scan(const uint32_t *in, uint32_t *out, size_t n, int device) {
    if (!in || !out) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    void *di = nullptr, *dout = nullptr, *tmp = nullptr;
    const size_t bytes = (n ? n : 1) * 4;
    HZ_HIP(hipMalloc(&di, bytes)); HZ_HIP(hipMalloc(&dout, bytes)); HZ_HIP(hipMalloc(&tmp, scan_temp_elems(n) * 4 + 16));
    HZ_HIP(hipMemcpy(di, in, n * 4, hipMemcpyHostToDevice));
    rc = exclusive_scan_u32((const uint32_t *)di, (uint32_t *)dout, n, (uint32_t *)tmp, st);
    if (!rc) {
        HZ_HIP(hipStreamSynchronize(st));
        HZ_HIP(hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost));
    }
    (void)hipFree(di); (void)hipFree(dout); (void)hipFree(tmp);
    return rc;
}

int hz_debug_valu_peak(int device, int packed, int waves_per_simd, double *winst_per_s_per_simd,
                       double *clock_ghz, int *simds) {
    int rc = select_device(device);
    if (rc) return rc;
    return bench_valu_peak(packed, waves_per_simd, winst_per_s_per_simd, clock_ghz, simds);
}

int hz_debug_set(const char *key, int value) {
    if (!key) return hz::set_error(HZ_ERR_ARG, "hz_debug_set: null key");
    if (!strcmp(key, "shadow_fast_cap")) hz::g_shadow_fast_cap.store(value < 0 ? HZ_SHADOW_FAST_CAP_DEFAULT : value, std::memory_order_relaxed);
    else if (!strcmp(key, "topo_wide")) hz::g_topo_wide.store(value != 0, std::memory_order_relaxed);
    else if (!strcmp(key, "leaf_lend")) hz::g_leaf_lend.store(value != 0, std::memory_order_relaxed);      // (< 0: the default, on)
    else if (!strcmp(key, "flat_refill")) hz::g_flat_refill.store(value != 0, std::memory_order_relaxed);  // (< 0: the default, on)
    else if (!strcmp(key, "regroup_round")) hz::g_regroup_round.store((value < 0 || value > 63) ? HZ_REGROUP_ROUND : value, std::memory_order_relaxed);
    else if (!strcmp(key, "regroup_rule")) hz::g_regroup_rule.store(value != 0, std::memory_order_relaxed);  // (< 0: the default, relative)
    else if (!strcmp(key, "accum_chunk")) hz::g_accum_chunk.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    else if (!strcmp(key, "coarse_tile")) hz::g_coarse_tile.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    else if (!strcmp(key, "horisun_chunk")) hz::g_horisun_chunk.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    else if (!strcmp(key, "horisun_coarse_tile")) hz::g_horisun_coarse_tile.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    else if (!strcmp(key, "horisun_coarse_route")) hz::g_horisun_coarse_route.store(value < 0 ? -1 : (value == 1 ? 1 : 0), std::memory_order_relaxed);
    else if (!strcmp(key, "planes_chunk")) g_planes_chunk.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    else if (!strcmp(key, "q16_chunk")) g_q16_chunk.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    else if (!strcmp(key, "horidist_traversal")) {    // (< 0: the default; results never depend on it)
        if (value > 1) return hz::set_error(HZ_ERR_ARG, "hz_debug_set: horidist_traversal is 0 or 1");
        hz::g_horidist_traversal.store(value, std::memory_order_relaxed);
    }
    else if (!strcmp(key, "horidist_block_w")) {      // (< 0: the default, 8; results never depend on it)
        if (value >= 0 && value != 8 && value != 16 && value != 32 && value != 64)
            return hz::set_error(HZ_ERR_ARG, "hz_debug_set: horidist_block_w is 8, 16, 32 or 64");
        hz::g_horidist_block_w.store(value < 0 ? 8 : value, std::memory_order_relaxed);
    }
    else return hz::set_error(HZ_ERR_ARG, "hz_debug_set: unknown key '%s'", key);
    return HZ_OK;
}

int hz_debug_inst_rate(int device, int op, double *cycles_per_inst) {
    int rc = select_device(device);
    if (rc) return rc;
    return bench_inst_rate(op, cycles_per_inst);
}

int hz_debug_copy_peak(int device, size_t bytes, double *gbs) {
    int rc = select_device(device);
    if (rc) return rc;
    return bench_copy_peak(bytes, gbs);
}

// ---------------------------------------------------------------------------------------
// slope and input preparation (hz_prep.hip)
// ---------------------------------------------------------------------------------------
static int slope_api(int which, const float *x, const float *y, const float *z, int len_0, int len_1,
                     const float *rot_mat, int output_rot, float *vec_tilt, int device) {
    if (!x || !y || !z || !vec_tilt) return set_error(HZ_ERR_ARG, "NULL argument");
    if (len_0 <= 0 || len_1 <= 0) return set_error(HZ_ERR_ARG, "Inconsistent shapes / number of dimensions of input arrays");
    if (which == 1 && output_rot && !rot_mat) return set_error(HZ_ERR_ARG, "'rot_mat' must be provided for 'output_rot = True'");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    const size_t n = (size_t)len_0 * len_1;
    DevIn<float> dx, dy, dz, dr;
    DevOut<float> dt;
    if ((rc = dx.bind(x, n, st))) return rc;
    if ((rc = dy.bind(y, n, st))) return rc;
    if ((rc = dz.bind(z, n, st))) return rc;
    if ((rc = dr.bind(rot_mat, rot_mat ? n * 9 : 0, st))) return rc;
    if ((rc = dt.bind(vec_tilt, n * 3))) return rc;
    if ((rc = prep_slope(which, dx.dev, dy.dev, dz.dev, len_0, len_1, dr.dev, output_rot, dt.dev, st))) return rc;
    if ((rc = dt.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

int hz_slope_plane_meth(const float *x, const float *y, const float *z, int len_0, int len_1,
                        const float *rot_mat, int output_rot, float *vec_tilt, int device) {
    return slope_api(0, x, y, z, len_0, len_1, rot_mat, output_rot, vec_tilt, device);
}
int hz_slope_vector_meth(const float *x, const float *y, const float *z, int len_0, int len_1,
                         const float *rot_mat, int output_rot, float *vec_tilt, int device) {
    return slope_api(1, x, y, z, len_0, len_1, rot_mat, output_rot, vec_tilt, device);
}

static int check_ellps(int ellps) {
    if (ellps < 0 || ellps > 2) return set_error(HZ_ERR_ARG, "Unknown value for 'ellps'");
    return HZ_OK;
}

int hz_lonlat2ecef(const double *lon, const double *lat, const float *h, size_t n, int ellps, double *x_ecef,
                   double *y_ecef, double *z_ecef, int device) {
    if (!lon || !lat || !h || !x_ecef || !y_ecef || !z_ecef) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = check_ellps(ellps);
    if (rc) return rc;
    if ((rc = select_device(device))) return rc;
    hipStream_t st = nullptr;
    DevIn<double> dlon, dlat; DevIn<float> dh; DevOut<double> ox, oy, oz;
    if ((rc = dlon.bind(lon, n, st)) || (rc = dlat.bind(lat, n, st)) || (rc = dh.bind(h, n, st))) return rc;
    if ((rc = ox.bind(x_ecef, n)) || (rc = oy.bind(y_ecef, n)) || (rc = oz.bind(z_ecef, n))) return rc;
    if ((rc = prep_lonlat2ecef(ellps, dlon.dev, dlat.dev, dh.dev, n, ox.dev, oy.dev, oz.dev, st))) return rc;
    if ((rc = ox.finish(st)) || (rc = oy.finish(st)) || (rc = oz.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

int hz_wgs2swiss(const double *lon, const double *lat, const float *h_wgs, size_t n, double *e, double *no, float *h_ch,
                 int device) {
    if (!lon || !lat || !h_wgs || !e || !no || !h_ch) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    DevIn<double> da, db; DevIn<float> dh; DevOut<double> oa, ob; DevOut<float> oh;
    if ((rc = da.bind(lon, n, st)) || (rc = db.bind(lat, n, st)) || (rc = dh.bind(h_wgs, n, st))) return rc;
    if ((rc = oa.bind(e, n)) || (rc = ob.bind(no, n)) || (rc = oh.bind(h_ch, n))) return rc;
    if ((rc = prep_wgs2swiss(da.dev, db.dev, dh.dev, n, oa.dev, ob.dev, oh.dev, st))) return rc;
    if ((rc = oa.finish(st)) || (rc = ob.finish(st)) || (rc = oh.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

int hz_swiss2wgs(const double *e, const double *no, const float *h_ch, size_t n, double *lon, double *lat, float *h_wgs,
                 int device) {
    if (!e || !no || !h_ch || !lon || !lat || !h_wgs) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    DevIn<double> da, db; DevIn<float> dh; DevOut<double> oa, ob; DevOut<float> oh;
    if ((rc = da.bind(e, n, st)) || (rc = db.bind(no, n, st)) || (rc = dh.bind(h_ch, n, st))) return rc;
    if ((rc = oa.bind(lon, n)) || (rc = ob.bind(lat, n)) || (rc = oh.bind(h_wgs, n))) return rc;
    if ((rc = prep_swiss2wgs(da.dev, db.dev, dh.dev, n, oa.dev, ob.dev, oh.dev, st))) return rc;
    if ((rc = oa.finish(st)) || (rc = ob.finish(st)) || (rc = oh.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

int hz_ecef2enu(const double *x_ecef, const double *y_ecef, const double *z_ecef, size_t n, double lon_or,
                double lat_or, int ellps, float *x_enu, float *y_enu, float *z_enu, int device) {
    if (!x_ecef || !y_ecef || !z_ecef || !x_enu || !y_enu || !z_enu) return set_error(HZ_ERR_ARG, "NULL argument");
    if (lon_or < -180.0 || lon_or > 180.0) return set_error(HZ_ERR_ARG, "Value for 'lon_or' is outside of valid range");
    if (lat_or < -90.0 || lat_or > 90.0) return set_error(HZ_ERR_ARG, "Value for 'lat_or' is outside of valid range");
    int rc = check_ellps(ellps);
    if (rc) return rc;
    if ((rc = select_device(device))) return rc;
    hipStream_t st = nullptr;
    DevIn<double> dx, dy, dz; DevOut<float> ox, oy, oz;
    if ((rc = dx.bind(x_ecef, n, st)) || (rc = dy.bind(y_ecef, n, st)) || (rc = dz.bind(z_ecef, n, st))) return rc;
    if ((rc = ox.bind(x_enu, n)) || (rc = oy.bind(y_enu, n)) || (rc = oz.bind(z_enu, n))) return rc;
    if ((rc = prep_ecef2enu(ellps, lon_or, lat_or, dx.dev, dy.dev, dz.dev, n, ox.dev, oy.dev, oz.dev, st))) return rc;
    if ((rc = ox.finish(st)) || (rc = oy.finish(st)) || (rc = oz.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

int hz_ecef2enu_vector(const float *vec_ecef, size_t n, double lon_or, double lat_or, int ellps, float *vec_enu,
                       int device) {
    if (!vec_ecef || !vec_enu) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = check_ellps(ellps);
    if (rc) return rc;
    if ((rc = select_device(device))) return rc;
    hipStream_t st = nullptr;
    DevIn<float> dv; DevOut<float> dout;
    if ((rc = dv.bind(vec_ecef, n * 3, st)) || (rc = dout.bind(vec_enu, n * 3))) return rc;
    if ((rc = prep_ecef2enu_vector(ellps, lon_or, lat_or, dv.dev, n, dout.dev, st))) return rc;
    if ((rc = dout.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

int hz_surf_norm(const double *lon, const double *lat, size_t n, float *vec_norm_ecef, int device) {
    if (!lon || !lat || !vec_norm_ecef) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    DevIn<double> dlon, dlat; DevOut<float> dout;
    if ((rc = dlon.bind(lon, n, st)) || (rc = dlat.bind(lat, n, st)) || (rc = dout.bind(vec_norm_ecef, n * 3))) return rc;
    if ((rc = prep_surf_norm(dlon.dev, dlat.dev, n, dout.dev, st))) return rc;
    if ((rc = dout.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

int hz_north_dir(const double *x_ecef, const double *y_ecef, const double *z_ecef, const float *vec_norm_ecef,
                 size_t n, int ellps, float *vec_north_ecef, int device) {
    if (!x_ecef || !y_ecef || !z_ecef || !vec_norm_ecef || !vec_north_ecef) return set_error(HZ_ERR_ARG, "NULL argument");
    int rc = check_ellps(ellps);
    if (rc) return rc;
    if ((rc = select_device(device))) return rc;
    hipStream_t st = nullptr;
    DevIn<double> dx, dy, dz; DevIn<float> dn; DevOut<float> dout;
    if ((rc = dx.bind(x_ecef, n, st)) || (rc = dy.bind(y_ecef, n, st)) || (rc = dz.bind(z_ecef, n, st))) return rc;
    if ((rc = dn.bind(vec_norm_ecef, n * 3, st)) || (rc = dout.bind(vec_north_ecef, n * 3))) return rc;
    if ((rc = prep_north_dir(ellps, dx.dev, dy.dev, dz.dev, dn.dev, n, dout.dev, st))) return rc;
    if ((rc = dout.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

size_t hz_vert_grid_len(size_t num_vertices) {
    // pad_buffer (auxiliary.py:128-131): 16 extra elements, plus what makes the byte size a multiple of 16
    const size_t n3 = 3 * num_vertices;
    size_t add = 16;
    if ((n3 * 4) % 16 != 0) add += (16 - (n3 * 4) % 16) / 4;
    return n3 + add;
}

int hz_pack_vertices(const float *x, const float *y, const float *z, size_t num_vertices, float *vert_grid,
                     size_t vert_grid_len, int device) {
    if (!x || !y || !z || !vert_grid) return set_error(HZ_ERR_ARG, "NULL argument");
    if (vert_grid_len < hz_vert_grid_len(num_vertices))
        return set_error(HZ_ERR_ARG, "vert_grid is shorter than hz_vert_grid_len(num_vertices)");
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    DevIn<float> dx, dy, dz; DevOut<float> dout;
    if ((rc = dx.bind(x, num_vertices, st)) || (rc = dy.bind(y, num_vertices, st)) || (rc = dz.bind(z, num_vertices, st))) return rc;
    if ((rc = dout.bind(vert_grid, vert_grid_len))) return rc;
    if ((rc = prep_pack_vertices(dx.dev, dy.dev, dz.dev, num_vertices, vert_grid_len, dout.dev, st))) return rc;
    if ((rc = dout.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

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
    if (!t->counters) HZ_HIP(hipMalloc((void **)&t->counters, 16 * sizeof(unsigned long long)));
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

static int terrain_run(Terrain *t, const float *sun_positions, int num_sun, int which, uint8_t *out_u8,
                       float *out_f32, hz_stats *stats) {
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_position' has incorrect shape");
    if ((which == 0 && !out_u8) || (which == 1 && !out_f32)) return set_error(HZ_ERR_ARG, "output buffer is NULL");
    HZ_HIP(hipSetDevice(t->device));
    std::lock_guard<std::mutex> run_lock(t->scene->run_mu);
    hipStream_t st = t->stream;
    Timer t_total; t_total.start();
    const size_t nc = (size_t)t->dim_in_0 * t->dim_in_1;
    std::vector<float> sun((size_t)num_sun * 3);
    if (is_device_ptr(sun_positions)) HZ_HIP(hipMemcpy(sun.data(), sun_positions, sun.size() * 4, hipMemcpyDeviceToHost));
    else memcpy(sun.data(), sun_positions, sun.size() * 4);
    DevOut<uint8_t> d_u8; DevOut<float> d_f32;
    int rc;
    if (which == 0) { if ((rc = d_u8.bind(out_u8, nc * (size_t)num_sun))) return rc; }
    else { if ((rc = d_f32.bind(out_f32, nc * (size_t)num_sun))) return rc; }
    ShadowArgs a = terrain_args(t, which);
    float ms = 0.0f;
    unsigned long long cnt[16];
    {
        // the sun positions go to the device once; one launch computes up to 32768 of them (grid.y)
        if (t->sun_cap < sun.size()) {
            if (t->sun_dev) (void)hipFree(t->sun_dev);
            t->sun_dev = nullptr; t->sun_cap = 0;
            const size_t cap = std::max<size_t>(sun.size(), 3 * 256);
            HZ_HIP(hipMalloc((void **)&t->sun_dev, cap * sizeof(float)));
            t->sun_cap = cap;
        }
        HZ_HIP(hipMemcpyAsync(t->sun_dev, sun.data(), sun.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HZ_HIP(hipMemsetAsync(t->counters, 0, 16 * sizeof(unsigned long long), st));
        hipEvent_t e0, e1;
        HZ_HIP(hipEventCreate(&e0)); HZ_HIP(hipEventCreate(&e1));
        HZ_HIP(hipEventRecord(e0, st));
        for (int s0 = 0; s0 < num_sun; s0 += 32768) {
            a.suns = t->sun_dev + 3 * (size_t)s0;
            a.num_sun = std::min(32768, num_sun - s0);
            a.out_u8 = d_u8.dev ? d_u8.dev + nc * (size_t)s0 : nullptr;
            a.out_f32 = d_f32.dev ? d_f32.dev + nc * (size_t)s0 : nullptr;
            if ((rc = shadow_launch(t->scene, a, st))) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return rc; }
        }
        HZ_HIP(hipEventRecord(e1, st));
        HZ_HIP(hipEventSynchronize(e1));
        HZ_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        HZ_HIP(hipMemcpyAsync(cnt, t->counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HZ_HIP(hipStreamSynchronize(st));
    }
    Timer t_d2h; t_d2h.start();
    if ((rc = d_u8.finish(st))) return rc;
    if ((rc = d_f32.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    if (stats) {
        stats->num_rays += cnt[0];
        stats->nodes_visited += cnt[1]; stats->tris_tested += cnt[2];
        stats->wave_node_iters += cnt[3]; stats->wave_leaf_iters += cnt[4];
        stats->t_kernel_s += (double)ms * 1e-3;
        stats->t_d2h_s += t_d2h.stop();
        stats->t_total_s += t_total.stop();
        stats->bvh_height = t->scene->hdr.height; stats->scene_bytes = t->scene->hdr.total_bytes;
    }
    return HZ_OK;
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

int hz_terrain_accumulate(hz_terrain *terrain, const float *sun_positions, const float *weights, int num_sun,
                          float *sw_dir_cor_sum, float *sunlit_sum, hz_stats *stats) {
    Terrain *t = reinterpret_cast<Terrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "Terrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_positions' has incorrect shape");
    if (!sw_dir_cor_sum && !sunlit_sum) return set_error(HZ_ERR_ARG, "no output buffer (sw_dir_cor_sum and sunlit_sum are NULL)");
    HZ_HIP(hipSetDevice(t->device));
    std::lock_guard<std::mutex> run_lock(t->scene->run_mu);
    hipStream_t st = t->stream;
    Timer t_total; t_total.start();
    const size_t nc = (size_t)t->dim_in_0 * t->dim_in_1;
    const bool want_sw = sw_dir_cor_sum != nullptr, want_lit = sunlit_sum != nullptr;
    // the sunlit sum needs the shadow code (which = 0: the shadow ray set); the correction alone traces its own, smaller set
    ShadowArgs a = terrain_args(t, want_lit ? 0 : 1);
    int k = g_accum_chunk.load(std::memory_order_relaxed);       // (hz_debug_set("accum_chunk", k): tests)
    if (k <= 0) {
        size_t free_b = 0, total_b = 0;
        HZ_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t budget = std::min<size_t>(HZ_ACCUM_BUDGET, free_b / 4);
        const size_t per_pos = nc * ((want_lit ? 1 : 0) + (want_sw ? 4 : 0));
        k = (int)std::max<size_t>(1, std::min<size_t>(HZ_ACCUM_CHUNK_MAX, budget / per_pos));
    }
    k = std::min(k, 32768);                                       // grid.y of one launch
    const bool sun_on_dev = is_device_ptr(sun_positions), w_on_dev = weights && is_device_ptr(weights);
    DevScratch codes, vals, acc, stage;
    size_t scratch = 0;
    if (want_lit) { HZ_HIP(hipMalloc(&codes.p, (size_t)k * nc)); scratch += (size_t)k * nc; }
    if (want_sw) { HZ_HIP(hipMalloc(&vals.p, (size_t)k * nc * 4)); scratch += (size_t)k * nc * 4; }
    const size_t n_acc = (want_sw ? 1 : 0) + (want_lit ? 1 : 0);
    HZ_HIP(hipMalloc(&acc.p, n_acc * nc * sizeof(double))); scratch += n_acc * nc * sizeof(double);
    double *acc_sw = want_sw ? static_cast<double *>(acc.p) : nullptr;
    double *acc_lit = want_lit ? static_cast<double *>(acc.p) + (want_sw ? nc : 0) : nullptr;
    float *stage_sun = nullptr, *stage_w = nullptr;             // host positions / weights go up one chunk at a time
    if (!sun_on_dev || (weights && !w_on_dev)) {
        HZ_HIP(hipMalloc(&stage.p, (size_t)k * 4 * sizeof(float))); scratch += (size_t)k * 4 * sizeof(float);
        stage_sun = static_cast<float *>(stage.p); stage_w = stage_sun + 3 * (size_t)k;
    }
    DevOut<float> d_sw, d_lit;
    int rc;
    if ((rc = d_sw.bind(sw_dir_cor_sum, want_sw ? nc : 0))) return rc;
    if ((rc = d_lit.bind(sunlit_sum, want_lit ? nc : 0))) return rc;
    if (d_sw.owned) scratch += nc * sizeof(float);
    if (d_lit.owned) scratch += nc * sizeof(float);
    float ms = 0.0f;
    unsigned long long cnt[16];
    {
        HZ_HIP(hipMemsetAsync(acc.p, 0, n_acc * nc * sizeof(double), st));
        HZ_HIP(hipMemsetAsync(t->counters, 0, 16 * sizeof(unsigned long long), st));
        hipEvent_t e0, e1;
        HZ_HIP(hipEventCreate(&e0)); HZ_HIP(hipEventCreate(&e1));
        struct EvFree { hipEvent_t a, b; ~EvFree() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev_free{e0, e1};
        HZ_HIP(hipEventRecord(e0, st));
        a.out_u8 = static_cast<uint8_t *>(codes.p);
        a.out_f32 = static_cast<float *>(vals.p);
        for (int s0 = 0; s0 < num_sun; s0 += k) {
            const int kc = std::min(k, num_sun - s0);
            if (sun_on_dev) a.suns = sun_positions + 3 * (size_t)s0;
            else {
                HZ_HIP(hipMemcpyAsync(stage_sun, sun_positions + 3 * (size_t)s0, (size_t)kc * 3 * sizeof(float), hipMemcpyHostToDevice, st));
                a.suns = stage_sun;
            }
            const float *w = nullptr;
            if (weights && w_on_dev) w = weights + s0;
            else if (weights) {
                HZ_HIP(hipMemcpyAsync(stage_w, weights + s0, (size_t)kc * sizeof(float), hipMemcpyHostToDevice, st));
                w = stage_w;
            }
            a.num_sun = kc;
            if ((rc = accum_trace_launch(t->scene, a, want_sw && want_lit, st))) return rc;
            if ((rc = accum_add_launch(a.out_u8, a.out_f32, nc, kc, w, acc_sw, acc_lit, st))) return rc;
        }
        if ((rc = accum_final_launch(a.mask, nc, t->fill, acc_sw, acc_lit, d_sw.dev, d_lit.dev, st))) return rc;
        HZ_HIP(hipEventRecord(e1, st));
        HZ_HIP(hipEventSynchronize(e1));
        HZ_HIP(hipEventElapsedTime(&ms, e0, e1));
        HZ_HIP(hipMemcpyAsync(cnt, t->counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HZ_HIP(hipStreamSynchronize(st));
    }
    Timer t_d2h; t_d2h.start();
    if ((rc = d_sw.finish(st))) return rc;
    if ((rc = d_lit.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    if (stats) {
        stats->num_rays += cnt[0];
        stats->nodes_visited += cnt[1]; stats->tris_tested += cnt[2];
        stats->wave_node_iters += cnt[3]; stats->wave_leaf_iters += cnt[4];
        stats->t_kernel_s += (double)ms * 1e-3;
        stats->t_d2h_s += t_d2h.stop();
        stats->t_total_s += t_total.stop();
        stats->bvh_height = t->scene->hdr.height; stats->scene_bytes = t->scene->hdr.total_bytes;
        stats->scratch_bytes = scratch;
    }
    return HZ_OK;
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
    if (p0 < 1 || p1 < 1 || p0 > t->dim_in_0 || p1 > t->dim_in_1 || t->dim_in_0 % p0 || t->dim_in_1 % p1)
        return set_error(HZ_ERR_ARG, "'pixel_per_gc' (%d, %d) must be positive and divide the inner domain (%d, %d)", p0, p1,
                         t->dim_in_0, t->dim_in_1);
    HZ_HIP(hipSetDevice(t->device));
    std::lock_guard<std::mutex> run_lock(t->scene->run_mu);
    hipStream_t st = t->stream;
    Timer t_total; t_total.start();
    const size_t nc = (size_t)t->dim_in_0 * t->dim_in_1;
    const int gy = t->dim_in_0 / p0, gx = t->dim_in_1 / p1;
    const size_t ng = (size_t)gy * gx;
    const bool want_sw = f_cor != nullptr, want_lit = sunlit_frac != nullptr;
    // the sunlit fraction needs the shadow code (which = 0: the shadow ray set); the correction alone traces its own, smaller set
    ShadowArgs a = terrain_args(t, want_lit ? 0 : 1);
    int k = g_accum_chunk.load(std::memory_order_relaxed);       // (hz_debug_set("accum_chunk", k): tests)
    if (k <= 0) {
        size_t free_b = 0, total_b = 0;
        HZ_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t budget = std::min<size_t>(HZ_ACCUM_BUDGET, free_b / 4);
        const size_t per_pos = nc * ((want_lit ? 1 : 0) + (want_sw ? 4 : 0));
        k = (int)std::max<size_t>(1, std::min<size_t>(HZ_ACCUM_CHUNK_MAX, budget / per_pos));
    }
    k = std::min(k, 32768);                                       // grid.y of one launch
    const bool sun_on_dev = is_device_ptr(sun_positions);
    DevScratch codes, vals, count, stage;
    size_t scratch = 0;
    if (want_lit) { HZ_HIP(hipMalloc(&codes.p, (size_t)k * nc)); scratch += (size_t)k * nc; }
    if (want_sw) { HZ_HIP(hipMalloc(&vals.p, (size_t)k * nc * 4)); scratch += (size_t)k * nc * 4; }
    HZ_HIP(hipMalloc(&count.p, ng * sizeof(unsigned))); scratch += ng * sizeof(unsigned);
    if (!sun_on_dev) { HZ_HIP(hipMalloc(&stage.p, (size_t)k * 3 * sizeof(float))); scratch += (size_t)k * 3 * sizeof(float); }
    float *stage_sun = static_cast<float *>(stage.p);           // host positions go up one chunk at a time
    DevOut<float> d_sw, d_lit;
    int rc;
    if ((rc = d_sw.bind(f_cor, want_sw ? ng * (size_t)num_sun : 0))) return rc;
    if ((rc = d_lit.bind(sunlit_frac, want_lit ? ng * (size_t)num_sun : 0))) return rc;
    float ms = 0.0f;
    unsigned long long cnt[16];
    {
        HZ_HIP(hipMemsetAsync(t->counters, 0, 16 * sizeof(unsigned long long), st));
        hipEvent_t e0, e1;
        HZ_HIP(hipEventCreate(&e0)); HZ_HIP(hipEventCreate(&e1));
        struct EvFree { hipEvent_t a, b; ~EvFree() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev_free{e0, e1};
        HZ_HIP(hipEventRecord(e0, st));
        if ((rc = coarse_count_launch(a.mask, t->dim_in_0, t->dim_in_1, p0, p1, static_cast<unsigned *>(count.p), st))) return rc;
        a.out_u8 = static_cast<uint8_t *>(codes.p);
        a.out_f32 = static_cast<float *>(vals.p);
        for (int s0 = 0; s0 < num_sun; s0 += k) {
            const int kc = std::min(k, num_sun - s0);
            if (sun_on_dev) a.suns = sun_positions + 3 * (size_t)s0;
            else {
                HZ_HIP(hipMemcpyAsync(stage_sun, sun_positions + 3 * (size_t)s0, (size_t)kc * 3 * sizeof(float), hipMemcpyHostToDevice, st));
                a.suns = stage_sun;
            }
            a.num_sun = kc;
            if ((rc = accum_trace_launch(t->scene, a, want_sw && want_lit, st))) return rc;
            if ((rc = coarse_reduce_launch(a.out_u8, a.out_f32, a.mask, static_cast<const unsigned *>(count.p), t->dim_in_0,
                                           t->dim_in_1, p0, p1, kc, t->fill, d_sw.dev ? d_sw.dev + ng * (size_t)s0 : nullptr,
                                           d_lit.dev ? d_lit.dev + ng * (size_t)s0 : nullptr, st)))
                return rc;
        }
        HZ_HIP(hipEventRecord(e1, st));
        HZ_HIP(hipEventSynchronize(e1));
        HZ_HIP(hipEventElapsedTime(&ms, e0, e1));
        HZ_HIP(hipMemcpyAsync(cnt, t->counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HZ_HIP(hipStreamSynchronize(st));
    }
    Timer t_d2h; t_d2h.start();
    if ((rc = d_sw.finish(st))) return rc;
    if ((rc = d_lit.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    if (stats) {
        stats->num_rays += cnt[0];
        stats->nodes_visited += cnt[1]; stats->tris_tested += cnt[2];
        stats->wave_node_iters += cnt[3]; stats->wave_leaf_iters += cnt[4];
        stats->t_kernel_s += (double)ms * 1e-3;
        stats->t_d2h_s += t_d2h.stop();
        stats->t_total_s += t_total.stop();
        stats->bvh_height = t->scene->hdr.height; stats->scene_bytes = t->scene->hdr.total_bytes;
        stats->scratch_bytes = scratch;
    }
    return HZ_OK;
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
        DevScratch elev, fac;
        int rc;
        if ((rc = horisun_copy(elevation, nc * sizeof(float), st, &elev.p))) return rc;
        HZ_HIP(hipMalloc(&fac.p, nc * sizeof(double)));
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

int hz_horizon_terrain_run(hz_horizon_terrain *terrain, const float *sun_positions, const float *weights, int num_sun,
                           const hz_horisun_out *out, hz_stats *stats) {
    HorizonTerrain *t = reinterpret_cast<HorizonTerrain *>(terrain);
    if (!t || !t->initialised) return set_error(HZ_ERR_ARG, "HorizonTerrain is not initialised");
    if (!sun_positions || num_sun <= 0) return set_error(HZ_ERR_ARG, "array 'sun_positions' has incorrect shape");
    if (!out || out->size != (int32_t)sizeof(hz_horisun_out))
        return set_error(HZ_ERR_ARG, "hz_horisun_out.size is %d, expected %d", out ? (int)out->size : 0, (int)sizeof(hz_horisun_out));
    const void *outs[4] = {out->shadow, out->sw_dir_cor, out->sw_dir_cor_sum, out->sunlit_sum};
    if (!outs[0] && !outs[1] && !outs[2] && !outs[3]) return set_error(HZ_ERR_ARG, "no output buffer (every pointer of hz_horisun_out is NULL)");
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (outs[i] && outs[i] == outs[j]) return set_error(HZ_ERR_ARG, "the outputs must be different arrays");
    const bool want_sums = out->sw_dir_cor_sum || out->sunlit_sum;
    HorisunPlan plan;
    if (horisun_plan(t->dim_in_0, t->dim_in_1, t->azim_num, num_sun, g_horisun_chunk.load(std::memory_order_relaxed),
                     (out->shadow ? 1 : 0) + (out->sw_dir_cor ? 4 : 0), &plan))
        return set_error(HZ_ERR_ARG, "too many sun positions for the per-position outputs");
    std::lock_guard<std::mutex> run_lock(t->run_mu);
    HZ_HIP(hipSetDevice(t->device));
    hipStream_t st = t->stream;
    Timer t_total; t_total.start();
    const size_t nc = plan.cells;
    const int k = plan.chunk;
    const bool sun_on_dev = is_device_ptr(sun_positions);
    const bool use_w = weights && want_sums, w_on_dev = use_w && is_device_ptr(weights);
    DevScratch acc, stage;
    size_t scratch = 0;
    // the sums live in registers during a launch and in two float64 maps between the launches of a call
    const size_t n_acc = (out->sw_dir_cor_sum ? 1 : 0) + (out->sunlit_sum ? 1 : 0);
    if (n_acc) { HZ_HIP(hipMalloc(&acc.p, n_acc * nc * sizeof(double))); scratch += n_acc * nc * sizeof(double); }
    float *stage_sun = nullptr, *stage_w = nullptr;              // host positions / weights go up one chunk at a time
    if (!sun_on_dev || (use_w && !w_on_dev)) {
        HZ_HIP(hipMalloc(&stage.p, (size_t)k * 4 * sizeof(float))); scratch += (size_t)k * 4 * sizeof(float);
        stage_sun = static_cast<float *>(stage.p); stage_w = stage_sun + 3 * (size_t)k;
    }
    DevOut<uint8_t> d_u8; DevOut<float> d_f32, d_sw, d_lit;
    int rc;
    if ((rc = d_u8.bind(out->shadow, out->shadow ? nc * (size_t)num_sun : 0))) return rc;
    if ((rc = d_f32.bind(out->sw_dir_cor, out->sw_dir_cor ? nc * (size_t)num_sun : 0))) return rc;
    if ((rc = d_sw.bind(out->sw_dir_cor_sum, out->sw_dir_cor_sum ? nc : 0))) return rc;
    if ((rc = d_lit.bind(out->sunlit_sum, out->sunlit_sum ? nc : 0))) return rc;
    if (d_sw.owned) scratch += nc * sizeof(float);
    if (d_lit.owned) scratch += nc * sizeof(float);
    HorisunArgs a;
    a.hori = t->hori; a.vert = (const float *)t->vert;
    a.vec_tilt = (const float *)t->tilt; a.vec_norm = (const float *)t->norm; a.vec_north = (const float *)t->north;
    a.surf_enl_fac = (const float *)t->enl; a.mask = (const uint8_t *)t->mask;
    a.cells = nc; a.azim_num = t->azim_num;
    a.fill = t->fill; a.dot_prod_min = cosf(deg2rad_f(t->ang_max));            // shadow_comp.cpp:498
    a.refrac_fac = t->refrac_fac;
    a.acc_sw = out->sw_dir_cor_sum ? static_cast<double *>(acc.p) : nullptr;
    a.acc_lit = out->sunlit_sum ? static_cast<double *>(acc.p) + (out->sw_dir_cor_sum ? nc : 0) : nullptr;
    a.sum_sw = d_sw.dev; a.sum_lit = d_lit.dev;
    float ms = 0.0f;
    {
        hipEvent_t e0, e1;
        HZ_HIP(hipEventCreate(&e0)); HZ_HIP(hipEventCreate(&e1));
        struct EvFree { hipEvent_t a, b; ~EvFree() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev_free{e0, e1};
        HZ_HIP(hipEventRecord(e0, st));
        for (int c = 0; c < plan.num_chunks; c++) {
            int s0 = 0, kc = 0;
            horisun_chunk(plan, num_sun, c, &s0, &kc);
            if (sun_on_dev) a.suns = sun_positions + 3 * (size_t)s0;
            else {
                HZ_HIP(hipMemcpyAsync(stage_sun, sun_positions + 3 * (size_t)s0, (size_t)kc * 3 * sizeof(float), hipMemcpyHostToDevice, st));
                a.suns = stage_sun;
            }
            a.weights = nullptr;
            if (use_w && w_on_dev) a.weights = weights + s0;
            else if (use_w) {
                HZ_HIP(hipMemcpyAsync(stage_w, weights + s0, (size_t)kc * sizeof(float), hipMemcpyHostToDevice, st));
                a.weights = stage_w;
            }
            a.num_sun = kc;
            a.out_u8 = d_u8.dev ? d_u8.dev + nc * (size_t)s0 : nullptr;
            a.out_f32 = d_f32.dev ? d_f32.dev + nc * (size_t)s0 : nullptr;
            a.first = c == 0; a.last = c == plan.num_chunks - 1;
            // planes: the same launch plan, the horizon read as planes[k * cells + c] (k_horisun_planes, hz_planes.hip)
            if ((rc = t->planes ? horisun_planes_launch(a, nc, plan.blocks, st, t->q16) : horisun_launch(a, plan.blocks, st, t->q16))) return rc;
        }
        HZ_HIP(hipEventRecord(e1, st));
        HZ_HIP(hipEventSynchronize(e1));
        HZ_HIP(hipEventElapsedTime(&ms, e0, e1));
    }
    Timer t_d2h; t_d2h.start();
    if ((rc = d_u8.finish(st))) return rc;
    if ((rc = d_f32.finish(st))) return rc;
    if ((rc = d_sw.finish(st))) return rc;
    if ((rc = d_lit.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    if (stats) {
        stats->num_cells = nc;
        stats->t_kernel_s += (double)ms * 1e-3;
        stats->t_d2h_s += t_d2h.stop();
        stats->t_total_s += t_total.stop();
        stats->scratch_bytes = scratch;
    }
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
    if (p0 < 1 || p1 < 1 || p0 > t->dim_in_0 || p1 > t->dim_in_1 || t->dim_in_0 % p0 || t->dim_in_1 % p1)
        return set_error(HZ_ERR_ARG, "'pixel_per_gc' (%d, %d) must be positive and divide the inner domain (%d, %d)", p0, p1,
                         t->dim_in_0, t->dim_in_1);
    const bool want_sw = f_cor != nullptr, want_lit = sunlit_frac != nullptr;
    HorisunPlan plan;
    if (horisun_plan(t->dim_in_0, t->dim_in_1, t->azim_num, num_sun, g_horisun_chunk.load(std::memory_order_relaxed), 0, &plan))
        return set_error(HZ_ERR_ARG, "too many sun positions");
    const int k = std::min(plan.chunk, HZ_HSC_CHUNK_MAX);        // grid.y of either route
    HorisunCoarsePlan cp;
    int rc;
    if ((rc = horisun_coarse_plan_for(t->dim_in_0, t->dim_in_1, p0, p1, k, t->planes, want_lit, want_sw, &cp))) return rc;
    if (t->q16) cp.fallback = 1;      // codes: always the two-pass route, whatever "horisun_coarse_route" says (no fused kernel reads them)
    const size_t nc = plan.cells;
    const int gy = t->dim_in_0 / p0, gx = t->dim_in_1 / p1;
    const size_t ng = (size_t)gy * gx;
    if (ng > (size_t)SIZE_MAX / sizeof(float) / (size_t)num_sun) return set_error(HZ_ERR_ARG, "too many sun positions");
    std::lock_guard<std::mutex> run_lock(t->run_mu);
    HZ_HIP(hipSetDevice(t->device));
    hipStream_t st = t->stream;
    Timer t_total; t_total.start();
    const bool sun_on_dev = is_device_ptr(sun_positions);
    DevScratch codes, vals, count, stage;
    size_t scratch = 0;
    if (cp.fallback) {
        if (want_lit) { HZ_HIP(hipMalloc(&codes.p, (size_t)k * nc)); scratch += (size_t)k * nc; }
        if (want_sw) { HZ_HIP(hipMalloc(&vals.p, (size_t)k * nc * 4)); scratch += (size_t)k * nc * 4; }
    }
    HZ_HIP(hipMalloc(&count.p, ng * sizeof(unsigned))); scratch += ng * sizeof(unsigned);
    if (!sun_on_dev) { HZ_HIP(hipMalloc(&stage.p, (size_t)k * 3 * sizeof(float))); scratch += (size_t)k * 3 * sizeof(float); }
    float *stage_sun = static_cast<float *>(stage.p);           // host positions go up one chunk at a time
    DevOut<float> d_sw, d_lit;
    if ((rc = d_sw.bind(f_cor, want_sw ? ng * (size_t)num_sun : 0))) return rc;
    if ((rc = d_lit.bind(sunlit_frac, want_lit ? ng * (size_t)num_sun : 0))) return rc;
    HorisunArgs a;
    a.hori = t->hori; a.vert = (const float *)t->vert;
    a.vec_tilt = (const float *)t->tilt; a.vec_norm = (const float *)t->norm; a.vec_north = (const float *)t->north;
    a.surf_enl_fac = (const float *)t->enl; a.mask = (const uint8_t *)t->mask;
    a.cells = nc; a.azim_num = t->azim_num;
    a.fill = t->fill; a.dot_prod_min = cosf(deg2rad_f(t->ang_max));            // shadow_comp.cpp:498
    a.refrac_fac = t->refrac_fac;
    a.weights = nullptr; a.acc_sw = a.acc_lit = nullptr; a.sum_sw = a.sum_lit = nullptr;
    a.first = a.last = 1;
    a.out_u8 = static_cast<uint8_t *>(codes.p);
    a.out_f32 = static_cast<float *>(vals.p);
    float ms = 0.0f;
    {
        hipEvent_t e0, e1;
        HZ_HIP(hipEventCreate(&e0)); HZ_HIP(hipEventCreate(&e1));
        struct EvFree { hipEvent_t a, b; ~EvFree() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev_free{e0, e1};
        HZ_HIP(hipEventRecord(e0, st));
        const unsigned *n = static_cast<const unsigned *>(count.p);
        if ((rc = coarse_count_launch(a.mask, t->dim_in_0, t->dim_in_1, p0, p1, static_cast<unsigned *>(count.p), st))) return rc;
        for (int s0 = 0; s0 < num_sun; s0 += k) {
            const int kc = std::min(k, num_sun - s0);
            if (sun_on_dev) a.suns = sun_positions + 3 * (size_t)s0;
            else {
                HZ_HIP(hipMemcpyAsync(stage_sun, sun_positions + 3 * (size_t)s0, (size_t)kc * 3 * sizeof(float), hipMemcpyHostToDevice, st));
                a.suns = stage_sun;
            }
            a.num_sun = kc;
            float *o_sw = d_sw.dev ? d_sw.dev + ng * (size_t)s0 : nullptr, *o_lit = d_lit.dev ? d_lit.dev + ng * (size_t)s0 : nullptr;
            if (cp.fallback) {
                if ((rc = t->planes ? horisun_planes_launch(a, nc, plan.blocks, st, t->q16) : horisun_launch(a, plan.blocks, st, t->q16))) return rc;
                if ((rc = coarse_reduce_launch(a.out_u8, a.out_f32, a.mask, n, t->dim_in_0, t->dim_in_1, p0, p1, kc, t->fill,
                                               o_sw, o_lit, st)))
                    return rc;
            } else if ((rc = horisun_coarse_launch(a, t->planes, nc, cp, n, t->dim_in_1, p0, p1, o_sw, o_lit, st))) return rc;
        }
        HZ_HIP(hipEventRecord(e1, st));
        HZ_HIP(hipEventSynchronize(e1));
        HZ_HIP(hipEventElapsedTime(&ms, e0, e1));
    }
    Timer t_d2h; t_d2h.start();
    if ((rc = d_sw.finish(st))) return rc;
    if ((rc = d_lit.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    if (stats) {
        stats->num_cells = nc;
        stats->t_kernel_s += (double)ms * 1e-3;
        stats->t_d2h_s += t_d2h.stop();
        stats->t_total_s += t_total.stop();
        stats->scratch_bytes = scratch;
    }
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
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (outs[i] && outs[i] == outs[j]) return set_error(HZ_ERR_ARG, "the outputs must be different arrays");
    HorisunPlan plan;
    if (horisun_plan(t->dim_in_0, t->dim_in_1, t->azim_num, num_sun, g_horisun_chunk.load(std::memory_order_relaxed), 0, &plan))
        return set_error(HZ_ERR_ARG, "too many sun positions");
    std::lock_guard<std::mutex> run_lock(t->run_mu);
    HZ_HIP(hipSetDevice(t->device));
    hipStream_t st = t->stream;
    Timer t_total; t_total.start();
    const bool sun_on_dev = is_device_ptr(sun_positions), times_on_dev = is_device_ptr(times);
    // the times on the host: they are checked here, and the one before each chunk is a kernel argument
    std::vector<double> times_down;
    const double *times_host = times;
    if (times_on_dev) {
        times_down.resize((size_t)num_sun);
        HZ_HIP(hipMemcpy(times_down.data(), times, (size_t)num_sun * sizeof(double), hipMemcpyDeviceToHost));
        times_host = times_down.data();
    }
    for (int s = 0; s < num_sun; s++)
        if (!std::isfinite(times_host[s]) || (s > 0 && !(times_host[s] > times_host[s - 1])))
            return set_error(HZ_ERR_ARG, "'times' must be finite and strictly increasing (times[%d])", s);
    const size_t nc = plan.cells;
    const int k = plan.chunk;
    DevScratch state, stage;
    size_t scratch = 0;
    if (plan.num_chunks > 1) { HZ_HIP(hipMalloc(&state.p, suntimes_state_bytes(nc))); scratch += suntimes_state_bytes(nc); }
    double *stage_times = nullptr; float *stage_sun = nullptr;   // host times / positions go up one chunk at a time
    if (!sun_on_dev || !times_on_dev) {
        HZ_HIP(hipMalloc(&stage.p, (size_t)k * (sizeof(double) + 3 * sizeof(float)))); scratch += (size_t)k * (sizeof(double) + 3 * sizeof(float));
        stage_times = static_cast<double *>(stage.p); stage_sun = reinterpret_cast<float *>(stage_times + k);
    }
    DevOut<float> d_rise, d_set, d_dur; DevOut<int32_t> d_n;
    int rc;
    if ((rc = d_rise.bind(out->sunrise, out->sunrise ? nc : 0))) return rc;
    if ((rc = d_set.bind(out->sunset, out->sunset ? nc : 0))) return rc;
    if ((rc = d_dur.bind(out->duration, out->duration ? nc : 0))) return rc;
    if ((rc = d_n.bind(out->intervals, out->intervals ? nc : 0))) return rc;
    for (const void *owned : {d_rise.owned, d_set.owned, d_dur.owned, d_n.owned})
        if (owned) scratch += nc * 4;
    SuntimesArgs a;
    a.hori = t->hori; a.stride = nc; a.vert = (const float *)t->vert;
    a.vec_tilt = (const float *)t->tilt; a.vec_norm = (const float *)t->norm; a.vec_north = (const float *)t->north;
    a.mask = (const uint8_t *)t->mask;
    a.cells = nc; a.azim_num = t->azim_num;
    a.fill = t->fill;
    a.refrac_fac = t->refrac_fac;
    a.state = static_cast<double *>(state.p);
    a.state_n = state.p ? reinterpret_cast<int32_t *>(a.state + 5 * nc) : nullptr;
    a.sunrise = d_rise.dev; a.sunset = d_set.dev; a.duration = d_dur.dev; a.intervals = d_n.dev;
    float ms = 0.0f;
    {
        hipEvent_t e0, e1;
        HZ_HIP(hipEventCreate(&e0)); HZ_HIP(hipEventCreate(&e1));
        struct EvFree { hipEvent_t a, b; ~EvFree() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev_free{e0, e1};
        HZ_HIP(hipEventRecord(e0, st));
        for (int c = 0; c < plan.num_chunks; c++) {
            int s0 = 0, kc = 0;
            horisun_chunk(plan, num_sun, c, &s0, &kc);
            if (sun_on_dev) a.suns = sun_positions + 3 * (size_t)s0;
            else {
                HZ_HIP(hipMemcpyAsync(stage_sun, sun_positions + 3 * (size_t)s0, (size_t)kc * 3 * sizeof(float), hipMemcpyHostToDevice, st));
                a.suns = stage_sun;
            }
            if (times_on_dev) a.times = times + s0;
            else {
                HZ_HIP(hipMemcpyAsync(stage_times, times + s0, (size_t)kc * sizeof(double), hipMemcpyHostToDevice, st));
                a.times = stage_times;
            }
            a.t_before = s0 > 0 ? times_host[s0 - 1] : times_host[0];
            a.num_sun = kc;
            a.first = c == 0; a.last = c == plan.num_chunks - 1;
            if ((rc = suntimes_launch(a, t->planes, plan.blocks, st, t->q16))) return rc;
        }
        HZ_HIP(hipEventRecord(e1, st));
        HZ_HIP(hipEventSynchronize(e1));
        HZ_HIP(hipEventElapsedTime(&ms, e0, e1));
    }
    Timer t_d2h; t_d2h.start();
    if ((rc = d_rise.finish(st))) return rc;
    if ((rc = d_set.finish(st))) return rc;
    if ((rc = d_dur.finish(st))) return rc;
    if ((rc = d_n.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    if (stats) {
        stats->num_cells = nc;
        stats->t_kernel_s += (double)ms * 1e-3;
        stats->t_d2h_s += t_d2h.stop();
        stats->t_total_s += t_total.stop();
        stats->scratch_bytes = scratch;
    }
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

// ---------------------------------------------------------------------------------------
// ocean masking (hz_coast.hip): coastline_distance / coastline_buffer, ocean_masking.py:163-345
// ---------------------------------------------------------------------------------------
// The largest double T with sqrt_rn(T) <= thr, so that `sqrt(d2) > thr` is `d2 > T` (sqrt_rn is monotone): no square root per
// cell and the same decisions.  thr < 0: no d2 qualifies (-1); a NaN threshold compares false with everything (+inf: every
// vertex is "within" it, as `dist > NaN` is false for every cell).
static double coast_threshold_squared(double thr) {
    if (thr != thr) return std::numeric_limits<double>::infinity();
    if (thr < 0.0) return -1.0;
    if (thr == std::numeric_limits<double>::infinity()) return thr;
    double t = thr * thr;
    if (t == std::numeric_limits<double>::infinity()) t = std::numeric_limits<double>::max();
    for (int k = 0; k < 64 && std::sqrt(t) > thr; k++) t = std::nextafter(t, -1.0);
    for (int k = 0; k < 64; k++) {
        const double up = std::nextafter(t, std::numeric_limits<double>::infinity());
        if (up == std::numeric_limits<double>::infinity() || std::sqrt(up) > thr) break;
        t = up;
    }
    return t;
}

static int coast_api(int any_hit, const double *x_ecef, const double *y_ecef, const double *z_ecef, const uint8_t *mask_land,
                     int len_0, int len_1, const double *pts_ecef, size_t num_pts, double dist_thr, double *dist_chord,
                     uint8_t *mask_buffer, int device, hz_stats *stats) {
    if (!x_ecef || !y_ecef || !z_ecef || !mask_land || (any_hit ? !mask_buffer : !dist_chord) || (num_pts && !pts_ecef))
        return set_error(HZ_ERR_ARG, "NULL argument");
    if (len_0 <= 0 || len_1 <= 0) return set_error(HZ_ERR_ARG, "Input data has inconsistent dimension length(s)");
    if (num_pts > 0x7fffffffull) return set_error(HZ_ERR_ARG, "too many coastline vertices (%zu; at most 2^31 - 1)", num_pts);
    int rc = select_device(device);
    if (rc) return rc;
    Timer t_total, t;
    t_total.start();
    hipStream_t st = nullptr;
    const size_t n = (size_t)len_0 * len_1;
    DevIn<double> dx, dy, dz, dp;
    DevIn<uint8_t> dm;
    DevOut<double> od;
    DevOut<uint8_t> ob;
    t.start();
    if ((rc = dx.bind(x_ecef, n, st)) || (rc = dy.bind(y_ecef, n, st)) || (rc = dz.bind(z_ecef, n, st)) ||
        (rc = dm.bind(mask_land, n, st)) || (rc = dp.bind(pts_ecef, num_pts * 3, st)))
        return rc;
    if ((rc = any_hit ? ob.bind(mask_buffer, n) : od.bind(dist_chord, n))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    const double t_h2d = t.stop();

    CoastIndex ix;
    DevScratch scratch;
    const size_t scratch_bytes = coast_scratch_bytes(num_pts, &ix);
    HZ_HIP(hipMalloc(&scratch.p, scratch_bytes));
    t.start();
    if ((rc = coast_index_build(dp.dev, scratch.p, &ix, st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    const double t_build = t.stop();

    t.start();
    const double thr2 = any_hit ? coast_threshold_squared(dist_thr) : 0.0;
    if ((rc = coast_query_launch(ix, dx.dev, dy.dev, dz.dev, dm.dev, len_0, len_1, any_hit, dist_thr, thr2, od.dev, ob.dev, st)))
        return rc;
    unsigned long long cnt[HZ_COAST_CNT_N] = {0, 0};
    HZ_HIP(hipMemcpyAsync(cnt, ix.counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HZ_HIP(hipStreamSynchronize(st));
    const double t_query = t.stop();
    if (cnt[1])
        return set_error(HZ_ERR_BOUND, "%llu cells left the coastline tree's walk at its iteration bound (a defect of the index; "
                         "no result was written for them)", cnt[1]);

    t.start();
    if ((rc = any_hit ? ob.finish(st) : od.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    const double t_d2h = t.stop();
    if (stats) {
        *stats = hz_stats();
        stats->num_cells = cnt[0];
        stats->t_bvh_s = t_build; stats->t_kernel_s = t_query; stats->t_h2d_s = t_h2d; stats->t_d2h_s = t_d2h;
        stats->t_total_s = t_total.stop();
        stats->scratch_bytes = scratch_bytes;
    }
    return HZ_OK;
}

int hz_coastline_distance(const double *x_ecef, const double *y_ecef, const double *z_ecef, const uint8_t *mask_land,
                          int len_0, int len_1, const double *pts_ecef, size_t num_pts, double *dist_chord, int device,
                          hz_stats *stats) {
    return coast_api(0, x_ecef, y_ecef, z_ecef, mask_land, len_0, len_1, pts_ecef, num_pts, 0.0, dist_chord, nullptr, device,
                     stats);
}

int hz_coastline_buffer(const double *x_ecef, const double *y_ecef, const double *z_ecef, const uint8_t *mask_land,
                        int len_0, int len_1, const double *pts_ecef, size_t num_pts, double dist_thr, uint8_t *mask_buffer,
                        int device, hz_stats *stats) {
    return coast_api(1, x_ecef, y_ecef, z_ecef, mask_land, len_0, len_1, pts_ecef, num_pts, dist_thr, nullptr, mask_buffer,
                     device, stats);
}

}  // extern "C"
