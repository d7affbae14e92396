// hz_api.hip -- C-ABI entry points of libhorayzon_hip.so (see include/horayzon_hip.h).
//
// Scenes, the stream pool, the stand-alone reductions and conversions, input preparation, the debug knobs and ocean masking.
// The horizon drivers are in hz_api_horizon.hip, the Terrain / HorizonTerrain drivers in hz_api_sun.hip.
#include "hz_internal.h"
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


int select_device(int device) {
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

void scene_free(Scene *sc) {
    if (!sc) return;
    (void)hipSetDevice(sc->device);
    stream_release(sc->device, sc->stream);
    if (sc->near_buf) (void)hipFree(sc->near_buf);
    if (sc->left_buf) (void)hipFree(sc->left_buf);
    if (sc->owns_blob && sc->blob) (void)hipFree(sc->blob);
    delete sc;
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
    DevBuf d_h, d_p;
    if (!hori_dev) HZ_HIP(d_h.alloc(chunk * A * sizeof(float)));
    if (!planes_dev) HZ_HIP(d_p.alloc(chunk * A * sizeof(float)));
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
    DevBuf d_src, d_dst;
    if (!src_dev) HZ_HIP(d_src.alloc(chunk * src_size));
    if (!dst_dev) HZ_HIP(d_dst.alloc(chunk * dst_size));
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

// ---------------------------------------------------------------------------------------
// the reductions over the azimuth axis (hz_topo.hip): three single-output entry points, hz_topo_params, hz_topo_params_planes,
// hz_topo_params_q16
// ---------------------------------------------------------------------------------------
// The planes form: rows [rb, re) of every plane back into a bounded cell-major buffer (k_planes_to_hori), then the
// reduction launch the cell-major form makes on it -- no numerics are written again, so every map is the same words.
// azim, tilt and the outputs are device memory (tilt and the outputs may be null).
static int topo_launch_planes(const float *azim, const float *planes, const float *tilt, int len_0, int len_1, int len_2,
                              float *svf, float *vsf, float *openness, hipStream_t st) {
    const size_t ncell = (size_t)len_0 * len_1, A = (size_t)len_2;
    const bool planes_dev = is_device_ptr(planes);
    const int rows = (int)std::max<size_t>(1, planes_chunk_cells(ncell, len_2) / (size_t)len_1);
    const size_t chunk = (size_t)rows * len_1;
    DevBuf d_h, d_p;
    HZ_HIP(d_h.alloc(chunk * A * sizeof(float)));
    if (!planes_dev) HZ_HIP(d_p.alloc(chunk * A * sizeof(float)));
    for (int rb = 0; rb < len_0; rb += rows) {
        const int re = std::min(rb + rows, len_0);
        const size_t c0 = (size_t)rb * len_1, n = (size_t)(re - rb) * len_1;
        int rc;
        if (planes_dev) rc = planes_to_hori_launch(planes, ncell, c0, n, len_2, (float *)d_h.p, st);
        else {
            HZ_HIP(hipMemcpy2DAsync(d_p.p, n * sizeof(float), planes + c0, ncell * sizeof(float), n * sizeof(float), A,
                                    hipMemcpyHostToDevice, st));
            rc = planes_to_hori_launch((const float *)d_p.p, n, 0, n, len_2, (float *)d_h.p, st);
        }
        if (!rc) rc = topo_launch(azim, (const float *)d_h.p, tilt ? tilt + 3 * c0 : nullptr, re - rb, len_1, len_2,
                                  svf ? svf + c0 : nullptr, vsf ? vsf + c0 : nullptr, openness ? openness + c0 : nullptr, st);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        HZ_HIP(hipStreamSynchronize(st));           // the chunk buffers are used again
    }
    return HZ_OK;
}

// The direct planes form (codes always; float planes under hz_debug_set("topo_planes_direct", 1)): k_topo_planes reads the
// planes as they lie, one lane per cell -- no cell-major buffer and no second pass.  Device planes are one launch; host
// planes go through the row-slab staging above at the element's size.
static std::atomic<int> g_topo_planes_direct{0};
static int topo_launch_planes_direct_staged(const float *azim, const void *planes, bool q16, const float *tilt, int len_0, int len_1,
                                            int len_2, float *svf, float *vsf, float *openness, hipStream_t st) {
    const size_t ncell = (size_t)len_0 * len_1, A = (size_t)len_2, elem = q16 ? sizeof(uint16_t) : sizeof(float);
    if (is_device_ptr(planes)) return topo_launch_planes_direct(azim, planes, q16, ncell, tilt, ncell, len_2, svf, vsf, openness, st);
    const int rows = (int)std::max<size_t>(1, planes_chunk_cells(ncell, len_2) / (size_t)len_1);
    const size_t chunk = (size_t)rows * len_1;
    DevBuf d_p;
    HZ_HIP(d_p.alloc(chunk * A * elem));
    for (int rb = 0; rb < len_0; rb += rows) {
        const int re = std::min(rb + rows, len_0);
        const size_t c0 = (size_t)rb * len_1, n = (size_t)(re - rb) * len_1;
        HZ_HIP(hipMemcpy2DAsync(d_p.p, n * elem, static_cast<const char *>(planes) + c0 * elem, ncell * elem, n * elem, A,
                                hipMemcpyHostToDevice, st));
        const int rc = topo_launch_planes_direct(azim, d_p.p, q16, n, tilt ? tilt + 3 * c0 : nullptr, n, len_2, svf ? svf + c0 : nullptr,
                                                 vsf ? vsf + c0 : nullptr, openness ? openness + c0 : nullptr, st);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        HZ_HIP(hipStreamSynchronize(st));           // the chunk buffer is used again
    }
    return HZ_OK;
}

// The one driver of the six entry points.  `planes`: hori is planes[azim][y][x] (host or device), else cell-major; `q16`: its
// elements are 16-bit codes, else float32.  `no_output`: the message when no output is asked for (a single-output entry
// point hands its one output in its slot).
static int topo_api(bool planes, bool q16, const char *no_output, const float *azim, const void *hori, const float *vec_tilt,
                    int len_0, int len_1, int len_2, float *svf, float *vsf, float *openness, int device) {
    const bool tilt = svf || vsf;
    if (!svf && !vsf && !openness) return set_error(HZ_ERR_ARG, "%s", no_output);
    if (!azim || !hori || (tilt && !vec_tilt)) return set_error(HZ_ERR_ARG, "NULL argument");
    if (q16 && (reinterpret_cast<uintptr_t>(hori) & (sizeof(uint16_t) - 1)))
        return set_error(HZ_ERR_ARG, "an array is not aligned to its element type");
    // (the openness reads no azim[1] - azim[0]: one azimuth is enough, as in the reference)
    if (len_0 <= 0 || len_1 <= 0 || len_2 < (tilt ? 2 : 1)) return set_error(HZ_ERR_ARG, "Inconsistent/incorrect shapes of input arrays");
    int rc;
    if ((planes || q16) && (rc = planes_check_shape(azim, hori, len_0, len_1, len_2))) return rc;
    if ((rc = select_device(device))) return rc;
    hipStream_t st = nullptr;
    const size_t ncell = (size_t)len_0 * len_1;
    DevIn<float> d_azim, d_tilt;
    DevIn<unsigned char> d_hori;                     // cell-major only: planes are staged by their route
    DevOut<float> d_svf, d_vsf, d_open;
    if ((rc = d_azim.bind(azim, (size_t)len_2, st))) return rc;
    if (!planes) if ((rc = d_hori.bind(static_cast<const unsigned char *>(hori), ncell * (size_t)len_2 * (q16 ? sizeof(uint16_t) : sizeof(float)), st))) return rc;
    if (tilt) if ((rc = d_tilt.bind(vec_tilt, ncell * 3, st))) return rc;
    if ((rc = d_svf.bind(svf, svf ? ncell : 0))) return rc;
    if ((rc = d_vsf.bind(vsf, vsf ? ncell : 0))) return rc;
    if ((rc = d_open.bind(openness, openness ? ncell : 0))) return rc;
    if (planes && (q16 || g_topo_planes_direct.load(std::memory_order_relaxed)))
        rc = topo_launch_planes_direct_staged(d_azim.dev, hori, q16, d_tilt.dev, len_0, len_1, len_2, d_svf.dev, d_vsf.dev, d_open.dev, st);
    else if (planes)
        rc = topo_launch_planes(d_azim.dev, static_cast<const float *>(hori), d_tilt.dev, len_0, len_1, len_2, d_svf.dev, d_vsf.dev, d_open.dev, st);
    else if (q16)
        rc = topo_launch_q16(d_azim.dev, reinterpret_cast<const uint16_t *>(d_hori.dev), d_tilt.dev, len_0, len_1, len_2, d_svf.dev, d_vsf.dev, d_open.dev, st);
    else
        rc = topo_launch(d_azim.dev, reinterpret_cast<const float *>(d_hori.dev), d_tilt.dev, len_0, len_1, len_2, d_svf.dev, d_vsf.dev, d_open.dev, st);
    if (rc) return rc;
    if ((rc = d_svf.finish(st)) || (rc = d_vsf.finish(st)) || (rc = d_open.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    return HZ_OK;
}

static const char *const TOPO_NO_OUTPUT = "no output requested (svf, vsf and openness are NULL)";

int hz_sky_view_factor(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1,
                       int len_2, float *svf, int device) {
    return topo_api(false, false, "NULL argument", azim, hori, vec_tilt, len_0, len_1, len_2, svf, nullptr, nullptr, device);
}
int hz_visible_sky_fraction(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1,
                            int len_2, float *vsf, int device) {
    return topo_api(false, false, "NULL argument", azim, hori, vec_tilt, len_0, len_1, len_2, nullptr, vsf, nullptr, device);
}
int hz_topographic_openness(const float *azim, const float *hori, int len_0, int len_1, int len_2, float *top,
                            int device) {
    return topo_api(false, false, "NULL argument", azim, hori, nullptr, len_0, len_1, len_2, nullptr, nullptr, top, device);
}
int hz_topo_params(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1, int len_2,
                   float *svf, float *vsf, float *openness, int device) {
    return topo_api(false, false, TOPO_NO_OUTPUT, azim, hori, vec_tilt, len_0, len_1, len_2, svf, vsf, openness, device);
}
int hz_topo_params_planes(const float *azim, const float *planes, const float *vec_tilt, int len_0, int len_1, int len_2,
                          float *svf, float *vsf, float *openness, int device) {
    return topo_api(true, false, TOPO_NO_OUTPUT, azim, planes, vec_tilt, len_0, len_1, len_2, svf, vsf, openness, device);
}
int hz_topo_params_q16(const float *azim, const uint16_t *hori_q, int planes, const float *vec_tilt, int len_0, int len_1, int len_2,
                       float *svf, float *vsf, float *openness, int device) {
    if (planes != 0 && planes != 1) return set_error(HZ_ERR_ARG, "planes must be 0 or 1");
    return topo_api(planes != 0, true, TOPO_NO_OUTPUT, azim, hori_q, vec_tilt, len_0, len_1, len_2, svf, vsf, openness, device);
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
    else if (!strcmp(key, "topo_planes_direct")) g_topo_planes_direct.store(value > 0, std::memory_order_relaxed);
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
    else if (!strcmp(key, "panorama_traversal")) {    // (< 0: the default; results never depend on it)
        if (value > 1) return hz::set_error(HZ_ERR_ARG, "hz_debug_set: panorama_traversal is 0 or 1");
        hz::g_panorama_traversal.store(value, std::memory_order_relaxed);
    }
    else if (!strcmp(key, "panorama_budget")) hz::g_panorama_budget.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    else if (!strcmp(key, "cast_budget")) hz::g_cast_budget.store(value < 0 ? 0 : value, std::memory_order_relaxed);
    else if (!strcmp(key, "cast_sort_only")) hz::g_cast_sort_only.store(value > 0 ? 1 : 0, std::memory_order_relaxed);
    else if (!strcmp(key, "cast_fast_cap")) hz::g_cast_fast_cap.store(value < 0 ? HZ_CAST_FAST_CAP_DEFAULT : value, std::memory_order_relaxed);
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
    DevBuf scratch;
    const size_t scratch_bytes = coast_scratch_bytes(num_pts, &ix);
    HZ_HIP(scratch.alloc(scratch_bytes));
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
