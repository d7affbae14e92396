/*
 * standin.cpp -- the sixteen Embree entry points of oracle/ref/embree4/rtcore.h, answered by the oracle.
 *
 * TEST INFRASTRUCTURE ONLY.  Linked with the reference's own horizon_comp.cpp / shadow_comp.cpp (compiled
 * unmodified, oracle/Makefile) into oracle/_ref/libhz_ref.so.  The reference's statements then run as written --
 * its searches, index arithmetic, trig tables, ray origins, rotation, refraction and shadow codes -- while every
 * hit / no-hit decision is the oracle's (orc_occluded1 / orc_closest1 of hz_oracle.c).  "Reference driver +
 * oracle intersector" must therefore equal "oracle driver + oracle intersector" word for word
 * (tests/test_ref_driver.py).  What Embree itself would decide is not modelled here.
 *
 * The scene is assembled at rtcCommitScene from what the reference handed over:
 *   - the shared vertex buffer of the DEM grid;
 *   - the index buffer the reference FILLED after rtcSetNewGeometryBuffer.  It is checked entry by entry against
 *     the topology the oracle assumes (two triangles per grid quad, (a, b, c) and (b, d, c) with a = (i, j),
 *     b = (i, j + 1), c = (i + 1, j), d = (i + 1, j + 1); for "quad" the quad (a, b, d, c); for "grid" one RTCGrid
 *     over all vertices).  A mismatch is an error, not a warning: the topology is one of the pinned facts;
 *   - the optional outer TIN (a second triangle geometry whose two buffers are shared).
 * "quad" and "grid" are accepted only while the oracle models their second triangle the way Embree's quad
 * intersector orders it (orc_set_quad_order(1)), "triangle" only while it does not, and rtcIntersect1 only for
 * "triangle" (the oracle's closest-hit query has no quad-order form).
 *
 * Ray budget: the reference's ray_guess_const / ray_discrete_sampling loops do not end when a ray is still
 * blocked at the top table index or still free at index 0.  hzref_set_ray_budget(n) makes the (n + 1)-th ray
 * throw hzref::budget_exceeded, which oracle/ref/entry.cpp turns into an error code.
 */
#include <embree4/rtcore.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "standin.h"

extern "C" {
/* oracle/hz_oracle.c */
struct orc_scene;
orc_scene *orc_scene_create(const float *vert_grid, int d0, int d1, const float *vert_simp, int nvs,
                            const int32_t *tri_simp, int nts);
void orc_scene_destroy(orc_scene *s);
int orc_occluded1(const orc_scene *s, const float *org, const float *dir, float tfar, int mode);
int orc_closest1(const orc_scene *s, const float *org, const float *dir, float tfar, int mode, float *dist);
int orc_get_quad_order(void);
}

struct HzRefDevice {
    int refs;
};

struct HzRefGeometry {
    int refs;
    RTCGeometryType type;
    const float *vert;
    size_t num_vert;
    const void *index;              /* shared index buffer, or owned.data() */
    bool index_shared;
    RTCBufferType index_type;
    RTCFormat index_format;
    size_t index_stride, num_index;
    std::vector<unsigned char> owned;
    bool committed;
};

struct HzRefScene {
    int refs;
    std::vector<HzRefGeometry *> geoms;
    orc_scene *orc;
    bool tri_topology;              /* rtcIntersect1 allowed */
};

namespace {

int64_t g_budget = -1, g_rays = 0;
int g_mode = 0;                     /* oracle query mode: 0 tree, 1 brute force */
float *g_rec = nullptr;             /* recorded rays: org[3], dir[3], tfar, kind (0 occluded, 1 intersect) */
int64_t g_rec_cap = 0, g_rec_n = 0;
std::vector<HzRefScene *> g_live_scenes;
std::vector<HzRefDevice *> g_live_devices;
std::vector<HzRefGeometry *> g_live_geoms;

[[noreturn]] void fail(const std::string &what) { throw hzref::standin_error("Embree stand-in: " + what); }

template <typename T>
void forget(std::vector<T *> &v, T *p) {
    for (size_t i = 0; i < v.size(); i++)
        if (v[i] == p) { v.erase(v.begin() + (long)i); return; }
}

void geometry_release(HzRefGeometry *g) {
    if (--g->refs == 0) { forget(g_live_geoms, g); delete g; }
}

void scene_free(HzRefScene *s) {
    for (HzRefGeometry *g : s->geoms) geometry_release(g);
    if (s->orc) orc_scene_destroy(s->orc);
    delete s;
}

void count_ray(const float *o, const float *d, float tfar, int kind) {
    if (g_budget >= 0 && g_rays >= g_budget) throw hzref::budget_exceeded();
    if (g_rec && g_rec_n < g_rec_cap) {
        float *r = g_rec + 8 * g_rec_n++;
        r[0] = o[0]; r[1] = o[1]; r[2] = o[2]; r[3] = d[0]; r[4] = d[1]; r[5] = d[2]; r[6] = tfar; r[7] = (float)kind;
    }
    g_rays++;
}

/* the DEM geometry: dimensions from the buffers, and the index buffer against the assumed topology */
void check_grid_geometry(const HzRefGeometry *g, int *d0_out, int *d1_out) {
    if (!g->vert || g->num_vert < 4) fail("DEM geometry without a vertex buffer of at least 2 x 2 vertices");
    if (!g->index || g->index_shared) fail("the DEM geometry's index buffer must be the one the caller filled");
    const int64_t nv = (int64_t)g->num_vert;
    int64_t d0 = 0, d1 = 0;
    if (g->type == RTC_GEOMETRY_TYPE_GRID) {
        if (g->index_type != RTC_BUFFER_TYPE_GRID || g->index_format != RTC_FORMAT_GRID || g->num_index != 1 ||
            g->index_stride != sizeof(RTCGrid))
            fail("grid geometry: expected one RTCGrid");
        const RTCGrid *q = (const RTCGrid *)g->index;
        d0 = q->height; d1 = q->width;
        if (q->startVertexID != 0 || q->stride != q->width || d0 < 2 || d1 < 2 || d0 * d1 != nv)
            fail("grid geometry: the RTCGrid does not span the vertex buffer row by row");
    } else {
        const bool tri = (g->type == RTC_GEOMETRY_TYPE_TRIANGLE);
        const int per = tri ? 3 : 4;
        if (g->index_type != RTC_BUFFER_TYPE_INDEX || g->index_format != (tri ? RTC_FORMAT_UINT3 : RTC_FORMAT_UINT4) ||
            g->index_stride != (size_t)per * 4 || g->num_index < 1)
            fail("DEM geometry: unexpected index buffer format");
        const uint32_t *ix = (const uint32_t *)g->index;
        /* row length: the third corner of the first triangle / fourth of the first quad is vertex (1, 0) */
        d1 = ix[per - 1];
        if (d1 < 2 || nv % d1 != 0) fail("DEM geometry: first primitive does not name vertex (1, 0)");
        d0 = nv / d1;
        const int64_t nq = (d0 - 1) * (d1 - 1);
        if (d0 < 2 || (int64_t)g->num_index != (tri ? 2 * nq : nq)) fail("DEM geometry: primitive count does not match the grid");
        int64_t n = 0;
        for (int64_t i = 0; i < d0 - 1; i++)
            for (int64_t j = 0; j < d1 - 1; j++) {
                const uint32_t a = (uint32_t)(i * d1 + j), b = a + 1, c = (uint32_t)((i + 1) * d1 + j), d = c + 1;
                bool ok;
                if (tri) {
                    const uint32_t *t0 = ix + 3 * n, *t1 = t0 + 3;
                    ok = t0[0] == a && t0[1] == b && t0[2] == c && t1[0] == b && t1[1] == d && t1[2] == c;
                    n += 2;
                } else {
                    const uint32_t *q = ix + 4 * n;
                    ok = q[0] == a && q[1] == b && q[2] == d && q[3] == c;
                    n += 1;
                }
                if (!ok) {
                    char msg[160];
                    snprintf(msg, sizeof msg, "index buffer differs from the oracle's topology at grid quad (%lld, %lld)",
                             (long long)i, (long long)j);
                    fail(msg);
                }
            }
    }
    if (d0 > std::numeric_limits<int>::max() || d1 > std::numeric_limits<int>::max()) fail("grid too large");
    *d0_out = (int)d0; *d1_out = (int)d1;
}

}  // namespace

/* ----------------------------------------------------------------------------------------------------------- */
/* control surface (oracle/ref.py)                                                                               */
/* ----------------------------------------------------------------------------------------------------------- */

extern "C" {

void hzref_set_ray_budget(int64_t max_rays) { g_budget = max_rays; g_rays = 0; }
int64_t hzref_rays_cast(void) { return g_rays; }
void hzref_set_mode(int mode) { g_mode = mode; }
void hzref_record(float *buf, int64_t cap_rays) { g_rec = buf; g_rec_cap = buf ? cap_rays : 0; g_rec_n = 0; }
int64_t hzref_recorded(void) { return g_rec_n; }

}

namespace hzref {

/* after an exception left the reference's function early: free what it did not release */
void release_leftovers() {
    for (HzRefScene *s : std::vector<HzRefScene *>(g_live_scenes)) scene_free(s);
    g_live_scenes.clear();
    for (HzRefGeometry *g : g_live_geoms) delete g;
    g_live_geoms.clear();
    for (HzRefDevice *d : g_live_devices) delete d;
    g_live_devices.clear();
}

/* the same for one Terrain object, whose scene and device outlive the call */
void forget_scene(RTCScene s) { forget(g_live_scenes, s); }
void forget_device(RTCDevice d) { forget(g_live_devices, d); }

}  // namespace hzref

/* ----------------------------------------------------------------------------------------------------------- */
/* the Embree entry points                                                                                       */
/* ----------------------------------------------------------------------------------------------------------- */

extern "C" {

RTCDevice rtcNewDevice(const char *) {
    HzRefDevice *d = new HzRefDevice{1};
    g_live_devices.push_back(d);
    return d;
}

void rtcReleaseDevice(RTCDevice d) {
    if (d && --d->refs == 0) { forget(g_live_devices, d); delete d; }
}

enum RTCError rtcGetDeviceError(RTCDevice) { return RTC_ERROR_NONE; }

void rtcSetDeviceErrorFunction(RTCDevice, RTCErrorFunction, void *) {}

RTCScene rtcNewScene(RTCDevice) {
    HzRefScene *s = new HzRefScene{1, {}, nullptr, false};
    g_live_scenes.push_back(s);
    return s;
}

void rtcSetSceneFlags(RTCScene, enum RTCSceneFlags flags) {
    if (flags != RTC_SCENE_FLAG_ROBUST) fail("the oracle's triangle test restates the ROBUST mode only");
}

RTCGeometry rtcNewGeometry(RTCDevice, enum RTCGeometryType type) {
    if (type != RTC_GEOMETRY_TYPE_TRIANGLE && type != RTC_GEOMETRY_TYPE_QUAD && type != RTC_GEOMETRY_TYPE_GRID)
        fail("unknown geometry type");
    HzRefGeometry *g = new HzRefGeometry();
    g->refs = 1; g->type = type; g->vert = nullptr; g->num_vert = 0; g->index = nullptr; g->index_shared = false;
    g->index_type = RTC_BUFFER_TYPE_INDEX; g->index_format = RTC_FORMAT_UNDEFINED; g->index_stride = 0; g->num_index = 0;
    g->committed = false;
    g_live_geoms.push_back(g);
    return g;
}

void rtcSetSharedGeometryBuffer(RTCGeometry g, enum RTCBufferType type, unsigned int slot, enum RTCFormat format,
                                const void *ptr, size_t byteOffset, size_t byteStride, size_t itemCount) {
    if (slot != 0 || byteOffset != 0 || !ptr) fail("shared buffer: slot 0, offset 0 and a pointer expected");
    if (type == RTC_BUFFER_TYPE_VERTEX) {
        if (format != RTC_FORMAT_FLOAT3 || byteStride != 3 * sizeof(float)) fail("vertex buffer: packed FLOAT3 expected");
        g->vert = (const float *)ptr; g->num_vert = itemCount;
    } else if (type == RTC_BUFFER_TYPE_INDEX) {
        if (g->type != RTC_GEOMETRY_TYPE_TRIANGLE || format != RTC_FORMAT_UINT3 || byteStride != 3 * sizeof(int))
            fail("shared index buffer: packed UINT3 of a triangle geometry expected");
        g->index = ptr; g->index_shared = true; g->index_type = type; g->index_format = format;
        g->index_stride = byteStride; g->num_index = itemCount;
    } else fail("shared buffer of an unexpected type");
}

void *rtcSetNewGeometryBuffer(RTCGeometry g, enum RTCBufferType type, unsigned int slot, enum RTCFormat format,
                              size_t byteStride, size_t itemCount) {
    if (slot != 0) fail("new buffer: slot 0 expected");
    if (type != RTC_BUFFER_TYPE_INDEX && type != RTC_BUFFER_TYPE_GRID) fail("new buffer of an unexpected type");
    /* poisoned, so that an entry the caller leaves unwritten cannot pass the topology check */
    g->owned.assign(byteStride * itemCount + 16, 0xff);
    g->index = g->owned.data(); g->index_shared = false; g->index_type = type; g->index_format = format;
    g->index_stride = byteStride; g->num_index = itemCount;
    return g->owned.data();
}

void rtcCommitGeometry(RTCGeometry g) { g->committed = true; }

unsigned int rtcAttachGeometry(RTCScene s, RTCGeometry g) {
    if (!g->committed) fail("geometry attached before it was committed");
    g->refs++;
    s->geoms.push_back(g);
    return (unsigned int)(s->geoms.size() - 1);
}

void rtcReleaseGeometry(RTCGeometry g) { geometry_release(g); }

void rtcCommitScene(RTCScene s) {
    if (s->orc) fail("scene committed twice");
    if (s->geoms.empty() || s->geoms.size() > 2) fail("one DEM geometry and at most one outer TIN expected");
    const HzRefGeometry *g = s->geoms[0];
    int d0 = 0, d1 = 0;
    check_grid_geometry(g, &d0, &d1);
    s->tri_topology = (g->type == RTC_GEOMETRY_TYPE_TRIANGLE);
    if (s->tri_topology && orc_get_quad_order() != 0)
        fail("geometry type 'triangle' while the oracle models Embree's quad order (orc_set_quad_order(1))");
    if (!s->tri_topology && orc_get_quad_order() != 1)
        fail("geometry types 'quad' / 'grid' are modelled only under orc_set_quad_order(1)");
    const float *vs = nullptr; const int32_t *ts = nullptr; int nvs = 0, nts = 0;
    if (s->geoms.size() == 2) {
        const HzRefGeometry *t = s->geoms[1];
        if (t->type != RTC_GEOMETRY_TYPE_TRIANGLE || !t->index_shared || !t->vert || t->num_vert < 3 || t->num_index < 1)
            fail("outer TIN: a triangle geometry with shared vertex and index buffers expected");
        const uint32_t *ix = (const uint32_t *)t->index;
        for (size_t k = 0; k < 3 * t->num_index; k++)
            if (ix[k] >= t->num_vert) fail("outer TIN: vertex index out of range");
        vs = t->vert; nvs = (int)t->num_vert; ts = (const int32_t *)t->index; nts = (int)t->num_index;
    }
    s->orc = orc_scene_create(g->vert, d0, d1, vs, nvs, ts, nts);
    if (!s->orc) fail("orc_scene_create failed");
}

void rtcReleaseScene(RTCScene s) {
    if (s && --s->refs == 0) { forget(g_live_scenes, s); scene_free(s); }
}

void rtcOccluded1(RTCScene s, struct RTCRay *ray, struct RTCOccludedArguments *) {
    if (!s->orc) fail("rtcOccluded1 on a scene that was not committed");
    if (ray->tnear != 0.0f) fail("the oracle's queries start at tnear = 0");
    const float o[3] = {ray->org_x, ray->org_y, ray->org_z}, d[3] = {ray->dir_x, ray->dir_y, ray->dir_z};
    count_ray(o, d, ray->tfar, 0);
    if (orc_occluded1(s->orc, o, d, ray->tfar, g_mode))
        ray->tfar = -std::numeric_limits<float>::infinity();
}

void rtcIntersect1(RTCScene s, struct RTCRayHit *rh, struct RTCIntersectArguments *) {
    if (!s->orc) fail("rtcIntersect1 on a scene that was not committed");
    if (!s->tri_topology) fail("rtcIntersect1 is modelled for geometry type 'triangle' only");
    if (rh->ray.tnear != 0.0f) fail("the oracle's queries start at tnear = 0");
    const float o[3] = {rh->ray.org_x, rh->ray.org_y, rh->ray.org_z};
    const float d[3] = {rh->ray.dir_x, rh->ray.dir_y, rh->ray.dir_z};
    count_ray(o, d, rh->ray.tfar, 1);
    float t = rh->ray.tfar;
    if (orc_closest1(s->orc, o, d, rh->ray.tfar, g_mode, &t)) {
        rh->ray.tfar = t;
        rh->hit.geomID = 0;
        rh->hit.primID = 0;
    }
}

}
