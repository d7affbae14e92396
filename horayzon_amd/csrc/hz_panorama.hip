// hz_panorama.hip -- Terrain.panorama (hz_terrain_panorama): depth images of the scene from observer points (gfx950;
// DESIGN.md section 4, clause 20).
//
// Per observer an image of elev_num x azim_num pixels; pixel (e, a) is one closest-hit ray from the observer in the direction
// the four trig tables and the observer's frame (east = north x norm) give, of length max_dist: the distance to the closest
// accepted triangle (hz_closest's minimum: oracle.Scene.closest), the hit point obs + dir * t, and per observer the number of
// pixels with a hit.  NaN where nothing is hit.  The kernel does no trigonometry.
//
// Organisation (k_horidist's): one wave = one workgroup owns a tile of 8 azimuths x 8 elevations of ONE observer, lane =
// 8 * (e mod 8) + (a mod 8).  Its 64 rays share the origin and leave it in neighbouring directions: they open the same nodes
// at the start and drift apart with the distance.  Observer, frame and tfar are the same for the whole wave and live in
// scalar registers.  The traversal is the front-to-back closest hit of hz_closest_order.h (stack of individual child links,
// up to 3 per tree level, in LDS: 3 x height x 64 x 4 B, no barrier); hz_closest itself stays selectable
// (hz_debug_set("panorama_traversal", 0)) for same-call comparisons.  (observer of the launch, tile) is blockIdx.x.
//
// Memory: `dist` rows of 8 consecutive azimuths are 32-byte runs, eight per wave; `point` is stored per component.  A lane
// whose pixel lies beyond azim_num or elev_num traces nothing and stores nothing.  hits: one ballot + popcount per wave, one
// 64-bit atomicAdd from lane 0 (the caller zeroes the counts).
#include "hz_internal.h"
#include "hz_closest_order.h"

namespace hz {

#define HZ_PN_TPB 64

#define HZ_PN_TRAVERSAL_DEFAULT 1
// hz_debug_set("panorama_traversal", 0 | 1): 0 = hz_closest as it is, 1 = the children of a node front to back (same-call A/Bs)
std::atomic<int> g_panorama_traversal{HZ_PN_TRAVERSAL_DEFAULT};
std::atomic<int> g_panorama_budget{0};       // hz_debug_set("panorama_budget", bytes): the staging budget of a chunk (hz_api_sun.hip)

struct PanoramaParams {
    SceneView sv;
    const float *obs;                    // f32[observers of the launch][3]
    const float *north, *norm;           // f32[observers of the launch][3], or both null: north = (0, 1, 0), norm = (0, 0, 1)
    const float *azim_sin, *azim_cos, *elev_sin, *elev_cos;
    int azim_num, elev_num;
    int tiles_a;                         // tiles of an image along the azimuth axis
    unsigned tiles;                      // tiles of an image
    float tfar;
    float *dist;                         // f32[observers][elev_num][azim_num] at the launch's first observer, or null
    float *point;                        // f32[observers][elev_num][azim_num][3] at the launch's first observer (WANT_POINT)
    unsigned long long *hits;            // u64[observers] at the launch's first observer, or null
};

// a value every lane of the wave holds alike, moved to a scalar register
__device__ __forceinline__ float pn_uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

template <bool WANT_POINT, int MODE>
__global__ __launch_bounds__(HZ_PN_TPB) void k_panorama(PanoramaParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *stack = reinterpret_cast<int *>(smem);
    const int lane = threadIdx.x;
    const unsigned s = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;        // observer of the launch, tile of its image
    const int te = (int)(tile / (unsigned)p.tiles_a), ta = (int)(tile % (unsigned)p.tiles_a);
    const int e = te * 8 + (lane >> 3), a = ta * 8 + (lane & 7);
    const bool live = e < p.elev_num && a < p.azim_num;
    // the origin and the frame, once per wave: k_horidist's rotation (east = north x norm)
    const float ox = pn_uniform(p.obs[3 * (size_t)s]), oy = pn_uniform(p.obs[3 * (size_t)s + 1]), oz = pn_uniform(p.obs[3 * (size_t)s + 2]);
    float north_x = 0.0f, north_y = 1.0f, north_z = 0.0f, norm_x = 0.0f, norm_y = 0.0f, norm_z = 1.0f;
    if (p.north) {
        north_x = pn_uniform(p.north[3 * (size_t)s]); north_y = pn_uniform(p.north[3 * (size_t)s + 1]); north_z = pn_uniform(p.north[3 * (size_t)s + 2]);
        norm_x = pn_uniform(p.norm[3 * (size_t)s]); norm_y = pn_uniform(p.norm[3 * (size_t)s + 1]); norm_z = pn_uniform(p.norm[3 * (size_t)s + 2]);
    }
    const float east_x = north_y * norm_z - north_z * norm_y;
    const float east_y = north_z * norm_x - north_x * norm_z;
    const float east_z = north_x * norm_y - north_y * norm_x;
    const float ocx = ox - p.sv.cx, ocy = oy - p.sv.cy, ocz = oz - p.sv.cz;
    const float tau = p.sv.tau;
    const float nan = __builtin_nanf("");
    float d = nan, hx = nan, hy = nan, hz_ = nan;
    bool hit = false;
    if (live) {
        const float ec = p.elev_cos[e], es = p.elev_sin[e];
        const float rx = ec * p.azim_sin[a], ry = ec * p.azim_cos[a], rz = es;
        const float dx = (east_x * rx + north_x * ry) + norm_x * rz;
        const float dy = (east_y * rx + north_y * ry) + norm_y * rz;
        const float dz = (east_z * rx + north_z * ry) + norm_z * rz;
        const RayBox rb = hz_raybox(ocx - tau * dx, ocy - tau * dy, ocz - tau * dz, dx, dy, dz);
        float t = 0.0f;
        hit = MODE != 0
            ? hd_closest_near_first<HZ_PN_TPB>(p.sv.nodes, p.sv.prims, stack, lane, ox, oy, oz, dx, dy, dz, p.tfar, tau, rb, &t)
            : hz_closest<HZ_PN_TPB>(p.sv.nodes, p.sv.prims, stack, lane, ox, oy, oz, dx, dy, dz, p.tfar, tau, rb, &t);
        if (hit) {
            // An origin on the surface is accepted by the triangles around it with T = +0 and T = -0: which zero a minimum
            // keeps depends on the order they are met in (v_min_f32 prefers -0, a compare keeps the first).  The clause
            // writes a zero distance as +0.0, so the words do not depend on the order.
            d = t == 0.0f ? 0.0f : t;
            if (WANT_POINT) {
                const float px = dx * d, py = dy * d, pz = dz * d;
                hx = ox + px; hy = oy + py; hz_ = oz + pz;
            }
        }
        const size_t pix = ((size_t)s * (size_t)p.elev_num + (size_t)e) * (size_t)p.azim_num + (size_t)a;
        if (p.dist) p.dist[pix] = d;
        if (WANT_POINT) {
            float *q = p.point + 3 * pix;
            q[0] = hx; q[1] = hy; q[2] = hz_;
        }
    }
    // the wave's tally, where all its lanes are here again
    const unsigned long long hit_mask = __ballot(hit);
    if (p.hits && lane == 0 && hit_mask != 0ull) atomicAdd(&p.hits[s], (unsigned long long)__popcll(hit_mask));
}

template <bool WANT_POINT, int MODE>
static int pn_launch2(const PanoramaParams &p, unsigned grid, size_t lds, hipStream_t st) {
    HZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_panorama<WANT_POINT, MODE>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_panorama<WANT_POINT, MODE>), dim3(grid), dim3(HZ_PN_TPB), lds, st, p);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

int panorama_launch(const Scene *sc, const PanoramaArgs &a, hipStream_t st) {
    if (a.num_obs <= 0 || a.azim_num <= 0 || a.elev_num <= 0) return HZ_OK;
    if (!a.dist && !a.point && !a.hits) return HZ_OK;
    if ((a.vec_north == nullptr) != (a.vec_norm == nullptr)) return set_error(HZ_ERR_ARG, "panorama: one of the two frame arrays is missing");
    PanoramaParams p;
    p.sv = scene_view(sc);
    p.obs = a.observers; p.north = a.vec_north; p.norm = a.vec_norm;
    p.azim_sin = a.azim_sin; p.azim_cos = a.azim_cos; p.elev_sin = a.elev_sin; p.elev_cos = a.elev_cos;
    p.azim_num = a.azim_num; p.elev_num = a.elev_num;
    p.tiles_a = (a.azim_num + 7) / 8;
    const size_t tiles = (size_t)p.tiles_a * (size_t)((a.elev_num + 7) / 8);
    const size_t blocks = tiles * (size_t)a.num_obs;
    if (blocks > 0x7fffffffu) return set_error(HZ_ERR_ARG, "panorama: %zu tiles in one launch", blocks);
    p.tiles = (unsigned)tiles;
    p.tfar = a.max_dist;
    p.dist = a.dist; p.point = a.point;
    p.hits = reinterpret_cast<unsigned long long *>(a.hits);
    // hz_closest keeps individual child links: up to 3 per tree level
    const size_t lds = (size_t)(3 * std::max(sc->hdr.height, 1)) * HZ_PN_TPB * 4;
    const unsigned grid = (unsigned)blocks;
    int mode = g_panorama_traversal.load(std::memory_order_relaxed);
    if (mode < 0) mode = HZ_PN_TRAVERSAL_DEFAULT;
    if (a.point) return mode == 0 ? pn_launch2<true, 0>(p, grid, lds, st) : pn_launch2<true, 1>(p, grid, lds, st);
    return mode == 0 ? pn_launch2<false, 0>(p, grid, lds, st) : pn_launch2<false, 1>(p, grid, lds, st);
}

}  // namespace hz
